"""What tests/test_gpu_input_domain.py leans on, checked without a GPU: the oracle reproduces the reference-made goldens of
tests/golden/make_golden_input_domain.py (other sample rates, silence) at the bounds of tests/test_oracle_cpu.py; the exact-recursion
references of tests/input_domain_cases.py agree with the oracle where the oracle's circular filters are alias-free, and the expander's
analytic adjoint with central differences of orc.expander; every part-C input keeps the references finite; the wrap term of every dynamics
case compared with the circular-filter oracle is below 1e-8; every EQ cutoff of part D is below Nyquist; and the float32 run of the oracle
at the 20 Hz corner is measured: it was meant as a fallback bound for part D on the condition that it stays below 1e-3, it does not
(1e-4 .. 1e-2), so part D holds the kernels to the existing bounds alone and only records it."""
import numpy as np
import pytest

from oracle import dasp_oracle as orc
from tests import input_domain_cases as idc
from tests.util import linf_peak, load_golden


@pytest.mark.parametrize("name", ["comp_sr48000_b2c1_n6000", "comp_sr96000_b2c1_n6000", "comp_silence_b2c2_n6000"])
def test_oracle_compressor_matches_reference_at_other_rates_and_on_silence(name):
    """Bounds of tests/test_oracle_cpu.py::test_oracle_compressor_matches_reference (:141-148)."""
    g = load_golden(name)
    sr = int(g["sample_rate"])
    p = g["params"].astype(np.float64)
    cols = [p[:, i] for i in range(6)]
    assert idc.dyn_wrap(g["x"].shape[-1], sr, p[:, 2]) < 1e-8
    y = orc.compressor(g["x"], sr, *cols)
    gx, gc = orc.compressor_vjp(g["x"], sr, *cols, g["w"])
    assert np.isfinite(y).all() and np.isfinite(gx).all()
    assert linf_peak(y, g["y64"]).max() < 2e-6
    assert linf_peak(gx, g["gx64"]).max() < 5e-6
    for j, k in enumerate(idc.DYN_KEYS):
        ref = g["gp64"][:, j]
        assert np.abs(gc[k] - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1e-30), (k, gc[k], ref)
    assert np.all(g["gp64"][:, 3] == 0)
    y32 = orc.compressor(g["x"], sr, *[c.astype(np.float32) for c in cols], dtype=np.float32)
    assert linf_peak(y32, g["y32"]).max() < 1e-4
    if "silence" in name:
        # what the golden pins: the cancelling pair's side chain is exactly zero, the reference passes no gradient through the clamp below
        # eps and sign(0) = 0, so grad x there is gy * gain alone; the zero tail comes out as exact zeros
        assert np.all(g["x"][0].sum(0) == 0) and np.all(g["x"][1, :, 1500:] == 0)
        assert np.all(g["y64"][1, :, 1500:] == 0)
        lin0 = 10 ** (p[0, 5] / 20)
        assert np.abs(g["y64"][0] - g["x"][0] * lin0).max() < 1e-6 * np.abs(g["x"][0]).max()
        assert np.abs(g["gx64"][0] - g["w"][0] * lin0).max() < 1e-6 * np.abs(g["w"][0]).max()
        # the padded reference and the exact recursion give the same numbers on this input
        yz, gxz, gpz = idc.compressor_ref(g["x"], sr, p, g["w"])
        ye, gxe, gpe = idc.dynamics_exact(0, g["x"], sr, p, g["w"])
        assert linf_peak(yz, g["y64"]).max() < 2e-6 and linf_peak(ye, g["y64"]).max() < 2e-6
        assert linf_peak(gxz, g["gx64"]).max() < 5e-6 and linf_peak(gxe, g["gx64"]).max() < 5e-6


@pytest.mark.parametrize("sr", idc.RATES)
def test_oracle_biquad_matches_reference_at_every_rate(sr):
    """Bounds of tests/test_oracle_cpu.py::test_oracle_biquad_matches_reference_all_types (:274-276); the float64 coefficients are stored as
    float64 here, so the comparison is to 1e-12."""
    g = load_golden("biquad_rates_b6")
    assert tuple(g["rates"]) == idc.RATES
    ins = [g[k].astype(np.float64)[:, 0] for k in ("gain_db", "cutoff_freq", "q_factor")]
    assert ins[1].max() < 0.45 * min(idc.RATES)
    for t in idc.BIQUAD_TYPES:
        b, a = orc.biquad(*ins, sr, t)
        assert np.abs(b - g[f"sr{sr}_{t}_b64"]).max() < 1e-12 * np.abs(b).max() and np.abs(a - g[f"sr{sr}_{t}_a64"]).max() < 2e-12, t
        # complex-step Jacobian of the design (orc.biquad takes complex input), not orc.biquad_vjp: its central differences carry
        # 1e-10 of absolute noise, which is 1e-5 of a low-pass row whose largest gradient is 7e-6 at 88.2 kHz
        gp = np.zeros((ins[0].shape[0], 3))
        for d in range(3):
            mod = [v.astype(np.complex128) for v in ins]
            mod[d] = mod[d] + 1e-30j
            bc, ac = orc.biquad(*mod, sr, t)
            gp[:, d] = (np.sum(bc.imag * g["wb"], 1) + np.sum(ac.imag * g["wa"], 1)) / 1e-30
        assert linf_peak(gp, g[f"sr{sr}_{t}_g64"]).max() < 5e-6, t


def test_exact_recursions_agree_with_the_oracle_where_it_is_alias_free():
    """sos_exact / peq_exact / lfilter_exact / dynamics_exact(0) against the oracle's (circular) functions on signals long enough for
    every impulse response to have decayed inside the transform."""
    rng = np.random.default_rng(1)
    B, C, N = 2, 2, 20000
    a, gy = idc.make(idc.BY_NAME["sosfilt_s3"], 3, B, C, N, 44100)
    y, gx, gsos = idc.sos_exact(a["sos"], a["x"], gy)
    gso, gxo = orc.sosfilt_via_fsm_vjp(a["sos"], a["x"], gy)
    assert linf_peak(y, orc.sosfilt_via_fsm(a["sos"], a["x"])).max() < 1e-9
    assert linf_peak(gx, gxo).max() < 1e-9 and linf_peak(gsos, gso).max() < 1e-8
    p = idc.peq_params(rng, B, 44100).astype(np.float64)
    p[:, 1] = 200.0; p[:, 2] = 1.0                                  # a low shelf that has decayed by 20000 samples
    x = idc.noise_x(rng, (B, C, N))
    y, gx, gp = idc.peq_exact(x, 44100, p, gy)
    gxo, gpo = orc.parametric_eq_vjp(x, 44100, p, gy)
    assert linf_peak(y, orc.parametric_eq(x, 44100, p)).max() < 1e-9
    assert linf_peak(gx, gxo).max() < 1e-9 and linf_peak(gp, gpo).max() < 1e-7
    ps = p[:1]                                                      # one parameter row shared by the batch: the gradients sum over items
    _, _, gp1 = idc.peq_exact(x, 44100, ps, gy)
    assert gp1.shape == (1, 18) and linf_peak(gp1, orc.parametric_eq_vjp(x, 44100, ps, gy)[1]).max() < 1e-7
    for K in (2, 11):
        a, gy1 = idc.make(idc.BY_NAME[f"lfilter_k{K}"], 4 + K, B, 1, N, 44100)
        y, gx, gb, ga = idc.lfilter_exact(a["x"], a["b"], a["a"], gy1)
        gxo, gbo, gao = orc.lfilter_via_fsm_vjp(a["x"], a["b"], a["a"], gy1)
        assert linf_peak(y, orc.lfilter_via_fsm(a["x"], a["b"], a["a"])).max() < 1e-9, K
        assert linf_peak(gx, gxo).max() < 1e-9 and linf_peak(gb, gbo).max() < 1e-8 and linf_peak(ga, gao).max() < 1e-8, K
    for look in (0, 3):
        x = idc.speechlike(rng, B, C, N)
        pd = idc.dyn_params(rng, B).astype(np.float64)
        pd[:, 2] = np.minimum(pd[:, 2], 20.0)
        assert idc.dyn_wrap(N, 44100, pd[:, 2]) < 1e-8
        y, gx, gp = idc.dynamics_exact(0, x, 44100, pd, gy, look)
        cols = [pd[:, i] for i in range(6)]
        gxo, gco = orc.compressor_vjp(x, 44100, *cols, gy, lookahead_samples=look)
        assert linf_peak(y, orc.compressor(x, 44100, *cols, lookahead_samples=look)).max() < 1e-7
        assert linf_peak(gx, gxo).max() < 1e-6
        for j, k in enumerate(idc.DYN_KEYS):
            assert np.abs(gp[:, j] - gco[k]).max() <= 1e-6 * max(np.abs(gco[k]).max(), 1e-30), (k, gp[:, j], gco[k])
        yz, gxz, gpz = idc.compressor_ref(x, 44100, pd, gy, look)      # zero padding changes nothing
        assert linf_peak(yz, y).max() < 1e-7 and linf_peak(gxz, gx).max() < 1e-6 and np.abs(gpz - gp).max() <= 1e-6 * np.abs(gp).max()


def test_expander_adjoint_against_central_differences():
    """dynamics_exact(1): forward = orc.expander, control gradients against central differences of it, grad x by a directional derivative
    on a signal whose side chain stays away from zero (the method of tests/test_gpu_dynamics.py::test_expander_design_model_and_gradcheck)."""
    rng = np.random.default_rng(5)
    B, C, N, sr = 2, 2, 6000, 48000
    p = np.array([[-35.0, 2.0, 12.0, 50.0, 6.0, 2.0], [-20.0, 3.5, 40.0, 50.0, 10.0, 0.0]])
    f = lambda xx, pp: orc.expander(xx, sr, *[pp[:, i] for i in range(6)])
    sign = rng.choice([-1.0, 1.0], size=(B, 1, N))
    x = sign * (0.02 + 0.3 * rng.random((B, C, N))) * 10 ** (-rng.random((B, 1, 1)) * 1.5)
    w = rng.standard_normal((B, C, N))
    y, gx, gp = idc.dynamics_exact(1, x, sr, p, w)
    assert np.abs(y - f(x, p)).max() < 1e-12 * np.abs(y).max()
    for j in (0, 1, 2, 4, 5):
        h = 1e-5 * max(1.0, abs(p[0, j]))
        pp, pm = p.copy(), p.copy(); pp[:, j] += h; pm[:, j] -= h
        fd = ((f(x, pp) - f(x, pm)) * w).sum((1, 2)) / (2 * h)
        assert np.abs(gp[:, j] - fd).max() <= 2e-4 * np.abs(fd).max(), (idc.DYN_KEYS[j], gp[:, j], fd)
    assert np.all(gp[:, 3] == 0)
    v = rng.standard_normal(x.shape)
    h = 1e-7
    fd = ((f(x + h * v, p) - f(x - h * v, p)) * w).sum() / (2 * h)
    assert abs((gx * v).sum() - fd) < 1e-4 * abs(fd), ((gx * v).sum(), fd)


@pytest.mark.parametrize("kind", idc.SILENCE_KINDS)
def test_silence_builders_keep_the_references_finite(kind):
    """Every input of part C through every reference of the table, at 16, 44.1 and 96 kHz: finite outputs and gradients."""
    for case in idc.CASES:
        if case.name == "reverb_seed" or (kind == "cancel" and case.name not in ("compressor", "expander", "stereo_widener", "chain_forward_saving",
                                                                             "chain_forward_expander", "chain_forward_saving_expander")):
            continue
        for sr in (16000, 44100, 96000):
            if sr < case.min_rate or (case.rate_free and sr != 44100):
                continue
            kw = dict(L=300, taps=63) if case.shapes else {}
            a, gy = idc.make(case, 11, 2, 2, 2048, sr, **kw)
            a["x"] = idc.silence(kind, a["x"], head=500)
            ref = case.ref(sr, a, gy.astype(np.float64), **kw)
            for k, v in ref.items():
                assert np.isfinite(v).all(), (case.name, sr, k)
            if kind == "zeros" and case.name.startswith(("reverb", "compressor", "expander", "parametric_eq", "gain")):
                assert np.all(ref["y"] == 0), case.name


def test_dynamics_cases_have_a_negligible_wrap_term():
    """Every dynamics case that goes through orc.compressor / orc.compressor_vjp (a circular filter) is zero-padded by compressor_ref to a
    length whose wrap term alpha^(n_fft - T) is below 1e-8 - at every rate, for the slowest attack the module allows."""
    for sr in idc.RATES + (44100,):
        for N in (1028, 6000, 8200, 40000):
            T = idc.dyn_pad_len(N, sr, np.array([100.0]))
            assert T >= N and idc.dyn_wrap(T, sr, np.array([100.0])) < 1e-8, (sr, N, T)
            assert T <= 1 << 18                                    # and stays cheap
    assert idc.dyn_wrap(6000, 96000, np.array([100.0])) > 0.05     # unpadded, the short shape at 96 kHz would be 9 % off


@pytest.mark.parametrize("sr", idc.RATES)
def test_eq_rate_cases_are_below_nyquist_and_the_float32_oracle_error_is_recorded_not_used(sr):
    rng = np.random.default_rng(sr)
    for _ in range(4):
        p = idc.eq_rate_params(rng, 3, sr)
        assert (p[:, 1::3] <= 0.45 * sr + 1e-3).all() and (p[:, 1::3] > 0).all()
        assert p[0, 1] == 20.0 and p[0, 2] == 6.0 and p[0, 0] == 20.0 and p[1, 0] == -20.0
    lo, span = idc.chain_tables(sr)
    assert all(l + s <= 0.45 * sr + 1e-3 for l, s in list(zip(lo, span))[1::3])
    # pole radius of the 20 Hz / Q 6 peaking corner: 0.99976 at 44.1 kHz and 0.99989 at 96 kHz with 0 dB, 0.999925 / 0.999966 at +20 dB
    radius = lambda fs, gain: float(np.sqrt(orc.biquad(np.array([gain]), np.array([20.0]), np.array([6.0]), fs, "peaking")[1][0, 2]))
    assert abs(radius(44100, 0.0) - 0.99976) < 1e-5 and abs(radius(96000, 20.0) - 0.999966) < 1e-6
    assert 0.99 < radius(sr, -20.0) < radius(sr, 20.0) < 1.0
    for N in (8200, 40000):
        rng = np.random.default_rng(N + sr)
        x = idc.noise_x(rng, (2, 1, N))
        e = idc.eq_f32_error(x, sr, idc.eq_rate_params(rng, 2, sr))
        print(f"float32 oracle against float64 oracle, {sr} Hz, N = {N}: {e}")
        # The float32 run of the reference's algorithm is NOT a usable yardstick at this corner: 1 - a2 is 7e-5 there, float32 coefficients
        # move the pole's damping by 1e-3, and the measured error is 1e-4 .. 1e-2 (3e-2 for single draws), erratic from rate to rate. Twice
        # that would excuse a broken kernel, so part D does not fall back on it: the kernels are held to the existing bounds at every rate.
        assert np.isfinite(e).all() and e.max() < 0.1, (sr, N, e)


def test_expander_behind_a_float32_eq_is_probed_before_it_is_compared():
    """The two expander chain cases (idc._ref_chain_expander): on the table's uniform noise the EQ's output passes close to zero, where the
    expander's gain follows 20 log10 |s| with the slope (ratio - 1) x 8.7 / |s|. Moving the EQ's output by EQ_PROBE = 3e-7 of its peak
    (the fused pass's EQ is measured at <= 5.4e-7, its bound is 1e-5) moves the float64 reference itself far beyond the bounds, so those
    quantities are handed back under "_<name>" and not compared; exact silence and levels below eps move nothing and are compared."""
    case = idc.BY_NAME["chain_forward_saving_expander"]
    sr, (B, C, N) = 22050, idc.PLAIN_SHAPES[0]
    a, gy = idc.make(case, sr + N, B, C, N, sr)
    a["ctl"][:, 2] = idc.dyn_rate_params(np.random.default_rng(sr + N), B, sr)[:, 2]        # the draw of part D at this rate
    gy = gy.astype(np.float64)
    p, comp, span = idc._chain_physical(sr, a)
    y, gx, gp, gc, y1 = idc.chain_grad_exact(1, a["x"], sr, p, comp, gy)
    d = (np.random.default_rng(12345).random(y1.shape) * 2 - 1) * idc.EQ_PROBE * np.abs(y1).reshape(B, -1).max(1)[:, None, None]
    yp, gxp, gpp, gcp, _ = idc.chain_grad_exact(1, a["x"], sr, p, comp, gy, dy1=d)
    moved = dict(y=linf_peak(yp, y).max(), g_x=linf_peak(gxp, gx).max(), g_eq_pn=np.abs(gpp - gp).max() / np.abs(gp).max(),
                 g_ctl=(np.abs(gcp - gc).max(0) / np.maximum(np.abs(gc).max(0), 1e-300)).max())
    print("expander behind the EQ, 22050 Hz (2,2,1028): a 3e-7 probe of the EQ output moves the float64 reference by " +
          ", ".join(f"{k} {v:.1e} ({v / idc.CHAIN_EXP_TOL[k][1]:.0f} bounds)" for k, v in moved.items()) +
          f"; smallest |s| / peak {np.abs(y1.sum(1)).min() / np.abs(y1).max():.1e}")
    assert moved["y"] > 10 * 2e-5 and moved["g_x"] > 10 * 5e-5
    # ... while the compressor on the same input, which leaves small |s| alone, moves by less than its bounds
    y0, gx0, _, _, _ = idc.chain_grad_exact(0, a["x"], sr, p, comp, gy)
    y0p, gx0p, _, _, _ = idc.chain_grad_exact(0, a["x"], sr, p, comp, gy, dy1=d)
    assert linf_peak(y0p, y0).max() < 2e-5 / 4 and linf_peak(gx0p, gx0).max() < 2e-5 / 4
    ref = case.ref(sr, a, gy)
    assert set(ref) == {"_y", "_g_x", "_g_eq_pn", "_g_ctl"} and all(np.isfinite(v).all() for v in ref.values())
    for kind in ("zeros", "amp_1e-9"):
        ref = case.ref(sr, dict(a, x=idc.silence(kind, a["x"])), gy)
        assert set(ref) == {"y", "g_x", "g_eq_pn", "g_ctl"}, (kind, sorted(ref))
