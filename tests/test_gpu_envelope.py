"""GPU tests of envelope_follower (csrc/envelope.hip): parity of E, grad x and the control gradient with the float64 restatement
(tests/envelope_restated.py) on the cases of tests/control_rate_cases.py, exact identities, the closed form of a constant level,
bit-for-bit reproducibility, where non-finite input reaches, views, the C ABI inside guard words, the autograd and call-state
contracts, dtypes and the empty signal.

Parity bounds, the house rule of the fused effects: the yardstick is the restatement in the kernel's arithmetic (float32 block sums
with weights from float64, float64 frame scans) on the same inputs, e32 = its error against the float64 sample loop relative to the peak
of the float64 result, per item; the kernel gets 4 x e32 and never less than 2e-6 of the peak for E and grad x and 1e-5 for the control
gradient. No bound exceeds ten floors (tests/test_envelope_cpu.py holds the restatement alone to that). The op has no atomics: wherever
two results are compared, every quantity is compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import control_rate_cases as K
from tests import envelope_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES, FLOOR = R.NAMES, R.FLOOR
T = K.TILE


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    assert lib().dasp_envelope_tile() == T
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def run_t(D, a, sr, hop=64, det="peak", need_gx=True, need_gs=True):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    sm = a["smoothing_ms"].to(DEV).requires_grad_(need_gs)
    E = D.envelope_follower(x, sr, sm, hop=hop, detector=det)
    leaves = ([x] if need_gx else []) + ([sm] if need_gs else [])
    grads = torch.autograd.grad((E * a["w"].to(DEV)).sum(), leaves)
    torch.cuda.synchronize()
    return dict(zip(("E",) + (("gx",) if need_gx else ()) + (("gsm",) if need_gs else ()), (E.detach(),) + grads))


def plain(B, C, N, hop=64, seed=0, lo=0.5, hi=200.0):
    g = torch.Generator().manual_seed(131 * seed + 7 * B + 3 * C + N)
    env = torch.exp(0.8 * torch.randn(B, 1, (N + 255) // 256, generator=g)).repeat_interleave(256, -1)[..., :N]
    return dict(x=0.3 * torch.randn(B, C, N, generator=g) * env, w=0.5 + 0.5 * torch.randn(B, R.control_frames(N, hop), generator=g),
                smoothing_ms=torch.exp(torch.rand(B, generator=g) * (np.log(hi) - np.log(lo)) + np.log(lo)))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", K.ENVELOPE_CONFIGS, ids=lambda c: "sr%d-hop%d-C%d-%s" % c[:4])
def test_parity_with_the_float64_restatement(D, cfg):
    sr, hop, chs, det, sm, seed = cfg
    worst = {k: (0.0, 0.0, 0.0, 0) for k in NAMES}                        # share of the bound, error, e32, length
    fails = []
    for n, b, want, f32 in K.envelope_calls(cfg):
        got = {k: v.cpu().numpy() for k, v in run_t(D, b, sr, hop, det).items()}
        for k, (e32, bound) in K.bounds(want, f32, FLOOR).items():
            assert got[k].shape == want[k].shape and bound <= 10 * FLOOR[k], (cfg, n, k, e32)
            e = K.per_item_err(got[k], want[k])
            if e / bound >= worst[k][0]:
                worst[k] = (e / bound, e, e32, n)
            if not e <= bound:
                fails.append((n, k, e, e32))
    record("envelope_parity sr=%d hop=%d C=%d %s" % cfg[:4], **{k: worst[k][1] for k in NAMES}, **{"fp32_" + k: worst[k][2] for k in NAMES},
           **{"share_" + k: worst[k][0] for k in NAMES}, **{"n_" + k: worst[k][3] for k in NAMES})
    assert not fails, (cfg, fails)


# ---- 2. exact identities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", R.DETECTORS)
def test_silence_gives_zero_and_no_gradient(D, det):
    a = plain(2, 2, T + 70)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100, 64, det)
    assert not got["E"].any() and not got["gx"].any() and not got["gsm"].any()
    assert all(torch.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_scaling_by_two_is_exact(D, hop):
    a = plain(3, 2, T + 70, hop)
    b = dict(a, x=2 * a["x"])
    for det, s in (("peak", 2.0), ("power", 4.0)):
        one, two = run_t(D, a, 44100, hop, det), run_t(D, b, 44100, hop, det)
        assert torch.equal(two["E"], s * one["E"]) and one["E"].any(), det


def test_a_silent_second_channel_leaves_peak_unchanged(D):
    a = plain(3, 1, T + 70)
    b = dict(a, x=torch.cat([a["x"], torch.zeros_like(a["x"])], 1))
    one, two = run_t(D, a, 44100), run_t(D, b, 44100)
    assert torch.equal(one["E"], two["E"]) and torch.equal(one["gsm"], two["gsm"])
    assert torch.equal(one["gx"][:, 0], two["gx"][:, 0]) and not two["gx"][:, 1].any()


def test_two_equal_channels_send_the_peak_gradient_to_channel_zero(D):
    a = plain(3, 1, T + 70)
    b = dict(a, x=torch.cat([a["x"], a["x"]], 1))
    one, two = run_t(D, a, 44100), run_t(D, b, 44100)
    assert torch.equal(one["E"], two["E"])
    assert torch.equal(one["gx"][:, 0], two["gx"][:, 0]) and not two["gx"][:, 1].any() and two["gx"][:, 0].any()


def test_clamped_smoothing_has_exactly_zero_gradient(D):
    a = plain(6, 2, T + 70)
    a["smoothing_ms"] = torch.tensor([0.01, 20000.0, 0.1, 10000.0, 5.0, 50.0])
    got = run_t(D, a, 44100)
    b = dict(a, smoothing_ms=a["smoothing_ms"].clamp(0.1, 10000.0))
    want = run_t(D, b, 44100)
    gs = got["gsm"].cpu().numpy()
    assert gs[0] == 0 and gs[1] == 0 and all(gs[q] != 0 for q in (2, 3, 4, 5))          # exactly zero where clamped - and only there
    for k in NAMES:
        assert torch.equal(got[k][2:], want[k][2:]), k
    for k in ("E", "gx"):                                # the clamp is to 0.1 and 10000 in float64, the float32 0.1 of `want` lies beside it
        assert K.per_item_err(got[k][:2].cpu().numpy(), want[k][:2].cpu().numpy()) <= FLOOR[k], k


# ---- 3. a constant level: the closed form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop,ms", [(8000, 8, 0.3), (44100, 64, 5.0), (192000, 2048, 50.0), (44100, 64, 2000.0)])
def test_constant_level_follows_the_closed_form(D, sr, hop, ms):
    """|x| = c gives e[m] = c (1 - a^(m + 1)), so E_j = c (1 - a^(j hop + 1)) while j hop < N: within the floor of the peak."""
    N, c = 2 * T + 5, 0.37
    x = (c * (-1.0) ** torch.arange(N)).expand(1, 2, N).contiguous()
    a = dict(x=x, w=torch.ones(1, R.control_frames(N, hop)), smoothing_ms=torch.tensor([ms]))
    E = run_t(D, a, sr, hop)["E"][0].cpu().double().numpy()
    lna = -R.LN9 / (sr * float(np.float32(ms)) / 1000.0)
    j = np.arange((N - 1) // hop + 1)
    want = -c * np.expm1((j * hop + 1) * lna)
    assert np.abs(E[:len(j)] - want).max() <= FLOOR["E"] * want.max()
    E2 = run_t(D, a, sr, hop, "power")["E"][0].cpu().double().numpy()
    assert np.abs(E2[:len(j)] - c * want).max() <= FLOOR["E"] * c * want.max()


# ---- 4. reproducibility: everything bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,det", [(8, "power"), (64, "peak"), (2048, "peak")])
def test_runs_are_bit_identical(D, hop, det):
    a = plain(5, 2, 2 * T + 5, hop)
    p, q = run_t(D, a, 44100, hop, det), run_t(D, a, 44100, hop, det)
    for k in NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, hop, det, need_gx=False)      # x needs no gradient: the elementwise pass is skipped, nothing else changes
    s = run_t(D, a, 44100, hop, det, need_gs=False)      # the control needs none: no tangent is formed
    assert torch.equal(p["E"], r["E"]) and torch.equal(p["gsm"], r["gsm"]) and torch.equal(p["E"], s["E"]) and torch.equal(p["gx"], s["gx"])
    with torch.no_grad():
        E = D.envelope_follower(a["x"].to(DEV), 44100, a["smoothing_ms"].to(DEV), hop=hop, detector=det)
    assert torch.equal(E, p["E"])


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_item_alone_and_inside_a_batch(D, hop):
    a = plain(3, 2, 2 * T + 5, hop)
    whole = run_t(D, a, 44100, hop)
    for b in (0, 2):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, hop)
        for k in NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation and no memset in the call path."""
    sr = 44100
    a = plain(4, 2, 2 * T + 5)
    eager = run_t(D, a, sr)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    sm = a["smoothing_ms"].to(DEV).requires_grad_(True)

    def step():
        E = D.envelope_follower(xt, sr, sm)
        return (E,) + torch.autograd.grad((E * wt).sum(), [xt, sm])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in range(3):
        for o in outs:
            o.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, o in zip(NAMES, outs):
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 5. off the nominal domain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", R.DETECTORS)
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_poisoned_sample_reaches_the_later_frame_points_of_its_item_only(D, value, det):
    hop, N = 64, 2 * T + 5
    a = plain(3, 2, N, lo=0.1, hi=50.0)
    clean = run_t(D, a, 44100, hop, det)
    for m0 in (0, 1, hop, T + 1, N - 1):
        b = {k: v.clone() for k, v in a.items()}
        b["x"][1, 1, m0] = value
        dirty = run_t(D, b, 44100, hop, det)
        for k in NAMES:
            assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), (m0, k)
        hit = (torch.arange(clean["E"].shape[1]) * hop >= m0).to(DEV)
        assert not torch.isfinite(dirty["E"][1][hit]).any() and torch.equal(dirty["E"][1][~hit], clean["E"][1][~hit]), m0
        assert not torch.isfinite(dirty["gsm"][1])
        keep = torch.ones(N, dtype=torch.bool, device=DEV)
        keep[m0] = False                                                    # grad x does not depend on E: it changes at the sample itself alone
        assert torch.equal(dirty["gx"][1][:, keep], clean["gx"][1][:, keep])


def test_nan_smoothing_and_upstream_gradients_stay_in_their_item(D):
    a = plain(3, 2, 2 * T + 5)
    clean = run_t(D, a, 44100)
    b = {k: v.clone() for k, v in a.items()}
    b["smoothing_ms"][1] = float("nan")
    dirty = run_t(D, b, 44100)
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
        assert torch.isnan(dirty[k][1]).all(), k
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, 40] = float("nan")
    dirty = run_t(D, b, 44100)
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
    assert torch.equal(clean["E"], dirty["E"]) and torch.isnan(dirty["gsm"][1])
    gx = dirty["gx"][1]
    assert torch.isnan(gx[:, :40 * 64 + 1]).all() and torch.equal(gx[:, 40 * 64 + 1:], clean["gx"][1][:, 40 * 64 + 1:])      # Lambda runs backwards


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * T + 5
    a = plain(3, 2, N)
    want = run_t(D, a, 44100)
    x = a["x"].to(DEV)
    if view == "offset":
        xv = torch.cat([torch.zeros(5, device=DEV), x.reshape(-1)])[5:].view(3, 2, N)
    elif view == "strided":
        xv = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not xv.is_contiguous()
    else:
        xv = torch.cat([x, torch.ones(3, 2, 40, device=DEV)], -1)[..., :N]
        assert not xv.is_contiguous()
    assert torch.equal(xv, x)
    xv.requires_grad_(True)
    sm = torch.stack([a["smoothing_ms"], a["smoothing_ms"]], -1).to(DEV)[:, 1].requires_grad_(True)          # a strided control
    E = D.envelope_follower(xv, 44100, sm)
    grads = torch.autograd.grad((E * a["w"].to(DEV)[:, ::1]).sum(), [xv, sm])
    for k, g in zip(NAMES, (E,) + grads):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_ignores_dirty_scratch_and_refuses_before_it_launches(D):
    """Through the C ABI: every output and both scratch buffers written inside NaN-filled guard words leave the guards NaN, a NaN-filled
    scratch gives the same bits as a zero-filled one, the optional outputs change nothing else, and a refused call writes nothing."""
    from dasp_pytorch_amd._lib import ptr, stream
    sr, G = 44100.0, 64
    B, C, N = 3, 2, 2 * T + 5
    Lb = lib()
    for hop in (8, 2048):
        F = R.control_frames(N, hop)
        a = plain(B, C, N, hop)
        x, gE, sm = a["x"].to(DEV), a["w"].to(DEV), a["smoothing_ms"].to(DEV)
        nscr = Lb.dasp_envelope_scratch_floats(B, N, hop)
        assert nscr == 2 * B * F

        def guarded(n, fill=float("nan")):
            buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
            buf[G:G + n] = fill
            return buf, buf[G:G + n]

        def run(fill, tangent=True, want_gx=True, hop=hop, expect=0):
            bufs = {k: guarded(n) for k, n in (("E", B * F), ("D", B * F), ("gx", B * C * N), ("gs", B))}
            bufs["scr_f"], bufs["scr_b"] = guarded(nscr, fill), guarded(nscr, fill)
            rc = Lb.dasp_envelope_forward(ptr(x), ptr(sm), ptr(bufs["E"][1]), ptr(bufs["D"][1] if tangent else None), ptr(bufs["scr_f"][1]), B, C, N, hop, 0,
                                          sr, stream())
            assert rc == expect
            rc = Lb.dasp_envelope_backward(ptr(x), ptr(sm), ptr(bufs["D"][1] if tangent else None), ptr(gE), ptr(bufs["gx"][1] if want_gx else None),
                                           ptr(bufs["gs"][1] if tangent else None), ptr(bufs["scr_b"][1]), B, C, N, hop, 0, sr, stream())
            assert rc == expect
            torch.cuda.synchronize()
            for k, (buf, inner) in bufs.items():
                assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
            return {k: inner.clone() for k, (buf, inner) in bufs.items()}

        zero, dirty = run(0.0), run(float("nan"))
        for k in ("E", "D", "gx", "gs"):
            assert torch.equal(zero[k].view(torch.int32), dirty[k].view(torch.int32)), k
        no_tan, no_gx = run(float("nan"), tangent=False), run(float("nan"), want_gx=False)
        assert torch.equal(zero["E"], no_tan["E"]) and torch.equal(zero["gx"], no_tan["gx"]) and torch.isnan(no_tan["D"]).all() and torch.isnan(no_tan["gs"]).all()
        assert torch.equal(zero["E"], no_gx["E"]) and torch.equal(zero["gs"], no_gx["gs"]) and torch.isnan(no_gx["gx"]).all()
        assert torch.isnan(no_gx["scr_b"]).all()                             # the backward scratch is Lambda, for grad x alone
        ref = run_t(D, a, sr, hop)
        assert torch.equal(zero["E"].view(B, F), ref["E"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"]) and torch.equal(zero["gs"], ref["gsm"])
        refused = run(float("nan"), hop=24, expect=-2)                        # nothing launched: every word is still NaN
        assert all(torch.isnan(v).all() for v in refused.values())
    assert lib().dasp_device_error() == 0


# ---- 6. what the forward pass leaves behind -------------------------------------------------------------------------------------------------
def test_forward_saves_nothing_per_sample(D):
    B, C, N, hop = 3, 2, 2 * T + 5, 64
    a = plain(B, C, N)
    x = a["x"].to(DEV).requires_grad_(True)
    sm = a["smoothing_ms"].to(DEV).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.envelope_follower(x, 44100, sm)
    assert any(t.data_ptr() == x.data_ptr() for t in saved)                   # x itself, not a copy
    assert sorted(t.numel() for t in saved) == sorted([B * C * N, B, B * R.control_frames(N, hop)])
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.envelope_follower(x, 44100, sm.detach())
    assert sorted(t.numel() for t in saved) == sorted([B * C * N, B])          # no tangent without a control gradient
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.envelope_follower(x.detach(), 44100, sm.detach())
    assert not saved


# ---- 7. the autograd and call-state contracts -----------------------------------------------------------------------------------------------
def _spec():
    """The op's entry for the contract batteries, in the form of the entries of tests/autograd_contract_cases.py (that table is closed:
    tests/test_call_state_cpu.py pins its size). What is watched is EnvelopeFollowerKernels, the class that holds the forward /
    backward pair that EnvelopeFollowerFunction binds to autograd."""
    from dasp_pytorch_amd._ctypes_ops import EnvelopeFollowerKernels
    from tests import autograd_contract_cases as A
    sr, hop, N = 8000, 64, 1501
    F = R.control_frames(N, hop)

    def arrays(seed):
        g = A.gen(seed, 173)
        return dict(x=0.5 * torch.randn(3, 2, N, generator=g), smoothing_ms=torch.rand(3, generator=g) * 45.0 + 5.0)

    def call(t):
        import dasp_pytorch_amd
        return dasp_pytorch_amd.envelope_follower(t["x"], sr, t["smoothing_ms"], hop=hop)

    names = dict(E="y0", gx="g_x", gsm="g_smoothing_ms")

    def ref(a, gys):
        w = torch.from_numpy(gys[0])
        r64 = R.forward_backward(a["x"], sr, a["smoothing_ms"], w, hop)
        r32 = R.forward_backward(a["x"], sr, a["smoothing_ms"], w, hop, arith=torch.float32)
        bound = {names[k]: max(4.0 * peak_err(r32[k], r64[k]), FLOOR[k]) for k in names}
        return dict({names[k]: r64[k] for k in names}, _bound=bound)
    spec = A.measured_bound("envelope_follower", arrays, call, ("x", "smoothing_ms"), ("x",), ("EnvelopeFollowerKernels",), ref,
                            {names[k]: FLOOR[k] for k in names}, forms={"smoothing_ms": "vector"}, lowp=("x",), outs=lambda a: [(3, F)],
                            cite="tests/test_gpu_envelope.py test_parity_with_the_float64_restatement")
    spec.functions = lambda: [EnvelopeFollowerKernels]
    return spec


def _contract(checks, check):
    spec, rec = _spec(), []
    try:
        find = checks[check](spec, rec)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in envelope_follower {check}: {e}", returncode=3)        # nothing more runs on a device that has faulted
        raise
    torch.cuda.synchronize()
    assert lib().dasp_device_error() == 0
    assert not find, "\n".join(find)


@pytest.mark.parametrize("check", ["C1_subsets", "C2_repeat", "C3_interleave", "C4_upstream_forms", "C5_leaf_forms", "C6_mutation", "C7_streams"])
def test_autograd_contract(D, check):
    from tests import autograd_contract_checks as C
    _contract(C.CHECKS, check)


@pytest.mark.parametrize("check", ["S1_arguments", "S4_memory"])
def test_call_state(D, check):
    from tests import call_state_checks as S
    _contract(S.CHECKS, check)


def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    E = D.envelope_follower(x, 44100, a["smoothing_ms"].to(DEV))
    (gx,) = torch.autograd.grad(E.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 E depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 8. dtypes and the empty signal ---------------------------------------------------------------------------------------------------------
def test_empty_input(D):
    for B, C, N, F in ((2, 2, 0, 1), (0, 2, 16, 3)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        sm = torch.ones(B, device=DEV, requires_grad=True)
        E = D.envelope_follower(x, 44100, sm, hop=8)
        assert E.shape == (B, F) and not E.any()
        E.sum().backward()
        assert x.grad.shape == x.shape and sm.grad.shape == sm.shape and not sm.grad.any()


def test_half_and_bfloat16_are_converted_and_float64_is_refused(D):
    from dasp_pytorch_amd import _lib
    a = plain(2, 2, 3000)
    sm = a["smoothing_ms"].to(DEV)
    for dt in (torch.float16, torch.bfloat16):
        xl = a["x"].to(DEV).to(dt)
        with torch.no_grad():
            E = D.envelope_follower(xl, 44100, sm)
            want = D.envelope_follower(xl.float(), 44100, sm).to(dt)
        assert E.dtype == dt and torch.equal(E, want)
    with pytest.raises(_lib.DaspHipError, match="envelope_follower: float64"):
        D.envelope_follower(a["x"].to(DEV).double(), 44100, sm)
