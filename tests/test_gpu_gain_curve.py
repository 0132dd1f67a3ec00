"""GPU tests of gain_curve (csrc/envelope.hip): parity of y, grad x and the frame gradients with the float64 restatement
(tests/gain_curve_restated.py) on the cases of tests/control_rate_cases.py, exact identities, agreement with `gain`, bit-for-bit
reproducibility, where a NaN frame value reaches, views, the C ABI inside guard words, the ducking composition with envelope_follower,
the autograd and call-state contracts, the module, dtypes and the empty signal.

Parity bounds, the house rule of the fused effects: e32 is the error of the restatement in float32 arithmetic against float64 relative
to the peak of the float64 result, per item; the kernel gets 4 x e32 and never less than 2e-6 of the peak for y and grad x and 1e-5 for
the frame gradients. No bound exceeds ten floors (tests/test_gain_curve_cpu.py holds the restatement alone to that). The op has no
atomics: wherever two results are compared, every quantity is compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import control_rate_cases as K
from tests import envelope_restated as ER
from tests import gain_curve_restated as R
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


def run_t(D, a, hop=64, need_gx=True, need_gp=True):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    P = a["gain_db"].to(DEV).requires_grad_(need_gp)
    y = D.gain_curve(x, 44100, P, hop=hop)
    leaves = ([x] if need_gx else []) + ([P] if need_gp else [])
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), leaves)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + (("ggain",) if need_gp else ()), (y.detach(),) + grads))


def plain(B, C, N, hop=64, seed=0):
    a = K.gain_curve_inputs(hop, C, N, seed)
    if B != K.BS:
        g = torch.Generator().manual_seed(977 * seed + B + N)
        a = dict(x=0.5 * torch.randn(B, C, N, generator=g), w=torch.randn(B, C, N, generator=g),
                 gain_db=torch.rand(B, R.control_frames(N, hop), generator=g) * 72.0 - 60.0)
    return a


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", K.GAIN_CURVE_CONFIGS, ids=lambda c: "hop%d-C%d" % c[:2])
def test_parity_with_the_float64_restatement(D, cfg):
    hop, chs, seed = cfg
    worst = {k: (0.0, 0.0, 0.0, 0) for k in NAMES}                        # share of the bound, error, e32, length
    fails = []
    for n, b, want, f32 in K.gain_curve_calls(cfg):
        got = {k: v.cpu().numpy() for k, v in run_t(D, b, hop).items()}
        for k, (e32, bound) in K.bounds(want, f32, FLOOR).items():
            assert got[k].shape == want[k].shape and bound <= 10 * FLOOR[k], (cfg, n, k, e32)
            e = K.per_item_err(got[k], want[k])
            if e / bound >= worst[k][0]:
                worst[k] = (e / bound, e, e32, n)
            if not e <= bound:
                fails.append((n, k, e, e32))
    record("gain_curve_parity hop=%d C=%d" % cfg[:2], **{k: worst[k][1] for k in NAMES}, **{"fp32_" + k: worst[k][2] for k in NAMES},
           **{"share_" + k: worst[k][0] for k in NAMES}, **{"n_" + k: worst[k][3] for k in NAMES})
    assert not fails, (cfg, fails)


# ---- 2. exact identities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_a_zero_curve_returns_x_bit_for_bit(D, hop):
    a = plain(3, 2, 2 * T + 5, hop)
    a["gain_db"] = torch.zeros_like(a["gain_db"])
    got = run_t(D, a, hop)
    assert torch.equal(got["y"].cpu(), a["x"]) and torch.equal(got["gx"].cpu(), a["w"])


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_the_last_frame_value_takes_nothing_when_the_last_sample_sits_on_a_frame_point(D, hop):
    """Frame point F - 1 lies at or after sample N. With N = k hop + 1 the last sample has t = 0, so the last frame value's gradient is
    exactly 0; with N = k hop the last interval runs up to t = (hop - 1) / hop and the last frame value - at sample N itself - takes its
    share, as the definition's interpolation says (tests/test_gain_curve_cpu.py shows the same on the restatement)."""
    for N, zero in ((T + hop + 1, True), (hop + 1, True), (T + hop, False)):
        g = run_t(D, plain(3, 2, N, hop), hop)["ggain"]
        assert bool((g[:, -1] == 0).all()) == zero, (N, g[:, -1])
        assert g[:, :-1].ne(0).all()


# ---- 3. a constant curve is `gain` -----------------------------------------------------------------------------------------------------------
def test_a_constant_curve_agrees_with_gain(D):
    hop, N = 64, 2 * T + 5
    a = plain(3, 2, N, hop)
    db = torch.tensor([-17.3, 0.7, 11.9])
    a["gain_db"] = db[:, None].expand(3, R.control_frames(N, hop)).contiguous()
    got = run_t(D, a, hop)
    x = a["x"].to(DEV).requires_grad_(True)
    gdb = db.to(DEV).requires_grad_(True)
    y = D.gain(x, 44100, gdb)
    gx, gg = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [x, gdb])
    assert K.per_item_err(got["y"].cpu().numpy(), y.detach().cpu().numpy()) <= FLOOR["y"]
    assert K.per_item_err(got["gx"].cpu().numpy(), gx.cpu().numpy()) <= FLOOR["gx"]
    # the frame gradients of a constant curve add up to the gradient of the one gain; sums in float64 on the host
    tot = got["ggain"].double().sum(1).cpu().numpy()
    assert np.abs(tot - gg.double().cpu().numpy()).max() <= FLOOR["ggain"] * np.abs(got["ggain"].double().cpu().numpy()).sum(1).max()


# ---- 4. reproducibility: everything bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_runs_are_bit_identical_and_an_item_alone_equals_the_item_in_a_batch(D, hop):
    a = plain(3, 2, 2 * T + 5, hop)
    p, q = run_t(D, a, hop), run_t(D, a, hop)
    for k in NAMES:
        assert torch.equal(p[k], q[k]), k
    r, s = run_t(D, a, hop, need_gx=False), run_t(D, a, hop, need_gp=False)
    assert torch.equal(p["ggain"], r["ggain"]) and torch.equal(p["gx"], s["gx"]) and torch.equal(p["y"], r["y"]) and torch.equal(p["y"], s["y"])
    for b in (0, 2):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, hop)
        for k in NAMES:
            assert torch.equal(p[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    a = plain(4, 2, 2 * T + 5)
    eager = run_t(D, a)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    P = a["gain_db"].to(DEV).requires_grad_(True)

    def step():
        y = D.gain_curve(xt, 44100, P)
        return (y,) + torch.autograd.grad((y * wt).sum(), [xt, P])

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
@pytest.mark.parametrize("hop,J", [(8, 0), (8, 3), (64, 64), (64, 65), (2048, 2), (64, 129)])
def test_a_nan_frame_value_reaches_its_two_intervals_of_its_item_only(D, hop, J):
    """Frame value J of item 1: samples (J - 1) hop < n < (J + 1) hop in y and grad x, frame points J - 1 .. J + 1 in the frame
    gradients; every other value of the item and the other items keep every bit. J on both sides of a tile boundary and at both ends."""
    N = 2 * T + 5
    a = plain(3, 2, N, hop)
    F = a["gain_db"].shape[1]
    J = min(J, F - 1)
    clean = run_t(D, a, hop)
    b = {k: v.clone() for k, v in a.items()}
    b["gain_db"][1, J] = float("nan")
    dirty = run_t(D, b, hop)
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
    n = torch.arange(N, device=DEV)
    hit = ((J - 1) * hop < n) & (n < (J + 1) * hop)
    for k in ("y", "gx"):
        assert torch.isnan(dirty[k][1][:, hit]).all() and torch.equal(dirty[k][1][:, ~hit], clean[k][1][:, ~hit]), k
    f = torch.arange(F, device=DEV)
    fhit = (f >= J - 1) & (f <= J + 1)
    assert torch.isnan(dirty["ggain"][1][fhit]).all() and torch.equal(dirty["ggain"][1][~fhit], clean["ggain"][1][~fhit])


def test_poisoned_audio_and_upstream_gradients_stay_at_their_samples(D):
    a = plain(3, 2, 2 * T + 5)
    clean = run_t(D, a)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, 0, 700] = float("nan")
    b["w"][1, 1, 4100] = float("inf")
    dirty = run_t(D, b)
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
    ok = torch.ones_like(clean["y"][1], dtype=torch.bool)
    ok[0, 700] = False
    assert torch.equal(dirty["y"][1][ok], clean["y"][1][ok]) and torch.isnan(dirty["y"][1, 0, 700])
    ok[0, 700], ok[1, 4100] = True, False
    assert torch.equal(dirty["gx"][1][ok], clean["gx"][1][ok]) and torch.isinf(dirty["gx"][1, 1, 4100])
    bad = torch.zeros(clean["ggain"].shape[1], dtype=torch.bool)
    bad[[700 // 64, 700 // 64 + 1, 4100 // 64, 4100 // 64 + 1]] = True
    assert not torch.isfinite(dirty["ggain"][1].cpu()[bad]).any() and torch.equal(dirty["ggain"][1].cpu()[~bad], clean["ggain"][1].cpu()[~bad])


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * T + 5
    a = plain(3, 2, N)
    want = run_t(D, a)
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
    P = torch.stack([a["gain_db"], a["gain_db"]], -1).to(DEV)[..., 1].requires_grad_(True)                  # a strided curve
    assert not P.is_contiguous()
    y = D.gain_curve(xv, 44100, P)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv, P])
    for k, g in zip(NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_ignores_dirty_scratch_and_refuses_before_it_launches(D):
    from dasp_pytorch_amd._lib import ptr, stream
    G = 64
    B, C, N = 3, 2, 2 * T + 5
    Lb = lib()
    for hop in (8, 2048):
        F = R.control_frames(N, hop)
        a = plain(B, C, N, hop)
        x, gy, P = a["x"].to(DEV), a["w"].to(DEV), a["gain_db"].to(DEV)
        nscr = Lb.dasp_gaincurve_scratch_floats(B, N, hop)
        assert nscr == 2 * B * F

        def guarded(n, fill=float("nan")):
            buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
            buf[G:G + n] = fill
            return buf, buf[G:G + n]

        def run(fill, want_gx=True, want_gp=True, hop=hop, expect=0):
            bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("gx", B * C * N), ("gP", B * F))}
            bufs["scr"] = guarded(nscr, fill)
            assert Lb.dasp_gaincurve_forward(ptr(x), ptr(P), ptr(bufs["y"][1]), B, C, N, hop, stream()) == expect
            rc = Lb.dasp_gaincurve_backward(ptr(x), ptr(P), ptr(gy), ptr(bufs["gx"][1] if want_gx else None), ptr(bufs["gP"][1] if want_gp else None),
                                            ptr(bufs["scr"][1] if want_gp else None), B, C, N, hop, stream())
            assert rc == expect
            torch.cuda.synchronize()
            for k, (buf, inner) in bufs.items():
                assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
            return {k: inner.clone() for k, (buf, inner) in bufs.items()}

        zero, dirty = run(0.0), run(float("nan"))
        for k in ("y", "gx", "gP"):
            assert torch.equal(zero[k].view(torch.int32), dirty[k].view(torch.int32)), k
        no_gx, no_gp = run(float("nan"), want_gx=False), run(float("nan"), want_gp=False)
        assert torch.equal(zero["gP"], no_gx["gP"]) and torch.isnan(no_gx["gx"]).all()
        assert torch.equal(zero["gx"], no_gp["gx"]) and torch.isnan(no_gp["gP"]).all() and torch.isnan(no_gp["scr"]).all()
        ref = run_t(D, a, hop)
        assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"]) and torch.equal(zero["gP"].view(B, F), ref["ggain"])
        refused = run(float("nan"), hop=24, expect=-2)                        # nothing launched: every word is still NaN
        assert all(torch.isnan(v).all() for v in refused.values())
    assert lib().dasp_device_error() == 0


# ---- 6. the composition: ducking ---------------------------------------------------------------------------------------------------------
def test_ducking_composition(D):
    """gain_curve(music, -0.5 relu(20 log10(envelope_follower(voice) + 1e-5) + 30)) at (2, 2, 3001), hop 64, against the same expression
    on the float64 restatements, with gradients to music, voice and smoothing_ms. Bounds: 4 x the error of the same composition on the
    float32 restatements, never below the floors (2e-6 of the peak for y and the audio gradients, 1e-5 for the control gradient); the
    errors are taken per item."""
    sr, hop, N = 44100, 64, 3001
    g = torch.Generator().manual_seed(11)
    music, w = 0.5 * torch.randn(2, 2, N, generator=g), torch.randn(2, 2, N, generator=g)
    burst = (torch.arange(N) % 1000 < 600).float()                          # the voice comes and goes: the curve crosses the -30 dB knee
    voice = 0.1 * torch.randn(2, 2, N, generator=g) * burst
    sm = torch.tensor([5.0, 20.0])

    def curve(E):
        return -0.5 * torch.relu(20.0 * torch.log10(E + 1e-5) + 30.0)

    def restated(arith):
        m, v, s = (t.double().clone().requires_grad_(True) for t in (music, voice, sm))
        if arith is torch.float64:
            E = ER.envelope(v, sr, s, hop)
            y = R.gain_curve(m, curve(E), hop)
            gm, gv, gs = torch.autograd.grad((y * w.double()).sum(), [m, v, s])
            return dict(y=y.detach().numpy(), gmusic=gm.numpy(), gvoice=gv.numpy(), gsm=gs.numpy())
        # float32: the two restatements in the kernels' arithmetic, chained by hand through the float32 curve
        F = ER.control_frames(N, hop)
        E32 = torch.from_numpy(ER.blocked(voice.numpy(), sr, sm.numpy(), np.zeros((2, F)), hop, "peak", np.float32)["E"]).float().requires_grad_(True)
        P = curve(E32)
        r = R.forward_backward(music, sr, P.detach(), w, hop, arith=torch.float32)
        (gE,) = torch.autograd.grad(P, E32, torch.from_numpy(r["ggain"]).float())
        e = ER.blocked(voice.numpy(), sr, sm.numpy(), gE.numpy(), hop, "peak", np.float32)
        return dict(y=r["y"], gmusic=r["gx"], gvoice=e["gx"], gsm=e["gsm"])

    want, f32 = restated(torch.float64), restated(torch.float32)
    mt, vt, st = (t.to(DEV).requires_grad_(True) for t in (music, voice, sm))
    y = D.gain_curve(mt, sr, curve(D.envelope_follower(vt, sr, st, hop=hop)), hop=hop)
    grads = torch.autograd.grad((y * w.to(DEV)).sum(), [mt, vt, st])
    got = dict(zip(("y", "gmusic", "gvoice", "gsm"), (y.detach().cpu().numpy(),) + tuple(t.cpu().numpy() for t in grads)))
    floor = dict(y=2e-6, gmusic=2e-6, gvoice=2e-6, gsm=1e-5)
    assert (want["y"] != music.double().numpy()).mean() > 0.3 and (want["y"] == music.double().numpy()).mean() > 0.05      # ducked, and not everywhere
    e, e32 = {}, {}
    for k in floor:
        e[k], e32[k] = K.per_item_err(got[k], want[k]), K.per_item_err(f32[k], want[k])
    record("ducking_composition", **e, **{"fp32_" + k: v for k, v in e32.items()})
    for k in floor:
        assert e[k] <= max(4 * e32[k], floor[k]), (k, e[k], e32[k])


def test_auto_wah_and_tremolo_compositions_run_and_differentiate(D):
    """The README's other two compositions: the envelope as the cutoff curve of time_varying_filter, and a sine on the frame points as
    a tremolo. Finite outputs of x's shape, finite gradients to the audio and to smoothing_ms; the tremolo against its closed form."""
    sr, hop, N = 44100, 64, 3001
    g = torch.Generator().manual_seed(12)
    x = (0.3 * torch.randn(2, 2, N, generator=g)).to(DEV).requires_grad_(True)
    sm = torch.tensor([5.0, 20.0], device=DEV, requires_grad=True)
    mix = torch.tensor([1.0, 0.7], device=DEV)
    env = D.envelope_follower(x, sr, sm, hop=hop)
    wah = D.time_varying_filter(x, sr, 300.0 + 6000.0 * env.clamp(max=1.0), torch.full_like(env, 4.0), mix, hop=hop, mode="bandpass")
    gx, gs = torch.autograd.grad(wah.pow(2).sum(), [x, sm])
    assert wah.shape == x.shape and all(torch.isfinite(t).all() for t in (wah, gx, gs)) and gs.ne(0).all() and float(env.min()) >= 0
    t = torch.arange(D.control_frames(N, hop), device=DEV) * hop / sr
    curve = (3.0 * torch.sin(2 * torch.pi * 5.0 * t) - 3.0).expand(2, -1)
    trem = D.gain_curve(x, sr, curve, hop=hop)
    want = x.detach().double() * torch.from_numpy(10.0 ** (R.interpolate(curve.cpu().double(), N, hop).numpy() / 20.0)).to(DEV)[:, None, :]
    assert float((trem.double() - want).abs().max() / want.abs().max()) <= FLOOR["y"]


# ---- 7. the autograd and call-state contracts -----------------------------------------------------------------------------------------------
def _spec():
    """The op's entry for the contract batteries, in the form of the entries of tests/autograd_contract_cases.py (that table is closed:
    tests/test_call_state_cpu.py pins its size). What is watched is GainCurveKernels, the class that holds the forward / backward pair
    that GainCurveFunction binds to autograd."""
    from dasp_pytorch_amd._ctypes_ops import GainCurveKernels
    from tests import autograd_contract_cases as A
    hop, N = 64, 1501
    F = R.control_frames(N, hop)

    def arrays(seed):
        g = A.gen(seed, 179)
        return dict(x=torch.rand(3, 2, N, generator=g) * 2 - 1, gain_db=torch.rand(3, F, generator=g) * 36.0 - 24.0)

    def call(t):
        import dasp_pytorch_amd
        return dasp_pytorch_amd.gain_curve(t["x"], 8000, t["gain_db"], hop=hop)

    names = dict(y="y0", gx="g_x", ggain="g_gain_db")

    def ref(a, gys):
        w = torch.from_numpy(gys[0])
        r64 = R.forward_backward(a["x"], 8000, a["gain_db"], w, hop)
        r32 = R.forward_backward(a["x"], 8000, a["gain_db"], w, hop, arith=torch.float32)
        bound = {names[k]: max(4.0 * peak_err(r32[k], r64[k]), FLOOR[k]) for k in names}
        return dict({names[k]: r64[k] for k in names}, _bound=bound)
    spec = A.measured_bound("gain_curve", arrays, call, ("x", "gain_db"), ("x",), ("GainCurveKernels",), ref, {names[k]: FLOOR[k] for k in names},
                            forms={"gain_db": "matrix"}, lowp=("x",), cite="tests/test_gpu_gain_curve.py test_parity_with_the_float64_restatement")
    spec.functions = lambda: [GainCurveKernels]
    return spec


def _contract(checks, check):
    spec, rec = _spec(), []
    try:
        find = checks[check](spec, rec)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in gain_curve {check}: {e}", returncode=3)        # nothing more runs on a device that has faulted
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
    y = D.gain_curve(x, 44100, a["gain_db"].to(DEV))
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 8. module, dtypes, the empty signal -----------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    x = plain(3, 2, 3000)["x"].to(DEV)
    F = R.control_frames(3000, 64)
    p = torch.rand(3, F, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = D.GainCurve(44100)
    with torch.no_grad():
        got = m.process_normalized(x, p)
        want = D.gain_curve(x, 44100, p * 72.0 - 60.0)
    assert torch.equal(got, want) and not torch.equal(got, x)


def test_empty_input(D):
    for B, C, N, F in ((2, 2, 0, 1), (0, 2, 16, 3)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        P = torch.zeros(B, F, device=DEV, requires_grad=True)
        y = D.gain_curve(x, 44100, P, hop=8)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and P.grad.shape == P.shape and not P.grad.any()


def test_half_and_bfloat16_are_converted_and_float64_is_refused(D):
    from dasp_pytorch_amd import _lib
    a = plain(2, 2, 3000)
    P = a["gain_db"].to(DEV)
    for dt in (torch.float16, torch.bfloat16):
        xl = a["x"].to(DEV).to(dt)
        with torch.no_grad():
            y = D.gain_curve(xl, 44100, P)
            want = D.gain_curve(xl.float(), 44100, P).to(dt)
        assert y.dtype == dt and torch.equal(y, want)
    with pytest.raises(_lib.DaspHipError, match="gain_curve: float64"):
        D.gain_curve(a["x"].to(DEV).double(), 44100, P)
