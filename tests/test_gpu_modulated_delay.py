"""GPU tests of modulated_delay (csrc/moddelay.hip): parity of y, grad x and the five control gradients with the float64 restatement
(tests/modulated_delay_restated.py), clamping, exact identities, the adjoint, reproducibility, what happens off the nominal domain, and
the module.

Parity bounds. The yardstick is the restatement with a float64 position and float32 arithmetic on the same inputs on the CPU: e32 = its
error against float64 / float64, relative to the peak of the float64 result. The kernel sums in another order, so it gets 4 x e32, and
never less than the floors of tests/test_gpu_oversampled_distortion.py: 2e-6 of the peak for y and grad x, 1e-5 for control gradients.

grad x is accumulated with LDS float adds whose order varies between runs (csrc/moddelay.hip, pass B): wherever the other quantities are
compared bit for bit, two grad x agree within the parity floor, 2e-6 of the peak, instead.
"""
import numpy as np
import pytest
import torch

from tests import modulated_delay_restated as R
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MDM = 40.0                                   # max_delay_ms of every case but the clamping one: H = 320, 1764, 7680 at the three rates
CTL = ("delay_ms", "depth_ms", "rate_hz", "phase", "mix")
GRADS = ("gdelay", "gdepth", "grate", "gphase", "gmix")
FLOOR = dict(y=2e-6, gx=2e-6, gdelay=1e-5, gdepth=1e-5, grate=1e-5, gphase=1e-5, gmix=1e-5)


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def tile(sr, mdm=MDM):
    from dasp_pytorch_amd import _lib
    return _lib.lib().dasp_moddelay_tile(R.delay_samples(sr, mdm))


def draw(B, C, N, V, seed=0, delay=(5.0, 25.0), depth=(0.0, 4.0)):
    """x in [-1, 1), w normal; delays of 5 - 25 ms moved by up to 4 ms (never clamped at 40 ms), 0.1 - 8 Hz, any phase, mix 0.2 - 1."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * C + N + 131 * V)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g), delay_ms=u(*delay, B, V), depth_ms=u(*depth, B, V),
                rate_hz=u(0.1, 8.0, B, V), phase=u(0.0, 1.0, B, V), mix=u(0.2, 1.0, B))


def run_t(D, a, sr, need_gx=True, **kw):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    y = D.modulated_delay(x, sr, *ctl, **kw)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + ctl)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + GRADS, (y.detach(),) + grads))


def restated(a, sr, **kw):
    return R.forward_backward(a["x"], sr, *[a[k] for k in CTL], a["w"], **kw)


def peak_err(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def close_gx(a, b):
    """Two grad x of the kernel on the same inputs: equal to the parity floor (the order of the LDS adds varies)."""
    return peak_err(a.cpu().numpy(), b.cpu().numpy()) <= FLOOR["gx"]


def check_parity(D, name, a, sr, **kw):
    want, f32 = restated(a, sr, **kw), restated(a, sr, arith=torch.float32, **kw)
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, sr, **kw).items()}
    e32 = {k: peak_err(f32[k], want[k]) for k in R.NAMES}
    e = {k: peak_err(got[k], want[k]) for k in R.NAMES}
    record(name, **e, **{"fp32_" + k: v for k, v in e32.items()})
    for k in R.NAMES:
        assert got[k].shape == want[k].shape, (name, k)
        assert e[k] <= max(4 * e32[k], FLOOR[k]), (name, k, e[k], e32[k])
    return want


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
def shapes(sr):
    T, H = tile(sr), R.delay_samples(sr, MDM)
    return [(1, 1, 1), (2, 2, 5), (2, 3, T - 1), (2, 2, T), (1, 2, T + 1), (1, 1, 2 * T + H + 1), (3, 1, 10001), (64, 2, 8192)]


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("V", [1, 3, 8])
@pytest.mark.parametrize("sr", [8000, 44100, 192000])
def test_parity_with_the_float64_restatement(D, sr, V, case):
    """Every delay is at least 5 ms - 40 samples at 8 kHz, 960 at 192 kHz - so the first samples of a tile read from the tile before it
    (or from before the signal), and the scatter of grad x reaches into the tile after it."""
    B, C, N = shapes(sr)[case]
    check_parity(D, f"moddelay_parity sr={sr} V={V} ({B},{C},{N})", draw(B, C, N, V), sr)


def test_parity_of_a_flanger_below_one_sample(D):
    """Delays of 0 - 0.1 ms at 8 kHz: d < 1 sample for most of the cycle, the footprint reaches x[n+1] and x[n+2]; H = 1."""
    sr, V = 8000, 2
    a = draw(2, 2, tile(sr, 0.125) + 77, V, delay=(0.03, 0.06), depth=(0.0, 0.03))
    check_parity(D, "moddelay_parity sub-sample", a, sr, max_delay_ms=0.125)


# ---- 2. clamping -------------------------------------------------------------------------------------------------------------------------
def test_parity_where_the_delay_is_clamped(D):
    """max_delay_ms = 10 with delays of 2 - 8 ms moved by 5 - 9 ms: d sits on 0 and on the upper bound for a good part of every cycle, and
    those samples give the delay gradients nothing."""
    sr, V, mdm = 44100, 3, 10.0
    a = draw(2, 2, tile(sr, mdm) + 500, V, delay=(2.0, 8.0), depth=(5.0, 9.0))
    a["rate_hz"] = a["rate_hz"] * 4 + 20.0                       # several cycles inside 4596 samples
    n = torch.arange(a["x"].shape[-1], dtype=torch.float64)
    raw = a["delay_ms"].double()[..., None] + a["depth_ms"].double()[..., None] * torch.sin(
        2 * np.pi * (a["rate_hz"].double()[..., None] * n / sr + a["phase"].double()[..., None]))
    low, high = float((raw < 0).double().mean()), float((raw > mdm).double().mean())
    assert low > 0.1 and high > 0.1, (low, high)
    check_parity(D, "moddelay_parity clamped", a, sr, max_delay_ms=mdm)


# ---- 3. exact identities -----------------------------------------------------------------------------------------------------------------
def test_mix_zero_is_the_identity(D):
    a = draw(2, 2, 5000, 3)
    a["mix"] = torch.zeros(2)
    with torch.no_grad():
        y = D.modulated_delay(a["x"].to(DEV), 44100, *[a[k].to(DEV) for k in CTL])
    assert torch.equal(y.cpu(), a["x"])


def test_whole_sample_delay_is_a_shift(D):
    """48 kHz, 2.5 ms, no modulation, all wet: d = 120 exactly, f = 0, the weights are 0, 1, 0, 0."""
    a = draw(2, 2, 9000, 1)
    x = a["x"]
    one = lambda v: torch.full((2,), v)
    with torch.no_grad():
        y = D.modulated_delay(x.to(DEV), 48000, one(2.5).to(DEV), one(0.0).to(DEV), a["rate_hz"].to(DEV), a["phase"].to(DEV), one(1.0).to(DEV)).cpu()
    assert torch.equal(y[..., 120:], x[..., :-120]) and not y[..., :120].any()


# ---- 4. adjoint --------------------------------------------------------------------------------------------------------------------------
def test_adjoint(D):
    """The op is linear in x: <y, w> = <x, gx>, both sums taken in float64 on the host from the kernel's float32 outputs. The relative
    difference, the largest over four draws of w, is within 4 x that of the float32-arithmetic restatement and never above 1e-5."""
    sr, V = 44100, 3
    a = draw(2, 2, tile(sr) + 1904, V)
    g = torch.Generator().manual_seed(77)
    rel = lambda y, gx, w: abs(float((np.float64(y) * w).sum() - (a["x"].double().numpy() * np.float64(gx)).sum())) / abs(float((np.float64(y) * w).sum()))
    got, want = [], []
    for _ in range(4):
        a["w"] = torch.randn(a["x"].shape, generator=g)
        w = a["w"].double().numpy()
        k = run_t(D, a, sr)
        got.append(rel(k["y"].cpu().numpy(), k["gx"].cpu().numpy(), w))
        r = restated(a, sr, arith=torch.float32)
        want.append(rel(r["y"].astype(np.float32), r["gx"].astype(np.float32), w))
    record("moddelay_adjoint", kernel=max(got), restated_fp32=max(want))
    assert max(got) <= 4 * max(want) and max(got) <= 1e-5, (got, want)


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------------
BITWISE = ("y",) + GRADS


def test_runs_are_bit_identical(D):
    sr = 44100
    a = draw(3, 2, 3 * tile(sr) + 77, 3)
    p, q = run_t(D, a, sr), run_t(D, a, sr)
    for k in BITWISE:
        assert torch.equal(p[k], q[k]), k
    assert close_gx(p["gx"], q["gx"])
    r = run_t(D, a, sr, need_gx=False)                         # x needs no gradient: the scatter pass is skipped, nothing else changes
    for k in BITWISE:
        assert torch.equal(p[k], r[k]), k


def test_item_alone_and_inside_a_batch(D):
    sr, b = 44100, 2
    a = draw(4, 2, 2 * tile(sr) + 13, 3)
    whole = run_t(D, a, sr)
    alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, sr)
    assert torch.equal(whole["y"][b], alone["y"][0])
    for k in GRADS:
        assert torch.equal(whole[k][b], alone[k][0]), k
    assert close_gx(whole["gx"][b], alone["gx"][0])


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path, nothing to zero."""
    sr = 44100
    a = draw(3, 2, 2 * tile(sr) + 500, 3)
    eager = run_t(D, a, sr)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.modulated_delay(xt, sr, *ctl)
        return (y,) + torch.autograd.grad((y * wt).sum(), [xt] + ctl)

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
        for key, o in zip(R.NAMES, outs):
            if key == "gx":
                assert close_gx(o.detach(), eager[key]), k
            else:
                assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 6. off the nominal domain -----------------------------------------------------------------------------------------------------------
def _item0_unchanged(clean, dirty):
    assert torch.equal(clean["y"][0], dirty["y"][0])
    for k in GRADS:
        assert torch.equal(clean[k][0], dirty[k][0]), k
    assert close_gx(clean["gx"][0], dirty["gx"][0])


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_audio_and_controls_stay_in_their_item(D, value):
    sr = 44100
    a = draw(2, 2, tile(sr) + 300, 3)
    clean = run_t(D, a, sr)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    for k in CTL:
        b[k][1] = float("nan")
    dirty = run_t(D, b, sr)
    _item0_unchanged(clean, dirty)
    assert torch.isnan(dirty["y"][1]).all() and torch.isnan(dirty["gx"][1]).all()


def test_poisoned_upstream_gradient_stays_in_its_item(D):
    sr = 44100
    a = draw(2, 2, tile(sr) + 300, 3)
    clean = run_t(D, a, sr)
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = float("nan")
    dirty = run_t(D, b, sr)
    _item0_unchanged(clean, dirty)
    assert torch.equal(clean["y"], dirty["y"]) and all(torch.isnan(dirty[k][1]).all() for k in GRADS)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["x", "w"])
def test_one_bad_sample_reaches_what_the_restatement_says(D, where, value):
    """One NaN or +inf at sample T - 1 of row (0, 0), the last sample of the first tile: in x, the isfinite mask of y equals the float64
    restatement's; in the upstream gradient, that of grad x does."""
    sr = 44100
    T = tile(sr)
    a = draw(2, 2, T + 2500, 3)
    a[where][0, 0, T - 1] = value
    got, want = run_t(D, a, sr), restated(a, sr)
    key = "y" if where == "x" else "gx"
    mask = torch.isfinite(got[key]).cpu().numpy()
    assert np.array_equal(mask, np.isfinite(want[key])) and 0 < (~mask).sum() < mask.size // 4


def test_nan_delay_gives_a_nan_item(D):
    sr = 44100
    a = draw(2, 2, tile(sr) + 300, 3)
    clean = run_t(D, a, sr)
    a["delay_ms"][1, 1] = float("nan")
    dirty = run_t(D, a, sr)
    _item0_unchanged(clean, dirty)
    assert torch.isnan(dirty["y"][1]).all() and torch.isnan(dirty["gx"][1]).all()


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    sr = 44100
    a = draw(3, 2, 2500, 3)
    want = run_t(D, a, sr)
    x = a["x"].to(DEV)
    if view == "offset":
        xv = torch.cat([torch.zeros(5, device=DEV), x.reshape(-1)])[5:].view(3, 2, 2500)
    elif view == "strided":
        xv = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not xv.is_contiguous()
    else:
        xv = torch.cat([x, torch.ones(3, 2, 40, device=DEV)], -1)[..., :2500]
        assert not xv.is_contiguous()
    assert torch.equal(xv, x)
    xv.requires_grad_(True)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    y = D.modulated_delay(xv, sr, *ctl)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    assert torch.equal(y, want["y"]) and close_gx(grads[0], want["gx"])
    for k, g in zip(GRADS, grads[1:]):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_and_ignores_dirty_scratch(D):
    """Through the C ABI: y, gx, gctl and gmix written inside NaN-filled guard words leave the guards NaN, and a NaN-filled partials buffer
    gives the same bits as a zero-filled one."""
    from dasp_pytorch_amd import _lib
    from dasp_pytorch_amd._lib import call, ptr, stream
    sr, V, G = 44100, 3, 64
    H = R.delay_samples(sr, MDM)
    B, C, N = 2, 2, tile(sr) + 333
    a = draw(B, C, N, V)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    ctl = torch.stack([a[k] for k in CTL[:4]], -1).contiguous().to(DEV)
    mix = a["mix"].to(DEV)
    npart = _lib.lib().dasp_moddelay_partial_floats(B * C, N, V, H)
    assert npart == B * C * 2 * (4 * V + 1)

    def guarded(n):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        return buf, buf[G:G + n]

    def run(fill):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("gx", B * C * N), ("gctl", B * V * 4), ("gmix", B))}
        partials = torch.full((npart,), fill, device=DEV)
        call("dasp_moddelay_forward", ptr(x), ptr(ctl), ptr(mix), ptr(bufs["y"][1]), B, C, N, V, H, float(sr), MDM, 0.25, stream())
        call("dasp_moddelay_backward", ptr(x), ptr(ctl), ptr(mix), ptr(gy), ptr(bufs["gx"][1]), ptr(bufs["gctl"][1]), ptr(bufs["gmix"][1]),
             ptr(partials), B, C, N, V, H, float(sr), MDM, 0.25, stream())
        torch.cuda.synchronize()
        for k, (buf, inner) in bufs.items():
            assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all() and torch.isfinite(inner).all(), k
        return {k: inner.clone() for k, (buf, inner) in bufs.items()}

    zero, dirty = run(0.0), run(float("nan"))
    for k in ("y", "gctl", "gmix"):
        assert torch.equal(zero[k], dirty[k]), k
    assert close_gx(zero["gx"], dirty["gx"])
    ref = run_t(D, a, sr)
    assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gmix"], ref["gmix"])
    for q, k in enumerate(GRADS[:4]):
        assert torch.equal(zero["gctl"].view(B, V, 4)[..., q], ref[k]), k


def test_silence_in_silence_out(D):
    sr = 44100
    a = draw(2, 2, tile(sr) + 300, 3)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, sr)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS)


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        ctl = [torch.zeros(B, 2, device=DEV, requires_grad=True) for _ in range(4)] + [torch.zeros(B, device=DEV, requires_grad=True)]
        y = D.modulated_delay(x, 44100, *ctl)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


def test_unsupported_configurations_raise(D):
    from dasp_pytorch_amd import _lib
    x = torch.zeros(1, 1, 64, device=DEV)
    nine = [torch.zeros(1, 9, device=DEV) for _ in range(4)] + [torch.zeros(1, device=DEV)]
    with pytest.raises(_lib.DaspHipError, match="unsupported"):
        D.modulated_delay(x, 44100, *nine)
    one = [torch.zeros(1, device=DEV) for _ in range(5)]
    with pytest.raises(_lib.DaspHipError, match="unsupported"):
        D.modulated_delay(x, 192000, *one, max_delay_ms=50.0)


# ---- 7. module ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voices", [1, 3])
def test_module_equals_functional(D, voices):
    sr = 44100
    x = draw(3, 2, 3000, 1)["x"].to(DEV)
    p = torch.rand(3, 4 * voices + 1, generator=torch.Generator().manual_seed(voices)).to(DEV)
    m = D.ModulatedDelay(sr, voices=voices)
    lo = torch.tensor([0.0, 0.0, 0.05, 0.0], device=DEV)
    span = torch.tensor([30.0, 5.0, 9.95, 1.0], device=DEV)
    with torch.no_grad():
        got = m.process_normalized(x, p)
        d = p[:, :-1].view(3, voices, 4) * span + lo
        want = D.modulated_delay(x, sr, d[..., 0], d[..., 1], d[..., 2], d[..., 3], p[:, -1], max_delay_ms=35.0)
    assert torch.equal(got, want)
