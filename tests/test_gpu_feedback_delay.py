"""GPU tests of feedback_delay (csrc/fbdelay.hip): parity of y, grad x and the four control gradients with the float64 restatement
(tests/feedback_delay_restated.py), exact identities, the adjoint, bit-for-bit reproducibility, what happens off the nominal domain, the refused
double backward and the module. The autograd and call-state contracts run on the op's entry in tests/autograd_contract_cases.py.

Parity bounds. The yardstick is the restatement with float64 D and float32 arithmetic on the same inputs on the CPU: e32 = its error
against float64 throughout, relative to the peak of the float64 result. The kernel's scan takes the one-pole in another order than the
restatement, so it gets 4 x e32, and never less than the floors of the other fused effects: 2e-6 of the peak for y and grad x, 1e-5 for
the control gradients. The op has no atomics: wherever two results are compared, every quantity is compared bit for bit.

The restatement is one torch step per block of at most L = i - 1 samples: a delay of two to four samples costs a Python step for every
one or two samples, which is what bounds the lengths here.
"""
import numpy as np
import pytest
import torch

from tests import feedback_delay_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTL, FLOOR = R.CTL, R.FLOOR
GRADS = ("gdelay", "gfeedback", "gdamping", "gmix")
# max_delay_ms per rate with sr/1000 max_delay_ms a whole number in float64: H = 5000, 5292, 4992
MDM = {8000: 625.0, 44100: 120.0, 192000: 26.0}
FEEDBACK = (0.0, 0.9, -0.9, 0.98)
DAMPING = (float("inf"), 8000.0, 300.0, -5.0)
INF = float("inf")


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def delays(sr, mdm, long_only=False):
    """delay_ms of the eight D of the parity cases, in samples: 2.0 (delay_ms = 0: the lower clamp, one-sample steps), 2.5, 3.999, 24 (a
    whole number at 8 kHz), 88.3, 4410.7, exactly H (delay_ms = max_delay_ms) and above H (clamped). long_only: without the first three."""
    k = sr / 1000.0
    d = [0.0, 2.5 / k, 3.999 / k, 24.0 / k, 88.3 / k, 4410.7 / k, mdm, 1.3 * mdm]
    return d[3:] if long_only else d


def draw(sr, C, N, mdm=None, case=0, long_only=False, repeat=1, seed=0):
    """One item per D of delays() (x repeat), every feedback of FEEDBACK and damping of DAMPING, paired differently from case to case (the
    cases of a rate together hold all sixteen pairs for every D); x in [-1, 1), w normal, mix 0.2 - 1."""
    mdm = MDM[sr] if mdm is None else mdm
    dl = delays(sr, mdm, long_only) * repeat
    B = len(dl)
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * C + N + sr)
    j = np.arange(B)
    return dict(x=torch.rand(B, C, N, generator=g) * 2 - 1, w=torch.randn(B, C, N, generator=g), delay_ms=torch.tensor(dl, dtype=torch.float32),
                feedback=torch.tensor([FEEDBACK[q % 4] for q in j], dtype=torch.float32),
                damping_hz=torch.tensor([DAMPING[(q + q // 4 + case) % 4] for q in j], dtype=torch.float32),
                mix=torch.rand(B, generator=g) * 0.8 + 0.2)


def plain(B, C, N, seed=0, delay=(0.06, 100.0), feedback=(-0.9, 0.9), damping=(200.0, 20000.0)):
    """Everything inside its range at 44.1 kHz / 120 ms: delays of 2.6 - 4410 samples, log-uniform."""
    g = torch.Generator().manual_seed(77 * seed + 7 * B + 3 * C + N)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g), delay_ms=torch.exp(u(np.log(delay[0]), np.log(delay[1]), B)),
                feedback=u(*feedback, B), damping_hz=u(*damping, B), mix=u(0.2, 1.0, B))


def run_t(D, a, sr, need_gx=True, **kw):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    y = D.feedback_delay(x, sr, *ctl, **kw)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + ctl)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + GRADS, (y.detach(),) + grads))


def restated(a, sr, **kw):
    return R.forward_backward(a["x"], sr, *[a[k] for k in CTL], a["w"], **kw)


def check_parity(D, name, a, sr, mdm):
    want, f32 = restated(a, sr, max_delay_ms=mdm), restated(a, sr, max_delay_ms=mdm, arith=torch.float32)
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, sr, max_delay_ms=mdm).items()}
    e32 = {k: peak_err(f32[k], want[k]) for k in R.NAMES}
    e = {k: peak_err(got[k], want[k]) for k in R.NAMES}
    record(name, **e, **{"fp32_" + k: v for k, v in e32.items()}, **{"share_" + k: e[k] / max(4 * e32[k], FLOOR[k]) for k in R.NAMES})
    for k in R.NAMES:
        assert got[k].shape == want[k].shape, (name, k)
        assert e[k] <= max(4 * e32[k], FLOOR[k]), (name, k, e[k], e32[k])
    k = sr / 1000.0
    clamped = (k * a["delay_ms"].double().numpy() < 2.0) | (k * a["delay_ms"].double().numpy() > k * mdm)
    assert not got["gdelay"][clamped].any() and not want["gdelay"][clamped].any()                # a clamped D: exactly no gradient
    off = ~(a["damping_hz"].numpy() >= 0) | np.isinf(a["damping_hz"].numpy())
    assert not got["gdamping"][off].any() and not want["gdamping"][off].any()                    # damping_hz < 0 or +inf: exactly none
    return got, want


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
def lengths(sr):
    """(channels, N, long_only). With S = dasp_fbdelay_block(H, L) samples per step: the 88.3-sample delay has L = S = 87 (86, 87, 88 are
    S - 1, S = L, S + 1 = L + 1), the 4410.7-sample one L = 4409 and S = 2048. The lengths from 2047 on are thresholds of the long delays
    only and leave the three shortest D out (a Python step per sample in the restatement)."""
    H = R.delay_samples(sr, MDM[sr])
    S = lib().dasp_fbdelay_block(H, 4409)
    assert S == 2048 and lib().dasp_fbdelay_block(H, 87) == 87 and lib().dasp_fbdelay_block(H, 1) == 1
    return [(1, 1, False), (2, 86, False), (2, 87, False), (1, 88, False), (1, S - 1, True), (2, S, True), (1, S + 1, True), (1, 4409, True),
            (2, 4410, True)]


@pytest.mark.parametrize("case", range(9))
@pytest.mark.parametrize("sr", [8000, 44100, 192000])
def test_parity_with_the_float64_restatement(D, sr, case):
    C, N, long_only = lengths(sr)[case]
    a = draw(sr, C, N, case=case, long_only=long_only)
    check_parity(D, f"fbdelay_parity sr={sr} ({a['x'].shape[0]},{C},{N})", a, sr, MDM[sr])


@pytest.mark.parametrize("sr", [8000, 44100, 192000])
def test_parity_past_two_wraps_of_the_ring(D, sr):
    """max_delay_ms of 300 samples: H = 300, a ring of 300 + 2 + 299 words, N five samples past two wraps. 4410.7 samples is one more
    clamped delay here."""
    mdm = 300.0 / (sr / 1000.0)
    H = R.delay_samples(sr, mdm)
    assert H in (300, 301)
    N = 2 * (H + 2 + H - 1) + 5
    check_parity(D, f"fbdelay_parity wraps sr={sr} (8,2,{N})", draw(sr, 2, N, mdm=mdm, case=3), sr, mdm)


@pytest.mark.parametrize("sr", [8000, 44100, 192000])
def test_parity_of_a_training_batch(D, sr):
    """(64, 2, 8192): 128 workgroups; the 2048-sample steps wrap the ring of 5000 + 2 + 2048 words once. The five D from 24 samples up,
    thirteen times over (the three shortest would be 8192 Python steps of the restatement: they have the next test)."""
    a = {k: v[:64] for k, v in draw(sr, 2, 8192, case=5, long_only=True, repeat=13).items()}
    assert a["x"].shape == (64, 2, 8192)
    check_parity(D, f"fbdelay_parity sr={sr} (64,2,8192)", a, sr, MDM[sr])


def test_parity_of_the_shortest_delays_over_thousands_of_steps(D):
    """D = 2.0, 2.5 and 3.999 at (3, 2, 4099): 4099 one-sample steps, 2050 two-sample steps."""
    sr = 44100
    a = {k: v[:3] for k, v in draw(sr, 2, 4099, case=2).items()}
    check_parity(D, "fbdelay_parity shortest (3,2,4099)", a, sr, MDM[sr])


def test_parity_at_the_longest_delay(D):
    """H = dasp_fbdelay_max_delay_samples(): the whole LDS ring, D on the bound and at 20000.3 samples, one length past two wraps."""
    sr = 44100
    H = lib().dasp_fbdelay_max_delay_samples()
    mdm = H / 44.1
    while R.delay_samples(sr, mdm) > H:
        mdm = np.nextafter(mdm, 0.0)
    assert R.delay_samples(sr, mdm) == H and H >= 32768
    N = 2 * (H + 2 + 2048) + 5
    g = torch.Generator().manual_seed(9)
    a = dict(x=torch.rand(2, 1, N, generator=g) * 2 - 1, w=torch.randn(2, 1, N, generator=g), delay_ms=torch.tensor([2.0 * mdm, 20000.3 / 44.1]),
             feedback=torch.tensor([0.9, -0.98]), damping_hz=torch.tensor([3000.0, INF]), mix=torch.tensor([0.5, 1.0]))
    check_parity(D, f"fbdelay_parity longest (2,1,{N})", a, sr, float(mdm))


# ---- 2. exact identities -----------------------------------------------------------------------------------------------------------------
def test_mix_zero_is_the_identity(D):
    a = plain(4, 2, 5000)
    a["mix"] = torch.zeros(4)
    with torch.no_grad():
        y = D.feedback_delay(a["x"].to(DEV), 44100, *[a[k].to(DEV) for k in CTL], max_delay_ms=120.0)
    assert torch.equal(y.cpu(), a["x"])


def test_whole_sample_delay_without_feedback_is_a_shift(D):
    """8 kHz, 3 ms and 275 ms, feedback 0, no damping, all wet: D = 24 and 2200 exactly, f = 0, the weights are 0, 1, 0, 0 and v = x."""
    x = plain(2, 2, 9000)["x"]
    t = lambda *v: torch.tensor(v, device=DEV)
    with torch.no_grad():
        y = D.feedback_delay(x.to(DEV), 8000, t(3.0, 275.0), t(0.0, 0.0), t(INF, INF), t(1.0, 1.0), max_delay_ms=625.0).cpu()
    for b, d in enumerate((24, 2200)):
        assert torch.equal(y[b, :, d:], x[b, :, :-d]) and not y[b, :, :d].any()


def test_no_echo_yet_where_the_signal_is_shorter_than_the_delay(D):
    """seq_len = 1000 under a delay of 4410.7 samples: r is zero, y = (1 - mix) x, grad x = (1 - mix) gy, and nothing reaches feedback,
    damping_hz or delay_ms; mix gets -sum gy x."""
    a = plain(2, 2, 1000)
    a["delay_ms"] = torch.full((2,), 4410.7 / 44.1)
    got = run_t(D, a, 44100, max_delay_ms=120.0)
    dry = (1 - a["mix"]).view(2, 1, 1)
    assert torch.equal(got["y"].cpu(), dry * a["x"]) and torch.equal(got["gx"].cpu(), dry * a["w"])
    assert not got["gdelay"].any() and not got["gfeedback"].any() and not got["gdamping"].any()
    want = -(a["w"].double() * a["x"].double()).sum((1, 2))
    assert peak_err(got["gmix"].cpu().numpy(), want.numpy()) < 1e-5


# ---- 3. adjoint --------------------------------------------------------------------------------------------------------------------------
def test_adjoint(D):
    """The op is linear in x: <y, w> = <x, gx>, both sums taken in float64 on the host from the kernel's float32 outputs. The relative
    difference, the largest over four draws of w, is within 4 x that of the float32-arithmetic restatement and never above 1e-5."""
    sr = 44100
    a = plain(4, 2, 6000, delay=(0.5, 100.0))
    g = torch.Generator().manual_seed(77)
    rel = lambda y, gx, w: abs(float((np.float64(y) * w).sum() - (a["x"].double().numpy() * np.float64(gx)).sum())) / abs(float((np.float64(y) * w).sum()))
    got, want = [], []
    for _ in range(4):
        a["w"] = torch.randn(a["x"].shape, generator=g)
        w = a["w"].double().numpy()
        k = run_t(D, a, sr, max_delay_ms=120.0)
        got.append(rel(k["y"].cpu().numpy(), k["gx"].cpu().numpy(), w))
        r = restated(a, sr, max_delay_ms=120.0, arith=torch.float32)
        want.append(rel(r["y"].astype(np.float32), r["gx"].astype(np.float32), w))
    record("fbdelay_adjoint", kernel=max(got), restated_fp32=max(want))
    assert max(got) <= 4 * max(want) and max(got) <= 1e-5, (got, want)


# ---- 4. reproducibility: everything bit for bit ------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(D):
    a = plain(6, 2, 9000)
    p, q = run_t(D, a, 44100, max_delay_ms=120.0), run_t(D, a, 44100, max_delay_ms=120.0)
    for k in R.NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, need_gx=False, max_delay_ms=120.0)         # x needs no gradient: gx is not written, nothing else changes
    for k in ("y",) + GRADS:
        assert torch.equal(p[k], r[k]), k


def test_item_alone_and_inside_a_batch(D):
    a = plain(5, 2, 7000)
    whole = run_t(D, a, 44100, max_delay_ms=120.0)
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, max_delay_ms=120.0)
        for k in R.NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path, nothing to zero, and the LDS
    limit of the kernels was raised when the library was loaded."""
    sr = 44100
    a = plain(4, 2, 6000)
    eager = run_t(D, a, sr, max_delay_ms=120.0)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.feedback_delay(xt, sr, *ctl, max_delay_ms=120.0)
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
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 5. off the nominal domain -----------------------------------------------------------------------------------------------------------
def _item0_unchanged(clean, dirty):
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_audio_and_controls_stay_in_their_item(D, value):
    a = plain(2, 2, 5000)
    clean = run_t(D, a, 44100, max_delay_ms=120.0)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    for k in CTL:
        b[k][1] = float("nan")
    dirty = run_t(D, b, 44100, max_delay_ms=120.0)
    _item0_unchanged(clean, dirty)
    assert torch.isnan(dirty["y"][1]).all() and torch.isnan(dirty["gx"][1]).all() and all(torch.isnan(dirty[k][1]) for k in GRADS)


def test_poisoned_upstream_gradient_stays_in_its_item(D):
    a = plain(2, 2, 5000)
    clean = run_t(D, a, 44100, max_delay_ms=120.0)
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = float("nan")
    dirty = run_t(D, b, 44100, max_delay_ms=120.0)
    _item0_unchanged(clean, dirty)
    assert torch.equal(clean["y"], dirty["y"]) and all(torch.isnan(dirty[k][1]) for k in GRADS)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["x", "w"])
def test_one_bad_sample_reaches_what_the_restatement_says(D, where, value):
    """One NaN or +inf in the middle of row (0, 0): in x, the isfinite mask of y equals the float64 restatement's (the sample stays in the
    line: every echo after it); in the upstream gradient, that of grad x does (every sample that echoes into it)."""
    a = plain(2, 2, 4000, delay=(5.0, 30.0))
    a[where][0, 0, 2000] = value
    got, want = run_t(D, a, 44100, max_delay_ms=120.0), restated(a, 44100, max_delay_ms=120.0, block=1)     # (a wider block is a matrix product: 0 x inf)
    key = "y" if where == "x" else "gx"
    mask = torch.isfinite(got[key]).cpu().numpy()
    assert np.array_equal(mask, np.isfinite(want[key])) and 0 < (~mask).sum() < mask.size // 2


def test_nan_delay_gives_a_nan_item(D):
    a = plain(3, 2, 5000)
    clean = run_t(D, a, 44100, max_delay_ms=120.0)
    a["delay_ms"][1] = float("nan")
    dirty = run_t(D, a, 44100, max_delay_ms=120.0)
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
        assert torch.isnan(dirty[k][1]).all(), k


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    a = plain(3, 2, 2500)
    want = run_t(D, a, 44100, max_delay_ms=120.0)
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
    ctl = [torch.stack([a[k], a[k]], -1).to(DEV)[:, 1].requires_grad_(True) for k in CTL]            # strided controls
    y = D.feedback_delay(xv, 44100, *ctl, max_delay_ms=120.0)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    for k, g in zip(R.NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_and_ignores_dirty_scratch(D):
    """Through the C ABI: y, v, gx, gctl and the partials written inside NaN-filled guard words leave the guards NaN, a NaN-filled
    partials buffer gives the same bits as a zero-filled one, and v = NULL / gx = NULL change nothing else."""
    from dasp_pytorch_amd._lib import call, ptr, stream
    sr, mdm, G = 44100, 120.0, 64
    H = R.delay_samples(sr, mdm)
    B, C, N = 3, 2, 5333
    a = plain(B, C, N)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    ctl = torch.stack([a[k] for k in CTL], -1).contiguous().to(DEV)
    npart = lib().dasp_fbdelay_partial_floats(B * C, N, H)
    assert npart == 4 * B * C

    def guarded(n, fill=float("nan")):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        buf[G:G + n] = fill
        return buf, buf[G:G + n]

    def run(fill, save=True, want_gx=True):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("v", B * C * N), ("gx", B * C * N), ("gctl", B * 4))}
        bufs["partials"] = guarded(npart, fill)
        call("dasp_fbdelay_forward", ptr(x), ptr(ctl), ptr(bufs["y"][1]), ptr(bufs["v"][1] if save else None), B, C, N, H, float(sr), mdm, stream())
        if not save:
            call("dasp_fbdelay_forward", ptr(x), ptr(ctl), ptr(torch.empty_like(x)), ptr(bufs["v"][1]), B, C, N, H, float(sr), mdm, stream())
        call("dasp_fbdelay_backward", ptr(x), ptr(ctl), ptr(bufs["v"][1]), ptr(gy), ptr(bufs["gx"][1] if want_gx else None), ptr(bufs["gctl"][1]),
             ptr(bufs["partials"][1]), B, C, N, H, float(sr), mdm, stream())
        torch.cuda.synchronize()
        for k, (buf, inner) in bufs.items():
            assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
            assert torch.isfinite(inner).all() or (k == "gx" and not want_gx and torch.isnan(inner).all()), k
        return {k: inner.clone() for k, (buf, inner) in bufs.items()}

    zero, dirty, lean = run(0.0), run(float("nan")), run(0.0, save=False, want_gx=False)
    for k in ("y", "v", "gx", "gctl", "partials"):
        assert torch.equal(zero[k], dirty[k]), k
    for k in ("y", "v", "gctl", "partials"):
        assert torch.equal(zero[k], lean[k]), k
    ref = run_t(D, a, sr, max_delay_ms=mdm)
    assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"])
    for q, k in enumerate(GRADS):
        assert torch.equal(zero["gctl"].view(B, 4)[:, q], ref[k]), k


def test_silence_in_silence_out(D):
    a = plain(2, 2, 5000)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100, max_delay_ms=120.0)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS)


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        ctl = [torch.ones(B, device=DEV, requires_grad=True) for _ in range(4)]
        y = D.feedback_delay(x, 44100, *ctl)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


def test_too_long_a_line_is_refused_on_the_host(D):
    from dasp_pytorch_amd import _lib
    x = torch.zeros(1, 1, 64, device=DEV)
    with pytest.raises(_lib.DaspHipError, match="unsupported"):
        D.feedback_delay(x, 192000, *[torch.ones(1, device=DEV) for _ in range(4)], max_delay_ms=500.0)


# ---- 6. double backward ------------------------------------------------------------------------------------------------------------------
def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.feedback_delay(x, 44100, *[a[k].to(DEV) for k in CTL], max_delay_ms=120.0)
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 7. module ---------------------------------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    sr = 44100
    x = plain(3, 2, 3000)["x"].to(DEV)
    p = torch.rand(3, 4, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = D.FeedbackDelay(sr, max_delay_ms=80.0)
    lo = torch.tensor([1.0, 0.0, 200.0, 0.0], device=DEV)
    span = torch.tensor([79.0, 0.95, 19800.0, 1.0], device=DEV)
    with torch.no_grad():
        got = m.process_normalized(x, p)
        d = p * span + lo
        want = D.feedback_delay(x, sr, d[:, 0], d[:, 1], d[:, 2], d[:, 3], max_delay_ms=80.0)
    assert torch.equal(got, want)
