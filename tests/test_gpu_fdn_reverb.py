"""GPU tests of fdn_reverb (csrc/fdn.hip): parity of y, grad x and the three control gradients with the float64 restatement
(tests/fdn_reverb_restated.py), exact identities, the adjoint, bit-for-bit reproducibility, what happens off the nominal domain, the refused
double backward and the module. The autograd and call-state contracts run on the op's entry in tests/autograd_contract_cases.py.

Parity bounds, the convention of the fused effects. The yardstick is the restatement with float64 g and a and float32 arithmetic on the
same inputs on the CPU: e32 = its error against float64 throughout, relative to the peak of the float64 result. The kernel's scans take
the one-poles in another order than the restatement, so it gets 4 x e32, and never less than the floors: 2e-6 of the peak for y and grad
x, 1e-5 for the control gradients. The op has no atomics: wherever two results are compared, every quantity is compared bit for bit.

The restatement runs in blocks of at most 256 samples (any block up to the shortest line gives the same float64 result to rounding,
tests/test_fdn_reverb_cpu.py): a block's one-pole is a matrix product whose cost grows with the square of the block."""
import math

import numpy as np
import pytest
import torch

from tests import fdn_reverb_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTL, FLOOR = R.CTL, R.FLOOR
GRADS = ("gdecay", "gdamping", "gmix")
DECAY = (0.005, 0.3, 3.0, 30.0, 500.0)                    # the first and the last are clamped
DAMPING = (float("inf"), 8000.0, 300.0, -5.0)
INF = float("inf")
BLOCK = 256


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


@pytest.fixture(autouse=True)
def no_device_error_after_any_test():
    yield
    torch.cuda.synchronize()
    assert lib().dasp_device_error() == 0


def draw(sr, C, N, case=0, seed=0):
    """One item per decay_s of DECAY, the dampings of DAMPING paired with them differently from case to case (four cases together hold all
    twenty pairs); x in [-1, 1), w normal, mix 0.2 - 1."""
    B = len(DECAY)
    g = torch.Generator().manual_seed(1000 * seed + 7 * case + 3 * C + N + sr)
    return dict(x=torch.rand(B, C, N, generator=g) * 2 - 1, w=torch.randn(B, C, N, generator=g), decay_s=torch.tensor(DECAY, dtype=torch.float32),
                damping_hz=torch.tensor([DAMPING[(q + case) % 4] for q in range(B)], dtype=torch.float32), mix=torch.rand(B, generator=g) * 0.8 + 0.2)


def plain(B, C, N, seed=0, decay=(0.2, 8.0), damping=(300.0, 20000.0)):
    """Everything inside its range."""
    g = torch.Generator().manual_seed(77 * seed + 7 * B + 3 * C + N)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g), decay_s=torch.exp(u(np.log(decay[0]), np.log(decay[1]), B)),
                damping_hz=u(*damping, B), mix=u(0.2, 1.0, B))


LINES = (149, 211, 263, 331)                               # the lines of the tests that are not about the lines: four primes, 3 - 8 ms at 44.1 kHz


def run_t(D, a, sr, delays=LINES, decorrelate=True, need_gx=True, need_ctl=True):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(need_ctl) for k in CTL]
    y = D.fdn_reverb(x, sr, *ctl, delays, decorrelate)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + (ctl if need_ctl else []))
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + (GRADS if need_ctl else ()), (y.detach(),) + grads))


def restated(a, sr, delays=LINES, decorrelate=True, **kw):
    return R.forward_backward(a["x"], sr, *[a[k] for k in CTL], delays, a["w"], decorrelate, **{"block": BLOCK, **kw})


def check_parity(D, name, a, sr, delays, decorrelate=True):
    want, f32 = restated(a, sr, delays, decorrelate), restated(a, sr, delays, decorrelate, arith=torch.float32)
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, sr, delays, decorrelate).items()}
    e32 = {k: peak_err(f32[k], want[k]) for k in R.NAMES}
    e = {k: peak_err(got[k], want[k]) for k in R.NAMES}
    record(name, **e, **{"fp32_" + k: v for k, v in e32.items()}, **{"share_" + k: e[k] / max(4 * e32[k], FLOOR[k]) for k in R.NAMES})
    for k in R.NAMES:
        assert got[k].shape == want[k].shape, (name, k)
        assert e[k] <= max(4 * e32[k], FLOOR[k]), (name, k, e[k], e32[k])
    d = a["decay_s"].double().numpy()
    clamped = (d < 0.01) | (d > 100.0)
    assert not got["gdecay"][clamped].any() and not want["gdecay"][clamped].any()                # a clamped decay_s: exactly no gradient
    off = ~(a["damping_hz"].numpy() >= 0) | np.isinf(a["damping_hz"].numpy())
    assert not got["gdamping"][off].any() and not want["gdamping"][off].any()                    # damping_hz < 0 or +inf: exactly none
    return got, want


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
CAP = 1024


def delay_sets():
    """name -> (delays, sample rate, decorrelate). K = 1, 2, 5, 8, 16; the five kinds of shortest line: 1, a small odd length, cap - 1 /
    cap / cap + 1, a set at the admissible sum (K = 16: 21504 samples), a set with repeated lengths."""
    L = lib()
    assert L.dasp_fdn_block(1, 10 ** 4) == CAP
    at_sum = [1289 + 7 * i for i in range(15)]
    at_sum.append(L.dasp_fdn_max_delay_sum(16) - sum(at_sum))
    assert sum(at_sum) == L.dasp_fdn_max_delay_sum(16) and min(at_sum) > CAP and max(at_sum) < 1500
    return {
        "one": ((1, 2, 5, 11, 16), 44100, True),
        "odd": ((37, 101), 8000, True),
        "cap-1": ((CAP - 1,), 192000, True),
        "cap": ((CAP, 1061, 1117, 1181, 1237, 1283, 1301, 1361), 44100, True),
        "cap+1": (tuple([CAP + 1] + [1031 + 18 * i for i in range(15)]), 44100, False),
        "sum": (tuple(at_sum), 8000, True),
        "repeat": ((211, 211, 307, 307, 401), 192000, True),
    }


SETS = ("one", "odd", "cap-1", "cap", "cap+1", "sum", "repeat")


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("name", SETS)
def test_parity_with_the_float64_restatement(D, name, which):
    """For each set, with S = dasp_fdn_block(K, shortest): one sample; S - 1, S, S + 1; a length that wraps the shortest and the longest
    ring (m_k + S words) twice plus five. The one-sample-step set has S - 1 = 0 (the empty input has its own test): it runs 300 there."""
    delays, sr, decorrelate = delay_sets()[name]
    S = lib().dasp_fdn_block(len(delays), min(delays))
    assert S == min(min(delays), CAP)
    N = [1, S - 1 if S > 1 else 300, S, S + 1, 2 * (max(delays) + S) + 5][which]
    assert N <= 6000
    C = 2 if which % 2 == 0 else 1
    a = draw(sr, C, N, case=which + SETS.index(name))
    check_parity(D, f"fdn_parity {name} K={len(delays)} sr={sr} (5,{C},{N})", a, sr, delays, decorrelate)


def test_parity_of_a_training_batch(D):
    """(16, 2, 8192) at 44.1 kHz with the default lines: 32 workgroups, eight rings of 1013 - 3659 words plus the step, steps of 1013."""
    delays = D.fdn_delay_lengths(44100)
    a = {k: torch.cat([v] * 4)[:16] for k, v in draw(44100, 2, 8192, case=2).items()}
    g = torch.Generator().manual_seed(11)
    a["x"], a["w"] = torch.rand(16, 2, 8192, generator=g) * 2 - 1, torch.randn(16, 2, 8192, generator=g)
    check_parity(D, "fdn_parity sr=44100 K=8 (16,2,8192)", a, 44100, delays)


# ---- 2. exact identities -----------------------------------------------------------------------------------------------------------------
def test_mix_zero_is_the_identity(D):
    a = plain(4, 2, 5000)
    with torch.no_grad():
        y = D.fdn_reverb(a["x"].to(DEV), 44100, a["decay_s"].to(DEV), a["damping_hz"].to(DEV), torch.zeros(4, device=DEV), LINES)
    assert torch.equal(y.cpu(), a["x"])


@pytest.mark.parametrize("decorrelate", [True, False])
def test_impulse_identity(D, decorrelate):
    """damping_hz = inf, mix = 1, a unit impulse: wet[n] = K^(-1/2) sum over {k : m_k = n} of s_ck for every n < 2 min m_k, bit for bit
    (K^(-1/2) is rounded once; the sum is a small whole number)."""
    delays = (301, 352, 352, 467, 589)
    K, N = len(delays), 2 * min(delays)
    x = torch.zeros(2, 2, N)
    x[..., 0] = 1.0
    t = lambda *v: torch.tensor(v, device=DEV)
    with torch.no_grad():
        y = D.fdn_reverb(x.to(DEV), 44100, t(0.3, 30.0), t(INF, INF), t(1.0, 1.0), delays, decorrelate).cpu()
    count = torch.zeros(2, N)
    for k, m in enumerate(delays):
        if m < N:
            count[:, m] += R.signs(2, K, decorrelate, torch.float32)[:, k]
    want = (np.float32(1.0 / math.sqrt(K)) * count.numpy()).astype(np.float32)
    assert count[1, 352] == (0.0 if decorrelate else 2.0)
    for b in range(2):
        assert np.array_equal(y[b].numpy(), want), b


def test_one_line_against_feedback_delay(D):
    """K = 1 is feedback_delay at a whole-sample delay with feedback = -g: 8 kHz, m = 24 (3 ms exactly). Kernel against kernel, y and
    grad x, within the parity bound of this op (e32 of this restatement)."""
    sr, m = 8000, 24
    a = plain(4, 2, 3000, decay=(0.02, 0.5), damping=(300.0, 3900.0))
    got = run_t(D, a, sr, (m,))
    fb = -R.gains(sr, a["decay_s"], [m])[:, 0].to(torch.float32)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.feedback_delay(x, sr, torch.full((4,), 3.0, device=DEV), fb.to(DEV), a["damping_hz"].to(DEV), a["mix"].to(DEV), max_delay_ms=625.0)
    (gx,) = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [x])
    want, f32 = restated(a, sr, (m,)), restated(a, sr, (m,), arith=torch.float32)
    for k, other in (("y", y.detach()), ("gx", gx)):
        e, e32 = peak_err(got[k].cpu().numpy(), other.cpu().numpy()), peak_err(f32[k], want[k])
        record("fdn_one_line_vs_feedback_delay " + k, err=e, fp32=e32, share=e / max(4 * e32, FLOOR[k]))
        assert e <= max(4 * e32, FLOOR[k]), (k, e, e32)


# ---- 3. adjoint --------------------------------------------------------------------------------------------------------------------------
def test_adjoint(D):
    """The op is linear in x: <y, w> = <x, gx> at mix = 1, both sums taken in float64 on the host from the kernel's float32 outputs. The
    relative difference, the largest over four draws of w, is held to the float32 restatement's own defect by the rule of the parity
    bounds: 4 x it, and never less than the floor of y and grad x, 2e-6."""
    sr = 44100
    a = plain(4, 2, 6000)
    a["mix"] = torch.ones(4)
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
    record("fdn_adjoint", kernel=max(got), restated_fp32=max(want), share=max(got) / max(4 * max(want), 2e-6))
    assert max(got) <= max(4 * max(want), 2e-6), (got, want)


# ---- 4. reproducibility: everything bit for bit ------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(D):
    a = plain(6, 2, 6000)
    p, q = run_t(D, a, 44100), run_t(D, a, 44100)
    for k in R.NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, need_gx=False)                  # x needs no gradient: gx is not written, nothing else changes
    for k in ("y",) + GRADS:
        assert torch.equal(p[k], r[k]), k
    r = run_t(D, a, 44100, need_ctl=False)                 # only x needs one: no line signal is saved, gx comes from the same walk
    for k in ("y", "gx"):
        assert torch.equal(p[k], r[k]), k


def test_item_alone_and_inside_a_batch(D):
    a = plain(5, 2, 5000)
    whole = run_t(D, a, 44100)
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100)
        for k in R.NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path, nothing to zero, and the LDS
    limit of the kernels was raised when the library was loaded."""
    sr = 44100
    a = plain(4, 2, 5000)
    eager = run_t(D, a, sr)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.fdn_reverb(xt, sr, *ctl, LINES)
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


def test_channel_zero_does_not_see_decorrelate(D):
    """s_0k = 1 either way: y and grad x of channel 0 keep every bit, and a mono input every control gradient too."""
    a = plain(3, 2, 5000)
    on, off = run_t(D, a, 44100, decorrelate=True), run_t(D, a, 44100, decorrelate=False)
    for k in ("y", "gx"):
        assert torch.equal(on[k][:, 0], off[k][:, 0]) and not torch.equal(on[k][:, 1], off[k][:, 1]), k
    mono = {k: (v[:, :1].contiguous() if v.dim() == 3 else v) for k, v in a.items()}
    on, off = run_t(D, mono, 44100, decorrelate=True), run_t(D, mono, 44100, decorrelate=False)
    for k in R.NAMES:
        assert torch.equal(on[k], off[k]), k


# ---- 5. off the nominal domain -----------------------------------------------------------------------------------------------------------
def _item0_unchanged(clean, dirty):
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e30])
def test_poisoned_audio_and_controls_stay_in_their_item(D, value):
    a = plain(2, 2, 4000)
    clean = run_t(D, a, 44100)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    for k in CTL:
        b[k][1] = float("nan")
    dirty = run_t(D, b, 44100)
    _item0_unchanged(clean, dirty)
    assert torch.isnan(dirty["y"][1]).all() and torch.isnan(dirty["gx"][1]).all() and all(torch.isnan(dirty[k][1]) for k in GRADS)
    torch.cuda.synchronize()
    assert lib().dasp_device_error() == 0


@pytest.mark.parametrize("ctl", CTL)
def test_one_nan_control_gives_a_nan_item(D, ctl):
    """A NaN passes the clamps. It reaches exactly what the sample loop with the hand adjoint says it reaches - y from the first echo on
    (all of it for a NaN mix), grad x up to the last sample that still echoes, its own gradient and the others' (the mix gradient
    sum gy (wet - x) holds no term with mix and stays finite under a NaN mix) - and nothing of the items beside it. (Autograd of the
    restatement is no yardstick here: it multiplies a NaN gain with the zero gradients it makes up for samples that echo no more.)"""
    a = plain(3, 2, 1500)
    clean = run_t(D, a, 44100)
    a[ctl][1] = float("nan")
    dirty = run_t(D, a, 44100)
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
    want = R.direct(a["x"][1:2].numpy(), 44100, *[a[k][1:2].numpy() for k in CTL], LINES, a["w"][1:2].numpy())
    want = {k: np.concatenate([v, v]) for k, v in want.items()}              # (item 1 stands at index 1 as in the kernel's results)
    for k in R.NAMES:
        assert np.array_equal(torch.isnan(dirty[k][1]).cpu().numpy(), np.isnan(want[k][1])), (ctl, k)
    assert torch.isnan(dirty["y"][1]).any() and torch.isnan(dirty["gx"][1]).any() and torch.isnan(dirty["gdecay"][1])
    assert torch.isnan(dirty["g" + ctl.split("_")[0]][1]) or ctl == "mix"


def test_poisoned_upstream_gradient_stays_in_its_item(D):
    a = plain(2, 2, 4000)
    clean = run_t(D, a, 44100)
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = float("nan")
    dirty = run_t(D, b, 44100)
    _item0_unchanged(clean, dirty)
    assert torch.equal(clean["y"], dirty["y"]) and all(torch.isnan(dirty[k][1]) for k in GRADS)
    assert lib().dasp_device_error() == 0


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["x", "w"])
def test_one_bad_sample_reaches_what_the_restatement_says(D, where, value):
    """One NaN or +inf in the middle of row (0, 0): in x, the isfinite mask of y equals the float64 restatement's (the sample stays in the
    lines: every echo after it); in the upstream gradient, that of grad x does (every sample that echoes into it)."""
    a = plain(2, 2, 2000)
    a[where][0, 0, 1000] = value
    got, want = run_t(D, a, 44100), restated(a, 44100, block=1)                  # (a wider block is a matrix product: 0 x inf)
    key = "y" if where == "x" else "gx"
    mask = torch.isfinite(got[key]).cpu().numpy()
    assert np.array_equal(mask, np.isfinite(want[key])) and 0 < (~mask).sum() < mask.size // 2


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    a = plain(3, 2, 2500)
    want = run_t(D, a, 44100)
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
    y = D.fdn_reverb(xv, 44100, *ctl, LINES)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    for k, g in zip(R.NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_and_ignores_dirty_scratch(D):
    """Through the C ABI: y, v, gx, gctl and the partials written inside NaN-filled guard words leave the guards NaN, a NaN-filled
    partials buffer gives the same bits as a zero-filled one, v = NULL in forward changes nothing else, and backward with v = NULL
    writes the same gx and nothing else."""
    import ctypes

    from dasp_pytorch_amd._lib import call, ptr, stream
    sr, G = 44100, 64
    B, C, N, K = 3, 2, 4333, len(LINES)
    a = plain(B, C, N)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    ctl = torch.stack([a[k] for k in CTL], -1).contiguous().to(DEV)
    lines = (ctypes.c_int * K)(*LINES)
    npart = lib().dasp_fdn_partial_floats(B * C)
    assert npart == 18 * B * C

    def guarded(n, fill=float("nan")):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        buf[G:G + n] = fill
        return buf, buf[G:G + n]

    def run(fill, lean=False):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("v", B * C * K * N), ("gx", B * C * N), ("gctl", B * 3))}
        bufs["partials"] = guarded(npart, fill)
        call("dasp_fdn_forward", ptr(x), ptr(ctl), lines, ptr(bufs["y"][1]), ptr(None if lean else bufs["v"][1]), B, C, N, K, float(sr), 1, stream())
        call("dasp_fdn_backward", ptr(x), ptr(ctl), lines, ptr(None if lean else bufs["v"][1]), ptr(gy), ptr(bufs["gx"][1]), ptr(bufs["gctl"][1]),
             ptr(bufs["partials"][1]), B, C, N, K, float(sr), 1, stream())
        torch.cuda.synchronize()
        untouched = ("v", "gctl") if lean else ()
        for k, (buf, inner) in bufs.items():
            assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
            if k in untouched:
                assert torch.isnan(inner).all(), k
            elif k == "partials":
                assert lean or torch.isfinite(inner.view(B * C, 18)[:, list(range(K)) + [16, 17]]).all()
            else:
                assert torch.isfinite(inner).all(), k
        return {k: inner.clone() for k, (buf, inner) in bufs.items()}

    zero, dirty, lean = run(0.0), run(float("nan")), run(0.0, lean=True)
    for k in ("y", "v", "gx", "gctl"):
        assert torch.equal(zero[k], dirty[k]), k
    used = list(range(K)) + [16, 17]
    assert torch.equal(zero["partials"].view(-1, 18)[:, used], dirty["partials"].view(-1, 18)[:, used])
    for k in ("y", "gx"):
        assert torch.equal(zero[k], lean[k]), k
    assert not lean["partials"].any()                       # zero-filled and left alone
    ref = run_t(D, a, sr)
    assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"])
    for q, k in enumerate(GRADS):
        assert torch.equal(zero["gctl"].view(B, 3)[:, q], ref[k]), k
    assert lib().dasp_device_error() == 0


def test_silence_in_silence_out(D):
    a = plain(2, 2, 4000)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS)


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        ctl = [torch.ones(B, device=DEV, requires_grad=True) for _ in range(3)]
        y = D.fdn_reverb(x, 44100, *ctl, LINES)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


def test_too_many_samples_of_delay_are_refused_on_the_host(D):
    from dasp_pytorch_amd import _lib
    x = torch.zeros(1, 1, 64, device=DEV)
    limit = lib().dasp_fdn_max_delay_sum(8)
    ctl = [torch.ones(1, device=DEV) for _ in range(3)]
    with pytest.raises(_lib.DaspHipError, match="unsupported"):
        D.fdn_reverb(x, 44100, *ctl, [limit // 8 + 1] * 8)
    with pytest.raises(_lib.DaspHipError, match="unsupported"):
        D.fdn_reverb(x, 192000, *ctl, D.fdn_delay_lengths(192000))
    y = D.fdn_reverb(x, 44100, *ctl, [limit // 8] * 8)      # at the sum: runs
    torch.cuda.synchronize()
    assert torch.equal(y, x) and lib().dasp_device_error() == 0


# ---- 6. double backward ------------------------------------------------------------------------------------------------------------------
def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.fdn_reverb(x, 44100, *[a[k].to(DEV) for k in CTL], LINES)
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 7. module ---------------------------------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    sr = 44100
    x = plain(3, 2, 3000)["x"].to(DEV)
    p = torch.rand(3, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    lo = torch.tensor([0.1, 500.0, 0.0], device=DEV)
    span = torch.tensor([9.9, 19500.0, 1.0], device=DEV)
    for m, lines, dec in ((D.FDNReverb(sr), tuple(D.fdn_delay_lengths(sr)), True), (D.FDNReverb(sr, delays=LINES, decorrelate=False), LINES, False)):
        with torch.no_grad():
            got = m.process_normalized(x, p)
            d = p * span + lo
            want = D.fdn_reverb(x, sr, d[:, 0], d[:, 1], d[:, 2], lines, dec)
        assert torch.equal(got, want)
