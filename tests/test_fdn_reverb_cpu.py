"""Host-side checks of fdn_reverb (no GPU): the restatement (tests/fdn_reverb_restated.py) against a sample-by-sample double loop whose
adjoint is written out by hand, one line against the feedback_delay restatement, the impulse identity, the exactly-zero gradients of
clamped controls, signal.fdn_delay_lengths, the errors of the Python layer, the size queries and argument checks of the C ABI and
modules.FDNReverb."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import fdn_reverb_restated as R
from tests import feedback_delay_restated as FB

INF = float("inf")
t64 = lambda *v: torch.tensor(v, dtype=torch.float64)


def peak_err(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delays,decorrelate", [((7,), True), ((5, 9), True), ((5, 9), False), ((3, 7, 11, 13, 17), True), ((4, 6, 6, 9, 9), False),
                                                ((1, 4, 6), True)])
def test_restatement_equals_the_direct_loop(delays, decorrelate):
    """(2, 2, 160) at 8 kHz: K = 1, 2, 5, both decorrelate settings with two channels, a repeated length, a shortest line of 1. decay_s
    of 20 and 50 ms (g from 0.2 to 0.98 over these lines), one damped and one not. Both sides are float64 and agree to rounding, 1e-11
    of each quantity's peak."""
    g = torch.Generator().manual_seed(sum(delays) + len(delays))
    bs, chs, N, sr = 2, 2, 160, 8000
    x, gy = torch.randn(bs, chs, N, generator=g, dtype=torch.float64), torch.randn(bs, chs, N, generator=g, dtype=torch.float64)
    ctl = (t64(0.02, 0.05), t64(900.0, 2500.0), t64(0.3, 0.8))
    a = R.forward_backward(x, sr, *ctl, delays, gy, decorrelate, block=4)
    b = R.direct(x.numpy(), sr, *[c.numpy() for c in ctl], delays, gy.numpy(), decorrelate)
    for k in R.NAMES:
        assert a[k].shape == b[k].shape, k
        assert np.abs(b[k]).max() > 0 and np.abs(a[k] - b[k]).max() <= 1e-11 * np.abs(b[k]).max(), (k, a[k], b[k])


def test_block_length_does_not_matter():
    g = torch.Generator().manual_seed(3)
    x, gy = torch.randn(2, 2, 400, generator=g), torch.randn(2, 2, 400, generator=g)
    ctl = (t64(0.3, 3.0), t64(3000.0, 500.0), t64(0.5, 1.0))
    a, b = R.forward_backward(x, 8000, *ctl, (11, 17, 23), gy, block=512), R.forward_backward(x, 8000, *ctl, (11, 17, 23), gy, block=1)
    for k in R.NAMES:
        assert peak_err(a[k], b[k]) < 1e-12, k


@pytest.mark.parametrize("m", [2, 24])
def test_one_line_is_feedback_delay_with_negative_feedback(m):
    """K = 1: the matrix is -1, so the line is feedback_delay at a whole-sample delay m >= 2 with feedback = -g. y and gx."""
    g = torch.Generator().manual_seed(m)
    sr, N = 8000, 300
    x, gy = torch.randn(2, 2, N, generator=g, dtype=torch.float64), torch.randn(2, 2, N, generator=g, dtype=torch.float64)
    decay, damp, mix = t64(0.05, 0.3), t64(900.0, INF), t64(0.3, 0.8)
    gain = R.gains(sr, decay, [m])[:, 0]
    a = R.forward_backward(x, sr, decay, damp, mix, [m], gy)
    b = FB.forward_backward(x, sr, torch.full((2,), m / 8.0, dtype=torch.float64), -gain, damp, mix, gy, max_delay_ms=10.0)
    for k in ("y", "gx"):
        assert peak_err(a[k], b[k]) < 1e-13, k


@pytest.mark.parametrize("decorrelate", [True, False])
def test_impulse_identity(decorrelate):
    """damping_hz = inf, mix = 1, a unit impulse: wet[n] = K^(-1/2) sum over {k : m_k = n} of s_ck for every n < 2 min m_k."""
    delays = (9, 11, 11, 14, 17)
    K, N = len(delays), 2 * min(delays)
    x = torch.zeros(1, 2, N, dtype=torch.float64)
    x[..., 0] = 1.0
    y = R.forward(x, 8000, t64(1.0), t64(INF), t64(1.0), delays, decorrelate)
    s = R.signs(2, K, decorrelate)
    want = torch.zeros(2, N, dtype=torch.float64)
    for k, m in enumerate(delays):
        if m < N:
            want[:, m] += s[:, k]
    assert torch.allclose(y[0], want / math.sqrt(K), rtol=0, atol=1e-15)
    assert want[1, 11] == (0.0 if decorrelate else 2.0)


def test_clamped_controls_have_exactly_no_gradient():
    """decay_s of 0.001 and 1000 (clamped to 0.01 and 100) and damping_hz of -5 and inf: zero, in the restatement and in the direct loop."""
    g = torch.Generator().manual_seed(5)
    x, gy = torch.randn(2, 1, 120, generator=g, dtype=torch.float64), torch.randn(2, 1, 120, generator=g, dtype=torch.float64)
    ctl = (t64(0.001, 1000.0), t64(-5.0, INF), t64(0.4, 0.9))
    a = R.forward_backward(x, 8000, *ctl, (5, 8), gy)
    b = R.direct(x.numpy(), 8000, *[c.numpy() for c in ctl], (5, 8), gy.numpy())
    for r in (a, b):
        assert not r["gdecay"].any() and not r["gdamping"].any() and r["gmix"].all() and r["gx"].any()
    inside = R.forward_backward(x, 8000, t64(0.02, 50.0), t64(100.0, 3000.0), ctl[2], (5, 8), gy)
    assert inside["gdecay"].all() and inside["gdamping"].all()


@pytest.mark.parametrize("decay", [0.3, 3.0, 30.0])
def test_float32_arithmetic_stays_below_1e_5_of_the_peak(decay):
    """e32, the yardstick of the GPU tests, at the default delay set of 8 kHz over 6000 samples, with and without damping."""
    g = torch.Generator().manual_seed(int(decay * 10))
    sr, N, delays = 8000, 6000, D.fdn_delay_lengths(8000)
    x, gy = torch.rand(2, 1, N, generator=g) * 2 - 1, torch.randn(2, 1, N, generator=g)
    ctl = (t64(decay, decay), t64(INF, 2000.0), t64(0.7, 0.7))
    ref = R.forward_backward(x, sr, *ctl, delays, gy)
    f32 = R.forward_backward(x, sr, *ctl, delays, gy, arith=torch.float32)
    for k in ("y", "gx"):
        assert peak_err(f32[k], ref[k]) < 1e-5, (k, peak_err(f32[k], ref[k]))


# ---- signal.fdn_delay_lengths ------------------------------------------------------------------------------------------------------------
def _prime(n):
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


@pytest.mark.parametrize("sr", [8000, 44100, 192000])
@pytest.mark.parametrize("lines", [1, 8, 16])
def test_delay_lengths_are_distinct_ascending_primes(sr, lines):
    m = D.signal.fdn_delay_lengths(sr, lines)
    assert len(m) == lines and all(isinstance(v, int) and _prime(v) for v in m)
    assert all(p < q for p, q in zip(m, m[1:]))
    lo, hi = sr / 1000.0 * 23.0, sr / 1000.0 * 83.0
    assert abs(m[0] - lo) <= 0.01 * lo + 2 and (lines == 1 or abs(m[-1] - hi) <= 0.01 * hi + 2)
    if lines > 2:                                                            # logarithmic: the ratios of neighbours agree to a few percent
        ratios = [q / p for p, q in zip(m, m[1:])]
        assert max(ratios) / min(ratios) < 1.1


def test_delay_lengths_collisions_and_arguments():
    m = D.signal.fdn_delay_lengths(1000, 8, 5.0, 9.0)                        # eight points between 5 and 9: collisions move on to free primes
    assert m == sorted(set(m)) and len(m) == 8 and all(_prime(v) for v in m) and m[0] == 5
    assert D.signal.fdn_delay_lengths(44100) == D.signal.fdn_delay_lengths(44100, 8, 23.0, 83.0) and D.fdn_delay_lengths is D.signal.fdn_delay_lengths
    for kw in (dict(sample_rate=0), dict(sample_rate=INF), dict(sample_rate=float("nan")), dict(lines=0), dict(lines=17), dict(lines=True),
               dict(lines=2.0), dict(shortest_ms=0.0), dict(shortest_ms=90.0), dict(longest_ms=INF)):
        with pytest.raises(ValueError):
            D.signal.fdn_delay_lengths(**{"sample_rate": 44100, **kw})


# ---- the Python layer: every refusal comes before a device is needed ---------------------------------------------------------------------
def _controls(bs):
    return [torch.full((bs,), 1.0), torch.full((bs,), 4000.0), torch.full((bs,), 0.5)]


@pytest.mark.parametrize("which,name", enumerate(("decay_s", "damping_hz", "mix")))
def test_wrong_control_count_names_the_control(which, name):
    ctl = _controls(2)
    ctl[which] = torch.zeros(5)
    with pytest.raises(RuntimeError, match=name):
        D.fdn_reverb(torch.zeros(2, 2, 64), 44100, *ctl, (5, 7))


@pytest.mark.parametrize("delays", [(), tuple(range(1, 18)), (5, 0), (5, -3), (5, True), (5, 7.0), (5, "7"), 7, "57", torch.tensor([5, 7]), None])
def test_bad_delays_raise_value_error(delays):
    with pytest.raises(ValueError, match="delays"):
        D.fdn_reverb(torch.zeros(1, 1, 8), 44100, *_controls(1), delays)


@pytest.mark.parametrize("sr", [0, -8000, float("nan"), INF])
def test_bad_sample_rate_raises_value_error(sr):
    with pytest.raises(ValueError, match="fdn_reverb"):
        D.fdn_reverb(torch.zeros(1, 1, 8), sr, *_controls(1), (5, 7))


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.fdn_reverb(torch.zeros(2, 2, 64), 44100, *_controls(2), [5, 7])
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.FDNReverb(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 3), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="fdn_reverb: float64"):
        D.fdn_reverb(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2), (5, 7))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    assert L.dasp_fdn_max_lines() == 16
    cap = L.dasp_fdn_block(1, 10 ** 4)
    assert cap == 1024
    for K in (1, 2, 5, 8, 16):
        limit = L.dasp_fdn_max_delay_sum(K)
        assert (limit + (K + 1) * cap) * 4 + 4096 <= 160 * 1024             # the rings, the staged step and the static words inside 160 KiB
        for shortest in (1, 2, 255, 256, 257, cap - 1, cap, cap + 1, limit // K):
            S = L.dasp_fdn_block(K, shortest)
            assert S == min(shortest, cap), (K, shortest, S)
        assert L.dasp_fdn_block(K, limit // K + 1) == -2 and L.dasp_fdn_block(K, 0) == -1
    assert L.dasp_fdn_max_delay_sum(8) >= 24000                              # eight lines of 0.54 s at 44.1 kHz together
    assert L.dasp_fdn_max_delay_sum(8) > L.dasp_fdn_max_delay_sum(16) > 16 * cap
    assert sum(D.fdn_delay_lengths(44100)) <= L.dasp_fdn_max_delay_sum(8) and sum(D.fdn_delay_lengths(48000)) <= L.dasp_fdn_max_delay_sum(8)
    for bad in (0, 17, -1):
        assert L.dasp_fdn_max_delay_sum(bad) == -1 and L.dasp_fdn_block(bad, 100) == -1
    assert [L.dasp_fdn_partial_floats(r) for r in (1, 3, 128)] == [18, 54, 2304] and L.dasp_fdn_partial_floats(0) == -1


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, K outside 1 .. 16, a line shorter than one sample and a bad sample rate; DASP_ERR_UNSUPPORTED
    (-2) for lines beyond the sum limit and a grid beyond 2^31 rows - all before any launch. The non-null device pointers are fakes, never
    read; the delays are host memory."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, sr=44100.0, delays=(1013, 1217, 1459), dec=1)
    ints = lambda d: None if d is None else (ctypes.c_int * max(len(d), 1))(*d)

    def fwd(x=f, ctl=f, y=f, v=f, **kw):
        a = {**ok, **kw}
        return L.dasp_fdn_forward(x, ctl, ints(a["delays"]), y, v, a["B"], a["C"], a["N"], a.get("K", len(a["delays"] or ())), a["sr"], a["dec"], None)

    def bwd(x=f, ctl=f, v=f, gy=f, gx=f, gctl=f, part=f, **kw):
        a = {**ok, **kw}
        return L.dasp_fdn_backward(x, ctl, ints(a["delays"]), v, gy, gx, gctl, part, a["B"], a["C"], a["N"], a.get("K", len(a["delays"] or ())), a["sr"],
                                   a["dec"], None)

    limit = L.dasp_fdn_max_delay_sum(3)
    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(ctl=None) == -1 and call(delays=None, K=3) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1
        assert call(K=0) == -1 and call(K=17) == -1 and call(delays=(5,) * 17) == -1
        assert call(delays=(5, 0, 7)) == -1 and call(delays=(5, -4, 7)) == -1
        assert call(sr=0.0) == -1 and call(sr=-1.0) == -1 and call(sr=float("nan")) == -1 and call(sr=INF) == -1
        assert call(delays=(limit - 10, 5, 6)) == -2 and call(delays=(limit // 3 + 1,) * 3) == -2
        assert call(B=1 << 16, C=1 << 16) == -2
    assert fwd(y=None) == -1
    assert bwd(gy=None) == -1 and bwd(gctl=None) == -1 and bwd(part=None) == -1
    assert bwd(v=None, gx=None) == -1                                       # gx alone is what a call without the saved v is for


# ---- the module --------------------------------------------------------------------------------------------------------------------------
def test_module_tables_and_plumbing():
    names = list(inspect.signature(D.functional.fdn_reverb).parameters)
    assert names == ["x", "sample_rate", "decay_s", "damping_hz", "mix", "delays", "decorrelate"]
    m = D.FDNReverb(44100)
    assert m.num_params == 3 and list(m.param_ranges) == names[2:5]
    assert m.param_ranges == {"decay_s": (0.1, 10.0), "damping_hz": (500.0, 20000.0), "mix": (0.0, 1.0)}
    assert m.delays == tuple(D.fdn_delay_lengths(44100)) and m.decorrelate is True and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.fdn_reverb and m.process_fn.keywords == {"delays": m.delays, "decorrelate": True}
    m = D.FDNReverb(48000, delays=[101, 211, 211], decorrelate=False, max_decay_s=4.0)
    assert m.delays == (101, 211, 211) and m.process_fn.keywords == {"delays": (101, 211, 211), "decorrelate": False}
    with pytest.raises(ValueError, match="delays"):
        D.FDNReverb(48000, delays=[101, 0])
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    p = torch.rand(3, 3, generator=torch.Generator().manual_seed(0))
    x = torch.zeros(3, 2, 16)
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and list(seen)[:3] == names[2:5]
    assert torch.allclose(seen["decay_s"], p[:, 0] * 3.9 + 0.1) and torch.allclose(seen["damping_hz"], p[:, 1] * 19500 + 500)
    assert torch.allclose(seen["mix"], p[:, 2])
    with pytest.raises(ValueError):
        m.process_normalized(x, torch.rand(3, 4))
    assert D.fdn_reverb is D.functional.fdn_reverb and D.FDNReverb is D.modules.FDNReverb
