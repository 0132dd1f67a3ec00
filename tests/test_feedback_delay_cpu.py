"""Host-side checks of feedback_delay (no GPU): the restatement (tests/feedback_delay_restated.py) against a sample-by-sample double loop
whose adjoint is written out by hand, the closed form of an undamped whole-sample echo, what float32 arithmetic costs (the yardstick e32
of the GPU tests), the size queries and argument checks of the C ABI, the errors of the Python layer and modules.FeedbackDelay."""
import inspect

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import feedback_delay_restated as R


def peak_err(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ds", [(2.0, 2.5), (3.999, 17.0), (40.3, 17.0), (1.0, 60.0)])
def test_restatement_equals_the_direct_loop(Ds):
    """(2, 2, 300) at 8 kHz, one D per item; (1.0, 60.0) is clamped at either end (max 50 samples): no delay_ms gradient there. The
    second item's damping is negative in the last case and +inf in the first: no damping_hz gradient. Both sides are float64 and agree
    to rounding, 1e-11 of each quantity's peak (the loop is a recurrence 300 samples long with feedback up to 0.9)."""
    g = torch.Generator().manual_seed(int(10 * sum(Ds)))
    bs, chs, N, sr, mdm = 2, 2, 300, 8000, 6.25
    x, gy = torch.randn(bs, chs, N, generator=g), torch.randn(bs, chs, N, generator=g)
    delay = torch.tensor(Ds, dtype=torch.float64) / (sr / 1000.0)
    fb = torch.tensor([0.9, -0.7], dtype=torch.float64)
    damp = torch.tensor([900.0, float("inf") if Ds[0] == 2.0 else (-5.0 if Ds[0] == 1.0 else 2500.0)], dtype=torch.float64)
    mix = torch.tensor([0.3, 0.8], dtype=torch.float64)
    a = R.forward_backward(x, sr, delay, fb, damp, mix, gy, max_delay_ms=mdm, block=7)
    b = R.direct(x.numpy(), sr, delay.numpy(), fb.numpy(), damp.numpy(), mix.numpy(), gy.numpy(), max_delay_ms=mdm)
    for k in R.NAMES:
        assert a[k].shape == b[k].shape, k
        assert np.abs(a[k] - b[k]).max() <= 1e-11 * np.abs(b[k]).max(), (k, a[k], b[k])
    if Ds[0] == 1.0:
        assert not a["gdelay"].any() and not b["gdelay"].any() and a["gdamping"][1] == 0 and b["gdamping"][1] == 0
    if Ds[0] == 2.0:
        assert a["gdamping"][1] == 0 and b["gdamping"][1] == 0 and a["gdamping"][0] != 0


def test_block_length_does_not_matter():
    """Any block of at most L samples gives the same float64 result to rounding."""
    g = torch.Generator().manual_seed(3)
    x, gy = torch.randn(2, 1, 500, generator=g), torch.randn(2, 1, 500, generator=g)
    ctl = (torch.tensor([5.04, 11.3]), torch.tensor([0.8, -0.9]), torch.tensor([3000.0, 500.0]), torch.tensor([0.5, 1.0]))
    a, b = R.forward_backward(x, 8000, *ctl, gy, max_delay_ms=20.0, block=512), R.forward_backward(x, 8000, *ctl, gy, max_delay_ms=20.0, block=3)
    for k in R.NAMES:
        assert peak_err(a[k], b[k]) < 1e-12, k


def test_undamped_whole_sample_echo_is_a_geometric_train():
    """Integer D, no damping, an impulse in: r is feedback^(k-1) at n = k D and zero elsewhere."""
    sr, Dn, N, fb = 8000, 24, 200, -0.8
    x = torch.zeros(1, 1, N, dtype=torch.float64)
    x[0, 0, 0] = 1.0
    one = lambda v: torch.tensor([v], dtype=torch.float64)
    y = R.forward(x, sr, one(Dn / 8.0), one(fb), one(float("inf")), one(1.0), max_delay_ms=10.0)[0, 0]
    want = torch.zeros(N, dtype=torch.float64)
    for k in range(1, N // Dn + 1):
        if k * Dn < N:
            want[k * Dn] = fb ** (k - 1)
    assert torch.allclose(y, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("Dv", [2.0, 2.5, 3.999, 88.3, 441.7, 11025.5])
def test_float32_arithmetic_stays_below_1e_5_of_the_peak(Dv):
    """e32, the yardstick of the GPU tests: float64 D and float32 arithmetic against float64 throughout, for |feedback| <= 0.98 with and
    without damping. Below 1e-5 of the peak of y and of grad x (N = 20000 for the long delays, 3000 for the sample-by-sample ones)."""
    sr = 44100
    N = 20000 if Dv > 4 else 3000
    g = torch.Generator().manual_seed(int(Dv * 10))
    fbs = torch.tensor([0.9, -0.9, 0.98, 0.98, -0.9, 0.9])
    damp = torch.tensor([float("inf"), float("inf"), float("inf"), 4865.0, 4865.0, 4865.0])          # a = 0 and a = 0.5
    bs = fbs.numel()
    x, gy = torch.rand(bs, 1, N, generator=g) * 2 - 1, torch.randn(bs, 1, N, generator=g)
    ctl = (torch.full((bs,), Dv / 44.1, dtype=torch.float64), fbs, damp, torch.full((bs,), 0.7))
    ref = R.forward_backward(x, sr, *ctl, gy, max_delay_ms=300.0)
    f32 = R.forward_backward(x, sr, *ctl, gy, max_delay_ms=300.0, arith=torch.float32)
    for k in ("y", "gx"):
        assert peak_err(f32[k], ref[k]) < 1e-5, (k, peak_err(f32[k], ref[k]))


def test_catmull_rom_weights_and_derivatives():
    f = torch.linspace(0, 1, 101, dtype=torch.float64, requires_grad=True)
    w = torch.stack(R.weights(f), -1)
    assert torch.allclose(w.sum(-1), torch.ones_like(f), atol=1e-15)
    for k, dw in enumerate(R.dweights(f.detach())):
        assert torch.allclose(torch.autograd.grad(w[:, k].sum(), f, retain_graph=True)[0], dw, atol=1e-14)
    assert [float(abs(v)) for v in R.weights(torch.zeros((), dtype=torch.float64))] == [0.0, 1.0, 0.0, 0.0]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    hmax = L.dasp_fbdelay_max_delay_samples()
    assert hmax >= 32768
    for H in (2, 3, 441, 22050, hmax):
        for lag in sorted({1, min(2, H - 1), min(255, H - 1), min(256, H - 1), min(2048, H - 1), H - 1}):
            S = L.dasp_fbdelay_block(H, lag)
            assert 1 <= S <= lag and S == min(lag, 2048), (H, lag, S)
            assert (H + 2 + S) * 4 + 1024 <= 160 * 1024                          # the ring and the static words inside a workgroup's 160 KiB
        assert L.dasp_fbdelay_block(H, 0) == -1 and L.dasp_fbdelay_block(H, H) == -1
        for rows in (1, 3, 128):
            for N in (1, 1000, 131072):
                assert L.dasp_fbdelay_partial_floats(rows, N, H) == 4 * rows
    assert L.dasp_fbdelay_block(1, 1) == -1 and L.dasp_fbdelay_block(hmax + 1, 5) == -2
    assert L.dasp_fbdelay_partial_floats(0, 10, 100) == -1 and L.dasp_fbdelay_partial_floats(4, 0, 100) == -1
    assert L.dasp_fbdelay_partial_floats(4, 10, 1) == -1 and L.dasp_fbdelay_partial_floats(4, 10, hmax + 1) == -2


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers and impossible sizes, DASP_ERR_UNSUPPORTED (-2) for an H beyond the limit and a grid beyond 2^31
    rows - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, H=1764, sr=44100.0, mdm=40.0)

    def fwd(x=f, ctl=f, y=f, v=f, **kw):
        a = {**ok, **kw}
        return L.dasp_fbdelay_forward(x, ctl, y, v, a["B"], a["C"], a["N"], a["H"], a["sr"], a["mdm"], None)

    def bwd(x=f, ctl=f, v=f, gy=f, gx=f, gctl=f, part=f, **kw):
        a = {**ok, **kw}
        return L.dasp_fbdelay_backward(x, ctl, v, gy, gx, gctl, part, a["B"], a["C"], a["N"], a["H"], a["sr"], a["mdm"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(ctl=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1 and call(H=0) == -1 and call(H=1) == -1
        assert call(H=1763) == -1                                            # H below sr/1000 max_delay_ms = 1764
        assert call(H=2, mdm=0.04) == -1                                     # fewer than two samples of delay at the most
        assert call(sr=0.0) == -1 and call(sr=float("nan")) == -1 and call(sr=float("inf")) == -1
        assert call(mdm=-1.0) == -1 and call(mdm=float("nan")) == -1 and call(mdm=float("inf")) == -1
        assert call(H=L.dasp_fbdelay_max_delay_samples() + 1) == -2
        assert call(B=1 << 16, C=1 << 16) == -2
    assert fwd(y=None) == -1
    assert bwd(v=None) == -1 and bwd(gy=None) == -1 and bwd(gctl=None) == -1 and bwd(part=None) == -1


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def _controls(bs):
    return [torch.full((bs,), 100.0), torch.full((bs,), 0.5), torch.full((bs,), 4000.0), torch.full((bs,), 0.5)]


@pytest.mark.parametrize("which,name", enumerate(("delay_ms", "feedback", "damping_hz", "mix")))
def test_wrong_control_count_names_the_control(which, name):
    ctl = _controls(2)
    ctl[which] = torch.zeros(5)
    with pytest.raises(RuntimeError, match=name):
        D.feedback_delay(torch.zeros(2, 2, 64), 44100, *ctl)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.feedback_delay(torch.zeros(2, 2, 64), 44100, *_controls(2))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.FeedbackDelay(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 4), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="feedback_delay: float64"):
        D.feedback_delay(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2))


def test_bad_scalars_raise_value_error():
    x = torch.zeros(1, 1, 8)
    for kw in (dict(max_delay_ms=-1.0), dict(max_delay_ms=float("nan")), dict(max_delay_ms=float("inf")), dict(max_delay_ms=0.04)):
        with pytest.raises(ValueError, match="feedback_delay"):
            D.feedback_delay(x, 44100, *_controls(1), **kw)
    for sr in (0, -8000, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="feedback_delay"):
            D.feedback_delay(x, sr, *_controls(1))


def test_module_tables_and_plumbing():
    names = list(inspect.signature(D.functional.feedback_delay).parameters)
    assert names == ["x", "sample_rate", "delay_ms", "feedback", "damping_hz", "mix", "max_delay_ms"]
    m = D.FeedbackDelay(44100)
    assert m.num_params == 4 and list(m.param_ranges) == names[2:6]
    assert m.param_ranges == {"delay_ms": (1.0, 500.0), "feedback": (0.0, 0.95), "damping_hz": (200.0, 20000.0), "mix": (0.0, 1.0)}
    assert m.max_delay_ms == 500.0 and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.feedback_delay and m.process_fn.keywords == {"max_delay_ms": 500.0}
    m = D.FeedbackDelay(48000, min_delay_ms=10.0, max_delay_ms=120.0, max_feedback=0.5)
    assert m.max_delay_ms == 120.0 and m.process_fn.keywords == {"max_delay_ms": 120.0}
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    p = torch.rand(3, 4, generator=torch.Generator().manual_seed(0))
    x = torch.zeros(3, 2, 16)
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and list(seen)[:4] == names[2:6]
    assert torch.allclose(seen["delay_ms"], p[:, 0] * 110 + 10) and torch.allclose(seen["feedback"], p[:, 1] * 0.5)
    assert torch.allclose(seen["damping_hz"], p[:, 2] * 19800 + 200) and torch.allclose(seen["mix"], p[:, 3])
    with pytest.raises(ValueError):
        m.process_normalized(x, torch.rand(3, 5))
    assert D.feedback_delay is D.functional.feedback_delay and D.FeedbackDelay is D.modules.FeedbackDelay
