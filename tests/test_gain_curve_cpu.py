"""gain_curve without a GPU: the hand-written adjoint and frame_gradients against autograd, the condition on the parity cases of the
GPU tests, where a NaN frame value reaches, the argument errors raised before the device is asked for, the C entry points' refusals and
the GainCurve module's parameter tensor."""
import inspect

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import control_rate_cases as K
from tests import gain_curve_restated as R


@pytest.mark.parametrize("hop,chs,N", [(8, 1, 7), (8, 2, 8), (8, 3, 203), (64, 2, 64), (64, 2, 65), (64, 1, 700), (2048, 2, 2100)])
def test_adjoint_by_hand_and_frame_gradients_against_autograd(hop, chs, N):
    b = K.gain_curve_inputs(hop, chs, N, seed=5)
    want = R.forward_backward(b["x"], 44100, b["gain_db"], b["w"], hop)
    gx, gP = R.adjoint_by_hand(b["x"], b["gain_db"], b["w"], hop)
    assert K.per_item_err(gx, want["gx"]) <= 1e-13 and K.per_item_err(gP, want["ggain"]) <= 1e-12
    # frame_gradients alone: the adjoint of the interpolation, against autograd of a linear functional of the interpolated curve
    P = b["gain_db"].double().requires_grad_(True)
    gs = torch.randn(K.BS, N, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (g,) = torch.autograd.grad((R.interpolate(P, N, hop) * gs).sum(), P)
    assert np.abs(R.frame_gradients(gs.numpy(), hop, P.shape[1]) - g.numpy()).max() <= 1e-13 * np.abs(g.numpy()).max()


def test_the_last_frame_value_has_a_gradient_unless_the_last_sample_sits_on_a_frame_point():
    """Frame point F - 1 lies at or after sample N. With N = k hop + 1 the last sample sits on frame point F - 2 (t = 0) and the last
    frame value takes nothing: its gradient is exactly 0. With N = k hop the last interval holds t up to (hop - 1) / hop, and the last
    frame value, which sits at sample N itself, takes its share."""
    hop = 8
    for N, zero in ((17, True), (16, False), (9, True), (8, False)):
        b = K.gain_curve_inputs(hop, 2, N, seed=1)
        g = R.forward_backward(b["x"], 44100, b["gain_db"], b["w"], hop)["ggain"]
        assert ((g[:, -1] == 0).all()) == zero, N


def test_a_nan_frame_value_reaches_its_two_intervals_without_their_first_sample():
    hop, N, J = 8, 43, 3
    b = K.gain_curve_inputs(hop, 2, N, seed=2)
    b["gain_db"][1, J] = float("nan")
    for arith in (torch.float64, torch.float32):
        r = R.forward_backward(b["x"], 44100, b["gain_db"], b["w"], hop, arith=arith)
        n = np.arange(N)
        hit = ((J - 1) * hop < n) & (n < (J + 1) * hop)
        for k in ("y", "gx"):
            assert np.isnan(r[k][1][:, hit]).all() and np.isfinite(r[k][1][:, ~hit]).all() and np.isfinite(r[k][[0, 2]]).all(), k
        assert np.isnan(r["ggain"][1, J - 1:J + 2]).all() and np.isfinite(np.delete(r["ggain"][1], [J - 1, J, J + 1])).all()
        assert np.isfinite(r["ggain"][[0, 2]]).all()


@pytest.mark.parametrize("cfg", K.GAIN_CURVE_CONFIGS, ids=lambda c: "hop%d-C%d" % c[:2])
def test_no_parity_bound_exceeds_ten_floors(cfg):
    for n, b, want, f32 in K.gain_curve_calls(cfg):
        for k, (e32, bound) in K.bounds(want, f32, R.FLOOR).items():
            assert bound <= 10 * R.FLOOR[k], (cfg, n, k, e32)


def test_wrong_frame_counts_and_bad_hops_raise_before_the_device_is_asked_for():
    """x is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    x = torch.zeros(2, 1, 100)
    for bad in (torch.zeros(2, 2), torch.zeros(2, 4), torch.zeros(3, 3), torch.zeros(6), torch.zeros(2, 3, 1)):
        with pytest.raises(RuntimeError, match=r"gain_db: expected shape \[2, 3\] \(F = ceil\(100 / 64\) \+ 1 = 3 frame points\)"):
            D.gain_curve(x, 44100, bad)
    for hop in (0, 4, 24, 4096, 64.0, True):
        with pytest.raises(ValueError, match="gain_curve: hop"):
            D.gain_curve(x, 44100, torch.zeros(2, 3), hop=hop)
        with pytest.raises(ValueError, match="hop"):
            D.GainCurve(44100, hop=hop)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.gain_curve(torch.zeros(2, 2, 64), 44100, torch.zeros(2, 2))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.GainCurve(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 2), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="gain_curve: float64"):
        D.gain_curve(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, torch.zeros(2, 2))


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers and impossible sizes, DASP_ERR_UNSUPPORTED (-2) for a hop that is no power of two from 8 to
    2048 - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, hop=64)

    def fwd(x=f, P=f, y=f, **kw):
        a = {**ok, **kw}
        return L.dasp_gaincurve_forward(x, P, y, a["B"], a["C"], a["N"], a["hop"], None)

    def bwd(x=f, P=f, gy=f, gx=f, gP=f, scr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_gaincurve_backward(x, P, gy, gx, gP, scr, a["B"], a["C"], a["N"], a["hop"], None)
    for call in (fwd, bwd):
        for kw in (dict(x=None), dict(P=None), dict(B=0), dict(C=0), dict(N=0), dict(hop=0), dict(hop=-8)):
            assert call(**kw) == -1, (call.__name__, kw)
        for hop in (4, 24, 4096):
            assert call(hop=hop) == -2
    assert fwd(y=None) == -1
    assert bwd(gy=None) == -1 and bwd(gx=None, gP=None) == -1 and bwd(scr=None) == -1      # frame gradients without their scratch


def test_module_parameter_tensor_and_range_check():
    names = list(inspect.signature(D.functional.gain_curve).parameters)
    assert names == ["x", "sample_rate", "gain_db", "hop"]
    m = D.GainCurve(44100)
    assert m.param_ranges == {"gain_db": (-60.0, 12.0)} and m.hop == 64 and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.gain_curve and m.process_fn.keywords == {"hop": 64}
    m = D.GainCurve(48000, hop=8, min_gain_db=-20.0, max_gain_db=20.0)
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    x = torch.zeros(3, 2, 20)
    F = 4                                                                  # ceil(20 / 8) + 1
    p = torch.rand(3, F, generator=torch.Generator().manual_seed(0))
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and seen["gain_db"].shape == (3, F) and torch.allclose(seen["gain_db"], p * 40 - 20)
    for bad in (torch.rand(3, F + 1), torch.rand(3, F - 1), torch.rand(3)):
        with pytest.raises(ValueError, match=f"processor has {F} parameters"):
            m.process_normalized(x, bad)
    q = p.clone()
    q[1, 2] = 1.5
    with pytest.raises(ValueError, match="gain_db"):
        m.process_normalized(x, q)
