"""envelope_follower without a GPU: the blocked identities that csrc/envelope.hip evaluates (E and the tangent D) against the sample
loop in float64, the hand-written adjoint against autograd, the condition on the parity cases of the GPU tests (the restatement in the
kernel's arithmetic alone stays within 2.5 floors of the oracle, so no bound exceeds ten), the argument errors raised before the
device is asked for, the size queries and the C entry points' refusals."""
import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import control_rate_cases as K
from tests import envelope_restated as R


def _inputs(bs, chs, N, hop, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(bs, chs, N, generator=g), w=torch.randn(bs, R.control_frames(N, hop), generator=g))


@pytest.mark.parametrize("detector", R.DETECTORS)
@pytest.mark.parametrize("sr,hop,N,sm", [(8000, 8, 203, (0.1, 3.0, 80.0)), (44100, 64, 700, (0.05, 50.0, 2000.0)), (192000, 2048, 4100, (1.0, 50.0, 20000.0)),
                                         (44100, 16, 1, (5.0, 5.0, 5.0)), (44100, 32, 32, (5.0, 0.5, 500.0))])
def test_blocked_identities_and_adjoint_against_the_sample_loop(detector, sr, hop, N, sm):
    """E, and by autograd through the loop gx and gsm, against the blocked form with its hand-written adjoint, both float64: 1e-12 of
    the peak for E (the issue measured 4e-15 on its case), 1e-9 for the gradients (D passes through a sum over the frames)."""
    a = _inputs(3, 2, N, hop, seed=hop + N)
    sm = torch.tensor(sm)
    want = R.forward_backward(a["x"], sr, sm, a["w"], hop, detector)
    got = R.blocked(a["x"].numpy(), sr, sm.numpy(), a["w"].numpy(), hop, detector, np.float64)
    assert K.per_item_err(got["E"], want["E"]) <= 1e-12
    assert K.per_item_err(got["gx"], want["gx"]) <= 1e-9
    assert np.abs(got["gsm"] - want["gsm"]).max() <= 1e-9 * np.abs(want["gsm"]).max()
    clamped = (sm < 0.1) | (sm > 10000.0)
    assert (got["gsm"][clamped.numpy()] == 0).all() and (want["gsm"][clamped.numpy()] == 0).all()


def test_tangent_against_a_central_difference():
    """D_j = dE_j/da frame by frame: the blocked tangent against (E(a + d) - E(a - d)) / 2 d of the sample loop, through t -> a."""
    sr, hop, N = 44100, 64, 700
    a = _inputs(2, 2, N, hop, seed=3)
    sm = torch.tensor([2.0, 40.0])
    lna, oma, t, _ = R.item_constants(sr, sm.numpy())
    D_ = R.blocked(a["x"].numpy(), sr, sm.numpy(), a["w"].numpy(), hop, "peak", np.float64)["D"]
    h = 1e-6 * sm.double()
    Ep, Em = (R.envelope(a["x"], sr, sm.double() + s * h, hop, "peak").numpy() for s in (1, -1))
    dadt = np.exp(lna) * R.LN9 * 1000.0 / (sr * t * t)
    fd = (Ep - Em) / (2 * h.numpy()[:, None]) / dadt[:, None]
    assert np.abs(fd - D_).max() <= 1e-6 * np.abs(D_).max()


def test_peak_gradient_goes_to_the_lowest_winning_channel_and_sign_zero_is_zero():
    x = torch.tensor([[[0.5, -0.5, 0.0, 0.2], [0.5, 0.7, 0.0, -0.2]]])
    w = torch.ones(1, R.control_frames(4, 8))
    for r in (R.forward_backward(x, 8000, torch.tensor([1.0]), w, 8, "peak"),
              R.blocked(x.numpy(), 8000, np.array([1.0]), w.numpy(), 8, "peak", np.float64)):
        gx = r["gx"][0]
        assert (gx[1, [0, 2, 3]] == 0).all() and gx[0, 1] == 0 and gx[0, 2] == 0          # ties to channel 0, sign(0) = 0
        assert gx[0, 0] > 0 and gx[1, 1] > 0 and gx[0, 3] > 0


@pytest.mark.parametrize("cfg", K.ENVELOPE_CONFIGS, ids=lambda c: "sr%d-hop%d-C%d-%s" % c[:4])
def test_no_parity_bound_exceeds_ten_floors(cfg):
    for n, b, want, f32 in K.envelope_calls(cfg):
        for k, (e32, bound) in K.bounds(want, f32, R.FLOOR).items():
            assert bound <= 10 * R.FLOOR[k], (cfg, n, k, e32)


def test_wrong_counts_and_bad_scalars_raise_before_the_device_is_asked_for():
    """x is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    x = torch.zeros(2, 1, 64)
    with pytest.raises(RuntimeError, match=r"smoothing_ms: shape '\[2\]' is invalid for input of size 3"):
        D.envelope_follower(x, 44100, torch.ones(3))
    for sr in (0, -8000, float("nan"), float("inf"), "fast"):
        with pytest.raises(ValueError, match="envelope_follower: finite sample_rate"):
            D.envelope_follower(x, sr, torch.ones(2))
    for hop in (0, 4, 24, 4096, 64.0, True):
        with pytest.raises(ValueError, match="envelope_follower: hop"):
            D.envelope_follower(x, 44100, torch.ones(2), hop=hop)
    for det in ("rms", "Peak", 0, None):
        with pytest.raises(ValueError, match="detector"):
            D.envelope_follower(x, 44100, torch.ones(2), detector=det)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.envelope_follower(torch.zeros(2, 2, 64), 44100, torch.ones(2))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="envelope_follower: float64"):
        D.envelope_follower(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, torch.ones(2))


def test_the_functions_define_no_forward_of_their_own():
    from dasp_pytorch_amd import _ctypes_ops as C
    for fn, kernels in ((C.EnvelopeFollowerFunction, C.EnvelopeFollowerKernels), (C.GainCurveFunction, C.GainCurveKernels)):
        assert "forward" not in vars(fn) and "backward" not in vars(fn) and issubclass(fn, kernels) and issubclass(fn, torch.autograd.Function)
        assert not issubclass(kernels, torch.autograd.Function)


def test_size_queries():
    L = _lib.lib()
    assert L.dasp_envelope_tile() == K.TILE
    for B in (1, 3, 256):
        for N in (1, 7, 64, 65, K.TILE, 2 * K.TILE + 3):
            for hop in (8, 64, 2048):
                assert L.dasp_envelope_scratch_floats(B, N, hop) == 2 * B * R.control_frames(N, hop) == L.dasp_gaincurve_scratch_floats(B, N, hop)
    for q in (L.dasp_envelope_scratch_floats, L.dasp_gaincurve_scratch_floats):
        assert q(0, 10, 64) == -1 and q(4, 0, 64) == -1 and q(4, 10, -8) == -1
        for hop in (4, 24, 4096):
            assert q(4, 10, hop) == -2


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, impossible sizes, detectors and rates and for an inconsistent pair of optional outputs,
    DASP_ERR_UNSUPPORTED (-2) for a hop that is no power of two from 8 to 2048 - all before any launch. The non-null device pointers are
    fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, hop=64, det=0, sr=44100.0)

    def fwd(x=f, sm=f, env=f, tan=f, scr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_envelope_forward(x, sm, env, tan, scr, a["B"], a["C"], a["N"], a["hop"], a["det"], a["sr"], None)

    def bwd(x=f, sm=f, tan=f, ge=f, gx=f, gs=f, scr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_envelope_backward(x, sm, tan, ge, gx, gs, scr, a["B"], a["C"], a["N"], a["hop"], a["det"], a["sr"], None)
    for call in (fwd, bwd):
        for kw in (dict(x=None), dict(sm=None), dict(scr=None), dict(B=0), dict(C=0), dict(N=0), dict(hop=0), dict(det=2), dict(det=-1), dict(sr=0.0),
                   dict(sr=float("nan")), dict(sr=float("inf"))):
            assert call(**kw) == -1, (call.__name__, kw)
        for hop in (4, 24, 4096):
            assert call(hop=hop) == -2
    assert fwd(env=None) == -1
    assert bwd(ge=None) == -1 and bwd(gx=None, gs=None, tan=None) == -1
    assert bwd(tan=None) == -1 and bwd(gs=None) == -1                       # the tangent and the control gradient come and go together
