"""block_level without a GPU: the hand-written forward pass and adjoint of tests/block_level_restated.py against the definition and
autograd, the winner rules, the condition on the parity cases of the GPU tests (no bound exceeds ten floors; peak is exact), the
argument errors raised before the device is asked for and the C entry points' refusals."""
import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import ballistics_cases as K
from tests import block_level_restated as R


@pytest.mark.parametrize("detector", R.DETECTORS)
@pytest.mark.parametrize("hop,chs,N", [(8, 1, 203), (64, 2, 700), (2048, 3, 4100), (16, 2, 1), (32, 2, 32), (8, 3, 9)])
def test_by_hand_equals_the_definition_and_autograd(detector, hop, chs, N):
    """float64 against float64: 1e-12 of the peak (peak: nothing is rounded at all)."""
    g = torch.Generator().manual_seed(hop + N)
    x, w = torch.randn(3, chs, N, generator=g).double(), torch.randn(3, R.control_frames(N, hop), generator=g).double()
    want = R.forward_backward(x, w, hop, detector)
    got = R.by_hand(x.numpy(), w.numpy(), hop, detector, np.float64)
    for k in R.NAMES:
        assert K.per_item_err(got[k], want[k]) <= (0.0 if detector == "peak" else 1e-12), k


def test_the_earliest_maximum_wins_on_its_lowest_channel_and_sign_zero_is_zero():
    hop, N = 8, 41
    x = torch.zeros(1, 3, N)
    x[0, 1, 3], x[0, 2, 3], x[0, 0, 5], x[0, 1, 8] = -0.5, 0.5, 0.5, 0.5
    x[0, 2, 16] = 0.25
    w = torch.arange(1.0, R.control_frames(N, hop) + 1)[None]
    want = np.zeros((3, N))
    want[1, 3], want[2, 16] = -2.0, 3.0
    for r in (R.forward_backward(x, w, hop, "peak"), R.by_hand(x.numpy(), w.numpy(), hop, "peak")):
        assert r["L"][0, :3].tolist() == [0.0, 0.5, 0.25] and np.array_equal(r["gx"][0], want)
    win = R.by_hand(x.numpy(), w.numpy(), hop, "peak")["win"][0]
    assert win[1] == (2 | 2 << 11 | 1 << 13) and win[2] == (7 | 1 << 11 | 2 << 13) and win[0] == 0 and win[3] == 0


def test_the_first_nan_of_a_block_wins_it():
    hop, N = 8, 30
    x = torch.randn(1, 2, N, generator=torch.Generator().manual_seed(1))
    x[0, 1, 11], x[0, 0, 13] = float("nan"), float("nan")
    r = R.by_hand(x.numpy(), np.ones((1, R.control_frames(N, hop))), hop, "peak")
    assert np.isnan(r["L"][0]).tolist() == [False, False, True, False, False]
    assert r["win"][0, 2] == (2 | 3 << 11 | 1 << 13)
    L = R.block_level(x, hop, "peak")
    assert torch.isnan(L[0]).tolist() == [False, False, True, False, False]


def test_power_always_divides_by_hop():
    x = torch.ones(1, 1, 13)
    L = R.block_level(x, 8, "power")[0]
    assert L.tolist() == [1.0, 1.0, 0.5]                                     # samples 9 .. 12 of the block 9 .. 16


@pytest.mark.parametrize("cfg", K.BLOCK_LEVEL_CONFIGS, ids=lambda c: "hop%d-C%d-%s-ties%d" % c[:4])
def test_no_parity_bound_exceeds_ten_floors_and_peak_is_exact(cfg):
    hop, chs, det, ties, seed = cfg
    repeats = 0
    for n, b, want, hand in K.block_level_calls(cfg):
        for k, (e32, bound) in K.bounds(want, hand, R.FLOOR).items():
            assert bound <= 10 * R.FLOOR[k], (cfg, n, k, e32)
            if det == "peak":
                assert e32 == 0.0, (cfg, n, k)
        if ties and n >= hop:
            p = b["x"].abs().amax(1)[:, 1:1 + (n - 1) // hop * hop].reshape(K.BS, -1, hop)
            repeats += int(((p == p.amax(-1, keepdim=True)).sum(-1) > 1).sum())
            if chs > 1:
                a = b["x"].abs()
                repeats += int(((a == a.amax(1, keepdim=True)).sum(1) > 1).sum())
    assert not ties or repeats > 100                                          # the ties case does hold repeated maxima


def test_bad_arguments_raise_before_the_device_is_asked_for():
    """x is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    x = torch.zeros(2, 1, 64)
    for hop in (0, 4, 24, 4096, 64.0, True):
        with pytest.raises(ValueError, match="block_level: hop"):
            D.block_level(x, 44100, hop=hop)
    for det in ("rms", "Peak", 0, None):
        with pytest.raises(ValueError, match="detector"):
            D.block_level(x, 44100, detector=det)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.block_level(x, 44100)


def test_float64_is_refused(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="block_level: float64"):
        D.block_level(torch.zeros(2, 2, 64, dtype=torch.float64), 44100)


def test_the_functions_define_no_forward_of_their_own():
    from dasp_pytorch_amd import _ctypes_ops as C
    for fn, kernels in ((C.BlockLevelFunction, C.BlockLevelKernels), (C.BallisticsFunction, C.BallisticsKernels)):
        assert "forward" not in vars(fn) and "backward" not in vars(fn) and issubclass(fn, kernels) and issubclass(fn, torch.autograd.Function)
        assert not issubclass(kernels, torch.autograd.Function)


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, impossible sizes and detectors, DASP_ERR_UNSUPPORTED (-2) for a hop that is no power of two
    from 8 to 2048 - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, hop=64, det=0)

    def fwd(x=f, lev=f, win=f, **kw):
        a = {**ok, **kw}
        return L.dasp_blocklevel_forward(x, lev, win, a["B"], a["C"], a["N"], a["hop"], a["det"], None)

    def bwd(x=f, win=f, gl=f, gx=f, **kw):
        a = {**ok, **kw}
        return L.dasp_blocklevel_backward(x, win, gl, gx, a["B"], a["C"], a["N"], a["hop"], a["det"], None)
    for call in (fwd, bwd):
        for kw in (dict(B=0), dict(C=0), dict(N=0), dict(hop=0), dict(det=2), dict(det=-1)):
            assert call(**kw) == -1, (call.__name__, kw)
        for hop in (4, 24, 4096):
            assert call(hop=hop) == -2
        assert call(C=(1 << 18) + 1) == -2
    assert fwd(x=None) == -1 and fwd(lev=None) == -1
    assert bwd(gl=None) == -1 and bwd(gx=None) == -1 and bwd(win=None) == -1 and bwd(x=None, det=1) == -1
