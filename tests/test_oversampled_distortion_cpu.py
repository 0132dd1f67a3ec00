"""Host-side checks of oversampled_distortion (no GPU): the taps against the numpy formula, the argument checks of the Python layer and
of the C entry points, and the two size queries."""
import ctypes

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import oversampled_distortion_restated as R


@pytest.mark.parametrize("L", [2, 4, 8])
@pytest.mark.parametrize("H", [1, 12, 16])
def test_taps_equal_the_numpy_formula(L, H):
    for beta, cutoff in ((8.0, 0.9), (5.0, 1.0), (0.0, 0.5)):
        h = D.signal.oversampling_taps(L, H, beta, cutoff)
        assert h.dtype is torch.float64 and h.device.type == "cpu" and h.shape == (2 * H * L + 1,)
        c = np.arange(-H * L, H * L + 1)
        want = cutoff * np.sinc(cutoff * c / L) * np.kaiser(2 * H * L + 1, beta)
        assert np.abs(h.numpy() - want).max() <= 1e-15
        assert np.array_equal(h.numpy(), R.taps(L, H, beta, cutoff))
        assert np.array_equal(h.numpy(), h.numpy()[::-1])                      # symmetric: the decimator reuses the interpolator's table


@pytest.mark.parametrize("L", [2, 4, 8])
def test_every_phase_has_unit_dc_gain_at_the_defaults(L):
    h = D.signal.oversampling_taps(L).numpy()
    assert h.shape == (2 * 12 * L + 1,)
    for p in range(L):
        assert abs(h[p::L].sum() - 1.0) <= 1e-4, (L, p, h[p::L].sum())


BAD = [dict(oversample=0), dict(oversample=3), dict(oversample=16), dict(oversample=-2), dict(oversample=4.0), dict(oversample="4"),
       dict(half_width=0), dict(half_width=17), dict(half_width=2.5), dict(half_width=-1),
       dict(cutoff=0.0), dict(cutoff=1.0001), dict(cutoff=-0.5), dict(cutoff=float("nan")),
       dict(beta=-1.0), dict(beta=float("nan")), dict(beta=float("inf"))]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v!r}" for d in BAD for k, v in d.items()])
def test_bad_arguments_raise_value_error(kw):
    (name, _), = kw.items()
    x, drive = torch.zeros(1, 1, 64), torch.zeros(1)
    with pytest.raises(ValueError, match=name):
        D.oversampled_distortion(x, 44100, drive, **kw)
    with pytest.raises(ValueError, match=name):
        D.signal.oversampling_taps(**{"oversample": 4, **kw})


def test_message_names_the_allowed_values():
    with pytest.raises(ValueError, match=r"oversample must be one of \(1, 2, 4, 8\), got 3"):
        D.oversampled_distortion(torch.zeros(1, 1, 8), 44100, torch.zeros(1), oversample=3)
    with pytest.raises(ValueError, match="half_width must be an integer from 1 to 16, got 17"):
        D.oversampled_distortion(torch.zeros(1, 1, 8), 44100, torch.zeros(1), half_width=17)


@pytest.mark.parametrize("L", [1, 2, 4, 8])
def test_cpu_tensor_is_refused(L):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.oversampled_distortion(torch.zeros(2, 2, 64), 44100, torch.zeros(4), oversample=L)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.OversampledDistortion(sample_rate=44100, oversample=L).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 1), 0.5))


def test_wrong_drive_count_raises_as_distortion_does():
    x = torch.zeros(2, 2, 64)
    for n in (3, 8, 5):
        with pytest.raises(RuntimeError) as want:
            D.distortion(x, 44100, torch.zeros(n))
        with pytest.raises(RuntimeError) as got:
            D.oversampled_distortion(x, 44100, torch.zeros(n))
        assert type(got.value) is type(want.value) and str(got.value) == str(want.value), n


def test_module_mirrors_distortion():
    m, d = D.OversampledDistortion(), D.Distortion()
    assert m.param_ranges == d.param_ranges == {"drive_db": (0.0, 24.0)} and m.num_params == 1 and m.sample_rate is None and m.oversample == 4
    m = D.modules.OversampledDistortion(-6.0, 12.0, 48000, oversample=8)
    assert m.param_ranges == {"drive_db": (-6.0, 12.0)} and m.sample_rate == 48000 and m.oversample == 8
    assert D.oversampled_distortion is D.functional.oversampled_distortion


def test_size_queries_agree():
    L = _lib.lib()
    assert [L.dasp_osdist_tile(f) for f in (2, 4, 8)] == sorted((L.dasp_osdist_tile(f) for f in (2, 4, 8)), reverse=True)
    for f in (2, 4, 8):
        T = L.dasp_osdist_tile(f)
        assert T > 2 * 16                                   # a tile is longer than the widest halo
        for rows in (1, 3, 128):
            for N in (1, T - 1, T, T + 1, 5 * T, 5 * T + 1, 131072):
                assert L.dasp_osdist_partial_floats(rows, N, f) == rows * -(-N // T), (f, rows, N)
    for f in (0, 1, 3, 16):
        assert L.dasp_osdist_tile(f) == -1 and L.dasp_osdist_partial_floats(4, 1000, f) == -1
    assert L.dasp_osdist_partial_floats(0, 1000, 4) == -1 and L.dasp_osdist_partial_floats(4, 0, 4) == -1


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) before the taps are read and before any launch; DASP_ERR_UNSUPPORTED (-2) for a grid beyond 2^31 workgroups.
    The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    taps = (ctypes.c_float * (2 * 16 * 8 + 1))()
    ok = dict(B=2, C=2, N=1000, L=4, H=12)

    def fwd(x=f, drive=f, h=taps, y=f, **kw):
        a = {**ok, **kw}
        return L.dasp_osdist_forward(x, drive, h, y, a["B"], a["C"], a["N"], a["L"], a["H"], None)

    def bwd(x=f, drive=f, h=taps, gy=f, gx=f, gd=f, part=f, **kw):
        a = {**ok, **kw}
        return L.dasp_osdist_backward(x, drive, h, gy, gx, gd, part, a["B"], a["C"], a["N"], a["L"], a["H"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1
        assert call(L=3) == -1 and call(L=1) == -1 and call(L=16) == -1
        assert call(H=17) == -1 and call(H=0) == -1
        assert call(drive=None) == -1 and call(h=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1
        assert call(B=1 << 15, C=1 << 15, N=1 << 20) == -2
    assert fwd(y=None) == -1
    assert bwd(gy=None) == -1 and bwd(gx=None) == -1 and bwd(gd=None) == -1 and bwd(part=None) == -1
