"""CPU-side checks of the BS.1770 meter: the float64 restatement against the recommendation's own numbers (coefficient table, the
997 Hz anchors, its gradient against a finite difference), the package's design table, argument validation before any device check,
and the pure host queries of csrc/loudness.hip."""
import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib

from tests import bs1770_restated as R


def test_design_reproduces_the_recommendations_table():
    want = np.array([list(R.BS1770_48K["b1"]) + list(R.BS1770_48K["a1"]), list(R.BS1770_48K["b2"]) + list(R.BS1770_48K["a2"])])
    got_r = R.k_weighting(48000)
    got_p = D.signal.k_weighting_sos(48000)
    assert got_p.shape == (2, 6) and got_p.dtype is torch.float64 and got_p.device.type == "cpu"
    print("restated", np.abs(got_r - want).max(), "package", np.abs(got_p.numpy() - want).max())
    assert np.abs(got_r - want).max() <= 1e-12
    assert np.abs(got_p.numpy() - want).max() <= 1e-12
    for fs in (8000, 44100, 96000, 384000):
        assert np.abs(D.signal.k_weighting_sos(fs).numpy() - R.k_weighting(fs)).max() <= 1e-14
    with pytest.raises(ValueError):
        D.signal.k_weighting_sos(4000)


def test_997_hz_anchors():
    left = R.loudness(R.sine_997([0]), 48000)["L"][0]
    both = R.loudness(R.sine_997([0, 1]), 48000)["L"][0]
    print("left", left, "both", both)
    assert abs(left - (-3.01)) <= 0.01
    assert abs(both - 0.0) <= 0.01


def test_restated_gradient_matches_a_finite_difference():
    x = R.gated_draw().astype(np.float64)
    r = R.loudness(x, 8000)
    assert list(r["nb"]) == [27, 27] and r["margin"].min() >= 0.5
    d = np.random.default_rng(1).standard_normal(x.shape)
    h = 1e-6
    for i in range(2):
        di = np.zeros_like(d)
        di[i] = d[i]
        fd = (R.loudness(x + h * di, 8000)["L"][i] - R.loudness(x - h * di, 8000)["L"][i]) / (2 * h)
        an = float((r["grad"][i] * d[i]).sum())
        print("item", i, "analytic", an, "finite difference", fd)
        assert abs(an - fd) <= 1e-6 * abs(fd)


def test_gated_draw_is_the_documented_one():
    r = R.loudness(R.gated_draw(), 8000)
    print({k: v for k, v in r.items() if k != "grad"})
    assert r["nb"][0] == 27 and r["nA"][0] == 20 and r["nJ"][0] == 10
    assert abs(r["L"][0] - (-5.926)) < 5e-3


def test_validation_runs_before_the_device_check():
    fs = 8000
    T = 3200
    with pytest.raises(ValueError, match="channels"):
        D.loudness(torch.zeros(1, 6, T), fs)
    with pytest.raises(ValueError, match="400 ms"):
        D.loudness(torch.zeros(1, 2, T - 1), fs)
    for bad in (4000, 500000):
        with pytest.raises(ValueError, match="sample_rate"):
            D.loudness(torch.zeros(1, 2, 4 * 50000), bad)
        with pytest.raises(ValueError, match="sample_rate"):
            D.loudness_normalize(torch.zeros(1, 2, 4 * 50000), bad)
    with pytest.raises(ValueError, match="bs, chs, seq_len"):
        D.loudness(torch.zeros(2, T), fs)
    with pytest.raises(ValueError, match="bs, chs, seq_len"):
        D.peak_normalize(torch.zeros(2, T), fs)
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.loudness(torch.zeros(1, 2, T, dtype=torch.float64), fs)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):     # valid arguments: only now the device matters
        D.loudness(torch.zeros(1, 2, T), fs)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.peak_normalize(torch.zeros(1, 2, T), fs)


def test_host_queries_answer_without_a_gpu():
    L = _lib.lib()
    fs, H, T = 8000.0, 800, 3200
    for N in (T, T + H - 1, T + H, 24123):
        assert L.dasp_loudness_blocks(N, fs) == R.num_blocks(N, fs)
    assert L.dasp_loudness_blocks(T - 1, fs) == -1 and L.dasp_loudness_blocks(T, 4000.0) == -1
    assert L.dasp_loudness_scratch_doubles(2, 2, 24123, fs) > 0
    assert L.dasp_loudness_scratch_doubles(2, 6, 24123, fs) == -1 and L.dasp_loudness_scratch_doubles(2, 2, T - 1, fs) == -1
    assert L.dasp_loudness_segments(512, 131072) == 1 and L.dasp_loudness_segments(80, 12000) == 1      # many rows; too short to cut
    g = L.dasp_loudness_segments(1, 2 ** 18 + 3)
    assert 1 < g <= 256
    assert L.dasp_loudness_segments(0, 100) == -1
    assert L.dasp_peaknorm_scratch_doubles(6, 4096) == 2 * 6 and L.dasp_peaknorm_scratch_doubles(6, 4097) == 2 * 12 and L.dasp_peaknorm_scratch_doubles(1, 2 ** 18 + 3) > 2


def test_argument_errors_return_without_a_launch():
    L = _lib.lib()
    assert L.dasp_loudness_forward(None, None, None, None, None, 1, 1, 3200, 8000.0, None) == -1
    assert L.dasp_loudness_forward(8, 8, 8, None, None, 1, 6, 3200, 8000.0, None) == -2
    assert L.dasp_loudness_forward(8, 8, 8, None, None, 1, 1, 3199, 8000.0, None) == -2
    assert L.dasp_loudness_forward(8, 8, 8, 8, None, 1, 1, 3200, 8000.0, None) == -1           # ysave without cov
    assert L.dasp_loudness_backward(None, None, None, None, None, 1, 1, 3200, 8000.0, None) == -1
    assert L.dasp_peaknorm_forward(None, None, None, None, 1, 16, 0.0, 1e-8, None) == -1
    assert L.dasp_peaknorm_forward(8, 8, 8, 8, 1, 16, 0.0, -1.0, None) == -1
    assert L.dasp_peaknorm_backward(None, None, None, None, None, 1, 16, 0.0, 1e-8, None) == -1
