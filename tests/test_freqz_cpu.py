"""fft_freqz / fft_sosfreqz without a GPU: the backward workspace query of the C ABI, the golden vectors of the reference's responses
(tests/golden/freqz_*.npz) against the CPU oracle, and the refusal of CPU tensors."""
import glob
import os

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from oracle import dasp_oracle as orc
from tests.freqz_exact import exact_for_golden
from tests.util import GOLDEN, load_golden

NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "freqz_*.npz")))


def test_goldens_exist():
    assert len([n for n in NAMES if n.startswith("freqz_sos_")]) >= 4 and len([n for n in NAMES if n.startswith("freqz_ba_")]) >= 4
    for n in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 1 << 20


def test_workspace_query_without_device():
    L = _lib.lib()
    # one partial per (row, workgroup of 64-bin tiles, coefficient): 257 bins = 5 tiles, one tile per workgroup while the device has room
    assert L.dasp_freqz_work_doubles(4, 6, 3, 3, 512) == 4 * 5 * 36
    assert L.dasp_freqz_work_doubles(256, 6, 3, 3, 262144) == 256 * 129 * 36          # 2049 tiles, 16 per workgroup
    assert L.dasp_freqz_work_doubles(1, 1, 5, 5, 3) == 1 * 1 * (3 + 3)                  # taps beyond n_fft are cropped
    assert L.dasp_freqz_work_doubles(0, 16, 3, 3, 512) == 0
    assert L.dasp_freqz_work_doubles(1, 17, 3, 3, 512) == -1 and L.dasp_freqz_work_doubles(1, 1, 33, 3, 512) == -1
    assert L.dasp_freqz_work_doubles(1, 1, 3, 3, 0) == -1
    assert L.dasp_freqz_work_doubles(1, 16, 4, 3, 512) == -2                            # 112 coefficients per row: more than the kernel holds
    assert L.dasp_freqz_forward(None, None, 1, 1, 3, 3, 512, 0, None, None) == -1


@pytest.mark.parametrize("name", NAMES)
def test_goldens_against_oracle(name):
    g = load_golden(name)
    n = int(g["n_fft"])
    if "sos" in g:
        H = orc.fft_sosfreqz(g["sos"].astype(np.float64), n)
    else:
        H = orc.fft_freqz(g["b"].astype(np.float64), g["a"].astype(np.float64), n)
    H64 = g["H64"]
    assert H.shape == H64.shape and H64.dtype == np.complex128
    # two float64 FFT implementations (numpy's, torch's) on the same coefficients; next to a pole close to the unit circle both lose
    # digits (tests/freqz_exact.py), so they agree to 1e-10 of the peak, not to rounding
    err = np.abs(H - H64).reshape(-1, H.shape[-1]).max(1) / np.abs(H64).reshape(-1, H.shape[-1]).max(1)
    assert err.max() < 1e-10, err.max()
    Hx, _ = exact_for_golden(g)
    assert (np.abs(Hx - H64).reshape(err.shape + (-1,)).max(1) / np.abs(Hx).reshape(err.shape + (-1,)).max(1)).max() < 1e-10
    # the reference's float32 response is the float32 FFT of the same coefficients: not equal, and on the corner designs (20 Hz shelves,
    # bands at the top of their range) off by up to 2e-2 of the peak - what the device kernel's fp64 evaluation removes
    e32 = np.abs(g["H32"] - H64).max() / np.abs(H64).max()
    assert 0 < e32 < 0.05


def test_no_cpu_path():
    sos = torch.randn(2, 3, 6)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.signal.fft_sosfreqz(sos)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.signal.fft_freqz(torch.randn(2, 3), torch.randn(2, 3), 64)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.ParametricEQ(44100).frequency_response(torch.rand(2, 18))


def test_frequency_response_refuses_another_filter():
    """frequency_response designs functional.parametric_eq's six sections: a processor whose process_fn was replaced or whose parameters
    were renamed would get the response of another filter than the one process_normalized runs - it raises instead."""
    eq = D.ParametricEQ(44100)
    eq.process_fn = lambda x, sample_rate, **kw: x
    with pytest.raises(NotImplementedError, match="parametric_eq"):
        eq.frequency_response(torch.rand(2, 18))
    eq = D.ParametricEQ(44100)
    eq.param_ranges = {k.replace("band0", "mid"): v for k, v in eq.param_ranges.items()}
    with pytest.raises(NotImplementedError):
        eq.frequency_response(torch.rand(2, 18))
