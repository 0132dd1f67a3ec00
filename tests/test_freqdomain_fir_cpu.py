"""signal.freqdomain_fir without a GPU: argument checks in the order a caller meets them (n_fft, the bins of H, float64, the device),
the scratch-size query of the C ABI and its refusal of null pointers, and the golden files."""
import glob
import os

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests.util import GOLDEN, load_golden

NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "fdfir_*.npz")))


def _xh(n=512, dtype=torch.float32):
    return torch.randn(2, 2, 100, dtype=dtype), torch.randn(2, 1, n // 2 + 1, dtype=torch.complex128 if dtype == torch.float64 else torch.complex64)


def test_no_cpu_path():
    x, H = _xh()
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.signal.freqdomain_fir(x, H, 512)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.signal.freqdomain_fir(x, H.real.contiguous(), 512)          # a real response


@pytest.mark.parametrize("n", [500, 768, 4, 1, 1 << 21, 3 << 19])
def test_unsupported_lengths_name_the_supported_set(n):
    x, _ = _xh()
    H = torch.randn(2, 1, n // 2 + 1, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match=r"powers of two from 8 to 1048576"):
        D.signal.freqdomain_fir(x, H, n)


def test_n_fft_as_a_zero_dim_integer_tensor():
    x, H = _xh()
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):          # accepted: the call gets as far as the device check
        D.signal.freqdomain_fir(x, H, torch.tensor(512))
    with pytest.raises(NotImplementedError, match="n_fft = 500"):
        D.signal.freqdomain_fir(x, H, torch.tensor(500))
    with pytest.raises(TypeError):
        D.signal.freqdomain_fir(x, H, torch.tensor(512.0))
    with pytest.raises(TypeError):
        D.signal.freqdomain_fir(x, H, torch.tensor([512]))


def test_bins_mismatch():
    x, H = _xh()
    with pytest.raises(RuntimeError, match=r"200 bins.*n_fft = 512 needs 257"):
        D.signal.freqdomain_fir(x, H[..., :200], 512)
    with pytest.raises(RuntimeError, match=r"257 bins.*n_fft = 1024 needs 513"):
        D.signal.freqdomain_fir(x, H, 1024)


def test_float64_is_refused():
    x, H = _xh(dtype=torch.float64)
    assert not D.config.plan.fp64_as_fp32
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.signal.freqdomain_fir(x, H, 512)
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.signal.freqdomain_fir(x.float(), H, 512)                       # complex128 response on float32 audio
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.signal.freqdomain_fir(x.float(), H.real.contiguous(), 512)     # float64 real response


def test_workspace_query_without_device():
    L = _lib.lib()
    # up to 8192 points: one launch per direction, no scratch
    assert L.dasp_fdfir_work_floats(4, 100, 512, 2) == 0
    assert L.dasp_fdfir_work_floats(512, 4096, 8192, 512) == 0
    assert L.dasp_fdfir_work_floats(0, 100, 16384, 0) == 0
    # four-step: the column transforms of gy and of x, one complex frame per two rows of an item, and one frame per item for the
    # products the response's gradient is taken from
    assert L.dasp_fdfir_work_floats(4, 6000, 16384, 2) == 2 * (2 * 2 * 16384) + 2 * 2 * 16384
    assert L.dasp_fdfir_work_floats(6, 10, 16384, 2) == 2 * (2 * 2 * 2 * 16384) + 2 * 2 * 16384       # 3 rows per item: 2 frames
    assert L.dasp_fdfir_work_floats(32, 131072, 262144, 16) == 3 * 2 * 16 * 262144
    # unsupported lengths, rows that the responses do not divide, no samples
    for args in ((1, 10, 1000, 1), (1, 10, 4, 1), (1, 10, 1 << 21, 1), (3, 10, 512, 2), (2, 0, 512, 2), (2, 10, 512, 0), (-1, 10, 512, 1)):
        assert L.dasp_fdfir_work_floats(*args) == -1, args


def test_null_pointers_are_refused_before_any_launch():
    L = _lib.lib()
    assert L.dasp_fdfir_forward(None, None, None, None, None, 0, 1, 10, 512, 1, None) == -1
    assert L.dasp_fdfir_forward(None, None, None, None, None, 0, 2, 10, 16384, 1, None) == -1
    assert L.dasp_fdfir_backward(None, None, None, None, None, None, None, 0, 1, 10, 512, 1, None) == -1
    assert L.dasp_fdfir_backward(None, None, None, None, None, None, None, 0, 2, 10, 16384, 1, None) == -1
    assert L.dasp_fdfir_forward(None, None, None, None, None, 0, 3, 10, 512, 2, None) == -1               # bad sizes
    assert L.dasp_fdfir_forward(None, None, None, None, None, 0, 1, 10, 500, 1, None) == -2               # unsupported length


def test_goldens_are_the_torch_fft_form():
    """The three files, each under 1 MiB, hold what irfft(rfft(x, n) * H, n) gives in float64 on their float32 inputs."""
    assert len(NAMES) == 3
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
        g = load_golden(name)
        n = int(g["n_fft"])
        x = torch.from_numpy(g["x"]).double()
        H = torch.complex(torch.from_numpy(g["H_re"]).double(), torch.from_numpy(g["H_im"]).double())
        y = torch.fft.irfft(torch.fft.rfft(x, n) * H, n)
        assert y.shape == g["y64"].shape and y.shape[-1] == n
        assert np.abs(y.numpy() - g["y64"]).max() <= 1e-6 * np.abs(g["y64"]).max()
        assert g["gx64"].shape == g["x"].shape and g["gH64_re"].shape == g["H_re"].shape
        assert np.all(g["gH64_im"][..., 0] == 0) and np.all(g["gH64_im"][..., -1] == 0)
