"""Golden vectors of the reference's freqdomain_fir (dasp_pytorch/signal.py:35-39), made by running the *reference itself*
(csteinmetz1/dasp-pytorch v0.0.1, imported from /root/reference) on the CPU, in the manner of make_golden.py. Run in the build
container only:

    python tests/golden/make_golden_freqdomain_fir.py

Every file (deflated) holds, as float32: the input x, the response H as H_re / H_im (complex64 values), the loss weights w, and y64, gx64,
gH64_re / gH64_im - the reference's float64 output and its float64 gradients of (y * w).sum() w.r.t. x and H, computed on the float32
inputs cast to float64 / complex128 and rounded to float32 on save (6e-8 relative, far below the tolerance of the tests). Seeds are
fixed and the archives are written with fixed member timestamps, so re-running the script reproduces the files bit for bit.
"""
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import dasp_pytorch.signal as RS  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def save(name, **arrays):
    """np.savez with a fixed timestamp on every member (np.savez stamps the current time)."""
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(arrays[key]), allow_pickle=False)
    print(name, {k: (v.shape, v.dtype.name) for k, v in arrays.items()}, f"{os.path.getsize(path) / 1024:.0f} KiB")


def case(name, x_shape, h_lead, n_fft, seed):
    g = torch.Generator().manual_seed(seed)
    bins = n_fft // 2 + 1
    x = torch.randn(x_shape, generator=g, dtype=torch.float64).to(torch.float32)
    # a response with structure: a random complex spectrum under a gentle low-pass tilt, non-zero imaginary parts at DC and Nyquist
    tilt = 1.0 / (1.0 + torch.arange(bins, dtype=torch.float64) / (0.25 * bins))
    H = (torch.randn(*h_lead, bins, generator=g, dtype=torch.float64) + 1j * torch.randn(*h_lead, bins, generator=g, dtype=torch.float64)) * tilt
    H = H.to(torch.complex64)
    # loss weights on a grid of 1/8 in [-2, 2]: as good a cotangent as any, and they deflate to a fifth (the 16384-point file stays
    # well under 1 MB)
    w = (torch.randint(-16, 17, (*x_shape[:-1], n_fft), generator=g).to(torch.float32) / 8.0)
    x64 = x.to(torch.float64).requires_grad_(True)
    H64 = H.to(torch.complex128).requires_grad_(True)
    y = RS.freqdomain_fir(x64, H64, n_fft)
    assert y.shape == tuple(x_shape[:-1]) + (n_fft,)
    (y * w.to(torch.float64)).sum().backward()
    f32 = lambda t: t.detach().to(torch.float32).numpy()
    save(name, x=x.numpy(), H_re=f32(H.real), H_im=f32(H.imag), w=w.numpy(), n_fft=np.int64(n_fft), y64=f32(y), gx64=f32(x64.grad),
         gH64_re=f32(H64.grad.real), gH64_im=f32(H64.grad.imag))


def main():
    torch.set_num_threads(1)
    case("fdfir_b2c2_t700_n512", (2, 2, 700), (2, 1), 512, 21)           # T > n_fft: cropped; H shared by the two channels
    case("fdfir_b2c3_t3000_n4096", (2, 3, 3000), (2, 3), 4096, 22)       # zero-padded; a response per row, odd row count
    case("fdfir_b2c2_t6000_n16384", (2, 2, 6000), (2, 1), 16384, 23)     # the four-step transform


if __name__ == "__main__":
    main()
