"""Restatement in torch of the oversampled distortion (functional.oversampled_distortion): interpolation by L with a Kaiser-windowed
sinc, tanh(g .), the same low-pass and decimation by L - conv_transpose1d -> tanh -> conv1d on the CPU, in float64 unless told
otherwise, with the vector-Jacobian product taken by autograd. The taps come from numpy, not from the product."""
import numpy as np
import torch
import torch.nn.functional as TF


def taps(L, H=12, beta=8.0, cutoff=0.9):
    """h[c], c = -H L .. H L, float64."""
    c = np.arange(-H * L, H * L + 1, dtype=np.float64)
    return cutoff * np.sinc(cutoff * c / L) * np.kaiser(2 * H * L + 1, beta)


def forward(x, drive_db, L, H=12, beta=8.0, cutoff=0.9, dtype=torch.float64):
    """x (bs, chs, n), drive_db with bs * chs values -> y (bs, chs, n) in `dtype` on the CPU. The taps are computed in float64 and rounded
    once to float32 - the values the product uses - before they are cast to `dtype`."""
    bs, chs, n = x.shape
    h = torch.from_numpy(taps(L, H, beta, cutoff)).to(torch.float32).to(dtype).view(1, 1, -1)
    g = (10.0 ** (drive_db.to(dtype).reshape(bs * chs, 1, 1) / 20.0))
    xr = x.to(dtype).reshape(bs * chs, 1, n)
    u = TF.conv_transpose1d(xr, h, stride=L)[..., H * L:H * L + L * n]
    y = TF.conv1d(torch.tanh(g * u), h / L, stride=L, padding=H * L)
    return y.reshape(bs, chs, n)


def forward_backward(x, drive_db, gy, L, H=12, beta=8.0, cutoff=0.9, dtype=torch.float64):
    """(y, gx, gdrive) on the CPU in `dtype`: gx and gdrive are the gradients of sum(y * gy)."""
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    dd = drive_db.detach().cpu().to(dtype).requires_grad_(True)
    y = forward(xd, dd, L, H, beta, cutoff, dtype)
    gx, gd = torch.autograd.grad(y, (xd, dd), gy.detach().cpu().to(dtype))
    return y.detach(), gx, gd


def inharmonic_share_db(y, bin0):
    """Energy of y (1-D, its length the period count's base) that sits on no harmonic of the tone on bin `bin0`, in dB relative to the total:
    Hann window over the full length, +-4 bins around every harmonic k * bin0 below Nyquist (and around DC) left out."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[-1]
    P = np.abs(np.fft.rfft(y * np.hanning(n))) ** 2
    keep = np.ones(P.shape[-1], dtype=bool)
    k = 0
    while k * bin0 <= n // 2:
        keep[max(0, k * bin0 - 4):k * bin0 + 5] = False
        k += 1
    return 10.0 * np.log10(P[keep].sum() / P.sum())
