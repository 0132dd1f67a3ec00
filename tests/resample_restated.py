"""Restatement of resample in torch on the CPU: torchaudio.functional.resample's published algorithm line by line - the
design in float64, the taps rounded once to float32, a strided conv1d with the full (n, 1, K) kernel, transpose / reshape, crop to
ceil(n N / o) - with the one deviation the definition makes: a tap is exactly 0 where the window's argument was clamped. torchaudio
itself is not installed here; parity of the kernels is pinned to this file, and this file to `direct`, a plain double loop in numpy
whose gradient is written by hand.

arith=torch.float64 is the oracle; arith=torch.float32 (the same float32 taps, float32 products and sums in conv1d's own order) is the
yardstick e32 of the GPU tests. Both come with autograd."""
import math

import numpy as np
import torch

FLOOR = 2e-6            # the least the kernel's parity bound is, for y and grad x alike
KAISER_BETA = 14.769656459379492
KAISER_FAST = dict(lowpass_filter_width=16, rolloff=0.85, resampling_method="sinc_interp_kaiser", beta=8.555504641634386)


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def out_len(o, n, N):
    return -((-n * N) // o)


def design(o, n, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """(taps float32 (n, K), width, inside bool (n, K)) for reduced rates: torchaudio's _get_sinc_resample_kernel in float64, then the
    zero rule, then one rounding."""
    W = lowpass_filter_width
    base = min(o, n) * rolloff
    width = math.ceil(W * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    t = t * base
    inside = t.abs() < W
    t = t.clamp(-W, W)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / W / 2) ** 2
    else:
        b = torch.tensor(KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
        window = torch.i0(b * torch.sqrt(1 - (t / W) ** 2)) / torch.i0(b)
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / o)
    k = torch.where(inside, k, torch.zeros_like(k))
    return k.to(torch.float32), width, inside


def forward(x, orig_freq, new_freq, arith=torch.float64, **kw):
    """x (..., N) -> (..., ceil(n N / o)) in `arith`; differentiable in x."""
    o, n = reduced(orig_freq, new_freq)
    if o == n:
        return x
    h, width, _ = design(o, n, **kw)
    lead, N = x.shape[:-1], x.shape[-1]
    xr = x.reshape(-1, N).to(arith)
    xp = torch.nn.functional.pad(xr, (width, width + o))
    y = torch.nn.functional.conv1d(xp[:, None], h.to(arith)[:, None], stride=o)           # (rows, n, frames)
    y = y.transpose(1, 2).reshape(xr.shape[0], -1)[..., :out_len(o, n, N)]
    return y.reshape(*lead, -1)


def forward_backward(x, w, orig_freq, new_freq, arith=torch.float64, **kw):
    """{y, gx} as float64 numpy arrays: gx the gradient of sum(y w)."""
    xt = x.detach().clone().to(arith).requires_grad_(True)
    y = forward(xt, orig_freq, new_freq, arith=arith, **kw)
    (gx,) = torch.autograd.grad((y * w.to(arith)).sum(), xt)
    return dict(y=y.detach().double().numpy(), gx=gx.double().numpy())


def taps_numpy(o, n, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """The formula of the definition tap by tap with Python floats - no clamp: outside |t| < W the tap is zero by definition.
    Returns (h float64 (n, K), width, inside)."""
    W = float(lowpass_filter_width)
    base = min(o, n) * rolloff
    width = math.ceil(W * o / base)
    K = 2 * width + o
    b = KAISER_BETA if beta is None else float(beta)
    h, inside = np.zeros((n, K)), np.zeros((n, K), bool)
    for r in range(n):
        for k in range(K):
            t = (-r / n + (k - width) / o) * base
            if abs(t) < W:
                inside[r, k] = True
                win = math.cos(math.pi * t / (2 * W)) ** 2 if resampling_method == "sinc_interp_hann" else \
                    float(np.i0(b * math.sqrt(1 - (t / W) ** 2)) / np.i0(b))
                h[r, k] = (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)) * win * base / o
    return h, width, inside


def direct(x, w, orig_freq, new_freq, **kw):
    """The definition as a double loop over outputs and taps in float64, taps from taps_numpy rounded to float32, and its gradient
    written out: every product h x[i] of output j sends h w[j] to gx[i]. x, w: numpy (rows, N), (rows, M)."""
    o, n = reduced(orig_freq, new_freq)
    h, width, inside = taps_numpy(o, n, **kw)
    h = h.astype(np.float32).astype(np.float64)
    rows, N = x.shape
    M = out_len(o, n, N)
    y, gx = np.zeros((rows, M)), np.zeros((rows, N))
    for j in range(M):
        q, r = divmod(j, n)
        for k in np.nonzero(inside[r])[0]:
            i = q * o + k - width
            if 0 <= i < N:
                y[:, j] += h[r, k] * x[:, i]
                gx[:, i] += h[r, k] * w[:, j]
    return dict(y=y, gx=gx)


def spans(o, n, N, **kw):
    """(lo, hi) int arrays of length M: output j reads exactly the inputs lo[j] <= i < hi[j] (before clipping to [0, N))."""
    _, width, inside = design(o, n, **kw)
    inside = inside.numpy()
    first, cnt = inside.argmax(1), inside.sum(1)
    j = np.arange(out_len(o, n, N))
    q, r = j // n, j % n
    lo = q * o + first[r] - width
    return lo, lo + cnt[r]
