"""Restatement in torch of functional.phaser, differentiable by autograd, on the CPU: the formulas of the docstring as a loop over the
samples and the stages. The LFO's phase is always float64 and reduced to a turn in float64. arith=torch.float64 (the default): float64
throughout. arith=torch.float32: the turn is rounded to float32 and everything after it - sin, exp2, the clamp, tan, a, the stages, the
mix - is float32, which is what the kernel does; its error against the float64 variant is the yardstick of the GPU tests.

    theta = 2 pi (rate_hz n / sr + phase + c stereo_spread)
    f[n]  = clamp(center_hz 2^(depth sin theta), sr/4096, 0.49 sr);   t = tan(pi f / sr);   a[n] = (t - 1) / (t + 1)
    s_0 = x;   s_k[n] = a[n] (s_{k-1}[n] - s_k[n-1]) + s_{k-1}[n-1],  k = 1..K;   y[n] = (1 - mix) x[n] + mix s_K[n]
"""
import math

import numpy as np
import torch

CTL = ("rate_hz", "center_hz", "depth", "phase", "mix")
GRADS = ("grate", "gcenter", "gdepth", "gphase", "gmix")
NAMES = ("y", "gx") + GRADS
# the least the kernel's parity bound is, whatever the float32 restatement's own error: the floors of the other fused effects
FLOOR = dict(y=2e-6, gx=2e-6, grate=1e-5, gcenter=1e-5, gdepth=1e-5, gphase=1e-5, gmix=1e-5)


def clamp_bounds(sr):
    return sr / 4096.0, 0.49 * sr


def sweep(sr, rate_hz, center_hz, depth, phase, chs, N, stereo_spread=0.25, arith=torch.float64):
    """(f before the clamp, a), both (bs, chs, N) in `arith`. rate_hz, center_hz, depth, phase: float64, (bs,) or (bs, chs) (a value per
    row: how the tests separate the channels' shares of a control gradient). The clamp is two comparisons: a NaN stays, and a clamped
    sample passes no gradient on."""
    ex = lambda t: (t if t.dim() == 2 else t[:, None].expand(-1, chs))[:, :, None]
    n = torch.arange(N, dtype=torch.float64)
    c = torch.arange(chs, dtype=torch.float64)[None, :, None]
    turns = ex(rate_hz) * n / sr + (ex(phase) + c * stereo_spread)
    th = (turns - torch.round(turns)).to(arith)
    raw = ex(center_hz).to(arith) * torch.exp2(ex(depth).to(arith) * torch.sin(2 * math.pi * th))
    lo, hi = (torch.tensor(v, dtype=arith) for v in clamp_bounds(sr))
    f = torch.where(raw < lo, lo, torch.where(raw > hi, hi, raw))
    t = torch.tan(f * torch.tensor(math.pi / sr, dtype=arith))
    return raw, (t - 1) / (t + 1)


def cascade(x, a, stages, keep=False):
    """s_K (bs, chs, N) of the K stages with the coefficient a (bs, chs, N), sample by sample. keep: all of s_0 .. s_K, (K + 1, bs, chs, N)."""
    N = x.shape[-1]
    prev = [torch.zeros_like(x[..., 0]) for _ in range(stages + 1)]
    out = []
    for n in range(N):
        an, cur = a[..., n], x[..., n]
        new = [cur]
        for k in range(1, stages + 1):
            cur = torch.addcmul(prev[k - 1], an, cur - prev[k])
            new.append(cur)
        prev = new
        out.append(torch.stack(new) if keep else cur)
    return torch.stack(out, -1)


def phaser(x, sr, rate_hz, center_hz, depth, phase, mix, stages=4, stereo_spread=0.25, arith=torch.float64):
    """y in `arith`; x (bs, chs, N), the controls float64, (bs,) or (bs, chs)."""
    bs, chs, N = x.shape
    _, a = sweep(sr, rate_hz, center_hz, depth, phase, chs, N, stereo_spread, arith)
    xa = x.to(arith)
    m = (mix if mix.dim() == 2 else mix[:, None].expand(-1, chs))[:, :, None].to(arith)
    return (1 - m) * xa + m * cascade(xa, a, stages)


def forward_backward(x, sr, rate_hz, center_hz, depth, phase, mix, w, stages=4, stereo_spread=0.25, arith=torch.float64, per_row=False):
    """y, gx and the five control gradients for the upstream gradient w, as float64 numpy arrays. per_row: the control gradients as
    (bs, chs), each row's share; otherwise summed over the channels, (bs,)."""
    bs, chs, N = x.shape
    xl = x.detach().double().clone().requires_grad_(True)
    ctl = [t.detach().double().reshape(bs, 1).expand(bs, chs).clone().requires_grad_(True) for t in (rate_hz, center_hz, depth, phase, mix)]
    y = phaser(xl, sr, *ctl, stages=stages, stereo_spread=stereo_spread, arith=arith)
    grads = torch.autograd.grad((y.double() * w.double()).sum(), [xl] + ctl)
    out = {"y": y.detach().double().numpy(), "gx": grads[0].numpy()}
    for k, g in zip(GRADS, grads[1:]):
        out[k] = g.numpy() if per_row else g.sum(1).numpy()
    return out


def adjoint_by_hand(x, a, mix, w, stages):
    """The adjoint written out, in numpy float64 and reverse time, for one coefficient sequence: x, a, w (rows, N), mix (rows,).
         gs_K = mix w;   lam_k[n] = gs_k[n] - a[n+1] lam_k[n+1]  (lam_k[N] = 0);   gs_{k-1}[n] = a[n] lam_k[n] + lam_k[n+1]
         ga[n] = sum_k lam_k[n] (s_{k-1}[n] - s_k[n-1]);   gx = gs_0 + (1 - mix) w;   gmix = sum w (s_K - x)
    Returns gx, ga (rows, N) and gmix (rows,)."""
    x, a, w, mix = (np.asarray(t, np.float64) for t in (x, a, w, mix))
    rows, N = x.shape
    s = np.zeros((stages + 1, rows, N + 1))                # s[k][:, n + 1] = s_k[n]; column 0 is the zero state
    s[0][:, 1:] = x
    for n in range(N):
        for k in range(1, stages + 1):
            s[k][:, n + 1] = a[:, n] * (s[k - 1][:, n + 1] - s[k][:, n]) + s[k - 1][:, n]
    gs = mix[:, None] * w
    ga = np.zeros_like(x)
    for k in range(stages, 0, -1):
        lam = np.zeros((rows, N + 1))
        for n in range(N - 1, -1, -1):
            lam[:, n] = gs[:, n] - (a[:, n + 1] * lam[:, n + 1] if n + 1 < N else 0.0)
        ga += lam[:, :N] * (s[k - 1][:, 1:] - s[k][:, :N])
        gs = a * lam[:, :N] + lam[:, 1:]
    return gs + (1 - mix[:, None]) * w, ga, (w * (s[stages][:, 1:] - x)).sum(1)
