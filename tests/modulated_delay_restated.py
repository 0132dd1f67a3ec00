"""Restatement in torch of functional.modulated_delay, differentiable by autograd, on the CPU. Two dtype switches: `pos` for the read
position (n, theta, d, p and the floor) and `arith` for the interpolation and the sums. float64 / float64 is the oracle; float64 / float32
is the yardstick of the GPU tests (what float32 arithmetic costs when the position is exact); float32 / float32 shows what a float32
position costs. `direct` is the same thing as a double loop with hand-derived gradients, for tiny cases.

  theta = 2 pi (rate_hz n / sr + phase + c stereo_spread)
  d = clamp(sr/1000 (delay_ms + depth_ms sin theta), 0, sr/1000 max_delay_ms),  p = n - d,  i = floor(p),  f = p - i  (rounded to `arith`)
  tap_v[n] = w_-1(f) x[i-1] + w_0(f) x[i] + w_1(f) x[i+1] + w_2(f) x[i+2],   y[n] = (1 - mix) x[n] + mix (1/V) sum_v tap_v[n]
x is zero outside [0, N). Where p is not finite, i = n and f stays NaN."""
import math

import numpy as np
import torch


def weights(f):
    """Catmull-Rom weights of x[i-1], x[i], x[i+1], x[i+2] at the fraction f, stacked on a new last axis."""
    f2, f3 = f * f, f * f * f
    return torch.stack(((-f3 + 2 * f2 - f) / 2, (3 * f3 - 5 * f2 + 2) / 2, (-3 * f3 + 4 * f2 + f) / 2, (f3 - f2) / 2), -1)


def delay_samples(sr, max_delay_ms):
    """H of the C ABI: the whole number of samples that bounds d."""
    return max(1, math.ceil(sr / 1000.0 * max_delay_ms))


def forward(x, sr, delay_ms, depth_ms, rate_hz, phase, mix, max_delay_ms=40.0, stereo_spread=0.25, pos=torch.float64, arith=torch.float64):
    """x (bs, chs, N); the four voice controls with bs * V values each, mix with bs -> y (bs, chs, N) in `arith`."""
    bs, chs, N = x.shape
    V = delay_ms.numel() // bs
    dl, dp, rt, ph = (t.to(pos).reshape(bs, 1, V, 1) for t in (delay_ms, depth_ms, rate_hz, phase))
    n = torch.arange(N, dtype=pos).view(1, 1, 1, N)
    c = torch.arange(chs, dtype=pos).view(1, chs, 1, 1)
    theta = 2 * math.pi * (rt * n / sr + ph + c * stereo_spread)
    k = sr / 1000.0
    d = torch.clamp(k * (dl + dp * torch.sin(theta)), 0.0, k * max_delay_ms)
    p = n - d
    ok = torch.isfinite(p)
    i = torch.where(ok, torch.floor(p), n.expand_as(p)).detach()
    f = (p - i).to(arith)                                                # NaN where p is
    H = delay_samples(sr, max_delay_ms)
    xp = torch.nn.functional.pad(x.to(arith), (H + 2, 3))                # x[j] at xp[j + H + 2]
    idx = i.long() + (H + 2)
    xe = xp.unsqueeze(2).expand(bs, chs, V, N + H + 5)
    taps = torch.stack([torch.gather(xe, 3, idx + kk) for kk in (-1, 0, 1, 2)], -1)
    wet = (weights(f) * taps).sum(-1).sum(2) / V
    m = mix.to(arith).reshape(bs, 1, 1)
    return (1 - m) * x.to(arith) + m * wet


NAMES = ("y", "gx", "gdelay", "gdepth", "grate", "gphase", "gmix")


def forward_backward(x, sr, delay_ms, depth_ms, rate_hz, phase, mix, gy, max_delay_ms=40.0, stereo_spread=0.25, pos=torch.float64,
                     arith=torch.float64):
    """dict of y and the gradients of sum(y * gy) by x and the five controls (each in its control's shape), as numpy float64."""
    leaves = [t.detach().cpu().to(torch.float64).requires_grad_(True) for t in (x, delay_ms, depth_ms, rate_hz, phase, mix)]       # exact
    y = forward(leaves[0], sr, *leaves[1:], max_delay_ms, stereo_spread, pos, arith)
    grads = torch.autograd.grad(y, leaves, gy.detach().cpu().to(arith))
    return {k: v.detach().double().numpy() for k, v in zip(NAMES, (y,) + tuple(grads))}


def direct(x, sr, delay_ms, depth_ms, rate_hz, phase, mix, gy, max_delay_ms=40.0, stereo_spread=0.25):
    """The same quantities by a loop over (b, c, v, n) in Python floats, the gradients written out by hand: with w'_k the derivatives of the
    weights, d tap / d d = -sum_k w'_k(f) x[i+k], zero where d was clamped; the chain rule through d gives the control gradients."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    bs, chs, N = x.shape
    ctl = [np.asarray(t, np.float64).reshape(bs, -1) for t in (delay_ms, depth_ms, rate_hz, phase)]
    V = ctl[0].shape[1]
    mix = np.asarray(mix, np.float64).reshape(bs)
    k, tau = sr / 1000.0, 2 * math.pi
    out = {"y": np.zeros_like(x), "gx": np.zeros_like(x), "gmix": np.zeros(bs)}
    g = {name: np.zeros((bs, V)) for name in ("gdelay", "gdepth", "grate", "gphase")}
    at = lambda b, c, j: x[b, c, j] if 0 <= j < N else 0.0
    for b in range(bs):
        for c in range(chs):
            for n in range(N):
                wet = 0.0
                for v in range(V):
                    dl, dp, rt, ph = (t[b, v] for t in ctl)
                    th = tau * (rt * n / sr + ph + c * stereo_spread)
                    raw = k * (dl + dp * math.sin(th))
                    d = min(max(raw, 0.0), k * max_delay_ms)
                    p = n - d
                    i = math.floor(p)
                    f = p - i
                    w = ((-f ** 3 + 2 * f ** 2 - f) / 2, (3 * f ** 3 - 5 * f ** 2 + 2) / 2, (-3 * f ** 3 + 4 * f ** 2 + f) / 2, (f ** 3 - f ** 2) / 2)
                    dw = ((-3 * f ** 2 + 4 * f - 1) / 2, (9 * f ** 2 - 10 * f) / 2, (-9 * f ** 2 + 8 * f + 1) / 2, (3 * f ** 2 - 2 * f) / 2)
                    xs = [at(b, c, i + kk) for kk in (-1, 0, 1, 2)]
                    wet += sum(a * s for a, s in zip(w, xs)) / V
                    for kk, a in zip((-1, 0, 1, 2), w):
                        if 0 <= i + kk < N:
                            out["gx"][b, c, i + kk] += mix[b] / V * a * gy[b, c, n]
                    gd = -gy[b, c, n] * mix[b] / V * sum(a * s for a, s in zip(dw, xs)) if 0.0 <= raw <= k * max_delay_ms else 0.0
                    g["gdelay"][b, v] += k * gd
                    g["gdepth"][b, v] += k * gd * math.sin(th)
                    g["gphase"][b, v] += k * gd * dp * math.cos(th) * tau
                    g["grate"][b, v] += k * gd * dp * math.cos(th) * tau * n / sr
                out["y"][b, c, n] = (1 - mix[b]) * x[b, c, n] + mix[b] * wet
                out["gx"][b, c, n] += (1 - mix[b]) * gy[b, c, n]
                out["gmix"][b] += gy[b, c, n] * (wet - x[b, c, n])
    out.update(g)
    return out
