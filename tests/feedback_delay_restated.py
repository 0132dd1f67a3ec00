"""Restatement in torch of functional.feedback_delay, differentiable by autograd, on the CPU. D, i and the pole a are always float64;
`arith` is the dtype of f, a and everything after them. float64 is the oracle; float32 is the yardstick e32 of the GPU tests (what
float32 arithmetic costs when the delay is exact).

  D = clamp(sr/1000 delay_ms, 2, sr/1000 max_delay_ms),  i = floor(D),  f = D - i  (rounded to `arith`);  a = exp(-2 pi max(damping_hz, 0) / sr)
  r[n] = w_-1(f) v[n-i+1] + w_0(f) v[n-i] + w_1(f) v[n-i-1] + w_2(f) v[n-i-2]      (Catmull-Rom; v zero before sample 0)
  w[n] = x[n] + feedback r[n],   v[n] = (1 - a) w[n] + a v[n-1],   y[n] = (1 - mix) x[n] + mix r[n]
A NaN D reads at i = 2 with f = NaN.

The smallest lag is L = i - 1, so a block of at most L samples reads v of earlier blocks only: one vectorised step per block of
min(L, `block`) samples, the items that share i taken together. Inside a block the one-pole is the lower-triangular Toeplitz matrix of
the powers of a applied to (1 - a) w, plus a^(j+1) times the block's carry."""
import math

import numpy as np
import torch


def weights(f):
    """Catmull-Rom weights w_-1, w_0, w_1, w_2 at the fraction f."""
    f2, f3 = f * f, f * f * f
    return (-f3 + 2 * f2 - f) / 2, (3 * f3 - 5 * f2 + 2) / 2, (-3 * f3 + 4 * f2 + f) / 2, (f3 - f2) / 2


def dweights(f):
    """Their derivatives by f."""
    f2 = f * f
    return (-3 * f2 + 4 * f - 1) / 2, (9 * f2 - 10 * f) / 2, (-9 * f2 + 8 * f + 1) / 2, (3 * f2 - 2 * f) / 2


def delay_samples(sr, max_delay_ms):
    """H of the C ABI: the whole number of samples that bounds D."""
    return math.ceil(sr / 1000.0 * max_delay_ms)


def delay(sr, delay_ms, max_delay_ms):
    """D in float64 (differentiable: the clamp passes no gradient where it acts; a NaN stays) and i as a list of ints (2 for a NaN D)."""
    k = sr / 1000.0
    D = torch.clamp(k * delay_ms.to(torch.float64).reshape(-1), 2.0, k * max_delay_ms)
    i = [int(math.floor(d)) if d == d else 2 for d in D.detach().tolist()]
    return D, i


def pole(sr, damping_hz):
    return torch.exp(-2 * math.pi * torch.clamp(damping_hz.to(torch.float64).reshape(-1), min=0.0) / sr)


def _group(x, i, f, a, fb, block):
    """Items that share i. x (G, C, N); f, a, fb (G, 1, 1) -> r (G, C, N), all in one dtype."""
    G, C, N = x.shape
    S = min(i - 1, block)
    wrev = torch.stack(weights(f)[::-1], -1)                                                                      # (G, 1, 1, 4): w_2, w_1, w_0, w_-1
    na = 1 - a
    j = torch.arange(S)
    e = (j.view(S, 1) - j.view(1, S))
    T = torch.where(e >= 0, a.view(G, 1, 1) ** e.clamp(min=0).to(x.dtype), torch.zeros((), dtype=x.dtype))       # (G, S, S): a^(j - m), j >= m
    decay = a ** (j + 1).to(x.dtype)                                                                              # (G, 1, S)
    hist = torch.zeros(G, C, i + 2, dtype=x.dtype)                                                                # v[n0 - i - 2 .. n0 - 1]
    rs = []
    for n0 in range(0, N, S):
        s = min(S, N - n0)
        r = (hist.unfold(-1, 4, 1)[..., :s, :] * wrev).sum(-1)                 # window j: v[n-i-2], v[n-i-1], v[n-i], v[n-i+1] of n = n0 + j
        w = x[..., n0:n0 + s] + fb * r
        if S == 1:
            v = na * w + a * hist[..., -1:]
        else:
            v = torch.einsum("gjm,gcm->gcj", T[:, :s, :s], na * w) + decay[..., :s] * hist[..., -1:]
        hist = torch.cat([hist[..., s:], v], -1)
        rs.append(r)
    return torch.cat(rs, -1)


def forward(x, sr, delay_ms, feedback, damping_hz, mix, max_delay_ms=500.0, arith=torch.float64, block=512):
    """x (bs, chs, N); the four controls with bs values each -> y (bs, chs, N) in `arith`."""
    bs, chs, N = x.shape
    D, i = delay(sr, delay_ms, max_delay_ms)
    col = lambda t: t.to(arith).reshape(bs, 1, 1)
    f = col(D - torch.tensor([float(v) for v in i], dtype=torch.float64))
    a, fb, m, xa = col(pole(sr, damping_hz)), col(feedback), col(mix), x.to(arith)
    order, parts = [], []
    for iv in sorted(set(i)):
        idx = [b for b in range(bs) if i[b] == iv]
        parts.append(_group(xa[idx], iv, f[idx], a[idx], fb[idx], block))
        order += idx
    inv = torch.tensor(sorted(range(bs), key=order.__getitem__), dtype=torch.long)
    r = torch.cat(parts, 0).index_select(0, inv)
    return (1 - m) * xa + m * r


NAMES = ("y", "gx", "gdelay", "gfeedback", "gdamping", "gmix")
CTL = ("delay_ms", "feedback", "damping_hz", "mix")
# the least the kernel's parity bound is, whatever the float32 restatement's own error: the floors of the other fused effects
FLOOR = dict(y=2e-6, gx=2e-6, gdelay=1e-5, gfeedback=1e-5, gdamping=1e-5, gmix=1e-5)


def forward_backward(x, sr, delay_ms, feedback, damping_hz, mix, gy, max_delay_ms=500.0, arith=torch.float64, block=512):
    """dict of y and the gradients of sum(y * gy) by x and the four controls (each in its control's shape), as numpy float64."""
    leaves = [t.detach().cpu().to(torch.float64).requires_grad_(True) for t in (x, delay_ms, feedback, damping_hz, mix)]           # exact
    y = forward(leaves[0], sr, *leaves[1:], max_delay_ms, arith, block)
    grads = torch.autograd.grad(y, leaves, gy.detach().cpu().to(arith), allow_unused=True)          # (one sample: the line's input reaches nothing)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    return {k: v.detach().double().numpy() for k, v in zip(NAMES, (y,) + tuple(grads))}


def direct(x, sr, delay_ms, feedback, damping_hz, mix, gy, max_delay_ms=500.0):
    """The same quantities sample by sample in numpy float64, the adjoint written out by hand and run backwards in time:
         gr[n] = mix gy[n] + feedback gw[n],   q[n] = sum_k w_k(f) gr[n+i+k] + a q[n+1],   gw[n] = (1 - a) q[n],   gx[n] = (1 - mix) gy[n] + gw[n]
         g_feedback = sum gw r,  g_mix = sum gy (r - x),  g_a = sum q[n] (v[n-1] - w[n]),  g_D = sum gr[n] sum_k w'_k(f) v[n-i-k]
       delay_ms: x sr/1000, nothing where D was clamped; damping_hz: x -2 pi/sr a, nothing where damping_hz < 0."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    bs, chs, N = x.shape
    dl, fbk, dh, mx = (np.asarray(t, np.float64).reshape(bs) for t in (delay_ms, feedback, damping_hz, mix))
    k = sr / 1000.0
    out = {name: np.zeros(bs) for name in NAMES[2:]}
    out["y"], out["gx"] = np.zeros_like(x), np.zeros_like(x)
    for b in range(bs):
        raw = k * dl[b]
        D = min(max(raw, 2.0), k * max_delay_ms)
        i = math.floor(D)
        f = D - i
        a = math.exp(-2 * math.pi * max(dh[b], 0.0) / sr)
        wk, dwk = weights(f), dweights(f)
        g_a = g_D = 0.0
        for c in range(chs):
            v, r, w = np.zeros(N), np.zeros(N), np.zeros(N)
            at = lambda j: v[j] if j >= 0 else 0.0
            for n in range(N):
                r[n] = sum(wk[q] * at(n - i - kk) for q, kk in enumerate((-1, 0, 1, 2)))
                w[n] = x[b, c, n] + fbk[b] * r[n]
                v[n] = (1 - a) * w[n] + a * at(n - 1)
            out["y"][b, c] = (1 - mx[b]) * x[b, c] + mx[b] * r
            gr, q = np.zeros(N + i + 3), np.zeros(N + 1)
            for n in range(N - 1, -1, -1):
                q[n] = sum(wk[j] * gr[n + i + kk] for j, kk in enumerate((-1, 0, 1, 2))) + a * q[n + 1]
                gw = (1 - a) * q[n]
                gr[n] = mx[b] * gy[b, c, n] + fbk[b] * gw
                out["gx"][b, c, n] = (1 - mx[b]) * gy[b, c, n] + gw
                out["gfeedback"][b] += gw * r[n]
                out["gmix"][b] += gy[b, c, n] * (r[n] - x[b, c, n])
                g_a += q[n] * (at(n - 1) - w[n])
                g_D += gr[n] * sum(dwk[j] * at(n - i - kk) for j, kk in enumerate((-1, 0, 1, 2)))
        out["gdelay"][b] = k * g_D if 2.0 <= raw <= k * max_delay_ms else 0.0
        out["gdamping"][b] = -2 * math.pi / sr * a * g_a if dh[b] >= 0 else 0.0
    return out
