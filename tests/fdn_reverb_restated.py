"""Restatement in torch of functional.fdn_reverb, differentiable by autograd, on the CPU. The line gains g_k and the pole a are always
float64; `arith` is the dtype they are rounded to and of everything after them. float64 is the oracle; float32 is the yardstick e32 of the
GPU tests (what float32 arithmetic costs).

  T = clamp(decay_s, 0.01, 100),  g_k = 10^(-3 m_k / (sr T)),  a = exp(-2 pi max(damping_hz, 0) / sr)
  r_k[n] = v_k[n - m_k],  u_k[n] = g_k r_k[n],  w_k[n] = x[n] + u_k[n] - (2/K) sum_j u_j[n],  v_k[n] = (1 - a) w_k[n] + a v_k[n-1]
  wet[n] = K^(-1/2) sum_k s_ck r_k[n],  s_ck = (-1)^(k c) if decorrelate else 1,   y[n] = (1 - mix) x[n] + mix wet[n]

The smallest lag is min m_k, so a block of at most that many samples reads v of earlier blocks only: one vectorised step per block of
min(min m_k, `block`) samples, as tests/feedback_delay_restated._group. Inside a block the one-pole is the lower-triangular Toeplitz
matrix of the powers of a applied to (1 - a) w_k, plus a^(j+1) times the block's carry; a block of one sample is the recurrence itself
(no matrix product: a NaN or inf sample then reaches exactly what it reaches sample by sample)."""
import math

import numpy as np
import torch

NAMES = ("y", "gx", "gdecay", "gdamping", "gmix")
CTL = ("decay_s", "damping_hz", "mix")
# the least the kernel's parity bound is, whatever the float32 restatement's own error: the floors of the other fused effects
FLOOR = dict(y=2e-6, gx=2e-6, gdecay=1e-5, gdamping=1e-5, gmix=1e-5)


def gains(sr, decay_s, delays):
    """g (bs, K) in float64, differentiable. The clamps are comparisons (torch.clamp gives a NaN no gradient): no gradient where they act;
    a NaN is not a clamped value, it stays and reaches the gradient."""
    d = decay_s.to(torch.float64).reshape(-1, 1)
    T = torch.where(d < 0.01, torch.full_like(d, 0.01), torch.where(d > 100.0, torch.full_like(d, 100.0), d))
    m = torch.tensor([float(v) for v in delays], dtype=torch.float64).reshape(1, -1)
    return 10.0 ** (-3.0 * m / (sr * T))


def pole(sr, damping_hz):
    d = damping_hz.to(torch.float64).reshape(-1)
    return torch.exp(-2 * math.pi * torch.where(d < 0.0, torch.zeros_like(d), d) / sr)


def signs(chs, K, decorrelate, dtype=torch.float64):
    """s (chs, K)."""
    c, k = torch.arange(chs).view(-1, 1), torch.arange(K).view(1, -1)
    return torch.where((c * k) % 2 == 1, -1.0, 1.0).to(dtype) if decorrelate else torch.ones(chs, K, dtype=dtype)


def forward(x, sr, decay_s, damping_hz, mix, delays, decorrelate=True, arith=torch.float64, block=512):
    """x (bs, chs, N); the three controls with bs values each; delays: K ints -> y (bs, chs, N) in `arith`."""
    bs, chs, N = x.shape
    delays = [int(m) for m in delays]
    K = len(delays)
    g = gains(sr, decay_s, delays).to(arith)                                 # (bs, K)
    a = pole(sr, damping_hz).to(arith).reshape(bs, 1, 1)
    mx, xa = mix.to(arith).reshape(bs, 1, 1), x.to(arith)
    na = 1 - a
    S = max(1, min(min(delays), block))
    j = torch.arange(S)
    e = j.view(S, 1) - j.view(1, S)
    T = torch.where(e >= 0, a.view(bs, 1, 1) ** e.clamp(min=0).to(arith), torch.zeros((), dtype=arith))          # (bs, S, S): a^(j - m), j >= m
    decay = a ** (j + 1).to(arith)                                           # (bs, 1, S)
    sg = signs(chs, K, decorrelate, arith)                                   # (chs, K)
    kinv, c2 = torch.tensor(1.0 / math.sqrt(K), dtype=torch.float64).to(arith), torch.tensor(2.0 / K, dtype=torch.float64).to(arith)
    hist = [torch.zeros(bs, chs, m, dtype=arith) for m in delays]           # v_k[n0 - m_k .. n0 - 1]
    wets = []
    for n0 in range(0, N, S):
        s = min(S, N - n0)
        r = [h[..., :s] for h in hist]
        u = [g[:, k].view(bs, 1, 1) * r[k] for k in range(K)]
        su = u[0]
        for k in range(1, K):
            su = su + u[k]
        wet = sg[:, 0].view(1, chs, 1) * r[0]
        for k in range(1, K):
            wet = wet + sg[:, k].view(1, chs, 1) * r[k]
        wets.append(kinv * wet)
        xs = xa[..., n0:n0 + s]
        for k in range(K):
            w = xs + u[k] - c2 * su
            if S == 1:
                v = na * w + a * hist[k][..., -1:]
            else:
                v = torch.einsum("bjm,bcm->bcj", T[:, :s, :s], na * w) + decay[..., :s] * hist[k][..., -1:]
            hist[k] = torch.cat([hist[k][..., s:], v], -1)
    wet = torch.cat(wets, -1) if wets else xa
    return (1 - mx) * xa + mx * wet


def forward_backward(x, sr, decay_s, damping_hz, mix, delays, gy, decorrelate=True, arith=torch.float64, block=512):
    """dict of y and the gradients of sum(y * gy) by x and the three controls (each in its control's shape), as numpy float64."""
    leaves = [t.detach().cpu().to(torch.float64).requires_grad_(True) for t in (x, decay_s, damping_hz, mix)]                  # exact
    y = forward(leaves[0], sr, *leaves[1:], delays, decorrelate, arith, block)
    grads = torch.autograd.grad(y, leaves, gy.detach().cpu().to(arith), allow_unused=True)
    grads = [torch.zeros_like(t) if q is None else q for q, t in zip(grads, leaves)]
    return {k: v.detach().double().numpy() for k, v in zip(NAMES, (y,) + tuple(grads))}


def direct(x, sr, decay_s, damping_hz, mix, delays, gy, decorrelate=True):
    """The same quantities sample by sample in numpy float64, the adjoint written out by hand and run backwards in time (the Householder
    matrix is symmetric), lam_k[N] = 0 and rho_k = 0 at and past N:
         lam_k[n] = a lam_k[n+1] + rho_k[n + m_k],   om_k[n] = (1 - a) lam_k[n]
         rho_k[n] = K^(-1/2) s_ck mix gy[n] + g_k (om_k[n] - (2/K) sum_j om_j[n]),   gx[n] = (1 - mix) gy[n] + sum_k om_k[n]
         g_{g_k} = sum_n r_k[n] (om_k[n] - (2/K) sum_j om_j[n]),  g_a = sum_k sum_n lam_k[n] (v_k[n-1] - w_k[n]),  g_mix = sum_n gy[n] (wet[n] - x[n])
       decay_s: sum_k g_{g_k} g_k ln(10) 3 m_k / (sr T^2), nothing where decay_s was clamped; damping_hz: x -2 pi/sr a, nothing where
       damping_hz < 0 or +inf."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    bs, chs, N = x.shape
    dc, dh, mx = (np.asarray(t, np.float64).reshape(bs) for t in (decay_s, damping_hz, mix))
    ms = [int(m) for m in delays]
    K = len(ms)
    out = {name: np.zeros(bs) for name in NAMES[2:]}
    out["y"], out["gx"] = np.zeros_like(x), np.zeros_like(x)
    for b in range(bs):
        T = min(max(dc[b], 0.01), 100.0)
        g = [10.0 ** (-3.0 * m / (sr * T)) for m in ms]
        a = math.exp(-2 * math.pi * max(dh[b], 0.0) / sr)
        g_g, g_a = np.zeros(K), 0.0
        for c in range(chs):
            sg = [(-1.0) ** (k * c) if decorrelate else 1.0 for k in range(K)]
            v, r, w, wet = np.zeros((K, N)), np.zeros((K, N)), np.zeros((K, N)), np.zeros(N)
            for n in range(N):
                for k in range(K):
                    r[k, n] = v[k, n - ms[k]] if n - ms[k] >= 0 else 0.0
                su = sum(g[k] * r[k, n] for k in range(K))
                for k in range(K):
                    w[k, n] = x[b, c, n] + g[k] * r[k, n] - 2.0 / K * su
                    v[k, n] = (1 - a) * w[k, n] + a * (v[k, n - 1] if n > 0 else 0.0)
                wet[n] = sum(sg[k] * r[k, n] for k in range(K)) / math.sqrt(K)
            out["y"][b, c] = (1 - mx[b]) * x[b, c] + mx[b] * wet
            rho, lam = np.zeros((K, N + max(ms) + 1)), np.zeros((K, N + 1))
            for n in range(N - 1, -1, -1):
                for k in range(K):
                    lam[k, n] = a * lam[k, n + 1] + rho[k, n + ms[k]]
                om = (1 - a) * lam[:, n]
                so = sum(om[k] for k in range(K))
                for k in range(K):
                    z = om[k] - 2.0 / K * so
                    rho[k, n] = sg[k] / math.sqrt(K) * mx[b] * gy[b, c, n] + g[k] * z
                    g_g[k] += r[k, n] * z
                    g_a += lam[k, n] * ((v[k, n - 1] if n > 0 else 0.0) - w[k, n])
                out["gx"][b, c, n] = (1 - mx[b]) * gy[b, c, n] + so
                out["gmix"][b] += gy[b, c, n] * (wet[n] - x[b, c, n])
        clamped, off = dc[b] < 0.01 or dc[b] > 100.0, dh[b] < 0.0 or dh[b] == math.inf                 # a NaN is neither
        out["gdecay"][b] = 0.0 if clamped else sum(g_g[k] * g[k] * math.log(10.0) * 3.0 * ms[k] / (sr * T * T) for k in range(K))
        out["gdamping"][b] = 0.0 if off else -2 * math.pi / sr * a * g_a
    return out
