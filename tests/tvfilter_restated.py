"""Restatement in torch of functional.time_varying_filter, differentiable by autograd, on the CPU: the formulas of the docstring as a loop
over the samples. The frame points G_j, K_j are always taken in float64. arith=torch.float64 (the default): float64 throughout - the
oracle. arith=torch.float32: the frame points are rounded once to float32 and everything after them - the interpolation, a1, a2, a3, the
recurrence, the mix - is float32, which is what the kernel does; its error against the float64 variant is the yardstick e32 of the GPU
tests.

    G_j = tan(pi clamp(cutoff_hz[b,j], sr/4096, 0.49 sr) / sr);   K_j = 1 / clamp(q[b,j], 0.1, 100)
    j = n // hop;   t = (n mod hop) / hop;   g = G_j + t (G_{j+1} - G_j);   k = K_j + t (K_{j+1} - K_j)
    a1 = 1 / (1 + g (g + k));   a2 = g a1;   a3 = g a2
    v3 = x[n] - ic2;   v1 = a1 ic1 + a2 v3;   v2 = ic2 + a2 ic1 + a3 v3;   ic1 <- 2 v1 - ic1;   ic2 <- 2 v2 - ic2
    w = v2 (lowpass) | k v1 (bandpass) | x - k v1 - v2 (highpass) | x - k v1 (notch);   y[n] = (1 - mix) x[n] + mix w
"""
import math

import numpy as np
import torch

MODES = ("lowpass", "bandpass", "highpass", "notch")
CTL = ("cutoff_hz", "q", "mix")
GRADS = ("gcutoff", "gq", "gmix")
NAMES = ("y", "gx") + GRADS
# the least the kernel's parity bound is, whatever the float32 restatement's own error: the floors of the other fused effects
FLOOR = dict(y=2e-6, gx=2e-6, gcutoff=1e-5, gq=1e-5, gmix=1e-5)
Q_LO, Q_HI = 0.1, 100.0


def control_frames(seq_len, hop):
    return -(-seq_len // hop) + 1


def clamp_bounds(sr):
    return sr / 4096.0, 0.49 * sr


def _clamp(v, lo, hi):
    """Two comparisons: a NaN stays, and a clamped value passes no gradient on."""
    lo, hi = torch.tensor(lo, dtype=v.dtype), torch.tensor(hi, dtype=v.dtype)
    return torch.where(v < lo, lo, torch.where(v > hi, hi, v))


def frame_points(sr, cutoff_hz, q):
    """G and K at the frame points, float64, the shape of the curves."""
    lo, hi = clamp_bounds(sr)
    return torch.tan(_clamp(cutoff_hz.double(), lo, hi) * (math.pi / sr)), 1.0 / _clamp(q.double(), Q_LO, Q_HI)


def interpolate(P, N, hop):
    """A curve's frame points (..., F) at the N samples: P_j + t (P_{j+1} - P_j), in P's dtype; t = (n mod hop) / hop is exact in float32."""
    assert P.shape[-1] == control_frames(N, hop)
    n = torch.arange(N)
    j = n // hop
    t = ((n % hop).double() / hop).to(P.dtype)
    return P[..., j] + t * (P[..., j + 1] - P[..., j])


def svf(x, g, k, mode):
    """w (bs, chs, N) of the filter with the per-sample g and k, (bs, chs, N), sample by sample from zero state."""
    a1 = 1 / (1 + g * (g + k))
    a2 = g * a1
    a3 = g * a2
    ic1 = ic2 = torch.zeros_like(x[..., 0])
    out = []
    for xn, kn, a1n, a2n, a3n in zip(x.unbind(-1), k.unbind(-1), a1.unbind(-1), a2.unbind(-1), a3.unbind(-1)):
        v3 = xn - ic2
        v1 = a1n * ic1 + a2n * v3
        v2 = ic2 + a2n * ic1 + a3n * v3
        ic1 = 2 * v1 - ic1
        ic2 = 2 * v2 - ic2
        out.append({"lowpass": lambda: v2, "bandpass": lambda: kn * v1, "highpass": lambda: xn - kn * v1 - v2, "notch": lambda: xn - kn * v1}[mode]())
    return torch.stack(out, -1)


def _rows(c, chs):
    """A curve (bs, F) or, a value per row, (bs, chs, F) - how the tests separate the channels' shares of a control gradient."""
    return c if c.dim() == 3 else c[:, None, :].expand(-1, chs, -1)


def time_varying_filter(x, sr, cutoff_hz, q, mix, hop=64, mode="lowpass", arith=torch.float64):
    """y in `arith`; x (bs, chs, N), the curves (bs, F) or (bs, chs, F), mix (bs,) or (bs, chs)."""
    bs, chs, N = x.shape
    G, K = frame_points(sr, _rows(cutoff_hz, chs), _rows(q, chs))
    g, k = interpolate(G.to(arith), N, hop), interpolate(K.to(arith), N, hop)
    xa = x.to(arith)
    m = (mix if mix.dim() == 2 else mix[:, None].expand(-1, chs))[:, :, None].to(arith)
    return (1 - m) * xa + m * svf(xa, g, k, mode)


def forward_backward(x, sr, cutoff_hz, q, mix, w, hop=64, mode="lowpass", arith=torch.float64, per_row=False):
    """y, gx and the three control gradients for the upstream gradient w, as float64 numpy arrays. per_row: the control gradients per
    (item, channel) row - (bs, chs, F) and (bs, chs); otherwise summed over the channels."""
    bs, chs, N = x.shape
    xl = x.detach().double().clone().requires_grad_(True)
    cut, qq = (t.detach().double()[:, None, :].expand(bs, chs, -1).clone().requires_grad_(True) for t in (cutoff_hz, q))
    mx = mix.detach().double().reshape(bs, 1).expand(bs, chs).clone().requires_grad_(True)
    y = time_varying_filter(xl, sr, cut, qq, mx, hop, mode, arith)
    grads = torch.autograd.grad((y.double() * w.double()).sum(), [xl, cut, qq, mx])
    out = {"y": y.detach().double().numpy(), "gx": grads[0].numpy()}
    for name, g in zip(GRADS, grads[1:]):
        out[name] = g.numpy() if per_row else g.sum(1).numpy()
    return out


def output_map(g, k, mode):
    """p (2, ...) and r with w[n] = p[n] . z[n-1] + r[n] x[n], and a1, a2, a3; numpy."""
    a1 = 1 / (1 + g * (g + k))
    a2 = g * a1
    a3 = g * a2
    if mode == "lowpass":
        p, r = (a2, 1 - a3), a3
    elif mode == "bandpass":
        p, r = (k * a1, -k * a2), k * a2
    elif mode == "highpass":
        p, r = (-k * a1 - a2, k * a2 - (1 - a3)), 1 - k * a2 - a3
    else:
        p, r = (-k * a1, k * a2), 1 - k * a2
    return a1, a2, a3, np.stack(p), r


def adjoint_by_hand(x, g, k, mix, w, mode):
    """The adjoint written out, in numpy float64 and reverse time, for given per-sample g and k: x, g, k, w (rows, N), mix (rows,). With
    z = (ic1, ic2), z[n] = A[n] z[n-1] + b[n] x[n], A = [[2 a1 - 1, -2 a2], [2 a2, 1 - 2 a3]], b = (2 a2, 2 a3), gw = mix w:
        lam[n] = A[n+1]^T lam[n+1] + p[n+1] gw[n+1]  (lam[N-1] = 0);   gx[n] = (1 - mix) w[n] + b[n] . lam[n] + r[n] gw[n]
        gA[n] = lam[n] z[n-1]^T,  gb[n] = lam[n] x[n],  gp[n] = gw[n] z[n-1],  gr[n] = gw[n] x[n];   gmix = sum w (filter output - x)
    chained through a1, a2, a3 to g and k. Returns gx, gg, gk (rows, N) and gmix (rows,)."""
    x, g, k, w, mix = (np.asarray(t, np.float64) for t in (x, g, k, w, mix))
    rows, N = x.shape
    a1, a2, a3, p, r = output_map(g, k, mode)
    A = np.array([[2 * a1 - 1, -2 * a2], [2 * a2, 1 - 2 * a3]])          # (2, 2, rows, N)
    b = np.stack([2 * a2, 2 * a3])
    z = np.zeros((2, rows, N + 1))                                        # z[:, :, n] is the state before sample n
    for n in range(N):
        z[:, :, n + 1] = np.einsum("ijr,jr->ir", A[:, :, :, n], z[:, :, n]) + b[:, :, n] * x[:, n]
    zp = z[:, :, :N]
    out = (p * zp).sum(0) + r * x
    gw = mix[:, None] * w
    lam = np.zeros((2, rows, N))
    for n in range(N - 2, -1, -1):
        lam[:, :, n] = np.einsum("jir,jr->ir", A[:, :, :, n + 1], lam[:, :, n + 1]) + p[:, :, n + 1] * gw[:, n + 1]
    gx = (1 - mix[:, None]) * w + (b * lam).sum(0) + r * gw
    gA = lam[:, None] * zp[None]                                          # gA[i][j] = lam_i z_j
    gb, gp, gr = lam * x, gw * zp, gw * x
    # a1, a2, a3 as they stand in A, b, p and r; then k where it stands beside them
    ga1 = 2 * gA[0][0]
    ga2 = -2 * gA[0][1] + 2 * gA[1][0] + 2 * gb[0]
    ga3 = -2 * gA[1][1] + 2 * gb[1]
    gk = np.zeros_like(x)
    if mode == "lowpass":
        ga2, ga3 = ga2 + gp[0], ga3 - gp[1] + gr
    elif mode == "bandpass":
        ga1, ga2 = ga1 + k * gp[0], ga2 - k * gp[1] + k * gr
        gk = a1 * gp[0] - a2 * gp[1] + a2 * gr
    elif mode == "highpass":
        ga1, ga2, ga3 = ga1 - k * gp[0], ga2 - gp[0] + k * gp[1] - k * gr, ga3 + gp[1] - gr
        gk = -a1 * gp[0] + a2 * gp[1] - a2 * gr
    else:
        ga1, ga2 = ga1 - k * gp[0], ga2 + k * gp[1] - k * gr
        gk = -a1 * gp[0] + a2 * gp[1] - a2 * gr
    ga2 = ga2 + g * ga3                                                   # a3 = g a2
    ga1 = ga1 + g * ga2                                                   # a2 = g a1
    gd = -a1 * a1 * ga1                                                   # a1 = 1 / (1 + g (g + k))
    gg = a2 * ga3 + a1 * ga2 + (2 * g + k) * gd
    return gx, gg, gk + g * gd, (w * (out - x)).sum(1)


def frame_gradients(gs, hop, F):
    """A per-sample gradient (rows, N) of an interpolated curve collected at its frame points (rows, F): frame point j takes (1 - t) of its
    own interval and t of the one before it."""
    rows, N = gs.shape
    n = np.arange(N)
    j, t = n // hop, (n % hop) / hop
    out = np.zeros((rows, F))
    np.add.at(out, (slice(None), j), (1 - t) * gs)
    np.add.at(out, (slice(None), j + 1), t * gs)
    return out


def curve_gradients(sr, cutoff_hz, q, gG, gK):
    """gcutoff_j = gG_j (pi / sr)(1 + G_j^2) and gq_j = -gK_j / q_j^2, exactly zero where the frame value was clamped; numpy float64."""
    c, qq = np.asarray(cutoff_hz, np.float64), np.asarray(q, np.float64)
    lo, hi = clamp_bounds(sr)
    G = np.tan(np.clip(c, lo, hi) * (math.pi / sr))
    return np.where((c < lo) | (c > hi), 0.0, gG * (math.pi / sr) * (1 + G * G)), np.where((qq < Q_LO) | (qq > Q_HI), 0.0, -gK / (qq * qq))
