"""Restatement in torch of functional.time_varying_eq, differentiable by autograd, on the CPU: the formulas of the docstring as a loop over
the samples, in the form of tests/tvfilter_restated.py. The frame points G_j, K_j, A_j are always taken in float64. arith=torch.float64
(the default): float64 throughout - the oracle. arith=torch.float32: the frame points are rounded once to float32 and everything after
them - the interpolation, a1, a2, a3, the recurrence, the output map - is float32, which is what the kernel does; its error against the
float64 variant is the yardstick e32 of the GPU tests.

    A_j = 10^(clamp(gain_db[b,j], -40, 40) / 40);   T_j = tan(pi clamp(cutoff_hz[b,j], sr/4096, 0.49 sr) / sr);   Qc = clamp(q[b,j], 0.1, 100)
    bell: G_j = T_j, K_j = 1 / (Qc A_j)    lowshelf: G_j = T_j / sqrt A_j, K_j = 1 / Qc    highshelf: G_j = T_j sqrt A_j, K_j = 1 / Qc
    j = n // hop;   t = (n mod hop) / hop;   g = G_j + t (G_{j+1} - G_j);   likewise k from K and A from A_j
    a1 = 1 / (1 + g (g + k));   a2 = g a1;   a3 = g a2
    v3 = x[n] - ic2;   v1 = a1 ic1 + a2 v3;   v2 = ic2 + a2 ic1 + a3 v3;   ic1 <- 2 v1 - ic1;   ic2 <- 2 v2 - ic2
    y[n] = x + k (A^2 - 1) v1 (bell) | x + k (A - 1) v1 + (A^2 - 1) v2 (lowshelf) | A^2 x + k (1 - A) A v1 + (1 - A^2) v2 (highshelf)
"""
import math

import numpy as np
import torch

from tests.tvfilter_restated import FLOOR as TV_FLOOR, Q_HI, Q_LO, _clamp, _rows, clamp_bounds, control_frames, frame_gradients, interpolate  # noqa: F401

MODES = ("bell", "lowshelf", "highshelf")
CTL = ("gain_db", "cutoff_hz", "q")
GRADS = ("ggain", "gcutoff", "gq")
NAMES = ("y", "gx") + GRADS
# the floors of tvfilter_restated.FLOOR: 2e-6 of the peak for y and gx, 1e-5 for a control gradient
FLOOR = dict(y=TV_FLOOR["y"], gx=TV_FLOOR["gx"], ggain=TV_FLOOR["gcutoff"], gcutoff=TV_FLOOR["gcutoff"], gq=TV_FLOOR["gq"])
DB_MAX = 40.0


def frame_points(sr, gain_db, cutoff_hz, q, mode):
    """G, K and A at the frame points, float64, the shape of the curves."""
    lo, hi = clamp_bounds(sr)
    A = 10.0 ** (_clamp(gain_db.double(), -DB_MAX, DB_MAX) / 40.0)
    T = torch.tan(_clamp(cutoff_hz.double(), lo, hi) * (math.pi / sr))
    Qc = _clamp(q.double(), Q_LO, Q_HI)
    if mode == "bell":
        return T, 1.0 / (Qc * A), A
    return (T / torch.sqrt(A) if mode == "lowshelf" else T * torch.sqrt(A)), 1.0 / Qc, A


def output_weights(k, A, mode):
    """cx, c1, c2 with y = cx x + c1 v1 + c2 v2 (c2 None: no such term); torch or numpy."""
    if mode == "bell":
        return None, k * (A * A - 1), None
    if mode == "lowshelf":
        return None, k * (A - 1), A * A - 1
    return A * A, k * (1 - A) * A, 1 - A * A


def svf_eq(x, g, k, A, mode):
    """y (bs, chs, N) of the band with the per-sample g, k and A, (bs, chs, N), sample by sample from zero state."""
    a1 = 1 / (1 + g * (g + k))
    a2 = g * a1
    a3 = g * a2
    cx, c1, c2 = output_weights(k, A, mode)
    ic1 = ic2 = torch.zeros_like(x[..., 0])
    cols = [t.unbind(-1) for t in (x, a1, a2, a3, c1) + (() if c2 is None else (c2,)) + (() if cx is None else (cx,))]
    out = []
    for n in range(x.shape[-1]):
        xn, a1n, a2n, a3n, c1n = (c[n] for c in cols[:5])
        v3 = xn - ic2
        v1 = a1n * ic1 + a2n * v3
        v2 = ic2 + a2n * ic1 + a3n * v3
        ic1 = 2 * v1 - ic1
        ic2 = 2 * v2 - ic2
        if mode == "bell":
            out.append(xn + c1n * v1)
        elif mode == "lowshelf":
            out.append(xn + c1n * v1 + cols[5][n] * v2)
        else:
            out.append(cols[6][n] * xn + c1n * v1 + cols[5][n] * v2)
    return torch.stack(out, -1)


def time_varying_eq(x, sr, gain_db, cutoff_hz, q, hop=64, mode="bell", arith=torch.float64):
    """y in `arith`; x (bs, chs, N), the curves (bs, F) or (bs, chs, F)."""
    bs, chs, N = x.shape
    G, K, A = frame_points(sr, _rows(gain_db, chs), _rows(cutoff_hz, chs), _rows(q, chs), mode)
    g, k, a = (interpolate(P.to(arith), N, hop) for P in (G, K, A))
    return svf_eq(x.to(arith), g, k, a, mode)


def forward_backward(x, sr, gain_db, cutoff_hz, q, w, hop=64, mode="bell", arith=torch.float64, per_row=False):
    """y, gx and the three control gradients for the upstream gradient w, as float64 numpy arrays. per_row: the control gradients per
    (item, channel) row - (bs, chs, F); otherwise summed over the channels."""
    bs, chs, N = x.shape
    xl = x.detach().double().clone().requires_grad_(True)
    ctl = [t.detach().double()[:, None, :].expand(bs, chs, -1).clone().requires_grad_(True) for t in (gain_db, cutoff_hz, q)]
    y = time_varying_eq(xl, sr, *ctl, hop, mode, arith)
    grads = torch.autograd.grad((y.double() * w.double()).sum(), [xl] + ctl)
    out = {"y": y.detach().double().numpy(), "gx": grads[0].numpy()}
    for name, g in zip(GRADS, grads[1:]):
        out[name] = g.numpy() if per_row else g.sum(1).numpy()
    return out


def adjoint_by_hand(x, g, k, A, w, mode):
    """The adjoint that csrc/tveq.hip implements, written out in numpy float64 and reverse time for given per-sample g, k and A: x, g, k,
    A, w (rows, N). With lam the gradient of the state after a sample (zero after the row) and y = cx x + c1 v1 + c2 v2:
        q1 = 2 lam1 + w c1,  q2 = 2 lam2 + w c2,  gv3 = a2 q1 + a3 q2,  gx = cx w + gv3
        ga3 = q2 v3,  ga2 = q1 v3 + q2 ic1 + g ga3,  ga1 = q1 ic1 + g ga2,  gd = -a1^2 ga1        (a3 = g a2, a2 = g a1, a1 = 1 / d)
        gg = a2 ga3 + a1 ga2 + (2 g + k) gd,  gk = g gd + w dy/dk,  gA = w dy/dA
        lam <- (a1 q1 + a2 q2 - lam1,  q2 - lam2 - gv3)
    Returns gx, gg, gk, gA (rows, N)."""
    x, g, k, A, w = (np.asarray(t, np.float64) for t in (x, g, k, A, w))
    rows, N = x.shape
    a1 = 1 / (1 + g * (g + k))
    a2 = g * a1
    a3 = g * a2
    cx, c1, c2 = output_weights(k, A, mode)
    cx = np.ones_like(x) if cx is None else cx
    c2 = np.zeros_like(x) if c2 is None else c2
    z1, z2, V1, V2 = (np.zeros((rows, N)) for _ in range(4))
    ic1, ic2 = np.zeros(rows), np.zeros(rows)
    for n in range(N):
        z1[:, n], z2[:, n] = ic1, ic2
        v3 = x[:, n] - ic2
        V1[:, n] = a1[:, n] * ic1 + a2[:, n] * v3
        V2[:, n] = ic2 + a2[:, n] * ic1 + a3[:, n] * v3
        ic1, ic2 = 2 * V1[:, n] - ic1, 2 * V2[:, n] - ic2
    if mode == "bell":
        dk, dA = (A * A - 1) * V1, 2 * A * k * V1
    elif mode == "lowshelf":
        dk, dA = (A - 1) * V1, k * V1 + 2 * A * V2
    else:
        dk, dA = (1 - A) * A * V1, 2 * A * x + k * (1 - 2 * A) * V1 - 2 * A * V2
    gx, gg, gk = (np.zeros((rows, N)) for _ in range(3))
    l1, l2 = np.zeros(rows), np.zeros(rows)
    for n in range(N - 1, -1, -1):
        s = np.s_[:, n]
        q1, q2 = 2 * l1 + w[s] * c1[s], 2 * l2 + w[s] * c2[s]
        gv3 = a2[s] * q1 + a3[s] * q2
        gx[s] = cx[s] * w[s] + gv3
        v3 = x[s] - z2[s]
        ga3 = q2 * v3
        ga2 = q1 * v3 + q2 * z1[s] + g[s] * ga3
        ga1 = q1 * z1[s] + g[s] * ga2
        gd = -a1[s] * a1[s] * ga1
        gg[s] = a2[s] * ga3 + a1[s] * ga2 + (2 * g[s] + k[s]) * gd
        gk[s] = g[s] * gd + w[s] * dk[s]
        l1, l2 = a1[s] * q1 + a2[s] * q2 - l1, q2 - l2 - gv3
    return gx, gg, gk, w * dA


def curve_gradients(sr, gain_db, cutoff_hz, q, gG, gK, gA, mode):
    """From the frame gradients of G, K and A to those of the three curves, exactly zero where the frame value was clamped; numpy float64.
        bell:      gT = gG,         gQ = -gK K / Q,  gA' = gA - gK K / A
        lowshelf:  gT = gG / sqrt A, gQ = -gK / Q^2,  gA' = gA - gG G / (2 A)
        highshelf: gT = gG sqrt A,   gQ = -gK / Q^2,  gA' = gA + gG G / (2 A)
        ggain = gA' A ln 10 / 40,   gcutoff = gT (pi / sr)(1 + T^2)"""
    a, c, qq = (np.asarray(t, np.float64) for t in (gain_db, cutoff_hz, q))
    lo, hi = clamp_bounds(sr)
    A = 10.0 ** (np.clip(a, -DB_MAX, DB_MAX) / 40.0)
    T = np.tan(np.clip(c, lo, hi) * (math.pi / sr))
    Q = np.clip(qq, Q_LO, Q_HI)
    if mode == "bell":
        K = 1.0 / (Q * A)
        gT, gQ, gAf = gG, -gK * K / Q, gA - gK * K / A
    else:
        r = np.sqrt(A)
        G = T / r if mode == "lowshelf" else T * r
        h = gG * G / (2 * A)
        gT, gQ, gAf = (gG / r, -gK / (Q * Q), gA - h) if mode == "lowshelf" else (gG * r, -gK / (Q * Q), gA + h)
    return (np.where((a < -DB_MAX) | (a > DB_MAX), 0.0, gAf * A * math.log(10.0) / 40.0),
            np.where((c < lo) | (c > hi), 0.0, gT * (math.pi / sr) * (1 + T * T)), np.where((qq < Q_LO) | (qq > Q_HI), 0.0, gQ))


def rbj(kind, f, Q, gain_db, sr):
    """The Audio EQ Cookbook's peakingEQ, lowShelf and highShelf with alpha = sin w0 / 2Q, for "bell", "lowshelf", "highshelf": (b, a)."""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2 * math.pi * f / sr
    al, c, r = math.sin(w0) / (2 * Q), math.cos(w0), 2 * math.sqrt(A) * math.sin(w0) / (2 * Q)
    if kind == "bell":
        return np.array([1 + al * A, -2 * c, 1 - al * A]), np.array([1 + al / A, -2 * c, 1 - al / A])
    if kind == "lowshelf":
        return (np.array([A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r)]),
                np.array([(A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r]))
    return (np.array([A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)]),
            np.array([(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r]))
