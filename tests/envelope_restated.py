"""Restatement of functional.envelope_follower on the CPU, in two forms.

`envelope` is the definition as a loop over the samples, in torch float64, differentiable by autograd - the oracle:

    t = clamp(smoothing_ms, 0.1, 10000);   a = exp(-ln 9 / (sr t / 1000))
    p[m] = max_c |x[b,c,m]| (the lowest channel wins a tie) | mean_c x[b,c,m]^2;   p = 0 from sample N on
    e[m] = a e[m-1] + (1 - a) p[m],  e[-1] = 0;   E[b,j] = e[j hop],  j = 0 .. F-1,  F = ceil(N / hop) + 1

`blocked` is the form the kernel evaluates, by hand and without autograd, in numpy at a chosen precision `dt`:

    E_j = a^h E_{j-1} + z_j,   z_j = sum_{i=1..h} (1-a) a^(h-i) p[(j-1) h + i],   E_0 = (1-a) p[0]
    D_j = dE_j/da = h a^(h-1) E_{j-1} + a^h D_{j-1} + dz_j,   dz_j = sum_i [-a^(h-i) + (1-a)(h-i) a^(h-i-1)] p[(j-1) h + i],   D_0 = -p[0]
    g_smoothing = (da/dt) sum_j gE_j D_j;   Lambda_j = gE_j + a^h Lambda_{j+1};   gx[b,c,m] = (1-a) a^(j h - m) Lambda_j dp/dx,  j = ceil(m / h)

with the kernel's arithmetic: a, 1 - a and the weights from float64, rounded once to `dt`; a weight is the product of two such factors,
a^d0 for the run of 8 samples it lies in (d0 samples between the run's end and the block's) and (1-a) a^r inside the run; block sums in
`dt`; both frame scans in float64, rounded once at the end. dt = float64 is the blocked identity itself (tests/test_envelope_cpu.py
holds it against the sample loop); dt = float32 is the yardstick e32 of the GPU tests. The float32 SAMPLE LOOP is no yardstick: its
1 - a and its thousands of roundings put it 1e-5 .. 1e-4 of the peak away once 1 - a < 1e-3.
"""
import math

import numpy as np
import torch

DETECTORS = ("peak", "power")
CTL = ("smoothing_ms",)
GRADS = ("gsm",)
NAMES = ("E", "gx") + GRADS
# the least the kernel's parity bound is, whatever the float32 restatement's own error: the floors of the other fused effects
FLOOR = dict(E=2e-6, gx=2e-6, gsm=1e-5)
LN9 = math.log(9.0)
T_LO, T_HI = 0.1, 10000.0
RUN = 8


def control_frames(seq_len, hop):
    return -(-seq_len // hop) + 1


def _clamp(v, lo, hi):
    """Two comparisons: a NaN stays, and a clamped value passes no gradient on."""
    lo, hi = torch.tensor(lo, dtype=v.dtype), torch.tensor(hi, dtype=v.dtype)
    return torch.where(v < lo, lo, torch.where(v > hi, hi, v))


def level(x, detector):
    """p (bs, N) of x (bs, chs, N), torch, differentiable: the winner alone takes the gradient of "peak"."""
    if detector == "power":
        p = x[:, 0] * x[:, 0]
        for c in range(1, x.shape[1]):
            p = p + x[:, c] * x[:, c]
        return p * (1.0 / x.shape[1])
    p = x[:, 0].abs()
    for c in range(1, x.shape[1]):
        a = x[:, c].abs()
        p = torch.where((a > p) | torch.isnan(a), a, p)
    return p


def envelope(x, sr, smoothing_ms, hop=64, detector="peak"):
    """E (bs, F), float64: the sample loop."""
    bs, chs, N = x.shape
    F = control_frames(N, hop)
    t = _clamp(smoothing_ms.double().reshape(bs), T_LO, T_HI)
    lna = -LN9 / (sr * t / 1000.0)
    a, oma = torch.exp(lna), -torch.expm1(lna)
    p = level(x.double(), detector)
    e = torch.zeros(bs, dtype=torch.float64)
    zero = torch.zeros(bs, dtype=torch.float64)
    out = []
    for m in range((F - 1) * hop + 1):
        e = a * e + oma * (p[:, m] if m < N else zero)
        if m % hop == 0:
            out.append(e)
    return torch.stack(out, -1)


def item_constants(sr, smoothing_ms):
    """ln a, 1 - a, t and whether t was clamped, float64 numpy (bs,), from the control as the kernel reads it (float32)."""
    s = np.asarray(smoothing_ms, np.float32).astype(np.float64).reshape(-1)
    clamped = (s < T_LO) | (s > T_HI)
    t = np.where(s < T_LO, T_LO, np.where(s > T_HI, T_HI, s))
    lna = -LN9 / (sr * t / 1000.0)
    return lna, -np.expm1(lna), t, clamped


def _pow(lna, k):
    """a^k for integer k >= 0 (arrays broadcast), 1 at k = 0 whatever a is."""
    k = np.asarray(k, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(k == 0, 1.0, np.exp(k * lna))


def level_np(x, detector, dt):
    """p (bs, N) and dp/dx (bs, chs, N) in dt."""
    x = np.asarray(x, dt)
    bs, chs, N = x.shape
    if detector == "power":
        p = x[:, 0] * x[:, 0]
        for c in range(1, chs):
            p = p + x[:, c] * x[:, c]
        invc = dt(1.0) / dt(chs)
        return p * invc, dt(2.0) * invc * x
    p, cs = np.abs(x[:, 0]), np.zeros((bs, N), np.int64)
    for c in range(1, chs):
        a = np.abs(x[:, c])
        take = a > p
        cs = np.where(take, c, cs)
        p = np.where(take | np.isnan(a), a, p)
    d = np.zeros_like(x)
    for c in range(chs):
        d[:, c] = np.where(cs == c, np.sign(x[:, c]), 0)
    return p, d


def block_sums(p, lna, oma, hop, dt):
    """z and dz (bs, F) in dt of the level p (bs, (F-1) hop + 1) in dt: entry 0 is sample 0, entry j the block that ends at sample j hop."""
    bs = p.shape[0]
    F = (p.shape[1] - 1) // hop + 1
    r = np.arange(RUN - 1, -1, -1)                                      # the sample r before its run's end
    ar = _pow(lna[:, None], r[None])
    wz = (oma[:, None] * ar).astype(dt)
    wd = (-ar + np.where(r[None] > 0, oma[:, None] * r[None] * _pow(lna[:, None], np.maximum(r[None] - 1, 0)), 0.0)).astype(dt)
    wa = ar.astype(dt)
    d0 = np.arange(hop - RUN, -1, -RUN)                                 # of the runs of a block, in time order
    a0 = _pow(lna[:, None], d0[None]).astype(dt)
    b0 = np.where(d0[None] > 0, oma[:, None] * d0[None] * _pow(lna[:, None], np.maximum(d0[None] - 1, 0)), 0.0).astype(dt)
    runs = p[:, 1:].reshape(bs, F - 1, hop // RUN, RUN)
    fsum = lambda v: np.add.reduce(v, axis=-1, dtype=dt)
    s1, s2, s3 = (fsum(runs * w[:, None, None, :]) for w in (wz, wd, wa))
    z = np.concatenate([(wz[:, -1] * p[:, 0])[:, None], fsum(a0[:, None] * s1)], 1)
    dz = np.concatenate([(-p[:, 0])[:, None], fsum(a0[:, None] * s2 + b0[:, None] * s3)], 1)
    return z.astype(dt), dz.astype(dt)


def blocked(x, sr, smoothing_ms, w, hop=64, detector="peak", dt=np.float32):
    """E, D, gx and gsm of the blocked form for the upstream gradient w (bs, F), as float64 numpy arrays of values held in dt."""
    x = np.asarray(x)
    bs, chs, N = x.shape
    F = control_frames(N, hop)
    lna, oma, t, clamped = item_constants(sr, smoothing_ms)
    p, dpdx = level_np(x, detector, dt)
    pp = np.zeros((bs, (F - 1) * hop + 1), dt)
    pp[:, :N] = p
    z, dz = block_sums(pp, lna, oma, hop, dt)
    A, Bc = _pow(lna, hop), hop * _pow(lna, hop - 1)
    E, D = np.zeros((bs, F)), np.zeros((bs, F))
    e, d = z[:, 0].astype(np.float64), dz[:, 0].astype(np.float64)
    E[:, 0], D[:, 0] = e, d
    for j in range(1, F):
        d = Bc * e + A * d + dz[:, j]
        e = A * e + z[:, j]
        E[:, j], D[:, j] = e, d
    E, D = E.astype(dt), D.astype(dt)
    gE = np.asarray(w, dt).astype(np.float64)
    lam, v = np.zeros((bs, F)), np.zeros(bs)
    for j in range(F - 1, -1, -1):
        v = gE[:, j] + A * v
        lam[:, j] = v
    lam = lam.astype(dt)
    m = np.arange(N)
    j = -(-m // hop)
    dist = j * hop - m
    hi = _pow(lna[:, None], (dist - dist % RUN)[None]).astype(dt)
    lo = (oma[:, None] * _pow(lna[:, None], (dist % RUN)[None])).astype(dt)
    gx = (hi * lo * lam[:, j])[:, None, :] * dpdx
    dadt = np.exp(lna) * LN9 * 1000.0 / (sr * t * t)
    gsm = np.where(clamped, 0.0, (gE * D.astype(np.float64)).sum(1) * dadt).astype(dt)
    f = lambda v: np.asarray(v, np.float64)
    return dict(E=f(E), D=f(D), gx=f(gx), gsm=f(gsm))


def forward_backward(x, sr, smoothing_ms, w, hop=64, detector="peak", arith=torch.float64):
    """E, gx and gsm for the upstream gradient w (bs, F), as float64 numpy arrays. arith=torch.float64: the sample loop and autograd;
    arith=torch.float32: the kernel's arithmetic, `blocked` in float32."""
    if arith is torch.float32:
        r = blocked(x.detach().numpy(), sr, smoothing_ms.detach().numpy(), w.detach().numpy(), hop, detector, np.float32)
        return {k: r[k] for k in NAMES}
    xl = x.detach().double().clone().requires_grad_(True)
    sm = smoothing_ms.detach().float().double().reshape(-1).clone().requires_grad_(True)
    E = envelope(xl, sr, sm, hop, detector)
    gx, gsm = torch.autograd.grad((E * w.double()).sum(), [xl, sm])
    return dict(E=E.detach().numpy(), gx=gx.numpy(), gsm=gsm.numpy())
