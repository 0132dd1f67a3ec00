"""ITU-R BS.1770-4 integrated loudness and its fixed-gate gradient, restated in float64 numpy: the definition that
dasp_pytorch_amd.functional.loudness is tested against. Not a port of anything: the filter design is the closed form of the
recommendation's two biquads, re-derived per sample rate, and the block / gate arithmetic is written out from the text of the
recommendation. Also the peak-normalisation formula and its gradient."""
import numpy as np
import scipy.signal

CHANNEL_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)      # L, R, C, Ls, Rs

BS1770_48K = {                                       # the coefficient table of BS.1770-4 (48 kHz)
    "b1": (1.53512485958697, -2.69169618940638, 1.19839281085285),
    "a1": (1.0, -1.69065929318241, 0.73248077421585),
    "b2": (1.0, -2.0, 1.0),
    "a2": (1.0, -1.99004745483398, 0.99007225036621),
}


def k_weighting(fs):
    """-> (2, 6) float64, rows [b0 b1 b2 a0 a1 a2]: the high shelf, then the high-pass."""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
          1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]
    return np.array([s1, s2], dtype=np.float64)


def block_sizes(fs):
    H = int(round(0.1 * float(fs)))
    return H, 4 * H


def num_blocks(N, fs):
    H, T = block_sizes(fs)
    return (N - T) // H + 1 if N >= T else 0


def k_filter(x, fs, reverse=False):
    """x (..., N) float64 through both sections; reverse: backwards in time (the adjoint)."""
    y = np.asarray(x, np.float64)
    if reverse:
        y = y[..., ::-1]
    for row in k_weighting(fs):
        y = scipy.signal.lfilter(row[:3], row[3:], y, axis=-1)
    return y[..., ::-1] if reverse else y


def loudness(x, fs, gL=None):
    """x (bs, chs, N) -> dict: L (bs), grad (bs, chs, N) = dL/dx (times gL[item] if given), nb, nA, nJ (bs) and margin (bs): the distance
    of the closest block level from either gate threshold, in LU."""
    x = np.asarray(x, np.float64)
    bs, chs, N = x.shape
    H, T = block_sizes(fs)
    nb = num_blocks(N, fs)
    assert nb >= 1 and chs <= 5
    G = np.array(CHANNEL_WEIGHTS[:chs])
    y = k_filter(x, fs)
    L = np.full(bs, -np.inf)
    grad = np.zeros_like(x)
    nA, nJ, margin = np.zeros(bs, int), np.zeros(bs, int), np.full(bs, np.inf)
    for i in range(bs):
        z = np.stack([[np.mean(y[i, c, j * H:j * H + T] ** 2) for j in range(nb)] for c in range(chs)])     # (chs, nb)
        p = G @ z
        with np.errstate(divide="ignore"):
            l = -0.691 + 10.0 * np.log10(p)
        A = l > -70.0
        nA[i] = A.sum()
        margin[i] = np.min(np.abs(l + 70.0))
        if not A.any():
            continue
        gamma = -0.691 + 10.0 * np.log10(np.mean(p[A])) - 10.0
        margin[i] = min(margin[i], np.min(np.abs(l - gamma)))
        J = A & (l > gamma)
        nJ[i] = J.sum()
        if not J.any():
            continue
        P = np.mean(p[J])
        L[i] = -0.691 + 10.0 * np.log10(P)
        u = np.zeros((chs, N))
        for c in range(chs):
            dz = (10.0 / np.log(10.0)) * G[c] / (J.sum() * P)
            wsum = np.zeros(N)
            for j in np.nonzero(J)[0]:
                wsum[j * H:j * H + T] += dz / T
            u[c] = 2.0 * y[i, c] * wsum
        grad[i] = k_filter(u, fs, reverse=True) * (1.0 if gL is None else float(gL[i]))
    return {"L": L, "grad": grad, "nb": np.full(bs, nb), "nA": nA, "nJ": nJ, "margin": margin}


def gain_db_apply(x, g_db):
    return np.asarray(x, np.float64) * (10.0 ** (np.asarray(g_db, np.float64) / 20.0))[:, None, None]


def loudness_normalize(x, fs, target, gy=None):
    """y = x 10^((target - L(x)) / 20) and, for an upstream gradient gy, dloss/dx through both paths (the gates held fixed)."""
    x = np.asarray(x, np.float64)
    r = loudness(x, fs)
    ok = np.isfinite(r["L"])
    g_db = np.where(ok, target - np.where(ok, r["L"], 0.0), 0.0)
    lin = 10.0 ** (g_db / 20.0)
    y = x * lin[:, None, None]
    if gy is None:
        return y, None
    gy = np.asarray(gy, np.float64)
    # d y / d g_db = y ln10 / 20;  d g_db / d x = -dL/dx
    g_gdb = (gy * y).sum((1, 2)) * np.log(10.0) / 20.0
    gx = gy * lin[:, None, None] - np.where(ok, g_gdb, 0.0)[:, None, None] * r["grad"]
    return y, gx


def peak_normalize(x, peak_db=0.0, eps=1e-8, gy=None):
    """Per row: y = x s / max(max|x|, eps), s = 10^(peak_db / 20); gradient per the closed form, the maximum at its lowest index. A row
    that holds a NaN has a NaN peak: y and the gradient are NaN throughout."""
    x = np.asarray(x, np.float64)
    s = 10.0 ** (peak_db / 20.0)
    p = np.abs(x).max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = x * s / np.maximum(p, eps)
    if gy is None:
        return y, None
    gy = np.asarray(gy, np.float64)
    k = np.abs(x).argmax(-1)                          # the first index attaining the maximum
    gx = np.empty_like(x)
    for idx in np.ndindex(x.shape[:-1]):
        pp = p[idx][0]
        if pp != pp:                                  # a NaN in the row: the peak is NaN and so is every derivative through it (torch's
            g = np.full_like(gy[idx], np.nan)         # autograd of x * s / x.abs().amax(-1, keepdim=True).clamp(min=eps) says the same)
        elif pp > eps:
            g = s * gy[idx] / pp
            g[k[idx]] -= s * np.sign(x[idx][k[idx]]) * np.dot(gy[idx], x[idx]) / pp ** 2
        else:
            g = s * gy[idx] / eps
        gx[idx] = g
    return y, gx


def gated_draw():
    """(2, 2, 24123) at 8 kHz: 0.3 randn, 25 dB down in the second second, 1e-5 from the third second on; rounded to float32."""
    rng = np.random.default_rng(0)
    x = 0.3 * rng.standard_normal((2, 2, 24123))
    x[..., 8000:16000] *= 10.0 ** (-25.0 / 20.0)
    x[..., 16000:] *= 1e-5 / 0.3
    return x.astype(np.float32)


def sine_997(channels):
    """The 997 Hz, 0 dBFS sine at 48 kHz, 48000 samples, in the given channels of a stereo item."""
    t = np.arange(48000) / 48000.0
    x = np.zeros((1, 2, 48000))
    for c in channels:
        x[0, c] = np.sin(2.0 * np.pi * 997.0 * t)
    return x
