"""Restatement of functional.block_level on the CPU, in two forms.

`block_level` is the definition in torch float64, differentiable by autograd - the oracle. With the level p of
tests/envelope_restated.level (p = 0 from sample N on), h = hop and F = ceil(N / h) + 1:

    L[b,0] = p[0];   L[b,j] = max_{i=1..h} p[(j-1) h + i]  (peak)  |  (1 / h) sum_{i=1..h} p[(j-1) h + i]  (power),   j = 1 .. F-1

The peak of a block is met in time order, a candidate replacing the current one when (a > cur) | (isnan(a) & !isnan(cur)), as
torch.where branches: the earliest sample that holds the maximum takes the gradient.

`by_hand` is the forward pass and the adjoint without autograd, in numpy at the kernel's arithmetic. Peak is exact - L, the saved
winners and gx are what the kernel gives bit for bit: per sample the signed value of the winning channel (the same rule over the
channels, so the first NaN channel wins), per block the winner in time order, saved as (i - 1) | sign << 11 | channel << 13 for the
sample (j-1) h + i with sign 0 zero, 1 positive, 2 negative, 3 NaN; gx = sign(x_winner) gL_j at the winner and a written zero
everywhere else. Power in `dt`: the channel mean, runs of 8 samples added in time order, the runs of a block as a balanced tree, then
times 1 / h; gx = (2 / (chs h) gL_j) x, and (2 / chs gL_0) x for sample 0. Its error against the float64 form is the yardstick e32.
"""
import numpy as np
import torch

from tests import envelope_restated as ER

DETECTORS = ER.DETECTORS
NAMES = ("L", "gx")
FLOOR = dict(L=ER.FLOOR["E"], gx=ER.FLOOR["gx"])
RUN = 8
control_frames = ER.control_frames


def block_level(x, hop=64, detector="peak"):
    """L (bs, F), float64, differentiable."""
    bs, chs, N = x.shape
    F = control_frames(N, hop)
    p = ER.level(x.double(), detector)
    p = torch.cat([p, torch.zeros(bs, (F - 1) * hop + 1 - N, dtype=torch.float64)], 1)
    blocks = p[:, 1:].reshape(bs, F - 1, hop)
    if detector == "power":
        body = blocks.sum(-1) / hop
    else:
        body = blocks[..., 0]
        for i in range(1, hop):
            a = blocks[..., i]
            body = torch.where((a > body) | (torch.isnan(a) & ~torch.isnan(body)), a, body)
    return torch.cat([p[:, :1], body], 1)


def _replaces(a, cur):
    with np.errstate(invalid="ignore"):
        return (a > cur) | (np.isnan(a) & ~np.isnan(cur))


def winners(x, hop):
    """The signed winner (bs, F) float32, its position in the block and its channel, met in the kernel's order."""
    x = np.asarray(x, np.float32)
    bs, chs, N = x.shape
    F = control_frames(N, hop)
    v, ch = x[:, 0].copy(), np.zeros((bs, N), np.int64)
    for c in range(1, chs):
        take = _replaces(np.abs(x[:, c]), np.abs(v))
        v, ch = np.where(take, x[:, c], v), np.where(take, c, ch)
    pad = (F - 1) * hop + 1 - N
    v, ch = np.concatenate([v, np.zeros((bs, pad), np.float32)], 1), np.concatenate([ch, np.zeros((bs, pad), np.int64)], 1)
    bv, bc = v[:, 1:].reshape(bs, F - 1, hop), ch[:, 1:].reshape(bs, F - 1, hop)
    wv, wc, wp = bv[..., 0].copy(), bc[..., 0].copy(), np.zeros((bs, F - 1), np.int64)
    for i in range(1, hop):
        take = _replaces(np.abs(bv[..., i]), np.abs(wv))
        wv, wc, wp = np.where(take, bv[..., i], wv), np.where(take, bc[..., i], wc), np.where(take, i, wp)
    cat = lambda first, rest: np.concatenate([first[:, None], rest], 1)
    return cat(v[:, 0], wv), cat(np.zeros(bs, np.int64), wp), cat(ch[:, 0], wc)


def winner_words(wv, wp, wc):
    """The int32 words the forward pass saves."""
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(wv), 3, np.where(wv > 0, 1, np.where(wv < 0, 2, 0)))
    return (wp | s << 11 | wc << 13).astype(np.int32)


def _tree(v):
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def by_hand(x, w, hop=64, detector="peak", dt=np.float32):
    """L, gx (float64 arrays of values held in dt) and, for peak, `win` (int32) for the upstream gradient w (bs, F)."""
    x = np.asarray(x, dt)
    bs, chs, N = x.shape
    F = control_frames(N, hop)
    g = np.asarray(w, dt)
    m = np.arange(N)
    j = -(-m // hop)
    if detector == "peak":
        wv, wp, wc = winners(x, hop)
        L = np.abs(wv).astype(dt)
        gx = np.zeros_like(x)
        at = np.where(np.arange(F)[None] > 0, (np.arange(F)[None] - 1) * hop + 1 + wp, 0)          # the winner's sample
        with np.errstate(invalid="ignore"):
            val = np.sign(wv).astype(dt) * g
        bb, jj = np.nonzero(at < N)                                          # a block of padding alone has its winner past the end
        gx[bb, wc[bb, jj], at[bb, jj]] = val[bb, jj]
        return dict(L=L.astype(np.float64), gx=gx.astype(np.float64), win=winner_words(wv, wp, wc))
    invc = dt(1.0) / dt(chs)
    p = x[:, 0] * x[:, 0]
    for c in range(1, chs):
        p = (x[:, c].astype(np.float64) * x[:, c].astype(np.float64) + p.astype(np.float64)).astype(dt) if dt is np.float32 else p + x[:, c] * x[:, c]
    p = p * invc
    p = np.concatenate([p, np.zeros((bs, (F - 1) * hop + 1 - N), dt)], 1)
    runs = p[:, 1:].reshape(bs, F - 1, hop // RUN, RUN)
    s = runs[..., 0]
    for i in range(1, RUN):
        s = s + runs[..., i]
    invh = dt(1.0) / dt(hop)
    L = np.concatenate([p[:, :1], (_tree(s) * invh)[:, :]], 1).astype(dt)
    scale = (dt(2.0) * invc) * np.where(m > 0, invh, dt(1.0)).astype(dt)[None] * g[:, j]
    gx = scale[:, None, :] * x
    return dict(L=L.astype(np.float64), gx=gx.astype(np.float64))


def forward_backward(x, w, hop=64, detector="peak", arith=torch.float64):
    """L and gx for the upstream gradient w (bs, F), as float64 numpy arrays. arith=torch.float64: the definition and autograd;
    arith=torch.float32: `by_hand` at the kernel's arithmetic."""
    if arith is torch.float32:
        r = by_hand(x.detach().numpy(), w.detach().numpy(), hop, detector, np.float32)
        return {k: r[k] for k in NAMES}
    xl = x.detach().double().clone().requires_grad_(True)
    L = block_level(xl, hop, detector)
    (gx,) = torch.autograd.grad((L * w.double()).sum(), [xl])
    return dict(L=L.detach().numpy(), gx=gx.numpy())
