"""Restatement in torch of functional.gain_curve, differentiable by autograd, on the CPU. The op has no recurrence, so the loop over
the samples is written as one vector expression per sample index:

    j = n // hop;   t = (n mod hop) / hop;   g[n] = P_j (t = 0) | P_j + t (P_{j+1} - P_j),  P = gain_db[b]
    y[b,c,n] = x[b,c,n] 10^(g[n] / 20)

arith=torch.float64 (the default): float64 throughout - the oracle. arith=torch.float32: the curve, the interpolation, the exponential
and the product in float32, which is what the kernel does; its error against the float64 variant is the yardstick e32 of the GPU tests.
"""
import math

import numpy as np
import torch

CTL = ("gain_db",)
GRADS = ("ggain",)
NAMES = ("y", "gx") + GRADS
# the least the kernel's parity bound is, whatever the float32 restatement's own error: the floors of the other fused effects
FLOOR = dict(y=2e-6, gx=2e-6, ggain=1e-5)
LN10_20 = math.log(10.0) / 20.0


def control_frames(seq_len, hop):
    return -(-seq_len // hop) + 1


def interpolate(P, N, hop):
    """A curve's frame points (..., F) at the N samples, in P's dtype; t = (n mod hop) / hop is exact in float32. At t = 0 the value is
    the frame point itself: the next one is not touched."""
    assert P.shape[-1] == control_frames(N, hop)
    n = torch.arange(N)
    j = n // hop
    t = ((n % hop).double() / hop).to(P.dtype)
    return torch.where(t == 0, P[..., j], P[..., j] + t * (P[..., j + 1] - P[..., j]))


def gain_curve(x, gain_db, hop=64, arith=torch.float64):
    """y in `arith`; x (bs, chs, N), gain_db (bs, F)."""
    g = interpolate(gain_db.to(arith), x.shape[-1], hop)
    return x.to(arith) * torch.exp(g * torch.tensor(LN10_20, dtype=arith))[:, None, :]


def forward_backward(x, sr, gain_db, w, hop=64, arith=torch.float64):
    """y, gx and ggain for the upstream gradient w, as float64 numpy arrays (sr is not used: the op's signature)."""
    xl = x.detach().double().clone().requires_grad_(True)
    P = gain_db.detach().double().clone().requires_grad_(True)
    y = gain_curve(xl, P, hop, arith)
    gx, gP = torch.autograd.grad((y * w.to(arith)).sum(), [xl, P])
    return dict(y=y.detach().double().numpy(), gx=gx.numpy(), ggain=gP.numpy())


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


def adjoint_by_hand(x, gain_db, w, hop):
    """gx and ggain written out, numpy float64: gx = w G; q = (ln 10 / 20) sum_c w x G; ggain = frame_gradients(q)."""
    x, P, w = (np.asarray(v, np.float64) for v in (x, gain_db, w))
    G = np.exp(LN10_20 * interpolate(torch.from_numpy(P), x.shape[-1], hop).numpy())[:, None, :]
    return w * G, frame_gradients(LN10_20 * (w * x * G).sum(1), hop, P.shape[-1])
