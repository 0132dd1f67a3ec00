"""The parity cases of envelope_follower and gain_curve, shared by the CPU tests (which hold the restatements alone to the condition
below) and the GPU tests (which hold the kernels to the restatements).

A case is one configuration on a batch of bs = 3 items at every length of `lengths(hop)`. The float64 restatement of the envelope is
a Python loop over samples, so it runs once per configuration on one batch that holds every length as three items, zero from the
length on - the definition's own padding (the level is zero from sample N on, so the frame points of a shorter signal are the first
frame points of the padded one). Errors are per item, relative to the peak of the item's float64 result; the kernel's bound is
max(4 e32, FLOOR) with e32 the error of the restatement in the kernel's arithmetic on the same item.

Condition on the cases: no bound may exceed ten times its floor, so that a loose e32 cannot hide a wrong kernel. The upstream
gradients are drawn with a mean (0.5 + 0.5 randn for the envelope) so that the control gradient, one sum per item, is not a
cancellation to nothing, which would make its relative error a property of the draw.
"""
import functools

import numpy as np
import torch

from tests import envelope_restated as ER
from tests import gain_curve_restated as GR

TILE = 4096                  # dasp_envelope_tile(): the tile of both ops
BS = 3

# (sample rate, hop, channels, detector, smoothing_ms of the three items, seed): every rate with every hop, and every smoothing time,
# channel count and detector with each of them at least once
ENVELOPE_CONFIGS = [
    (8000, 8, 1, "peak", (0.1, 1.0, 50.0), 0),
    (8000, 64, 2, "power", (1.0, 50.0, 2000.0), 1),
    (8000, 2048, 3, "peak", (50.0, 2000.0, 0.1), 2),
    (44100, 8, 2, "peak", (2000.0, 0.1, 1.0), 3),
    (44100, 64, 3, "power", (0.1, 1.0, 50.0), 4),
    (44100, 2048, 1, "power", (1.0, 50.0, 2000.0), 5),
    (192000, 8, 3, "power", (50.0, 2000.0, 0.1), 6),
    (192000, 64, 1, "peak", (2000.0, 0.1, 1.0), 7),
    (192000, 2048, 2, "peak", (0.1, 1.0, 50.0), 8),
    (44100, 64, 2, "peak", (50.0, 2000.0, 1.0), 9),
]
# (hop, channels, seed): the op does not read the sample rate
GAIN_CURVE_CONFIGS = [(8, 1, 0), (64, 2, 1), (2048, 3, 2), (8, 3, 3), (64, 1, 4), (2048, 2, 5)]


def lengths(hop):
    return sorted({1, 7, 8, 9, hop - 1, hop, hop + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3})


def per_item_err(got, want):
    """max |got - want| / max |want| per item, the largest over the items (an item whose reference is all zero must be matched exactly)."""
    g, w = (np.asarray(v, np.float64).reshape(len(want), -1) for v in (got, want))
    d, pk = np.abs(g - w).max(1), np.abs(w).max(1)
    return float(np.where(pk > 0, d / np.where(pk > 0, pk, 1.0), np.where(d > 0, np.inf, 0.0)).max())


def bounds(want, f32, floor):
    """{name: (e32, bound)} of one call's references."""
    out = {}
    for k in floor:
        e32 = per_item_err(f32[k], want[k])
        out[k] = (e32, max(4.0 * e32, floor[k]))
    return out


def envelope_inputs(cfg):
    sr, hop, chs, det, sm, seed = cfg
    ns = lengths(hop)
    g = torch.Generator().manual_seed(1000 + seed)
    N = ns[-1]
    B = BS * len(ns)
    # noise under a slow log-normal envelope: levels that move over a few hundred samples
    env = torch.exp(0.8 * torch.randn(B, 1, (N + 255) // 256, generator=g)).repeat_interleave(256, -1)[..., :N]
    x = 0.3 * torch.randn(B, chs, N, generator=g) * env
    w = 0.5 + 0.5 * torch.randn(B, ER.control_frames(N, hop), generator=g)
    for q, n in enumerate(ns):
        x[BS * q:BS * (q + 1), :, n:] = 0.0
        w[BS * q:BS * (q + 1), ER.control_frames(n, hop):] = 0.0
    return dict(x=x, w=w, smoothing_ms=torch.tensor(sm * len(ns), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def envelope_reference(cfg):
    """(inputs, float64 results) on the batch of all lengths; unchanged by the tests that share it."""
    sr, hop, chs, det, sm, seed = cfg
    a = envelope_inputs(cfg)
    return a, ER.forward_backward(a["x"], sr, a["smoothing_ms"], a["w"], hop, det)


def envelope_calls(cfg):
    """Per length: the inputs of the call of three items, its float64 results and those of the kernel's arithmetic in float32."""
    sr, hop, chs, det, sm, seed = cfg
    a, r64 = envelope_reference(cfg)
    for q, n in enumerate(lengths(hop)):
        s, F = slice(BS * q, BS * (q + 1)), ER.control_frames(n, hop)
        b = dict(x=a["x"][s, :, :n].contiguous(), w=a["w"][s, :F].contiguous(), smoothing_ms=a["smoothing_ms"][s])
        want = dict(E=r64["E"][s, :F], gx=r64["gx"][s, :, :n], gsm=r64["gsm"][s])
        f32 = ER.forward_backward(b["x"], sr, b["smoothing_ms"], b["w"], hop, det, arith=torch.float32)
        yield n, b, want, f32


def gain_curve_inputs(hop, chs, n, seed):
    g = torch.Generator().manual_seed(2000 + 31 * seed + n)
    F = GR.control_frames(n, hop)
    return dict(x=0.5 * torch.randn(BS, chs, n, generator=g), w=torch.randn(BS, chs, n, generator=g),
                gain_db=torch.rand(BS, F, generator=g) * 72.0 - 60.0)          # the module's default range, -60 .. 12 dB


def gain_curve_calls(cfg):
    hop, chs, seed = cfg
    for n in lengths(hop):
        b = gain_curve_inputs(hop, chs, n, seed)
        want = GR.forward_backward(b["x"], 44100, b["gain_db"], b["w"], hop)
        f32 = GR.forward_backward(b["x"], 44100, b["gain_db"], b["w"], hop, arith=torch.float32)
        yield n, b, want, f32
