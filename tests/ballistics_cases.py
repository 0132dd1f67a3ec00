"""The parity cases of block_level and ballistics, shared by the CPU tests (which hold the restatements alone to the conditions below)
and the GPU tests (which hold the kernels to the restatements).

ballistics: the nine rate x hop pairs of control_rate_cases.ENVELOPE_CONFIGS, each on a batch of three items with times drawn from
0.1, 1, 5, 50 and 2000 ms (attack > release, attack == release and attack < release all occur), at every length of `frame_counts()`.
The float64 restatement is a Python loop over frames, so it runs once per configuration on one batch that holds every length as three
items with the upstream gradient zero from the length on: the smoother is causal, and with no upstream gradient past F the adjoint of
the longer curve is that of the first F frames. The curves are a non-negative "gain reduction" shape with per-frame noise (`curve`),
busy enough that both branches are taken whatever the two times are.

Conditions, held by tests/test_ballistics_cpu.py: in every item with F >= 64 each branch takes at least 5 % of the frames (otherwise
one branch's coefficient and gradient would go untested); no bound max(4 e32, floor) exceeds ten floors; and no branch decision is a
near-tie: the masks stay what they are when both coefficients move by an ulp either way, so that an exp of another library cannot flip
one.

block_level: both detectors, 1 - 3 channels, hop 8 / 64 / 2048 at the lengths of control_rate_cases.lengths(hop) (tile 4096); the
configurations marked `ties` quantise the signal to steps of 1/4, so that maxima repeat inside a block and across channels.
"""
import functools

import numpy as np
import torch

from tests import ballistics_restated as BR
from tests import block_level_restated as LR
from tests.control_rate_cases import BS, ENVELOPE_CONFIGS, TILE, bounds, lengths, per_item_err  # noqa: F401

CHUNK = 1024                 # dasp_ballistics_chunk()
TIMES = (0.1, 1.0, 5.0, 50.0, 2000.0)
# (sample rate, hop, attack_ms of the three items, release_ms of the three items, seed)
BALLISTICS_CONFIGS = [
    (8000, 8, (0.1, 50.0, 5.0), (2000.0, 1.0, 5.0), 0),
    (8000, 64, (1.0, 2000.0, 50.0), (50.0, 0.1, 50.0), 1),
    (8000, 2048, (5.0, 0.1, 2000.0), (1.0, 2000.0, 5.0), 2),
    (44100, 8, (0.1, 5.0, 2000.0), (2000.0, 50.0, 0.1), 3),
    (44100, 64, (5.0, 50.0, 1.0), (50.0, 5.0, 1.0), 4),
    (44100, 2048, (50.0, 2000.0, 0.1), (2000.0, 50.0, 5.0), 5),
    (192000, 8, (0.1, 1.0, 50.0), (2000.0, 0.1, 50.0), 6),
    (192000, 64, (2000.0, 0.1, 5.0), (0.1, 2000.0, 50.0), 7),
    (192000, 2048, (1.0, 5.0, 2000.0), (5.0, 1.0, 0.1), 8),
]
assert [c[:2] for c in BALLISTICS_CONFIGS] == [c[:2] for c in ENVELOPE_CONFIGS[:9]]
# (hop, channels, detector, ties, seed)
BLOCK_LEVEL_CONFIGS = [(8, 1, "peak", False, 0), (64, 2, "power", False, 1), (2048, 3, "peak", False, 2), (8, 3, "power", False, 3),
                       (64, 1, "peak", True, 4), (2048, 2, "power", False, 5), (64, 3, "peak", True, 6), (8, 2, "peak", True, 7),
                       (2048, 2, "peak", True, 8), (64, 1, "power", False, 9)]


def frame_counts():
    return [1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 16385]


def curve(B, F, g):
    """A gain-reduction curve in dB, non-negative: per item a ceiling A, log-normal about 6 dB, and per frame one of three states - no
    reduction (exactly 0, 30 % of the frames), at the ceiling (A (1 - u / 1000), 30 %) or anywhere between (40 %). A slow shape alone
    will not do: with a fast attack and a slow release the smoother is a peak hold, whose attack share on any curve that does not
    come back to its top again and again is about c_r / c_a (the issue found 1 %); the mirrored case rests on the floor."""
    A = 6.0 * torch.exp(0.5 * torch.randn(B, 1, generator=g))
    state, u = torch.rand(B, F, generator=g), torch.rand(B, F, generator=g)
    return A * torch.where(state < 0.3, torch.zeros(B, F), torch.where(state < 0.6, 1.0 - 1e-3 * u, u))


def ballistics_inputs(cfg):
    sr, hop, att, rel, seed = cfg
    fs = frame_counts()
    g = torch.Generator().manual_seed(3000 + seed)
    B, F = BS * len(fs), fs[-1]
    P = curve(B, F, g)
    w = 0.5 + 0.5 * torch.randn(B, F, generator=g)
    for q, f in enumerate(fs):
        w[BS * q:BS * (q + 1), f:] = 0.0
    return dict(P=P, w=w, attack_ms=torch.tensor(att * len(fs), dtype=torch.float32), release_ms=torch.tensor(rel * len(fs), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def ballistics_reference(cfg):
    """(inputs, float64 results) on the batch of all lengths; unchanged by the tests that share it."""
    sr, hop, att, rel, seed = cfg
    a = ballistics_inputs(cfg)
    return a, BR.forward_backward(a["P"], sr, a["attack_ms"], a["release_ms"], a["w"], hop)


def ballistics_calls(cfg):
    """Per length: the inputs of the call of three items, its float64 results and those of the kernel's arithmetic."""
    sr, hop, att, rel, seed = cfg
    a, r64 = ballistics_reference(cfg)
    for q, f in enumerate(frame_counts()):
        s = slice(BS * q, BS * (q + 1))
        b = dict(P=a["P"][s, :f].contiguous(), w=a["w"][s, :f].contiguous(), attack_ms=a["attack_ms"][s], release_ms=a["release_ms"][s])
        want = dict(E=r64["E"][s, :f], up=r64["up"][s, :f], gP=r64["gP"][s, :f], gatt=r64["gatt"][s], grel=r64["grel"][s])
        f32 = BR.forward_backward(b["P"], sr, b["attack_ms"], b["release_ms"], b["w"], hop, arith=torch.float32)
        yield f, b, want, f32


def block_level_inputs(cfg, n):
    hop, chs, det, ties, seed = cfg
    g = torch.Generator().manual_seed(4000 + 31 * seed + n)
    env = torch.exp(0.8 * torch.randn(BS, 1, (n + 255) // 256, generator=g)).repeat_interleave(256, -1)[..., :n]
    x = 0.3 * torch.randn(BS, chs, n, generator=g) * env
    if ties:
        x = torch.round(4.0 * x) / 4.0
    return dict(x=x, w=0.5 + 0.5 * torch.randn(BS, LR.control_frames(n, hop), generator=g))


def block_level_calls(cfg):
    hop, chs, det, ties, seed = cfg
    for n in lengths(hop):
        b = block_level_inputs(cfg, n)
        want = LR.forward_backward(b["x"], b["w"], hop, det)
        hand = LR.by_hand(b["x"].numpy(), b["w"].numpy(), hop, det, np.float32)
        yield n, b, want, hand


def branch_shares(up):
    """Per item: the share of attack frames and of release frames."""
    u = np.asarray(up, bool)
    return u.mean(1), (~u).mean(1)
