"""The parity cases of limiter, shared by tests/test_limiter_cpu.py (which checks that they are well conditioned) and
tests/test_gpu_limiter.py (which runs the kernels on them): per configuration one batch whose items are the lengths of the case, every
item zero from its length on - which is the definition's own padding, so that item q over [0, n_q) is the op on the signal cut to n_q
samples - and the restatement's float64 and float32 results on it, computed once per process and never modified."""
import functools

import numpy as np
import torch

from tests import limiter_restated as R

TILE = 2048                  # dasp_limiter_tile(): asserted by the GPU tests
MAX_LOOKAHEAD = 1024         # dasp_limiter_max_lookahead(): the same
#          sample rate, L, channels, seed   (every L of {0, 1, 63, 64, 65, 220, max}, every channel count, every rate). The seeds are the first
# for which no decision of the float64 restatement is closer than 1e-4 (tests/test_limiter_cpu.py checks it): of some 20000 decisions per
# case a few are closer than that for most draws.
CONFIGS = [(8000, 0, 1, 2), (8000, 63, 2, 213), (44100, 1, 3, 158), (44100, 64, 1, 51), (44100, 220, 2, 18), (192000, 65, 2, 112), (192000, 1024, 3, 15)]


def lookahead_ms(sr, L):
    ms = L * 1000.0 / sr
    assert R.lookahead_samples(sr, ms) == L
    return ms


def lengths(L, T=TILE):
    out = []
    for n in (1, 2, L, L + 1, T - L - 1, T - L, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5):
        if n >= 1 and n not in out:
            out.append(n)
    return out


def inputs(sr, L, C, seed, Ls=None):
    """Noise under a log-normal envelope that changes every 48 samples; thresholds of -20 .. -8 dB, releases of 30 .. 4000 samples
    (1 - rho >= 5e-4: a held peak beats its own decay by more than the conditioning asks for)."""
    Ls = lengths(L) if Ls is None else Ls
    B, N = len(Ls), max(Ls)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + sr + C)
    env = torch.exp(0.8 * torch.randn(B, 1, (N + 47) // 48, generator=g)).repeat_interleave(48, -1)[..., :N]
    x = 0.35 * torch.randn(B, C, N, generator=g) * env
    w = torch.randn(B, C, N, generator=g)
    for q, n in enumerate(Ls):
        x[q, :, n:] = 0
        w[q, :, n:] = 0
    u = lambda lo, hi: torch.rand(B, generator=g) * (hi - lo) + lo
    thr = u(-20.0, -8.0)
    rel = torch.exp(u(np.log(30.0), np.log(4000.0))) / sr * 1000.0
    return dict(x=x, w=w, threshold_db=thr, release_ms=rel)


@functools.lru_cache(maxsize=None)
def reference(sr, L, C, seed):
    a = inputs(sr, L, C, seed)
    args = (a["x"], sr, a["threshold_db"], a["release_ms"], a["w"])
    want = R.forward_backward(*args, lookahead=L)
    f32 = R.forward_backward(*args, lookahead=L, arith=torch.float32)
    return a, want, f32
