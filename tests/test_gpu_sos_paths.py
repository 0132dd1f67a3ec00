"""The code paths of the Gram-matrix backward kernel (csrc/sosfilt.hip sos_bwd_gram_kernel) at the smallest shapes that take them:
parametric_eq forward + backward with gradients for x and the 18 controls against the fp64 oracle. Up to 256 rows the launcher gives a
row 8 waves, above that 4; rows of fewer than 16 tiles are never cut into segments, and neither are more than 128 rows.

    (2,2,4096)     8 waves, every tile full: the all-full variant, 4 tiles - one per wave, four waves idle
    (2,2,8192)     8 waves, all-full, 8 tiles: every wave exactly one
    (2,2,12288)    8 waves, all-full, 12 tiles: waves 0 - 3 run two - the second meets the constant vmcnt wait at the top of the tile
                   loop with the first tile's output stores and the LDS-DMA of its own images really in flight (without gx: the same
                   loop with the full wait)
    (2,2,5000)     last tile ragged: the general variant with its guarded loads and stores
    (1,1,1024)     a single tile, the other waves idle
    (2,2,4096)     without a gradient for x: the all-full variant without the output map
    (129,2,8192)   258 rows: the 4-wave all-full variants (the headline's instantiations), two tiles per wave, with and without gx; four
                   of the items against the oracle (rows are independent: a sample of the launch is a test of the launch)

The oracle is the reference's frequency-sampling algorithm in fp64 (oracle/dasp_oracle.py). It is a circular convolution over
2^ceil(log2(2T - 1)) points, which at these lengths would alias the undecayed tail of the low-frequency sections (test_gpu_sosfilt.py
test_ragged_shapes), so x and the output weights are zero-padded to PAD samples first: the tail has decayed by exp(-28) at worst
(20 Hz, Q = 6: pole radius 1 - 2.4e-4, 2 PAD - 12288 samples) and the first N samples / the gradients are those of the exact LTI
system. The backward pass is anticausal, so nothing here compares one shape's results with a prefix of another's.
Tolerances: TOL_SIG / TOL_PAR of test_gpu_sosfilt.py for the same quantities."""
import functools

import numpy as np
import pytest
import torch

from oracle import dasp_oracle as orc
from tests.util import linf_peak, record

pytestmark = pytest.mark.gpu
SR = 44100
TOL_SIG, TOL_PAR = 1e-5, 1e-4
PAD = 65536

PEQ_RANGES = [(-20, 20), (20, 2000), (0.1, 6), (-20, 20), (80, 2000), (0.1, 6), (-20, 20), (2000, 8000), (0.1, 6),
              (-20, 20), (8000, 12000), (0.1, 6), (-20, 20), (12000, 21050), (0.1, 6), (-20, 20), (4000, 21050), (0.1, 6)]


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared case arrays are read-only)


@functools.lru_cache(maxsize=None)
def case(B, C, N, pick=None):
    """inputs of one shape and the oracle's (y, gx, gp) for the items `pick` (None = all), computed once and shared (read-only)"""
    g = np.random.default_rng(1000 + N + B)
    x = (g.random((B, C, N)) * 2 - 1).astype(np.float32)
    w = g.standard_normal((B, C, N)).astype(np.float32)
    u = g.random((B, 18))
    lo = np.array([r[0] for r in PEQ_RANGES]); hi = np.array([r[1] for r in PEQ_RANGES])
    p = (u * (hi - lo) + lo).astype(np.float32)
    idx = np.arange(B) if pick is None else np.array(pick)
    xp = np.zeros((len(idx), C, PAD)); xp[..., :N] = x[idx]
    wp = np.zeros((len(idx), C, PAD)); wp[..., :N] = w[idx]
    yo = orc.parametric_eq(xp, SR, p[idx])[..., :N]
    gxo, gpo = orc.parametric_eq_vjp(xp, SR, p[idx], wp)
    out = (x, w, p, idx, yo, gxo[..., :N], gpo)
    for a in out:
        a.setflags(write=False)
    return out


def run_eq(D, x, p, w, want_gx):
    xt = dev(x).requires_grad_(want_gx)
    cols = [dev(p[:, i]).requires_grad_(True) for i in range(18)]
    y = D.parametric_eq(xt, SR, *cols)
    (y * dev(w)).sum().backward()
    torch.cuda.synchronize()
    return (y.detach().cpu().numpy(), xt.grad.cpu().numpy() if want_gx else None,
            torch.stack([c.grad for c in cols], 1).cpu().numpy())


MANY = (129, 2, 8192, (0, 57, 127, 128))      # more than 256 rows: four waves per row


@pytest.mark.parametrize("B,C,N,pick,want_gx", [(2, 2, 4096, None, True), (2, 2, 8192, None, True), (2, 2, 12288, None, True),
                                                (2, 2, 5000, None, True), (1, 1, 1024, None, True), (2, 2, 4096, None, False),
                                                (2, 2, 12288, None, False), MANY + (True,), MANY + (False,)])
def test_gram_backward_paths_vs_oracle(D, B, C, N, pick, want_gx):
    x, w, p, idx, yo, gxo, gpo = case(B, C, N, pick)
    y, gx, gp = run_eq(D, x, p, w, want_gx)
    ey, egp = linf_peak(y[idx], yo).max(), linf_peak(gp[idx], gpo).max()
    egx = linf_peak(gx[idx], gxo).max() if want_gx else 0.0
    record(f"gram_paths[{B},{C},{N},gx={int(want_gx)}]", y=ey, gx=egx, gp=egp)
    assert np.isfinite(y).all() and np.isfinite(gp).all() and (not want_gx or np.isfinite(gx).all())
    assert ey < TOL_SIG
    assert egx < TOL_SIG
    assert egp < TOL_PAR
