"""Shared helper of tests/test_dynamics_exact_cpu.py and tests/test_gpu_dynamics_exact.py (not collected): inputs on which the
hand-written derivatives of the static gain computer (csrc/dyn_common.hpp gain_computer, csrc/ref64.hip gain_computer64) are compared
sharply with the analytic float64 adjoint tests/input_domain_cases.py::dynamics_exact.

Why not the inputs of the other dynamics tests: a speech-like signal wanders through all three branches of the curve (below the knee,
inside it, above it) and a Gaussian upstream gradient makes the per-sample terms of every control-gradient sum cancel - the cancellation
(sum of |terms|) / |sum of terms| reaches 1e4 for the expander's knee column and is routinely 50 .. 1100 for the attack and make-up
columns, so a bound "relative to the column maximum" says little about the formula behind the column, and the knee branch holds a small
share of the samples. Here

  region_signal   the side chain of every item stays wholly inside ONE branch: s[n] = +-10^(level_dB[n] / 20) with level_dB uniform in
                  below [lo - 25, lo - 0.5] / knee [lo + 0.05, hi - 0.05] / above [hi + 0.5, hi + 15], lo, hi = thr -+ knee / 2, split
                  over the channels by fixed shares that sum to 1 (the three-channel shares hold a negative one: channels cancel inside
                  the side-chain sum);
  matched_gy      gy = sign(x_d) (0.2 + U[0, 1)), x_d the delayed x: every gy x_d term is positive, so the threshold, ratio, knee and
                  make-up columns are sums of same-sign terms inside a region (cancellation 1.0; the attack column, whose terms carry
                  the sign of g[n-1] - g_c[n], 11.3 at the most). test_dynamics_exact_cpu.py asserts cancellation <= 32 for every case,
                  and the GPU test asserts it again before it compares: a condition of the comparison, not a tolerance.

Bounds. y and grad x: the project's (COMP_TOL / EXP_TOL of input_domain_cases: 2e-5 of the item's peak, 5e-5 for the expander's grad
x). Compressor control columns: 1e-4 of the column maximum (CTL_TOL of tests/test_gpu_dynamics.py). Expander control columns and the
float64 bounds: measured on an MI355X against dynamics_exact, profiles/r23/dynamics_exact/parity.jsonl; the values stand beside the
constants below."""
import functools

import numpy as np

from tests import input_domain_cases as idc

SR = 44100
KEYS = idc.DYN_KEYS
REGIONS = ("below", "knee", "above")
SHARES = {1: (1.0,), 2: (0.7, 0.3), 3: (1.5, -0.9, 0.4)}
# threshold_db, ratio, attack_ms, release_ms (no path to the output), knee_db, makeup_gain_db
CONTROLS = np.array([[-30.0, 4.0, 5.0, 50.0, 6.0, 2.0],
                     [-18.0, 2.5, 12.0, 50.0, 3.0, 0.5],
                     [-42.0, 12.0, 1.0, 50.0, 12.0, 0.0]], np.float32)
MAX_CANCELLATION = 32.0

# (B, C, N, look): DMA backward with one full 512-sample tile and a 4-sample ragged one; the non-DMA backward (C > 2, look > 0); 10 tiles
# for the 8 backward waves (a wave's second tile, the swap of its two LDS ring slots, a ragged last tile)
REGION_SHAPES = ((3, 2, 516, 0), (3, 3, 1028, 5), (3, 2, 4612, 0))
# speech-like signal, random controls, gy = randn; look >= N: everything is exactly zero
EDGE_SHAPES = ((1, 1, 1, 0), (2, 1, 7, 0), (1, 2, 255, 0), (2, 2, 512, 0), (2, 1, 513, 0), (1, 2, 516, 0), (1, 3, 1028, 0),
               (2, 2, 4608, 0),       # 9 full tiles, DMA
               (1, 2, 8708, 0),       # 18 tiles for the 16 forward waves, still one workgroup per item (fewer than 32 tiles)
               (2, 2, 1028, 3), (1, 2, 1500, 512), (1, 2, 1500, 700), (2, 1, 300, 300), (2, 1, 300, 1000))
HARD_SHAPE = (3, 2, 1028, 0)
F64_SHAPES = ((2, 2, 516, 0), (1, 3, 1028, 5), (2, 1, 300, 300))

# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
Y_TOL = 2e-5                               # L-inf / peak per item (idc.COMP_TOL, idc.EXP_TOL)
GX_TOL = {0: 2e-5, 1: 5e-5}
COMP_CTL_TOL = 1e-4                        # of the column maximum (tests/test_gpu_dynamics.py CTL_TOL)
# Expander control columns against the exact adjoint (not finite differences). Rule: the compressor's 1e-4 if the worst column error
# of every float32 expander case of tests/test_gpu_dynamics_exact.py is <= 2.5e-5 (the 4x margin the project's bounds keep over their
# measurements), else 4x the measured value. Measured on an MI355X: 4.69e-5 (attack_ms, knee region, (3,2,4612); why: beside
# idc.EXP_CTL_TOL, which the input-domain and autograd-contract suites share), so 1.9e-4.
EXP_CTL_MEASURED = 4.688e-5
EXP_CTL_TOL = idc.EXP_CTL_TOL
assert 4 * EXP_CTL_MEASURED <= EXP_CTL_TOL <= 4.1 * EXP_CTL_MEASURED
# float64 (ref64.hip dyn64_*): both sides are plain double recursions that differ by log / exp rounding and summation order; bound =
# 8x the measured worst of the 26 float64 cases, far under the ceilings of tests/test_gpu_fp64.py (5e-7 of the peak for y and grad x, 2e-6
# for the columns)
F64_MEASURED = dict(y=2.51e-15, g_x=2.317e-14, g_params=1.28e-13)
F64_TOL = {k: 8 * v for k, v in F64_MEASURED.items()}
assert F64_TOL["y"] < 5e-7 and F64_TOL["g_x"] < 5e-7 and F64_TOL["g_params"] < 2e-6


def ctl_tol(mode):
    return COMP_CTL_TOL if mode == 0 else EXP_CTL_TOL


def controls(B, hard=False):
    """(B, 6) float32: the rows of CONTROLS in turn; hard: knee_db = 0."""
    p = CONTROLS[np.arange(B) % len(CONTROLS)].copy()
    if hard:
        p[:, 4] = 0.0
    return p


def band(region, thr, knee):
    lo, hi = thr - knee / 2, thr + knee / 2
    return {"below": (lo - 25.0, lo - 0.5), "knee": (lo + 0.05, hi - 0.05), "above": (hi + 0.5, hi + 15.0)}[region]


def side_db(x):
    """Level of the side chain in dB as the reference sees the float32 x: (B, N)."""
    with np.errstate(divide="ignore"):
        return 20 * np.log10(np.abs(np.asarray(x, np.float64).sum(1)))


def region_of(x, p):
    """-> (B, N) of 0 / 1 / 2 (below / knee / above) for the side chain of x under the controls p."""
    p = np.asarray(p, np.float64)
    d = side_db(x)
    lo, hi = (p[:, 0] - p[:, 4] / 2)[:, None], (p[:, 0] + p[:, 4] / 2)[:, None]
    return np.where(d < lo, 0, np.where(d > hi, 2, 1))


def _spread(s, C):
    return (s[:, None, :] * np.array(SHARES[C], np.float64)[None, :, None]).astype(np.float32)


def region_signal(rng, region, p, C, N):
    """x (B, C, N) float32 whose side chain lies wholly in `region` of the static curve of each item's controls p (B, 6)."""
    p = np.asarray(p, np.float64)
    B = p.shape[0]
    level = np.empty((B, N))
    for b in range(B):
        lo, hi = band(region, p[b, 0], p[b, 4])
        assert hi > lo
        level[b] = lo + (hi - lo) * rng.random(N)
    x = _spread(rng.choice([-1.0, 1.0], size=(B, N)) * 10 ** (level / 20), C)
    assert np.all(region_of(x, p) == REGIONS.index(region))     # float32 rounding of the channels moved no sample out of its band
    return x


def hard_knee_signal(rng, p, C, N):
    """knee_db = 0: every sample drawn from the 'below' or the 'above' band (a coin per sample); none within 1e-3 dB of the threshold,
    where the reference's knee branch is 0 / 0."""
    p = np.asarray(p, np.float64)
    assert np.all(p[:, 4] == 0)
    B = p.shape[0]
    level = np.empty((B, N))
    for b in range(B):
        (l0, h0), (l1, h1) = band("below", p[b, 0], 0.0), band("above", p[b, 0], 0.0)
        u, up = rng.random(N), rng.random(N) < 0.5
        level[b] = np.where(up, l1 + (h1 - l1) * u, l0 + (h0 - l0) * u)
    x = _spread(rng.choice([-1.0, 1.0], size=(B, N)) * 10 ** (level / 20), C)
    assert np.abs(side_db(x) - p[:, :1]).min() > 1e-3
    return x


def delayed(x, look):
    x_d = np.zeros_like(x)
    if look < x.shape[-1]:
        x_d[..., look:] = x[..., :x.shape[-1] - look]
    return x_d


def matched_gy(rng, x, look=0):
    """gy = sign(x_d) (0.2 + U[0, 1)): every gy x_d term is positive (zero where the delayed signal is)."""
    return (np.sign(delayed(x, look)) * (0.2 + rng.random(x.shape))).astype(np.float32)


def exact(mode, x, p, gy, look=0, scale=None):
    """dynamics_exact with the cancellation of every control column: -> y, gx, gp (B, 6), cancellation (B, 6) = (sum of |per-sample
    terms|) / |gradient| (1 where the column is exactly zero term by term)."""
    y, gx, gp, absum, _ = idc.dynamics_exact(mode, x, SR, p, gy, look, terms=True, scale=scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        canc = np.where(absum > 0, absum / np.abs(gp), 1.0)
    return y, gx, gp, canc


@functools.lru_cache(maxsize=None)      # computed once, shared by the float32 and float64 tests: callers leave the arrays unchanged
def region_case(mode, region, B, C, N, look, seed=0):
    """-> x, p, gy (float32) and the float64 reference (y, gx, gp, cancellation) of one region case. The attack column's terms carry the
    sign of g[n-1] - g_c[n], which follows the draw: a draw whose cancellation misses the condition (decided on the float64 reference
    alone - one of the 18 region cases, 32.9, on its first draw) is drawn again from the next seed; the tests assert the condition on
    what comes back."""
    live = [j for j in range(6) if j not in zero_columns(mode, region)]
    for attempt in range(4):
        rng = np.random.default_rng(1000 * mode + 100 * REGIONS.index(region) + N + look + seed + 10007 * attempt)
        p = controls(B)
        x = region_signal(rng, region, p, C, N)
        gy = matched_gy(rng, x, look)
        ref = exact(mode, x, p, gy, look)
        if ref[3][:, live].max() <= MAX_CANCELLATION:
            break
    return x, p, gy, ref


@functools.lru_cache(maxsize=None)      # computed once, shared by the float32 and float64 tests: callers leave the arrays unchanged
def hard_knee_case(mode, B, C, N, look=0):
    rng = np.random.default_rng(7000 + mode)
    p = controls(B, hard=True)
    x = hard_knee_signal(rng, p, C, N)
    gy = matched_gy(rng, x, look)
    return x, p, gy, exact(mode, x, p, gy, look)


@functools.lru_cache(maxsize=None)      # computed once, shared by the float32 and float64 tests: callers leave the arrays unchanged
def edge_case(mode, B, C, N, look):
    """Speech-like signal, controls drawn from the modules' ranges, gy = randn: the inputs of the existing comparisons."""
    rng = np.random.default_rng(31 * N + 7 * look + B + 500 * mode)
    x = idc.speechlike(rng, B, C, N)
    p = idc.dyn_params(rng, B)
    gy = rng.standard_normal((B, C, N)).astype(np.float32)
    return x, p, gy, exact(mode, x, p, gy, look)


def zero_columns(mode, region, hard=False):
    """Columns of gp that are exactly zero: no dependence on threshold, ratio, attack and knee where the curve is the identity (the
    smoothed gain is identically 0 there, so the attack column vanishes with it); release_ms always; knee_db at a hard knee and wherever
    no sample lies inside the knee (the straight branches do not hold the knee width)."""
    z = {3}
    if (mode == 0 and region == "below") or (mode == 1 and region == "above"):
        z |= {0, 1, 2, 4}
    if hard or region != "knee":
        z.add(4)
    return sorted(z)


def col_errors(gp, ref):
    """Per column: max over the items |gp - ref| / max |ref| (0 where the reference column is exactly zero and gp is too)."""
    gp = np.asarray(gp, np.float64)
    e, s = np.abs(gp - ref).max(0), np.abs(ref).max(0)
    return np.where(s > 0, e / np.where(s > 0, s, 1.0), np.where(e > 0, np.inf, 0.0))
