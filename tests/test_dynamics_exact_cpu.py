"""What tests/test_gpu_dynamics_exact.py leans on, checked without a GPU (tests/dynamics_exact_cases.py has the inputs):

  * the reference: on the region-isolated inputs dynamics_exact agrees in both modes with central differences of its own forward pass in
    float64 to 1e-7 (control columns, of the column maximum) and 1e-6 (grad x, a directional derivative) - measured <= 1.4e-8 and
    <= 1.6e-7. This is the standing of the reference; the 2e-4 of tests/test_input_domain_cpu.py came from a signal that crosses the kinks;
  * the condition of the GPU comparison: with the matched upstream gradient the cancellation of every compared column of every region case
    is <= 32 (measured: attack 11.3 at the most, the others 1.0);
  * the columns that are exactly zero by region and at a hard knee;
  * the power of the comparison: a reference with ONE derivative formula off by 1 % moves the quantity the GPU test compares by more than
    ten times the bound the GPU test applies to it - in every mode and region where that formula is not zero. The same figure is printed
    (nothing asserted) for a speech-like signal with a Gaussian upstream gradient, the input of the older tests;
  * hard knee and look-ahead beyond the signal in the reference itself."""
import numpy as np
import pytest

from oracle import dasp_oracle as orc
from tests import dynamics_exact_cases as dx
from tests import input_domain_cases as idc
from tests.util import linf_peak

SR = dx.SR
MODES = (0, 1)
NAME = {0: "compressor", 1: "expander"}


def forward(mode, x, p, look):
    return idc.dynamics_exact(mode, x, SR, p, np.zeros_like(x), look)[0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("region", dx.REGIONS)
def test_reference_against_central_differences_inside_a_region(mode, region):
    worst_c, worst_x = 0.0, 0.0
    for C in (1, 2, 3):
        for look in (0, 5, 600):
            B, N = 3, 700
            x, p, gy, (y, gx, gp, _) = dx.region_case(mode, region, B, C, N, look, seed=C)
            x, p, gy = x.astype(np.float64), p.astype(np.float64), gy.astype(np.float64)
            for j in (0, 1, 2, 4, 5):
                h = 1e-6 * np.maximum(1.0, np.abs(p[:, j]))
                pp, pm = p.copy(), p.copy(); pp[:, j] += h; pm[:, j] -= h
                fd = ((forward(mode, x, pp, look) - forward(mode, x, pm, look)) * gy).sum((1, 2)) / (2 * h)
                scale = np.abs(fd).max()
                if j in dx.zero_columns(mode, region):
                    assert scale == 0 and np.all(gp[:, j] == 0), (C, look, dx.KEYS[j])
                    continue
                e = np.abs(gp[:, j] - fd).max() / scale
                worst_c = max(worst_c, e)
                assert e <= 1e-7, (C, look, dx.KEYS[j], gp[:, j], fd)
            rng = np.random.default_rng(C + look)
            # relative steps: every sample stays inside its band. The difference quotient carries the rounding of the forward pass over the
            # step, 1e-16 / 1e-7 = 1e-9 of the sum of |gx v|: a direction whose terms cancel to less than 1 / 100 of that sum (the sum of
            # a random-sign direction can land anywhere near zero: 1 / 4500 for one draw of 54, which then read 2.4e-6) measures that rounding and not the
            # adjoint, and is drawn again - decided on the reference alone
            for _ in range(8):
                v = rng.standard_normal(x.shape) * np.abs(x)
                if np.abs(gx * v).sum() <= 100 * abs((gx * v).sum()):
                    break
            assert np.abs(gx * v).sum() <= 100 * abs((gx * v).sum())
            h = 1e-7
            assert np.all(dx.region_of(x + h * v, p) == dx.REGIONS.index(region)) and np.all(dx.region_of(x - h * v, p) == dx.REGIONS.index(region))
            fd = ((forward(mode, x + h * v, p, look) - forward(mode, x - h * v, p, look)) * gy).sum() / (2 * h)
            e = abs((gx * v).sum() - fd) / abs(fd)
            worst_x = max(worst_x, e)
            assert e <= 1e-6, (C, look, (gx * v).sum(), fd)
    print(f"dynamics_exact vs central differences, {NAME[mode]}, {region}: control columns {worst_c:.2e} (bound 1e-7), grad x {worst_x:.2e} (bound 1e-6)")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("region", dx.REGIONS)
def test_cancellation_of_every_region_case_and_the_exact_zeros(mode, region):
    for B, C, N, look in dx.REGION_SHAPES:
        x, p, gy, (y, gx, gp, canc) = dx.region_case(mode, region, B, C, N, look)
        zero = dx.zero_columns(mode, region)
        print(f"cancellation {NAME[mode]} {region} ({B},{C},{N}) look {look}: " + " ".join(f"{k} {canc[:, j].max():.1f}" for j, k in enumerate(dx.KEYS)))
        assert np.all(gp[:, zero] == 0)
        live = [j for j in range(6) if j not in zero]
        assert np.all(gp[:, live] != 0)
        assert canc[:, live].max() <= dx.MAX_CANCELLATION, canc
        assert np.isfinite(y).all() and np.isfinite(gx).all() and np.abs(y).max() > 0


@pytest.mark.parametrize("mode", MODES)
def test_hard_knee_reference(mode):
    """knee_db = 0: no NaN, the knee column exactly zero, the forward pass equal to the oracle's, cancellation within the condition."""
    B, C, N, look = dx.HARD_SHAPE
    x, p, gy, (y, gx, gp, canc) = dx.hard_knee_case(mode, B, C, N, look)
    assert np.isfinite(y).all() and np.isfinite(gx).all() and np.isfinite(gp).all()
    assert np.all(gp[:, 4] == 0) and np.all(gp[:, 3] == 0) and np.all(gp[:, [0, 1, 2, 5]] != 0)
    assert canc[:, [0, 1, 2, 5]].max() <= dx.MAX_CANCELLATION, canc
    r = dx.region_of(x, p)
    assert (r == 0).any() and (r == 2).any() and not (r == 1).any()
    pd = p.astype(np.float64)
    cols = [pd[:, i] for i in range(6)]
    if mode == 1:
        d = np.abs(y - orc.expander(x, SR, *cols)).max()
        print(f"hard knee, dynamics_exact(1) forward against orc.expander: {d:.1e}")
        assert d <= 1e-15 * np.abs(y).max()
    else:
        e = linf_peak(y, idc.compressor_ref(x, SR, pd, None)).max()
        print(f"hard knee, dynamics_exact(0) forward against the padded orc.compressor: {e:.1e}")
        assert e < 1e-7


@pytest.mark.parametrize("mode", MODES)
def test_reference_with_a_look_ahead_beyond_the_signal(mode):
    """look >= N: the delayed signal is all zero, so the output and every gradient are; look = N - 1 still carries one sample."""
    B, C, N = 2, 1, 300
    rng = np.random.default_rng(3)
    x, p = idc.speechlike(rng, B, C, N), idc.dyn_params(rng, B)
    gy = rng.standard_normal(x.shape)
    for look in (N, N + 1, 2 * N - 1, 2 * N, 1000):
        y, gx, gp, absum, gx_abs = idc.dynamics_exact(mode, x, SR, p, gy, look, terms=True)
        assert not y.any() and not gx.any() and not gp.any() and not absum.any() and not gx_abs.any(), look
    y, gx, gp = idc.dynamics_exact(mode, x, SR, p, gy, N - 1)
    assert y[..., -1].all() and not y[..., :-1].any() and gp[:, 5].all()
    y0 = idc.dynamics_exact(mode, x, SR, p, gy, 0)[0]
    assert np.allclose(y[..., -1] / x[..., 0], y0[..., -1] / x[..., -1], rtol=1e-12)      # the gain curve is not delayed


SCALED = {"d_thr": 0, "d_rat": 1, "d_knee": 4, "d_xdb": None}      # formula -> the control column it feeds (d_xdb: grad x)


def moved(mode, x, p, gy, look, ref, name):
    """How far a reference whose formula `name` is 1 % off moves the quantity the GPU test compares, in the GPU test's own metric."""
    _, gx, gp, _ = dx.exact(mode, x, p, gy, look, scale={name: 1.01})
    if SCALED[name] is None:
        return float(linf_peak(gx, ref[1]).max()), dx.GX_TOL[mode]
    j = SCALED[name]
    return float(dx.col_errors(gp, ref[2])[j]), dx.ctl_tol(mode)


@pytest.mark.parametrize("mode", MODES)
def test_a_derivative_one_percent_off_is_ten_bounds_away(mode):
    for region in dx.REGIONS:
        zero = dx.zero_columns(mode, region)
        for B, C, N, look in dx.REGION_SHAPES:
            x, p, gy, ref = dx.region_case(mode, region, B, C, N, look)
            for name, j in SCALED.items():
                if (0 in zero) if j is None else (j in zero):
                    continue                                # the formula is identically zero in this region
                m, bound = moved(mode, x, p, gy, look, ref, name)
                print(f"1 % off in {name}, {NAME[mode]} {region} ({B},{C},{N}) look {look}: moves by {m:.2e} = {m / bound:.0f} x the bound {bound}")
                assert m > 10 * bound, (region, name, m, bound)
    # the inputs of the older comparisons (speech-like signal, Gaussian upstream gradient): printed, nothing asserted. The column metric
    # is the same 1 % here (a column is linear in its formula), but it is 1 % of a sum that has cancelled: the float32 rounding of the
    # kernel's per-sample terms stands as high beside it as the cancellation printed next to it, and the knee branch is a small share
    B, C, N, look = 2, 2, 4608, 0
    x, p, gy, ref = dx.edge_case(mode, B, C, N, look)
    share = [float((dx.region_of(x, p) == k).mean()) for k in range(3)]
    for name, j in SCALED.items():
        m, bound = moved(mode, x, p, gy, look, ref, name)
        c = "" if j is None else f", cancellation of the column {ref[3][:, j].max():.0f}"
        print(f"1 % off in {name}, {NAME[mode]} speech-like + randn ({B},{C},{N}): moves by {m:.2e} = {m / bound:.0f} x the bound{c}; "
              f"samples below / in the knee / above: {share[0]:.2f} / {share[1]:.2f} / {share[2]:.2f}")


def test_edge_cases_have_finite_references():
    """Every shape-edge case of the GPU file: finite reference, and exact zeros from look >= N on."""
    for mode in MODES:
        for B, C, N, look in dx.EDGE_SHAPES + dx.F64_SHAPES:
            x, p, gy, (y, gx, gp, canc) = dx.edge_case(mode, B, C, N, look)
            assert all(np.isfinite(v).all() for v in (y, gx, gp)), (mode, B, C, N, look)
            if look >= N:
                assert not y.any() and not gx.any() and not gp.any()
