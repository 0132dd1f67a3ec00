"""What tests/test_gpu_chain_exact.py leans on, checked without a GPU (tests/chain_exact_cases.py has the inputs):

  * the reference: the composed float64 adjoint idc.chain_grad_exact (EQ -> compressor / expander) agrees with central differences of its
    own forward pass in float64, at the bounds of tests/test_dynamics_exact_cpu.py: 1e-7 per column (the 5 live control columns and the
    18 EQ parameters, of the column maximum) and 1e-6 for a directional derivative in x;
  * the conditions of the GPU comparison, for every case the GPU file runs: every zero of every EQ section inside the unit circle (the
    pre-distortion is a stable filter), the EQ's output of the float32-rounded x in the wanted region at every sample, the cancellation of
    every live compressor column <= 32;
  * the power of the comparison: a reference with ONE partial derivative of the static curve 1 % off moves at least one quantity the GPU
    test compares by more than ten times its bound, in every mode and region where that derivative is not identically zero. The factors
    are printed for grad x, the EQ-parameter gradient and the control columns."""
import numpy as np
import pytest

from tests import chain_exact_cases as cx
from tests import dynamics_exact_cases as dx
from tests import input_domain_cases as idc
from tests.util import linf_peak

SR = cx.SR


def forward(mode, x, p, comp):
    y1 = idc.peq_exact(x, SR, p)
    return idc.dynamics_exact(mode, y1, SR, comp, np.zeros_like(y1))[0], y1


@pytest.mark.parametrize("eq", cx.EQS)
@pytest.mark.parametrize("region", cx.REGIONS)
@pytest.mark.parametrize("mode", cx.MODES)
def test_composed_adjoint_against_central_differences(mode, region, eq):
    B, C, N = 2, 2, 300
    case = cx.region_case(mode, region, eq, B, C, N)
    cx.check_conditions(case, mode, region)
    x, p, comp, gy = (case[k].astype(np.float64) for k in ("x", "p", "comp", "gy"))
    y, gx, gp, gc, y1 = idc.chain_grad_exact(mode, x, SR, p, comp, gy)
    R = cx.REGIONS.index(region)
    span = np.asarray(idc.chain_tables(SR)[1], np.float64)
    worst_c = worst_p = 0.0
    for j in (0, 1, 2, 4, 5):
        h = 1e-6 * np.maximum(1.0, np.abs(comp[:, j]))
        cp, cm = comp.copy(), comp.copy(); cp[:, j] += h; cm[:, j] -= h
        fd = ((forward(mode, x, p, cp)[0] - forward(mode, x, p, cm)[0]) * gy).sum((1, 2)) / (2 * h)
        if j in dx.zero_columns(mode, region):
            assert not fd.any() and not gc[:, j].any(), dx.KEYS[j]
            continue
        e = np.abs(gc[:, j] - fd).max() / np.abs(fd).max()
        worst_c = max(worst_c, e)
        assert e <= 1e-7, (dx.KEYS[j], gc[:, j], fd)
    assert not gc[:, 3].any()
    # EQ parameters: the five-point central difference (error h^4), steps of 1e-3 dB for a gain (every level moves by less than 2e-3 dB: the
    # region margins are 0.05 dB) and 1e-4 of a frequency or a Q. The three-point form cannot hold 1e-7 here: the output depends on a
    # frequency through n w0 up to n = 300, so its h^2 term is 3e-7 at that step, and a smaller step measures the ~1e-14 of rounding noise
    # of the forward pass instead of the adjoint
    for j in range(18):
        h = np.full(B, 1e-3) if j % 3 == 0 else 1e-4 * np.abs(p[:, j])
        d = []
        for k in (1, 2):
            pp, pm = p.copy(), p.copy(); pp[:, j] += k * h; pm[:, j] -= k * h
            (yp, y1p), (ym, y1m) = forward(mode, x, pp, comp), forward(mode, x, pm, comp)
            assert np.all(dx.region_of(y1p, comp) == R) and np.all(dx.region_of(y1m, comp) == R)      # the step leaves every sample in its branch
            d.append(((yp - ym) * gy).sum((1, 2)))
        fd = (8 * d[0] - d[1]) / (12 * h)
        if eq == "flat" and j % 3:
            # at 0 dB a band is the identity whatever its frequency and Q: zero on both sides, to the rounding of the sums
            assert max(np.abs(fd).max(), np.abs(gp[:, j]).max()) * span[j] <= 1e-7 * np.abs(gp * span).max(), (j, fd, gp[:, j])
            continue
        e = np.abs(gp[:, j] - fd).max() / np.abs(fd).max()
        worst_p = max(worst_p, e)
        assert e <= 1e-7, ("EQ parameter", j, gp[:, j], fd)
    # a direction in x whose terms do not cancel to less than 1 / 100 of their sum (as tests/test_dynamics_exact_cpu.py: the difference
    # quotient carries the rounding of the forward pass over the step), decided on the reference alone
    rng = np.random.default_rng(mode + 10 * R)
    for _ in range(8):
        v = rng.standard_normal(x.shape) * np.abs(x)
        if np.abs(gx * v).sum() <= 100 * abs((gx * v).sum()):
            break
    assert np.abs(gx * v).sum() <= 100 * abs((gx * v).sum())
    h = 1e-7
    (yp, y1p), (ym, y1m) = forward(mode, x + h * v, p, comp), forward(mode, x - h * v, p, comp)
    assert np.all(dx.region_of(y1p, comp) == R) and np.all(dx.region_of(y1m, comp) == R)
    fd = ((yp - ym) * gy).sum() / (2 * h)
    ex = abs((gx * v).sum() - fd) / abs(fd)
    assert ex <= 1e-6, ((gx * v).sum(), fd)
    print(f"chain_grad_exact vs central differences, {cx.NAME[mode]}, {region}, {eq} EQ: control columns {worst_c:.2e}, EQ parameters "
          f"{worst_p:.2e} (bound 1e-7), grad x {ex:.2e} (bound 1e-6)")


def gpu_region_cases():
    """(mode, region, eq, B, C, N, shared) of every region case tests/test_gpu_chain_exact.py runs."""
    out = []
    for mode in cx.MODES:
        for region in cx.REGIONS:
            for eq in cx.EQS:
                out += [(mode, region, eq) + s + (False,) for s in cx.FWD_SHAPES]
                out += [(mode, region, eq) + s + (True,) for s in cx.SHARED_SHAPES if eq == "shaped"]
    return out


@pytest.mark.parametrize("mode", cx.MODES)
@pytest.mark.parametrize("region", cx.REGIONS)
def test_conditions_of_every_gpu_region_case(mode, region):
    for m, r, eq, B, C, N, shared in gpu_region_cases():
        if (m, r) != (mode, region):
            continue
        case = cx.region_case(m, r, eq, B, C, N, shared)
        radius, canc = cx.check_conditions(case, m, r)
        moved = linf_peak(case["ref"]["y1"], case["wanted"].astype(np.float64)).max()
        print(f"{cx.NAME[m]} {r} {eq} ({B},{C},{N}){' shared EQ row' if shared else ''}: zero radius {radius:.5f}, float32 x moves the EQ output by "
              f"{moved:.1e} of its peak, worst cancellation {canc:.1f} (draw {case['attempts']}), peak |x| {np.abs(case['x']).max():.2f}")
        assert moved < 1e-5              # far inside the region margins (0.05 dB = 5.8e-3)


def test_ordinary_cases_have_finite_references():
    for mode in cx.MODES:
        for B, C, N in cx.ORDINARY_SHAPES + cx.GRAD_SHAPES + (cx.SEG_SHAPE,):
            case = cx.ordinary_case(mode, B, C, N)
            assert all(np.isfinite(case["ref"][k]).all() for k in ("y", "g_x", "g_eq_pn", "g_ctl")), (mode, B, C, N)
            if N >= 512:
                assert np.isfinite(cx.smoothed_gain_at_tiles(case)).all()
    for mode in cx.MODES:
        for B, C, N in cx.GRAD_SHAPES:
            g = cx.smoothed_gain_at_tiles(cx.region_case(mode, "knee", "shaped", B, C, N))
            assert g.shape == (B, (N + 511) // 512) and np.isfinite(g).all() and not g[:, 0].any() and g[:, 1:].all()


SCALED = ("d_thr", "d_rat", "d_knee", "d_xdb")
FEEDS = {"d_thr": 0, "d_rat": 1, "d_knee": 4, "d_xdb": None}       # formula -> the control column it feeds (d_xdb: grad x and, through it, the EQ)


def moved_in_bounds(mode, case, name):
    """How far a reference whose formula `name` is 1 % off moves grad x, the EQ-parameter gradient and the control columns, each in the
    GPU test's own metric and in units of the GPU test's own bound."""
    ref, t = case["ref"], cx.tol(mode)
    span = np.asarray(idc.chain_tables(SR)[1], np.float64)
    _, gx, gp, gc, _ = idc.chain_grad_exact(mode, case["x"], SR, case["p"], case["comp"], case["gy"], scale={name: 1.01})
    return {"grad x": float(linf_peak(gx, ref["g_x"]).max()) / t["g_x"][1],
            "EQ parameters": float(np.abs(gp * span - ref["g_eq_pn"]).max() / np.abs(ref["g_eq_pn"]).max()) / t["g_eq_pn"][1],
            "control columns": float(np.max(dx.col_errors(gc[:, [0, 1, 2, 4, 5]], ref["g_ctl"]))) / t["g_ctl"][1]}


@pytest.mark.parametrize("eq", cx.EQS)
@pytest.mark.parametrize("mode", cx.MODES)
def test_a_derivative_one_percent_off_is_ten_bounds_away(mode, eq):
    """d_thr, d_rat and d_knee each feed one control column and nothing else: grad x and the EQ-parameter gradient do not react to them in
    any region (factor 0, printed). d_xdb feeds grad x and through it the EQ-parameter gradient; no control column reacts to it."""
    for region in cx.REGIONS:
        zero = dx.zero_columns(mode, region)
        for B, C, N in cx.GRAD_SHAPES:
            case = cx.region_case(mode, region, eq, B, C, N)
            for name in SCALED:
                j = FEEDS[name]
                if (0 in zero) if j is None else (j in zero):
                    continue                                # the formula is identically zero in this region
                m = moved_in_bounds(mode, case, name)
                print(f"1 % off in {name}, {cx.NAME[mode]} {region} {eq} EQ ({B},{C},{N}): " + ", ".join(f"{k} {v:.0f} bounds" for k, v in m.items()))
                assert max(m.values()) > 10, (region, name, m)
                if j is None:
                    assert m["control columns"] == 0 and m["grad x"] > 10 and m["EQ parameters"] > 10, m
                else:
                    assert m["grad x"] == 0 and m["EQ parameters"] == 0 and m["control columns"] > 10, m
