"""compressor / expander (csrc/dynamics.hip, csrc/dyn_common.hpp; float64: csrc/ref64.hip dyn64_*) against the analytic float64 adjoint
tests/input_domain_cases.py::dynamics_exact - y, grad x and all six control gradients, through the public functions:

  * by region of the static curve (below the knee, inside it, above it), with the matched upstream gradient, under the condition that no
    compared column cancels by more than 32 (tests/dynamics_exact_cases.py; the reference and the power of these inputs are checked on
    the CPU in tests/test_dynamics_exact_cpu.py): a hand-written partial derivative that is 1 % off misses its bound here by a factor
    of 100 or more;
  * at the edges of the launch shapes: single samples, ragged and exact multiples of the 512-sample tile, the DMA and the register-staged
    backward kernel, more tiles than waves, a look-ahead of a whole tile, of more than a tile and of the whole signal and more;
  * at a hard knee (knee_db = 0);
  * in float64.

No control gradient here is held to a finite-difference bound. Bounds: tests/dynamics_exact_cases.py (measured values beside them;
profiles/r23/dynamics_exact/parity.jsonl)."""
import numpy as np
import pytest
import torch

from tests import dynamics_exact_cases as dx
from tests.util import linf_peak, record

pytestmark = pytest.mark.gpu
SR = dx.SR
MODES = (0, 1)
NAME = {0: "compressor", 1: "expander"}


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def run(D, mode, x, p, gy, look, f64=False):
    dt = torch.float64 if f64 else torch.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)
    xt = dev(x).requires_grad_(True)
    cols = [dev(p[:, i]).requires_grad_(True) for i in range(6)]
    y = (D.compressor if mode == 0 else D.expander)(xt, SR, *cols, lookahead_samples=look)
    assert y.dtype == dt and y.shape == xt.shape
    y.backward(dev(gy))
    torch.cuda.synchronize()
    gp = torch.stack([c.grad for c in cols], 1).cpu().numpy()
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy(), gp


def compare(tag, mode, got, ref, zero=(3,), f64=False):
    """got (y, gx, gp) against ref (y, gx, gp, cancellation): y and grad x per item relative to the item's peak, every control column
    relative to its maximum over the items; the columns `zero` exactly zero. Records first, asserts after."""
    y, gx, gp = got
    yo, gxo, gpo, _ = ref
    assert np.isfinite(y).all() and np.isfinite(gx).all() and np.isfinite(gp).all(), tag
    nothing = not yo.any()                                   # look >= N
    ey = linf_peak(y, yo).max() if not nothing else float(np.abs(y).max())
    egx = linf_peak(gx, gxo).max() if gxo.any() else float(np.abs(gx).max())
    eg = dx.col_errors(gp, gpo)
    record(f"dynamics_exact[{'f64,' if f64 else ''}{NAME[mode]},{tag}]", y=ey, gx=egx, gctl=np.where(np.isfinite(eg), eg, 9.999e99))
    if f64:
        ty, tx, tc = dx.F64_TOL["y"], dx.F64_TOL["g_x"], dx.F64_TOL["g_params"]
    else:
        ty, tx, tc = dx.Y_TOL, dx.GX_TOL[mode], dx.ctl_tol(mode)
    if nothing:
        assert not y.any() and not gx.any() and not gp.any(), tag
        return
    assert ey < ty, (tag, "y", ey)
    assert egx < tx, (tag, "grad x", egx)
    assert np.all(gp[:, list(zero)] == 0), (tag, gp)
    for j in range(6):
        assert eg[j] <= tc, (tag, dx.KEYS[j], eg[j], gp[:, j], gpo[:, j])


def region_check(D, mode, region, B, C, N, look, f64=False):
    x, p, gy, ref = dx.region_case(mode, region, B, C, N, look)
    zero = dx.zero_columns(mode, region)
    live = [j for j in range(6) if j not in zero]
    assert ref[3][:, live].max() <= dx.MAX_CANCELLATION                # the condition of the comparison
    assert np.all(ref[2][:, zero] == 0)
    compare(f"{region},{B},{C},{N},{look}", mode, run(D, mode, x, p, gy, look, f64), ref, zero, f64)


@pytest.mark.parametrize("B,C,N,look", dx.REGION_SHAPES)
@pytest.mark.parametrize("region", dx.REGIONS)
@pytest.mark.parametrize("mode", MODES)
def test_by_region(D, mode, region, B, C, N, look):
    region_check(D, mode, region, B, C, N, look)


@pytest.mark.parametrize("B,C,N,look", dx.EDGE_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_shape_edges(D, mode, B, C, N, look):
    x, p, gy, ref = dx.edge_case(mode, B, C, N, look)
    compare(f"edge,{B},{C},{N},{look}", mode, run(D, mode, x, p, gy, look), ref)


@pytest.mark.parametrize("mode", MODES)
def test_hard_knee(D, mode):
    B, C, N, look = dx.HARD_SHAPE
    x, p, gy, ref = dx.hard_knee_case(mode, B, C, N, look)
    assert ref[3][:, [0, 1, 2, 5]].max() <= dx.MAX_CANCELLATION
    compare(f"hard,{B},{C},{N},{look}", mode, run(D, mode, x, p, gy, look), ref, zero=(3, 4))


@pytest.mark.parametrize("B,C,N,look", dx.REGION_SHAPES)
@pytest.mark.parametrize("region", dx.REGIONS)
@pytest.mark.parametrize("mode", MODES)
def test_float64_by_region(D, mode, region, B, C, N, look):
    region_check(D, mode, region, B, C, N, look, f64=True)


@pytest.mark.parametrize("mode", MODES)
def test_float64_hard_knee(D, mode):
    B, C, N, look = dx.HARD_SHAPE
    x, p, gy, ref = dx.hard_knee_case(mode, B, C, N, look)
    compare(f"hard,{B},{C},{N},{look}", mode, run(D, mode, x, p, gy, look, f64=True), ref, zero=(3, 4), f64=True)


@pytest.mark.parametrize("B,C,N,look", dx.F64_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_float64_shapes(D, mode, B, C, N, look):
    x, p, gy, ref = dx.edge_case(mode, B, C, N, look)
    compare(f"edge,{B},{C},{N},{look}", mode, run(D, mode, x, p, gy, look, f64=True), ref, f64=True)
