"""The fused EQ -> compressor / expander forward (csrc/chainfwd.hip chain_fwd_kernel: both modes; SEG 0, the SEG 2 + SEG 1 pair of the
segmented launch, and the SAVE variant that feeds both backward kernels) against the composed float64 reference
tests/input_domain_cases.py::chain_grad_exact, on the inputs of tests/chain_exact_cases.py (conditions and power of these inputs:
tests/test_chain_exact_cpu.py):

  1  by region of the static curve, flat and shaped EQ: y of ops.chain_eq_compressor_forward at four shapes (the last one segmented), and
     y, grad x, the EQ-parameter gradient and the five control columns of ops.eq_dynamics_norm at the three one-workgroup shapes;
  2  where the curve is the identity: control columns exactly zero, every output sample its EQ output times ONE float32 factor per item;
  3  what the saving pass hands on: the EQ's output at the EQ's own bound, the smoothing state entering every 512-sample compressor tile
     against the float64 smoothed gain and against the carries the compressor's own forward saves, every entry written;
  4  the expander on ordinary inputs (speech-like signal, random controls and EQ, Gaussian upstream gradient) at the launch-shape edges.

Bounds: tests/chain_exact_cases.py (the project's, the derived 1.74e-4 dB of the carries, and - the expander on ordinary inputs: grad x,
the EQ-parameter gradient and the carries at gains of -300 dB - 4 x the measured error of the unfused sequence, where both miss). The unfused sequence
(ops.parametric_eq_norm, then ops.dynamics_ctl) runs on the same inputs and its errors are recorded beside the fused pass's."""
import numpy as np
import pytest
import torch

from dasp_pytorch_amd import config

from tests import chain_exact_cases as cx
from tests import input_domain_cases as idc
from tests.util import record

pytestmark = pytest.mark.gpu
SR = cx.SR
DEV = "cuda:0"
NAMES = ("y", "g_x", "g_eq_pn", "g_ctl")


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def eq_args():
    from dasp_pytorch_amd.functional import _PEQ_TYPES
    lo, span = idc.chain_tables(SR)
    return _PEQ_TYPES, lo, span


def forward_only(case, mode):
    from dasp_pytorch_amd import ops
    types, lo, span = eq_args()
    with torch.no_grad():
        y = ops.chain_eq_compressor_forward(dev(case["x"]), dev(case["eq_pn"]), types, lo, span, float(SR), dev(case["ctl"]), mode=mode)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def with_gradients(case, mode, fused=True):
    """-> {y, g_x, g_eq_pn, g_ctl} of the saving forward + the two backward kernels (fused) or of the two forward launches (not fused)."""
    from dasp_pytorch_amd import ops
    types, lo, span = eq_args()
    x, pn, ctl = (dev(case[k]).requires_grad_(True) for k in ("x", "eq_pn", "ctl"))
    if fused:
        with config.override(chain_fused_grad=True):
            assert ops.eq_dynamics_norm_ok(x, pn, ctl)
            y = ops.eq_dynamics_norm(x, pn, types, lo, span, float(SR), ctl, mode, 1e-8, None)
    else:
        y = ops.dynamics_ctl(ops.parametric_eq_norm(x, pn, float(SR), types, lo, span), mode, float(SR), 1e-8, 0, ctl)
    y.backward(dev(case["gy"]))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu().numpy(), g_x=x.grad.cpu().numpy(), g_eq_pn=pn.grad.cpu().numpy(), g_ctl=ctl.grad.cpu().numpy())


def saving_forward(case, mode):
    """-> y, yeq, dyn_carries of torch.ops.dasp._eq_dyn_norm_forward (csrc/chainfwd.hip dasp_chain_forward_saving)."""
    types, lo, span = eq_args()
    y, yeq, _, _, dcar = torch.ops.dasp._eq_dyn_norm_forward(dev(case["x"]), dev(case["eq_pn"]), float(SR), [int(v) for v in types], [float(v) for v in lo],
                                                             [float(v) for v in span], dev(case["ctl"]), mode, 1e-8, None)
    torch.cuda.synchronize()
    return y, yeq, dcar


def measure(got, ref, gy, tol, names=NAMES):
    """-> {name: (worst error / scale, bound, ok)} in the metrics of idc.errors: y and grad x per item of the item's peak, the EQ-parameter
    gradient of the tensor's largest entry, every control column of its own maximum."""
    out = {}
    gy_peak = float(np.abs(gy).max())
    for name in names:
        g = np.asarray(got[name], np.float64)
        assert np.isfinite(g).all(), (name, "non-finite")
        kind, bound = tol[name]
        e, s = idc.errors(kind, g.reshape(ref[name].shape), ref[name], gy_peak, name == "y")
        out[name] = (e / np.maximum(s, 1e-300), bound, bool(np.all(e <= bound * s + idc.FLT_MIN)))
    return out


def report(tag, fused, unfused=None):
    row = {k: v[0].max() for k, v in fused.items() if k != "g_ctl"}
    if "g_ctl" in fused:
        row["g_ctl"] = fused["g_ctl"][0]
    if unfused:
        row.update({"unfused_" + k: v[0].max() for k, v in unfused.items()})
    record(f"chain_exact[{tag}]", **row)


def eq_shape_params(shapes, shared_shapes):
    """(eq, B, C, N, shared): both EQ settings at every shape, and one shared row of the shaped EQ (a shared flat row is the flat EQ)."""
    return [(eq,) + s + (False,) for eq in cx.EQS for s in shapes] + [("shaped",) + s + (True,) for s in shared_shapes]


def tag_of(mode, what, B, C, N, shared):
    return f"{cx.NAME[mode]},{what},{B},{C},{N}{',shared' if shared else ''}"


def expect_segments(B, N, monkeypatch):
    """The planner's own choice: (3, 33809) is cut into 3 segments of 16 tiles, the last one of 2 tiles and ragged; the others run as one
    workgroup per item."""
    from dasp_pytorch_amd import _lib
    monkeypatch.setattr(config.plan, "chain_segment", True)
    monkeypatch.setattr(config.plan, "chain_segment_tiles", None)
    tiles = _lib.lib().dasp_chain_segment_tiles(B, N)
    assert tiles == (cx.SEG_TILES if (B, N) == (cx.SEG_SHAPE[0], cx.SEG_SHAPE[2]) else 0), (B, N, tiles)


# ---- 1: by region ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eq,B,C,N,shared", eq_shape_params(cx.FWD_SHAPES, cx.SHARED_SHAPES))
@pytest.mark.parametrize("region", cx.REGIONS)
@pytest.mark.parametrize("mode", cx.MODES)
def test_forward_by_region(D, monkeypatch, mode, region, eq, B, C, N, shared):
    expect_segments(B, N, monkeypatch)
    case = cx.region_case(mode, region, eq, B, C, N, shared)
    cx.check_conditions(case, mode, region)
    m = measure(dict(y=forward_only(case, mode)), case["ref"], case["gy"], cx.tol(mode), ("y",))
    report("forward," + tag_of(mode, f"{region},{eq}", B, C, N, shared), m)
    assert m["y"][2], ("y", m["y"])


@pytest.mark.parametrize("eq,B,C,N,shared", eq_shape_params(cx.GRAD_SHAPES, cx.SHARED_SHAPES[:1]))
@pytest.mark.parametrize("region", cx.REGIONS)
@pytest.mark.parametrize("mode", cx.MODES)
def test_gradients_by_region(D, mode, region, eq, B, C, N, shared):
    case = cx.region_case(mode, region, eq, B, C, N, shared)
    cx.check_conditions(case, mode, region)
    got = with_gradients(case, mode)
    m = measure(got, case["ref"], case["gy"], cx.tol(mode))
    report("grad," + tag_of(mode, f"{region},{eq}", B, C, N, shared), m, measure(with_gradients(case, mode, fused=False), case["ref"], case["gy"], cx.tol(mode)))
    zero = cx.zero_ctl_columns(mode, region)
    assert np.all(got["g_ctl"][:, zero] == 0), (zero, got["g_ctl"])
    for name in NAMES:
        assert m[name][2], (name, m[name])


# ---- 2: where the curve is the identity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C,N", cx.GRAD_SHAPES)
@pytest.mark.parametrize("eq", cx.EQS)
@pytest.mark.parametrize("mode", cx.MODES)
def test_identity_region_is_one_factor_per_item(D, mode, eq, B, C, N):
    """Compressor below the knee, expander above it: the gain computer returns exactly 0 dB, so the smoothed gain is exactly 0 and every
    sample leaves as its EQ output times exp2f(makeup * log2(10) / 20), the same float32 number for the whole item (1.0 for the item
    whose make-up gain is 0 dB). The factor is read off the float64 value and searched within 4 float32 steps of it."""
    region = "below" if mode == 0 else "above"
    case = cx.region_case(mode, region, eq, B, C, N)
    y, yeq, dcar = saving_forward(case, mode)
    assert bool((dcar == 0).all()), dcar
    y, yeq = y.cpu().numpy(), yeq.cpu().numpy()
    for b in range(B):
        f = np.float32(10 ** (float(case["comp"][b, 5]) / 20))
        cands = [f]
        for step in (np.float32(np.inf), np.float32(-np.inf)):
            c = f
            for _ in range(4):
                c = np.nextafter(c, step)
                cands.append(c)
        hits = [c for c in cands if np.array_equal(yeq[b] * c, y[b])]
        assert hits, (b, f, float(np.abs(yeq[b] * f - y[b]).max()))
        if case["comp"][b, 5] == 0:
            assert hits == [np.float32(1.0)] and np.array_equal(y[b], yeq[b])
    assert np.abs(yeq).max() > 0


# ---- 3: what the saving pass hands on --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C,N", cx.GRAD_SHAPES)
@pytest.mark.parametrize("kind", ["knee", "speech"])
@pytest.mark.parametrize("mode", cx.MODES)
def test_saving_pass_hand_offs(D, mode, kind, B, C, N):
    from dasp_pytorch_amd import _lib
    case = cx.region_case(mode, "knee", "shaped", B, C, N) if kind == "knee" else cx.ordinary_case(mode, B, C, N)
    ref = case["ref"]
    y, yeq, dcar = saving_forward(case, mode)
    nt = (N + 511) // 512
    assert dcar.dtype == torch.float32 and dcar.numel() == _lib.lib().dasp_dyn_carry_floats(B, N) == B * nt
    # the carries the compressor's own forward saves when it runs on the fused pass's EQ output
    _, own, _ = torch.ops.dasp._dynamics_forward(yeq, dev(case["ctl"]), mode, float(SR), 1e-8, 0, 0, True)
    torch.cuda.synchronize()
    assert own.numel() == dcar.numel()
    dcar, own = dcar.cpu().numpy().astype(np.float64).reshape(B, nt), own.cpu().numpy().astype(np.float64).reshape(B, nt)
    want = cx.smoothed_gain_at_tiles(case)
    e_eq = idc.errors(idc.EQ_TOL["y"][0], yeq.cpu().numpy(), ref["y1"], 0.0, True)
    e_ref, e_own = np.abs(dcar - want).max(), np.abs(dcar - own).max()
    record(f"chain_exact[handoff,{tag_of(mode, kind, B, C, N, False)}]", yeq=(e_eq[0] / e_eq[1]).max(), carries_vs_float64_db=e_ref, carries_vs_dynamics_forward_db=e_own,
           own_carries_vs_float64_db=np.abs(own - want).max(), largest_gain_db=np.abs(want).max())
    assert np.isfinite(dcar).all()                                 # (the binding allocates the tensor itself: no sentinel; every entry is compared)
    assert np.all(e_eq[0] <= idc.EQ_TOL["y"][1] * e_eq[1]), e_eq
    assert np.all(dcar[:, 0] == 0)
    bound = cx.CARRY_TOL_EXPANDER_SPEECH_DB if (mode, kind) == (1, "speech") else cx.CARRY_TOL_DB
    assert e_ref <= bound, (e_ref, np.abs(dcar - want).max(1))
    assert e_own <= bound, e_own


# ---- 4: the expander on ordinary inputs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C,N", cx.ORDINARY_SHAPES)
def test_expander_on_ordinary_inputs(D, B, C, N):
    mode = 1
    case = cx.ordinary_case(mode, B, C, N)
    got, two = with_gradients(case, mode), with_gradients(case, mode, fused=False)
    m = measure(got, case["ref"], case["gy"], cx.ORDINARY_EXP_TOL)
    report("ordinary," + tag_of(mode, "speech", B, C, N, False), m, measure(two, case["ref"], case["gy"], cx.ORDINARY_EXP_TOL))
    fwd = forward_only(case, mode)
    mf = measure(dict(y=fwd), case["ref"], case["gy"], cx.tol(mode), ("y",))
    # fused against unfused at the bounds of test_fused_training_forward_equals_the_two_launches (tests/test_gpu_chain.py: y 1e-5, grad x 2e-5,
    # parameter gradients 1e-4, each of the tensor's largest entry)
    rel = {k: float(np.abs(got[k] - two[k]).max() / max(np.abs(two[k]).max(), 1e-30)) for k in NAMES}
    record(f"chain_exact[ordinary,fused_vs_unfused,{B},{C},{N}]", forward_only_y=mf["y"][0].max(), **rel)
    for name in NAMES:
        assert m[name][2], (name, m[name])
    assert mf["y"][2], mf["y"]
    assert rel["y"] < 1e-5 and rel["g_x"] < 2e-5 and rel["g_eq_pn"] < 1e-4 and rel["g_ctl"] < 1e-4, rel


@pytest.mark.parametrize("shared", [False, True])
def test_expander_on_ordinary_inputs_segmented_forward(D, monkeypatch, shared):
    mode = 1
    B, C, N = cx.SEG_SHAPE
    expect_segments(B, N, monkeypatch)
    case = cx.ordinary_case(mode, B, C, N, shared)
    m = measure(dict(y=forward_only(case, mode)), case["ref"], case["gy"], cx.tol(mode), ("y",))
    report("ordinary,forward," + tag_of(mode, "speech", B, C, N, shared), m)
    monkeypatch.setattr(config.plan, "chain_segment", False)
    one = measure(dict(y=forward_only(case, mode)), case["ref"], case["gy"], cx.tol(mode), ("y",))
    report("ordinary,forward,one_workgroup," + tag_of(mode, "speech", B, C, N, shared), one)
    assert m["y"][2] and one["y"][2], (m["y"], one["y"])
