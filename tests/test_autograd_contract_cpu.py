"""The autograd-contract battery without a GPU (tests/autograd_contract_checks.py, tests/autograd_contract_cases.py):

* completeness: every torch.autograd.Function defined under dasp_pytorch_amd and every torch.ops.dasp op with an autograd kernel is
  reached by at least one table entry - a new op without an entry fails here;
* the battery catches what it claims: pure-torch toy Functions, one correct and one planted defect per check C1 - C6 (C7 needs two
  streams); every check passes the correct toy and every defect is flagged by its own check and by no other;
* functional._StackColumns, which is pure torch, through C1, C2, C4 and C5 for real, against torch.stack;
* every entry's float64 reference evaluated once on the entry's own small shape (finite, the outputs' and the leaves' shapes); the few
  whose reference is the device's generated noise stream are listed;
* the float64 references of the table against torch.autograd of a float64 torch composition where one exists (gain, distortion, the
  stereo ops, stereo_mix, peak_normalize, the time-domain losses, the FIR filter): subsets and shapes of the references themselves."""
import numpy as np
import pytest
import torch

from tests import autograd_contract_cases as T
from tests import autograd_contract_checks as K
from tests.autograd_contract_checks import Spec

CPU_CHECKS = ("C1_subsets", "C2_repeat", "C3_interleave", "C4_upstream_forms", "C5_leaf_forms", "C6_mutation")


# ---- completeness --------------------------------------------------------------------------------------------------------------------

def test_every_function_and_every_registered_op_has_a_table_entry():
    reached = {r for e in T.table() for r in e.reaches}
    functions, ops = T.package_functions(), T.registered_ops()
    assert len(functions) >= 30 and len(ops) >= 13, (sorted(functions), ops)
    missing = sorted(set(functions) - reached) + sorted(set(ops) - reached)
    assert not missing, f"no entry of tests/autograd_contract_cases.py reaches {missing}"
    unknown = sorted(reached - set(functions) - set(ops))
    assert not unknown, f"the table names {unknown}, which the package does not define"
    for e in T.table():
        assert e.reaches and e.cite, e.name


def test_the_table_covers_both_bindings_and_both_forwards():
    names = [e.name for e in T.table()]
    for op in ("gain", "distortion", "parametric_eq", "parametric_eq_seg", "compressor", "compressor_seg", "expander", "sosfilt_s3", "reverb_noise",
               "reverb_seed", "parametric_eq_norm", "compressor_ctl", "chain_controls", "reverb_matrices"):
        assert f"{op}[ctypes]" in names and f"{op}[torch_ops]" in names, op
    by = T.by_name()
    assert by["parametric_eq_seg[ctypes]"].plan == {"sos_segment_tiles": 1, "torch_ops": False}
    assert by["compressor_seg[torch_ops]"].plan == {"dyn_segment_tiles": 1, "torch_ops": True}
    # the forced segment length does cut the table's rows into segments (the size queries need no GPU)
    L = T.lmc.lib()
    assert L.dasp_sos_segments(1028, 1) == 2 and L.dasp_dyn_segments(1028, 1) >= 2
    assert L.dasp_loudness_segments(3, T.lmc.loud_segmented_n()) > 1 and L.dasp_loudness_segments(3 * 2, 9001) == 1


# ---- toy Functions -------------------------------------------------------------------------------------------------------------------
# y0 = a * b, y1 = 2 a + b for a (3, 2, 7) and one b per item; computed in float32, returned in a's dtype.

_SCRATCH = {}


def _toy(defect=None):
    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            a32, b32 = a.detach().float(), b.detach().reshape(-1).float().contiguous()
            ctx.meta = (a.dtype, b.dtype, b.shape)
            if defect == "ctx_attribute":
                ctx.a, ctx.b32 = a, b32                              # an input kept as a plain attribute: no version check
            else:
                ctx.save_for_backward(a32, b32)
            if defect == "inplace_saved":
                ctx.scale = b32.clone()
            if defect == "module_scratch":
                _SCRATCH["a"] = a32.clone()
            bb = b32.view(-1, 1, 1)
            return (a32 * bb).to(a.dtype), (2 * a32 + bb).to(a.dtype)

        @staticmethod
        def backward(ctx, g0, g1):
            adt, bdt, bshape = ctx.meta
            a32, b32 = (ctx.a.detach().float(), ctx.b32) if defect == "ctx_attribute" else ctx.saved_tensors
            if defect == "module_scratch":
                a32 = _SCRATCH["a"]
            if defect == "inplace_saved":
                b32 = ctx.scale
            if defect == "as_strided":
                c0, c1 = (torch.as_strided(g, g.shape, torch.empty(g.shape).stride(), 0).float() if g.numel() <= g.untyped_storage().nbytes() // g.element_size()
                          else g.float().contiguous() for g in (g0, g1))
            else:
                c0, c1 = g0.float().contiguous(), g1.float().contiguous()
                if defect == "shared_temporary" and not g0.is_contiguous() and not g1.is_contiguous():
                    c0 = c1                                          # the first copy's block, reused by the second
            bb = b32.view(-1, 1, 1)
            ga = c0 * bb + 2 * c1
            gb = (c0 * a32).sum((1, 2)) + c1.sum((1, 2))
            if defect == "inplace_saved":
                ctx.scale.mul_(2.0)
            if defect == "wrong_when_b_frozen" and not ctx.needs_input_grad[1]:
                ga = ga * 1.001
            ga = ga if defect == "float32_for_bf16" else ga.to(adt)
            gb = gb.reshape(bshape).to(bdt)
            if defect == "ignores_needs":
                return ga, gb
            return (ga if ctx.needs_input_grad[0] else None), (gb if ctx.needs_input_grad[1] else None)
    Toy.__name__ = "Toy_" + (defect or "correct")
    return Toy


def toy_spec(defect=None):
    fn = _toy(defect)

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return dict(a=torch.randn(3, 2, 7, generator=g), b=torch.rand(3, generator=g) + 0.5)
    return Spec("toy_" + (defect or "correct"), make, lambda t: fn.apply(t["a"], t["b"]), ("a", "b"), audio=("a",), lowp=("a",),
                forms={"b": "vector"}, functions=lambda: [fn])


DEFECTS = {"ignores_needs": "C1_subsets", "wrong_when_b_frozen": "C1_subsets", "inplace_saved": "C2_repeat", "module_scratch": "C3_interleave",
           "as_strided": "C4_upstream_forms", "shared_temporary": "C4_upstream_forms", "float32_for_bf16": "C5_leaf_forms",
           "ctx_attribute": "C6_mutation"}


def findings(check, spec):
    try:
        return K.CHECKS[check](spec, [])
    except RuntimeError as e:                                        # a backward that raises is a finding too
        return [f"{check} raised {type(e).__name__}: {e}"]


@pytest.mark.parametrize("check", CPU_CHECKS)
def test_the_correct_toy_passes(check):
    rec = []
    assert K.CHECKS[check](toy_spec(), rec) == []
    assert rec, "the check measured nothing"


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_planted_defect_is_flagged_by_its_own_check_only(defect):
    flagged = {check for check in CPU_CHECKS if findings(check, toy_spec(defect))}
    assert flagged == {DEFECTS[defect]}, (defect, {c: findings(c, toy_spec(defect)) for c in flagged})


def test_every_cpu_check_owns_a_defect():
    assert set(DEFECTS.values()) == set(CPU_CHECKS)


# ---- functional._StackColumns: pure torch ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("check", ["C1_subsets", "C2_repeat", "C4_upstream_forms", "C5_leaf_forms"])
def test_stack_columns_holds_the_contract(check):
    spec = T.stack_columns_spec("cpu")
    spec.functions = lambda: [T.package_functions()["_StackColumns"]]
    rec = []
    assert K.CHECKS[check](spec, rec) == []
    assert rec


# ---- the references, against autograd of a float64 torch composition -----------------------------------------------------------------------

def _db(v):
    return 10.0 ** (v / 20.0)


def _pan(x, pan):
    th = pan * (np.pi / 2)                   # the reference's pan law (dasp_pytorch/functional.py:621-626)
    left, right = torch.sqrt((np.pi / 2 - th) * (2 / np.pi) * torch.cos(th)), torch.sqrt(th * (2 / np.pi) * torch.sin(th))
    return torch.stack([x * left[..., None], x * right[..., None]], 1)        # (B, 2, T, N)


def _td_mix(p, t, reduction):
    d = p - t
    eps = 1e-8
    rows = (d ** 2).sum(-1) / ((t ** 2).sum(-1) + eps) + d.mean(-1) ** 2 / ((t ** 2).mean(-1) + eps) + 100.0 * (d ** 2).mean(-1)
    return rows.mean() if reduction == "mean" else rows


def _fir(ft):
    def f(t):
        import torch.nn.functional as F
        from dasp_pytorch_amd import losses
        taps = torch.from_numpy(np.asarray(losses.FIRFilter(ft, coef=0.85, fs=T.SR)._taps, np.float64))
        K_ = taps.numel()
        conv = lambda v: F.conv1d(v.reshape(-1, 1, v.shape[-1]), taps.view(1, 1, K_), padding=K_ // 2).reshape(v.shape)
        return conv(t["input"]), conv(t["target"])
    return f


COMPOSITIONS = {
    "gain[ctypes]": lambda t: t["x"] * _db(t["gain_db"]).view(-1, 1, 1),
    "gain_f64": lambda t: t["x"] * _db(t["gain_db"]).view(-1, 1, 1),
    "distortion[ctypes]": lambda t: torch.tanh(t["x"] * _db(t["drive_db"]).view(t["x"].shape[0], t["x"].shape[1], 1)),
    "distortion_sample": lambda t: torch.tanh(t["x"] * _db(t["drive_db"])),
    "stereo_widener": lambda t: torch.stack([t["x"][:, 0] + (1 - 2 * t["width"].view(-1, 1)) * t["x"][:, 1],
                                             (1 - 2 * t["width"].view(-1, 1)) * t["x"][:, 0] + t["x"][:, 1]], 1),
    "stereo_panner": lambda t: _pan(t["x"], t["pan"]),
    "stereo_bus": lambda t: (t["x"] * _db(t["send_db"]).view(t["x"].shape[0], 1, -1, 1)).sum(2),
    "stereo_mix": lambda t: (_pan(t["x"], t["pan"]) * _db(t["gain_db"]).view(t["x"].shape[0], 1, -1, 1)).sum(2),
    "stereo_mix_send": lambda t: ((_pan(t["x"], t["pan"]) * _db(t["gain_db"]).view(t["x"].shape[0], 1, -1, 1)).sum(2),
                                  (_pan(t["x"], t["pan"]) * _db(t["gain_db"] + t["send_db"]).view(t["x"].shape[0], 1, -1, 1)).sum(2)),
    "peak_normalize": lambda t: t["x"] * _db(torch.tensor(T.lmc.PEAK_DB, dtype=torch.float64)) / t["x"].abs().amax(-1, keepdim=True).clamp(min=T.lmc.PEAK_EPS),
    "time_domain_loss_mean": lambda t: _td_mix(t["input"], t["target"], "mean"),
    "time_domain_loss_none": lambda t: _td_mix(t["input"], t["target"], "none"),
    "fir_filter_hp": _fir("hp"),
    "fir_filter_aw": _fir("aw"),
}


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_reference_against_autograd_of_a_float64_composition(name):
    """Each reference and its gradients, on the table's own small shape and for every leaf, against torch.autograd in float64: 1e-10 of
    the largest entry (both are float64 evaluations of one formula)."""
    spec = T.by_name()[name]
    t = {k: v.double().requires_grad_(k in spec.leaves) for k, v in _cpu_inputs(spec).items()}
    outs = COMPOSITIONS[name](t)
    outs = outs if isinstance(outs, tuple) else (outs,)
    gys = K.upstream(outs, 0)
    torch.autograd.backward(outs, gys)
    ref = spec.reference(0, gys)
    want = {"y%d" % i: o.detach() for i, o in enumerate(outs)}
    want.update({"g_" + n: t[n].grad for n in spec.leaves})
    for k, w in want.items():
        r = T.as_np(ref[k]).reshape(T.as_np(w).shape)
        err = np.abs(r - T.as_np(w)).max() / np.abs(T.as_np(w)).max()
        assert err <= 1e-10, (name, k, err)


def _cpu_inputs(spec):
    return spec.make(0, "cpu")


# the references that are themselves computed with the device: the generated noise stream is written out by dasp_reverb_noise
ON_DEVICE = sorted(e.name for e in T.table() if e.on_device)


def test_the_references_that_need_the_device_are_the_generated_noise_ones():
    assert ON_DEVICE and all(n.startswith(("reverb_seed[", "reverb_seed_mono[", "reverb_seed_offset[")) for n in ON_DEVICE), ON_DEVICE


@pytest.mark.parametrize("name", [e.name for e in T.table() if not e.on_device])
def test_every_reference_evaluates_on_the_table_shape(name):
    """Every entry's float64 reference once, on the entry's own inputs and upstream gradients of the outputs' shapes: every value finite,
    every output of the stated shape, a gradient for every leaf with the leaf's number of elements (a grouped one: the members joined per
    item). A reference that raises at the table's shape is found here, not on the GPU machine."""
    spec = T.by_name()[name]
    assert spec.reference is not None and spec.compare is not None, "an entry without a float64 reference"
    t = spec.make(0, "cpu")
    shapes = spec.outs(0)
    gys = K.upstream([torch.zeros(s, dtype=torch.complex128 if cplx else torch.float64) for s, cplx in shapes], 0)
    ref = spec.reference(0, gys)
    for i, (shape, cplx) in enumerate(shapes):
        y = T.as_np(ref["y%d" % i])
        assert np.isfinite(y).all() and y.shape == tuple(shape) + ((2,) if cplx else ()), (name, i, y.shape, shape)
    members = {m: g for g, ms in spec.groups.items() for m in ms}
    seen = set()
    for leaf in spec.leaves:
        key = members.get("g_" + leaf, "g_" + leaf)
        key = key if key in ref else "g_" + leaf            # (a reference may hold a group's members one by one)
        if key in seen:
            continue
        seen.add(key)
        g = T.as_np(ref[key])
        want = sum(t[m[2:]].numel() for m in spec.groups[key]) if key in spec.groups else t[leaf].numel()
        assert np.isfinite(g).all() and g.size == want * (2 if t[leaf].is_complex() else 1), (name, key, g.shape, want)
