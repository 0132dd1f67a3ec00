"""The table of tests/test_gpu_autograd_contract.py and tests/test_autograd_contract_cpu.py (not collected): one entry per differentiable
public entry point of dasp_pytorch_amd and, where it has two, per binding (config.plan.torch_ops). The checks that run over it are in
tests/autograd_contract_checks.py.

An entry is a checks.Spec: inputs from a seed, the differentiable leaves, the call, the float64 reference the op's parity test already
uses, and that test's bounds - cited in `cite`, taken as they stand. Shapes are the smallest that reach each launch shape, three items
with their own controls. Builders, references and most bounds come from the tables of the earlier off-domain tests:
tests/input_domain_cases.py (the original effects), tests/level_mix_input_domain_cases.py (levels, stereo_mix, the oversampler) and
tests/loss_input_domain_cases.py (the losses and spectral ops).

How equal two runs of one computation must be (`same`): bit for bit unless an existing test documents a sum whose order is not fixed -
  segmented dynamics, control gradients     1e-4 of each control's largest entry (tests/test_gpu_input_domain.py:135-136, test_gpu_dynamics.py:336)
  reverb (band split)                       y / grad x 2e-6, control gradients 1e-5 (tests/test_gpu_input_domain.py:137-138, test_gpu_reverb.py:184-185)
  STFT losses, gradients                    1e-5 of the largest entry (tests/test_gpu_mrstft_options.py:208)
  modulated_delay, grad x                   2e-6 of the peak (tests/test_gpu_modulated_delay.py:9-10, 66-68)
Kinds of bound: those of tests/input_domain_cases.errors, plus "each1" |d| <= b max(1, |ref|) per element, "rowl2" / "rowmax" relative
L2 norm / largest entry per row of the last axis, "l2" relative L2 norm of the whole array, "item_l2" per item, "abs" |d| <= b, and "freqz32"
|d| <= 1e-6 |ref| + 1e-7 max|ref row| (tests/test_gpu_freqz.py:350)."""
import functools

import numpy as np
import torch

from tests import input_domain_cases as idc
from tests import level_mix_input_domain_cases as lmc
from tests import loss_input_domain_cases as lc
from tests.autograd_contract_checks import Spec

DEV = "cuda:0"
SR = 44100
FLT_MIN = idc.FLT_MIN


def D():
    import dasp_pytorch_amd
    return dasp_pytorch_amd


# ---- comparison at an op's existing bound ------------------------------------------------------------------------------------------------

def as_np(v):
    if isinstance(v, torch.Tensor):
        v = v.detach()
        v = torch.view_as_real(v.resolve_conj()) if v.is_complex() else v
        return v.double().cpu().numpy()
    v = np.asarray(v)
    if np.iscomplexobj(v):
        v = np.stack([v.real, v.imag], -1)
    return v.astype(np.float64)


def peak_err(a, b):
    """Largest difference relative to the peak of b: the measure of the fused effects' parity tests."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def errors(kind, got, ref):
    """-> (error, scale) arrays: the bound asks error <= b * scale."""
    d = np.abs(got - ref)
    if kind == "each1":
        return d, np.maximum(1.0, np.abs(ref))
    if kind == "abs":
        return d, np.ones_like(d)
    if kind in ("rowl2", "rowmax"):
        d2, r2 = d.reshape(-1, d.shape[-1]), ref.reshape(-1, ref.shape[-1])
        return (np.sqrt((d2 ** 2).sum(1)), np.sqrt((r2 ** 2).sum(1))) if kind == "rowl2" else (d2.max(1), np.abs(r2).max(1))
    if kind == "item_l2":
        d2, r2 = d.reshape(d.shape[0], -1), ref.reshape(ref.shape[0], -1)
        return np.sqrt((d2 ** 2).sum(1)), np.sqrt((r2 ** 2).sum(1))
    if kind == "l2":
        return np.array([np.sqrt((d ** 2).sum())]), np.array([np.sqrt((ref ** 2).sum())])
    if kind == "freqz32":              # ref (rows, bins, 2)
        mag = np.sqrt((ref ** 2).sum(-1))
        return np.sqrt((d ** 2).sum(-1)), mag + 0.1 * mag.max(-1, keepdims=True)
    if got.ndim == 0:
        got, ref = got.reshape(1), ref.reshape(1)
    return idc.errors(kind, got, ref, 0.0, False)


def comparer(tol, groups=None):
    """compare(keys, got, want, rec, what) of a Spec: tol {key: [(kind, bound), ...]}; groups {key: member keys}, the members flattened per
    item and joined along axis 1 (18 control gradients as one (bs, 18) matrix, as the parity tests judge them). A member that `got` does
    not hold (a subset run) is taken from `want`, where `want` is another run."""
    groups = groups or {}
    owner = {m: g for g, ms in groups.items() for m in ms}

    def joined(d, key, fill=None):
        if key not in groups or d.get(key) is not None:
            return as_np(d[key])
        cols = []
        for m in groups[key]:
            v = d.get(m)
            cols.append(as_np(v if v is not None else fill[m]))
        return np.concatenate([c.reshape(c.shape[0], -1) for c in cols], 1)

    def compare(keys, got, want, rec, what):
        find, done = [], set()
        for k in keys:
            key = owner.get(k, k)
            if key in done or key not in tol:
                continue
            done.add(key)
            W = joined(want, key)
            G = joined(got, key, want).reshape(W.shape)
            if not np.isfinite(G).all():
                find.append(f"{what} {key}: non-finite")
                continue
            if key in groups:                                   # a control without a path to the output (release_ms): exactly zero
                dead = ~W.reshape(W.shape[0], -1).any(0)
                if G.reshape(G.shape[0], -1)[:, dead].any():
                    find.append(f"{what} {key}: a gradient that is exactly 0 in the reference is not")
            for kind, bound in tol[key]:
                e, s = errors(kind, G, W)
                worst = float(np.max(e / np.maximum(s, 1e-300))) if np.max(e) > 0 else 0.0
                rec.append((what, f"{key}:{kind}", worst))
                if not np.all(e <= bound * s + FLT_MIN + (1e-6 if kind == "fd" else 0.0)):
                    find.append(f"{what} {key}: {worst:.3e} ({kind}), bound {bound}")
        return find
    return compare


def lists(tol):
    return {k: (v if isinstance(v, list) else [v]) for k, v in tol.items()}


# ---- entries built on tests/input_domain_cases.py ----------------------------------------------------------------------------------------

SEG_SAME = {"g_params.%02d" % i: 1e-4 for i in range(6)}
REV_SAME = dict({"y0": 2e-6, "g_x": 2e-6}, **{"g_params.%02d" % i: 1e-5 for i in range(25)})
F64_TOL = dict(y=("peak", 5e-7), g_x=("peak", 5e-7), g_params=("peak", 2e-6), g_sos=("peak", 2e-6), g_b=("peak", 2e-6), g_a=("peak", 2e-6),
               g_gain_db=("max", 5e-7), g_drive_db=("max", 5e-7))          # tests/test_gpu_fp64.py:40-42, 52-54, 62-65, 92-94
# the float64 compressor's six control gradients are judged per column, each against its own largest entry (tests/test_gpu_fp64.py:76-81:
# the columns differ by orders of magnitude)
F64_DYN_TOL = dict(F64_TOL, g_params=("col", 2e-6))
VECTOR_CONTROLS = ("gain_db", "drive_db", "width", "pan", "send_db")


def from_idc(case_name, shape, reaches, binding=None, f64=False, plan=None, kw=None, name=None, same=None, twice=None, lowp=True, cite="",
             f64_controls=True):
    case, kw = idc.BY_NAME[case_name], dict(kw or {})
    B, C, N = shape
    dt = torch.float64 if f64 else torch.float32
    plan = dict(plan or {})
    if binding is not None:
        plan["torch_ops"] = binding == "torch_ops"
    name = name or case_name + ("_f64" if f64 else "") + ("[%s]" % binding if binding else "")

    @functools.lru_cache(maxsize=4)
    def arrays(seed):
        a, _ = idc.make(case, 100 + seed, B, C, N, SR, **kw)
        return a

    def make(seed, device=None):
        out = {}
        for k, v in arrays(seed).items():
            if k in case.cols:
                for i in range(v.shape[1]):
                    out["%s.%02d" % (k, i)] = torch.from_numpy(np.ascontiguousarray(v[:, i])).to(device or DEV).to(dt)
            else:
                out[k] = torch.from_numpy(np.array(v)).to(device or DEV).to(dt)
        return out

    a0 = arrays(0)
    leaves, groups, forms = [], {}, {}
    for k in case.grads:
        if k in case.cols:
            members = ["%s.%02d" % (k, i) for i in range(a0[k].shape[1])]
            leaves += members
            groups["g_" + k] = ["g_" + m for m in members]
            forms.update({m: "vector" for m in members})
        else:
            leaves.append(k)
            if k != "x":
                forms[k] = "vector" if k in VECTOR_CONTROLS and a0[k].size <= B * 8 else "matrix"

    def call(t):
        t2 = dict(t)
        for k in case.cols:
            t2[k] = [t["%s.%02d" % (k, i)] for i in range(a0[k].shape[1])]
        return case.call(D(), SR, t2, **kw)

    def reference(seed, gys):
        a = dict(arrays(seed))
        if case_name == "reverb_seed":
            from dasp_pytorch_amd import ops
            a["_noise"] = ops.reverb_noise(idc.REVERB_SEED, B, 12, kw["L"] + kw["taps"] - 1, DEV).cpu().numpy()
        ref = case.ref(SR, a, as_np(gys[0]), **kw)
        ref["y0"] = ref.pop("y")
        return ref

    tol = dict(idc.tol_for(case, N))
    if f64:
        tol = {k: (F64_DYN_TOL if case.segment == "dyn" else F64_TOL)[k] for k in tol}
    tol["y0"] = tol.pop("y")
    return Spec(name, make, call, leaves, audio=("x",), device=DEV, same=same, compare=comparer(lists(tol), groups), reference=reference,
                lowp=("x",) if lowp and not f64 else (), forms=forms, twice=twice, plan=plan, reaches=reaches, f64_controls=f64_controls,
                groups=groups, outs=lambda seed: [(idc.out_shape(case, arrays(seed)), False)], on_device=case_name == "reverb_seed",
                cite=cite or "tests/input_domain_cases.py (%s)" % case_name)


def idc_entries():
    E = []
    S3, SEG1 = (3, 2, 1028), 1
    both = ("ctypes", "torch_ops")
    for b in both:
        t = b == "torch_ops"
        E.append(from_idc("gain", S3, ("dasp::gain",) if t else ("GainFunction",), b))
        E.append(from_idc("distortion", S3, ("dasp::distortion",) if t else ("DistortionFunction",), b))
        for seg in (False, True):
            plan = {"sos_segment_tiles": SEG1} if seg else {"sos_segment": False}
            sfx = "_seg" if seg else ""
            E.append(from_idc("parametric_eq", S3, ("dasp::parametric_eq",) if t else ("ParametricEQFunction",), b, plan=plan,
                              name=f"parametric_eq{sfx}[{b}]", twice=("params.00", "params.03")))
            E.append(from_idc("parametric_eq_shared", S3, ("dasp::parametric_eq",) if t else ("ParametricEQFunction",), b, plan=plan,
                              name=f"parametric_eq_shared{sfx}[{b}]"))
            E.append(from_idc("sosfilt_s3", S3, ("dasp::sosfilt",) if t else ("SosFiltFunction",), b, plan=plan, name=f"sosfilt_s3{sfx}[{b}]"))
            plan = {"dyn_segment_tiles": SEG1} if seg else {"dyn_segment": False}
            same = SEG_SAME if seg else None
            E.append(from_idc("compressor", S3, ("dasp::dynamics",) if t else ("DynamicsFunction",), b, plan=plan, same=same,
                              name=f"compressor{sfx}[{b}]", twice=("params.02", "params.03")))
            E.append(from_idc("compressor_look3", S3, ("dasp::dynamics",) if t else ("DynamicsFunction",), b, plan=plan, same=same,
                              name=f"compressor_look3{sfx}[{b}]"))
            E.append(from_idc("expander", S3, ("dasp::dynamics",) if t else ("DynamicsFunction",), b, plan=plan, same=same,
                              name=f"expander{sfx}[{b}]"))
        for C in (2, 1):
            rk = dict(L=256, taps=31)
            tag = "" if C == 2 else "_mono"
            E.append(from_idc("reverb_noise", (2, C, 100), ("dasp::noise_shaped_reverb",) if t else ("ReverbFunction", "_StackColumns"), b, kw=rk,
                              same=REV_SAME, name=f"reverb_noise{tag}[{b}]"))
            E.append(from_idc("reverb_seed", (2, C, 100), ("dasp::noise_shaped_reverb",) if t else ("ReverbFunction", "_StackColumns"), b, kw=rk,
                              same=REV_SAME, name=f"reverb_seed{tag}[{b}]"))
    E.append(from_idc("distortion_sample", S3, ("DistortionSampleFunction",)))
    # (no low-precision run: lfilter_via_fsm rounds the coefficients to x's dtype, as the reference's type_as does)
    E.append(from_idc("lfilter_k2", (3, 1, 1028), ("SosFiltFunction",), plan={"torch_ops": False}, lowp=False))
    E.append(from_idc("lfilter_k11", (3, 1, 1028), ("LFilterFunction",), lowp=False))
    E.append(from_idc("stereo_widener", S3, ("WidenerFunction",)))
    E.append(from_idc("stereo_panner", S3, ("PannerFunction",)))
    E.append(from_idc("stereo_bus", S3, ("BusFunction",)))
    E.append(from_idc("chain_forward_saving", S3, ("dasp::eq_dyn_norm",), name="eq_dyn_norm[torch_ops]", plan={"torch_ops": True}, lowp=False, f64_controls=False))     # (float32 only: chain.py takes the unfused pair otherwise)
    # the five float64 functions of ops64.py
    E.append(from_idc("gain", S3, ("Elementwise64Function",), f64=True))
    E.append(from_idc("distortion", S3, ("Elementwise64Function",), f64=True))
    E.append(from_idc("parametric_eq", S3, ("ParametricEQ64Function",), f64=True))
    E.append(from_idc("sosfilt_s3", S3, ("SosFilt64Function",), f64=True))
    E.append(from_idc("lfilter_k11", (3, 1, 1028), ("LFilterFunction",), f64=True))
    E.append(from_idc("compressor", S3, ("Dynamics64Function",), f64=True))
    return E


# ---- entries with their own builders -----------------------------------------------------------------------------------------------------

def simple(name, arrays, call, leaves, audio, reaches, tol=None, ref=None, groups=None, outs=None, **kw):
    """arrays(seed) -> {name: CPU tensor}; ref(arrays, gys as float64 numpy) -> {key: array}; outs(arrays) -> the outputs' shapes (a
    complex one as (shape, True)), default: one output shaped like x."""
    cached = functools.lru_cache(maxsize=4)(arrays)

    def make(seed, device=None):
        return {k: v.to(device or DEV).clone() for k, v in cached(seed).items() if not k.startswith("_")}

    def reference(seed, gys):
        return ref(cached(seed), [as_np(g) for g in gys])

    def out_shapes(seed):
        a = cached(seed)
        shapes = outs(a) if outs else [tuple(a["x"].shape)]
        return [s if len(s) == 2 and isinstance(s[1], bool) else (tuple(s), False) for s in shapes]
    return Spec(name, make, call, leaves, audio=audio, device=DEV, compare=comparer(lists(tol), groups) if tol else None,
                reference=reference if ref else None, reaches=reaches, groups=groups, outs=out_shapes, **kw)


def gen(seed, *salt):
    return torch.Generator().manual_seed(7919 * seed + sum(int(s) * (31 ** i) for i, s in enumerate(salt)) % 100003)


def peq_norm_entries():
    """The normalised (bs, 18) tensor, and a parameter batch of 1 shared by all items, through both bindings."""
    out = []
    lo, span = idc.chain_tables(SR)
    for shared in (False, True):
        for b in ("ctypes", "torch_ops"):
            def arrays(seed, shared=shared):
                g = gen(seed, 1, shared)
                return dict(x=torch.rand(3, 2, 1028, generator=g) * 2 - 1, pn=torch.rand(1 if shared else 3, 18, generator=g) * 0.9 + 0.05)

            def call(t):
                from dasp_pytorch_amd import ops
                from dasp_pytorch_amd.functional import _PEQ_TYPES
                return ops.parametric_eq_norm(t["x"], t["pn"], float(SR), _PEQ_TYPES, lo, span)

            def ref(a, gys):
                p = np.asarray(lo) + a["pn"].double().numpy() * np.asarray(span)
                y, gx, gp = idc.peq_exact(a["x"].numpy(), SR, p, gys[0])
                return dict(y0=y, g_x=gx, g_pn=gp * np.asarray(span))
            tol = dict(y0=("abs1", 2e-5), g_x=("abs1", 2e-5), g_pn=("max", 1e-4))    # tests/test_gpu_sosfilt.py:118-119, tests/test_gpu_chain.py:215
            out.append(simple(f"parametric_eq_norm{'_shared' if shared else ''}[{b}]", arrays, call, ("x", "pn"), ("x",),
                              ("dasp::parametric_eq_norm",) if b == "torch_ops" else ("ParametricEQNormFunction",), tol, ref,
                              plan={"torch_ops": b == "torch_ops", "sos_segment": False}, forms={"pn": "matrix"}, lowp=("x",),
                              cite="tests/test_gpu_sosfilt.py:118-119, tests/test_gpu_chain.py:215"))
    return out


def dyn_matrix_entries():
    """compressor / expander on the (bs, 6) matrix and on the (bs, 5) rows the kernels read, with and without look-ahead."""
    out = []

    def arrays(seed):
        rng = np.random.default_rng(300 + seed)
        a = idc._build_dyn(rng, 3, 2, 1028, SR)
        return dict(x=torch.from_numpy(a["x"]), controls=torch.from_numpy(a["params"]))
    for mode, look in ((0, 0), (0, 3), (1, 0)):
        def ref(a, gys, mode=mode, look=look):
            x, p = a["x"].numpy(), a["controls"].numpy()
            y, gx, gp = idc.compressor_ref(x, SR, p, gys[0], look) if mode == 0 else idc.dynamics_exact(1, x, SR, p, gys[0])
            return dict(y0=y, g_x=gx, g_controls=gp)
        tol = idc.COMP_TOL if mode == 0 else idc.EXP_TOL
        tol6 = dict(y0=tol["y"], g_x=tol["g_x"], g_controls=tol["g_params"])
        tag = ("compressor" if mode == 0 else "expander") + ("_look3" if look else "")

        def call6(t, mode=mode, look=look):
            from dasp_pytorch_amd import functional as F
            return F._dynamics_from_matrix(mode, t["x"], SR, t["controls"], lookahead_samples=look)
        out.append(simple(f"{tag}_matrix", arrays, call6, ("x", "controls"), ("x",), ("DynamicsMatrixFunction",), tol6, ref,
                          plan={"dyn_segment": False}, forms={"controls": "matrix"}, lowp=("x",), cite="tests/test_gpu_dynamics.py:63, 68, 147, 152"))
        for b in ("ctypes", "torch_ops"):
            def arrays5(seed):
                a = arrays(seed)
                return dict(x=a["x"], ctl=a["controls"][:, [0, 1, 2, 4, 5]].contiguous(), _p=a["controls"])

            def call5(t, mode=mode, look=look):
                from dasp_pytorch_amd import ops
                return ops.dynamics_ctl(t["x"], mode, float(SR), 1e-8, look, t["ctl"])

            def ref5(a, gys, ref=ref):
                r = ref(dict(x=a["x"], controls=a["_p"]), gys)
                return dict(y0=r["y0"], g_x=r["g_x"], g_ctl=r["g_controls"][:, [0, 1, 2, 4, 5]])
            tol5 = dict(y0=tol["y"], g_x=tol["g_x"], g_ctl=tol["g_params"])
            for seg in (False, True):
                out.append(simple(f"{tag}_ctl{'_seg' if seg else ''}[{b}]", arrays5, call5, ("x", "ctl"), ("x",),
                                  ("dasp::dynamics_ctl",) if b == "torch_ops" else ("DynamicsCtlFunction",), tol5, ref5,
                                  plan={"torch_ops": b == "torch_ops", **({"dyn_segment_tiles": 1} if seg else {"dyn_segment": False})},
                                  same={"g_ctl": 1e-4} if seg else None, forms={"ctl": "matrix"}, lowp=("x",), mutate=("x", "ctl"),
                                  cite="tests/test_gpu_dynamics.py:63, 68, 147, 152"))
    return out


def reverb_matrix_entries():
    """ops.reverb on the (bs, 12) matrices (what the modules call), both bindings; the generated noise with its offset word; and the
    default draw from the CPU generator, stereo and mono."""
    out = []
    L, taps = 256, 31
    rev_out = lambda a: [(a["x"].shape[0], 2, a["x"].shape[2])]

    def arrays(seed, C=2):
        g = gen(seed, 5)
        return dict(x=torch.rand(2, C, 100, generator=g) * 2 - 1, gains=torch.rand(2, 12, generator=g), decays=torch.rand(2, 12, generator=g),
                    mix=torch.rand(2, generator=g), noise=torch.randn(4, 12, L + taps - 1, generator=g))

    def ref(a, gys, noise=None):
        n = {k: v.numpy() for k, v in a.items()}
        if noise is not None:
            n["noise"] = noise
        y = idc.orc.noise_shaped_reverberation(n["x"], SR, n["gains"].astype(np.float64), n["decays"].astype(np.float64), n["mix"].astype(np.float64),
                                               n["noise"], L, taps)
        gx, gg, gd, gm = idc.orc.noise_shaped_reverberation_vjp(n["x"], SR, n["gains"].astype(np.float64), n["decays"].astype(np.float64),
                                                                 n["mix"].astype(np.float64), n["noise"], gys[0], L, taps)
        return dict(y0=y, g_x=gx, g_gains=gg, g_decays=gd, g_mix=gm)
    tol = dict(y0=("peak", 2e-5), g_x=("peak", 2e-5), g_gains=("peak", 1e-4), g_decays=("peak", 1e-4), g_mix=("max", 1e-4))   # tests/test_gpu_reverb.py:60-62
    same = {"y0": 2e-6, "g_x": 2e-6, "g_gains": 1e-5, "g_decays": 1e-5, "g_mix": 1e-5}
    for b in ("ctypes", "torch_ops"):
        def call(t):
            from dasp_pytorch_amd import functional as F
            return F._reverb_from_matrices(t["x"], SR, t["gains"], t["decays"], t["mix"], L, taps, noise=t["noise"])
        out.append(simple(f"reverb_matrices[{b}]", arrays, call, ("x", "gains", "decays", "mix"), ("x",),
                          ("dasp::reverb",) if b == "torch_ops" else ("ReverbFunction",), tol, ref, plan={"torch_ops": b == "torch_ops"}, same=same, outs=rev_out,
                          forms={"gains": "matrix", "decays": "matrix", "mix": "vector"}, lowp=("x",), cite="tests/test_gpu_reverb.py:60-62, 184-185"))

        def arrays_off(seed):
            a = dict(arrays(seed))
            del a["noise"]
            a["offset"] = torch.tensor([3 + seed], dtype=torch.int64)
            return a

        def call_off(t):
            from dasp_pytorch_amd import functional as F
            return F._reverb_from_matrices(t["x"], SR, t["gains"], t["decays"], t["mix"], L, taps, noise_seed=77, noise_seed_offset=t["offset"])

        def ref_off(a, gys):
            """The stream of seed 77 + offset as dasp_reverb_noise writes it out (tests/test_gpu_reverb.py:231, 247): needs the device."""
            from dasp_pytorch_amd import ops
            noise = ops.reverb_noise(77, 2, 12, L + taps - 1, DEV, seed_offset=a["offset"].to(DEV)).cpu().numpy()
            return ref({k: v for k, v in a.items() if k != "offset"}, gys, noise)
        out.append(simple(f"reverb_seed_offset[{b}]", arrays_off, call_off, ("x", "gains", "decays", "mix"), ("x",),
                          ("dasp::reverb",) if b == "torch_ops" else ("ReverbFunction",), tol, ref_off, plan={"torch_ops": b == "torch_ops"}, same=same,
                          outs=rev_out, on_device=True, forms={"gains": "matrix", "decays": "matrix", "mix": "vector"}, lowp=("x",),
                          cite="tests/test_gpu_reverb.py:60-62, 184-185"))

        def call_cpu(t):
            torch.manual_seed(4242)            # the reference's draw: torch.randn on the global CPU generator, made inside the call
            cols = [t[k][:, i] for k in ("gains", "decays") for i in range(12)]
            return D().noise_shaped_reverberation(t["x"], SR, *cols, t["mix"], num_samples=L, num_bandpass_taps=taps)

        def ref_cpu(a, gys):
            state = torch.get_rng_state()
            torch.manual_seed(4242)            # (functional.py:548 of the reference: torch.randn(bs * 2, 12, num_samples + taps - 1))
            noise = torch.randn(4, 12, L + taps - 1).numpy()
            torch.set_rng_state(state)
            return ref(a, gys, noise)
        for C in (2, 1):
            def arrays_cpu(seed, C=C):
                a = dict(arrays(seed, C))
                del a["noise"]
                return a
            out.append(simple(f"reverb_cpu_generator{'' if C == 2 else '_mono'}[{b}]", arrays_cpu, call_cpu, ("x", "gains", "decays", "mix"), ("x",),
                              ("dasp::noise_shaped_reverb",) if b == "torch_ops" else ("ReverbFunction", "_StackColumns"), tol, ref_cpu,
                              plan={"torch_ops": b == "torch_ops"}, same=same, outs=rev_out, forms={"gains": "matrix", "decays": "matrix", "mix": "vector"},
                              lowp=("x",), cite="tests/test_gpu_reverb.py:60-62, 184-185"))
    return out


def chain_controls_entries():
    out = []
    for b in ("ctypes", "torch_ops"):
        def arrays(seed):
            g = gen(seed, 9)
            return {k: torch.rand(3, n, generator=g) * 0.9 + 0.05 for k, n in (("comp", 6), ("rev", 25), ("gain", 1))}

        def call(t):
            from dasp_pytorch_amd import ops
            return ops.chain_controls(t["comp"], t["rev"], t["gain"], *_chain_tables())

        def ref(a, gys):
            """lo + span * p per column in float64 (the tables as the kernel holds them, float32), the chain's gain added to the make-up
            gain, release_ms dropped; the gradients by autograd of that."""
            lo, span = (torch.tensor(list(v), dtype=torch.float64) for v in _chain_tables())
            p = {k: v.double().requires_grad_(True) for k, v in a.items()}
            c = lo[:6] + span[:6] * p["comp"]
            r = lo[6:31] + span[6:31] * p["rev"]
            ctl = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 4], c[:, 5] + lo[31] + span[31] * p["gain"][:, 0]], 1)
            outs = (ctl, r[:, :12], r[:, 12:24], r[:, 24])
            torch.autograd.backward(outs, [torch.from_numpy(g) for g in gys])
            return dict({"y%d" % i: o.detach() for i, o in enumerate(outs)}, **{"g_" + k: v.grad for k, v in p.items()})
        # values: the float32 tables, one fused multiply-add and, for the make-up gain, one more and an add - 4 float32 roundings at the
        # most, 4 x 2^-23 = 4.8e-7 of the tensor's largest entry; gradients: tests/test_gpu_modules.py:209 (1e-5 of the largest entry)
        tol = dict({"y%d" % i: ("max", 4.8e-7) for i in range(4)}, **{"g_" + k: ("max", 1e-5) for k in ("comp", "rev", "gain")})
        out.append(simple(f"chain_controls[{b}]", arrays, call, ("comp", "rev", "gain"), (),
                          ("dasp::chain_controls",) if b == "torch_ops" else ("ChainControlsFunction",), tol, ref, plan={"torch_ops": b == "torch_ops"},
                          outs=lambda a: [(3, 5), (3, 12), (3, 12), (3,)], forms={"comp": "matrix", "rev": "matrix", "gain": "matrix"},
                          cite="tests/test_gpu_modules.py:207-210"))
    return out


@functools.lru_cache(maxsize=1)
def _chain_tables():
    """lo / span of the chain's 32 parameters as the two float[32] arrays dasp_chain_controls takes (chain.StyleTransferChain._tables)."""
    from dasp_pytorch_amd.chain import StyleTransferChain
    return StyleTransferChain(SR)._tables()


def mix_os_delay_entries():
    from tests import modulated_delay_restated as MD
    out = []
    shape = (3, 5, 1501)
    for with_send in (False, True):
        def arrays(seed, with_send=with_send):
            rng = np.random.default_rng(500 + seed)
            B, T, N = shape
            a = dict(x=rng.random(shape) * 2 - 1, gain_db=rng.random((B, T, 1)) * 36 - 24, pan=rng.random((B, T)) * 0.9 + 0.05)
            if with_send:
                a["send_db"] = rng.random((B, T, 1)) * 36 - 24
            return {k: torch.from_numpy(v.astype(np.float32)) for k, v in a.items()}

        def call(t):
            return D().stereo_mix(t["x"], SR, t["gain_db"], t["pan"], t.get("send_db"))

        def ref(a, gys):
            n = {k: v.numpy() for k, v in a.items()}
            r = lmc.MR.compose(n["x"], n["gain_db"], n["pan"], n.get("send_db"), gys[0], gys[1] if len(gys) > 1 else None)
            o = dict(y0=r["mix"], g_x=r["gx"], g_gain_db=r["ggain"], g_pan=r["gpan"])
            if "send_db" in n:
                o.update(y1=r["send"], g_send_db=r["gsend"])
            return o
        names = ("gain_db", "pan") + (("send_db",) if with_send else ())
        tol = dict({k: ("max", lmc.MIX_VAL_TOL) for k in ("y0", "y1", "g_x")}, **{"g_" + k: ("max", lmc.MIX_CTL_TOL) for k in names})
        out.append(simple("stereo_mix" + ("_send" if with_send else ""), arrays, call, ("x",) + names, ("x",), ("StereoMixFunction",), tol, ref,
                          forms={k: "vector" for k in names}, lowp=("x",), twice=("gain_db", "send_db") if with_send else None,
                          outs=lambda a: [(a["x"].shape[0], 2, a["x"].shape[2])] * (2 if "send_db" in a else 1), cite="tests/test_gpu_stereo_mix.py:122"))
    for L in (2, 4, 8):
        B, C, N = lmc.os_shape(L)

        def arrays(seed, L=L, B=B, C=C, N=N):
            g = gen(seed, 61, L)
            return dict(x=torch.rand(B, C, N, generator=g) * 2 - 1, drive_db=torch.rand(B * C, generator=g) * 30 - 6)

        def call(t, L=L):
            return D().oversampled_distortion(t["x"], SR, t["drive_db"], oversample=L)

        def ref(a, gys, L=L):
            w = torch.from_numpy(gys[0])
            r64 = lmc.os_ref(a["x"], a["drive_db"], w, L, 12)
            r32 = lmc.os_ref(a["x"], a["drive_db"], w, L, 12, torch.float32)
            # the bound of tests/test_gpu_oversampled_distortion.py:79-80 travels with the reference: 4 x the float32 restatement's error, floored
            bound = {k: max(4.0 * float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()), lmc.OS_FLOORS[k]) for k in r64}
            return dict(y0=r64["y"], g_x=r64["gx"], g_drive_db=r64["gdrive"], _bound=dict(y0=bound["y"], g_x=bound["gx"], g_drive_db=bound["gdrive"]))
        out.append(measured_bound(f"oversampled_distortion_x{L}", arrays, call, ("x", "drive_db"), ("x",), ("OversampledDistortionFunction",), ref,
                                  dict(y0=lmc.OS_FLOORS["y"], g_x=lmc.OS_FLOORS["gx"], g_drive_db=lmc.OS_FLOORS["gdrive"]),
                                  forms={"drive_db": "vector"}, lowp=("x",), cite="tests/test_gpu_oversampled_distortion.py:79-80"))
    sr, V = 8000, 3
    N = 2 * lmc.lib().dasp_moddelay_tile(MD.delay_samples(sr, 40.0)) + 5
    CTL = ("delay_ms", "depth_ms", "rate_hz", "phase", "mix")

    def arrays(seed):
        g = gen(seed, 131)
        u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
        return dict(x=u(-1.0, 1.0, 3, 2, N), delay_ms=u(5.0, 25.0, 3, V), depth_ms=u(0.0, 4.0, 3, V), rate_hz=u(0.1, 8.0, 3, V), phase=u(0.0, 1.0, 3, V),
                    mix=u(0.2, 1.0, 3))

    def call(t):
        return D().modulated_delay(t["x"], sr, *[t[k] for k in CTL])

    def ref(a, gys):
        w = torch.from_numpy(gys[0])
        r64 = MD.forward_backward(a["x"], sr, *[a[k] for k in CTL], w)
        r32 = MD.forward_backward(a["x"], sr, *[a[k] for k in CTL], w, arith=torch.float32)
        names = dict(y="y0", gx="g_x", gdelay="g_delay_ms", gdepth="g_depth_ms", grate="g_rate_hz", gphase="g_phase", gmix="g_mix")
        floor = dict(y=2e-6, gx=2e-6)
        bound = {names[k]: max(4.0 * float(np.abs(as_np(r32[k]) - as_np(r64[k])).max() / np.abs(as_np(r64[k])).max()), floor.get(k, 1e-5)) for k in names}
        return dict({names[k]: as_np(r64[k]) for k in names}, _bound=bound)
    floors = dict(y0=2e-6, g_x=2e-6, **{"g_" + k: 1e-5 for k in CTL})
    out.append(measured_bound("modulated_delay", arrays, call, ("x",) + CTL, ("x",), ("ModulatedDelayFunction",), ref, floors, same={"g_x": 2e-6},
                              forms={k: "vector" for k in CTL}, lowp=("x",), cite="tests/test_gpu_modulated_delay.py:5-10, 24, 79"))
    return out


def measured_bound(name, arrays, call, leaves, audio, reaches, ref, floors, **kw):
    """An op whose parity bound is 4 x the error of its float64 restatement run in float32 arithmetic, never less than a floor: the
    reference returns the bound with the values ("_bound"); run against run (a subset against all leaves) is held to the floor."""
    spec = simple(name, arrays, call, leaves, audio, reaches, None, ref, **kw)

    def compare(keys, got, want, rec, what):
        bound = want.get("_bound", floors)
        return comparer({k: [("max", bound[k])] for k in floors})(keys, got, want, rec, what)
    spec.compare = compare
    return spec


def delay_filter_limiter_entries():
    """feedback_delay, fdn_reverb, limiter, phaser, time_varying_filter and resample at (3, 2, 1501), every one against its float64
    restatement at its parity test's bound: 4 x the error of the restatement in float32 arithmetic, never below the op's FLOOR (which
    lives beside the restatement: tests/<op>_restated.py)."""
    from tests import fdn_reverb_restated as FDN, feedback_delay_restated as FB, limiter_restated as LIM, phaser_restated as PH
    from tests import resample_restated as RS, tvfilter_restated as TV
    out = []
    sr, N = 8000, 1501

    def entry(name, R, salt, draw, call, restate, reaches, cite, ctl, names=None, forms=None, **kw):
        """draw(u, g) -> the inputs, u(lo, hi, *shape) uniform from the generator g; restate(a, w, **arith) -> R.forward_backward's dict."""
        names = dict(zip(names or R.NAMES, ("y0", "g_x") + tuple("g_" + k for k in ctl)))
        floor = R.FLOOR if isinstance(R.FLOOR, dict) else dict.fromkeys(names, R.FLOOR)

        def arrays(seed):
            g = gen(seed, salt)
            return draw(lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo, g)

        def ref(a, gys):
            w = torch.from_numpy(gys[0])
            r64, r32 = restate(a, w), restate(a, w, arith=torch.float32)
            bound = {names[k]: max(4.0 * peak_err(r32[k], r64[k]), floor[k]) for k in names}
            return dict({names[k]: r64[k] for k in names}, _bound=bound)
        out.append(measured_bound(name, arrays, call, ("x",) + tuple(ctl), ("x",), reaches, ref, {names[k]: floor[k] for k in names},
                                  forms={k: "vector" for k in ctl} if forms is None else forms, lowp=("x",), cite=cite, **kw))

    mdm = 50.0
    entry("feedback_delay", FB, 149,
          lambda u, g: dict(x=u(-1.0, 1.0, 3, 2, N), delay_ms=u(2.0, 45.0, 3), feedback=u(-0.9, 0.9, 3), damping_hz=u(300.0, 6000.0, 3), mix=u(0.2, 1.0, 3)),
          lambda t: D().feedback_delay(t["x"], sr, *[t[k] for k in FB.CTL], max_delay_ms=mdm),
          lambda a, w, **kw: FB.forward_backward(a["x"], sr, *[a[k] for k in FB.CTL], w, max_delay_ms=mdm, **kw),
          ("FeedbackDelayFunction",), "tests/test_gpu_feedback_delay.py check_parity", FB.CTL)
    lines = (53, 71, 97)
    entry("fdn_reverb", FDN, 151,
          lambda u, g: dict(x=u(-1.0, 1.0, 3, 2, N), decay_s=u(0.05, 1.0, 3), damping_hz=u(300.0, 3900.0, 3), mix=u(0.2, 1.0, 3)),
          lambda t: D().fdn_reverb(t["x"], sr, *[t[k] for k in FDN.CTL], lines),
          lambda a, w, **kw: FDN.forward_backward(a["x"], sr, *[a[k] for k in FDN.CTL], lines, w, **kw),
          ("FdnReverbFunction",), "tests/test_gpu_fdn_reverb.py check_parity", FDN.CTL)
    look = 40                                       # lookahead_ms = 5 at 8 kHz
    entry("limiter", LIM, 167,
          lambda u, g: dict(x=0.5 * torch.randn(3, 2, N, generator=g), threshold_db=u(-20.0, -8.0, 3), release_ms=u(5.0, 100.0, 3)),
          lambda t: D().limiter(t["x"], sr, t["threshold_db"], t["release_ms"], lookahead_ms=5.0),
          lambda a, w, **kw: LIM.forward_backward(a["x"], sr, a["threshold_db"], a["release_ms"], w, lookahead=look, **kw),
          ("LimiterFunction",), "tests/test_gpu_limiter.py test_parity_with_the_float64_restatement", LIM.CTL)
    stages = 4
    entry("phaser", PH, 163,
          lambda u, g: dict(x=u(-1.0, 1.0, 3, 2, N), rate_hz=u(0.5, 10.0, 3), center_hz=u(100.0, 800.0, 3), depth=u(0.5, 2.0, 3), phase=u(0.0, 1.0, 3),
                            mix=u(0.2, 1.0, 3)),
          lambda t: D().phaser(t["x"], sr, *[t[k] for k in PH.CTL], stages=stages),
          lambda a, w, **kw: PH.forward_backward(a["x"], sr, *[a[k] for k in PH.CTL], w, stages=stages, **kw),
          ("PhaserFunction",), "tests/test_gpu_phaser.py test_parity_with_the_float64_restatement", PH.CTL)
    hop, mode = 64, "bandpass"
    F = TV.control_frames(N, hop)
    entry("time_varying_filter", TV, 167,
          lambda u, g: dict(x=u(-1.0, 1.0, 3, 2, N), cutoff_hz=u(100.0, 3000.0, 3, F), q=u(0.5, 8.0, 3, F), mix=u(0.2, 1.0, 3)),
          lambda t: D().time_varying_filter(t["x"], sr, *[t[k] for k in TV.CTL], hop=hop, mode=mode),
          lambda a, w, **kw: TV.forward_backward(a["x"], sr, *[a[k] for k in TV.CTL], w, hop, mode, **kw),
          ("TimeVaryingFilterFunction",), "tests/test_gpu_tvfilter.py test_parity_with_the_float64_restatement", TV.CTL,
          forms={"cutoff_hz": "matrix", "q": "matrix", "mix": "vector"})
    o, n, shape = 147, 160, (3, 2, N)
    M = RS.out_len(o, n, N)
    entry("resample", RS, 151,
          lambda u, g: dict(x=torch.rand(*shape, generator=g) * 2 - 1),
          lambda t: D().resample(t["x"], 44100, 48000),
          lambda a, w, **kw: RS.forward_backward(a["x"], w, o, n, **kw),
          ("ResampleFunction",), "tests/test_gpu_resample.py check_parity", (), names=("y", "gx"), outs=lambda a: [shape[:-1] + (M,)])
    return out


def level_entries():
    out = []
    for name in ("one_segment", "segmented"):
        shape, fs, _ = lmc.loud_cases()[name]

        def arrays(seed, shape=shape):
            rng = np.random.default_rng([21, seed, *shape])
            return dict(x=torch.from_numpy((0.3 * rng.standard_normal(shape)).astype(np.float32)))

        def call(t, fs=fs):
            return D().loudness(t["x"], fs)

        def ref(a, gys, fs=fs):
            r = lmc.loud_ref(a["x"].numpy(), fs, gys[0])
            return dict(y0=r["L"], g_x=r["grad"])
        tol = dict(y0=("each1", 2e-5), g_x=[("rowl2", 1e-4), ("rowmax", 1e-4)])
        out.append(simple("loudness_" + name, arrays, call, ("x",), ("x",), ("_LoudnessFunction",), tol, ref, lowp=("x",),
                          outs=lambda a: [(a["x"].shape[0],)], cite="tests/test_gpu_loudness.py:15, 110"))
    shape, fs = (3, 2, 9001), 8000

    def arrays(seed):
        rng = np.random.default_rng([22, seed])
        return dict(x=torch.from_numpy((0.3 * rng.standard_normal(shape)).astype(np.float32)))

    def ref(a, gys):
        y, gx = lmc.R.loudness_normalize(a["x"].numpy(), fs, -23.0, gys[0])
        return dict(y0=y, g_x=gx)
    out.append(simple("loudness_normalize", arrays, lambda t: D().loudness_normalize(t["x"], fs, -23.0), ("x",), ("x",), ("_LoudnessFunction", "dasp::gain"),
                      dict(y0=("l2", 1e-4), g_x=[("l2", 1e-4), ("max", 1e-4)]), ref, lowp=(), cite="tests/test_gpu_loudness.py:237"))

    def arrays_p(seed):
        rng = np.random.default_rng([51, seed])
        return dict(x=torch.from_numpy((0.3 * rng.standard_normal((3, 2, 4097))).astype(np.float32)))

    def ref_p(a, gys):
        y, gx = lmc.peak_ref(a["x"].numpy(), gys[0])
        return dict(y0=y, g_x=gx)
    out.append(simple("peak_normalize", arrays_p, lambda t: D().peak_normalize(t["x"], SR, lmc.PEAK_DB, lmc.PEAK_EPS), ("x",), ("x",), ("_PeakNormFunction",),
                      dict(y0=("max", 3e-7), g_x=[("l2", 1e-6), ("max", 1e-5)]), ref_p, lowp=("x",), cite="tests/test_gpu_loudness.py:255-256"))
    return out


def spectral_entries():
    from tests.freqz_exact import exact_response
    out = []
    for kind in ("sos", "ba"):
        for f64 in (False, True):
            b0, a0, n, _ = lc.freqz_arrays(kind)
            dt = torch.float64 if f64 else torch.float32

            def arrays(seed, b0=b0, a0=a0, dt=dt, kind=kind):
                rng = np.random.default_rng(700 + seed)
                jit = lambda v: torch.from_numpy(v * (1 + 0.01 * rng.standard_normal(v.shape))).to(dt)
                if kind == "sos":
                    return dict(sos=jit(np.concatenate([b0, a0], -1)))
                return dict(b=jit(b0[:, 0]), a=jit(a0[:, 0]))

            def call(t, kind=kind, n=n):
                return D().signal.fft_sosfreqz(t["sos"], n) if kind == "sos" else D().signal.fft_freqz(t["b"], t["a"], n)

            def ref(a, gys, kind=kind, n=n):
                W = gys[0][..., 0] + 1j * gys[0][..., 1]
                if kind == "sos":
                    s = a["sos"].double().numpy()
                    H, gb, ga = exact_response(s[..., :3], s[..., 3:], n, W)
                    return dict(y0=H, g_sos=np.concatenate([gb, ga], -1))
                H, gb, ga = exact_response(a["b"].double().numpy()[:, None], a["a"].double().numpy()[:, None], n, W)
                return dict(y0=H, g_b=gb[:, 0], g_a=ga[:, 0])
            if f64:        # tests/test_gpu_freqz.py:342
                tol = dict(y0=("peak", 1e-12), g_sos=("item_l2", 1e-11), g_ba=("item_l2", 1e-11))
            else:          # tests/test_gpu_freqz.py:350-352
                tol = dict(y0=("freqz32", 1e-6), g_sos=("item_l2", 1e-5), g_ba=("item_l2", 1e-5))
            leaves = ("sos",) if kind == "sos" else ("b", "a")
            out.append(simple(f"fft_{'sos' if kind == 'sos' else ''}freqz{'_f64' if f64 else ''}", arrays, call, leaves, (), ("dasp::freqz",), tol, ref,
                              groups={"g_ba": ["g_b", "g_a"]}, forms={k: "matrix" for k in leaves}, f64_controls=False,
                              outs=lambda a, n=n: [((3, n // 2 + 1), True)], cite="tests/test_gpu_freqz.py:342, 350-352"))
    for n in (64, 16384):
        def arrays(seed, n=n):
            x, H, _ = lc.fdfir_arrays(n, "shared2", seed)
            return dict(x=x, H=H)

        def ref(a, gys, n=n):
            y, gx, gH = lc.fdfir_ref(a["x"], a["H"], torch.from_numpy(gys[0]), n)
            return dict(y0=y.numpy(), g_x=gx.numpy(), g_H=gH.numpy())
        out.append(simple(f"freqdomain_fir_n{n}", arrays, lambda t, n=n: D().signal.freqdomain_fir(t["x"], t["H"], n), ("x", "H"), ("x",),
                          ("dasp::freqdomain_fir",), {k: ("peak", lc.FDFIR_TOL) for k in ("y0", "g_x", "g_H")}, ref,
                          outs=lambda a, n=n: [tuple(a["x"].shape[:-1]) + (n,)], cite="tests/test_gpu_freqdomain_fir.py:16, 110"))
    return out


STFT_RES = ((256, 64, 256), (64, 16, 48))
STFT_SAME = {"g_input": lc.ATOMICS_TOL, "g_target": lc.ATOMICS_TOL}


def loss_entries():
    from dasp_pytorch_amd import losses
    from tests import auraloss_mel_restated as amr, auraloss_restated as ar, auraloss_sumdiff_restated as sdr, auraloss_time_restated as atr
    out = []

    def pair(shape, salt):
        def arrays(seed):
            p, t = lc.generic(shape, 900 + 17 * seed + salt)
            return dict(input=torch.from_numpy(p), target=torch.from_numpy(t))
        return arrays
    res3 = lambda res: dict(fft_sizes=[r[0] for r in res], hop_sizes=[r[1] for r in res], win_lengths=[r[2] for r in res])
    cfgs = [("mrstft_linear", STFT_RES, {}, (2, 2, 4097)), ("mrstft_mel", STFT_RES, dict(scale="mel", n_bins=8, sample_rate=SR), (2, 2, 4097)),
            ("mrstft_aw", STFT_RES, dict(perceptual_weighting=True, sample_rate=SR), (2, 2, 4097)), ("mrstft_8192", lc.BIG, {}, (2, 1, 9000))]
    for name, res, opt, shape in cfgs:
        def call(t, res=res, opt=opt):
            return D().losses.mrstft_loss(t["input"], t["target"], **res3(res), **opt)

        def ref(a, gys, res=res, opt=opt):
            p, t = a["input"].numpy(), a["target"].numpy()
            kw = dict(taps=losses.a_weighting_taps(float(SR))) if opt.get("perceptual_weighting") else {}
            r = amr.loss_and_grads(p, t, res, SR, opt["n_bins"], **kw) if "n_bins" in opt else ar.loss_and_grads(p, t, res, **kw)
            g = float(gys[0])
            return dict(y0=np.asarray(r[0]), g_input=np.asarray(r[1]) * g, g_target=np.asarray(r[2]) * g)
        gb = [("rowl2", 1e-2)] + ([] if "n_bins" in opt else [("rowmax", 2e-2)])
        out.append(simple(name, pair(shape, len(out)), call, ("input", "target"), ("input", "target"), ("_MRSTFTFunction",),
                          dict(y0=("max", lc.LOSS_TOL), g_input=gb, g_target=gb), ref, same=STFT_SAME, lowp=("input", "target"),
                          outs=lambda a: [()], cite="tests/test_gpu_losses.py:40-43, tests/test_gpu_mel_stft.py:78, tests/test_gpu_mrstft_options.py:208"))

    def call_sd(t):
        _, s, d = D().losses.sum_and_difference_stft_loss(t["input"], t["target"], **res3(STFT_RES), output="full")
        return s, d

    def ref_sd(a, gys):
        p, t = (torch.from_numpy(a[k].numpy().astype(np.float64)).requires_grad_(True) for k in ("input", "target"))
        s, d = (ar.mrstft_loss(*[sdr.sum_diff(v)[i] for v in (p, t)], STFT_RES) for i in (0, 1))
        (s * float(gys[0]) + d * float(gys[1])).backward()
        return dict(y0=s.detach().numpy(), y1=d.detach().numpy(), g_input=p.grad.numpy(), g_target=t.grad.numpy())
    out.append(simple("sum_and_difference_stft_loss", pair((2, 2, 4097), 50), call_sd, ("input", "target"), ("input", "target"), ("_SumDiffFunction",),
                      dict(y0=("max", lc.LOSS_TOL), y1=("max", lc.LOSS_TOL), g_input=("item_l2", 1e-2), g_target=("item_l2", 1e-2)), ref_sd,
                      same=STFT_SAME, lowp=("input", "target"), outs=lambda a: [(), ()], cite="tests/test_gpu_sumdiff_stft.py:114, tests/test_gpu_mrstft_options.py:208"))

    def arrays_td(seed):
        rng = np.random.default_rng([0, seed, *lc.TD_SHAPE])
        t = (0.3 * rng.standard_normal(lc.TD_SHAPE)).astype(np.float32)
        return dict(input=torch.from_numpy((t + 0.09 * rng.standard_normal(lc.TD_SHAPE) + 0.05).astype(np.float32)), target=torch.from_numpy(t))
    for red in ("mean", "none"):
        def call_td(t, red=red):
            return D().losses.time_domain_loss(t["input"], t["target"], reduction=red, **lc.td_keywords("mix"))

        def ref_td(a, gys, red=red):
            r = atr.loss_and_grads(a["input"].numpy(), a["target"].numpy(), lc.TD_MIX, reduction=red, upstream=gys[0])
            return dict(y0=np.asarray(r[0]), g_input=np.asarray(r[1]), g_target=np.asarray(r[2]))
        gb = [("rowl2", lc.TD_GRAD_TOL), ("rowmax", lc.TD_GRAD_TOL)]
        out.append(simple("time_domain_loss_" + red, arrays_td, call_td, ("input", "target"), ("input", "target"), ("_TimeDomainFunction",),
                          dict(y0=("max", lc.TD_LOSS_TOL), g_input=gb, g_target=gb), ref_td, lowp=("input", "target"), twice=("input", "target"),
                          outs=lambda a, red=red: [() if red == "mean" else tuple(a["input"].shape[:-1])], cite="tests/test_gpu_time_losses.py:22, 88-95"))
    for ft in ("hp", "aw"):
        def call_fir(t, ft=ft):
            return D().losses.FIRFilter(ft, coef=0.85, fs=SR)(t["input"], t["target"])

        def ref_fir(a, gys, ft=ft):
            taps = np.asarray(D().losses.FIRFilter(ft, coef=0.85, fs=SR)._taps, np.float64)
            p, t, g0, g1 = a["input"].double(), a["target"].double(), torch.from_numpy(gys[0]), torch.from_numpy(gys[1])
            return dict(y0=ar.fir_same(p, taps), y1=ar.fir_same(t, taps), g_input=ar.fir_same_adjoint(g0, taps), g_target=ar.fir_same_adjoint(g1, taps))
        gb = [("l2", 1e-4), ("max", 1e-4)]
        out.append(simple("fir_filter_" + ft, pair((3, 2, 1501), 70), call_fir, ("input", "target"), ("input", "target"), ("_FIRPairFunction",),
                          dict(y0=("max", 2e-5), y1=("max", 2e-5), g_input=gb, g_target=gb), ref_fir, lowp=("input", "target"),
                          outs=lambda a: [tuple(a["input"].shape)] * 2, cite="tests/test_gpu_time_losses.py:230-248"))
    return out


def biquad_entries():
    out = []
    for ft in ("peaking", "high_shelf"):
        def arrays(seed):
            g = gen(seed, 13)
            return dict(gain_db=torch.rand(3, generator=g) * 24 - 12, cutoff_freq=torch.rand(3, generator=g) * 8000 + 100, q_factor=torch.rand(3, generator=g) * 4 + 0.3)

        def ref(a, gys, ft=ft):
            c = [a[k].double().numpy() for k in ("gain_db", "cutoff_freq", "q_factor")]
            b, aa = idc.orc.biquad(*c, SR, ft)
            return dict(y0=b, y1=aa, g_ctl=idc.orc.biquad_vjp(*c, SR, ft, gys[0], gys[1]))
        out.append(simple("biquad_" + ft, arrays, lambda t, ft=ft: D().signal.biquad(t["gain_db"], t["cutoff_freq"], t["q_factor"], SR, ft),
                          ("gain_db", "cutoff_freq", "q_factor"), (), ("BiquadFunction",), dict(y0=("max", 2e-6), y1=("abs", 4e-6), g_ctl=("peak", 1e-5)), ref,
                          groups={"g_ctl": ["g_gain_db", "g_cutoff_freq", "g_q_factor"]}, forms={k: "vector" for k in ("gain_db", "cutoff_freq", "q_factor")},
                          f64_controls=False, outs=lambda a: [(3, 3), (3, 3)], cite="tests/test_gpu_sosfilt.py:492-496"))
    return out


def stack_columns_spec(device="cpu"):
    """functional._StackColumns is pure torch: the one entry that also runs without a GPU, against torch.stack."""
    def make(seed, device=device):
        g = gen(seed, 3)
        return {"c%d" % i: torch.rand(3, generator=g).to(device) for i in range(4)}

    def call(t):
        from dasp_pytorch_amd.functional import _StackColumns
        return _StackColumns.apply(*[t["c%d" % i] for i in range(4)])

    def reference(seed, gys):
        t = {k: v.double().requires_grad_(True) for k, v in make(seed, "cpu").items()}
        y = torch.stack([t["c%d" % i] for i in range(4)], 1)
        y.backward(gys[0].double().cpu())
        return dict(y0=y.detach(), **{"g_" + k: v.grad for k, v in t.items()})
    names = tuple("c%d" % i for i in range(4))
    return Spec("_StackColumns" + ("" if device == "cpu" else "[gpu]"), make, call, names, device=device,
                compare=comparer({k: [("max", 0.0)] for k in ("y0",) + tuple("g_" + n for n in names)}), reference=reference,
                forms={n: "vector" for n in names}, twice=("c0", "c2"), reaches=("_StackColumns",), outs=lambda seed: [((3, 4), False)],
                cite="torch.stack, exactly")


def package_functions():
    """{name: class} of every torch.autograd.Function subclass defined under dasp_pytorch_amd that has a forward of its own (the shared
    bases _ElementwiseFunction / _StereoFunction have none: they are reached through their subclasses)."""
    import dasp_pytorch_amd          # noqa: F401
    from dasp_pytorch_amd import chain, distributed, functional, losses, modules, ops64, signal      # noqa: F401
    out, stack = {}, list(torch.autograd.Function.__subclasses__())
    while stack:
        c = stack.pop()
        stack += c.__subclasses__()
        if c.__module__.startswith("dasp_pytorch_amd") and "forward" in vars(c):
            out[c.__name__] = c
    return out


def registered_ops():
    """The torch.ops.dasp ops with an autograd kernel, read from the fake registrations of _torch_ops.py: the public names (the
    underscored ones are the forward / backward halves those kernels call)."""
    import os
    import re
    import dasp_pytorch_amd
    src = open(os.path.join(os.path.dirname(dasp_pytorch_amd.__file__), "_torch_ops.py")).read()
    return sorted({"dasp::" + n for n in re.findall(r'register_fake\("dasp::(\w+)"\)', src) if not n.startswith("_")})


@functools.lru_cache(maxsize=1)
def table():
    E = (idc_entries() + peq_norm_entries() + dyn_matrix_entries() + reverb_matrix_entries() + chain_controls_entries() + mix_os_delay_entries()
         + delay_filter_limiter_entries() + level_entries() + spectral_entries() + loss_entries() + biquad_entries() + [stack_columns_spec(DEV)])
    for e in E:
        e.functions = lambda names=e.reaches: [c for n, c in package_functions().items() if n in names]
    names = [e.name for e in E]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return E


def by_name():
    return {e.name: e for e in table()}
