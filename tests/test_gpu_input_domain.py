"""The original effects (gain, distortion, parametric_eq / sosfilt_via_fsm, lfilter_via_fsm, compressor, expander, the stereo utilities,
noise_shaped_reverberation and the fused EQ -> compressor forward) off their nominal domain - the table and the references are in
tests/input_domain_cases.py:

  A  guard bands and alignment: every caller-supplied tensor as a contiguous view inside a NaN-filled allocation (16-byte aligned:
     bit-equal to stand-alone tensors; 4-byte aligned with N % 4 == 0: inside the oracle bound), as a row slice of a wider NaN tensor, and
     every output of the C ABI inside a sentinel-filled buffer whose guard words must survive the call;
  B  poisoned neighbour: NaN / inf / 1e30 / a NaN control / a NaN upstream gradient in item 1 leave items 0 and 2 bit-identical, and the
     clean batch afterwards is bit-identical to the clean batch before;
  C  silence: exact zeros, zero tails and heads, a cancelling stereo pair, levels below and just above eps, against the float64 references;
  D  sample rates 16 .. 96 kHz against the references at that rate.

Bounds are those of each op's existing shapes-vs-oracle test (restated in the table with their lines). Where the order of a float sum is
documented as not fixed, "equal" means the bound of the existing test that says so: the control gradients of the segmented dynamics
(tests/test_gpu_dynamics.py:336, 1e-4 of the largest entry) and the band-split reverb's float atomics (tests/test_gpu_reverb.py:184-185:
y / grad x 2e-6, control gradients 1e-5). The two fused passes also run with the expander's curve (chain_forward_expander,
chain_forward_saving_expander): their references compare a quantity with the float64 chain only where the float32 rounding of the EQ's
output in front of the expander leaves that possible (tests/input_domain_cases.py, beside EQ_PROBE); every bit-equality, NaN-propagation
and exact-zero part runs for them as for the others."""
import copy
import functools

import numpy as np
import pytest
import torch

from dasp_pytorch_amd import config

from tests import input_domain_cases as idc
from tests.input_domain_cases import CASES, DEV, GUARD
from tests.test_gpu_reverb import reverb_plan
from tests.util import load_golden, record

pytestmark = pytest.mark.gpu
SR = 44100
NAN = float("nan")


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def guarded(a, offset=GUARD, dtype=torch.float32):
    """`a` on the device as a contiguous view `offset` elements into a NaN-filled allocation with GUARD elements of NaN on either side."""
    n = int(np.size(a))
    buf = torch.full((2 * GUARD + n + 8,), NAN, dtype=dtype, device=DEV)
    v = buf[offset:offset + n].view(np.shape(a))
    v.copy_(dev(a).to(dtype))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * offset) % 16 and torch.isnan(buf[:offset]).all() and torch.isnan(buf[offset + n:]).all()
    return v


def misaligned(a):
    v = guarded(a, GUARD + 1)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def row_slice(a):
    """`a` as the slice wide[..., 9:9 + N] of a wider NaN tensor: not contiguous."""
    wide = torch.full(tuple(np.shape(a)[:-1]) + (np.shape(a)[-1] + 21,), NAN, device=DEV)
    v = wide[..., 9:9 + np.shape(a)[-1]]
    v.copy_(dev(a))
    assert not v.is_contiguous()
    return v


def run(case, D, sr, a, gy, place=None, kw=None, dtype=torch.float32):
    """One forward + backward of the case on the arrays a; place[name] puts a tensor on the device (default: a stand-alone tensor)."""
    place = place or {}
    t = {}
    for name, arr in a.items():
        if name.startswith("_"):
            continue
        if name in case.cols:
            t[name] = [dev(arr[:, i]).to(dtype).requires_grad_(True) for i in range(arr.shape[1])]
            continue
        v = place.get(name, dev)(arr).to(dtype)
        t[name] = v.requires_grad_(True) if name in case.grads else v
    y = case.call(D, sr, t, **(kw or {}))
    out = {"y": y.detach()}
    if case.grads:
        y.backward(place.get("gy", dev)(gy).to(dtype))
        for name in case.grads:
            out["g_" + name] = torch.stack([c.grad for c in t[name]], 1) if name in case.cols else t[name].grad
    torch.cuda.synchronize()
    return out


def arrays(case, seed, B, C, N, sr, kw):
    a, gy = idc.make(case, seed, B, C, N, sr, **kw)
    if case.name == "reverb_seed":          # the stream of the seed as dasp_reverb_noise writes it out (tests/test_gpu_reverb.py:231)
        from dasp_pytorch_amd import ops
        a["_noise"] = ops.reverb_noise(idc.REVERB_SEED, B, 12, kw["L"] + kw["taps"] - 1, DEV).cpu().numpy()
    return a, gy


@functools.lru_cache(maxsize=None)
def _reference(name, seed, B, C, N, sr, kwt):
    case, kw = idc.BY_NAME[name], dict(kwt)
    a, gy = arrays(case, seed, B, C, N, sr, kw)
    ref = case.ref(sr, a, gy.astype(np.float64), **kw)
    for v in list(a.values()) + [gy] + list(ref.values()):
        v.setflags(write=False)
    return a, gy, ref


def reference(case, seed, B, C, N, sr=SR, kw=None):
    """(arrays, gy, float64 reference) of a case: computed once per process, shared by the tests and read-only."""
    return _reference(case.name, seed, B, C, N, sr, tuple(sorted((kw or {}).items())))


def configure(monkeypatch, case, segmented=False, lookback=True, torch_ops=True):
    monkeypatch.setattr(config.plan, "torch_ops", torch_ops)
    for k in ("sos", "dyn", "chain"):
        monkeypatch.setattr(config.plan, k + "_segment_tiles", 16 if (segmented and case.segment == k) else None)
    monkeypatch.setattr(config.plan, "lookback", lookback)


def launch_shapes(case, B_plain=None):
    """-> [(B, C, N, kw, segmented, lookback)]: the plain shapes, then the segmented shape in its one-launch and two-launch forms."""
    out = [(B_plain or B, C, N, kw, False, True) for B, C, N, kw in idc.shapes_of(case)]
    if case.segment:
        B, C, N = idc.SEG_SHAPE
        out += [(B_plain or B, C, N, {}, True, True), (B_plain or B, C, N, {}, True, False)]
    return out


def loose_bounds(case, segmented, band_split):
    """The documented not-fixed-order sums: {output name: bound relative to the largest entry} (module docstring)."""
    if case.segment == "dyn" and segmented:
        return {"g_params": (1e-4, True)}                 # every control against its own largest entry
    if case.name.startswith("reverb") and band_split != 1:
        return {"y": (2e-6, False), "g_x": (2e-6, False), "g_params": (1e-5, False)}
    return {}


def assert_same(case, got, base, loose, what, items=None):
    """got == base bit for bit (or inside `loose`), over the batch items `items` (None: everything)."""
    for k, b in base.items():
        g = got[k]
        if items is not None:
            if case.name == "parametric_eq_shared" and k == "g_params":
                continue                               # one parameter row shared by the batch: its gradients sum over the items
            B = base["y"].shape[0]
            g, b = g.reshape(B, -1)[items], b.reshape(B, -1)[items]
        assert torch.isfinite(g).all(), (case.name, what, k, "non-finite")
        if k in loose:
            bound, per_column = loose[k]
            e, m = ((g - b).abs().amax(0), b.abs().amax(0)) if per_column else ((g - b).abs().max(), b.abs().max())
            assert bool((e <= bound * m).all()), (case.name, what, k, e, m)
        else:
            assert torch.equal(g, b), (case.name, what, k, float((g - b).abs().max()))


def splits_of(case):
    return (1, 4) if case.name.startswith("reverb") else (None,)


class maybe_split:
    def __init__(self, split):
        self.cm = reverb_plan(band_split=split) if split else None

    def __enter__(self):
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *exc):
        if self.cm:
            self.cm.__exit__(*exc)


# ---- A1: inputs in guarded views, through the public API ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=str)
def test_a1_inputs_as_offset_views(D, monkeypatch, case):
    for B, C, N, kw, segmented, lookback in launch_shapes(case):
        for torch_ops in ((True, False) if case.bindings else (True,)):
            for split in splits_of(case):
                configure(monkeypatch, case, segmented, lookback, torch_ops)
                a, gy, ref = reference(case, 100 + N, B, C, N, SR, kw)
                what = (B, C, N, segmented, lookback, torch_ops, split)
                tol = idc.tol_for(case, N)
                names = ("x",) + case.big
                with maybe_split(split):
                    base = run(case, D, SR, a, gy, kw=kw)
                    idc.check(case, base, ref, gy, what, tol)
                    loose = loose_bounds(case, segmented, split)
                    # 16-byte aligned views 2048 floats into NaN-filled allocations: the same kernels on the same numbers
                    got = run(case, D, SR, a, gy, dict({n: guarded for n in names}, gy=guarded), kw)
                    assert_same(case, got, base, loose, what + ("aligned views",))
                    # 4-byte aligned views with N % 4 == 0: the scalar kernel variants, picked by the pointers alone
                    assert N % 4 == 0
                    for which in (names + ("gy",), ("gy",), ("x",)):
                        if "gy" in which and not case.grads:
                            continue
                        got = run(case, D, SR, a, gy, {n: misaligned for n in which}, kw)
                        idc.check(case, got, ref, gy, what + ("misaligned",) + which, tol)
                    # a row slice of a wider NaN tensor
                    got = run(case, D, SR, a, gy, dict(x=row_slice, gy=row_slice), kw)
                    assert_same(case, got, base, loose, what + ("row slice",))


# ---- A2: outputs in guarded buffers, through the C ABI --------------------------------------------------------------------------------

SENTINEL = 0x7FC0DEAD          # a quiet-NaN bit pattern no kernel writes


class OutBuf:
    """An output of n floats as a view inside a sentinel-filled buffer, GUARD words before and after."""

    def __init__(self, n, offset):
        self.n, self.offset = int(n), offset
        self.words = torch.full((2 * GUARD + self.n + 8,), SENTINEL, dtype=torch.int32, device=DEV)
        self.view = self.words[offset:offset + self.n].view(torch.float32)
        assert self.view.data_ptr() % 16 == (4 * offset) % 16 and self.view.numel() == self.n

    def payload(self, what):
        torch.cuda.synchronize()
        w = self.words
        assert bool((w[:self.offset] == SENTINEL).all()) and bool((w[self.offset + self.n:] == SENTINEL).all()), (what, "a guard word was written")
        return self.view.clone()


def _abi_ops():
    """name -> function(out) that runs the entry points with every output allocated by out(key, n floats) and returns {key: flat payload};
    inputs, controls and work areas are stand-alone tensors sized by the library's own size functions."""
    import ctypes
    from dasp_pytorch_amd import _lib
    from dasp_pytorch_amd._lib import call, ptr, stream
    L = _lib.lib()
    ops = {}

    def elementwise(name, fwd, bwd, per_sample):
        case = idc.BY_NAME[name]

        def go(out, B=3, C=2, N=1028):
            a, gy = arrays(case, 100 + N, B, C, N, SR, {})
            x, g = dev(a["x"]), dev(gy)
            c = dev(a[case.grads[1]]).reshape(-1)
            y, gx = out("y", x.numel()), out("gx", x.numel())
            if per_sample:
                gc = out("gdrive", x.numel())
                call(fwd, ptr(x), ptr(c), ptr(y), x.numel(), stream())
                call(bwd, ptr(x), ptr(c), ptr(g), ptr(gx), ptr(gc), x.numel(), stream())
                return dict(y=y, gx=gx, gdrive=gc)
            gc = torch.empty_like(c)
            part = torch.empty(L.dasp_ew_partial_floats(B * C, N), dtype=torch.float32, device=DEV)
            call(fwd, ptr(x), ptr(c), ptr(y), B, C, N, stream())
            call(bwd, ptr(x), ptr(c), ptr(g), ptr(gx), ptr(gc), ptr(part), B, C, N, stream())
            return dict(y=y, gx=gx)
        ops[name] = go

    elementwise("gain", "dasp_gain_forward", "dasp_gain_backward", False)
    elementwise("distortion", "dasp_distortion_forward", "dasp_distortion_backward", False)
    elementwise("distortion_sample", "dasp_distortion_sample_forward", "dasp_distortion_sample_backward", True)

    def stereo(name, op, fwd, bwd):
        case = idc.BY_NAME[name]

        def go(out, B=3, C=2, N=1028):
            a, gy = arrays(case, 100 + N, B, C, N, SR, {})
            x, g = dev(a["x"]), dev(gy)
            c = dev(a[case.grads[1]]).reshape(-1)
            T = 1 if op == 0 else (x.shape[1] if op == 1 else x.shape[2])
            dims = (B, N) if op == 0 else (B, T, N)
            y, gx = out("y", g.numel()), out("gx", x.numel())
            gc = torch.empty_like(c)
            part = torch.empty(L.dasp_stereo_partial_floats(op, B, T, N), dtype=torch.float32, device=DEV)
            call(fwd, ptr(x), ptr(c), ptr(y), *dims, stream())
            call(bwd, ptr(x), ptr(c), ptr(g), ptr(gx), ptr(gc), ptr(part), *dims, stream())
            return dict(y=y, gx=gx)
        ops[name] = go

    stereo("stereo_widener", 0, "dasp_widener_forward", "dasp_widener_backward")
    stereo("stereo_panner", 1, "dasp_panner_forward", "dasp_panner_backward")
    stereo("stereo_bus", 2, "dasp_bus_forward", "dasp_bus_backward")

    def sosfilt(out, B=3, C=2, N=8200, S=6):
        """dasp_sosfilt_forward / dasp_sosfilt_backward_ex on a designed EQ, as _raw_setup of tests/test_gpu_sosfilt.py."""
        case = idc.BY_NAME["parametric_eq"]
        a, gy = arrays(case, 100 + N, B, C, N, SR, {})
        x, g = dev(a["x"]), dev(gy)
        p = dev(a["params"].reshape(B, S, 3))
        tab = torch.empty(B * L.dasp_sos_table_floats(S), dtype=torch.float32, device=DEV)
        dtab = torch.empty(B * L.dasp_sos_dtab_doubles(S), dtype=torch.float64, device=DEV)
        types = (ctypes.c_int * S)(1, 0, 0, 0, 0, 2)
        call("dasp_peq_prepare", ptr(p), B, S, types, float(SR), ptr(tab), ptr(dtab), stream())
        car = torch.empty(L.dasp_sos_carry_floats(B * C, N, S), dtype=torch.float32, device=DEV)
        part = torch.empty(L.dasp_sos_partial_floats(B * C, S), dtype=torch.float32, device=DEV)
        y, gx = out("y", x.numel()), out("gx", x.numel())
        call("dasp_sosfilt_forward", ptr(tab), B, ptr(x), ptr(y), ptr(car), B, C, N, S, stream())
        call("dasp_sosfilt_backward_ex", ptr(tab), B, ptr(x), ptr(g), ptr(car), ptr(gx), ptr(part), B, C, N, S, stream())
        return dict(y=y, gx=gx)
    ops["sosfilt"] = sosfilt

    def dynamics(mode):
        def go(out, B=3, C=2, N=8200):
            """dasp_dynamics_forward / _backward, one workgroup per item (Tseg = 0: no segment scratch, no counters), as _ctypes_ops._dyn_forward."""
            case = idc.BY_NAME["compressor" if mode == 0 else "expander"]
            a, gy = arrays(case, 100 + N, B, C, N, SR, {})
            x, g = dev(a["x"]), dev(gy)
            ctl = dev(np.ascontiguousarray(a["params"][:, [0, 1, 2, 4, 5]]))
            car = torch.empty(L.dasp_dyn_carry_floats(B, N), dtype=torch.float32, device=DEV)
            part = torch.empty(L.dasp_dyn_partial_floats(B), dtype=torch.float32, device=DEV)
            gctl = torch.empty(B, 5, dtype=torch.float32, device=DEV)
            y, gx = out("y", x.numel()), out("gx", x.numel())
            none = ctypes.c_void_p(0)
            call("dasp_dynamics_forward", mode, ptr(x), ptr(ctl), ptr(y), ptr(car), none, none, B, C, N, float(SR), 1e-8, 0, 0, none, stream())
            call("dasp_dynamics_backward", mode, ptr(x), ptr(ctl), ptr(g), ptr(car), none, ptr(gx), ptr(gctl), ptr(part), none, B, C, N, float(SR),
                 1e-8, 0, 0, none, stream())
            return dict(y=y, gx=gx)
        return go
    ops["compressor"] = dynamics(0)
    ops["expander"] = dynamics(1)
    return ops


# the y / grad x bound of each op's existing test: elementwise and stereo 2e-6 (tests/test_gpu_elementwise.py:83-84, test_gpu_stereo.py:59-60),
# the EQ 1e-5 / 2e-5 (tests/test_gpu_sosfilt.py:121, 321), the dynamics 2e-5 (tests/test_gpu_dynamics.py:63)
A2_BOUND = dict(gain=2e-6, distortion=2e-6, distortion_sample=2e-6, stereo_widener=2e-6, stereo_panner=2e-6, stereo_bus=2e-6, sosfilt=1e-5,
                compressor=2e-5, expander=2e-5)


@pytest.mark.parametrize("name", list(A2_BOUND))
def test_a2_outputs_inside_guarded_buffers(D, name):
    """Every output of the C-ABI entry points (y, gx, the per-sample drive gradient) as a view inside a sentinel-filled buffer, 16-byte
    and 4-byte aligned: the guard words, compared as int32, are untouched, and the payload is what a stand-alone buffer receives."""
    go = _abi_ops()[name]
    alone = {k: v.clone() for k, v in go(lambda key, n: torch.full((n,), NAN, device=DEV)).items()}
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in alone.values())
    for offset in (GUARD, GUARD + 1):
        bufs = {}

        def out(key, n):
            bufs[key] = OutBuf(n, offset)
            return bufs[key].view
        go(out)
        for key, ob in bufs.items():
            got = ob.payload((name, key, offset))
            if offset % 4 == 0:
                assert torch.equal(got, alone[key]), (name, key, "aligned view")
            else:
                # the scalar variants: the stand-alone call's numbers inside the op's y / grad x bound
                assert ob.view.data_ptr() % 16 == 4
                assert torch.isfinite(got).all()
                bound = A2_BOUND[name] * (2 if (name, key) == ("sosfilt", "gx") else 1)
                assert float((got - alone[key]).abs().max()) <= bound * float(alone[key].abs().max()), (name, key, "misaligned view")


# ---- B: poisoned neighbour ------------------------------------------------------------------------------------------------------------

def poisons(case, N):
    out = [("x", "nan", 0), ("x", "nan", N // 2), ("x", "nan", N - 1), ("x", "inf", N // 2), ("x", "1e30", N // 2)]
    if case.ctl:
        out.append(("ctl", "nan", None))
    if case.grads:
        out.append(("gy", "nan", N // 2))
    return out


@pytest.mark.parametrize("case", CASES, ids=str)
def test_b_poisoned_item_leaves_its_neighbours_alone(D, monkeypatch, case):
    for B, C, N, kw, segmented, lookback in launch_shapes(case, B_plain=3):
        for split in splits_of(case):
            configure(monkeypatch, case, segmented, lookback)
            a, gy, ref = reference(case, 200 + N, B, C, N, SR, kw)
            what = (B, C, N, segmented, lookback, split)
            loose = loose_bounds(case, segmented, split)
            with maybe_split(split):
                base = run(case, D, SR, a, gy, kw=kw)
                idc.check(case, base, ref, gy, what, idc.tol_for(case, N))
                for target, value, pos in poisons(case, N):
                    ap = {k: (v.copy() if not k.startswith("_") else v) for k, v in a.items()}
                    gp = gy.copy()
                    v = dict(nan=NAN, inf=float("inf"))[value] if value != "1e30" else 1e30
                    if target == "x":
                        ap["x"][1].reshape(-1, N)[0, pos] = v
                    elif target == "ctl":
                        ap[case.ctl[0]].reshape(B, -1)[1, case.ctl[1]] = v
                    else:
                        gp[1].reshape(-1, N)[0, pos] = v
                    got = run(case, D, SR, ap, gp, kw=kw)
                    assert_same(case, got, base, loose, what + (target, value, pos), items=[0, 2])
                    if target == "x" and (value == "nan" or (value == "inf" and not case.inf_saturates)):
                        assert not bool(torch.isfinite(got["y"][1][..., pos]).all()), (case.name, what, value, pos, "swallowed")
                    if target == "x" and value == "nan" and case.recursive:
                        # the poisoned row from that sample on, as in the reference (a filter's state; the side chain's clamp is a
                        # torch.clamp, which hands a NaN on to the smoothing state - an fmaxf in its place turns it into silence)
                        row = got["y"][1].reshape(-1, N)[0, pos:]
                        assert not bool(torch.isfinite(row).any()), (case.name, what, pos, "NaN swallowed", int(torch.isfinite(row).sum()))
                    if target == "gy":
                        assert not bool(torch.isfinite(got["g_x"][1][..., pos]).all()), (case.name, what, "NaN in gy swallowed")
                        assert_same(case, dict(y=got["y"]), dict(y=base["y"]), loose, what + ("y with a NaN in gy",))
                # work areas, tag words and counters are left clean
                again = run(case, D, SR, a, gy, kw=kw)
                assert_same(case, again, base, loose, what + ("clean run after the poisoned ones",))


# ---- C: silence and degenerate levels -------------------------------------------------------------------------------------------------

def _silence_applies(case, kind):
    if kind == "cancel":
        return case.name in ("compressor", "compressor_look3", "expander", "stereo_widener", "chain_forward", "chain_forward_saving",
                             "chain_forward_expander", "chain_forward_saving_expander")
    return True


@pytest.mark.parametrize("case,kind", [(c, k) for c in CASES for k in idc.SILENCE_KINDS if _silence_applies(c, k)], ids=str)
def test_c_silence_against_the_references(D, monkeypatch, case, kind):
    configure(monkeypatch, case)
    B, C, N = 2, 2, 8200
    kw = dict(L=300, taps=63) if case.shapes else {}
    a, gy = arrays(case, 300, B, C, N, SR, kw)
    a = dict(a, x=idc.silence(kind, a["x"]))
    ref = case.ref(SR, a, gy.astype(np.float64), **kw)
    got = run(case, D, SR, a, gy, kw=kw)
    idc.check(case, got, ref, gy, kind, idc.tol_for(case, N), cancelling_columns=True)
    if case.cols == ("params",) and case.segment == "dyn":
        assert bool((got["g_params"][:, 3] == 0).all())                # release_ms has no path to the output
    if kind == "zeros" and (case.name.startswith("reverb") or case.segment in ("sos", "dyn", "chain") or case.name.startswith("lfilter")):
        assert bool((got["y"] == 0).all()), case.name                  # silence in, exact silence out
    if kind == "zero_tail" and case.name in ("parametric_eq", "sosfilt_s3", "lfilter_k2", "lfilter_k11"):
        # the decaying tail (recursion state running down through the float32 subnormals) against the float64 recursion, and the adjoint
        # with an upstream gradient that is nonzero only inside the silent stretch
        tail = np.abs(got["y"].cpu().numpy()[..., 1500:] - ref["y"][..., 1500:]).max()
        kind_, bound = idc.tol_for(case, N)["y"]
        assert tail <= bound * np.abs(ref["y"]).max()
        gz = gy.copy(); gz[..., :1500] = 0
        refz = case.ref(SR, a, gz.astype(np.float64), **kw)
        idc.check(case, run(case, D, SR, a, gz, kw=kw), refz, gz, "gy inside the silent stretch", idc.tol_for(case, N), cancelling_columns=True)


def test_c_compressor_silence_golden(D):
    """The reference's own run on a cancelling stereo pair and a zero tail (tests/golden/make_golden_input_domain.py): its conventions on
    silence - no gradient through the clamp below eps, sign(0) = 0 - at the bounds of test_compressor_golden (tests/test_gpu_dynamics.py:63-70)."""
    g = load_golden("comp_silence_b2c2_n6000")
    x = dev(g["x"]).requires_grad_(True)
    cols = [dev(g["params"][:, i]).requires_grad_(True) for i in range(6)]
    y = D.compressor(x, int(g["sample_rate"]), *cols)
    (y * dev(g["w"])).sum().backward()
    case = idc.BY_NAME["compressor"]
    got = dict(y=y.detach(), g_x=x.grad, g_params=torch.stack([c.grad for c in cols], 1))
    idc.check(case, got, dict(y=g["y64"], g_x=g["gx64"], g_params=g["gp64"]), g["w"], "silence golden", record_as="input_domain_compressor_silence_golden")
    assert bool((got["g_params"][:, 3] == 0).all()) and bool((got["y"][1, :, 1500:] == 0).all())
    from tests.util import linf_peak
    assert linf_peak(got["y"].cpu().numpy(), g["y32"]).max() < 1e-4


# ---- D: sample rates ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_d_biquad_design_matches_reference_at_every_rate(D, dtype):
    """signal.biquad on the reference's own coefficients at 16 .. 96 kHz, bounds of test_biquad_design_matches_reference
    (tests/test_gpu_sosfilt.py:492-496; the float64 goldens are stored as float64 here, so float64 is held to 1e-12)."""
    from tests.util import linf_peak
    g = load_golden("biquad_rates_b6")
    for sr in idc.RATES:
        for t in idc.BIQUAD_TYPES:
            ins = [dev(g[k]).to(dtype).requires_grad_(True) for k in ("gain_db", "cutoff_freq", "q_factor")]
            b, a = D.signal.biquad(*ins, sr, t)
            assert b.dtype == dtype and b.shape == (6, 3) and a.shape == (6, 3)
            ((b * dev(g["wb"]).to(dtype)).sum() + (a * dev(g["wa"]).to(dtype)).sum()).backward()
            tol = 2e-6 if dtype == torch.float32 else 1e-12
            rb, ra = g[f"sr{sr}_{t}_b64"], g[f"sr{sr}_{t}_a64"]
            assert np.abs(b.detach().cpu().numpy() - rb).max() < tol * np.abs(rb).max(), (sr, t)
            assert np.abs(a.detach().cpu().numpy() - ra).max() < tol * 2, (sr, t)
            gp = torch.cat([v.grad for v in ins], 1).cpu().numpy()
            assert linf_peak(gp, g[f"sr{sr}_{t}_g64"]).max() < 1e-5, (sr, t)


DYN_RATE_CASES = ["compressor", "compressor_look3", "expander", "chain_forward", "chain_forward_saving", "chain_forward_expander",
                  "chain_forward_saving_expander"]


def _dyn_rate_case(case, sr, B, C, N):
    rng = np.random.default_rng(sr + N)
    a, gy = idc.make(case, sr + N, B, C, N, sr)
    key, col = ("params", 2) if "params" in a else ("ctl", 2)
    a[key][:, col] = idc.dyn_rate_params(rng, B, sr)[:, 2]
    return a, gy


@pytest.mark.parametrize("sr", idc.RATES)
@pytest.mark.parametrize("name", DYN_RATE_CASES)
def test_d_dynamics_at_every_rate(D, monkeypatch, name, sr):
    """y, grad x and every control gradient against the exact recursion at that rate; attack 100 ms at 96 kHz (the a^1024 power chain) and
    5 ms at 16 kHz; the attack_ms gradient carries the explicit sample_rate / 1e3 factor (bound: the existing CTL_TOL). The saving
    forward's grad x has a test of its own below."""
    case = idc.BY_NAME[name]
    for B, C, N, kw, segmented, lookback in launch_shapes(case):
        if segmented and not lookback:
            continue
        configure(monkeypatch, case, segmented, lookback)
        a, gy = _dyn_rate_case(case, sr, B, C, N)
        ref = case.ref(sr, a, gy.astype(np.float64))
        if name == "chain_forward_saving":
            del ref["g_x"]
        got = run(case, D, sr, a, gy)
        idc.check(case, got, ref, gy, (sr, B, C, N, segmented), record_as=f"input_domain_rates[{name},{sr},{N}{',seg' if segmented else ''}]")


# grad x of the saving forward against the oracle at 2e-5 of peak |grad x| (tests/test_gpu_chain.py:213) is missed by one draw: 16 kHz,
# (2, 2, 1028), item 0 at 3.8e-5. Measured on that draw: the saving forward is 1.2e-7 from the unfused sequence (parametric_eq_norm, then
# dynamics_ctl: the same two backward kernels), which is 3.8e-5 from the oracle as well; each stage alone on the oracle's own input holds
# its bound (compressor grad x 7.1e-6, EQ adjoint 2.7e-6), and the compressor's grad x on the float32 EQ output - 2.2e-7 from the
# oracle's - is 4.2e-5 off: above the threshold (-43 dB, ratio 1.19, knee 0.55 dB) its side-chain term goes with 1 / s, and where the side
# chain passes |s| = 0.012 a 2e-7 change of the input is a 2e-5 change of that term. The composition's conditioning, the same for
# both paths, not what the saving forward saves; left as a strict xfail rather than given a bound of its own.
SAVING_GX_MISSES = {(16000, 1028)}


@pytest.mark.parametrize("sr,shape", [pytest.param(sr, shape, marks=[pytest.mark.xfail(strict=True, reason="grad x of EQ -> compressor, fused or not, is 3.8e-5 "
                                      "of its peak from the float64 oracle on this draw (the compressor's 1 / s side-chain term amplifies the EQ's float32 "
                                      "rounding); bound 2e-5 (tests/test_gpu_chain.py:213)")]
                                      if (sr, shape[2]) in SAVING_GX_MISSES else []) for sr in idc.RATES for shape in idc.PLAIN_SHAPES], ids=str)
def test_d_saving_forward_grad_x_at_every_rate(D, monkeypatch, sr, shape):
    """dasp_chain_forward_saving at every rate: (i) everything it hands on against the unfused sequence on the same inputs at the bounds
    of test_fused_training_forward_equals_the_two_launches (tests/test_gpu_chain.py:260: y 1e-5, grad x 2e-5, parameter gradients 1e-4,
    of the largest entry) - what the saving forward saves, isolated; (ii) the unfused sequence's grad x against the oracle, recorded;
    (iii) its own grad x against the oracle at 2e-5 of peak |grad x| per item."""
    case = idc.BY_NAME["chain_forward_saving"]
    B, C, N = shape
    configure(monkeypatch, case)
    a, gy = _dyn_rate_case(case, sr, B, C, N)
    ref = case.ref(sr, a, gy.astype(np.float64))
    got = run(case, D, sr, a, gy)
    unfused = copy.copy(case)
    unfused.call = idc.call_chain_unfused
    two = run(unfused, D, sr, a, gy)
    for k, bound in (("y", 1e-5), ("g_x", 2e-5), ("g_eq_pn", 1e-4), ("g_ctl", 1e-4)):
        e, m = float((got[k] - two[k]).abs().max()), float(two[k].abs().max())
        assert e <= bound * m, (sr, shape, k, e, m)
    peak_err = lambda t: (idc.errors("peak", t["g_x"].cpu().numpy(), ref["g_x"], 1.0, False))
    (ef, sf), (eu, su) = peak_err(got), peak_err(two)
    record(f"input_domain_saving_forward_grad_x[{sr},{N}]", fused_vs_oracle_of_peak=(ef / sf).max(), unfused_vs_oracle_of_peak=(eu / su).max(),
           fused_vs_unfused_of_max=float((got["g_x"] - two["g_x"]).abs().max() / two["g_x"].abs().max()))
    if (sr, N) in SAVING_GX_MISSES:
        assert (eu / su).max() > 2e-5, "the unfused sequence holds the bound on this draw: the miss is the saving forward's"
    idc.check(case, got, dict(g_x=ref["g_x"]), gy, (sr, shape))


@pytest.mark.parametrize("sr", [48000, 96000])
def test_d_chain_module_picks_the_saving_forward_at_other_rates(D, monkeypatch, sr):
    """chain.StyleTransferChain.process_normalized with config.plan.chain_fused_grad = True (the entry of tests/test_gpu_chain.py) at 48
    and 96 kHz, x and the upstream gradient as 4-byte aligned views: the Python dispatch hands the module's rate to eq_dyn_norm, and the
    chain gives what it gives with the two launches, at the bounds of test_fused_training_forward_equals_the_two_launches (:260)."""
    from dasp_pytorch_amd.chain import StyleTransferChain
    B, C, N = 3, 2, 8200
    rng = np.random.default_rng(sr)
    x, w = idc.noise_x(rng, (B, C, N)), rng.standard_normal((B, 2, N)).astype(np.float32)
    ps = [rng.random((B, k)).astype(np.float32) for k in (18, 6, 25, 1)]
    real = torch.ops.dasp.eq_dyn_norm
    rates = []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def __call__(self, *args, **kwargs):
            rates.append(args[2])
            return real(*args, **kwargs)
    monkeypatch.setattr(torch.ops.dasp, "eq_dyn_norm", Spy(), raising=False)

    def go(fused):
        monkeypatch.setattr(config.plan, "chain_fused_grad", fused)
        xt = misaligned(x).requires_grad_(True)
        pp = [dev(p).requires_grad_(True) for p in ps]
        y = StyleTransferChain(sr, num_samples=2048, num_bandpass_taps=127, noise_seed=5).process_normalized(xt, *pp)
        y.backward(misaligned(w))
        return [y.detach(), xt.grad] + [p.grad for p in pp]
    f = go(True)
    assert rates == [float(sr)]
    s = go(False)
    assert rates == [float(sr)]
    errs = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(f, s)]
    record(f"input_domain_chain_module_saving_forward[{sr}]", y=errs[0], gx=errs[1], gparams=errs[2:])
    assert errs[0] < 1e-5 and errs[1] < 2e-5 and max(errs[2:]) < 1e-4, errs
    assert all(bool(torch.isfinite(t).all()) for t in f)


@pytest.mark.parametrize("sr", [48000, 96000])
@pytest.mark.parametrize("name", ["compressor", "expander"])
def test_d_dynamics_float64_path_at_other_rates(D, name, sr):
    """csrc/ref64.hip at 48 and 96 kHz, bounds of tests/test_gpu_fp64.py:76-81 (y / grad x 5e-7, control gradients 2e-6 of the column)."""
    case = idc.BY_NAME[name]
    B, C, N = 3, 1, 8200
    a, gy = idc.make(case, sr + 1, B, C, N, sr)
    a["params"][:, 2] = idc.dyn_rate_params(np.random.default_rng(sr), B, sr)[:, 2]
    a = {k: v.astype(np.float64) for k, v in a.items()}
    ref = case.ref(sr, a, gy.astype(np.float64))
    got = run(case, D, sr, a, gy, dtype=torch.float64)
    assert got["y"].dtype == torch.float64
    tol = dict(y=("peak", 5e-7), g_x=("peak", 5e-7), g_params=("col", 2e-6) if name == "compressor" else case.tol["g_params"])
    idc.check(case, got, ref, gy, (sr, "float64"), tol, record_as=f"input_domain_rates_fp64[{name},{sr}]")


@pytest.mark.parametrize("sr", idc.RATES)
def test_d_parametric_eq_at_every_rate(D, monkeypatch, sr):
    """The module's Hz ranges capped at 0.45 x rate, items 0 / 1 at the 20 Hz / Q 6 / +-20 dB corner, N = 8200 and N = 40000 segmented,
    against scipy.signal.sosfilt in float64 on orc.peq_sos(..., sample_rate), at the existing bounds of test_parameter_range_corners /
    test_ragged_shapes (tests/test_gpu_sosfilt.py:121-123, 321). The reference's own float32 error at the corner (1e-4 .. 1e-2, erratic;
    tests/test_input_domain_cpu.py) is recorded beside the kernel's and NOT used as a bound."""
    case = idc.BY_NAME["parametric_eq"]
    for B, C, N, segmented in ((3, 1, 8200, False), (2, 2, 40000, True)):
        configure(monkeypatch, case, segmented)
        rng = np.random.default_rng(sr + N)
        a, gy = idc.make(case, sr + N, B, C, N, sr)
        a["params"] = idc.eq_rate_params(rng, B, sr)
        ref = case.ref(sr, a, gy.astype(np.float64))
        got = run(case, D, sr, a, gy)
        f32 = idc.eq_f32_error(a["x"], sr, a["params"])
        tag = f"input_domain_eq_rates[{sr},{N}{',seg' if segmented else ''}]"
        e = {k: idc.errors("peak", got[k].cpu().numpy(), ref[k], 1.0, k == "y") for k in ref}
        record(tag, **{k: (v[0] / v[1]).max() for k, v in e.items()}, reference_float32_y=f32.max())
        idc.check(case, got, ref, gy, tag)


@pytest.mark.parametrize("name", ["reverb_noise", "reverb_seed"])
def test_d_reverb_at_other_rates_and_the_per_rate_caches(D, name):
    """48, 88.2 and 96 kHz against the oracle with its filter bank at that rate; then 44.1 kHz with the same taps in the same process and 48 kHz
    again: each equal to its first result bit for bit (functional._device_filterbank is keyed by (taps, sample_rate, device), the spectra
    by the bank). One workgroup per window (band_split = 1), so that no float atomics stand between two runs."""
    case = idc.BY_NAME[name]
    B, C, N, L, taps = idc.REVERB_SHAPES[0]
    kw = dict(L=L, taps=taps)
    first = {}
    with reverb_plan(band_split=1):
        for sr in idc.REVERB_RATES + (SR, 48000):
            a, gy, ref = reference(case, 400, B, C, N, sr, kw)
            got = run(case, D, sr, a, gy, kw=kw)
            if sr in first:
                assert_same(case, got, first[sr], {}, (sr, "second call at this rate"))
                continue
            first[sr] = got
            idc.check(case, got, ref, gy, sr, record_as=f"input_domain_rates[{name},{sr}]")
        assert not torch.equal(first[48000]["y"], first[SR]["y"])


@pytest.mark.parametrize("sr", idc.REVERB_BAD_RATES)
def test_d_reverb_rates_without_a_filter_bank_raise(D, sr):
    """Below 36 kHz the filter bank's 18 kHz high-pass lies above Nyquist (and below about 22.7 kHz the 16 kHz octave band has
    f_min > f_max): the reference's firwin design raises, and so does this package, rather than producing something."""
    x = torch.rand(1, 2, 2000, device=DEV)
    cols = [torch.rand(1, device=DEV) for _ in range(25)]
    with pytest.raises(ValueError):
        D.noise_shaped_reverberation(x, sr, *cols, num_samples=300, num_bandpass_taps=63, noise=torch.randn(2, 12, 362, device=DEV))


@pytest.mark.parametrize("case", [c for c in CASES if c.rate_free and not c.name.startswith(("sosfilt", "lfilter"))], ids=str)   # (those take no rate at all)
def test_d_rate_free_ops_ignore_the_rate(D, monkeypatch, case):
    configure(monkeypatch, case)
    B, C, N, kw = idc.shapes_of(case)[0]
    a, gy, _ = reference(case, 100 + N, B, C, N, SR, kw)
    r1, r2 = run(case, D, SR, a, gy), run(case, D, 96000, a, gy)
    assert_same(case, r2, r1, {}, "44100 against 96000")
