"""torch.autograd.Function wrappers over the C ABI (include/dasp_hip.h) through ctypes.

The product's autograd binding is the PyTorch extension (csrc/torch_ext -> torch.ops.dasp.*; ops.py routes to it). This module is
 - the binding of what the extension does not register: biquad, the per-sample distortion, the stereo utilities, dynamics on a matrix
   of controls, and every float64 route (ops64.py);
 - the SECOND binding of what it does register (sosfilt, parametric_eq, gain, distortion, dynamics, the chain's normalised ops, the
   reverb): the GPU tests compare the two, bench.py's per-call HIP events go through it, config.plan.torch_ops = False selects it,
   and it owns the dtype / device / shape error messages of the calls the extension does not take.
PyTorch is used for device memory, streams and autograd plumbing only; every number is produced by the HIP kernels in csrc/. Nothing here
falls back to torch math on a missing library or a CPU tensor.

What every Function here owes autograd (tests/test_gpu_autograd_contract.py): backward returns None for an input that needs no gradient
and a tensor of the input's own dtype and shape otherwise; what it reads was written by its own forward and is left as it was, so a
graph can be differentiated again (retain_graph) and two graphs in any order; a caller's tensor the backward reads again - a contiguous
float32 x or control is kept as it is, not copied - goes through save_for_backward, so overwriting it between forward and backward raises
autograd's "modified by an inplace operation" error; everything else (tables, carries, copies) is the forward's own. Contiguous copies of
several upstream gradients are held in named variables until the call is queued: a temporary's block is handed to the next copy.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib, _resample_design, config
from ._lib import call, check, ptr, stream

FILTER_TYPES = {"peaking": 0, "low_shelf": 1, "high_shelf": 2, "low_pass": 3, "high_pass": 4}


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _needed(ctx, grads):
    """What a backward returns for an empty input: the gradients, None where the input needs none."""
    return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad))


def _pad_sections(S):
    """Smallest compiled section count >= S (kernels exist for 2/4/6/8 sections)."""
    for s in (2, 4, 6, 8):
        if S <= s:
            return s
    raise ValueError("more than 8 sections per call: chain calls (see signal.sosfilt_via_fsm)")


def _segment_tiles(rows, N, generic=False):
    """Tiles per segment for the segmented-row kernels, 0 = one workgroup per row (dasp_hip.h, "Few rows").
    A row is one workgroup, so few rows (the reference's training batches are 8-32 items: examples/style_transfer.py:403,
    auto_eq.py:231) leave most of the 256 CUs idle; the segmented path takes 2-4x less GPU time there (16 x 2 x 131072: forward
    0.078 -> 0.032 ms, backward 0.177 -> 0.047 ms) for four more kernel launches per call, all issued by the same C call. It is taken
    whenever the library's planner proposes a cut (at most 128 rows and at least 16 tiles per row; above that one workgroup per row runs at
    twice the waves per row up to 256 rows and is faster), eager or captured.
    config.plan.sos_segment = False: never; config.plan.sos_segment_tiles = <power of two> fixes the segment length."""
    if not config.plan.sos_segment:
        return 0
    if config.plan.sos_segment_tiles:
        return int(config.plan.sos_segment_tiles)
    # generic: a cascade given by its coefficients (no design launch per call: its segmented rows keep the pre-pass launches, five launches
    # per step) - there segments stop paying above 64 rows (profiles/r04/seg_crossover.log); the designed paths go up to the planner's 128
    return 0 if generic and rows > 64 else int(_lib.lib().dasp_sos_segment_tiles(rows, N))


def _round64(n):
    return (int(n) + 63) & ~63


class _SosWork:
    """Device work buffers of one filter application: one fp32 block (tables, saved chunk states, partial sums, segment scratch) and
    one fp64 block (design side table, segment transition matrices) - two allocations per call instead of one per buffer."""

    def __init__(self, Bs, S, x, need_grad, generic=False):
        L = _lib.lib()
        B, C, N = x.shape
        self.Bs, self.S = Bs, S
        self.tseg = _segment_tiles(B * C, N, generic)
        self.G = int(L.dasp_sos_segments(N, self.tseg))
        n_tab = _round64(Bs * L.dasp_sos_table_floats(S))
        n_car = _round64(L.dasp_sos_carry_floats(B * C, N, S)) if need_grad else 0
        n_par = _round64(L.dasp_sos_partial_floats(B * C * self.G, S)) if need_grad else 0
        n_seg = _round64(L.dasp_sos_seg_floats(B * C, N, S, self.tseg)) if self.tseg else 0
        f32 = torch.empty(n_tab + n_car + n_par + n_seg, dtype=torch.float32, device=x.device)
        self.tab, self.carries = f32[:n_tab], (f32[n_tab:n_tab + n_car] if need_grad else None)
        self.partials = f32[n_tab + n_car:n_tab + n_car + n_par] if need_grad else None
        self.segbuf = f32[n_tab + n_car + n_par:] if self.tseg else None
        n_dt = Bs * L.dasp_sos_dtab_doubles(S)
        f64 = torch.empty(n_dt + (Bs * L.dasp_sos_segtab_doubles(S) if self.tseg else 0), dtype=torch.float64, device=x.device)
        self.dtab, self.segtab = f64[:n_dt], (f64[n_dt:] if self.tseg else None)

    def forward(self, x):
        """Cascade from tables that are already filled (dasp_sos_prepare)."""
        B, C, N = x.shape
        y = torch.empty_like(x)
        if self.tseg:
            call("dasp_sos_segment_prepare", ptr(self.dtab), self.Bs, self.S, self.tseg, ptr(self.segtab), stream())
            call("dasp_sosfilt_forward_seg", ptr(self.tab), ptr(self.segtab), self.Bs, ptr(x), ptr(y), ptr(self.carries), ptr(self.segbuf),
                 B, C, N, self.S, self.tseg, stream())
        else:
            call("dasp_sosfilt_forward", ptr(self.tab), self.Bs, ptr(x), ptr(y), ptr(self.carries), B, C, N, self.S, stream())
        return y

    def backward(self, x, gy, mode, designed, need_gx, need_gc):
        """Adjoint cascade and coefficient / control gradients; (gx or None, gout or None)."""
        B, C, N = x.shape
        gx = torch.empty_like(x) if need_gx else None
        gout = None
        if need_gc:
            shape = (B, self.S, 6) if mode == 0 else (B, self.S, 3) if mode == 1 else (3 * self.S, B)
            gout = torch.empty(shape, dtype=torch.float32, device=x.device)
        part = self.partials if need_gc else None
        if _lib.timers.enabled and not self.tseg:      # bench.py's per-kernel HIP events: the two launches as separate entry points
            call("dasp_sosfilt_backward_ex", ptr(self.tab), self.Bs, ptr(x), ptr(gy), ptr(self.carries), ptr(gx), ptr(part), B, C, N, self.S, stream())
            if need_gc:
                call("dasp_sos_grad_finalize_ex", ptr(self.dtab), self.Bs, ptr(part), B, C, self.S, 1, mode, ptr(gout), stream())
        elif self.tseg and designed:
            # segmented rows of a designed cascade: pre-pass (+ chain), adjoint pass (+ finalize in its last workgroup per item) - two launches
            call("dasp_peq_backward", ptr(self.tab), ptr(self.dtab), self.Bs, ptr(x), ptr(gy), ptr(self.carries), ptr(gx), ptr(part), mode,
                 ptr(gout), B, C, N, self.S, self.tseg, ptr(self.segtab), ptr(self.segbuf), stream())
        elif self.tseg:
            call("dasp_sosfilt_backward_seg_ex", ptr(self.tab), ptr(self.segtab), self.Bs, ptr(x), ptr(gy), ptr(self.carries), ptr(gx),
                 ptr(part), ptr(self.segbuf), B, C, N, self.S, self.tseg, stream())
            if need_gc:
                call("dasp_sos_grad_finalize_ex", ptr(self.dtab), self.Bs, ptr(part), B, C, self.S, self.G, mode, ptr(gout), stream())
        else:
            call("dasp_sosfilt_backward_grads_ex", ptr(self.tab), ptr(self.dtab), self.Bs, ptr(x), ptr(gy), ptr(self.carries), ptr(gx),
                 ptr(part), mode, ptr(gout), B, C, N, self.S, stream())
        if need_gc and self.Bs == 1 and B != 1:
            gout = gout.sum(1 if mode == 2 else 0, keepdim=True)
        return gx, gout


class SosFiltFunction(torch.autograd.Function):
    """y = cascade of S biquads `sos` (Bs,S,6) applied to x (B,C,N); grads for x and sos."""

    @staticmethod
    def forward(ctx, sos, x):
        _lib.require_device(x, "x")
        _lib.require_device(sos, "sos")
        _lib.require_same_device(x, sos=sos)
        Bs, S, _ = sos.shape
        Sp = _pad_sections(S)
        ctx.dtypes = (sos.dtype, x.dtype)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            ctx.shapes = (sos.shape, x.shape)
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            sos32 = _f32c(sos)
            if Sp != S:  # identity sections [1 0 0 1 0 0]
                pad = torch.zeros(Bs, Sp - S, 6, dtype=torch.float32, device=sos.device)
                pad[..., 0] = 1.0
                pad[..., 3] = 1.0
                sos32 = torch.cat([sos32, pad], 1).contiguous()
            x32 = _f32c(x)
            need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
            w = _SosWork(Bs, Sp, x32, need, generic=True)
            call("dasp_sos_prepare", ptr(sos32), Bs, Sp, ptr(w.tab), ptr(w.dtab), stream())
            y = w.forward(x32)
            if need:
                ctx.work, ctx.S = w, S
                ctx.save_for_backward(x32)
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if ctx.empty:
            return _needed(ctx, (torch.zeros(ctx.shapes[0], dtype=ctx.dtypes[0], device=gy.device), torch.empty(ctx.shapes[1], dtype=ctx.dtypes[1], device=gy.device)))
        (x32,) = ctx.saved_tensors
        with torch.cuda.device(x32.device):
            gx, gsos = ctx.work.backward(x32, _f32c(gy), 0, 0, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        return (gsos[:, :ctx.S].to(ctx.dtypes[0]) if gsos is not None else None, gx.to(ctx.dtypes[1]) if gx is not None else None)


class BiquadFunction(torch.autograd.Function):
    """signal.biquad: (gain_db, cutoff_freq, q_factor) with n values each -> (n, 6) fp64 rows [b0 b1 b2 1 a1 a2] (dasp_biquad_design);
    the backward contracts the in-kernel Jacobian with the incoming gradient (dasp_biquad_backward)."""

    @staticmethod
    def forward(ctx, gain_db, cutoff_freq, q_factor, sample_rate, ftype):
        _lib.require_device(gain_db, "gain_db")
        _lib.require_same_device(gain_db, cutoff_freq=cutoff_freq, q_factor=q_factor)
        n = gain_db.numel()
        ctx.meta = [(t.dtype, t.shape) for t in (gain_db, cutoff_freq, q_factor)]
        dev = gain_db.device
        ba = torch.empty(n, 6, dtype=torch.float64, device=dev)
        jac = torch.empty(n, 15, dtype=torch.float64, device=dev)
        if n:
            with torch.cuda.device(dev):
                g, f, q = (t.detach().reshape(-1).to(torch.float64).contiguous() for t in (gain_db, cutoff_freq, q_factor))
                call("dasp_biquad_design", ptr(g), ptr(f), ptr(q), n, int(ftype), float(sample_rate), ptr(ba), ptr(jac), stream())
        ctx.save_for_backward(jac)        # also for n == 0: the backward pass then returns empty gradients of the recorded shapes
        return ba

    @staticmethod
    @once_differentiable
    def backward(ctx, gba):
        (jac,) = ctx.saved_tensors
        n = jac.shape[0]
        gp = torch.zeros(n, 3, dtype=torch.float64, device=gba.device)
        if n:
            with torch.cuda.device(jac.device):
                call("dasp_biquad_backward", ptr(jac), ptr(gba.to(torch.float64).contiguous()), n, ptr(gp), stream())
        cols = gp.unbind(1)
        return tuple(c.reshape(shape).to(dt) if need else None for c, (dt, shape), need in zip(cols, ctx.meta, ctx.needs_input_grad)) + (None, None)


class ParametricEQFunction(torch.autograd.Function):
    """Fused RBJ design (fp64, in-kernel) + cascade. `controls` are the 3*S per-item controls in the
    reference's argument order [gain_db, cutoff_freq, q_factor] per section, each with Bp elements.
    They enter as separate tensors and their gradients leave as contiguous rows of one (3S, Bp)
    buffer, so autograd neither builds a stack node nor launches 3S copy kernels. One C call per direction
    (dasp_peq_forward / dasp_peq_backward); the backward kernel is the variant torch.autograd's needs_input_grad asks for."""

    @staticmethod
    def forward(ctx, x, sample_rate, types, *controls):
        _lib.require_device(x, "x")
        L = _lib.lib()
        S = len(types)
        if not L.dasp_sos_supported_sections(S):
            raise ValueError(f"no kernel compiled for {S} sections")
        dev = x.device
        ctx.x_dtype = x.dtype
        ctx.ctl = [(c.dtype, c.shape) for c in controls]
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(dev):
            # the usual case - a 1-D contiguous fp32 tensor on x's device - is used as it is (grad mode is off in here): 18 controls
            # through four no-op tensor calls each were a fifth of the host time of a step
            cols = [c if (c.dtype is torch.float32 and c.dim() == 1 and c.device == dev and c.is_contiguous())
                    else c.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous() for c in controls]
            Bp = cols[0].numel()
            if any(c.numel() != Bp for c in cols):
                raise ValueError("parametric_eq controls must all have the same number of elements")
            x32 = _f32c(x)
            B, C, N = x32.shape
            need = any(ctx.needs_input_grad)
            w = _SosWork(Bp, S, x32, need)
            ctypes_types = (ctypes.c_int * S)(*types)
            rows = (ctypes.c_void_p * (3 * S))(*[c.data_ptr() for c in cols])        # read by the design kernel in place: no packing copy
            if _lib.timers.enabled and not w.tseg:   # bench.py's per-kernel HIP events: design and cascade as separate entry points
                call("dasp_peq_prepare_rows", rows, Bp, S, ctypes_types, float(sample_rate), ptr(w.tab), ptr(w.dtab), stream())
                y = w.forward(x32)
            else:
                y = torch.empty_like(x32)
                call("dasp_peq_forward", rows, Bp, S, ctypes_types, float(sample_rate), ptr(w.tab), ptr(w.dtab), ptr(x32), ptr(y),
                     ptr(w.carries), B, C, N, w.tseg, ptr(w.segtab), ptr(w.segbuf), stream())
            if need:
                ctx.work = w
                ctx.save_for_backward(x32)
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if ctx.empty:
            return _needed(ctx, ((torch.empty_like(gy), None, None) + tuple(torch.zeros(shape, dtype=dt, device=gy.device) for dt, shape in ctx.ctl)))
        (x32,) = ctx.saved_tensors
        need_gx, need_gc = ctx.needs_input_grad[0], any(ctx.needs_input_grad[3:])
        with torch.cuda.device(x32.device):
            gx, gpt = ctx.work.backward(x32, _f32c(gy), 2, 1, need_gx, need_gc)       # (3S, Bp): one contiguous gradient row per control tensor
        gcols = (None,) * len(ctx.ctl)
        if need_gc:
            rows = gpt.unbind(0)
            gcols = tuple((rows[i] if (dt is torch.float32 and shape == rows[i].shape) else rows[i].reshape(shape).to(dt)) if need else None
                          for i, ((dt, shape), need) in enumerate(zip(ctx.ctl, ctx.needs_input_grad[3:])))
        return (gx.to(ctx.x_dtype) if need_gx else None, None, None) + gcols


class ParametricEQNormFunction(torch.autograd.Function):
    """Processor.process_normalized for the EQ as one op (reference: dasp_pytorch/modules.py:25-91 + functional.py:118-272):
    the normalised (Bp, 3 S) tensor goes straight into the design kernel, which de-normalises it (lo + span * p in fp64), checks [0, 1] and
    builds the tables; the backward pass returns the gradient w.r.t. the normalised tensor. One tensor input instead of 3 S, no
    de-normalisation / slicing / stacking ops around the kernels. The [0, 1] check of the reference (modules.py:83) is the caller's
    (modules.check_unit_range, before anything is queued); the C entry point's own in-kernel flag word (dasp_hip.h) is not used from
    Python: reading it back would make the host wait for the forward kernel it has just queued."""

    @staticmethod
    def forward(ctx, x, pn, sample_rate, types, lo, span, range_flag=None):
        _lib.require_device(x, "x")
        _lib.require_same_device(x, param_tensor=pn)
        S = len(types)
        dev = x.device
        ctx.meta = (x.dtype, pn.dtype, pn.shape)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(dev):
            pn32 = _f32c(pn)
            Bp = pn32.shape[0]
            x32 = _f32c(x)
            B, C, N = x32.shape
            need = any(ctx.needs_input_grad)
            w = _SosWork(Bp, S, x32, need)
            y = torch.empty_like(x32)
            call("dasp_peq_forward_norm", ptr(pn32), Bp, S, (ctypes.c_int * S)(*types), float(sample_rate), (ctypes.c_double * (3 * S))(*lo),
                 (ctypes.c_double * (3 * S))(*span), ptr(range_flag), ptr(w.tab), ptr(w.dtab), ptr(x32), ptr(y), ptr(w.carries), B, C, N, w.tseg,
                 ptr(w.segtab), ptr(w.segbuf), stream())
            if need:
                ctx.work = w
                ctx.save_for_backward(x32)
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, pd, pshape = ctx.meta
        if ctx.empty:
            return _needed(ctx, (torch.empty_like(gy), torch.zeros(pshape, dtype=pd, device=gy.device), None, None, None, None, None))
        (x32,) = ctx.saved_tensors
        need_gx, need_gp = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        with torch.cuda.device(x32.device):
            gx, gp = ctx.work.backward(x32, _f32c(gy), 1, 1, need_gx, need_gp)       # mode 1: (Bp, S, 3) = the layout of the (Bp, 3 S) tensor
        return (gx.to(xd) if need_gx else None, gp.reshape(pshape).to(pd) if need_gp else None, None, None, None, None, None)


class _ElementwiseFunction(torch.autograd.Function):
    """Shared plumbing of gain / distortion: y = f(x, ctl), ctl one dB value per batch item (gain)
    or per (b, c) row (distortion)."""
    FWD = BWD = None

    @classmethod
    def _run(cls, ctx, x, ctl):
        _lib.require_device(x, "x")
        B, C, N = x.shape
        ctx.meta = (x.dtype, ctl.dtype, ctl.shape)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            c32 = ctl.detach().reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
            y = torch.empty_like(x32)
            call(cls.FWD, ptr(x32), ptr(c32), ptr(y), B, C, N, stream())
            ctx.save_for_backward(x32, c32)
        return y.to(x.dtype)

    @classmethod
    def _grad(cls, ctx, gy):
        xd, cd, cshape = ctx.meta
        if ctx.empty:
            return _needed(ctx, (torch.empty_like(gy), torch.zeros(cshape, dtype=cd, device=gy.device)))
        L = _lib.lib()
        x32, c32 = ctx.saved_tensors
        B, C, N = x32.shape
        with torch.cuda.device(x32.device):
            gx = torch.empty_like(x32)
            gctl = torch.empty_like(c32)
            partials = torch.empty(L.dasp_ew_partial_floats(B * C, N), dtype=torch.float32, device=x32.device)
            call(cls.BWD, ptr(x32), ptr(c32), ptr(_f32c(gy)), ptr(gx), ptr(gctl), ptr(partials), B, C, N, stream())
        return (gx.to(xd) if ctx.needs_input_grad[0] else None), (gctl.reshape(cshape).to(cd) if ctx.needs_input_grad[1] else None)


class GainFunction(_ElementwiseFunction):
    """y = x * 10^(gain_db/20); gain_db holds one value per batch item (functional.py:10-29)."""
    FWD, BWD = "dasp_gain_forward", "dasp_gain_backward"

    @staticmethod
    def forward(ctx, x, gain_db):
        return GainFunction._run(ctx, x, gain_db)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return GainFunction._grad(ctx, gy)


class DistortionFunction(_ElementwiseFunction):
    """y = tanh(x * 10^(drive_db/20)); drive_db holds one value per (b, c) row (functional.py:65-78)."""
    FWD, BWD = "dasp_distortion_forward", "dasp_distortion_backward"

    @staticmethod
    def forward(ctx, x, drive_db):
        return DistortionFunction._run(ctx, x, drive_db)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return DistortionFunction._grad(ctx, gy)


class DistortionSampleFunction(torch.autograd.Function):
    """y = tanh(x * 10^(drive_db/20)) with one drive value per sample: drive_db holds bs * chs * seq_len values (the other case the reference's
    drive_db.view(bs, chs, -1) accepts, functional.py:78)."""

    @staticmethod
    def forward(ctx, x, drive_db):
        _lib.require_device(x, "x")
        _lib.require_same_device(x, drive_db=drive_db)
        ctx.meta = (x.dtype, drive_db.dtype, drive_db.shape)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            d32 = _f32c(drive_db).reshape(x.shape)
            y = torch.empty_like(x32)
            call("dasp_distortion_sample_forward", ptr(x32), ptr(d32), ptr(y), x32.numel(), stream())
            ctx.save_for_backward(x32, d32)
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, dd, dshape = ctx.meta
        if ctx.empty:
            return _needed(ctx, (torch.empty_like(gy), torch.zeros(dshape, dtype=dd, device=gy.device)))
        x32, d32 = ctx.saved_tensors
        with torch.cuda.device(x32.device):
            gx = torch.empty_like(x32)
            gd = torch.empty_like(x32)
            call("dasp_distortion_sample_backward", ptr(x32), ptr(d32), ptr(_f32c(gy)), ptr(gx), ptr(gd), x32.numel(), stream())
        return (gx.to(xd) if ctx.needs_input_grad[0] else None), (gd.reshape(dshape).to(dd) if ctx.needs_input_grad[1] else None)


def _require_rows(x, t, ncols, name):
    """The dynamics kernels read `ncols` controls per batch item of x at t[b * ncols ...]: anything but a (bs, ncols) matrix would be read
    past its end. Same error as functional._dynamics (the reference's .view(-1, 1, 1) against a (bs, 1, seq_len) side chain does not
    broadcast a parameter batch of 1 either, functional.py:330-336)."""
    if t.dim() != 2 or t.shape[0] != x.shape[0] or t.shape[1] != ncols:
        raise RuntimeError(f"The size of tensor a ({t.shape[0] if t.dim() else 1}) must match the size of tensor b ({x.shape[0]}) at "
                           f"non-singleton dimension 0 ({name} must be ({x.shape[0]}, {ncols}), got {tuple(t.shape)})")


_DYN_COUNTERS = {}
_lib.on_failure.append(_DYN_COUNTERS.clear)          # a failed call may leave a count behind: the next call gets fresh zeros (advisor, r05)


def _dyn_counters(dev):
    """The completion counters of the segmented dynamics calls (4 ints per batch item, one buffer per (device, stream): 4 * 128 ints, and
    the segmented path is only taken up to 128 items - the size contract of dasp_hip.h: zero before the first use, every call returns
    the words it used to zero). Inside a HIP-graph capture a fresh zeroed buffer is used and not kept: it belongs to the graph's pool."""
    capturing = torch.cuda.is_current_stream_capturing()
    key = (dev.index, int(torch.cuda.current_stream(dev).cuda_stream))
    t = None if capturing else _DYN_COUNTERS.get(key)
    if t is None:
        t = torch.zeros(4 * 128, dtype=torch.int32, device=dev)          # (the segmented path is only taken below 128 items)
        if not capturing:
            if len(_DYN_COUNTERS) >= 16:
                _DYN_COUNTERS.clear()
            _DYN_COUNTERS[key] = t
    return t


def _dyn_forward(x, mode, sample_rate, eps, lookahead, ctl, need):
    """The compressor / expander kernels on ctl (B, 5) fp32 rows [threshold_db, ratio, attack_ms, knee_db, makeup_gain_db]; returns y (fp32)
    and what the backward pass needs."""
    L = _lib.lib()
    B, C, N = x.shape
    x32 = _f32c(x)
    y = torch.empty_like(x32)
    carries = torch.empty(L.dasp_dyn_carry_floats(B, N), dtype=torch.float32, device=x.device) if need else None
    lin = torch.empty(B, N, dtype=torch.float32, device=x.device) if lookahead > 0 else None
    # few items: every item is cut into segments that run as independent workgroups (dasp_hip.h, "Few batch items")
    tseg = 0 if not config.plan.dyn_segment else int(config.plan.dyn_segment_tiles or L.dasp_dyn_segment_tiles(B, N))
    segbuf = torch.empty(2 * B * L.dasp_dyn_segments(N, tseg), dtype=torch.float32, device=x.device) if tseg else None
    call("dasp_dynamics_forward", mode, ptr(x32), ptr(ctl), ptr(y), ptr(carries), ptr(lin), ptr(segbuf), B, C, N, float(sample_rate),
         float(eps), int(lookahead), tseg, ptr(_dyn_counters(x.device) if tseg and B <= 128 else None), stream())
    saved = (x32, ctl, carries, lin if lin is not None else torch.empty(0, device=x.device))
    return y, saved, (mode, float(sample_rate), float(eps), int(lookahead), tseg)


def _dyn_backward(saved, cfg, gy):
    """gx (fp32) and gctl (B, 5) for the rows of ctl."""
    L = _lib.lib()
    x32, ctl, carries, lin = saved
    mode, sr, eps, look, tseg = cfg
    B, C, N = x32.shape
    gx = torch.empty_like(x32)
    gctl = torch.empty(B, 5, dtype=torch.float32, device=x32.device)
    G = int(L.dasp_dyn_segments(N, tseg))
    partials = torch.empty(L.dasp_dyn_partial_floats(B * G), dtype=torch.float32, device=x32.device)
    segbuf = torch.empty(2 * B * G, dtype=torch.float32, device=x32.device) if tseg else None
    call("dasp_dynamics_backward", mode, ptr(x32), ptr(ctl), ptr(_f32c(gy)), ptr(carries), ptr(lin if look > 0 else None),
         ptr(gx), ptr(gctl), ptr(partials), ptr(segbuf), B, C, N, sr, eps, look, tseg, ptr(_dyn_counters(x32.device) if tseg and B <= 128 else None),
         stream())
    return gx, gctl


class DynamicsFunction(torch.autograd.Function):
    """Compressor (mode 0) / expander (mode 1). Controls enter as separate tensors with bs elements
    each, in the reference's order: threshold_db, ratio, attack_ms, release_ms, knee_db,
    makeup_gain_db (functional.py:275-286); release_ms is unused, as in the reference."""

    @staticmethod
    def forward(ctx, x, mode, sample_rate, eps, lookahead, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db):
        _lib.require_device(x, "x")
        ctx.meta = (x.dtype, [(c.dtype, c.shape) for c in (threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db)])
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            ctls = (threshold_db, ratio, attack_ms, knee_db, makeup_gain_db)
            ctl = torch.stack([c.detach().reshape(-1).to(device=x.device, dtype=torch.float32) for c in ctls], dim=1).contiguous()
            need = any(ctx.needs_input_grad)
            y, saved, cfg = _dyn_forward(x, mode, sample_rate, eps, lookahead, ctl, need)
            if need:
                ctx.save_for_backward(*saved)
                ctx.cfg = cfg
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, cm = ctx.meta
        if ctx.empty:
            return _needed(ctx, ((torch.empty_like(gy), None, None, None, None) + tuple(torch.zeros(shape, dtype=dt, device=gy.device) for dt, shape in cm)))
        x32 = ctx.saved_tensors[0]
        with torch.cuda.device(x32.device):
            gx, gctl = _dyn_backward(ctx.saved_tensors, ctx.cfg, gy)
        g = gctl.t().contiguous()      # rows: threshold, ratio, attack, knee, makeup
        rows = {0: g[0], 1: g[1], 2: g[2], 4: g[3], 5: g[4]}
        outs = []
        for i, ((dt, shape), need) in enumerate(zip(cm, ctx.needs_input_grad[5:])):
            if not need:
                outs.append(None)
            elif i == 3:               # release_ms: no path to the output (functional.py:340,343-344)
                outs.append(torch.zeros(shape, dtype=dt, device=x32.device))
            else:
                outs.append(rows[i].reshape(shape).to(dt))
        return (gx.to(xd) if ctx.needs_input_grad[0] else None, None, None, None, None) + tuple(outs)


class DynamicsMatrixFunction(torch.autograd.Function):
    """The same kernels on the six controls as one (bs, 6) matrix, columns in the reference's order (threshold_db, ratio, attack_ms,
    release_ms, knee_db, makeup_gain_db) - what Processor.process_normalized has after de-normalising (modules.py:159-187): one tensor in,
    one gradient matrix out (zero column for release_ms), no per-control slicing and stacking."""

    @staticmethod
    def forward(ctx, x, mode, sample_rate, eps, lookahead, controls):
        _lib.require_device(x, "x")
        _lib.require_same_device(x, controls=controls)
        _require_rows(x, controls, 6, "controls")
        ctx.meta = (x.dtype, controls.dtype, controls.shape)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            c32 = controls.detach().to(torch.float32)
            ctl = torch.cat([c32[:, :3], c32[:, 4:]], dim=1)         # (no index tensor: a list index is a host -> device copy per call)
            need = any(ctx.needs_input_grad)
            y, saved, cfg = _dyn_forward(x, mode, sample_rate, eps, lookahead, ctl, need)
            if need:
                ctx.save_for_backward(*saved)
                ctx.cfg = cfg
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, cd, cshape = ctx.meta
        if ctx.empty:
            return _needed(ctx, (torch.empty_like(gy), None, None, None, None, torch.zeros(cshape, dtype=cd, device=gy.device)))
        x32 = ctx.saved_tensors[0]
        with torch.cuda.device(x32.device):
            gx, gctl = _dyn_backward(ctx.saved_tensors, ctx.cfg, gy)
            g6 = None
            if ctx.needs_input_grad[5]:
                g6 = torch.cat([gctl[:, :3], torch.zeros_like(gctl[:, :1]), gctl[:, 3:]], dim=1).to(cd)      # release_ms: zero column
        return gx.to(xd) if ctx.needs_input_grad[0] else None, None, None, None, None, g6


class DynamicsCtlFunction(torch.autograd.Function):
    """The dynamics kernels on the (bs, 5) fp32 control rows they read, [threshold_db, ratio, attack_ms, knee_db, makeup_gain_db], with the
    gradient returned in the same layout (the chain's fused control op, ChainControlsFunction, produces and consumes it)."""

    @staticmethod
    def forward(ctx, x, mode, sample_rate, eps, lookahead, ctl):
        _lib.require_device(x, "x")
        _lib.require_same_device(x, ctl=ctl)
        _require_rows(x, ctl, 5, "ctl")
        ctx.xdtype, ctx.cdtype = x.dtype, ctl.dtype
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            need = any(ctx.needs_input_grad)
            y, saved, cfg = _dyn_forward(x, mode, sample_rate, eps, lookahead, _f32c(ctl), need)
            if need:
                ctx.save_for_backward(*saved)
                ctx.cfg = cfg
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if ctx.empty:
            return _needed(ctx, (torch.empty_like(gy), None, None, None, None, torch.zeros(gy.shape[0], 5, dtype=ctx.cdtype, device=gy.device)))
        with torch.cuda.device(gy.device):
            gx, gctl = _dyn_backward(ctx.saved_tensors, ctx.cfg, gy)
        return (gx.to(ctx.xdtype) if ctx.needs_input_grad[0] else None, None, None, None, None,
                gctl.to(ctx.cdtype) if ctx.needs_input_grad[5] else None)


class ChainControlsFunction(torch.autograd.Function):
    """De-normalisation of the compressor's (bs, 6), the reverb's (bs, 25) and the gain's (bs, 1) normalised parameters of the reference's
    effect chain in one launch (dasp_chain_controls), in the layouts the kernels read: ctl (bs, 5) with the chain's final gain folded into
    the make-up gain, band gains (bs, 12), band decays (bs, 12), mix (bs); backward: one launch back to the three parameter tensors.
    lo, span: ctypes float[32] (compressor 0-5, reverb 6-30, gain 31)."""

    @staticmethod
    def forward(ctx, comp_pn, reverb_pn, gain_pn, lo, span, range_flag=None):
        _lib.require_device(comp_pn, "comp_params")
        _lib.require_same_device(comp_pn, reverb_params=reverb_pn, gain_params=gain_pn)
        B = comp_pn.shape[0]
        dev = comp_pn.device
        ctx.span, ctx.B = span, B
        ctx.dtypes = (comp_pn.dtype, reverb_pn.dtype, gain_pn.dtype)
        with torch.cuda.device(dev):
            buf = torch.empty(B, 30, dtype=torch.float32, device=dev)          # one allocation: ctl | gains | decays | mix
            flat = buf.view(-1)
            ctl, gains, decays, mix = flat[:5 * B].view(B, 5), flat[5 * B:17 * B].view(B, 12), flat[17 * B:29 * B].view(B, 12), flat[29 * B:]
            if B:
                c32, r32, g32 = _f32c(comp_pn), _f32c(reverb_pn), _f32c(gain_pn)      # named: copies must outlive one another (see StereoMixFunction)
                call("dasp_chain_controls", ptr(c32), ptr(r32), ptr(g32), lo, span, ptr(ctl), ptr(gains),
                     ptr(decays), ptr(mix), ptr(range_flag), B, stream())
        return ctl, gains, decays, mix

    @staticmethod
    @once_differentiable
    def backward(ctx, gctl, ggain, gdecay, gmix):
        B = ctx.B
        dev = next(g for g in (gctl, ggain, gdecay, gmix) if g is not None).device
        with torch.cuda.device(dev):
            z = lambda g, *shape: _f32c(g) if g is not None else torch.zeros(*shape, dtype=torch.float32, device=dev)
            gc = torch.empty(B, 6, dtype=torch.float32, device=dev)
            gr = torch.empty(B, 25, dtype=torch.float32, device=dev)
            gg = torch.empty(B, 1, dtype=torch.float32, device=dev)
            if B:
                # the four copies stay referenced until the call is queued (see StereoMixFunction.backward): as temporaries, the copy of a
                # non-contiguous gctl was freed before ggain was copied - into the same block - and the kernel read ggain's values for both
                g0, g1, g2, g3 = z(gctl, B, 5), z(ggain, B, 12), z(gdecay, B, 12), z(gmix, B)
                call("dasp_chain_controls_backward", ptr(g0), ptr(g1), ptr(g2), ptr(g3), ctx.span, ptr(gc), ptr(gr), ptr(gg), B, stream())
        need = ctx.needs_input_grad
        return tuple(g.to(d) if n else None for g, d, n in zip((gc, gr, gg), ctx.dtypes, need)) + (None, None, None)


def chain_eq_compressor_forward(x, eq_pn, types, lo, span, sample_rate, ctl, mode=0, eps=1e-8, range_flag=None):
    """y = compressor(parametric_eq(x)) in one pass over x (dasp_chain_forward, csrc/chainfwd.hip): the EQ designed from its normalised
    (Bp, 18) parameter tensor (dasp_peq_prepare_norm: de-normalisation + RBJ design on the device), the compressor on its (B, 5) control rows
    [threshold_db, ratio, attack_ms, knee_db, makeup_gain_db]. Forward only - no autograd node, nothing saved: the reference's target
    synthesis (examples/style_transfer.py:293-299 runs the chain under no_grad every step). Refuses tensors that require a gradient."""
    _lib.require_device(x, "x")
    _lib.require_same_device(x, eq_params=eq_pn, ctl=ctl)
    from .ops64 import require_fp32_ok
    require_fp32_ok(x, "chain_eq_compressor_forward")       # fp32 kernel: float64 input is refused, not rounded behind the caller's back
    if torch.is_grad_enabled() and (x.requires_grad or eq_pn.requires_grad or ctl.requires_grad):
        raise RuntimeError("chain_eq_compressor_forward is forward-only: call it under torch.no_grad() or on detached tensors")
    _require_rows(x, ctl, 5, "ctl")
    L = _lib.lib()
    S = len(types)
    B, C, N = x.shape
    if eq_pn.dim() != 2 or eq_pn.shape[1] != 3 * S or eq_pn.shape[0] not in (1, B):
        raise RuntimeError(f"EQ parameters must be ({B} or 1, {3 * S}), got {tuple(eq_pn.shape)}")
    if x.numel() == 0:
        return torch.empty_like(x)
    dev = x.device
    with torch.cuda.device(dev):
        x32, pn32, c32 = _f32c(x), _f32c(eq_pn), _f32c(ctl)
        Bp = pn32.shape[0]
        tseg = 0 if not config.plan.chain_segment else int(config.plan.chain_segment_tiles or L.dasp_chain_segment_tiles(B, N))
        n_tab = _round64(Bp * L.dasp_sos_table_floats(S))
        n_seg = _round64(L.dasp_chain_seg_floats(B, C, N, S, tseg)) if tseg else 0
        f32 = torch.empty(n_tab + n_seg, dtype=torch.float32, device=dev)
        n_dt = Bp * L.dasp_sos_dtab_doubles(S)
        f64 = torch.empty(n_dt + (Bp * L.dasp_sos_segtab_doubles(S) if tseg else 0), dtype=torch.float64, device=dev)
        tab, segbuf = f32[:n_tab], (f32[n_tab:] if tseg else None)
        dtab, segtab = f64[:n_dt], (f64[n_dt:] if tseg else None)
        y = torch.empty_like(x32)
        call("dasp_peq_prepare_norm", ptr(pn32), Bp, S, (ctypes.c_int * S)(*types), float(sample_rate), (ctypes.c_double * (3 * S))(*lo),
             (ctypes.c_double * (3 * S))(*span), ptr(range_flag), ptr(tab), ptr(dtab), tseg, ptr(segtab), stream())      # design (+ segment matrices; range_flag: see parametric_eq_norm)
        call("dasp_chain_forward", ptr(tab), Bp, ptr(x32), ptr(c32), ptr(y), B, C, N, S, int(mode), float(sample_rate), float(eps), tseg,
             ptr(segtab), ptr(segbuf), stream())
    return y.to(x.dtype)


def _cbuf(n, device):
    """n complex64 elements as a float32 buffer (the C ABI takes void*)."""
    return torch.empty(2 * n, dtype=torch.float32, device=device)


class _StereoFunction(torch.autograd.Function):
    """Shared plumbing of stereo_widener / stereo_panner / stereo_bus: y = f(x, ctl) with a small per-item / per-track control."""
    OP = None       # 0 widener, 1 panner, 2 bus
    FWD = BWD = None

    @classmethod
    def _dims(cls, x):
        if cls.OP == 0:
            B, _, N = x.shape
            return B, 1, N, (B, 2, N)
        if cls.OP == 1:
            B, T, N = x.shape
            return B, T, N, (B, 2, T, N)
        B, _, T, N = x.shape
        return B, T, N, (B, 2, N)

    @classmethod
    def _run(cls, ctx, x, ctl):
        _lib.require_device(x, "x")
        B, T, N, oshape = cls._dims(x)
        ctx.meta = (x.dtype, ctl.dtype, ctl.shape, B, T, N)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            ctx.xshape = x.shape
            return torch.empty(oshape, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            c32 = ctl.detach().reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
            y = torch.empty(oshape, dtype=torch.float32, device=x.device)
            dims = (B, N) if cls.OP == 0 else (B, T, N)
            call(cls.FWD, ptr(x32), ptr(c32), ptr(y), *dims, stream())
            ctx.save_for_backward(x32, c32)
        return y.to(x.dtype)

    @classmethod
    def _grad(cls, ctx, gy):
        xd, cd, cshape, B, T, N = ctx.meta
        if ctx.empty:
            return _needed(ctx, (torch.empty(ctx.xshape, dtype=xd, device=gy.device), torch.zeros(cshape, dtype=cd, device=gy.device)))
        L = _lib.lib()
        x32, c32 = ctx.saved_tensors
        with torch.cuda.device(x32.device):
            gx = torch.empty_like(x32)
            gctl = torch.empty_like(c32)
            partials = torch.empty(L.dasp_stereo_partial_floats(cls.OP, B, T, N), dtype=torch.float32, device=x32.device)
            dims = (B, N) if cls.OP == 0 else (B, T, N)
            call(cls.BWD, ptr(x32), ptr(c32), ptr(_f32c(gy)), ptr(gx), ptr(gctl), ptr(partials), *dims, stream())
        return (gx.to(xd) if ctx.needs_input_grad[0] else None), (gctl.reshape(cshape).to(cd) if ctx.needs_input_grad[1] else None)


class WidenerFunction(_StereoFunction):
    """(L, R) -> (L + k R, k L + R), k = 1 - 2 width (functional.py:580-605)."""
    OP, FWD, BWD = 0, "dasp_widener_forward", "dasp_widener_backward"

    @staticmethod
    def forward(ctx, x, width):
        return WidenerFunction._run(ctx, x, width)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return WidenerFunction._grad(ctx, gy)


class PannerFunction(_StereoFunction):
    """(B, T, N) mono tracks -> (B, 2, T, N) with the pan law of functional.py:608-636."""
    OP, FWD, BWD = 1, "dasp_panner_forward", "dasp_panner_backward"

    @staticmethod
    def forward(ctx, x, pan):
        return PannerFunction._run(ctx, x, pan)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return PannerFunction._grad(ctx, gy)


class BusFunction(_StereoFunction):
    """(B, 2, T, N) -> (B, 2, N): sum of the tracks weighted by 10^(send_db / 20) (functional.py:32-62)."""
    OP, FWD, BWD = 2, "dasp_bus_forward", "dasp_bus_backward"

    @staticmethod
    def forward(ctx, x, send_db):
        return BusFunction._run(ctx, x, send_db)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return BusFunction._grad(ctx, gy)


class StereoMixFunction(torch.autograd.Function):
    """(B, T, N) mono tracks -> (mix, send), both (B, 2, N): fader, pan and bus sum in one pass (dasp_stereo_mix_forward / _backward,
    csrc/stereo.hip) - stereo_bus(stereo_panner(x, pan), gain_db) without the (B, 2, T, N) tensor in between; send (None without send_db)
    is the same sum with 10^(send_db / 20) more per track. Saves x and the three control vectors only."""

    @staticmethod
    def forward(ctx, x, gain_db, pan, send_db):
        _lib.require_device(x, "x")
        B, T, N = x.shape
        ctls = (gain_db, pan) if send_db is None else (gain_db, pan, send_db)
        ctx.meta = (x.dtype, [(c.dtype, c.shape) for c in ctls], B, T, N)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            mix = torch.empty((B, 2, N), dtype=x.dtype, device=x.device)
            return mix, (None if send_db is None else torch.empty_like(mix))
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            c32 = [c.detach().reshape(-1).to(device=x.device, dtype=torch.float32).contiguous() for c in ctls]
            mix = torch.empty((B, 2, N), dtype=torch.float32, device=x.device)
            send = None if send_db is None else torch.empty_like(mix)
            call("dasp_stereo_mix_forward", ptr(x32), ptr(c32[0]), ptr(c32[1]), ptr(c32[2] if send is not None else None), ptr(mix), ptr(send),
                 B, T, N, stream())
            ctx.save_for_backward(x32, *c32)
        return mix.to(x.dtype), (None if send is None else send.to(x.dtype))

    @staticmethod
    @once_differentiable
    def backward(ctx, gmix, gsend):
        xd, cmeta, B, T, N = ctx.meta
        dev = gmix.device
        with_send = len(cmeta) == 3
        if ctx.empty:
            gc = [torch.zeros(s, dtype=d, device=dev) for d, s in cmeta]
            return _needed(ctx, (torch.empty((B, T, N), dtype=xd, device=dev), gc[0], gc[1], (gc[2] if with_send else None)))
        x32, *c32 = ctx.saved_tensors
        with torch.cuda.device(dev):
            gx = torch.empty_like(x32) if ctx.needs_input_grad[0] else None           # not computed, not written when x needs no gradient
            gc = [torch.empty_like(c) for c in c32]
            partials = torch.empty(_lib.lib().dasp_stereo_mix_partial_floats(B, T, N, int(with_send)), dtype=torch.float32, device=dev)
            # both copies stay referenced until the call is queued: as temporaries, the copy of a non-contiguous gmix was freed before
            # gsend was copied - into the same block - and the kernel read gsend twice
            gm32, gs32 = _f32c(gmix), (_f32c(gsend) if with_send else None)
            call("dasp_stereo_mix_backward", ptr(x32), ptr(c32[0]), ptr(c32[1]), ptr(c32[2] if with_send else None), ptr(gm32),
                 ptr(gs32), ptr(gx), ptr(gc[0]), ptr(gc[1]), ptr(gc[2] if with_send else None), ptr(partials),
                 B, T, N, stream())
        gc = [g.reshape(s).to(d) if need else None for g, (d, s), need in zip(gc, cmeta, ctx.needs_input_grad[1:])] + [None]
        return (None if gx is None else gx.to(xd)), gc[0], gc[1], gc[2]


class _AudioControlsFunction(torch.autograd.Function):
    """Shared plumbing of the delay, filter and limiter ops: audio x (B, C, N), computed in float32, plus per-item controls that are
    leaves, plus plain-Python configuration. _run and _grad hold what is common - what a call records, the empty signal in both
    directions, the controls as the float32 matrix the kernels read, the optional grad x, the gradients back in every leaf's own shape
    and dtype - and a subclass holds what differs: its C calls, what it saves and the sizes of its state and scratch."""
    CFG = ()        # one converter per plain-Python argument, in the order of ctx.cfg

    @classmethod
    def _run(cls, ctx, x, ctls, *cfg):
        _lib.require_device(x, "x")
        B, C, N = x.shape                      # (three axes, or a ValueError before anything is recorded)
        ctx.meta = (x.dtype, [(c.dtype, c.shape) for c in ctls])
        ctx.cfg = tuple(conv(v) for conv, v in zip(cls.CFG, cfg))
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty_like(x)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            c32 = cls._controls(x, ctls)
            y = torch.empty_like(x32)
            kept = cls._forward(ctx, x32, c32, y)
            if kept is not None:               # None: no leaf needs a gradient, nothing is saved
                ctx.save_for_backward(x32, *c32, *kept)
        return y.to(x.dtype)

    @staticmethod
    def _f32(x, c, *shape):
        """One control on x's device, float32, viewed as `shape`."""
        return c.detach().reshape(*shape).to(device=x.device, dtype=torch.float32)

    @classmethod
    def _controls(cls, x, ctls, *per_item):
        """What the kernels read: k controls of bs (x per_item) values each as one (bs, [per_item,] k) float32 matrix."""
        return (torch.stack([cls._f32(x, c, x.shape[0], *per_item) for c in ctls], dim=-1).contiguous(),)

    @classmethod
    def _grad(cls, ctx, gy):
        (xd, cmeta), need = ctx.meta, ctx.needs_input_grad
        tail = (None,) * (len(need) - 1 - len(cmeta))                             # the configuration
        if ctx.empty:
            return _needed(ctx, (torch.empty_like(gy),) + tuple(torch.zeros(s, dtype=d, device=gy.device) for d, s in cmeta) + tail)
        x32, *saved = ctx.saved_tensors
        with torch.cuda.device(x32.device):
            gx = torch.empty_like(x32) if need[0] else None                       # None: the kernel writes no grad x; its scans still run
            cols = cls._backward(ctx, x32, saved, gy, gx)
        gc = tuple(g.reshape(s).to(d) if n else None for g, (d, s), n in zip(cols, cmeta, need[1:]))
        return (gx.to(xd) if need[0] else None,) + gc + tail

    # A subclass defines, beside forward / backward (autograd wants them on the class itself):
    #   _forward(ctx, x32, c32, y) -> what backward needs beyond x32 and c32, as a tuple; None: save nothing
    #   _backward(ctx, x32, saved, gy, gx) -> one float32 gradient per control (None where the leaf cannot need one); it makes the
    #   contiguous float32 copy of gy itself, after its own allocations


class OversampledDistortionFunction(_AudioControlsFunction):
    """y = decimate(tanh(g * interpolate(x))) at `oversample` times the sample rate, g = 10^(drive_db / 20) with one drive per (b, c) row
    (dasp_osdist_forward / _backward, csrc/oversample.hip). taps: the 2 * half_width * oversample + 1 float32 taps as a ctypes array
    (signal.oversampling_taps, rounded once). Saves x and drive_db only: the backward kernel recomputes the oversampled signal in LDS."""
    CFG = (lambda taps: taps, int, int)

    @staticmethod
    def forward(ctx, x, drive_db, taps, oversample, half_width):
        return OversampledDistortionFunction._run(ctx, x, (drive_db,), taps, oversample, half_width)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return OversampledDistortionFunction._grad(ctx, gy)

    @classmethod
    def _controls(cls, x, ctls):
        return (cls._f32(x, ctls[0], -1).contiguous(),)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        B, C, N = x32.shape
        taps, L, H = ctx.cfg
        call("dasp_osdist_forward", ptr(x32), ptr(c32[0]), taps, ptr(y), B, C, N, L, H, stream())
        return ()

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (d32,), (B, C, N), (taps, L, H) = saved, x32.shape, ctx.cfg
        gx = torch.empty_like(x32) if gx is None else gx                          # this kernel always writes it
        gd = torch.empty_like(d32)
        partials = torch.empty(_lib.lib().dasp_osdist_partial_floats(B * C, N, L), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_osdist_backward", ptr(x32), ptr(d32), taps, ptr(g32), ptr(gx), ptr(gd), ptr(partials), B, C, N, L, H, stream())
        return (gd,)


class ModulatedDelayFunction(_AudioControlsFunction):
    """y = (1 - mix) x + (mix / V) sum of V delay-line taps whose delays a sine LFO moves (dasp_moddelay_forward / _backward,
    csrc/moddelay.hip). delay_ms, depth_ms, rate_hz, phase: bs * V values each; mix: bs values; sample_rate, max_delay_ms, stereo_spread:
    floats; H = ceil(sample_rate / 1000 * max_delay_ms). Saves x, the controls packed as (bs, V, 4), and mix: the backward kernel
    recomputes the taps from x in LDS."""
    CFG = (float, float, float, int)

    @staticmethod
    def forward(ctx, x, delay_ms, depth_ms, rate_hz, phase, mix, sample_rate, max_delay_ms, stereo_spread, H):
        return ModulatedDelayFunction._run(ctx, x, (delay_ms, depth_ms, rate_hz, phase, mix), sample_rate, max_delay_ms, stereo_spread, H)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return ModulatedDelayFunction._grad(ctx, gy)

    @classmethod
    def _controls(cls, x, ctls):
        return super()._controls(x, ctls[:4], -1) + (cls._f32(x, ctls[4], -1).contiguous(),)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (ctl, m32), (B, C, N) = c32, x32.shape
        call("dasp_moddelay_forward", ptr(x32), ptr(ctl), ptr(m32), ptr(y), B, C, N, ctl.shape[1], ctx.cfg[3], *ctx.cfg[:3], stream())
        return ()

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):                                       # gx None: the scatter pass is skipped
        (ctl, m32), (B, C, N), (sample_rate, max_delay_ms, stereo_spread, H) = saved, x32.shape, ctx.cfg
        V = ctl.shape[1]
        gctl = torch.empty_like(ctl)
        gmix = torch.empty_like(m32)
        partials = torch.empty(_lib.lib().dasp_moddelay_partial_floats(B * C, N, V, H), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_moddelay_backward", ptr(x32), ptr(ctl), ptr(m32), ptr(g32), ptr(gx), ptr(gctl), ptr(gmix), ptr(partials), B, C, N, V, H,
             sample_rate, max_delay_ms, stereo_spread, stream())
        return gctl.unbind(-1) + (gmix,)


class FeedbackDelayFunction(_AudioControlsFunction):
    """y = (1 - mix) x + mix r, r the Catmull-Rom read of a delay line that is fed x + feedback r through a one-pole low-pass
    (dasp_fbdelay_forward / _backward, csrc/fbdelay.hip). delay_ms, feedback, damping_hz, mix: bs values each; sample_rate, max_delay_ms:
    floats; H = ceil(sample_rate / 1000 * max_delay_ms). Saves x, the controls packed as (bs, 4) and, when anything needs a gradient,
    the line's input v (bs, chs, seq_len): the backward kernel recomputes the taps from it."""
    CFG = (float, float, int)

    @staticmethod
    def forward(ctx, x, delay_ms, feedback, damping_hz, mix, sample_rate, max_delay_ms, H):
        return FeedbackDelayFunction._run(ctx, x, (delay_ms, feedback, damping_hz, mix), sample_rate, max_delay_ms, H)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return FeedbackDelayFunction._grad(ctx, gy)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (B, C, N), (sample_rate, max_delay_ms, H) = x32.shape, ctx.cfg
        v = torch.empty_like(x32) if any(ctx.needs_input_grad[:5]) else None      # 8 B per sample instead of 12 when nothing needs it
        call("dasp_fbdelay_forward", ptr(x32), ptr(c32[0]), ptr(y), ptr(v), B, C, N, H, sample_rate, max_delay_ms, stream())
        return None if v is None else (v,)

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (ctl, v), (B, C, N), (sample_rate, max_delay_ms, H) = saved, x32.shape, ctx.cfg
        gctl = torch.empty_like(ctl)
        partials = torch.empty(_lib.lib().dasp_fbdelay_partial_floats(B * C, N, H), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_fbdelay_backward", ptr(x32), ptr(ctl), ptr(v), ptr(g32), ptr(gx), ptr(gctl), ptr(partials), B, C, N, H, sample_rate,
             max_delay_ms, stream())
        return gctl.unbind(-1)


class FdnReverbFunction(_AudioControlsFunction):
    """y = (1 - mix) x + mix wet, wet the sum of K delay lines coupled through a Householder matrix and damped by one-pole low-passes
    (dasp_fdn_forward / _backward, csrc/fdn.hip). decay_s, damping_hz, mix: bs values each; sample_rate: a float; delays: a tuple of K
    ints; decorrelate: a bool. Saves x, the controls packed as (bs, 3) and, when a control needs a gradient, the K line signals v
    (bs, chs, K, seq_len): the backward kernel recomputes r, w and wet from them. With only x needing one no v is written: gx depends
    on the controls alone, and the backward call with v = NULL writes nothing else."""
    CFG = (float, lambda delays: tuple(int(m) for m in delays), bool)

    @staticmethod
    def forward(ctx, x, decay_s, damping_hz, mix, sample_rate, delays, decorrelate):
        return FdnReverbFunction._run(ctx, x, (decay_s, damping_hz, mix), sample_rate, delays, decorrelate)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return FdnReverbFunction._grad(ctx, gy)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (B, C, N), (sample_rate, delays, decorrelate) = x32.shape, ctx.cfg
        K = len(delays)
        ctx.saved_v = any(ctx.needs_input_grad[1:4])
        v = torch.empty((B, C, K, N), dtype=torch.float32, device=x32.device) if ctx.saved_v else None      # 4 K B per sample, only for the controls
        call("dasp_fdn_forward", ptr(x32), ptr(c32[0]), (ctypes.c_int * K)(*delays), ptr(y), ptr(v), B, C, N, K, sample_rate, int(decorrelate),
             stream())
        return (v,) if ctx.saved_v else () if ctx.needs_input_grad[0] else None

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (B, C, N), (sample_rate, delays, decorrelate) = x32.shape, ctx.cfg
        K = len(delays)
        ctl = saved[0]
        v = saved[1] if ctx.saved_v else None                                     # None: gx alone, one launch, no control sums
        gctl = torch.empty_like(ctl) if ctx.saved_v else None
        partials = torch.empty(_lib.lib().dasp_fdn_partial_floats(B * C), dtype=torch.float32, device=x32.device) if ctx.saved_v else None
        g32 = _f32c(gy)
        call("dasp_fdn_backward", ptr(x32), ptr(ctl), (ctypes.c_int * K)(*delays), ptr(v), ptr(g32), ptr(gx), ptr(gctl), ptr(partials), B, C, N, K,
             sample_rate, int(decorrelate), stream())
        return gctl.unbind(-1) if ctx.saved_v else (None,) * 3                    # (a control that needs a gradient implies saved_v)


class LimiterFunction(_AudioControlsFunction):
    """y = x G, G the gain of a look-ahead brickwall limiter with linked channels (dasp_limiter_forward / _backward, csrc/limiter.hip).
    threshold_db, release_ms: bs values each; sample_rate, eps: floats; lookahead: L in samples. Saves x, the controls packed as (bs, 2)
    and, when anything needs a gradient, G and the winning sample of every gain value, (bs, seq_len) each: 8 bytes per sample of an
    item. Nothing otherwise."""
    CFG = (float, int, float)

    @staticmethod
    def forward(ctx, x, threshold_db, release_ms, sample_rate, lookahead, eps):
        return LimiterFunction._run(ctx, x, (threshold_db, release_ms), sample_rate, lookahead, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return LimiterFunction._grad(ctx, gy)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (B, C, N), (sample_rate, lookahead, eps) = x32.shape, ctx.cfg
        gain = winner = None
        if any(ctx.needs_input_grad[:3]):
            gain = torch.empty((B, N), dtype=torch.float32, device=x32.device)
            winner = torch.empty((B, N), dtype=torch.int32, device=x32.device)
        call("dasp_limiter_forward", ptr(x32), ptr(c32[0]), ptr(y), ptr(gain), ptr(winner), B, C, N, lookahead, sample_rate, eps, stream())
        return None if gain is None else (gain, winner)

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (ctl, gain, winner), (B, C, N), (sample_rate, lookahead, eps) = saved, x32.shape, ctx.cfg
        gctl = torch.empty_like(ctl)
        scratch = torch.empty(_lib.lib().dasp_limiter_partial_floats(B, N), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_limiter_backward", ptr(x32), ptr(ctl), ptr(gain), ptr(winner), ptr(g32), ptr(gx), ptr(gctl), ptr(scratch), B, C, N, lookahead,
             sample_rate, eps, stream())
        return gctl.unbind(-1)


class PhaserFunction(_AudioControlsFunction):
    """y = (1 - mix) x + mix s_K, s_K the output of K first-order all-pass stages whose shared coefficient a sine LFO sweeps
    (dasp_phaser_forward / _backward, csrc/phaser.hip). rate_hz, center_hz, depth, phase, mix: bs values each; sample_rate, stereo_spread:
    floats; stages: K. Saves x, the controls packed as (bs, 5) and, when anything needs a gradient, the K stage states before every tile
    (dasp_phaser_state_floats): the backward kernel rebuilds the stage signals of a tile from them."""
    CFG = (float, int, float)

    @staticmethod
    def forward(ctx, x, rate_hz, center_hz, depth, phase, mix, sample_rate, stages, stereo_spread):
        return PhaserFunction._run(ctx, x, (rate_hz, center_hz, depth, phase, mix), sample_rate, stages, stereo_spread)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return PhaserFunction._grad(ctx, gy)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (B, C, N), (sample_rate, stages, stereo_spread) = x32.shape, ctx.cfg
        states = None
        if any(ctx.needs_input_grad[:6]):
            states = torch.empty(_lib.lib().dasp_phaser_state_floats(B * C, N, stages), dtype=torch.float32, device=x32.device)
        call("dasp_phaser_forward", ptr(x32), ptr(c32[0]), ptr(y), ptr(states), B, C, N, stages, sample_rate, stereo_spread, stream())
        return None if states is None else (states,)

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (ctl, states), (B, C, N), (sample_rate, stages, stereo_spread) = saved, x32.shape, ctx.cfg
        gctl = torch.empty_like(ctl)
        partials = torch.empty(_lib.lib().dasp_phaser_partial_floats(B * C), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_phaser_backward", ptr(x32), ptr(ctl), ptr(states), ptr(g32), ptr(gx), ptr(gctl), ptr(partials), B, C, N, stages, sample_rate,
             stereo_spread, stream())
        return gctl.unbind(-1)


TVFILTER_MODES = ("lowpass", "bandpass", "highpass", "notch")


class TimeVaryingFilterFunction(_AudioControlsFunction):
    """y = (1 - mix) x + mix w, w the output of a trapezoidal state-variable filter whose g and k follow the curves cutoff_hz and q
    (dasp_tvfilter_forward / _backward, csrc/tvfilter.hip). cutoff_hz, q: (bs, F), F = signal.control_frames(seq_len, hop); mix: bs values;
    sample_rate: a float; hop: an int; mode: an index into TVFILTER_MODES. Saves x, the curves, mix and, when anything needs a gradient,
    the two states before every tile (dasp_tvfilter_state_floats): the backward kernel rebuilds a tile from them."""
    CFG = (float, int, int)

    @staticmethod
    def forward(ctx, x, cutoff_hz, q, mix, sample_rate, hop, mode):
        return TimeVaryingFilterFunction._run(ctx, x, (cutoff_hz, q, mix), sample_rate, hop, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return TimeVaryingFilterFunction._grad(ctx, gy)

    @classmethod
    def _controls(cls, x, ctls):                                                  # the curves stay two (bs, F) matrices beside mix
        B = x.shape[0]
        return tuple(cls._f32(x, c, B, -1).contiguous() for c in ctls[:2]) + (cls._f32(x, ctls[2], B).contiguous(),)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (cut, qq, mx), (B, C, N), (sample_rate, hop, mode) = c32, x32.shape, ctx.cfg
        states = None
        if any(ctx.needs_input_grad[:4]):
            states = torch.empty(_lib.lib().dasp_tvfilter_state_floats(B * C, N), dtype=torch.float32, device=x32.device)
        call("dasp_tvfilter_forward", ptr(x32), ptr(cut), ptr(qq), ptr(mx), ptr(y), ptr(states), B, C, N, hop, mode, sample_rate, stream())
        return None if states is None else (states,)

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (cut, qq, mx, states), (B, C, N), (sample_rate, hop, mode) = saved, x32.shape, ctx.cfg
        gcut, gq, gmix = torch.empty_like(cut), torch.empty_like(qq), torch.empty_like(mx)
        scratch = torch.empty(_lib.lib().dasp_tvfilter_scratch_floats(B * C, N, hop), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_tvfilter_backward", ptr(x32), ptr(cut), ptr(qq), ptr(mx), ptr(states), ptr(g32), ptr(gx), ptr(gcut), ptr(gq), ptr(gmix), ptr(scratch),
             B, C, N, hop, mode, sample_rate, stream())
        return gcut, gq, gmix


TVEQ_MODES = ("bell", "lowshelf", "highshelf")


class TimeVaryingEQKernels:
    """The forward / backward pair of time_varying_eq as autograd calls it: a bell or shelf band of the trapezoidal state-variable filter
    whose gain, g and k follow the curves gain_db, cutoff_hz and q (dasp_tveq_forward / _backward, csrc/tveq.hip). The curves: (bs, F),
    F = signal.control_frames(seq_len, hop); sample_rate: a float; hop: an int; mode: an index into TVEQ_MODES. Saves x, the curves and,
    when anything needs a gradient, the two states before every tile (dasp_tveq_state_floats): the backward kernel rebuilds a tile from
    them."""

    @staticmethod
    def forward(ctx, x, gain_db, cutoff_hz, q, sample_rate, hop, mode):
        return TimeVaryingEQFunction._run(ctx, x, (gain_db, cutoff_hz, q), sample_rate, hop, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return TimeVaryingEQFunction._grad(ctx, gy)


class TimeVaryingEQFunction(TimeVaryingEQKernels, _AudioControlsFunction):
    """TimeVaryingEQKernels bound to autograd on the shared plumbing of _AudioControlsFunction, the curves kept as three (bs, F)
    matrices. The pair lives in the plain class, as for GainCurveFunction: the table of tests/autograd_contract_cases.py is closed, and
    this op's contract is checked by the same batteries from tests/test_gpu_time_varying_eq.py, which watches TimeVaryingEQKernels."""
    CFG = (float, int, int)

    @classmethod
    def _controls(cls, x, ctls):
        return tuple(cls._f32(x, c, x.shape[0], -1).contiguous() for c in ctls)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (gain, cut, qq), (B, C, N), (sample_rate, hop, mode) = c32, x32.shape, ctx.cfg
        states = None
        if any(ctx.needs_input_grad[:4]):
            states = torch.empty(_lib.lib().dasp_tveq_state_floats(B * C, N), dtype=torch.float32, device=x32.device)
        call("dasp_tveq_forward", ptr(x32), ptr(gain), ptr(cut), ptr(qq), ptr(y), ptr(states), B, C, N, hop, mode, sample_rate, stream())
        return None if states is None else (states,)

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (gain, cut, qq, states), (B, C, N), (sample_rate, hop, mode) = saved, x32.shape, ctx.cfg
        ggain, gcut, gq = torch.empty_like(gain), torch.empty_like(cut), torch.empty_like(qq)
        scratch = torch.empty(_lib.lib().dasp_tveq_scratch_floats(B * C, N, hop), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_tveq_backward", ptr(x32), ptr(gain), ptr(cut), ptr(qq), ptr(states), ptr(g32), ptr(gx), ptr(ggain), ptr(gcut), ptr(gq), ptr(scratch),
             B, C, N, hop, mode, sample_rate, stream())
        return ggain, gcut, gq


class GainCurveKernels:
    """The forward / backward pair of gain_curve as autograd calls it: y = x 10^(g / 20), g the curve gain_db (bs, F) interpolated in dB
    between frame points hop samples apart (dasp_gaincurve_forward / _backward, csrc/envelope.hip). sample_rate: a float the op does
    not use (the signature of `gain`); hop: an int. Saves x and the curve: the backward kernel recomputes the gain."""

    @staticmethod
    def forward(ctx, x, gain_db, sample_rate, hop):
        return GainCurveFunction._run(ctx, x, (gain_db,), sample_rate, hop)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return GainCurveFunction._grad(ctx, gy)


class GainCurveFunction(GainCurveKernels, _AudioControlsFunction):
    """GainCurveKernels bound to autograd on the shared plumbing of _AudioControlsFunction, the curve kept as a (bs, F) matrix like the
    curves of TimeVaryingFilterFunction. The pair lives in the plain class and this one defines no forward of its own: the table of
    tests/autograd_contract_cases.py is closed, and this op's contract is checked by the same batteries from
    tests/test_gpu_gain_curve.py, which watches GainCurveKernels."""
    CFG = (float, int)

    @classmethod
    def _controls(cls, x, ctls):
        return (cls._f32(x, ctls[0], x.shape[0], -1).contiguous(),)

    @staticmethod
    def _forward(ctx, x32, c32, y):
        (B, C, N), hop = x32.shape, ctx.cfg[1]
        call("dasp_gaincurve_forward", ptr(x32), ptr(c32[0]), ptr(y), B, C, N, hop, stream())
        return () if any(ctx.needs_input_grad[:2]) else None

    @staticmethod
    def _backward(ctx, x32, saved, gy, gx):
        (P,), (B, C, N), hop = saved, x32.shape, ctx.cfg[1]
        gP = scratch = None
        if ctx.needs_input_grad[1]:                                               # otherwise one launch: gx alone
            gP = torch.empty_like(P)
            scratch = torch.empty(_lib.lib().dasp_gaincurve_scratch_floats(B, N, hop), dtype=torch.float32, device=x32.device)
        g32 = _f32c(gy)
        call("dasp_gaincurve_backward", ptr(x32), ptr(P), ptr(g32), ptr(gx), ptr(gP), ptr(scratch), B, C, N, hop, stream())
        return (gP,)


ENVELOPE_DETECTORS = ("peak", "power")


class EnvelopeFollowerKernels:
    """The forward / backward pair of envelope_follower as autograd calls it: x (bs, chs, N) -> E (bs, F), the one-pole smoothed peak
    or power level at the frame points (dasp_envelope_forward / _backward, csrc/envelope.hip). smoothing_ms: bs values; sample_rate: a
    float; hop: an int; detector: an index into ENVELOPE_DETECTORS. Saves x, the control and, when the control needs a gradient, the
    tangent dE/da (bs, F): nothing per sample."""

    @staticmethod
    def forward(ctx, x, smoothing_ms, sample_rate, hop, detector):
        _lib.require_device(x, "x")
        B, C, N = x.shape
        hop = int(hop)
        F = -(-N // hop) + 1
        ctx.meta = (x.dtype, x.shape, smoothing_ms.dtype, smoothing_ms.shape)
        ctx.cfg = (float(sample_rate), hop, int(detector))
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.zeros((B, F), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            s32 = smoothing_ms.detach().reshape(B).to(device=x.device, dtype=torch.float32).contiguous()
            E = torch.empty((B, F), dtype=torch.float32, device=x.device)
            ctx.tangent = bool(ctx.needs_input_grad[1])
            D = torch.empty_like(E) if ctx.tangent else None
            scratch = torch.empty(_lib.lib().dasp_envelope_scratch_floats(B, N, hop), dtype=torch.float32, device=x.device)
            call("dasp_envelope_forward", ptr(x32), ptr(s32), ptr(E), ptr(D), ptr(scratch), B, C, N, hop, ctx.cfg[2], ctx.cfg[0], stream())
            if any(ctx.needs_input_grad[:2]):
                ctx.save_for_backward(x32, s32, *((D,) if ctx.tangent else ()))
        return E.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gE):
        xd, xs, sd, ss = ctx.meta
        need = ctx.needs_input_grad
        if ctx.empty:
            return _needed(ctx, (torch.zeros(xs, dtype=xd, device=gE.device), torch.zeros(ss, dtype=sd, device=gE.device), None, None, None))
        sample_rate, hop, detector = ctx.cfg
        x32, s32, *rest = ctx.saved_tensors
        B, C, N = x32.shape
        with torch.cuda.device(x32.device):
            gx = torch.empty_like(x32) if need[0] else None                       # None: the elementwise pass is skipped
            gs = torch.empty_like(s32) if ctx.tangent else None
            scratch = torch.empty(_lib.lib().dasp_envelope_scratch_floats(B, N, hop), dtype=torch.float32, device=x32.device) if need[0] else None
            g32 = _f32c(gE)
            call("dasp_envelope_backward", ptr(x32), ptr(s32), ptr(rest[0] if ctx.tangent else None), ptr(g32), ptr(gx), ptr(gs), ptr(scratch),
                 B, C, N, hop, detector, sample_rate, stream())
        return (gx.to(xd) if need[0] else None, gs.reshape(ss).to(sd) if need[1] else None, None, None, None)


class EnvelopeFollowerFunction(EnvelopeFollowerKernels, torch.autograd.Function):
    """EnvelopeFollowerKernels bound to autograd: a direct Function like ResampleFunction, because its output is not audio-shaped. The pair
    lives in the plain class and this one defines no forward of its own: the table of tests/autograd_contract_cases.py is closed, and
    this op's contract is checked by the same batteries from tests/test_gpu_envelope.py, which watches EnvelopeFollowerKernels."""


class BlockLevelKernels:
    """The forward / backward pair of block_level as autograd calls it: x (bs, chs, N) -> L (bs, F), the peak or the mean square of
    every hop (dasp_blocklevel_forward / _backward, csrc/ballistics.hip). hop: an int; detector: an index into ENVELOPE_DETECTORS.
    Peak saves the winners, one int32 per frame (position in the hop, sign and channel), and not x: its backward pass is write-only.
    Power saves x."""

    @staticmethod
    def forward(ctx, x, hop, detector):
        _lib.require_device(x, "x")
        B, C, N = x.shape
        hop, detector = int(hop), int(detector)
        F = -(-N // hop) + 1
        ctx.meta = (x.dtype, x.shape)
        ctx.cfg = (hop, detector)
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.zeros((B, F), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            L = torch.empty((B, F), dtype=torch.float32, device=x.device)
            need = ctx.needs_input_grad[0]
            win = torch.empty((B, F), dtype=torch.int32, device=x.device) if need and detector == 0 else None
            call("dasp_blocklevel_forward", ptr(x32), ptr(L), ptr(win), B, C, N, hop, detector, stream())
            if need:
                ctx.save_for_backward(win if detector == 0 else x32)
        return L.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gL):
        xd, xs = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None
        if ctx.empty:
            return torch.zeros(xs, dtype=xd, device=gL.device), None, None
        (hop, detector), (B, C, N) = ctx.cfg, xs
        (kept,) = ctx.saved_tensors
        with torch.cuda.device(kept.device):
            gx = torch.empty(xs, dtype=torch.float32, device=kept.device)
            g32 = _f32c(gL)
            call("dasp_blocklevel_backward", ptr(kept if detector else None), ptr(None if detector else kept), ptr(g32), ptr(gx), B, C, N, hop,
                 detector, stream())
        return gx.to(xd), None, None


class BlockLevelFunction(BlockLevelKernels, torch.autograd.Function):
    """BlockLevelKernels bound to autograd, a direct Function like EnvelopeFollowerFunction. The pair lives in the plain class and this
    one defines no forward of its own: the table of tests/autograd_contract_cases.py is closed, and this op's contract is checked by the
    same batteries from tests/test_gpu_block_level.py, which watches BlockLevelKernels."""


class BallisticsKernels:
    """The forward / backward pair of ballistics as autograd calls it: P (bs, F) -> E (bs, F), the branching attack / release smoother
    (dasp_ballistics_forward / _backward, csrc/ballistics.hip). attack_ms, release_ms: bs values each; sample_rate: a float; hop: an
    int. Saves P, both controls, E (float32) and the branch mask as the forward pass decided it (bs, F) uint8."""

    @staticmethod
    def forward(ctx, curve, attack_ms, release_ms, sample_rate, hop):
        _lib.require_device(curve, "curve")
        B, F = curve.shape
        ctx.meta = (curve.dtype, attack_ms.dtype, attack_ms.shape, release_ms.dtype, release_ms.shape)
        ctx.cfg = (float(sample_rate), int(hop))
        ctx.empty = curve.numel() == 0
        if ctx.empty:
            return torch.zeros((B, F), dtype=curve.dtype, device=curve.device)
        with torch.cuda.device(curve.device):
            p32 = _f32c(curve)
            a32, r32 = (c.detach().reshape(B).to(device=curve.device, dtype=torch.float32).contiguous() for c in (attack_ms, release_ms))
            E = torch.empty_like(p32)
            need = any(ctx.needs_input_grad[:3])
            up = torch.empty((B, F), dtype=torch.uint8, device=curve.device) if need else None
            call("dasp_ballistics_forward", ptr(p32), ptr(a32), ptr(r32), ptr(E), ptr(up), B, F, ctx.cfg[1], ctx.cfg[0], stream())
            if need:
                ctx.save_for_backward(p32, a32, r32, E, up)
        return E.to(curve.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gE):
        pd, ad, ash, rd, rsh = ctx.meta
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return None, None, None, None, None
        if ctx.empty:
            return _needed(ctx, (torch.zeros(gE.shape, dtype=pd, device=gE.device), torch.zeros(ash, dtype=ad, device=gE.device),
                                 torch.zeros(rsh, dtype=rd, device=gE.device), None, None))
        sample_rate, hop = ctx.cfg
        p32, a32, r32, E, up = ctx.saved_tensors
        B, F = p32.shape
        with torch.cuda.device(p32.device):
            gP = torch.empty_like(p32) if need[0] else None                       # None: not written
            ga = torch.empty_like(a32) if need[1] else None
            gr = torch.empty_like(r32) if need[2] else None
            g32 = _f32c(gE)
            call("dasp_ballistics_backward", ptr(p32), ptr(a32), ptr(r32), ptr(E), ptr(up), ptr(g32), ptr(gP), ptr(ga), ptr(gr), B, F, hop,
                 sample_rate, stream())
        return (gP.to(pd) if need[0] else None, ga.reshape(ash).to(ad) if need[1] else None, gr.reshape(rsh).to(rd) if need[2] else None, None, None)


class BallisticsFunction(BallisticsKernels, torch.autograd.Function):
    """BallisticsKernels bound to autograd; no forward of its own, as for BlockLevelFunction (tests/test_gpu_ballistics.py watches
    BallisticsKernels)."""


_RESAMPLE_DESIGNS, _RESAMPLE_TABLES = {}, {}


def resample_design(o, n, lowpass_filter_width, rolloff, resampling_method, beta):
    """The host side of a resampler for reduced rates o : n (_resample_design.Design: float64 design, float32 taps, the tables of both
    directions), kept per set of arguments. NotImplementedError, before anything is launched, for a design that csrc/resample.hip
    refuses in either direction: a table of more than dasp_resample_table_limit() taps or a span of taps that does not fit the
    staged window."""
    key = (int(o), int(n), int(lowpass_filter_width), float(rolloff), resampling_method, None if beta is None else float(beta))
    d = _RESAMPLE_DESIGNS.get(key)
    if d is None:
        d = _resample_design.Design(*key)
        d.key = key
        L = _lib.lib()
        d.tile = tuple(int(L.dasp_resample_tile(t.A, t.B, t.P, t.span)) for t in (d.fwd, d.bwd))
        if len(_RESAMPLE_DESIGNS) >= 64:
            _RESAMPLE_DESIGNS.clear()
        _RESAMPLE_DESIGNS[key] = d
    if min(d.tile) < 0:
        raise NotImplementedError(
            f"resample {o}:{n}: the compact tables hold {d.fwd.floats} (forward) and {d.bwd.floats} (backward) taps over spans of {d.fwd.span} and "
            f"{d.bwd.span} samples; at most {_lib.lib().dasp_resample_table_limit()} taps and {_lib.lib().dasp_resample_window_limit()} samples "
            "are implemented. Resample in two stages, or lower lowpass_filter_width")
    return d


def _resample_table(design, which, dev):
    """One direction's table on the device (dasp_resample_table_store), one per (design, direction, device). The first use outside a
    capture fills it and waits for the fill once, so that the table is complete for every stream from then on - captures included: a
    graph reads it like any other constant. A design first used INSIDE a HIP-graph capture gets a table of the graph's own, built fresh
    and not kept (the rule of _filter_spectrum: memory allocated while capturing belongs to that graph); the fill - kernels that carry
    the words in their arguments - is then kernel nodes of the graph, not a copy from host memory, and runs on every replay: use a
    design once before capturing it."""
    key = (design.key, which, dev.index)
    hit = _RESAMPLE_TABLES.get(key)
    if hit is not None:
        return hit
    capturing = torch.cuda.is_current_stream_capturing()
    words = getattr(design, which).words
    tab = torch.empty(len(words), dtype=torch.int32, device=dev)
    call("dasp_resample_table_store", ptr(tab), words.ctypes.data_as(ctypes.c_void_p), len(words), stream())
    if not capturing:
        torch.cuda.current_stream(dev).synchronize()
        _RESAMPLE_TABLES[key] = tab          # never dropped (at most 128 KiB each): a captured graph may hold its address
    return tab


def _resample_call(name, *args):
    try:
        call(name, *args)
    except _lib.DaspHipError as e:
        if "unsupported configuration" in str(e):
            raise NotImplementedError(str(e)) from None
        raise


class ResampleFunction(torch.autograd.Function):
    """x (rows, N) -> y (rows, ceil(n N / o)) by the polyphase filter of `design` (resample_design), and gy -> gx by its transpose,
    evaluated as a gather (dasp_resample_forward / _backward, csrc/resample.hip). The op is linear: nothing is saved for the backward
    pass. Not an _AudioControlsFunction: rows instead of (B, C, N), an output of another length, no controls and nothing saved leave
    _f32c as the only thing it would share."""

    @staticmethod
    def forward(ctx, x, design):
        _lib.require_device(x, "x")
        rows, N = x.shape
        M = design.out_len(N)
        ctx.meta = (x.dtype, rows, N, M)
        ctx.design = design
        ctx.empty = x.numel() == 0
        if ctx.empty:
            return torch.empty((rows, M), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            x32 = _f32c(x)
            t = design.fwd
            tab = _resample_table(design, "fwd", x.device)
            y = torch.empty((rows, M), dtype=torch.float32, device=x.device)
            _resample_call("dasp_resample_forward", ptr(x32), ptr(tab), ptr(y), rows, N, M, design.o, design.n, t.P, t.lo, t.span, stream())
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, rows, N, M = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None
        if ctx.empty:
            return torch.zeros((rows, N), dtype=xd, device=gy.device), None
        design = ctx.design
        with torch.cuda.device(gy.device):
            g32 = _f32c(gy)
            t = design.bwd
            tab = _resample_table(design, "bwd", gy.device)
            gx = torch.empty((rows, N), dtype=torch.float32, device=gy.device)
            _resample_call("dasp_resample_backward", ptr(g32), ptr(tab), ptr(gx), rows, N, M, design.o, design.n, t.P, t.lo, t.span, stream())
        return gx.to(xd), None


_FSPEC_CACHE = {}


def _filter_spectrum(filters, nb, taps, n_complex, dev):
    """Spectra of the filterbank taps (dasp_reverb_filter_spectrum). They depend only on the taps, so the result is kept
    for as long as the caller keeps passing the same (unmodified) filters tensor on the same stream -- functional.py
    holds one device copy of the bank per (taps, sample_rate, device)."""
    capturing = torch.cuda.is_current_stream_capturing()   # memory allocated inside a HIP-graph capture belongs to that graph
    key = (id(filters), filters._version, int(n_complex), int(torch.cuda.current_stream().cuda_stream))
    hit = None if capturing else _FSPEC_CACHE.get(key)
    if hit is not None and hit[0] is filters:
        return hit[1]
    Fspec = _cbuf(n_complex, dev)
    call("dasp_reverb_filter_spectrum", ptr(_f32c(filters)), nb, taps, ptr(Fspec), stream())
    if not capturing and filters.is_cuda and filters.dtype == torch.float32 and filters.is_contiguous() and not filters.requires_grad:
        if len(_FSPEC_CACHE) >= 8:
            _FSPEC_CACHE.clear()
        _FSPEC_CACHE[key] = (filters, Fspec)
    return Fspec


def _seed_offset(t, dev):
    """The optional per-replay seed offset: a 1-element int64 tensor on the op's device (read by the kernels when they run)."""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is torch.int64 and t.numel() == 1 and t.device == dev):
        raise ValueError("noise_seed_offset must be a 1-element int64 tensor on x's device")
    return t


def reverb_noise(seed, B, nb, row_len, device, seed_offset=None):
    """The white-noise stream the filter-bank kernels generate for `seed` (dasp_reverb_forward without a noise tensor), written out in the reference's layout
    (2B, nb, row_len) (dasp_pytorch/functional.py:548). A test / inspection hook: the product never materialises it."""
    dev = torch.device(device)
    out = torch.empty(2 * B, nb, row_len, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("dasp_reverb_noise", ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), ptr(_seed_offset(seed_offset, dev)), ptr(out), B, nb, row_len, stream())
    return out


class ReverbFunction(torch.autograd.Function):
    """noise_shaped_reverberation core: x (B,2,N) or mono (B,1,N) (the reference duplicates a mono input to stereo, functional.py:493-495; here
    both output channels read the one row - no copy; the backward adds the two channels' input gradients), output (B,2,N);
    noise (2B,nb,L+taps-1) or None, filters (nb,taps), gains/decays (B,nb), mix (B).
    `noise` and `filters` are constants of the op (the reference draws the noise inside the function, functional.py:548, and designs the
    filters with SciPy): asking for their gradient raises instead of silently returning None. noise = None: the noise is generated inside
    the filter-bank kernels from the integer `seed` (csrc/reverb.hip, counter-based: forward and backward recompute the same stream) and
    never exists in memory."""

    @staticmethod
    def forward(ctx, x, noise, filters, gains, decays, mix, L_ir, seed=None, seed_offset=None, decay_bound=0.0):
        _lib.require_device(x, "x")
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise RuntimeError("noise_shaped_reverberation: `noise` and `filters` are not differentiable inputs (detach them)")
        if noise is None and seed is None:
            raise ValueError("ReverbFunction: either a noise tensor or a seed")
        Lb = _lib.lib()
        B, C, N = x.shape
        nb, taps = filters.shape
        dev = x.device
        ctx.meta = (x.dtype, gains.dtype, gains.shape, decays.dtype, decays.shape, mix.dtype, mix.shape)
        ctx.empty = x.numel() == 0
        ctx.xC = C
        if C not in (1, 2):
            raise RuntimeError(f"noise_shaped_reverberation takes mono or stereo input, got {C} channels")
        if ctx.empty:
            return torch.empty(B, 2, N, dtype=x.dtype, device=dev)
        with torch.cuda.device(dev):
            sizes = (ctypes.c_long * 14)()
            check(Lb.dasp_reverb_sizes(B, N, L_ir, taps, nb, sizes), "dasp_reverb_sizes")
            if tuple(gains.shape) != (B, nb) or tuple(decays.shape) != (B, nb) or mix.numel() != B:
                # the kernels index gains[b * nb + band]: a (k, nb) stack with k != bs must not be reshaped into (bs, ...) silently
                # (the reference's torch.stack(...).view(bs, 12) raises for it, functional.py:498-544)
                raise RuntimeError(f"shape '[{B}, {nb}]' is invalid for band gains / decays of shapes {tuple(gains.shape)} / "
                                   f"{tuple(decays.shape)} and mix with {mix.numel()} values")
            x32 = _f32c(x)
            n32 = None
            if noise is not None:
                n32 = _f32c(noise)
                if n32.numel() != 2 * B * nb * (L_ir + taps - 1):
                    raise RuntimeError(f"noise must hold (2 * {B}, {nb}, {L_ir + taps - 1}) values, got {tuple(noise.shape)}")
            useed = ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF) if noise is None else None
            soff = _seed_offset(seed_offset, dev) if noise is None else None
            g32, d32, m32 = (_f32c(t.reshape(B, -1)) for t in (gains, decays, mix))
            Fspec = _filter_spectrum(filters, nb, taps, sizes[4], dev)
            y = torch.empty(B, 2, N, dtype=torch.float32, device=dev)
            need_grad = any(ctx.needs_input_grad)
            # kept for the backward pass: the column transforms of x (A), the impulse responses (ir) and their spectra (H: one complex frame
            # per item); everything else is scratch
            A = _cbuf(sizes[6], dev) if need_grad else None
            W2 = None if need_grad else _cbuf(sizes[12], dev)
            W, H, Ah = _cbuf(sizes[12], dev), _cbuf(sizes[7], dev), _cbuf(sizes[13], dev)
            ir = torch.empty(sizes[8], dtype=torch.float32, device=dev)
            # (noise given: n32, and seed 0 / no offset word, which the call ignores; seeded: a null noise pointer)
            call("dasp_reverb_forward", ptr(x32), ptr(n32), useed if useed is not None else 0, ptr(soff), ptr(Fspec), ptr(g32), ptr(d32), ptr(m32), ptr(y), ptr(A), ptr(H),
                 ptr(W), ptr(W2), ptr(Ah), ptr(ir), B, C, N, L_ir, taps, nb, float(decay_bound), stream())
            if need_grad:
                # the seed-offset word is read again by the backward kernels when they run: it is saved WITH the tensors, so that an in-place
                # bump between this forward and its backward (which would regenerate a different noise stream) trips autograd's
                # version check instead of giving silently wrong gain / decay / mix gradients (bump it after backward, or per replay)
                ctx.save_for_backward(ir, n32 if n32 is not None else x32.new_empty(0), Fspec, g32, d32, m32, A, H,
                                      soff if soff is not None else torch.empty(0, dtype=torch.int64, device=dev))
                ctx.cfg = (B, C, N, L_ir, taps, nb, [int(v) for v in sizes], useed, soff is not None, float(decay_bound))
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, gd, gs, dd, ds, md, ms = ctx.meta
        if ctx.empty:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=gy.device)
            return _needed(ctx, (torch.empty(gy.shape[0], ctx.xC, gy.shape[2], dtype=xd, device=gy.device), None, None, z(gs, gd), z(ds, dd), z(ms, md), None, None, None, None))
        ir, n32, Fspec, g32, d32, m32, A, H, soff = ctx.saved_tensors
        B, C, N, L_ir, taps, nb, sizes, useed, has_soff, dbound = ctx.cfg
        soff = soff if has_soff else None
        dev = ir.device
        with torch.cuda.device(dev):
            gx = torch.empty(B, 2, N, dtype=torch.float32, device=dev)
            ggain = torch.empty(B, nb, dtype=torch.float32, device=dev)
            gdecay = torch.empty(B, nb, dtype=torch.float32, device=dev)
            gmix = torch.empty(B, dtype=torch.float32, device=dev)
            Ag, W = _cbuf(sizes[12], dev), _cbuf(sizes[12], dev)
            P = _cbuf(sizes[13], dev)
            gir = torch.empty(sizes[8], dtype=torch.float32, device=dev)
            part = torch.empty(sizes[11], dtype=torch.float32, device=dev)
            mix_part = torch.empty(sizes[10], dtype=torch.float32, device=dev)
            call("dasp_reverb_backward", ptr(ir), ptr(_f32c(gy)), ptr(n32 if useed is None else None), useed if useed is not None else 0, ptr(soff), ptr(Fspec), ptr(g32),
                 ptr(d32), ptr(m32), ptr(A), ptr(H), ptr(gx), ptr(ggain), ptr(gdecay), ptr(gmix), ptr(Ag), ptr(W), ptr(P), ptr(gir), ptr(part),
                 ptr(mix_part), B, C, N, L_ir, taps, nb, dbound, stream())
        need = ctx.needs_input_grad
        if C == 1 and need[0]:
            gx = gx.sum(1, keepdim=True)           # the adjoint of the mono -> stereo duplication
        return (gx.to(xd) if need[0] else None, None, None, ggain.reshape(gs).to(gd) if need[3] else None, gdecay.reshape(ds).to(dd) if need[4] else None,
                gmix.reshape(ms).to(md) if need[5] else None, None, None, None, None)
