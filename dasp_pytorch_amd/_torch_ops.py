"""torch.ops.dasp.*: the PyTorch-ROCm extension (csrc/torch_ext/dasp_torch_ops.cpp -> csrc/libdasp_torch.so) over the C ABI, as SURVEY 8(b) /
BASELINE north_star specify the boundary: ops with schemas registered through TORCH_LIBRARY, forward + hand-derived adjoint as
torch::autograd::Function in C++ - for the reference's own callables (parametric_eq on its 18 control tensors, dynamics on the six of
compressor / expander, gain, distortion, sosfilt, noise_shaped_reverb on its 25; round 5) and for the four ops of its effect chain on
normalised parameters (examples/style_transfer.py:150-154; round 4).

This module loads the library, registers the fake (meta) implementations that torch.compile / AOTAutograd / torch.library.opcheck need
(output shapes only; the work-buffer sizes come from the C ABI's own size queries), and answers `enabled()` for the call sites in
ops.py. The ctypes binding stays: it is the binding for every other op, for float64, for bench.py's per-call HIP events, and the
fallback when the extension is not built (config.plan.torch_ops = False forces it: A/B of the two bindings)."""
import os

import torch

from . import _lib, config

_HERE = os.path.dirname(os.path.abspath(__file__))
EXT_PATH = os.path.join(_HERE, "csrc", "libdasp_torch.so")
_state = {"loaded": None}


def _r64(n):
    return (int(n) + 63) & ~63


def _concrete(*vals):
    return all(isinstance(v, int) for v in vals)


def _n(fn, *args):
    """A buffer size from the library's size query - or, while tracing with symbolic shapes, a fresh unbacked size (the buffers are opaque
    work areas whose length no traced code looks at)."""
    if _concrete(*args):
        return int(fn(*args))
    return torch.library.get_ctx().new_dynamic_size()


def _register_fakes():
    L = _lib.lib()
    f32 = lambda t, *shape: t.new_empty(shape, dtype=torch.float32)

    like = lambda x: torch.empty_like(x, memory_format=torch.contiguous_format)

    def sos_work(x, Bp, S, tseg, save):
        """The two work buffers of a cascade call: [tab | carries] fp32, [dtab | segtab] fp64 (sizes from the C ABI's own queries)."""
        B, C, N = x.shape
        n32 = _n(lambda bp, b, c, n: _r64(bp * L.dasp_sos_table_floats(S)) + (_r64(L.dasp_sos_carry_floats(b * c, n, S)) if save else 0), Bp, B, C, N)
        n64 = _n(lambda bp: bp * L.dasp_sos_dtab_doubles(S) + (bp * L.dasp_sos_segtab_doubles(S) if tseg else 0), Bp)
        return f32(x, n32), x.new_empty((n64,), dtype=torch.float64)

    # ---- the reference's own callables
    @torch.library.register_fake("dasp::parametric_eq")
    def _(x, sample_rate, controls, types):
        return like(x)

    @torch.library.register_fake("dasp::_peq_forward")
    def _(x, controls, sample_rate, types, tseg, save):
        return (like(x),) + sos_work(x, controls[0].numel(), len(types), tseg, save)

    @torch.library.register_fake("dasp::_peq_backward")
    def _(x, grad_y, work32, work64, Bp, S, tseg, need_gx, need_gc):
        return (like(x) if need_gx else f32(x, 0)), (f32(x, 3 * S, Bp) if need_gc else f32(x, 0))

    @torch.library.register_fake("dasp::dynamics")
    def _(x, sample_rate, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db, eps, lookahead_samples, mode):
        return like(x)

    @torch.library.register_fake("dasp::gain")
    def _(x, gain_db):
        return like(x)

    @torch.library.register_fake("dasp::distortion")
    def _(x, drive_db):
        return like(x)

    @torch.library.register_fake("dasp::_ew_forward")
    def _(x, ctl, op):
        return like(x)

    @torch.library.register_fake("dasp::_ew_backward")
    def _(x, ctl, grad_y, op):
        return like(x), f32(x, ctl.numel())

    @torch.library.register_fake("dasp::sosfilt")
    def _(sos, x):
        return like(x)

    @torch.library.register_fake("dasp::_sosfilt_forward")
    def _(sos, x, tseg, save):
        return (like(x),) + sos_work(x, sos.shape[0], (sos.shape[1] + 1) // 2 * 2, tseg, save)

    @torch.library.register_fake("dasp::_sosfilt_backward")
    def _(x, grad_y, work32, work64, Bs, Sp, tseg, need_gx, need_gs):
        return (like(x) if need_gx else f32(x, 0)), (f32(x, Bs, Sp, 6) if need_gs else f32(x, 0))

    @torch.library.register_fake("dasp::noise_shaped_reverb")
    def _(x, band_gains, band_decays, mix, noise, fspec, num_samples, taps, seed, seed_offset, decay_bound):
        return f32(x, x.shape[0], 2, x.shape[2])

    # ---- the chain on normalised parameters
    @torch.library.register_fake("dasp::parametric_eq_norm")
    def _(x, param_tensor, sample_rate, types, lo, span, range_flag=None):
        return like(x)

    @torch.library.register_fake("dasp::_peq_norm_forward")
    def _(x, param_tensor, sample_rate, types, lo, span, tseg, save, range_flag=None):
        return (like(x),) + sos_work(x, param_tensor.shape[0], len(types), tseg, save)

    @torch.library.register_fake("dasp::_peq_norm_backward")
    def _(x, grad_y, work32, work64, Bp, S, tseg, need_gx, need_gp):
        gx = torch.empty_like(x, memory_format=torch.contiguous_format) if need_gx else f32(x, 0)
        return gx, (f32(x, Bp, 3 * S) if need_gp else f32(x, 0))

    @torch.library.register_fake("dasp::dynamics_ctl")
    def _(x, ctl, mode, sample_rate, eps, lookahead_samples):
        return torch.empty_like(x, memory_format=torch.contiguous_format)

    @torch.library.register_fake("dasp::eq_dyn_norm")
    def _(x, param_tensor, sample_rate, types, lo, span, ctl, mode, eps, range_flag=None):
        return like(x)

    @torch.library.register_fake("dasp::_eq_dyn_norm_forward")
    def _(x, param_tensor, sample_rate, types, lo, span, ctl, mode, eps, range_flag=None):
        B, C, N = x.shape
        ncar = _n(lambda b, n: L.dasp_dyn_carry_floats(b, n) if b * n else 0, B, N)
        return (like(x), like(x)) + sos_work(x, param_tensor.shape[0], len(types), 0, True) + (f32(x, ncar),)

    @torch.library.register_fake("dasp::_dynamics_forward")
    def _(x, ctl, mode, sample_rate, eps, lookahead_samples, tseg, save):
        B, C, N = x.shape
        ncar = _n(lambda b, n: L.dasp_dyn_carry_floats(b, n) if save and b * n else 0, B, N)
        return torch.empty_like(x, memory_format=torch.contiguous_format), f32(x, ncar), (f32(x, B, N) if lookahead_samples > 0 else f32(x, 0))

    @torch.library.register_fake("dasp::_dynamics_backward")
    def _(x, ctl, grad_y, carries, lin, mode, sample_rate, eps, lookahead_samples, tseg):
        return torch.empty_like(x, memory_format=torch.contiguous_format), f32(x, x.shape[0], 5)

    @torch.library.register_fake("dasp::_dynamics6_forward")
    def _(x, five, mode, sample_rate, eps, lookahead_samples, tseg, save):
        B, C, N = x.shape
        ncar = _n(lambda b, n: L.dasp_dyn_carry_floats(b, n) if save and b * n else 0, B, N)
        return torch.empty_like(x, memory_format=torch.contiguous_format), f32(x, ncar), (f32(x, B, N) if lookahead_samples > 0 else f32(x, 0))

    @torch.library.register_fake("dasp::_dynamics6_backward")
    def _(x, five, grad_y, carries, lin, mode, sample_rate, eps, lookahead_samples, tseg):
        return torch.empty_like(x, memory_format=torch.contiguous_format), f32(x, 6, x.shape[0])

    @torch.library.register_fake("dasp::chain_controls")
    def _(comp_params, reverb_params, gain_params, lo, span, range_flag=None):
        B = comp_params.shape[0]
        return f32(comp_params, B, 5), f32(comp_params, B, 12), f32(comp_params, B, 12), f32(comp_params, B)

    @torch.library.register_fake("dasp::_chain_controls_backward")
    def _(gctl, ggain, gdecay, gmix, span):
        B = gctl.shape[0]
        return f32(gctl, B, 6), f32(gctl, B, 25), f32(gctl, B, 1)

    def _rv_sizes(B, N, Lir, taps, nb):
        import ctypes
        sizes = (ctypes.c_long * 14)()
        _lib.check(L.dasp_reverb_sizes(B, N, Lir, taps, nb, sizes), "dasp_reverb_sizes")
        return sizes

    @torch.library.register_fake("dasp::reverb")
    def _(x, noise, fspec, gains, decays, mix, num_samples, taps, bands, seed, seed_offset, decay_bound):
        return f32(x, x.shape[0], 2, x.shape[2])

    @torch.library.register_fake("dasp::_reverb_forward")
    def _(x, noise, fspec, gains, decays, mix, num_samples, taps, bands, seed, seed_offset, decay_bound, save):
        B, _, N = x.shape
        if _concrete(B, N):
            s = _rv_sizes(B, N, num_samples, taps, bands) if B * N else [0] * 14
            nA, nH, nir = (2 * s[6] if save else 0), 2 * s[7], s[8]
        else:
            ctx = torch.library.get_ctx()
            nA, nH, nir = (ctx.new_dynamic_size() if save else 0), ctx.new_dynamic_size(), ctx.new_dynamic_size()
        return f32(x, B, 2, N), f32(x, nA), f32(x, nH), f32(x, nir)

    # ---- frequency responses (signal.fft_freqz / fft_sosfreqz)
    @torch.library.register_fake("dasp::freqz")
    def _(b, a, n_fft):
        return b.new_empty((b.shape[0], n_fft // 2 + 1), dtype=torch.complex128 if b.dtype == torch.float64 else torch.complex64)

    @torch.library.register_fake("dasp::_freqz_backward")
    def _(b, a, grad_H, n_fft):
        return like(b), like(a)

    # ---- filtering by a supplied frequency response (signal.freqdomain_fir)
    @torch.library.register_fake("dasp::freqdomain_fir")
    def _(x, H, n_fft):
        return x.new_empty((x.shape[0], n_fft))

    @torch.library.register_fake("dasp::_freqdomain_fir_backward")
    def _(x, H, grad_y, n_fft, need_gx, need_gH):
        return (like(x) if need_gx else f32(x, 0)), (like(H) if need_gH else H.new_empty((0,)))

    @torch.library.register_fake("dasp::_reverb_backward")
    def _(grad_y, ir, A, H, noise, fspec, gains, decays, mix, Cx, num_samples, taps, bands, seed, seed_offset, decay_bound):
        B, _, N = grad_y.shape
        return f32(grad_y, B, Cx, N), f32(grad_y, B, bands), f32(grad_y, B, bands), f32(grad_y, B)


def load():
    """Load csrc/libdasp_torch.so (once) and register the fake implementations. Returns True when torch.ops.dasp.* is usable."""
    if _state["loaded"] is None:
        ok = False
        if os.path.exists(EXT_PATH) and os.path.exists(_lib.LIB_PATH):
            try:
                L = _lib.lib()                           # libdasp_hip.so first (the extension links against it by soname)
                torch.ops.load_library(EXT_PATH)
                # both carry the hash of include/dasp_hip.h they were built against (csrc/build.py): a kernel-library-only rebuild after
                # an ABI change must not leave a stale extension calling entry points with yesterday's argument lists (round 4, advisor)
                have, want = int(torch.ops.dasp._abi_hash()), int(L.dasp_abi_hash())
                if have != want:
                    raise RuntimeError(f"built against another include/dasp_hip.h than libdasp_hip.so (hash {have:#x} vs {want:#x}): "
                                       "rebuild with python -m dasp_pytorch_amd.csrc.build")
                _register_fakes()
                ok = True
            except (OSError, RuntimeError) as e:         # a stale or foreign build: the ctypes binding still works
                import warnings
                warnings.warn(f"dasp_pytorch_amd: could not load {EXT_PATH} ({e}); using the ctypes binding")
        _state["loaded"] = ok
    return _state["loaded"]


def _plan_from_config():
    """The segment-plan overrides of the two scan families as the extension takes them: -1 = the library's planner, 0 = never segment,
    > 0 = tiles per segment (config.plan.sos_segment / sos_segment_tiles / dyn_segment / dyn_segment_tiles - the same switches the
    ctypes binding reads in ops.py; the compiled code reads no environment)."""
    def one(on, tiles):
        if not on:
            return 0
        return int(tiles) if tiles and int(tiles) > 0 else -1
    p = config.plan
    return one(p.sos_segment, p.sos_segment_tiles), one(p.dyn_segment, p.dyn_segment_tiles)


def sync_plan():
    """Push config.plan's overrides to the extension when they changed since the last push."""
    plan = _plan_from_config()
    if plan != _state.get("plan", (-1, -1)):
        torch.ops.dasp._plan_override(*plan)
        _state["plan"] = plan


def enabled():
    """True when the chain ops should go through torch.ops.dasp.* (the extension is built and loadable, config.plan.torch_ops is on, and
    bench.py's per-call HIP-event timers - which live in the ctypes binding - are off)."""
    on = config.plan.torch_ops and not _lib.timers.enabled and load()
    if on:
        sync_plan()
    return on
