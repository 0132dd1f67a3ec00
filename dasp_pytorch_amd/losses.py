"""Multi-resolution STFT loss on the HIP kernels of csrc/stftloss.hip: the loss the reference's training loops put directly after
the effect chain (auraloss.freq.MultiResolutionSTFTLoss(), examples/style_transfer.py:341,363, auto_eq.py:252, virtual_analog.py:288).
Same defaults and call convention as auraloss 0.4.0: `loss_fn(input, target)` with (bs, chs, seq_len) tensors, per resolution
w_sc * spectral convergence + w_log_mag * log-magnitude L1 + w_lin_mag * linear-magnitude L1, mean over the resolutions; with
perceptual_weighting=True both signals first go through auraloss's 101-tap A-weighting FIR; with scale="mel", n_bins and sample_rate
the three terms are taken on mel-scaled magnitudes W |X| (librosa's Slaney filterbank, mel_filterbank below), which is also what
MelSTFTLoss computes. SumAndDifferenceSTFTLoss is that loss on the sum and on the difference of a stereo pair, from kernels whose workgroups own
both channels of an item. Both arguments receive gradients. The two losses are one forward and one backward body (_stft_forward,
_stft_backward) over the entry points dasp_mrstft_* and dasp_mrstft_sd_*, which take the term weights, n_bins (0: linear bins) with the
mel tables, and in the backward which argument to differentiate.

The time-domain half of auraloss (auraloss.time: ESRLoss, DCLoss, LogCoshLoss, SNRLoss, SISDRLoss, SDSDRLoss) and the MSE term of the
reference's examples/virtual_analog.py:299,324-326 are one weighted sum, time_domain_loss, from one moment pass over both signals
(csrc/tdloss.hip); FIRFilter is auraloss.perceptual.FIRFilter, the pre-emphasis / A-weighting filter those losses are used behind.

Autograd (tests/test_gpu_autograd_contract.py): a contiguous float32 input or target is saved as it is, so overwriting it between the
forward and a late backward raises autograd's in-place error (any other dtype or layout, and everything behind the A-weighting, is the
forward's own copy); the saved signals, statistics and per-stream device constants are only read by a backward, which may run any number
of times and in any order with other graphs'; a loss passed the same tensor twice returns the sum of both gradients."""
import ctypes
import functools
import math
import operator

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call, ptr, stream


AW_TAPS = 101
_AW_F = (20.598997, 107.65265, 737.86223, 12194.217)      # IEC 61672 A-weighting corner frequencies (Hz), as auraloss.perceptual
_AW_A1000 = 1.9997


@functools.lru_cache(maxsize=16)
def a_weighting_taps(sample_rate: float) -> np.ndarray:
    """The 101 float32 taps of auraloss.perceptual.FIRFilter(filter_type="aw", fs=sample_rate, ntaps=101): the analog A-weighting,
    its bilinear transform, that filter's magnitude on 512 frequencies, and the least-squares linear-phase FIR through them."""
    import scipy.signal
    f1, f2, f3, f4 = _AW_F
    num = [(2 * np.pi * f4) ** 2 * (10 ** (_AW_A1000 / 20)), 0, 0, 0, 0]
    den = np.polymul([1, 4 * np.pi * f4, (2 * np.pi * f4) ** 2], [1, 4 * np.pi * f1, (2 * np.pi * f1) ** 2])
    den = np.polymul(np.polymul(den, [1, 2 * np.pi * f3]), [1, 2 * np.pi * f2])
    b, a = scipy.signal.bilinear(num, den, fs=sample_rate)
    w, h = scipy.signal.freqz(b, a, worN=512, fs=sample_rate)
    taps = scipy.signal.firls(AW_TAPS, w, abs(h), fs=sample_rate).astype(np.float32)
    taps.flags.writeable = False
    return taps


MEL_MAX_BINS = 256
_MEL_F_SP = 200.0 / 3.0                    # Slaney's mel scale (librosa.filters.mel, htk=False): linear below 1 kHz, 27 log steps up to 6.4 kHz
_MEL_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f / _MEL_F_SP, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / _MEL_LOGSTEP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, _MEL_F_SP * m, 1000.0 * np.exp(_MEL_LOGSTEP * (np.maximum(m, 15.0) - 15.0)))


@functools.lru_cache(maxsize=32)
def mel_edges(sample_rate: float, n_mels: int) -> np.ndarray:
    """The n_mels + 2 edge frequencies (Hz, float64) of librosa.filters.mel(sr=sample_rate, n_mels=n_mels) with its defaults fmin=0,
    fmax=sr/2: equally spaced on the Slaney mel scale. The device table is built from these very numbers (dasp_mel_table_store)."""
    e = np.ascontiguousarray(mel_to_hz(np.linspace(float(hz_to_mel(0.0)), float(hz_to_mel(float(sample_rate) / 2.0)), int(n_mels) + 2)))
    e.flags.writeable = False
    return e


@functools.lru_cache(maxsize=32)
def mel_filterbank(sample_rate: float, n_fft: int, n_mels: int) -> np.ndarray:
    """librosa.filters.mel(sr=sample_rate, n_fft=n_fft, n_mels=n_mels) with librosa's defaults (fmin=0, fmax=sr/2, Slaney scale,
    norm="slaney"), which is what auraloss's scale="mel" multiplies the magnitudes by: (n_mels, n_fft // 2 + 1) float32, computed in
    float64 and rounded once. W[m, k] = max(0, min((f_k - e[m]) / (e[m+1] - e[m]), (e[m+2] - f_k) / (e[m+2] - e[m+1]))) * (2 / (e[m+2] - e[m])),
    f_k = k sample_rate / n_fft - the host-side statement of what the kernels' per-resolution table holds (csrc/stftloss.hip)."""
    e = mel_edges(sample_rate, n_mels)
    f = np.arange(int(n_fft) // 2 + 1, dtype=np.float64) * float(sample_rate) / float(n_fft)
    lo = (f[None, :] - e[:-2, None]) / (e[1:-1] - e[:-2])[:, None]
    hi = (e[2:, None] - f[None, :]) / (e[2:] - e[1:-1])[:, None]
    W = (np.maximum(0.0, np.minimum(lo, hi)) * (2.0 / (e[2:] - e[:-2]))[:, None]).astype(np.float32)
    W.flags.writeable = False
    return W


@functools.lru_cache(maxsize=64)
def _mel_empty_rows(sample_rate, n_fft, n_mels):
    return int((~mel_filterbank(sample_rate, n_fft, n_mels).any(axis=1)).sum())


_DEFAULTS = {"w_sc": 1.0, "w_log_mag": 1.0, "w_lin_mag": 0.0, "sample_rate": None, "perceptual_weighting": False, "w_phs": 0.0,
             "window": "hann_window", "scale": None, "n_bins": None, "scale_invariance": False, "reduction": "mean", "mag_distance": "L1",
             "output": "loss", "device": None}
_NOT_IMPLEMENTED = ("w_phs", "window", "scale", "n_bins", "scale_invariance", "reduction", "mag_distance", "output")


def _options(what, options):
    """auraloss 0.4.0's keyword options -> None (the default loss) or (w_sc, w_log_mag, w_lin_mag, sample_rate or None). `device` is
    ignored: the kernels follow the inputs."""
    for name in options:
        if name not in _DEFAULTS:
            raise TypeError(f"{what}() got an unexpected keyword argument {name!r}")
    o = dict(_DEFAULTS, **options)
    mel = o["scale"] == "mel" and o["n_bins"] is not None and o["sample_rate"] is not None          # carried separately: _mel_options
    for name in _NOT_IMPLEMENTED:
        if mel and name in ("scale", "n_bins"):
            continue
        v, d = o[name], _DEFAULTS[name]
        if (v is not None) if d is None else (v != d):
            raise NotImplementedError(f"{what}: {name}={v!r} is not implemented (only the default {name}={d!r})")
    if o["perceptual_weighting"] and o["sample_rate"] is None:
        raise ValueError("`sample_rate` must be supplied when `perceptual_weighting = True`.")
    w = (float(o["w_sc"]), float(o["w_log_mag"]), float(o["w_lin_mag"]))
    if not all(math.isfinite(v) for v in w):
        raise ValueError(f"{what}: the term weights must be finite, got w_sc, w_log_mag, w_lin_mag = {w}")
    if w == (1.0, 1.0, 0.0) and not o["perceptual_weighting"]:
        return None
    return w + (float(o["sample_rate"]) if o["perceptual_weighting"] else None,)


def _mel_options(what, options, fft_sizes):
    """None, or (n_bins, sample_rate) for scale="mel" with n_bins and sample_rate (anything less raises in _options, as every other
    unimplemented option does). The same n_bins for every resolution, as in auraloss; 1 <= n_bins <= 256 and n_bins <= n_fft / 2 + 1. A
    filter narrower than the bin spacing is an all-zero row of the filterbank: its log-magnitude term is log 0 - log 0, so that
    configuration is refused here unless w_log_mag = 0 (then the row adds 0 to the sums and still counts in the mean)."""
    if options.get("scale") != "mel" or options.get("n_bins") is None or options.get("sample_rate") is None:
        return None
    nb, sr = options["n_bins"], float(options["sample_rate"])
    try:
        nb = operator.index(nb)
    except TypeError:
        raise NotImplementedError(f"{what}: n_bins={options['n_bins']!r} is not implemented (an integer from 1 to {MEL_MAX_BINS})") from None
    if not (math.isfinite(sr) and sr > 0):
        raise ValueError(f"{what}: sample_rate must be positive, got {options['sample_rate']!r}")
    for n_fft in fft_sizes:
        if not 1 <= nb <= min(MEL_MAX_BINS, int(n_fft) // 2 + 1):
            raise NotImplementedError(f"{what}: n_bins={nb} is not implemented for n_fft={n_fft} (1 <= n_bins <= {MEL_MAX_BINS} and "
                                      "n_bins <= n_fft / 2 + 1)")
    if float(options.get("w_log_mag", _DEFAULTS["w_log_mag"])) != 0.0:
        for n_fft in fft_sizes:
            empty = _mel_empty_rows(sr, int(n_fft), nb)
            if empty:
                raise ValueError(f"{what}: at sample_rate={sr:g}, n_fft={n_fft}, {empty} of the {nb} mel filters are narrower than the bin spacing "
                                 "and empty, so the log-magnitude term is log 0 - log 0 (auraloss returns NaN there); use fewer bins, longer "
                                 "frames, or w_log_mag=0")
    return nb, sr


def _device_constant(cache, limit, key, device, build):
    """A device constant, one per (key, device, stream): build() allocates it and launches the kernel that writes it from its arguments.
    Inside a HIP-graph capture it is built fresh and not kept: memory allocated while capturing belongs to that graph's pool, and the
    fill kernel only runs on replay (the same rule as ops._filter_spectrum); filled from arguments, it is then a kernel node, not a copy
    from host memory. Keyed by stream as well: the fill is ordered only against work on the stream it was launched on. A full cache is
    cleared."""
    capturing = torch.cuda.is_current_stream_capturing()
    key = key + (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    if not capturing and key in cache:
        return cache[key]
    t = build()
    if not capturing:
        if len(cache) >= limit:
            cache.clear()
        cache[key] = t
    return t


_TW, _MEL_DEV, _FIR_DEV = {}, {}, {}


def _twiddles(device):
    """The 4096-entry twiddle table (dasp_mrstft_table)."""
    def build():
        tw = torch.empty(2 * 4096, dtype=torch.float32, device=device)
        call("dasp_mrstft_table", ptr(tw), stream())
        return tw
    return _device_constant(_TW, 16, (), device, build)


def _fir_taps(host, device):
    """Host float32 taps on the device (dasp_fir_taps_store)."""
    def build():
        taps = torch.empty(len(host), dtype=torch.float32, device=device)
        call("dasp_fir_taps_store", ptr(taps), host.ctypes.data_as(ctypes.c_void_p), len(host), stream())
        return taps
    return _device_constant(_FIR_DEV, 16, (host.tobytes(),), device, build)


def _mel_table(sample_rate, n_fft, n_bins, device):
    """One resolution's mel table (per bin: first filter and two weights; per filter: first bin and bin count), built on the device in
    fp64 from the edge frequencies (dasp_mel_table_store)."""
    def build():
        nfl = _lib.lib().dasp_mel_table_floats(int(n_fft), int(n_bins))
        if nfl < 0:
            raise _lib.DaspHipError(f"unsupported mel table: n_fft={n_fft}, n_bins={n_bins}")
        edges = mel_edges(float(sample_rate), int(n_bins))
        tab = torch.empty(nfl, dtype=torch.float32, device=device)
        call("dasp_mel_table_store", ptr(tab), edges.ctypes.data_as(ctypes.c_void_p), float(sample_rate), int(n_fft), int(n_bins), stream())
        return tab
    return _device_constant(_MEL_DEV, 64, (float(sample_rate), int(n_fft), int(n_bins)), device, build)


def _pair_rows(inp, target, what):
    """The entry checks of a loss on two signals (both on one GPU, a dtype the float32 kernels take, one shape), then both as
    contiguous float32 (rows, seq_len). The shape check is _MRSTFTFunction's: the other callers have compared the shapes before their
    device checks (_check_pair, _sum_diff) and cannot fail it."""
    _lib.require_device(inp, "input")
    _lib.require_device(target, "target")
    _lib.require_same_device(inp, target=target)
    from .ops64 import require_fp32_ok
    require_fp32_ok(inp, what)
    if inp.shape != target.shape:
        raise RuntimeError(f"input {tuple(inp.shape)} and target {tuple(target.shape)} must have the same shape")
    N = inp.shape[-1]
    return tuple(x.detach().reshape(-1, N).to(torch.float32).contiguous() for x in (inp, target))


def _fir_pair(name, a, b, taps):
    """dasp_fir_same_forward or dasp_fir_same_adjoint (name) in one launch on whichever of the (rows, N) tensors a, b exist -> (a, b)
    filtered, None where there was None."""
    live = [x for x in (a, b) if x is not None]
    if not live:
        return a, b
    outs = [torch.empty_like(x) for x in live]
    rows, N = live[0].shape
    call(name, ptr(live[0]), ptr(live[1] if len(live) > 1 else None), ptr(outs[0]), ptr(outs[1] if len(outs) > 1 else None), ptr(taps),
         taps.numel(), rows, N, stream())
    outs = iter(outs)
    return tuple(next(outs) if x is not None else None for x in (a, b))


def _as_arguments(g, gt, shape, dtype, tdtype):
    """A pair of float32 row tensors (outputs or gradients, None allowed) in the shape and the dtypes of the two arguments."""
    return (g.reshape(shape).to(dtype) if g is not None else None), (gt.reshape(shape).to(tdtype) if gt is not None else None)


# the two layouts of the STFT loss: (entry-point prefix, signal rows per unit the kernels own, shape of the loss, name in error messages);
# the library keeps 4 stats per resolution and loss
_MONO = ("dasp_mrstft_", 1, (), "MultiResolutionSTFTLoss")
_STEREO = ("dasp_mrstft_sd_", 2, (2,), "SumAndDifferenceSTFTLoss")


def _stft_forward(ctx, layout, inp, target, res, eps, opts, mel):
    """opts: None or (w_sc, w_log_mag, w_lin_mag, sample_rate or None), None meaning (1, 1, 0, None); with a sample rate the A-weighting
    FIR goes in front (per channel row: it is linear, the sum and difference are formed behind it) and the STFTs and the backward see
    the filtered pair. mel: None or (n_bins, sample_rate), the terms on mel-scaled magnitudes."""
    prefix, halves, loss_shape, what = layout
    p32, t32 = _pair_rows(inp, target, what)
    rows, N = p32.shape
    units, nres = rows // halves, len(res)
    arr = [(ctypes.c_int * nres)(*[int(r[i]) for r in res]) for i in range(3)]
    *wts, sr = opts if opts is not None else (1.0, 1.0, 0.0, None)
    nb = 0 if mel is None else int(mel[0])
    nfl = getattr(_lib.lib(), prefix + "partial_floats")(units, N, nres, *arr, nb)
    if nfl < 0:
        raise _lib.DaspHipError("unsupported STFT resolutions (fft a power of two in 8..8192, win <= fft, fft / 2 < seq_len, <= 8 of them"
                                + ("" if mel is None else f"; n_bins <= {MEL_MAX_BINS} and <= fft / 2 + 1") + ")")
    dev = inp.device
    with torch.cuda.device(dev):
        tw = _twiddles(dev)
        taps = None
        if sr is not None:
            taps = _fir_taps(a_weighting_taps(float(sr)), dev)
            p32, t32 = _fir_pair("dasp_fir_same_forward", p32, t32, taps)
        partials = torch.empty(nfl, dtype=torch.float32, device=dev)
        stats = torch.empty(4 * halves * nres, dtype=torch.float32, device=dev)
        loss = torch.empty(loss_shape, dtype=torch.float32, device=dev)
        tables, tabs = (), None
        if mel is not None:
            tables = tuple(_mel_table(mel[1], int(r[0]), nb, dev) for r in res)
            tabs = (ctypes.c_void_p * nres)(*[t.data_ptr() for t in tables])
        call(prefix + "forward", ptr(p32), ptr(t32), ptr(tw), tabs, ptr(partials), ptr(stats), ptr(loss), units, N, nres, *arr, float(eps), *wts,
             nb, stream())
    ctx.save_for_backward(p32, t32, stats, tw, taps, *tables)
    ctx.cfg = (prefix, units, N, nres, arr, float(eps), wts, nb, inp.shape, inp.dtype, target.dtype)
    return loss.to(inp.dtype)


def _stft_backward(ctx, gloss):
    """gloss: the upstream gradients as float32, one per loss. One call per requested gradient (auraloss differentiates both arguments: a
    consistency loss between two model outputs), then both through the A-weighting FIR's adjoint in one launch."""
    p32, t32, stats, tw, taps, *tables = ctx.saved_tensors
    prefix, units, N, nres, arr, eps, wts, nb, shape, dtype, tdtype = ctx.cfg
    tabs = (ctypes.c_void_p * nres)(*[t.data_ptr() for t in tables]) if tables else None
    grads = [None, None]
    with torch.cuda.device(p32.device):
        gloss = gloss.contiguous()
        for wrt_target in (0, 1):
            if ctx.needs_input_grad[wrt_target]:
                grads[wrt_target] = g = torch.empty_like(p32)
                call(prefix + "backward", ptr(p32), ptr(t32), ptr(tw), tabs, ptr(stats), ptr(gloss), ptr(g), units, N, nres, *arr, eps, *wts, nb,
                     wrt_target, stream())
        if taps is not None:
            grads = _fir_pair("dasp_fir_same_adjoint", *grads, taps)
    return _as_arguments(*grads, shape, dtype, tdtype)


class _MRSTFTFunction(torch.autograd.Function):
    """The loss of (..., N) signals (dasp_mrstft_*); opts and mel as _stft_forward's."""

    @staticmethod
    def forward(ctx, inp, target, res, eps, opts=None, mel=None):
        return _stft_forward(ctx, _MONO, inp, target, res, eps, opts, mel)

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss):
        return _stft_backward(ctx, gloss.detach().reshape(1).to(torch.float32)) + (None,) * 4


class _SumDiffFunction(torch.autograd.Function):
    """(sum_loss, diff_loss) of (bs, 2, N) signals from the item-owned kernels (dasp_mrstft_sd_*); opts and mel as _stft_forward's. The
    backward hands the kernels the two upstream gradients as a two-element gloss, so either output may be differentiated alone."""

    @staticmethod
    def forward(ctx, inp, target, res, eps, opts=None, mel=None):
        return tuple(_stft_forward(ctx, _STEREO, inp, target, res, eps, opts, mel))

    @staticmethod
    @once_differentiable
    def backward(ctx, gsum, gdiff):
        gloss = torch.stack((gsum.detach().reshape(()), gdiff.detach().reshape(()))).to(torch.float32)
        return _stft_backward(ctx, gloss) + (None,) * 4


class MultiResolutionSTFTLoss(torch.nn.Module):
    """auraloss.freq.MultiResolutionSTFTLoss (0.4.0). Positional arguments fft_sizes, hop_sizes, win_lengths, eps; keyword-only, with
    auraloss's defaults: w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, sample_rate=None, perceptual_weighting=False (True: the A-weighting
    FIR of auraloss.perceptual in front, needs sample_rate), device=None (ignored: the kernels follow the inputs), scale=None, n_bins=None
    (scale="mel" with an integer n_bins <= 256 and a sample_rate: the terms on mel-scaled magnitudes, librosa's Slaney filterbank with
    n_bins filters at every resolution; any other scale, "mel" without n_bins or sample_rate, or n_bins without a scale raises
    NotImplementedError). w_phs, window, scale_invariance, reduction, mag_distance and output are accepted at their defaults only (0.0,
    "hann_window", False, "mean", "L1", "loss"); any other value raises NotImplementedError. n_fft: powers of two 8 .. 8192, at most 8
    resolutions."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), eps: float = 1e-8, **options):
        super().__init__()
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")
        self._opts = _options(type(self).__name__, options)
        self._mel = _mel_options(type(self).__name__, options, fft_sizes)
        self.resolutions = tuple(zip(fft_sizes, hop_sizes, win_lengths))
        self.eps = eps

    def forward(self, input: torch.Tensor, target: torch.Tensor):
        if self._mel is None:
            return _MRSTFTFunction.apply(input, target, self.resolutions, self.eps, self._opts)
        return _MRSTFTFunction.apply(input, target, self.resolutions, self.eps, self._opts, self._mel)


class STFTLoss(MultiResolutionSTFTLoss):
    """auraloss.freq.STFTLoss with its default arguments (one resolution: fft 1024, hop 256, window 1024; w_sc = w_log_mag = 1, hann window,
    L1 magnitude distance, mean reduction) - the loss of the reference's examples/blind_estimation.py:141. One resolution of the same
    kernels (csrc/stftloss.hip); the keyword options of MultiResolutionSTFTLoss."""

    def __init__(self, fft_size: int = 1024, hop_size: int = 256, win_length: int = 1024, eps: float = 1e-8, **options):
        super().__init__((fft_size,), (hop_size,), (win_length,), eps, **options)


class MelSTFTLoss(STFTLoss):
    """auraloss.freq.MelSTFTLoss (0.4.0), its signature and defaults: STFTLoss(fft_size, hop_size, win_length, scale="mel", n_bins=n_mels,
    sample_rate=sample_rate, ...) - one resolution, the three terms on n_mels mel-scaled magnitudes. window and w_phs are accepted at
    their defaults only; further keywords are those of MultiResolutionSTFTLoss (and eps)."""

    def __init__(self, sample_rate, fft_size: int = 1024, hop_size: int = 256, win_length: int = 1024, window: str = "hann_window",
                 w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0, n_mels: int = 128, **kwargs):
        super().__init__(fft_size, hop_size, win_length, window=window, w_sc=w_sc, w_log_mag=w_log_mag, w_lin_mag=w_lin_mag, w_phs=w_phs,
                         sample_rate=sample_rate, scale="mel", n_bins=n_mels, **kwargs)


def mrstft_loss(input: torch.Tensor, target: torch.Tensor, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240),
                eps: float = 1e-8, **options):
    """MultiResolutionSTFTLoss(fft_sizes, hop_sizes, win_lengths, eps, **options)(input, target) as a function."""
    opts = _options("mrstft_loss", options)
    mel = _mel_options("mrstft_loss", options, fft_sizes)
    return _MRSTFTFunction.apply(input, target, tuple(zip(fft_sizes, hop_sizes, win_lengths)), eps, opts, mel)


def _sum_diff_options(what, window, output, options):
    """The loss's own keywords (window and output at the values it implements), then MultiResolutionSTFTLoss's validation of the rest."""
    if window != _DEFAULTS["window"]:
        raise NotImplementedError(f"{what}: window={window!r} is not implemented (only the default window={_DEFAULTS['window']!r})")
    if output not in ("loss", "full"):
        raise NotImplementedError(f"{what}: output={output!r} is not implemented (only output='loss' and output='full')")
    return _options(what, options)


def _sum_diff(input, target, res, eps, opts, mel, w_sum, w_diff, output):
    if input.dim() != 3 or input.shape[1] != 2:
        chs = input.shape[1] if input.dim() == 3 else f"shape {tuple(input.shape)}: not (bs, 2, seq_len);"
        raise ValueError(f"Input must be stereo: {chs} channel(s).")
    if input.shape != target.shape:
        raise RuntimeError(f"input {tuple(input.shape)} and target {tuple(target.shape)} must have the same shape")
    sum_loss, diff_loss = _SumDiffFunction.apply(input, target, res, eps, opts, mel)
    loss = (w_sum * sum_loss + w_diff * diff_loss) / 2
    return loss if output == "loss" else (loss, sum_loss, diff_loss)


class SumAndDifferenceSTFTLoss(torch.nn.Module):
    """auraloss.freq.SumAndDifferenceSTFTLoss (0.4.0): for (bs, 2, seq_len) signals, MultiResolutionSTFTLoss(fft_sizes, hop_sizes,
    win_lengths, **kwargs) on L + R and on L - R as two separate losses, loss = (w_sum * sum_loss + w_diff * diff_loss) / 2;
    output="full" returns (loss, sum_loss, diff_loss), each differentiable. fft_sizes, hop_sizes and win_lengths have no defaults, as in
    auraloss. kwargs: the keyword options of MultiResolutionSTFTLoss (w_sc, w_log_mag, w_lin_mag, perceptual_weighting + sample_rate,
    scale="mel" + n_bins, eps, device), refused where it refuses them; window at its default only. One workgroup owns a frame group of
    both channels of an item (csrc/stftloss.hip: dasp_mrstft_sd_*): no L + R / L - R signals exist in memory, and the backward returns to channels in
    the frequency domain, through one inverse transform. A channel count other than 2 raises ValueError."""

    def __init__(self, fft_sizes, hop_sizes, win_lengths, window: str = "hann_window", w_sum: float = 1.0, w_diff: float = 1.0,
                 output: str = "loss", **kwargs):
        super().__init__()
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")
        kwargs = dict(kwargs)
        self.eps = kwargs.pop("eps", 1e-8)
        self._opts = _sum_diff_options(type(self).__name__, window, output, kwargs)
        self._mel = _mel_options(type(self).__name__, kwargs, fft_sizes)
        self.resolutions = tuple(zip(fft_sizes, hop_sizes, win_lengths))
        self.w_sum, self.w_diff, self.output = float(w_sum), float(w_diff), output

    def forward(self, input: torch.Tensor, target: torch.Tensor):
        return _sum_diff(input, target, self.resolutions, self.eps, self._opts, self._mel, self.w_sum, self.w_diff, self.output)


def sum_and_difference_stft_loss(input: torch.Tensor, target: torch.Tensor, fft_sizes, hop_sizes, win_lengths, eps: float = 1e-8,
                                 w_sum: float = 1.0, w_diff: float = 1.0, output: str = "loss", **options):
    """SumAndDifferenceSTFTLoss(fft_sizes, hop_sizes, win_lengths, w_sum=w_sum, w_diff=w_diff, output=output, eps=eps, **options)(input,
    target) as a function."""
    if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
        raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")
    options = dict(options)
    window = options.pop("window", _DEFAULTS["window"])
    opts = _sum_diff_options("sum_and_difference_stft_loss", window, output, options)
    mel = _mel_options("sum_and_difference_stft_loss", options, fft_sizes)
    return _sum_diff(input, target, tuple(zip(fft_sizes, hop_sizes, win_lengths)), eps, opts, mel, float(w_sum), float(w_diff), output)


# ---- auraloss.time on the fused moment kernels (csrc/tdloss.hip) ------------------------------------------------------------------------
_TD_TERMS = ("w_esr", "w_dc", "w_log_cosh", "w_snr", "w_si_sdr", "w_sd_sdr", "w_mse")       # the order of the C ABI's weight arguments
_TD_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _time_options(what, weights, a, zero_mean, eps, reduction):
    """-> (the seven weights, a, eps, zero_mean, reduction code), validated as _options validates the STFT losses' keywords."""
    w = tuple(float(v) for v in weights)
    if not all(math.isfinite(v) for v in w):
        raise ValueError(f"{what}: the term weights must be finite, got {', '.join(_TD_TERMS)} = {w}")
    if not any(v != 0.0 for v in w):
        raise ValueError(f"{what}: at least one of the term weights {', '.join(_TD_TERMS)} must be non-zero")
    a, eps = float(a), float(eps)
    if not (math.isfinite(a) and a > 0.0):
        raise ValueError(f"{what}: a must be positive and finite, got {a!r}")
    if not math.isfinite(eps):
        raise ValueError(f"{what}: eps must be finite, got {eps!r}")
    if reduction not in _TD_REDUCTIONS:
        raise ValueError(f"{what}: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    return w, a, eps, bool(zero_mean), _TD_REDUCTIONS[reduction]


def _check_pair(input, target):
    if not isinstance(input, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("input and target must be torch.Tensors")
    if input.shape != target.shape:
        raise RuntimeError(f"input {tuple(input.shape)} and target {tuple(target.shape)} must have the same shape")
    if input.dim() < 1 or input.numel() == 0:
        raise ValueError(f"input must be shaped (..., seq_len) with at least one sample, got {tuple(input.shape)}")


class _TimeDomainFunction(torch.autograd.Function):
    """cfg: _time_options' tuple. One forward call (moment pass, per-row finalize, scalar) and one backward launch for both gradients."""

    @staticmethod
    def forward(ctx, inp, target, cfg):
        p32, t32 = _pair_rows(inp, target, "time_domain_loss")
        rows, N = p32.shape
        w, a, eps, zero_mean, red = cfg
        nd = _lib.lib().dasp_tdloss_scratch_doubles(rows, N)
        if nd < 0:
            raise _lib.DaspHipError(f"time_domain_loss: {rows} rows of {N} samples are not supported")
        dev = inp.device
        with torch.cuda.device(dev):
            scratch = torch.empty(nd, dtype=torch.float64, device=dev)
            moments = torch.empty(6 * rows, dtype=torch.float64, device=dev)
            row_loss = torch.empty(rows, dtype=torch.float32, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev) if red else None
            call("dasp_tdloss_forward", ptr(p32), ptr(t32), ptr(scratch), ptr(moments), ptr(row_loss), ptr(loss), rows, N, *w, a, eps,
                 int(zero_mean), red, stream())
        ctx.save_for_backward(p32, t32, moments)
        ctx.cfg = (cfg, rows, N, inp.shape, inp.dtype, target.dtype)
        return (loss if red else row_loss.reshape(inp.shape[:-1])).to(inp.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        p32, t32, moments = ctx.saved_tensors
        (w, a, eps, zero_mean, red), rows, N, shape, dtype, tdtype = ctx.cfg
        g = gt = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            with torch.cuda.device(p32.device):
                gl = gout.detach().reshape(-1).to(torch.float32).contiguous()          # one value, or one per row for reduction="none"
                g = torch.empty_like(p32) if ctx.needs_input_grad[0] else None
                gt = torch.empty_like(t32) if ctx.needs_input_grad[1] else None
                call("dasp_tdloss_backward", ptr(p32), ptr(t32), ptr(moments), ptr(gl), ptr(g), ptr(gt), rows, N, *w, a, eps, int(zero_mean), red,
                     stream())
        return _as_arguments(g, gt, shape, dtype, tdtype) + (None,)


def time_domain_loss(input: torch.Tensor, target: torch.Tensor, *, w_esr: float = 0.0, w_dc: float = 0.0, w_log_cosh: float = 0.0,
                     w_snr: float = 0.0, w_si_sdr: float = 0.0, w_sd_sdr: float = 0.0, w_mse: float = 0.0, a: float = 1.0,
                     zero_mean: bool = True, eps: float = 1e-8, reduction: str = "mean"):
    """The weighted sum of auraloss.time's losses and an MSE term from one pass over (..., seq_len) signals. Per row (all leading axes),
    with d = input - target: esr sum d^2 / (sum t^2 + eps); dc mean(d)^2 / (mean(t^2) + eps); log_cosh mean(log(cosh(a d) + eps) / a);
    snr -10 log10(sum t^2 / (sum d^2 + eps) + eps); si_sdr and sd_sdr with alpha = sum p t / (sum t^2 + eps): -10 log10(sum (alpha t)^2 /
    (sum (p - alpha t)^2 + eps) + eps) and -10 log10(sum (alpha t)^2 / (sum d^2 + eps) + eps), these three on the signals minus their row
    means when zero_mean; mse mean(d^2). A weight of exactly 0 leaves its term out of value and gradient; one must be non-zero.
    reduction: "mean" / "sum" over the rows, "none" the per-row values shaped input.shape[:-1]; the mse term is a per-row mean under every
    reduction (w_mse=1 with "mean" is torch.nn.MSELoss(); "sum" is the sum of the rows' means, not MSELoss(reduction="sum")).
    Both arguments are differentiable. float32, float16 and bfloat16 are computed in float32 and returned in the input's dtype."""
    cfg = _time_options("time_domain_loss", (w_esr, w_dc, w_log_cosh, w_snr, w_si_sdr, w_sd_sdr, w_mse), a, zero_mean, eps, reduction)
    _check_pair(input, target)
    return _TimeDomainFunction.apply(input, target, cfg)


class _TimeLoss(torch.nn.Module):
    """One term of time_domain_loss with weight 1."""
    _term = None

    def __init__(self, a=1.0, zero_mean=True, eps=1e-8, reduction="mean"):
        super().__init__()
        weights = tuple(1.0 if name == self._term else 0.0 for name in _TD_TERMS)
        self._cfg = _time_options(type(self).__name__, weights, a, zero_mean, eps, reduction)
        self.eps, self.reduction = eps, reduction

    def forward(self, input: torch.Tensor, target: torch.Tensor):
        _check_pair(input, target)
        return _TimeDomainFunction.apply(input, target, self._cfg)


class ESRLoss(_TimeLoss):
    """auraloss.time.ESRLoss (0.4.0): error-to-signal ratio sum (target - input)^2 / (sum target^2 + eps) per row."""
    _term = "w_esr"

    def __init__(self, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(eps=eps, reduction=reduction)


class DCLoss(_TimeLoss):
    """auraloss.time.DCLoss (0.4.0): mean(target - input)^2 / (mean(target^2) + eps) per row."""
    _term = "w_dc"

    def __init__(self, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(eps=eps, reduction=reduction)


class LogCoshLoss(_TimeLoss):
    """auraloss.time.LogCoshLoss (0.4.0): mean(log(cosh(a (input - target)) + eps) / a) per row, evaluated without overflow at large
    a |input - target| and without losing eps beside cosh ~ 1."""
    _term = "w_log_cosh"

    def __init__(self, a: float = 1.0, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(a=a, eps=eps, reduction=reduction)
        self.a = a


class SNRLoss(_TimeLoss):
    """auraloss.time.SNRLoss (0.4.0): -10 log10(sum target^2 / (sum (input - target)^2 + eps) + eps) per row, zero_mean: on the signals
    minus their row means."""
    _term = "w_snr"

    def __init__(self, zero_mean: bool = True, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(zero_mean=zero_mean, eps=eps, reduction=reduction)
        self.zero_mean = zero_mean


class SISDRLoss(_TimeLoss):
    """auraloss.time.SISDRLoss (0.4.0): alpha = sum input target / (sum target^2 + eps); -10 log10(sum (alpha target)^2 /
    (sum (input - alpha target)^2 + eps) + eps) per row."""
    _term = "w_si_sdr"

    def __init__(self, zero_mean: bool = True, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(zero_mean=zero_mean, eps=eps, reduction=reduction)
        self.zero_mean = zero_mean


class SDSDRLoss(_TimeLoss):
    """auraloss.time.SDSDRLoss (0.4.0): SISDRLoss's alpha; -10 log10(sum (alpha target)^2 / (sum (input - target)^2 + eps) + eps) per row."""
    _term = "w_sd_sdr"

    def __init__(self, zero_mean: bool = True, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__(zero_mean=zero_mean, eps=eps, reduction=reduction)
        self.zero_mean = zero_mean


class _FIRPairFunction(torch.autograd.Function):
    """Both signals through dasp_fir_same_forward in one launch; the backward is dasp_fir_same_adjoint on the gradients that exist."""

    @staticmethod
    def forward(ctx, inp, target, host_taps):
        p32, t32 = _pair_rows(inp, target, "FIRFilter")
        with torch.cuda.device(inp.device):
            taps = _fir_taps(host_taps, inp.device)
            pf, tf = _fir_pair("dasp_fir_same_forward", p32, t32, taps)
        ctx.save_for_backward(taps)
        ctx.cfg = (p32.shape, inp.shape, inp.dtype, target.dtype)
        return _as_arguments(pf, tf, inp.shape, inp.dtype, target.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gp, gt):
        (taps,) = ctx.saved_tensors
        rows_shape, shape, dtype, tdtype = ctx.cfg
        grads = [g.detach().reshape(rows_shape).to(torch.float32).contiguous() if need else None
                 for g, need in zip((gp, gt), ctx.needs_input_grad[:2])]
        with torch.cuda.device(taps.device):
            grads = _fir_pair("dasp_fir_same_adjoint", *grads, taps)
        return _as_arguments(*grads, shape, dtype, tdtype) + (None,)


class FIRFilter(torch.nn.Module):
    """auraloss.perceptual.FIRFilter(filter_type="hp", coef=0.85, fs=44100, ntaps=101): forward(input, target) returns both signals
    filtered, for ESRLoss()(*FIRFilter("hp")(y_hat, y)). Taps under conv1d's cross-correlation convention, y[n] = sum_k taps[k] x[n + k -
    ntaps // 2]: "hp" [1, -coef, 0] (first-order pre-emphasis), "fd" [1, 0, -coef] (folded differentiator), "aw" the 101 A-weighting
    taps of a_weighting_taps(fs) (ntaps must be 101). ntaps is odd. This library's definition of the length: the output has seq_len
    samples, the signal taken as zero outside the row ("same" padding, conv1d(padding=ntaps // 2)). Both signals go through one launch
    (dasp_fir_same_forward); the backward is the filter's adjoint."""

    def __init__(self, filter_type: str = "hp", coef: float = 0.85, fs: float = 44100, ntaps: int = 101):
        super().__init__()
        ntaps = operator.index(ntaps)
        if ntaps % 2 == 0:
            raise ValueError(f"ntaps must be odd (default is 101), got {ntaps}")
        if filter_type not in ("hp", "fd", "aw"):
            raise ValueError(f"Invalid filter_type: {filter_type!r} (one of 'hp', 'fd', 'aw')")
        coef = float(coef)
        if not math.isfinite(coef):
            raise ValueError(f"FIRFilter: coef must be finite, got {coef!r}")
        self.filter_type, self.coef, self.fs, self.ntaps = filter_type, coef, fs, ntaps
        if filter_type == "aw":
            if ntaps != AW_TAPS:
                raise NotImplementedError(f"FIRFilter: filter_type='aw' is implemented for ntaps={AW_TAPS} only, got {ntaps}")
            taps = a_weighting_taps(float(fs))
        else:
            taps = np.array([1.0, -coef, 0.0] if filter_type == "hp" else [1.0, 0.0, -coef], dtype=np.float32)
            taps.flags.writeable = False
        self._taps = taps

    def forward(self, input: torch.Tensor, target: torch.Tensor):
        _check_pair(input, target)
        return _FIRPairFunction.apply(input, target, self._taps)
