"""DSP primitives with the reference's names and signatures (dasp_pytorch/signal.py).

`sosfilt_via_fsm` keeps the reference's name for drop-in use, but it is evaluated as an exact
recurrence (chunked parallel scan, csrc/sosfilt.hip) instead of the reference's frequency-sampling
approximation; the two agree to <= 1e-13 in fp64 for stable filters whose impulse response has
decayed within the signal length. float64 input takes the double-precision
kernels of csrc/ref64.hip (ops64.py): float64 in, float64 arithmetic, as in the reference.

`fft_freqz` / `fft_sosfreqz` keep the reference's frequency responses: evaluated per bin in fp64 (csrc/freqz.hip) instead of through
zero-padded FFTs, for float32 and float64 alike, with a hand-written adjoint. `freqdomain_fir` applies such a response (or any other) to
audio: irfft(rfft(x, n_fft) * H, n_fft) on the library's own transforms (csrc/fdfir.hip), float32, n_fft a power of two from 8 to 2^20.
"""
import functools
import numbers
import operator

import numpy as np
import scipy.signal
import torch

from . import _lib, _resample_design
from . import ops as _ops
from .ops import FILTER_TYPES, BiquadFunction, SosFiltFunction
from .ops64 import LFilterFunction, SosFilt64Function, is_f64


def biquad(gain_db: torch.Tensor, cutoff_freq: torch.Tensor, q_factor: torch.Tensor, sample_rate: float, filter_type: str = "peaking"):
    """RBJ-cookbook biquad design (reference: dasp_pytorch/signal.py:242-306): gain_db, cutoff_freq, q_factor with bs values each
    (the reference's (bs, 1)) -> b, a of shape (bs, 3), normalised by a0 (so a[:, 0] == 1), dtype and device of gain_db.
    filter_type: "peaking", "low_shelf", "high_shelf", "low_pass", "high_pass"; anything else raises ValueError as in the reference.
    The design runs on the device in fp64 (the kernel the fused parametric_eq path uses, csrc/sosfilt.hip rbj_design) and is
    differentiable w.r.t. all three controls through its in-kernel Jacobian."""
    if filter_type not in FILTER_TYPES:
        raise ValueError(f"Invalid filter_type: {filter_type}.")
    bs = gain_db.size(0)
    if any(t.numel() != bs for t in (gain_db, cutoff_freq, q_factor)):
        raise RuntimeError(f"biquad: gain_db, cutoff_freq and q_factor must hold one value per batch item ({bs}); "
                           f"got {[tuple(t.shape) for t in (gain_db, cutoff_freq, q_factor)]}")
    ba = BiquadFunction.apply(gain_db.reshape(bs), cutoff_freq.reshape(bs), q_factor.reshape(bs), float(sample_rate), FILTER_TYPES[filter_type])
    ba = ba.to(gain_db.dtype)
    return ba[:, :3], ba[:, 3:]


OVERSAMPLE_FACTORS = (1, 2, 4, 8)
OVERSAMPLE_MAX_HALF_WIDTH = 16


def check_oversampling(oversample, half_width, beta, cutoff):
    """The argument ranges of oversampling_taps / functional.oversampled_distortion: ValueError naming the argument and what it may be."""
    if isinstance(oversample, bool) or not isinstance(oversample, numbers.Integral) or oversample not in OVERSAMPLE_FACTORS:
        raise ValueError(f"oversample must be one of {OVERSAMPLE_FACTORS}, got {oversample!r}")
    if isinstance(half_width, bool) or not isinstance(half_width, numbers.Integral) or not 1 <= half_width <= OVERSAMPLE_MAX_HALF_WIDTH:
        raise ValueError(f"half_width must be an integer from 1 to {OVERSAMPLE_MAX_HALF_WIDTH}, got {half_width!r}")
    if not (isinstance(beta, numbers.Real) and not isinstance(beta, bool) and 0.0 <= beta < float("inf")):
        raise ValueError(f"beta must be a finite number >= 0, got {beta!r}")
    if not (isinstance(cutoff, numbers.Real) and not isinstance(cutoff, bool) and 0.0 < cutoff <= 1.0):
        raise ValueError(f"cutoff must lie in (0, 1], got {cutoff!r}")


def oversampling_taps(oversample: int, half_width: int = 12, beta: float = 8.0, cutoff: float = 0.9):
    """The low-pass of functional.oversampled_distortion, used once to interpolate by L = `oversample` and once to decimate: a Kaiser-windowed
    sinc over `half_width` base samples to either side, h[c] = cutoff sinc(cutoff c / L) I0(beta sqrt(1 - (c / (H L))^2)) / I0(beta) for
    c = -H L .. H L, with its cutoff at `cutoff` times the base Nyquist frequency. Every phase h[p::L] sums to about 1 (unit gain at DC
    after interpolation). Returns the 2 H L + 1 taps as a float64 CPU tensor."""
    check_oversampling(oversample, half_width, beta, cutoff)
    L, H = int(oversample), int(half_width)
    c = np.arange(-H * L, H * L + 1, dtype=np.float64)
    return torch.from_numpy(cutoff * np.sinc(cutoff * c / L) * np.kaiser(2 * H * L + 1, beta))


def control_frames(seq_len: int, hop: int):
    """The number of frame points F = ceil(seq_len / hop) + 1 that a control curve of functional.time_varying_filter holds for a signal of
    seq_len samples: frame point j sits at sample j hop, and every sample lies between two of them. ValueError for a hop that is no
    power of two from 8 to 2048 or a negative seq_len."""
    if isinstance(hop, bool) or not isinstance(hop, numbers.Integral) or not 8 <= hop <= 2048 or hop & (hop - 1):
        raise ValueError(f"hop must be a power of two from 8 to 2048, got {hop!r}")
    if isinstance(seq_len, bool) or not isinstance(seq_len, numbers.Integral) or seq_len < 0:
        raise ValueError(f"seq_len must be a non-negative integer, got {seq_len!r}")
    return -(-int(seq_len) // int(hop)) + 1


FDN_MAX_LINES = 16


def check_fdn_delays(delays):
    """The line lengths of functional.fdn_reverb as a tuple of ints: ValueError unless they are a sequence of 1 to 16 ints >= 1 (bools
    and tensors refused; repeats allowed)."""
    if isinstance(delays, (str, bytes, torch.Tensor, np.ndarray)) or not isinstance(delays, (list, tuple, range)):
        raise ValueError(f"delays must be a list or tuple of 1 to {FDN_MAX_LINES} ints >= 1, got {delays!r}")
    if not 1 <= len(delays) <= FDN_MAX_LINES:
        raise ValueError(f"delays must hold 1 to {FDN_MAX_LINES} line lengths, got {len(delays)}")
    for m in delays:
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m < 2 ** 31:
            raise ValueError(f"delays must be ints >= 1 (samples), got {m!r}")
    return tuple(int(m) for m in delays)


def _is_prime(n):
    if n < 2:
        return False
    d = 2
    while d * d <= n:
        if n % d == 0:
            return False
        d += 1
    return True


def fdn_delay_lengths(sample_rate: float, lines: int = 8, shortest_ms: float = 23.0, longest_ms: float = 83.0):
    """A default delay set for functional.fdn_reverb: `lines` distinct primes, in samples and in ascending order. Point k of a logarithmic
    spacing from sample_rate/1000 shortest_ms to sample_rate/1000 longest_ms (the shortest alone when lines = 1) goes to the prime
    nearest to it (the smaller on a tie), and on to the next larger free prime where that one is taken. Primes share no factor, so the
    lines' echoes do not pile up on common multiples. Pure Python, no device. ValueError for a sample rate that is not positive and
    finite, lines outside 1 .. 16, or lengths that are not 0 < shortest_ms <= longest_ms < inf."""
    try:
        sr, lo, hi = float(sample_rate), float(shortest_ms), float(longest_ms)
    except (TypeError, ValueError):
        raise ValueError(f"fdn_delay_lengths: numbers expected, got {sample_rate!r}, {shortest_ms!r}, {longest_ms!r}") from None
    if not (0.0 < sr < float("inf")):
        raise ValueError(f"sample_rate must be positive and finite, got {sample_rate!r}")
    if isinstance(lines, bool) or not isinstance(lines, numbers.Integral) or not 1 <= lines <= FDN_MAX_LINES:
        raise ValueError(f"lines must be an integer from 1 to {FDN_MAX_LINES}, got {lines!r}")
    if not (0.0 < lo <= hi < float("inf")):
        raise ValueError(f"0 < shortest_ms <= longest_ms < inf expected, got {shortest_ms!r}, {longest_ms!r}")
    a, b = sr / 1000.0 * lo, sr / 1000.0 * hi
    taken = []
    for k in range(lines):
        point = a if lines == 1 else a * (b / a) ** (k / (lines - 1))
        below = max(int(point), 2)
        while not _is_prime(below):
            below -= 1
        above = max(int(point), 2)
        while not _is_prime(above) or above < point:
            above += 1
        p = below if point - below <= above - point else above
        while p in taken or not _is_prime(p):
            p += 1
        taken.append(p)
    return sorted(taken)


check_resampling = _resample_design.check_resampling


def resample_taps(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                  resampling_method: str = "sinc_interp_hann", beta: float = None):
    """The polyphase filter of functional.resample (torchaudio.functional.resample's published design, restated). With
    o : n the rates divided by their gcd, base = min(o, n) rolloff, width = ceil(lowpass_filter_width o / base) and K = 2 width + o:
        t = (-r / n + (k - width) / o) base, clamped to +-lowpass_filter_width = +-W                  r in [0, n), k in [0, K)
        window = cos^2(pi t / (2 W))  ("sinc_interp_hann")   or   I0(beta sqrt(1 - (t / W)^2)) / I0(beta)  ("sinc_interp_kaiser",
                                                                  beta = 14.769656459379492 when None)
        h[r][k] = sinc(t) window base / o
    One deviation from torchaudio: where t was clamped, h[r][k] is exactly 0 (torchaudio's formula gives at most 1e-20 there for the
    Kaiser window and a float32 zero for the Hann window), so every phase has a compact span of taps. Output q n + r of the resampler is
    sum_k h[r][k] x[q o + k - width]. Returns (h as a float64 CPU tensor (n, K), width). check_resampling(...) is the argument check:
    ValueError for rates that are not positive integers, lowpass_filter_width < 1, a rolloff outside (0, 1], an unknown method, a
    negative or non-finite beta."""
    o, n = check_resampling(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    h, width, _ = _resample_design.taps(o, n, lowpass_filter_width, rolloff, resampling_method, beta)
    return torch.from_numpy(h), width


def lfilter_via_fsm(x: torch.Tensor, b: torch.Tensor, a: torch.Tensor = None):
    """IIR / FIR filter along the last dimension of x (reference: dasp_pytorch/signal.py:95-133): x (bs, 1, timesteps), b (bs, K)
    numerator and a (bs, K) denominator coefficients (any a0), or a = None for an FIR filter. As in the reference x must have one
    channel (`assert chs == 1`). Evaluated as an exact recurrence - one section of the cascaded-biquad scan (csrc/sosfilt.hip) - instead
    of the reference's frequency-sampling approximation; differentiable w.r.t. x, b and a.
    K <= 3 (the reference's only caller is the compressor's one-pole smoother, K = 2, functional.py:372-380) is one section of the
    cascaded-biquad kernels. K = 4 .. 16 runs the recurrence of order K - 1 in double arithmetic, chunks of time side by side and
    stitched by their state transition (csrc/lfilter.hip - the boundary's long tail, not one of the tuned kernels). More than 16
    coefficients raise NotImplementedError (factor into second-order sections and call sosfilt_via_fsm)."""
    bs, chs, seq_len = x.size()  # enforce shape
    assert chs == 1
    K = b.shape[-1]
    if b.dim() != 2 or b.shape[0] not in (1, bs) or (a is not None and a.shape != b.shape):
        raise RuntimeError(f"lfilter_via_fsm: b (and a) must have shape ({bs}, K); got {tuple(b.shape)}" + (f", {tuple(a.shape)}" if a is not None else ""))
    if K > 16:
        raise NotImplementedError(f"lfilter_via_fsm: K = {K} coefficients; recurrences of up to 16 coefficients are evaluated directly. "
                                  "Factor the filter into second-order sections, e.g. sos = scipy.signal.tf2sos(b, a) per batch item, "
                                  "stack them as (bs, n_sections, 6) and call dasp_pytorch_amd.signal.sosfilt_via_fsm(sos, x) "
                                  "(differentiable w.r.t. the sections; any number of sections)")
    if K > 3:
        b = b.type_as(x).double()                        # the reference's rounding of the coefficients (signal.py:113,119), then exact
        if a is None:
            an = torch.zeros_like(b)
            an[:, 0] = 1.0
            bn = b
        else:
            a = a.type_as(x).double()
            bn, an = b / a[:, :1], a / a[:, :1]          # H = B / A for any a0 (signal.py:7-11); torch differentiates the normalisation
        return LFilterFunction.apply(x, bn, an)
    b = b.type_as(x)
    if a is None:
        a = torch.zeros_like(b)
        a[:, 0] = 1.0
    else:
        a = a.type_as(x)
    if K < 3:
        pad = torch.zeros(b.shape[0], 3 - K, dtype=b.dtype, device=b.device)
        b, a = torch.cat([b, pad], 1), torch.cat([a, pad], 1)
    sos = torch.cat([b, a], 1).unsqueeze(1)                  # (bs, 1, 6) rows [b0 b1 b2 a0 a1 a2]
    return (SosFilt64Function if is_f64(x) else SosFiltFunction).apply(sos, x)


def _frequency_domain_helper(name, line):
    def fn(*args, **kwargs):
        raise NotImplementedError(
            f"dasp_pytorch_amd.signal.{name}: the reference's frequency-sampling internals (dasp_pytorch/signal.py:{line}) have no counterpart "
            "here - the filters are evaluated as exact recurrences (sosfilt_via_fsm, lfilter_via_fsm), not as spectra")
    fn.__name__ = name
    return fn


# The reference's L1 helpers of the frequency-sampling method are not part of this package's boundary; they exist as names
# so that `from dasp_pytorch_amd.signal import *` fails loudly at the call, not at import. one_pole_butter_lowpass / one_pole_filter
# are dead code in the reference (they print to stdout). freqdomain_fir is implemented below.
one_pole_butter_lowpass = _frequency_domain_helper("one_pole_butter_lowpass", "169-198")
one_pole_filter = _frequency_domain_helper("one_pole_filter", "201-239")


FREQZ_MAX_TAPS = 32           # per polynomial of fft_freqz (csrc/freqz.hip evaluates every bin directly)
FREQZ_MAX_SECTIONS = 16       # of fft_sosfreqz


def _freqz_n(n_fft):
    """n_fft as a Python int: an integer or a 0-dim integer tensor (the reference's sosfilt_via_fsm passes one, signal.py:150-151)."""
    if isinstance(n_fft, torch.Tensor):
        if n_fft.dim() != 0 or n_fft.is_floating_point() or n_fft.is_complex():
            raise TypeError(f"n_fft must be an integer or a 0-dim integer tensor, got a {n_fft.dtype} tensor of shape {tuple(n_fft.shape)}")
        n_fft = n_fft.item()
    n = operator.index(n_fft)
    if n < 1:
        raise ValueError(f"n_fft must be >= 1, got {n}")
    return n


def _freqz_dtype(*tensors):
    """float64 if the inputs promote to float64, else float32 (the kernels compute in fp64 either way and store in this precision)."""
    dt = functools.reduce(torch.promote_types, [t.dtype for t in tensors])
    if not dt.is_floating_point:
        raise TypeError(f"filter coefficients must be real floating-point tensors, got {', '.join(str(t.dtype) for t in tensors)}")
    return torch.float64 if dt == torch.float64 else torch.float32


def fft_freqz(b: torch.Tensor, a: torch.Tensor, n_fft: int = 512):
    """Complex frequency response H = rfft(b, n_fft) / rfft(a, n_fft) (reference: dasp_pytorch/signal.py:7-11), shape (..., n_fft // 2 + 1).

    b (..., Kb) and a (..., Ka) are real; their leading shapes broadcast. a0 is not normalised. Taps beyond n_fft are cropped, as
    torch.fft.rfft crops its input; n_fft is any integer >= 1 or a 0-dim integer tensor. Evaluated per bin in fp64 (csrc/freqz.hip,
    through torch.ops.dasp.freqz) instead of two FFTs: complex64 out for float32 in, complex128 for float64. Differentiable w.r.t. b
    and a. At most 32 taps each: a longer FIR wants an FFT, not a per-bin polynomial (NotImplementedError)."""
    _lib.require_device(b, "b")
    _lib.require_device(a, "a")
    _lib.require_same_device(b, a=a)
    n = _freqz_n(n_fft)
    dt = _freqz_dtype(b, a)
    if b.dim() < 1 or a.dim() < 1 or b.shape[-1] < 1 or a.shape[-1] < 1:
        raise ValueError(f"fft_freqz: b and a need at least one tap, got shapes {tuple(b.shape)} and {tuple(a.shape)}")
    b, a = b[..., :n], a[..., :n]
    Kb, Ka = b.shape[-1], a.shape[-1]
    if max(Kb, Ka) > FREQZ_MAX_TAPS:
        raise NotImplementedError(f"fft_freqz: {Kb} numerator / {Ka} denominator taps (after cropping to n_fft = {n}); polynomials of up to "
                                  f"{FREQZ_MAX_TAPS} taps are evaluated per bin. A longer FIR wants an FFT, not a per-bin polynomial: "
                                  "torch.fft.rfft(b, n_fft), or factor the filter into second-order sections and call fft_sosfreqz")
    lead = torch.broadcast_shapes(b.shape[:-1], a.shape[:-1])
    bb = b.to(dt).expand(*lead, Kb).reshape(-1, 1, Kb)
    aa = a.to(dt).expand(*lead, Ka).reshape(-1, 1, Ka)
    return _ops.freqz(bb, aa, n).reshape(*lead, n // 2 + 1)


def fft_sosfreqz(sos: torch.Tensor, n_fft: int = 512):
    """Complex frequency response of a cascade of biquads, H = prod_s B_s / A_s (reference: dasp_pytorch/signal.py:14-32).

    sos: (bs, n_sections, 6) rows [b0 b1 b2 a0 a1 a2], 1 to 16 sections -> H (bs, n_fft // 2 + 1), complex64 for float32 and complex128
    for float64. One kernel evaluates every section per bin in fp64 (csrc/freqz.hip); differentiable w.r.t. sos."""
    bs, n_sections, n_coeffs = sos.size()
    assert n_coeffs == 6  # must be second order (signal.py:24)
    _lib.require_device(sos, "sos")
    n = _freqz_n(n_fft)
    if not 1 <= n_sections <= FREQZ_MAX_SECTIONS:
        raise NotImplementedError(f"fft_sosfreqz: {n_sections} sections; 1 to {FREQZ_MAX_SECTIONS} are evaluated in one call "
                                  "(multiply the responses of successive calls for a longer cascade)")
    s = sos.to(_freqz_dtype(sos))
    return _ops.freqz(s[..., :3], s[..., 3:], n)


FDFIR_MIN_N, FDFIR_MAX_N = 8, 1 << 20        # transform lengths of freqdomain_fir (csrc/fdfir.hip): the powers of two in between
FDFIR_MAX_SHARED = 8                         # rows that share one response inside the kernels (one wave / workgroup walks them in turn)


def freqdomain_fir(x: torch.Tensor, H: torch.Tensor, n_fft: int):
    """Filter by a supplied frequency response: irfft(rfft(x, n_fft) * H, n_fft) (reference: dasp_pytorch/signal.py:35-39) - circular
    convolution of length n_fft. The result is not cropped: its last dimension is n_fft.

    x (..., T) real float32, T >= 1: zero-padded to n_fft, or cropped to it, as torch.fft.rfft does. H (..., n_fft // 2 + 1) complex64 in
    rfft order; its leading dimensions broadcast against x.shape[:-1]. A real H is a zero-phase response (the reference's `H.type_as(X)`)
    and gets a real gradient. The imaginary parts of the DC and Nyquist bins do not reach the output (irfft ignores them); their gradient
    is exactly 0. n_fft: an integer or a 0-dim integer tensor, a power of two from 8 to 2^20 (NotImplementedError otherwise).
    Differentiable w.r.t. x and H (PyTorch's convention for complex gradients); gradients are bit-identical from run to run.

    One launch per direction up to n_fft = 8192, a four-step transform above (csrc/fdfir.hip, through torch.ops.dasp.freqdomain_fir). A
    response per row, or one shared by the trailing dimensions of x (H (bs, 1, bins) on x (bs, chs, T): the reference's own call) is read
    as it is (up to 8 rows per response) - two rows that share a response travel as one complex transform; any other broadcast pattern
    is expanded first.
    float64 / complex128 input is refused unless config.plan.fp64_as_fp32 (then cast, computed in float32 and cast back)."""
    from .ops64 import require_fp32_ok
    for name, t in (("x", x), ("H", H)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    n = _freqz_n(n_fft)
    if n < FDFIR_MIN_N or n > FDFIR_MAX_N or n & (n - 1):
        raise NotImplementedError(f"freqdomain_fir: n_fft = {n}; supported are the powers of two from {FDFIR_MIN_N} to {FDFIR_MAX_N} (2^20). "
                                  "For another length: torch.fft.irfft(torch.fft.rfft(x, n_fft) * H, n_fft)")
    if x.is_complex() or not x.is_floating_point():
        raise TypeError(f"freqdomain_fir: x must be a real floating-point tensor, got {x.dtype}")
    if not (H.is_complex() or H.is_floating_point()):
        raise TypeError(f"freqdomain_fir: H must be a complex or real floating-point tensor, got {H.dtype}")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"freqdomain_fir: x needs at least one sample along its last dimension, got shape {tuple(x.shape)}")
    bins = n // 2 + 1
    if H.dim() < 1 or H.shape[-1] != bins:
        raise RuntimeError(f"freqdomain_fir: H has {H.shape[-1] if H.dim() else 0} bins along its last dimension, n_fft = {n} needs {bins}")
    require_fp32_ok(x, "freqdomain_fir")
    if H.dtype in (torch.float64, torch.complex128):
        require_fp32_ok(torch.empty(0, dtype=torch.float64), "freqdomain_fir (H)")
    _lib.require_device(x, "x")
    _lib.require_device(H, "H")
    _lib.require_same_device(x, H=H)
    out_dtype = torch.float64 if torch.float64 in (x.dtype, H.real.dtype if H.is_complex() else H.dtype) else torch.float32
    xx = x.to(torch.float32)
    Hc = H.to(torch.complex64) if H.is_complex() else torch.complex(H.to(torch.float32), torch.zeros_like(H, dtype=torch.float32))
    lead = torch.broadcast_shapes(xx.shape[:-1], Hc.shape[:-1])
    T = xx.shape[-1]
    if tuple(xx.shape[:-1]) != tuple(lead):
        xx = xx.expand(*lead, T)
    hl = (1,) * (len(lead) - (Hc.dim() - 1)) + tuple(Hc.shape[:-1])
    # H shared by the trailing dimensions of x (hl = lead[:m] + (1, ..., 1)) goes in as it is; anything else is expanded to a response per row
    m = len(lead)
    while m > 0 and hl[m - 1] == 1:
        m -= 1
    shared = functools.reduce(operator.mul, lead[m:], 1)
    if hl[:m] != tuple(lead[:m]) or shared > FDFIR_MAX_SHARED:
        Hc = Hc.expand(*lead, bins)
    y = _ops.freqdomain_fir(xx.reshape(-1, T), Hc.reshape(-1, bins), n).reshape(*lead, n)
    return y if out_dtype == torch.float32 else y.to(out_dtype)


def sosfilt_via_fsm(sos: torch.Tensor, x: torch.Tensor):
    """Cascade of second-order sections along the last dim of x (reference: signal.py:136-166).

    sos: (bs, n_sections, 6) rows [b0 b1 b2 a0 a1 a2]; bs may be 1 (broadcast). x: (bs, ..., T).
    Differentiable w.r.t. both. Up to 8 sections are one launch per direction (the backward pass is the Gram-matrix kernel for every
    section count: 0.46 ms forward + backward for 8 sections on (256, 2, 131072), profiles/r04/sections_per_call.log); longer cascades are
    applied as successive calls of at most 6 sections."""
    bs, n_sections, n_coeffs = sos.size()
    assert n_coeffs == 6  # must be second order (signal.py:24)
    shape = x.shape
    xx = x.reshape(shape[0], -1, shape[-1])
    if is_f64(x):            # float64 in, float64 arithmetic, as the reference (ops64.py): any number of sections in one call
        return SosFilt64Function.apply(sos, xx).reshape(shape)
    step = 8 if n_sections <= 8 else 6
    for s0 in range(0, n_sections, step):
        xx = _ops.sosfilt(sos[:, s0:s0 + step], xx)         # torch.ops.dasp.sosfilt (csrc/torch_ext), or the ctypes binding
    return xx.reshape(shape)


OCTAVE_BANDS = (31.5, 63, 125, 250, 500, 1000, 2000, 4000, 8000, 16000)


@functools.lru_cache(maxsize=16)
def _octave_band_taps(num_taps: int, sample_rate: float):
    """SciPy window-method design of the 12 filters, exactly the reference's calls (signal.py:60-87); host-side and
    parameter-free, so it is designed once per (num_taps, sample_rate) and cached (the reference redesigns per call)."""
    filts = [scipy.signal.firwin(num_taps, 12, fs=sample_rate)]
    for fc in OCTAVE_BANDS:
        f_min = fc / np.sqrt(2)
        f_max = np.clip(fc * np.sqrt(2), a_min=0, a_max=(sample_rate / 2) * 0.999)
        filts.append(scipy.signal.firwin(num_taps, [f_min, f_max], fs=sample_rate, pass_zero=False))
    filts.append(scipy.signal.firwin(num_taps, 18000, fs=sample_rate, pass_zero=False))
    return np.stack([f.astype("float32")[::-1] for f in filts], 0).copy()   # the reference's torch.flip (a no-op: symmetric)


def octave_band_filterbank(num_taps: int, sample_rate: float):
    """Octave-spaced linear-phase FIR bank, shape (12, 1, num_taps) float32 on the CPU, as the reference
    (dasp_pytorch/signal.py:42-92): lowpass 12 Hz, ten octave bandpasses 31.5 Hz .. 16 kHz, highpass 18 kHz."""
    return torch.from_numpy(_octave_band_taps(int(num_taps), float(sample_rate)).copy()).unsqueeze(1)   # a fresh tensor per call, as the reference


def k_weighting_sos(sample_rate: float):
    """The K-weighting filter of ITU-R BS.1770-4 designed for `sample_rate` (8000 .. 384000 Hz): a (2, 6) float64 tensor on the CPU, rows
    [b0 b1 b2 a0 a1 a2] - the high-frequency shelf, then the high-pass. It is the table functional.loudness's kernels use (the library's
    own host-side design, csrc/loudness.hip), so it can be fed to sosfilt_via_fsm or fft_sosfreqz. At 48 kHz it reproduces the
    recommendation's coefficient table to 1e-15."""
    import ctypes
    fs = float(sample_rate)
    if not 8000.0 <= fs <= 384000.0:
        raise ValueError(f"k_weighting_sos: sample_rate must lie in [8000, 384000], got {sample_rate!r}")
    out = (ctypes.c_double * 12)()
    _lib.check(_lib.lib().dasp_loudness_kweighting(fs, out), "dasp_loudness_kweighting")
    return torch.tensor(list(out), dtype=torch.float64).reshape(2, 6)
