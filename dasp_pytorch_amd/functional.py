"""Drop-in for dasp_pytorch.functional on MI355X: same names, argument order and keyword names
(dasp_pytorch/functional.py), every effect computed by hand-written HIP kernels (csrc/)."""
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import signal as _signal
from . import _mt19937
from . import ops as _ops
from . import _lib
from .ops import (ENVELOPE_DETECTORS, FILTER_TYPES, BallisticsFunction, BlockLevelFunction, BusFunction, DistortionSampleFunction, EnvelopeFollowerFunction, FdnReverbFunction, FeedbackDelayFunction, GainCurveFunction,
                  LimiterFunction, ModulatedDelayFunction, OversampledDistortionFunction, PannerFunction,
                  PhaserFunction, ResampleFunction, StereoMixFunction, TVEQ_MODES, TVFILTER_MODES, TimeVaryingEQFunction, TimeVaryingFilterFunction, WidenerFunction)
from .ops import reverb as _ops_reverb
from .ops64 import Dynamics64Function, Elementwise64Function, ParametricEQ64Function, is_f64, require_fp32_ok

_PEQ_TYPES = [FILTER_TYPES[t] for t in ("low_shelf", "peaking", "peaking", "peaking", "peaking", "high_shelf")]


def gain(x: torch.Tensor, sample_rate: int, gain_db: torch.Tensor):
    """Apply gain in dB; the same gain is applied to every channel of a batch item
    (reference: dasp_pytorch/functional.py:10-29). gain_db: bs values (any shape that views to (bs, 1, 1))."""
    bs, chs, seq_len = x.size()
    if gain_db.numel() != bs:   # the reference's gain_db.view(bs, 1, 1)
        raise RuntimeError(f"shape '[{bs}, 1, 1]' is invalid for input of size {gain_db.numel()}")
    if is_f64(x):            # float64 in, float64 arithmetic, as the reference (ops64.py)
        return Elementwise64Function.apply(x, gain_db, 0)
    return _ops.gain(x, gain_db)                      # torch.ops.dasp.gain (csrc/torch_ext), or the ctypes binding


def distortion(x: torch.Tensor, sample_rate: int, drive_db: torch.Tensor):
    """Soft-clipping distortion tanh(x * 10^(drive_db/20)) (reference: dasp_pytorch/functional.py:65-78).
    As in the reference's drive_db.view(bs, chs, -1), drive_db holds one value per (batch item, channel) row, i.e. bs*chs values (so a
    (bs,) drive only works for mono input), or one value per sample, bs*chs*seq_len values; any other count fails as the reference's
    view / broadcast does."""
    bs, chs, seq_len = x.size()
    n = drive_db.numel()
    if n == bs * chs * seq_len and seq_len != 1:
        if is_f64(x):
            require_fp32_ok(x, "distortion with per-sample drive_db")
        return DistortionSampleFunction.apply(x, drive_db)
    if n != bs * chs:
        if bs * chs == 0 or n % (bs * chs) != 0:
            raise RuntimeError(f"shape '[{bs}, {chs}, -1]' is invalid for input of size {n}")
        raise RuntimeError(f"The size of tensor a ({seq_len}) must match the size of tensor b ({n // (bs * chs)}) at non-singleton dimension 2")
    if is_f64(x):
        return Elementwise64Function.apply(x, drive_db, 1)
    return _ops.distortion(x, drive_db)


_OS_TAPS = {}


def _oversampling_taps_f32(oversample, half_width, beta, cutoff):
    """The float64 taps of signal.oversampling_taps rounded once to float32, as the ctypes array the C call takes; kept per design."""
    key = (oversample, half_width, float(beta), float(cutoff))
    hit = _OS_TAPS.get(key)
    if hit is None:
        h = _signal.oversampling_taps(oversample, half_width, beta, cutoff).to(torch.float32)
        hit = (ctypes.c_float * h.numel())(*h.tolist())
        if len(_OS_TAPS) >= 32:
            _OS_TAPS.clear()
        _OS_TAPS[key] = hit
    return hit


def oversampled_distortion(x: torch.Tensor, sample_rate: int, drive_db: torch.Tensor, oversample: int = 4, half_width: int = 12,
                           beta: float = 8.0, cutoff: float = 0.9):
    """Anti-aliased soft clipper: `distortion` evaluated at `oversample` times the sample rate. x (bs, chs, seq_len) is interpolated by
    L = oversample with the Kaiser-windowed sinc of signal.oversampling_taps(oversample, half_width, beta, cutoff), goes through
    tanh(. * 10^(drive_db/20)), is low-passed by the same taps and decimated by L - centred: no latency, same length as x, zeros assumed
    outside the signal. In torch terms, with h the taps and H = half_width:
        u = conv_transpose1d(x, h, stride=L)[..., H*L : H*L + L*seq_len];  y = conv1d(tanh(g * u), h / L, stride=L, padding=H*L)
    as one kernel per direction that keeps the L-times-longer signal on chip (csrc/oversample.hip). The harmonics that tanh at the base
    rate folds back below Nyquist are rejected by about 62 dB at the defaults and 78 dB with oversample=8.
    drive_db holds one value per (batch item, channel) row, bs*chs values, as in `distortion`. oversample is 1, 2, 4 or 8 (1 is
    `distortion` itself), half_width an integer from 1 to 16, 0 < cutoff <= 1 and beta >= 0: anything else raises ValueError.
    float32 only. Differentiable in x and drive_db."""
    _signal.check_oversampling(oversample, half_width, beta, cutoff)
    if oversample == 1:
        return distortion(x, sample_rate, drive_db)
    bs, chs, seq_len = x.size()
    n = drive_db.numel()
    if n != bs * chs:
        if bs * chs == 0 or n % (bs * chs) != 0:
            raise RuntimeError(f"shape '[{bs}, {chs}, -1]' is invalid for input of size {n}")
        raise RuntimeError(f"The size of tensor a ({seq_len}) must match the size of tensor b ({n // (bs * chs)}) at non-singleton dimension 2")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "oversampled_distortion")
    oversample, half_width = int(oversample), int(half_width)
    return OversampledDistortionFunction.apply(x, drive_db, _oversampling_taps_f32(oversample, half_width, beta, cutoff), oversample, half_width)


def modulated_delay(x: torch.Tensor, sample_rate: float, delay_ms: torch.Tensor, depth_ms: torch.Tensor, rate_hz: torch.Tensor,
                    phase: torch.Tensor, mix: torch.Tensor, max_delay_ms: float = 40.0, stereo_spread: float = 0.25):
    """Chorus / flanger / vibrato: V voices of a delay line whose length a sine LFO moves, mixed with the dry signal. x (bs, chs, seq_len);
    delay_ms, depth_ms, rate_hz and phase hold bs*V values each, shaped (bs,) or (bs, V), V = numel / bs voices, 1 <= V <= 8; mix holds
    bs values. phase and stereo_spread are in turns. For item b, voice v, channel c and sample n, with x zero outside the signal:
        theta = 2 pi (rate_hz n / sample_rate + phase + c stereo_spread)
        d = clamp(sample_rate/1000 (delay_ms + depth_ms sin theta), 0, sample_rate/1000 max_delay_ms);  p = n - d, i = floor(p), f = p - i
        tap_v[n] = Catmull-Rom interpolation of x[i-1], x[i], x[i+1], x[i+2] at f;   y[n] = (1 - mix) x[n] + mix (1/V) sum_v tap_v[n]
    A flanger is one voice of 1-5 ms with mix = 0.5; a chorus a few voices of 10-30 ms at different phases; a vibrato mix = 1. The read
    position is float64 in the kernel, the interpolation float32 (csrc/moddelay.hip). The op works on whole tensors, not on a stream:
    where d < 1 sample the four-point footprint reaches x[n+1]. There is no feedback path: feedback_delay is the line that has one.
    Differentiable in x and in all five controls; the delay gradients take no contribution from samples where d was clamped - size
    max_delay_ms (a plain float, like stereo_spread; at most 8192 samples) so that delay_ms + depth_ms stays inside it.
    float32 only. A wrong control count raises RuntimeError naming the control; more than 8 voices or a max_delay_ms beyond 8192
    samples raise DaspHipError (unsupported configuration)."""
    bs, chs, seq_len = x.size()
    n = delay_ms.numel()
    if bs and (n == 0 or n % bs != 0):
        raise RuntimeError(f"delay_ms: shape '[{bs}, -1]' is invalid for input of size {n}")
    for name, c in (("depth_ms", depth_ms), ("rate_hz", rate_hz), ("phase", phase)):
        if c.numel() != n:
            raise RuntimeError(f"{name}: shape '[{bs}, {n // bs if bs else 0}]' is invalid for input of size {c.numel()}")
    if mix.numel() != bs:
        raise RuntimeError(f"mix: shape '[{bs}]' is invalid for input of size {mix.numel()}")
    max_delay_ms, stereo_spread = float(max_delay_ms), float(stereo_spread)
    if not (max_delay_ms >= 0.0 and max_delay_ms != float("inf")) or stereo_spread - stereo_spread != 0.0 or not float(sample_rate) > 0.0:
        raise ValueError(f"modulated_delay: sample_rate > 0, finite max_delay_ms >= 0 and finite stereo_spread, got {sample_rate}, {max_delay_ms}, {stereo_spread}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "modulated_delay")
    H = max(1, math.ceil(float(sample_rate) / 1000.0 * max_delay_ms))
    return ModulatedDelayFunction.apply(x, delay_ms, depth_ms, rate_hz, phase, mix, float(sample_rate), max_delay_ms, stereo_spread, H)


def feedback_delay(x: torch.Tensor, sample_rate: float, delay_ms: torch.Tensor, feedback: torch.Tensor, damping_hz: torch.Tensor,
                   mix: torch.Tensor, max_delay_ms: float = 500.0):
    """Echo / slap-back / comb resonator: a delay line that feeds its own output back through a one-pole low-pass (the damping), mixed
    with the dry signal. x (bs, chs, seq_len); delay_ms, feedback, damping_hz and mix hold bs values each. For item b, every channel and
    sample n, with the line empty (zero) before sample 0:
        D = clamp(sample_rate/1000 delay_ms, 2, sample_rate/1000 max_delay_ms);  i = floor(D), f = D - i
        a = exp(-2 pi max(damping_hz, 0) / sample_rate)                          (damping_hz = inf: a = 0, no filter in the loop)
        r[n] = Catmull-Rom interpolation of v[n-i+1], v[n-i], v[n-i-1], v[n-i-2] at f              (the line read D samples back)
        w[n] = x[n] + feedback r[n];   v[n] = (1 - a) w[n] + a v[n-1];   y[n] = (1 - mix) x[n] + mix r[n]
    An echo is 100-500 ms with feedback 0.3-0.7; a slap-back 60-120 ms with little feedback; a comb resonator a few ms with feedback
    near +-1. The delay is at least two samples (the interpolation's footprint must lie in the past). feedback is not clamped: for
    |feedback| >= 1 the output grows, which is the caller's business; below 1 the loop is stable. D and a are float64 in the kernel,
    everything after them float32 (csrc/fbdelay.hip). The op works on whole tensors, not on a stream.
    Differentiable in x and in all four controls. The delay_ms gradient is zero where D was clamped - size max_delay_ms (a plain float;
    at most dasp_fbdelay_max_delay_samples() = 34816 samples, 789 ms at 44.1 kHz) so that delay_ms stays inside it; the damping_hz gradient
    is zero where damping_hz < 0 and at inf. A NaN delay_ms makes its item NaN (an infinite one is clamped like any other).
    One workgroup walks one (item, channel) row in steps shorter than the delay: the op cannot fill the chip at training batch sizes,
    and delays of a few samples are slow.
    Out of scope: an LFO on the fed-back delay (modulated_delay has one, without feedback), cross-channel (ping-pong) feedback, and
    float64. A wrong control count raises RuntimeError naming the control; a bad sample_rate or max_delay_ms (sample_rate/1000
    max_delay_ms below two samples included) ValueError; a max_delay_ms beyond the maximum DaspHipError (unsupported configuration)."""
    bs, chs, seq_len = x.size()
    for name, c in (("delay_ms", delay_ms), ("feedback", feedback), ("damping_hz", damping_hz), ("mix", mix)):
        if c.numel() != bs:
            raise RuntimeError(f"{name}: shape '[{bs}]' is invalid for input of size {c.numel()}")
    sr, max_delay_ms = float(sample_rate), float(max_delay_ms)
    if not (sr > 0.0 and sr != float("inf")) or not (max_delay_ms != float("inf") and sr / 1000.0 * max_delay_ms >= 2.0):
        raise ValueError(f"feedback_delay: finite sample_rate > 0 and finite max_delay_ms of at least two samples, got {sample_rate}, {max_delay_ms}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "feedback_delay")
    H = math.ceil(sr / 1000.0 * max_delay_ms)
    return FeedbackDelayFunction.apply(x, delay_ms, feedback, damping_hz, mix, sr, max_delay_ms, H)


def fdn_reverb(x: torch.Tensor, sample_rate: float, decay_s: torch.Tensor, damping_hz: torch.Tensor, mix: torch.Tensor, delays,
               decorrelate: bool = True):
    """Feedback delay network reverb: K delay lines coupled through the Householder matrix I - (2/K) 1 1^T, each fed through a one-pole
    low-pass (the damping), mixed with the dry signal. x (bs, chs, seq_len); decay_s, damping_hz and mix hold bs values each; delays is a
    plain sequence of K ints, the line lengths m_k in samples (1 <= K <= 16, every m_k >= 1, repeats allowed; signal.fdn_delay_lengths
    gives a sensible set), shared by the batch; decorrelate a plain bool. For item b, channel c and sample n, with every line empty
    (zero) before sample 0:
        T = clamp(decay_s, 0.01, 100);  g_k = 10^(-3 m_k / (sample_rate T))      (the low-frequency tail falls by 60 dB in T seconds)
        a = exp(-2 pi max(damping_hz, 0) / sample_rate)                          (damping_hz = inf: a = 0, no filter in the loop)
        r_k[n] = v_k[n - m_k];   u_k[n] = g_k r_k[n];   w_k[n] = x[n] + u_k[n] - (2/K) sum_j u_j[n];   v_k[n] = (1 - a) w_k[n] + a v_k[n-1]
        wet[n] = K^(-1/2) sum_k s_ck r_k[n],  s_ck = (-1)^(k c) if decorrelate else 1;   y[n] = (1 - mix) x[n] + mix wet[n]
    Every g_k < 1, the matrix is orthogonal and the one-pole's gain is at most 1: the loop is stable for every finite input. With
    decorrelate the odd channels sum the lines with alternating signs, so that a stereo pair gets two different tails from one set of
    lines; channel 0 is the same with and without it. g_k and a are float64 in the kernel and rounded once, everything after them
    float32 (csrc/fdn.hip). The op works on whole tensors, not on a stream.
    Differentiable in x, decay_s, damping_hz and mix, once (no double backward). The decay_s gradient is zero where decay_s was clamped,
    the damping_hz gradient zero where damping_hz < 0 and at inf. A NaN control makes its own item NaN, gradients included, and no other.
    One workgroup walks one (item, channel) row in steps of min(shortest line, 1024) samples with all K rings in LDS: the op cannot fill
    the chip at training batch sizes, short lines are slow, and sum(delays) is at most 38912 - 1024 (K + 1) samples (29696 at K = 8:
    0.67 s at 44.1 kHz; 21504 at K = 16). A gradient for a control keeps the K line signals: 4 K bytes per sample.
    Out of scope: fractional or modulated line lengths, learnable or non-Householder matrices, per-line absorption filters matched to
    the line length (a frequency-dependent RT60 target), per-line input and output gains, an early-reflection section, checkpointing
    instead of the saved line signals, several rows per workgroup for short lines, float64, and a torch.ops.dasp op.
    A wrong control count raises RuntimeError naming the control; delays that are not 1 - 16 ints >= 1 (bools refused) or a sample_rate
    that is not positive and finite ValueError, before anything touches the device; delays beyond the sum limit DaspHipError
    (unsupported configuration)."""
    bs, chs, seq_len = x.size()
    for name, c in (("decay_s", decay_s), ("damping_hz", damping_hz), ("mix", mix)):
        if c.numel() != bs:
            raise RuntimeError(f"{name}: shape '[{bs}]' is invalid for input of size {c.numel()}")
    try:
        sr = float(sample_rate)
    except (TypeError, ValueError):
        sr = float("nan")
    if not (sr > 0.0 and sr != float("inf")):
        raise ValueError(f"fdn_reverb: finite sample_rate > 0, got {sample_rate}")
    lines = _signal.check_fdn_delays(delays)
    _lib.require_device(x, "x")
    require_fp32_ok(x, "fdn_reverb")
    return FdnReverbFunction.apply(x, decay_s, damping_hz, mix, sr, lines, bool(decorrelate))


LIMITER_MAX_LOOKAHEAD = 1024          # samples: dasp_limiter_max_lookahead() (csrc/limiter.hip), checked here before the device is touched


def limiter_lookahead(sample_rate: float, lookahead_ms: float) -> int:
    """The look-ahead of `limiter` in samples, L = round(sample_rate * lookahead_ms / 1000), after the checks of its arguments."""
    try:
        sr, ms = float(sample_rate), float(lookahead_ms)
    except (TypeError, ValueError):
        sr = ms = float("nan")
    if not (sr > 0.0 and sr != float("inf")):
        raise ValueError(f"limiter: finite sample_rate > 0, got {sample_rate}")
    if not (ms >= 0.0 and ms != float("inf")):
        raise ValueError(f"limiter: finite lookahead_ms >= 0, got {lookahead_ms}")
    L = round(sr * ms / 1000.0)
    if L > LIMITER_MAX_LOOKAHEAD:
        raise ValueError(f"limiter: a look-ahead of {L} samples ({lookahead_ms} ms at {sample_rate} Hz) is above the maximum of {LIMITER_MAX_LOOKAHEAD}")
    return int(L)


def limiter(x: torch.Tensor, sample_rate: float, threshold_db: torch.Tensor, release_ms: torch.Tensor, lookahead_ms: float = 5.0,
            eps: float = 1e-8):
    """Look-ahead brickwall limiter with linked channels: the op that guarantees a ceiling. x (bs, chs, seq_len); threshold_db and
    release_ms hold bs values each; lookahead_ms and eps are plain floats. y has the shape of x and is aligned with it: the op works on
    whole tensors and looks into the future, there is no latency. For item b, with N = seq_len and an internal timeline m in
    [0, N + L); everything before 0 and the level from N on are zero:
        L   = round(sample_rate * lookahead_ms / 1000)          0 <= L <= 1024
        thr = clamp(threshold_db, -120, 40);  t = clamp(release_ms, 0.1, 10000)
        rho = exp(-ln 9 / (sample_rate * t / 1000))             (the compressor's 10-90 % constant)
        p[m] = max_c |x[b,c,m]|                                 (channels linked; the lowest channel wins a tie)
        r[m] = max(0, 20 log10(max(p[m], eps)) - thr)           (required reduction in dB; 0 for m >= N)
        h[m] = max_{0<=k<=L} r[m-k]                             (hold; the latest sample wins a tie)
        e[m] = max(h[m], rho * e[m-1])                          (release; h wins a tie) = max_j rho^max(0, m-j-L) * r[j]
        s[m] = (1/(L+1)) * sum_{j=0..L} e[m-j]                  (attack: a box of the look-ahead's length, in dB)
        G[m] = 10^(-s[m]/20);     y[b,c,n] = x[b,c,n] * G[n+L]
    Each e[n+L-j], 0 <= j <= L, is at least r[n], so |y| <= 10^(thr/20) at every sample (to the rounding of r, G and the product: a
    few 1e-7 of the ceiling); an item that stays below its threshold comes back bit for bit. The release is linear in dB: the
    reduction falls to a ninth in release_ms. r, the powers of rho, the box and G are float64 in the kernel and rounded once, e is
    float32 (it underflows to 0 after about 87 / |ln rho| samples of release) (csrc/limiter.hip).
    Differentiable in x, threshold_db and release_ms, once (no double backward), by a hand-derived adjoint that follows the winning
    sample of every e[m]; both control gradients are exactly zero where the control was clamped. No atomics: every result is
    bit-identical run to run and for an item alone or inside a batch. A gradient keeps G and the winners, 8 bytes per sample of an
    item; nothing is kept without one. A NaN control makes its own item NaN, gradients included; a NaN or inf sample stays in its item.
    One workgroup walks one item tile by tile: bs items use bs compute units.
    Out of scope: true-peak (oversampled) detection, input gain and makeup gain (compose `gain`), unlinked channels, a soft knee,
    program-dependent release, streaming state, float64, a torch.ops.dasp registration and a chain.py entry.
    A wrong control count raises RuntimeError naming the control; a sample_rate that is not positive and finite, a lookahead_ms that
    is negative or not finite, a look-ahead beyond 1024 samples or an eps that is negative or not finite ValueError, before anything
    touches the device."""
    bs, chs, seq_len = x.size()
    for name, c in (("threshold_db", threshold_db), ("release_ms", release_ms)):
        if c.numel() != bs:
            raise RuntimeError(f"{name}: shape '[{bs}]' is invalid for input of size {c.numel()}")
    L = limiter_lookahead(sample_rate, lookahead_ms)
    e = float(eps)
    if not (e >= 0.0 and e != float("inf")):
        raise ValueError(f"limiter: finite eps >= 0, got {eps}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "limiter")
    return LimiterFunction.apply(x, threshold_db, release_ms, float(sample_rate), L, e)


def phaser(x: torch.Tensor, sample_rate: float, rate_hz: torch.Tensor, center_hz: torch.Tensor, depth: torch.Tensor, phase: torch.Tensor,
           mix: torch.Tensor, stages: int = 4, stereo_spread: float = 0.25):
    """Phaser: `stages` first-order all-pass sections in series whose shared break frequency a sine LFO sweeps, mixed with the dry
    signal. x (bs, chs, seq_len); rate_hz, center_hz, depth, phase and mix hold bs values each. phase and stereo_spread are in turns,
    depth in octaves (the conventions of modulated_delay); stages is a plain int K, 1 <= K <= 12, stereo_spread a plain float. For item
    b, channel c and sample n, with every state zero before sample 0:
        theta = 2 pi (rate_hz n / sample_rate + phase + c stereo_spread)
        f[n] = clamp(center_hz 2^(depth sin theta), sample_rate/4096, 0.49 sample_rate)
        t = tan(pi f / sample_rate);   a[n] = (t - 1) / (t + 1)                                        (|a| < 1 by the clamp)
        s_0 = x;   s_k[n] = a[n] (s_{k-1}[n] - s_k[n-1]) + s_{k-1}[n-1],  k = 1..K                      (all stages share a[n])
        y[n] = (1 - mix) x[n] + mix s_K[n]
    mix = 0.5 gives the classic notches, K / 2 of them; mix = 1 is the pure all-pass, a vibrato-like phase wobble. The LFO's phase is
    float64 in the kernel and reduced to a turn before it is rounded; everything after it is float32 (csrc/phaser.hip). The op works on
    whole tensors, not on a stream.
    Differentiable in x and in all five controls. The gradients of rate_hz, center_hz, depth and phase take no contribution from samples
    where f was clamped. A NaN control makes its own item NaN and no other.
    One workgroup walks one (item, channel) row tile by tile: the op cannot fill the chip at training batch sizes.
    Out of scope: a feedback ("resonance") path around the cascade - it couples the K stages into one (K+1)-dimensional time-varying
    system whose scan composes (K+1) x (K+1) matrices instead of scalar pairs -, per-stage break frequencies, LFO shapes other than
    sine, and float64. A wrong control count raises RuntimeError naming the control; a sample_rate that is not positive and finite, a
    non-finite stereo_spread or stages outside 1..12 ValueError, before anything touches the device."""
    bs, chs, seq_len = x.size()
    for name, c in (("rate_hz", rate_hz), ("center_hz", center_hz), ("depth", depth), ("phase", phase), ("mix", mix)):
        if c.numel() != bs:
            raise RuntimeError(f"{name}: shape '[{bs}]' is invalid for input of size {c.numel()}")
    sr, spread = float(sample_rate), float(stereo_spread)
    if not (sr > 0.0 and sr != float("inf")) or spread - spread != 0.0:
        raise ValueError(f"phaser: finite sample_rate > 0 and finite stereo_spread, got {sample_rate}, {stereo_spread}")
    if isinstance(stages, bool) or int(stages) != stages or not 1 <= stages <= 12:
        raise ValueError(f"phaser: stages must be an integer from 1 to 12, got {stages}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "phaser")
    return PhaserFunction.apply(x, rate_hz, center_hz, depth, phase, mix, sr, int(stages), spread)


def time_varying_filter(x: torch.Tensor, sample_rate: float, cutoff_hz: torch.Tensor, q: torch.Tensor, mix: torch.Tensor, hop: int = 64,
                        mode: str = "lowpass"):
    """Resonant filter whose cutoff and resonance follow control curves: Simper's trapezoidal (TPT) state-variable filter, the published
    Cytomic form, which stays well-behaved when its coefficients move every sample - wah, filter sweeps, the synth low-pass, automation
    of an EQ band. x (bs, chs, seq_len); cutoff_hz and q (bs, F) with F = signal.control_frames(seq_len, hop) = ceil(seq_len / hop) + 1,
    frame point j at sample j hop, shared by an item's channels; mix holds bs values. hop is a plain int, a power of two from 8 to 2048;
    mode one of "lowpass", "bandpass", "highpass", "notch". For item b, every channel and sample n, with both states zero before sample 0:
        G_j = tan(pi clamp(cutoff_hz[b,j], sample_rate/4096, 0.49 sample_rate) / sample_rate);   K_j = 1 / clamp(q[b,j], 0.1, 100)
        j = n // hop;   t = (n mod hop) / hop;   g = G_j + t (G_{j+1} - G_j);   k = K_j + t (K_{j+1} - K_j)
        a1 = 1 / (1 + g (g + k));   a2 = g a1;   a3 = g a2
        v3 = x[n] - ic2;   v1 = a1 ic1 + a2 v3;   v2 = ic2 + a2 ic1 + a3 v3;   ic1 <- 2 v1 - ic1;   ic2 <- 2 v2 - ic2
        w = v2 (lowpass) | k v1 (bandpass, 0 dB at the centre) | x - k v1 - v2 (highpass) | x - k v1 (notch)
        y[n] = (1 - mix) x[n] + mix w
    What is interpolated is G and K, not Hz: the frame points are taken in float64 in the kernel and rounded once, everything after them
    is float32 (csrc/tvfilter.hip). With constant curves the outputs are the RBJ low-pass, high-pass and constant-peak band-pass biquads
    at the same frequency and Q. The op works on whole tensors, not on a stream.
    Differentiable in x, cutoff_hz, q and mix, every frame value included. The gradient of a frame value that was clamped is exactly
    zero. The clamps are comparisons, which a NaN passes: a NaN frame value j makes its item NaN from sample (j - 1) hop on and leaves
    earlier samples and other items alone.
    One workgroup walks one (item, channel) row tile by tile: the op cannot fill the chip at training batch sizes.
    Out of scope: an envelope follower inside the op (compose `envelope_follower`, whose output is a curve for it), per-channel curves, cascaded sections or a morphing mode
    mix, look-back segments for few rows, float64, and a torch.ops.dasp registration. A wrong frame count raises RuntimeError naming the
    control and the expected F; a hop that is no power of two from 8 to 2048, an unknown mode or a sample_rate that is not positive and
    finite ValueError, before anything touches the device."""
    bs, chs, seq_len = x.size()
    sr = float(sample_rate)
    if not (sr > 0.0 and sr != float("inf")):
        raise ValueError(f"time_varying_filter: finite sample_rate > 0, got {sample_rate}")
    if mode not in TVFILTER_MODES:
        raise ValueError(f"time_varying_filter: mode must be one of {', '.join(TVFILTER_MODES)}, got {mode!r}")
    try:
        frames = _signal.control_frames(seq_len, hop)
    except ValueError as e:
        raise ValueError(f"time_varying_filter: {e}") from None
    for name, c in (("cutoff_hz", cutoff_hz), ("q", q)):
        if c.dim() != 2 or tuple(c.shape) != (bs, frames):
            raise RuntimeError(f"{name}: expected shape [{bs}, {frames}] (F = ceil({seq_len} / {hop}) + 1 = {frames} frame points), got {list(c.shape)}")
    if mix.numel() != bs:
        raise RuntimeError(f"mix: shape '[{bs}]' is invalid for input of size {mix.numel()}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "time_varying_filter")
    return TimeVaryingFilterFunction.apply(x, cutoff_hz, q, mix, sr, int(hop), TVFILTER_MODES.index(mode))


def time_varying_eq(x: torch.Tensor, sample_rate: float, gain_db: torch.Tensor, cutoff_hz: torch.Tensor, q: torch.Tensor, hop: int = 64,
                    mode: str = "bell"):
    """One EQ band whose gain, frequency and Q follow control curves: a bell, low shelf or high shelf from Simper's trapezoidal
    state-variable filter, the recurrence of `time_varying_filter` - the de-esser, the dynamic EQ, a band of a multiband compressor, EQ
    automation, a tilt driven by level. x (bs, chs, seq_len); gain_db, cutoff_hz and q (bs, F) with F = signal.control_frames(seq_len,
    hop), frame point j at sample j hop, shared by an item's channels - the convention of time_varying_filter, gain_curve and
    envelope_follower, so a curve from any of them fits. hop is a plain int, a power of two from 8 to 2048; mode one of "bell",
    "lowshelf", "highshelf". There is no mix: the gain is the amount. For item b, every channel and sample n, with both states zero
    before sample 0:
        A_j = 10^(clamp(gain_db[b,j], -40, 40) / 40);   T_j = tan(pi clamp(cutoff_hz[b,j], sample_rate/4096, 0.49 sample_rate) / sample_rate)
        Qc = clamp(q[b,j], 0.1, 100)
        bell: G_j = T_j, K_j = 1 / (Qc A_j)    lowshelf: G_j = T_j / sqrt A_j, K_j = 1 / Qc    highshelf: G_j = T_j sqrt A_j, K_j = 1 / Qc
        j = n // hop;   t = (n mod hop) / hop;   g = G_j + t (G_{j+1} - G_j);   likewise k from K and A from A_j
        a1 = 1 / (1 + g (g + k));   a2 = g a1;   a3 = g a2
        v3 = x[n] - ic2;   v1 = a1 ic1 + a2 v3;   v2 = ic2 + a2 ic1 + a3 v3;   ic1 <- 2 v1 - ic1;   ic2 <- 2 v2 - ic2
        bell:       y[n] = x[n] + k (A^2 - 1) v1
        lowshelf:   y[n] = x[n] + k (A - 1) v1 + (A^2 - 1) v2
        highshelf:  y[n] = A^2 x[n] + k (1 - A) A v1 + (1 - A^2) v2
    What is interpolated is G, K and A, not Hz or dB: the frame points are taken in float64 in the kernel and rounded once, everything
    after them is float32 (csrc/tveq.hip). With constant curves the result is the RBJ peaking, low-shelf and high-shelf biquad of
    signal.biquad at the same frequency, Q and gain - the sections parametric_eq is built from. An all-zero gain_db returns x bit for
    bit and hands the upstream gradient to x bit for bit, while the gradient of gain_db is generally not zero there.
    Differentiable once in x, gain_db, cutoff_hz and q, every frame value included. The gradient of a frame value that was clamped is
    exactly zero. No atomics: every result is bit-identical run to run and for an item alone or in a batch. The clamps are comparisons,
    which a NaN passes: a NaN frame value j of any curve makes its item NaN from sample (j - 1) hop on and leaves earlier samples and
    other items alone. Half and bfloat16 are converted, float64 is refused.
    One workgroup walks one (item, channel) row tile by tile: the op cannot fill the chip at training batch sizes.
    Out of scope: several bands in one kernel (the follow-up, in the manner of phaser's stages), per-channel curves, a side chain inside
    the op (compose time_varying_filter and envelope_follower), look-back segments for few rows, float64, and double backward, which is
    refused as for the siblings. A wrong frame count raises RuntimeError naming the curve and the expected F; a hop that is no power of
    two from 8 to 2048, an unknown mode or a sample_rate that is not positive and finite ValueError, before anything touches the
    device."""
    bs, chs, seq_len = x.size()
    try:
        sr = float(sample_rate)
    except (TypeError, ValueError):
        sr = float("nan")
    if not (sr > 0.0 and sr != float("inf")):
        raise ValueError(f"time_varying_eq: finite sample_rate > 0, got {sample_rate}")
    if mode not in TVEQ_MODES:
        raise ValueError(f"time_varying_eq: mode must be one of {', '.join(TVEQ_MODES)}, got {mode!r}")
    try:
        frames = _signal.control_frames(seq_len, hop)
    except ValueError as e:
        raise ValueError(f"time_varying_eq: {e}") from None
    for name, c in (("gain_db", gain_db), ("cutoff_hz", cutoff_hz), ("q", q)):
        if c.dim() != 2 or tuple(c.shape) != (bs, frames):
            raise RuntimeError(f"{name}: expected shape [{bs}, {frames}] (F = ceil({seq_len} / {hop}) + 1 = {frames} frame points), got {list(c.shape)}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "time_varying_eq")
    return TimeVaryingEQFunction.apply(x, gain_db, cutoff_hz, q, sr, int(hop), TVEQ_MODES.index(mode))


def envelope_follower(x: torch.Tensor, sample_rate: float, smoothing_ms: torch.Tensor, hop: int = 64, detector: str = "peak"):
    """Envelope follower: a control curve from a signal. x (bs, chs, seq_len); smoothing_ms holds bs values; hop is a plain int, a power
    of two from 8 to 2048; detector "peak" or "power". Returns E (bs, F), F = signal.control_frames(seq_len, hop), frame point j at
    sample j hop - the convention of time_varying_filter and gain_curve, so E is directly a curve for them. For item b, with the level
    zero from sample seq_len on and e[-1] = 0:
        t = clamp(smoothing_ms, 0.1, 10000);   a = exp(-ln 9 / (sample_rate t / 1000))          (the compressor's 10-90 % constant)
        p[m] = max_c |x[b,c,m]|   ("peak": channels linked, the lowest channel wins a tie)   |   mean_c x[b,c,m]^2   ("power")
        e[m] = a e[m-1] + (1 - a) p[m]                                                          (unit DC gain)
        E[b,j] = e[j hop],  j = 0 .. F-1                                  ((F-1) hop >= seq_len: the last points see the decay)
    The output is linear - amplitude for "peak", mean square for "power": dB, square roots, thresholds and ratios are the caller's torch
    code on (bs, F), so the op has no eps and no singular gradient. The recurrence is not walked: a is constant per item, so
    E_j = a^hop E_{j-1} + z_j with z_j a weighted sum over hop samples; the sums are float32 with weights from float64 (rounded once),
    over independent tiles that fill the chip at any batch size, and the frame-rate recurrence is float64 (csrc/envelope.hip).
    Differentiable once in x and smoothing_ms: "peak" sends sign(x) to the winning channel (sign(0) = 0), "power" 2 x / chs to every
    channel; the gradient of smoothing_ms is exactly zero where it was clamped. Nothing per sample is saved: x, the control and, when
    the control needs a gradient, dE/da (bs, F). No atomics: every result is bit-identical run to run and for an item alone or in a
    batch. A NaN smoothing_ms makes its own item NaN and no other; a NaN or inf sample at m0 reaches the frame points j hop >= m0 of
    its item and nothing else. Half and bfloat16 are converted, float64 is refused; seq_len = 0 returns the (bs, 1) zero curve.
    Out of scope: separate attack and release, unlinked channels, per-sample output, float64, a torch.ops.dasp registration and a
    chain.py entry. A wrong control count raises RuntimeError naming the control; a hop that is no power of two from 8 to 2048, an
    unknown detector or a sample_rate that is not positive and finite ValueError, before anything touches the device."""
    bs, chs, seq_len = x.size()
    if smoothing_ms.numel() != bs:
        raise RuntimeError(f"smoothing_ms: shape '[{bs}]' is invalid for input of size {smoothing_ms.numel()}")
    try:
        sr = float(sample_rate)
    except (TypeError, ValueError):
        sr = float("nan")
    if not (sr > 0.0 and sr != float("inf")):
        raise ValueError(f"envelope_follower: finite sample_rate > 0, got {sample_rate}")
    if detector not in ENVELOPE_DETECTORS:
        raise ValueError(f"envelope_follower: detector must be one of {', '.join(ENVELOPE_DETECTORS)}, got {detector!r}")
    try:
        _signal.control_frames(seq_len, hop)
    except ValueError as e:
        raise ValueError(f"envelope_follower: {e}") from None
    _lib.require_device(x, "x")
    require_fp32_ok(x, "envelope_follower")
    return EnvelopeFollowerFunction.apply(x, smoothing_ms, sr, int(hop), ENVELOPE_DETECTORS.index(detector))


def gain_curve(x: torch.Tensor, sample_rate: float, gain_db: torch.Tensor, hop: int = 64):
    """Gain that follows a control curve: fader automation, fades, tremolo, ducking. x (bs, chs, seq_len); gain_db (bs, F) with
    F = signal.control_frames(seq_len, hop), frame point j at sample j hop, shared by an item's channels; hop is a plain int, a power of
    two from 8 to 2048; sample_rate is not used (the signature of `gain`). For item b, every channel and sample n, with P = gain_db[b]:
        j = n // hop;   t = (n mod hop) / hop;   g[n] = P_j + t (P_{j+1} - P_j)                 (interpolated in dB, float32)
        y[b,c,n] = x[b,c,n] 10^(g[n] / 20)
    An all-zero curve returns x bit for bit. Differentiable once in x and in every frame value: frame point j takes (1 - t) of its own
    interval and t of the one before it, summed over the channels in a fixed order - no atomics, every result bit-identical run to run
    and for an item alone or in a batch (csrc/envelope.hip). At t = 0 the gain is P_j itself: a NaN frame value j reaches the samples
    (j - 1) hop < n < (j + 1) hop of its item only, in y and in both gradients. Frame values are expected finite; +-inf is not a mute.
    Half and bfloat16 are converted, float64 is refused.
    A wrong frame count raises RuntimeError naming gain_db and the expected F; a hop that is no power of two from 8 to 2048 ValueError,
    before anything touches the device."""
    bs, chs, seq_len = x.size()
    try:
        frames = _signal.control_frames(seq_len, hop)
    except ValueError as e:
        raise ValueError(f"gain_curve: {e}") from None
    if gain_db.dim() != 2 or tuple(gain_db.shape) != (bs, frames):
        raise RuntimeError(f"gain_db: expected shape [{bs}, {frames}] (F = ceil({seq_len} / {hop}) + 1 = {frames} frame points), got {list(gain_db.shape)}")
    _lib.require_device(x, "x")
    require_fp32_ok(x, "gain_curve")
    return GainCurveFunction.apply(x, gain_db, float(sample_rate), int(hop))


def _finite_rate(sample_rate, who):
    try:
        sr = float(sample_rate)
    except (TypeError, ValueError):
        sr = float("nan")
    if not (sr > 0.0 and sr != float("inf")):
        raise ValueError(f"{who}: finite sample_rate > 0, got {sample_rate}")
    return sr


def block_level(x: torch.Tensor, sample_rate: float, hop: int = 64, detector: str = "peak"):
    """Block detector: the peak or the mean square of every hop, as a control curve. x (bs, chs, seq_len); hop is a plain int, a power
    of two from 8 to 2048; detector "peak" or "power"; sample_rate is not used (the common signature of the control-rate layer).
    Returns L (bs, F), F = signal.control_frames(seq_len, hop), frame point j at sample j hop. With the level of envelope_follower,
        p[m] = max_c |x[b,c,m]|   ("peak": the lowest channel wins a tie, a NaN channel makes p NaN)   |   mean_c x[b,c,m]^2   ("power")
    and p = 0 from sample seq_len on:
        L[b,0] = p[0];   L[b,j] = max_{i=1..hop} p[(j-1) hop + i]   |   (1 / hop) sum_{i=1..hop} p[(j-1) hop + i],   j = 1 .. F-1
    Unlike a fast envelope_follower read at the frame points, it misses no peak between them. "peak" is exact: the earliest sample of
    a block that holds the maximum wins, on its lowest winning channel, and the first NaN sample of a block wins it, so a NaN sample
    m0 reaches frame ceil(m0 / hop) of its item and nothing else. "power" sums in float32 in one fixed order: runs of 8 samples in time
    order, the runs of a block as a balanced tree, then the division by hop - always by hop, also where the signal ends inside the
    block. Differentiable once in x: "peak" sends sign(x) gL_j to the winner (sign(0) = 0) and writes zero everywhere else, "power"
    2 x / (chs hop) gL_j, and 2 x / chs gL_0 for sample 0. "peak" saves the winners, one int32 per frame, and not x - its backward
    pass only writes; "power" saves x. Independent tiles of 4096 samples fill the chip at any batch size; no atomics: every result
    is bit-identical run to run and for an item alone or in a batch (csrc/ballistics.hip). Half and bfloat16 are converted, float64 is
    refused; seq_len = 0 returns the (bs, 1) zero curve.
    Out of scope: unlinked channels, float64, a torch.ops.dasp registration and a chain.py entry. A hop that is no power of two from 8
    to 2048 or an unknown detector raises ValueError before anything touches the device."""
    bs, chs, seq_len = x.size()
    if detector not in ENVELOPE_DETECTORS:
        raise ValueError(f"block_level: detector must be one of {', '.join(ENVELOPE_DETECTORS)}, got {detector!r}")
    try:
        _signal.control_frames(seq_len, hop)
    except ValueError as e:
        raise ValueError(f"block_level: {e}") from None
    _lib.require_device(x, "x")
    require_fp32_ok(x, "block_level")
    return BlockLevelFunction.apply(x, int(hop), ENVELOPE_DETECTORS.index(detector))


def ballistics(curve: torch.Tensor, sample_rate: float, attack_ms: torch.Tensor, release_ms: torch.Tensor, hop: int = 64):
    """Attack / release ballistics at the control rate: the classic branching one-pole smoother on a curve. curve P (bs, F) with any
    F >= 1 - it is not tied to a signal length; attack_ms and release_ms hold bs values each; hop, a plain int and a power of two
    from 8 to 2048, is the distance of the frame points in samples. Returns E (bs, F). For item b, with E_{-1} = 0:
        t_a = clamp(attack_ms, 0.1, 10000);   c_a = -expm1(-ln 9 hop / (sample_rate t_a / 1000));   c_r likewise from release_ms
        up_j = P_j > E_{j-1};   c_j = c_a if up_j else c_r;   E_j = E_{j-1} + c_j (P_j - E_{j-1})
    so the 10 - 90 % rise and fall times of a step are attack_ms and release_ms (to within a hop). A tie takes the release branch;
    a NaN P_j compares false, takes the release branch and makes E NaN from j on in its item only; a NaN control makes its own item
    NaN and no other. With attack_ms == release_ms it is the linear one-pole. The constants are float64 from the float32 controls,
    the recurrence is float64 and E is rounded once to float32. The recurrence is walked, not scanned: a composition of these
    max-of-affine maps has no fixed-size form. One wave per item walks the F values, which is affordable at the frame rate and would
    not be at the sample rate (csrc/ballistics.hip).
    Differentiable once in the curve and both times. The branch mask is saved as the forward pass decided it - the gradient is
    discontinuous across the branches - with P, the controls and E:
        Lambda_j = gE_j + (1 - c_{j+1}) Lambda_{j+1};   gP_j = c_j Lambda_j
        g_attack = (dc_a/dt_a) sum_{j: up_j} Lambda_j (P_j - E_{j-1});   g_release likewise over the other frames
    in float64 in one fixed order; a control gradient is exactly zero where its control was clamped. No atomics: every result is
    bit-identical run to run and for an item alone or in a batch. Half and bfloat16 are converted, float64 is refused.
    Out of scope: sample-rate (per-sample) ballistics, a hold time, float64, a torch.ops.dasp registration and a chain.py entry;
    compressor and expander keep ignoring release_ms. A wrong control count raises RuntimeError naming the control; a hop that is no
    power of two from 8 to 2048 or a sample_rate that is not positive and finite ValueError, before any launch."""
    if curve.dim() != 2 or curve.shape[1] < 1:
        raise RuntimeError(f"curve: expected shape [bs, F] with F >= 1, got {list(curve.shape)}")
    bs = curve.shape[0]
    for name, c in (("attack_ms", attack_ms), ("release_ms", release_ms)):
        if c.numel() != bs:
            raise RuntimeError(f"{name}: shape '[{bs}]' is invalid for input of size {c.numel()}")
    sr = _finite_rate(sample_rate, "ballistics")
    try:
        _signal.control_frames(0, hop)
    except ValueError as e:
        raise ValueError(f"ballistics: {e}") from None
    _lib.require_device(curve, "curve")
    require_fp32_ok(curve, "ballistics")
    return BallisticsFunction.apply(curve, attack_ms, release_ms, sr, int(hop))


def _soft_knee_level(l_db, threshold_db, ratio, knee_db):
    """The static curve of `compressor` on levels in dB (Giannoulis, Massberg & Reiss 2012): the level itself below the knee, the
    quadratic blend inside it, threshold + (level - threshold) / ratio above. The controls broadcast against l_db. The knee's division
    is by a width made safe where knee_db == 0 - a branch that is then never taken - so every gradient is finite."""
    half = 0.5 * knee_db
    over = l_db - threshold_db
    wide = torch.where(knee_db > 0, knee_db, torch.ones_like(knee_db))
    knee = l_db + (1.0 / ratio - 1.0) * (over + half) ** 2 / (2.0 * wide)
    above = threshold_db + over / ratio
    in_knee = (knee_db > 0) & (over >= -half) & (over <= half)
    return torch.where(over > half, above, torch.where(in_knee, knee, l_db))


def sidechain_compressor(x: torch.Tensor, sample_rate: float, threshold_db: torch.Tensor, ratio: torch.Tensor, attack_ms: torch.Tensor,
                         release_ms: torch.Tensor, knee_db: torch.Tensor, makeup_gain_db: torch.Tensor, key: torch.Tensor = None, hop: int = 64,
                         eps: float = 1e-5):
    """Feed-forward compressor at the control rate whose release_ms is real, keyed by x itself or by another signal. Plain torch on
    (bs, F) around three fused ops:
        L = block_level(key if key is not None else x, sample_rate, hop, "peak")          (the peak of every hop, channels linked)
        l_db = 20 log10(L + eps)
        g_db = the soft-knee static curve of `compressor` on l_db                         (Giannoulis, Massberg & Reiss 2012)
        r = l_db - g_db                                                                   (the gain reduction, >= 0 dB)
        r_s = ballistics(r, sample_rate, attack_ms, release_ms, hop)                      (reduction rises with attack, falls with release)
        y = gain_curve(x, sample_rate, makeup_gain_db[:, None] - r_s, hop)
    x (bs, chs, seq_len); key (bs, chs_k, seq_len) of the same seq_len, any channel count; the six controls hold bs values each; hop is
    a plain int, a power of two from 8 to 2048. Differentiable in x, key and all six controls; the differentiability of the static curve
    is torch's, and knee_db == 0 gives finite gradients, as `compressor`'s stated deviation does. With a key, the gradient of x flows
    through the gain alone. Out of scope: sample-rate ballistics (the gain moves at frame points and is interpolated between them),
    hold time and look-ahead for the side chain, unlinked channels, float64, a torch.ops.dasp registration and a chain.py entry;
    `compressor` and `expander` are unchanged and keep ignoring release_ms."""
    bs, chs, seq_len = x.size()
    ctls = dict(threshold_db=threshold_db, ratio=ratio, attack_ms=attack_ms, release_ms=release_ms, knee_db=knee_db, makeup_gain_db=makeup_gain_db)
    for name, c in ctls.items():
        if c.numel() != bs:
            raise RuntimeError(f"{name}: shape '[{bs}]' is invalid for input of size {c.numel()}")
    side = x if key is None else key
    if side.dim() != 3 or side.shape[0] != bs or side.shape[2] != seq_len:
        raise RuntimeError(f"key: expected shape [{bs}, chs_k, {seq_len}], got {list(side.shape)}")
    _finite_rate(sample_rate, "sidechain_compressor")
    L = block_level(side, sample_rate, hop, "peak")
    col = lambda c: c.reshape(bs, 1).to(device=L.device, dtype=L.dtype)
    l_db = 20.0 * torch.log10(L + eps)
    r = l_db - _soft_knee_level(l_db, col(threshold_db), col(ratio), col(knee_db))
    r_s = ballistics(r, sample_rate, attack_ms, release_ms, hop)
    return gain_curve(x, sample_rate, col(makeup_gain_db) - r_s, hop)


def resample(x: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta: float = None):
    """Sample-rate conversion by a polyphase windowed sinc: torchaudio.functional.resample's signature and published algorithm, restated
    (torchaudio itself is not a dependency). x (..., N), time last, every leading dimension a row; returns
    (..., ceil(n N / o)) with o : n the rates divided by their gcd - (44100, 48000) and (147, 160) give the same bits. Equal rates
    return x itself. With h, width = signal.resample_taps(...) rounded once to float32 and x zero outside [0, N):
        y[q n + r] = sum_k h[r][k] x[q o + k - width]
    in float32, one fused kernel per direction that forms only the products inside each phase's compact span (13 of 161 taps at
    44.1 -> 48 kHz; csrc/resample.hip). One deviation from torchaudio: h is exactly 0 where the window's argument was clamped, so a
    NaN or inf sample reaches only the outputs whose span covers it - in torchaudio's conv1d form it poisons every output of the
    2 width + o window. resampling_method: "sinc_interp_hann" or "sinc_interp_kaiser" (beta = 14.769656459379492 when None).
    Differentiable in x: the gradient is the transposed filter applied to the upstream gradient, a gather without atomics; y and the
    gradient are bit-identical run to run and for a row alone or inside a batch. Nothing is saved for the backward pass. The rates and
    the design are not differentiable; double backward is refused. float32 compute (half and bfloat16 are converted), float64 refused.
    ValueError for bad arguments (signal.check_resampling); NotImplementedError, before any launch, for a design whose compact table
    has more than 16384 taps in either direction or whose span of taps does not fit the staged window - every ratio with both reduced
    rates up to 1024 at the default parameters fits."""
    o, n = _signal.check_resampling(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    if o == n:
        return x
    _lib.require_device(x, "x")
    require_fp32_ok(x, "resample")
    if x.dim() < 1:
        raise RuntimeError("resample: x must have at least one dimension (..., time)")
    design = _ops.resample_design(o, n, lowpass_filter_width, rolloff, resampling_method, beta)
    lead, N = x.shape[:-1], x.shape[-1]
    rows = 1
    for s in lead:
        rows *= s
    y = ResampleFunction.apply(x.reshape(rows, N), design)
    return y.reshape(*lead, design.out_len(N))


def stereo_bus(x: torch.Tensor, sample_rate: int, send_db: torch.Tensor):
    """Sum stereo tracks (bs, 2, tracks, seq_len) into one stereo bus (bs, 2, seq_len) with send levels in dB, bs*tracks values
    (reference: dasp_pytorch/functional.py:32-62, send_db.view(bs, 1, tracks, 1)). At most 64 tracks."""
    bs, chs, tracks, seq_len = x.size()
    assert chs == 2, "Input tensor must have shape (bs, 2, tracks, seq_len)"
    if send_db.numel() != bs * tracks:
        raise RuntimeError(f"shape '[{bs}, 1, {tracks}, 1]' is invalid for input of size {send_db.numel()}")
    require_fp32_ok(x, "stereo_bus")
    return BusFunction.apply(x, send_db)


def advanced_distortion(x, sample_rate, input_gain_db, output_gain_db, tone, dc_offset):
    """Not implemented in the reference either (dasp_pytorch/functional.py:81-111)."""
    raise NotImplementedError


def graphic_eq(x: torch.Tensor, sample_rate: float):
    """Not implemented in the reference either (dasp_pytorch/functional.py:114-115)."""
    raise NotImplementedError


def stereo_widener(x: torch.Tensor, sample_rate: float, width: torch.Tensor):
    """Mid/side stereo widener on (bs, 2, seq_len), width with bs values (the reference needs them shaped (bs, 1)): mid * 2 (1 - width), side * 2 width
    (reference: dasp_pytorch/functional.py:580-605)."""
    bs, chs, seq_len = x.size()
    assert chs == 2, "Input tensor must have shape (bs, 2, seq_len)"
    if width.numel() != bs:
        raise RuntimeError(f"The size of tensor a ({bs}) must match the size of tensor b ({width.numel()})")
    require_fp32_ok(x, "stereo_widener")
    return WidenerFunction.apply(x, width)


def stereo_panner(x: torch.Tensor, sample_rate: float, pan: torch.Tensor):
    """Pan mono tracks (bs, num_tracks, seq_len) across the stereo field; pan in [0, 1] with bs*num_tracks values. Returns
    (bs, 2, num_tracks, seq_len), the shape the reference's code produces (its docstring says otherwise;
    dasp_pytorch/functional.py:608-636)."""
    bs, num_tracks, seq_len = x.size()
    if pan.numel() != bs * num_tracks:
        raise RuntimeError(f"shape '[{bs}, 1, {num_tracks}, 1]' is invalid for input of size {pan.numel()}")
    require_fp32_ok(x, "stereo_panner")
    return PannerFunction.apply(x, pan)


def stereo_mix(x: torch.Tensor, sample_rate: float, gain_db: torch.Tensor, pan: torch.Tensor, send_db: torch.Tensor = None):
    """Mix mono tracks (bs, num_tracks, seq_len) onto a stereo bus (bs, 2, seq_len): a fader gain_db and a pan in [0, 1] per track, bs*num_tracks
    values each, in one pass over x. The result is what the reference's functions compose to,
    stereo_bus(stereo_panner(x, sample_rate, pan), sample_rate, gain_db), without the (bs, 2, num_tracks, seq_len) tensor between them.
    With send_db (bs*num_tracks values) it returns the tuple (mix, send): send is an effects send taken post-fader and post-pan,
    stereo_bus(stereo_panner(x, sample_rate, pan), sample_rate, gain_db + send_db). Differentiable in x and in every control.
    At most 256 tracks (dasp_stereo_mix_max_tracks); more raise DaspHipError (unsupported configuration)."""
    bs, num_tracks, seq_len = x.size()
    for name, c in (("gain_db", gain_db), ("pan", pan), ("send_db", send_db)):
        if c is not None and c.numel() != bs * num_tracks:
            raise RuntimeError(f"{name}: shape '[{bs}, {num_tracks}]' is invalid for input of size {c.numel()}")
    require_fp32_ok(x, "stereo_mix")
    mix, send = StereoMixFunction.apply(x, gain_db, pan, send_db)
    return mix if send_db is None else (mix, send)


def parametric_eq(
    x: torch.Tensor,
    sample_rate: float,
    low_shelf_gain_db: torch.Tensor,
    low_shelf_cutoff_freq: torch.Tensor,
    low_shelf_q_factor: torch.Tensor,
    band0_gain_db: torch.Tensor,
    band0_cutoff_freq: torch.Tensor,
    band0_q_factor: torch.Tensor,
    band1_gain_db: torch.Tensor,
    band1_cutoff_freq: torch.Tensor,
    band1_q_factor: torch.Tensor,
    band2_gain_db: torch.Tensor,
    band2_cutoff_freq: torch.Tensor,
    band2_q_factor: torch.Tensor,
    band3_gain_db: torch.Tensor,
    band3_cutoff_freq: torch.Tensor,
    band3_q_factor: torch.Tensor,
    high_shelf_gain_db: torch.Tensor,
    high_shelf_cutoff_freq: torch.Tensor,
    high_shelf_q_factor: torch.Tensor,
):
    """Six-band parametric EQ: low-shelf -> 4 peaking bands -> high-shelf
    (reference: dasp_pytorch/functional.py:118-272). Each control is a tensor with bs (or 1)
    elements; the same filter is applied to every channel of a batch item."""
    bs, chs, seq_len = x.size()
    controls = [
        low_shelf_gain_db, low_shelf_cutoff_freq, low_shelf_q_factor,
        band0_gain_db, band0_cutoff_freq, band0_q_factor,
        band1_gain_db, band1_cutoff_freq, band1_q_factor,
        band2_gain_db, band2_cutoff_freq, band2_q_factor,
        band3_gain_db, band3_cutoff_freq, band3_q_factor,
        high_shelf_gain_db, high_shelf_cutoff_freq, high_shelf_q_factor,
    ]
    n = controls[0].numel()
    if any(c.numel() != n for c in controls) or n not in (1, bs):
        raise RuntimeError(f"parametric_eq controls must each hold {bs} (or 1) values, got {[c.numel() for c in controls]}")
    if is_f64(x):
        return ParametricEQ64Function.apply(x, float(sample_rate), _PEQ_TYPES, *controls)
    return _ops.parametric_eq(x, sample_rate, _PEQ_TYPES, controls)


def _dynamics(mode, x, sample_rate, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db, eps, lookahead_samples):
    bs, chs, seq_len = x.size()
    ctls = (threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db)
    for c in ctls:   # the reference's .view(-1, 1, 1) against a (bs, 1, seq_len) side chain: no parameter broadcasting
        if c.numel() != bs:
            raise RuntimeError(f"The size of tensor a ({c.numel()}) must match the size of tensor b ({bs}) at non-singleton dimension 0")
    if is_f64(x):
        return Dynamics64Function.apply(x, mode, float(sample_rate), float(eps), int(lookahead_samples), *ctls)
    return _ops.dynamics(x, mode, sample_rate, eps, lookahead_samples, ctls)


def compressor(
    x: torch.Tensor,
    sample_rate: float,
    threshold_db: torch.Tensor,
    ratio: torch.Tensor,
    attack_ms: torch.Tensor,
    release_ms: torch.Tensor,
    knee_db: torch.Tensor,
    makeup_gain_db: torch.Tensor,
    eps: float = 1e-8,
    lookahead_samples: int = 0,
):
    """Feed-forward dynamic range compressor (reference: dasp_pytorch/functional.py:275-399): summed side
    chain, soft-knee gain computer in dB, one-pole smoothing with the attack time constant (release_ms is
    accepted and ignored, exactly like the reference), optional look-ahead delay of the signal path, make-up
    gain. The smoothing filter is evaluated as an exact recurrence (chunked scan) instead of the reference's
    frequency-sampling FFT filter. Deviation: knee_db == 0 gives finite gradients (the reference's are NaN)."""
    return _dynamics(0, x, sample_rate, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db, eps, lookahead_samples)


def expander(
    x: torch.Tensor,
    sample_rate: float,
    threshold_db: torch.Tensor,
    ratio: torch.Tensor,
    attack_ms: torch.Tensor,
    release_ms: torch.Tensor,
    knee_db: torch.Tensor,
    makeup_gain_db: torch.Tensor,
    eps: float = 1e-8,
    lookahead_samples: int = 0,
):
    """Downward expander with the compressor's structure and signature. The reference's `expander()` raises
    NotImplementedError (dasp_pytorch/functional.py:402-403), so there is no reference behaviour: below
    threshold - knee/2 the level is mapped to T + (x_db - T) * ratio, with the standard quadratic soft knee
    (Giannoulis, Massberg & Reiss 2012), above the knee the signal is untouched."""
    return _dynamics(1, x, sample_rate, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_gain_db, eps, lookahead_samples)


_FB_CACHE = {}


def _device_filterbank(num_taps: int, sample_rate: float, device: torch.device):
    """One device-resident copy of the octave filterbank per (taps, sample_rate, device): the taps are constants, so the
    host->device copy and their spectra (ops._filter_spectrum) are paid once, not per call. Not kept when first asked for inside a
    HIP-graph capture (that memory belongs to the graph being captured)."""
    key = (num_taps, sample_rate, device)
    hit = _FB_CACHE.get(key)
    if hit is not None:
        return hit
    bank = _signal.octave_band_filterbank(num_taps, sample_rate).squeeze(1).to(device).contiguous()
    if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        if len(_FB_CACHE) >= 8:
            _FB_CACHE.clear()
        _FB_CACHE[key] = bank
    return bank


def noise_shaped_reverberation(
    x: torch.Tensor,
    sample_rate: float,
    band0_gain: torch.Tensor,
    band1_gain: torch.Tensor,
    band2_gain: torch.Tensor,
    band3_gain: torch.Tensor,
    band4_gain: torch.Tensor,
    band5_gain: torch.Tensor,
    band6_gain: torch.Tensor,
    band7_gain: torch.Tensor,
    band8_gain: torch.Tensor,
    band9_gain: torch.Tensor,
    band10_gain: torch.Tensor,
    band11_gain: torch.Tensor,
    band0_decay: torch.Tensor,
    band1_decay: torch.Tensor,
    band2_decay: torch.Tensor,
    band3_decay: torch.Tensor,
    band4_decay: torch.Tensor,
    band5_decay: torch.Tensor,
    band6_decay: torch.Tensor,
    band7_decay: torch.Tensor,
    band8_decay: torch.Tensor,
    band9_decay: torch.Tensor,
    band10_decay: torch.Tensor,
    band11_decay: torch.Tensor,
    mix: torch.Tensor,
    num_samples: int = 65536,
    num_bandpass_taps: int = 1023,
    noise: torch.Tensor = None,
    device_noise: bool = False,
    noise_seed: int = None,
    noise_seed_offset: torch.Tensor = None,
):
    """Artificial reverberation from frequency-band noise shaping (reference: dasp_pytorch/functional.py:406-577).
    Mono input is duplicated to stereo and the output always has 2 channels, as in the reference.

    White noise: by default it is what the reference draws -- torch.randn(bs*2, 12, num_samples + num_bandpass_taps - 1) from the
    global *CPU* generator (functional.py:548) -- so the same torch.manual_seed gives the same impulse responses as the reference,
    and the CPU generator is left in the state that call leaves it in; the values are computed on x's device from the generator's
    state (csrc/mtrand.hip, _mt19937.py: the twister run in parallel by jump-ahead, torch's float and Box-Muller layout), not drawn
    on the host and copied (0.56 s + 0.8 GB at (128,2,262144)). `device_noise=True` generates it on x's device
    instead, inside the filter-bank kernels (a counter-based stream, csrc/reverb.hip: the noise tensor - 0.8 GB at the default sizes
    and 128 items - never exists, forward and backward recompute it); its 63-bit seed is `noise_seed` (giving a seed selects this
    mode by itself), or, when that is None, one draw
    from torch's global CPU generator per call - so torch.manual_seed makes it reproducible and successive calls differ, as with the
    reference. Inside a HIP-graph capture that draw happens once, at capture time; `noise_seed_offset`, a 1-element int64 tensor
    on x's device, is added to the seed when the kernels run - bump it once per replay (e.g. `offset.add_(1)` at the end of the
    captured step) and every replay draws new noise. `noise=` supplies the noise tensor explicitly. The keywords are additions; Processor.process_normalized passes only the named parameters above."""
    assert num_bandpass_taps % 2 == 1, "num_bandpass_taps must be odd"
    bs, chs, seq_len = x.size()
    assert chs <= 2, "only mono/stereo signals are supported"
    require_fp32_ok(x, "noise_shaped_reverberation")
    for c in (band0_gain, band1_gain, band2_gain, band3_gain, band4_gain, band5_gain, band6_gain, band7_gain, band8_gain, band9_gain,
              band10_gain, band11_gain, band0_decay, band1_decay, band2_decay, band3_decay, band4_decay, band5_decay, band6_decay,
              band7_decay, band8_decay, band9_decay, band10_decay, band11_decay, mix):
        if c.numel() != bs:   # the reference's torch.stack(...).view(bs, 12) / mix.view(bs, 1, 1) (functional.py:498-544): no broadcasting
            raise RuntimeError(f"shape '[{bs}, 12]' is invalid for input of size {12 * c.numel()}")
    # (chs == 1: the reference copies mono to stereo, functional.py:493-495; the kernels read the one row for both output channels,
    # ops.ReverbFunction)
    gains = (band0_gain, band1_gain, band2_gain, band3_gain, band4_gain, band5_gain, band6_gain, band7_gain, band8_gain, band9_gain, band10_gain, band11_gain)
    decays = (band0_decay, band1_decay, band2_decay, band3_decay, band4_decay, band5_decay, band6_decay, band7_decay, band8_decay, band9_decay, band10_decay,
              band11_decay)
    if _ops.noise_shaped_reverb_ok(x, gains, decays, mix, noise):
        # the 25 tensors as they are: torch.ops.dasp.noise_shaped_reverb stacks them and hands their gradients back in C++ (csrc/torch_ext)
        filters, noise, seed, offset, pending = _reverb_noise(x, sample_rate, num_samples, num_bandpass_taps, noise, device_noise, noise_seed, noise_seed_offset)
        try:
            return _ops.noise_shaped_reverb(x, noise, filters, gains, decays, mix, int(num_samples), seed, offset, 0.0)
        finally:
            pending.finish()
    return _reverb_from_matrices(x, sample_rate, _StackColumns.apply(*gains), _StackColumns.apply(*decays), mix.view(bs), num_samples, num_bandpass_taps, noise,
                                 device_noise, noise_seed, noise_seed_offset)


class _StackColumns(torch.autograd.Function):
    """torch.stack([c.view(bs) for c in cols], dim=1) with a backward that hands every column its gradient as a contiguous row of one
    transposed matrix: autograd's own stack backward returns 12 strided column views, each of which AccumulateGrad then copies with a
    kernel of its own (24 launches per reverb step for the 2 x 12 band controls; here: one transpose per matrix)."""

    @staticmethod
    def forward(ctx, *cols):
        ctx.shapes = [c.shape for c in cols]
        return torch.stack([c.reshape(-1) for c in cols], dim=1)

    @staticmethod
    def backward(ctx, g):
        rows = g.t().contiguous().unbind(0)
        return tuple(r.reshape(shape) if need else None for r, shape, need in zip(rows, ctx.shapes, ctx.needs_input_grad))


def _reverb_noise(x, sample_rate, num_samples, num_bandpass_taps, noise, device_noise, noise_seed, noise_seed_offset):
    """The filter bank on x's device and the white noise of one call, as the reference draws it (functional.py:548) or as the keywords of
    noise_shaped_reverberation ask for it: (filters, noise tensor or None, seed or None, seed offset or None, pending). `pending.finish()`
    installs the CPU generator's state after a default draw (its read-back rides behind the generating kernels): call it once the
    forward kernels are queued, before returning to the caller."""
    filters = _device_filterbank(int(num_bandpass_taps), float(sample_rate), x.device)
    seed, pending = None, _mt19937._NothingPending()
    if noise_seed_offset is not None and (noise is not None or not (device_noise or noise_seed is not None)):
        raise ValueError("noise_seed_offset only applies to the generated noise (device_noise=True or noise_seed=...)")
    if noise is None:
        if device_noise or noise_seed is not None:
            # one 63-bit draw from the global CPU generator (a host-side scalar: no device work, no sync) unless the caller fixed the seed
            seed = int(noise_seed) if noise_seed is not None else int(torch.empty((), dtype=torch.int64).random_().item())
        else:
            # the reference's draw (functional.py:548), made where it is used: the values and the CPU generator's state afterwards are
            # those of torch.randn(bs*2, 12, ...) on the global CPU generator, computed by csrc/mtrand.hip from that generator's state
            noise, pending = _mt19937.randn_cpu_stream(x.shape[0] * 2, 12, num_samples + num_bandpass_taps - 1, device=x.device, defer=True)
    return filters, noise, seed, (noise_seed_offset if seed is not None else None), pending


def _reverb_from_matrices(x, sample_rate, band_gains, band_decays, mix, num_samples=65536, num_bandpass_taps=1023, noise=None, device_noise=False,
                          noise_seed=None, noise_seed_offset=None, decay_bound=0.0):
    """noise_shaped_reverberation on the band gains / decays as (bs, 12) matrices and mix (bs): what NoiseShapedReverb.process_normalized has
    as slices of its de-normalised (bs, 25) tensor. x: (bs, 1 or 2, seq_len).
    decay_bound > 0: the caller vouches that no band decay exceeds it (a validated parameter range) - lets the filter bank skip a launch."""
    filters, noise, seed, offset, pending = _reverb_noise(x, sample_rate, num_samples, num_bandpass_taps, noise, device_noise, noise_seed, noise_seed_offset)
    try:
        return _ops_reverb(x, noise, filters, band_gains.to(x.device), band_decays.to(x.device), mix.to(x.device), int(num_samples), seed, offset, float(decay_bound))
    finally:
        pending.finish()


def _dynamics_from_matrix(mode, x, sample_rate, controls, eps=1e-8, lookahead_samples=0):
    """compressor / expander on the (bs, 6) matrix of controls (columns in the functions' argument order)."""
    from .ops import DynamicsMatrixFunction
    return DynamicsMatrixFunction.apply(x, mode, float(sample_rate), float(eps), int(lookahead_samples), controls)


# ---- level metering and normalisation (csrc/loudness.hip) ---------------------------------------------------------------------------------
def _level_rows(x, what, sample_rate=None, max_chs=None):
    """Shape, channel count, sample rate and length checks of the level ops, before any device check. -> H (samples per 100 ms) or None."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: x must be a torch.Tensor")
    if x.dim() != 3:
        raise ValueError(f"{what}: x must be shaped (bs, chs, seq_len), got {tuple(x.shape)}")
    bs, chs, seq_len = x.shape
    if bs < 1 or chs < 1 or seq_len < 1:
        raise ValueError(f"{what}: x must hold at least one item, channel and sample, got {tuple(x.shape)}")
    H = None
    if max_chs is not None:
        if chs > max_chs:
            raise ValueError(f"{what}: 1 to {max_chs} channels (L, R, C, Ls, Rs) are supported, got {chs}")
        fs = float(sample_rate)
        if not 8000.0 <= fs <= 384000.0:
            raise ValueError(f"{what}: sample_rate must lie in [8000, 384000], got {sample_rate!r}")
        H = int(round(0.1 * fs))
        if seq_len < 4 * H:
            raise ValueError(f"{what}: seq_len {seq_len} is shorter than one 400 ms block ({4 * H} samples at {sample_rate} Hz)")
    require_fp32_ok(x, what)
    _lib.require_device(x)
    return H


def _rows32(x):
    return x.detach().to(torch.float32).contiguous()


class _LoudnessFunction(torch.autograd.Function):
    """x (bs, chs, N) -> L (bs) LUFS. Forward: filter pass (+ a state pre-pass for few rows) and the gate launch; backward: one filter
    pass backwards in time over the K-weighted signal the forward call kept (its own buffer: x may be overwritten after the forward,
    and the backward repeated - scratch is allocated per call)."""

    @staticmethod
    def forward(ctx, x, fs):
        x32 = _rows32(x)
        bs, chs, N = x32.shape
        nd = _lib.lib().dasp_loudness_scratch_doubles(bs, chs, N, fs)
        nb = _lib.lib().dasp_loudness_blocks(N, fs)
        if nd < 0 or nb < 0:
            raise _lib.DaspHipError(f"loudness: {tuple(x32.shape)} at {fs} Hz is not supported")
        dev, grad = x.device, ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            scratch = torch.empty(nd, dtype=torch.float64, device=dev)
            L = torch.empty(bs, dtype=torch.float32, device=dev)
            ysave = torch.empty_like(x32) if grad else None
            cov = torch.empty(bs * chs * (nb + 3), dtype=torch.float32, device=dev) if grad else None
            _lib.call("dasp_loudness_forward", _lib.ptr(x32), _lib.ptr(scratch), _lib.ptr(L), _lib.ptr(ysave), _lib.ptr(cov), bs, chs, N, fs, _lib.stream())
        if grad:
            ctx.save_for_backward(ysave, cov)
        ctx.cfg = (fs, nd, x.dtype)
        return L.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gL):
        if not ctx.needs_input_grad[0]:
            return None, None
        ysave, cov = ctx.saved_tensors
        fs, nd, dtype = ctx.cfg
        bs, chs, N = ysave.shape
        with torch.cuda.device(ysave.device):
            g32 = gL.detach().reshape(-1).to(torch.float32).contiguous()
            scratch = torch.empty(nd, dtype=torch.float64, device=ysave.device)
            gx = torch.empty_like(ysave)
            _lib.call("dasp_loudness_backward", _lib.ptr(ysave), _lib.ptr(cov), _lib.ptr(g32), _lib.ptr(scratch), _lib.ptr(gx), bs, chs, N, fs, _lib.stream())
        return gx.to(dtype), None


class _PeakNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, peak_db, eps):
        x32 = _rows32(x)
        bs, chs, N = x32.shape
        rows = bs * chs
        nd = _lib.lib().dasp_peaknorm_scratch_doubles(rows, N)
        if nd < 0:
            raise _lib.DaspHipError(f"peak_normalize: {tuple(x32.shape)} is not supported")
        dev = x.device
        with torch.cuda.device(dev):
            scratch = torch.empty(nd, dtype=torch.float64, device=dev)
            peak = torch.empty(2 * rows, dtype=torch.float64, device=dev)
            y = torch.empty_like(x32)
            _lib.call("dasp_peaknorm_forward", _lib.ptr(x32), _lib.ptr(scratch), _lib.ptr(peak), _lib.ptr(y), rows, N, peak_db, eps, _lib.stream())
        ctx.save_for_backward(x32, peak)
        ctx.cfg = (peak_db, eps, nd, x.dtype)
        return y.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x32, peak = ctx.saved_tensors
        peak_db, eps, nd, dtype = ctx.cfg
        bs, chs, N = x32.shape
        with torch.cuda.device(x32.device):
            g32 = gy.detach().to(torch.float32).contiguous()
            scratch = torch.empty(nd, dtype=torch.float64, device=x32.device)
            gx = torch.empty_like(x32)
            _lib.call("dasp_peaknorm_backward", _lib.ptr(x32), _lib.ptr(g32), _lib.ptr(peak), _lib.ptr(scratch), _lib.ptr(gx), bs * chs, N, peak_db, eps,
                      _lib.stream())
        return gx.to(dtype), None, None


def loudness(x: torch.Tensor, sample_rate: float):
    """Integrated loudness in LUFS (ITU-R BS.1770-4 / EBU R128) of each batch item of x (bs, chs, seq_len), 1 <= chs <= 5 in the order
    L, R, C, Ls, Rs with the weights 1, 1, 1, 1.41, 1.41 -> (bs,). K-weighting (signal.k_weighting_sos), 400 ms blocks every 100 ms - a
    tail that does not complete a block is ignored -, the absolute gate at -70 LUFS and the relative gate 10 LU below the gated mean.
    An item with no block past the gates gives -inf and a zero gradient. Differentiable with respect to x with the gates held fixed
    (what autograd of a masked mean gives). 8000 <= sample_rate <= 384000 and seq_len >= one block, else ValueError.
    Non-finite samples: the gates are IEEE comparisons, so a block that holds a NaN (every block from a NaN or inf sample on: the
    K-weighting is recursive) passes neither and is left out of the mean. A NaN in the middle of an item therefore gives a FINITE
    loudness, measured on the blocks before it, and a gradient that is NaN over the whole row that holds it (the item's other rows stay
    finite); a NaN in the first block gives -inf and a zero gradient. Other items are not affected. A sample as large as 1e30 is
    metered (+567 LUFS); its gradient underflows float32 to 0."""
    _level_rows(x, "loudness", sample_rate, 5)
    return _LoudnessFunction.apply(x, float(sample_rate))


def loudness_normalize(x: torch.Tensor, sample_rate: float, target_lufs=-23.0):
    """gain(x, sample_rate, target_lufs - loudness(x, sample_rate)): every item is brought to `target_lufs` (a float, or a tensor with bs
    values). Gradients flow through the gain and through the meter. Items whose loudness is -inf are returned unchanged (0 dB)."""
    _level_rows(x, "loudness_normalize", sample_rate, 5)
    bs = x.shape[0]
    L = _LoudnessFunction.apply(x, float(sample_rate))
    if isinstance(target_lufs, torch.Tensor):
        if target_lufs.numel() != bs:
            raise RuntimeError(f"shape '[{bs}]' is invalid for input of size {target_lufs.numel()}")
        target = target_lufs.to(device=x.device, dtype=L.dtype).reshape(bs)
    else:
        target = torch.full((bs,), float(target_lufs), dtype=L.dtype, device=x.device)
    gain_db = torch.where(torch.isfinite(L), target - L, torch.zeros_like(L))
    return gain(x, sample_rate, gain_db)


def peak_normalize(x: torch.Tensor, sample_rate: float, peak_db: float = 0.0, eps: float = 1e-8):
    """Per row - per (item, channel), as the reference's examples do by hand (examples/auto_eq.py:289-291) -:
    y = x * 10^(peak_db / 20) / max(max_n |x[n]|, eps); eps = 0 is the examples' plain division. Differentiable: the maximum's
    gradient goes to the lowest index attaining it; a peak of exactly eps takes the constant branch (gy * scale / eps).
    A row that holds a NaN has a NaN peak, as x.abs().amax(-1) has: the row and its gradient are NaN throughout. A row that holds an inf
    comes out as 0 with a NaN at that sample. eps = 0 on a row of zeros gives NaN (0 / 0). Other rows are not affected."""
    _level_rows(x, "peak_normalize")
    peak_db, eps = float(peak_db), float(eps)
    if not (peak_db == peak_db and abs(peak_db) != float("inf")) or not eps >= 0.0:
        raise ValueError(f"peak_normalize: peak_db must be finite and eps >= 0, got {peak_db!r}, {eps!r}")
    return _PeakNormFunction.apply(x, peak_db, eps)
