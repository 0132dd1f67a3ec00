"""Host side of resample: the argument checks, the windowed-sinc design in float64 and the two compact tables that
csrc/resample.hip reads. numpy only; signal.resample_taps and the binding (_ctypes_ops.ResampleFunction) both build on it.

The design restates torchaudio.functional.resample's published algorithm with one deviation: where the window's argument was clamped
to +-lowpass_filter_width the tap is exactly 0 (torchaudio's formula gives <= 1e-20 there for the Kaiser window and a float32 zero for
the Hann window), so every phase has a compact span of taps."""
import math
import numbers

import numpy as np

METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")
KAISER_BETA = 14.769656459379492


def _rate(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v != int(v) or int(v) < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


def check_resampling(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """The argument ranges of signal.resample_taps / functional.resample: ValueError naming the argument and what it may be. Returns the
    reduced rates (o, n)."""
    o, n = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
    W = lowpass_filter_width
    if isinstance(W, bool) or not isinstance(W, numbers.Integral) or W < 1:
        raise ValueError(f"lowpass_filter_width must be an integer >= 1, got {W!r}")
    if isinstance(rolloff, bool) or not isinstance(rolloff, numbers.Real) or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff must lie in (0, 1], got {rolloff!r}")
    if resampling_method not in METHODS:
        raise ValueError(f"resampling_method must be one of {METHODS}, got {resampling_method!r}")
    if beta is not None and (isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not 0.0 <= beta < float("inf")):
        raise ValueError(f"beta must be None or a finite number >= 0, got {beta!r}")
    g = math.gcd(o, n)
    return o // g, n // g


def taps(o, n, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """(h float64 (n, K), width, inside bool (n, K)) for reduced rates o : n. inside: where the window's argument was not clamped; h is
    exactly zero elsewhere."""
    W = float(lowpass_filter_width)
    base = min(o, n) * float(rolloff)
    width = int(math.ceil(W * o / base))
    K = 2 * width + o
    r = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    t = (-r / n + (k - width) / o) * base
    inside = np.abs(t) < W
    t = np.clip(t, -W, W)
    if resampling_method == "sinc_interp_hann":
        window = np.cos(t * math.pi / W / 2.0) ** 2
    else:
        b = KAISER_BETA if beta is None else float(beta)
        window = np.i0(b * np.sqrt(np.maximum(1.0 - (t / W) ** 2, 0.0))) / np.i0(b)
    h = np.sinc(t) * window * (base / o)                 # np.sinc(t) = sin(pi t) / (pi t), 1 at 0
    return np.where(inside, h, 0.0), width, inside


class Table:
    """One direction's table: out[Q A + p] = sum_{m < cnt[p]} T[m][p] in[Q B + off[p] + m]. words: A P float32 bit patterns, tap-major,
    then A words (off[p] - lo) | cnt[p] << 16."""

    def __init__(self, A, B, off, cnt, rows):
        self.A, self.B = int(A), int(B)
        self.off, self.cnt = np.asarray(off, np.int64), np.asarray(cnt, np.int64)
        self.P = int(self.cnt.max())
        self.lo = int(self.off.min())
        self.span = int((self.off + self.cnt).max()) - self.lo
        self.rows = rows                                 # per phase: its float32 taps
        self._words = None

    @property
    def floats(self):
        return self.A * self.P

    @property
    def words(self):
        if self._words is None:
            T = np.zeros((self.P, self.A), np.float32)
            for p, row in enumerate(self.rows):
                T[:len(row), p] = row
            meta = (self.off - self.lo).astype(np.uint32) | (self.cnt.astype(np.uint32) << np.uint32(16))
            self._words = np.ascontiguousarray(np.concatenate([T.reshape(-1).view(np.uint32), meta]))
        return self._words


class Design:
    """A resampler for reduced rates o : n: the float32 taps (n, K) and the tables of the two directions."""

    def __init__(self, o, n, lowpass_filter_width, rolloff, resampling_method, beta):
        self.o, self.n = o, n
        h, self.width, inside = taps(o, n, lowpass_filter_width, rolloff, resampling_method, beta)
        self.K = h.shape[1]
        self.h32 = h.astype(np.float32)
        self.first = inside.argmax(1)
        self.cnt = inside.sum(1)
        assert all(inside[r, self.first[r]:self.first[r] + self.cnt[r]].all() for r in range(n))         # t is monotonic in k
        self.fwd = Table(n, o, self.first - self.width, self.cnt, [self.h32[r, self.first[r]:self.first[r] + self.cnt[r]] for r in range(n)])
        # the transposed index: tap (r, k) of output q n + r reads input q o + k - width = (q + d) o + s, so input (Q, s) is read by
        # output Q n + (r - d n) - consecutive outputs for one s, because |i / o - j / n| base < lowpass_filter_width is an interval of j
        rr, kk = np.nonzero(inside)
        e = kk - self.width
        d = np.floor_divide(e, o)
        s, j = e - d * o, rr - d * n
        order = np.lexsort((j, s))
        s, j, v = s[order], j[order], self.h32[rr, kk][order]
        start = np.searchsorted(s, np.arange(o))
        stop = np.searchsorted(s, np.arange(o), side="right")
        assert (stop > start).all() and all((np.diff(j[a:b]) == 1).all() for a, b in zip(start, stop))
        self.bwd = Table(o, n, j[start], stop - start, [v[a:b] for a, b in zip(start, stop)])

    def out_len(self, N):
        return -((-self.n * int(N)) // self.o)           # ceil(n N / o) in Python's integers
