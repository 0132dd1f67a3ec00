"""The losses and spectral ops off their nominal domain: the case table and the float64 references of tests/test_gpu_loss_input_domain.py
(GPU) and tests/test_loss_input_domain_cpu.py (the references' own behaviour, without a GPU). Ops: the three STFT-loss layouts (linear
bins, mel bins, sum / difference), the time-domain losses, the A-weighting FIR exports, signal.freqdomain_fir and fft_freqz /
fft_sosfreqz. References: tests/auraloss_restated.py, auraloss_mel_restated.py, auraloss_sumdiff_restated.py, auraloss_time_restated.py,
torch.fft in float64 and tests/freqz_exact.py, each run on the SAME off-domain input as the kernels.

Bounds are those of each op's existing generic-input test, restated with their lines:
  STFT loss            2e-5 relative (tests/test_gpu_losses.py:40)
  STFT gradients       mono, linear bins: 1e-2 in relative L2 norm and 2e-2 of the largest entry (tests/test_gpu_losses.py:42-43);
                       mel bins and sum / difference: 1e-2 in relative L2 norm (tests/test_gpu_mel_stft.py:78, test_gpu_sumdiff_stft.py:114)
  STFT gradients, run against run (float atomics fix only the order of a sum): 1e-5 of the largest entry
                       (tests/test_gpu_mrstft_options.py:208, test_graph_replay_of_the_example_loss)
  time-domain losses   loss 2e-5 (dB terms: of max(1, |loss|)), gradients 1e-4 in relative L2 norm and of the largest entry
                       (tests/test_gpu_time_losses.py:22, 88-95)
  freqdomain_fir       L-inf / peak 2e-5 per item (tests/test_gpu_freqdomain_fir.py:16, 110)
Gradients are judged per row (per item for the stereo loss): a poisoned row says nothing about its neighbours."""
import functools

import numpy as np
import torch

from tests import auraloss_mel_restated as amr
from tests import auraloss_restated as ar
from tests import auraloss_sumdiff_restated as sdr
from tests import auraloss_time_restated as atr

SR = 44100
EPS = 1e-8
NAN, INF = float("nan"), float("inf")
LOSS_TOL = 2e-5
ATOMICS_TOL = 1e-5
MIXES = {"sc+log": (1.0, 1.0, 0.0), "log+lin": (0.0, 1.0, 1.0)}
W_SUMDIFF = dict(w_sum=0.7, w_diff=1.3)                      # as tests/test_gpu_sumdiff_stft.py


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

def generic(shape, seed):
    """The generic pair of tests/test_gpu_mrstft_options.py:54-58."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(shape) * 0.3).astype(np.float32)
    b = (0.6 * a + 0.2 * rng.standard_normal(shape)).astype(np.float32)
    return a, b


POSITIONS = ("first", "mid", "last")                         # sample 0, N // 2, N - 1: the first and the last are also read through the reflect padding
POISONS = [(arg, value, pos) for arg in ("input", "target") for value in ("nan", "inf") for pos in POSITIONS]


def position(pos, N):
    return {"first": 0, "mid": N // 2, "last": N - 1}[pos]


def poisoned(p, t, poison):
    """Copies of (p, t) with one sample of item 1 (channel: the position's index modulo the channel count) set to NaN or +inf."""
    arg, value, pos = poison
    p, t = np.array(p), np.array(t)
    x = p if arg == "input" else t
    x[1, POSITIONS.index(pos) % x.shape[1], position(pos, x.shape[-1])] = NAN if value == "nan" else INF
    return p, t


def items(a):
    """(items, everything else) of an array whose first axis is the batch item."""
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1)


# ---- the STFT losses ------------------------------------------------------------------------------------------------------------------

def shape_for(n_fft, chs):
    return (3, chs, 3000 if n_fft <= 256 else (5000 if n_fft <= 2048 else 9000))


class StftCase:
    """One resolution of one layout: layout "mono" (MultiResolutionSTFTLoss) or "sd" (SumAndDifferenceSTFTLoss), linear bins
    (n_bins None) or mel bins, with or without the A-weighting at 44100, one of the two weight mixes."""

    def __init__(self, layout, res, mix, n_bins=None, aw=False):
        self.layout, self.res, self.mix, self.n_bins, self.aw = layout, (tuple(res),), mix, n_bins, aw
        self.shape = shape_for(res[0], 2 if layout == "sd" else 1)
        self.name = f"{layout}-{res[0]}-{mix}" + (f"-mel{n_bins}" if n_bins else "") + ("-aw" if aw else "")

    def __str__(self):
        return self.name

    @property
    def w_sc(self):
        return MIXES[self.mix][0]

    def options(self, **more):
        """The package's keywords."""
        w = MIXES[self.mix]
        o = dict(fft_sizes=[r[0] for r in self.res], hop_sizes=[r[1] for r in self.res], win_lengths=[r[2] for r in self.res],
                 w_sc=w[0], w_log_mag=w[1], w_lin_mag=w[2])
        if self.aw or self.n_bins:
            o["sample_rate"] = SR
        if self.aw:
            o["perceptual_weighting"] = True
        if self.n_bins:
            o.update(scale="mel", n_bins=self.n_bins)
        if self.layout == "sd":
            o.update(W_SUMDIFF)
        return dict(o, **more)

    def loss_fn(self, D, **more):
        cls = D.losses.SumAndDifferenceSTFTLoss if self.layout == "sd" else D.losses.MultiResolutionSTFTLoss
        return cls(**self.options(**more))

    def grad_bounds(self):
        """(relative L2, of the largest entry or None) on generic inputs: the module docstring."""
        return (1e-2, 2e-2) if self.layout == "mono" and not self.n_bins else (1e-2, None)

    def ref(self, p, t, eps=EPS):
        """(loss, d / d input, d / d target) of the float64 restatement; non-finite values are results, not errors."""
        from dasp_pytorch_amd import losses
        w = MIXES[self.mix]
        kw = dict(w_sc=w[0], w_log_mag=w[1], w_lin_mag=w[2], taps=losses.a_weighting_taps(float(SR)) if self.aw else None, eps=eps)
        if self.layout == "sd":
            out = sdr.loss_and_grads(p, t, self.res, **W_SUMDIFF, **(dict(sample_rate=SR, n_bins=self.n_bins) if self.n_bins else {}), **kw)
            return out[0], out[3], out[4]
        if self.n_bins:
            return amr.loss_and_grads(p, t, self.res, SR, self.n_bins, **kw)
        return ar.loss_and_grads(p, t, self.res, **kw)


SMALL = ((64, 16, 48), (256, 64, 256))                       # the generic LOGN = 12 kernel
SPLIT = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))        # the split kernels: 1, 2 and 4 waves per frame
BIG = ((8192, 2048, 8191),)                                  # the 8192-point kernel
ALL_RES = SMALL + SPLIT + BIG
_A, _B = "sc+log", "log+lin"

STFT_CASES = (
    # linear bins, mono: every resolution with both mixes, the A-weighting once per kernel family
    [StftCase("mono", r, m) for r in ALL_RES for m in MIXES]
    + [StftCase("mono", SMALL[1], _A, aw=True), StftCase("mono", SPLIT[1], _B, aw=True), StftCase("mono", BIG[0], _A, aw=True)]
    # mel bins, mono (mrstft_mel_*: the generic geometry at every size): 8 and 40 filters
    + [StftCase("mono", SMALL[0], _A, 8), StftCase("mono", SMALL[1], _B, 8, aw=True), StftCase("mono", SPLIT[0], _B, 8),
       StftCase("mono", SPLIT[1], _A, 40), StftCase("mono", SPLIT[2], _B, 40), StftCase("mono", BIG[0], _A, 40, aw=True)]
    # sum / difference on (3, 2, N): every resolution, the mixes alternating
    + [StftCase("sd", r, (_A, _B)[k % 2]) for k, r in enumerate(ALL_RES)]
    + [StftCase("sd", SMALL[1], _A, aw=True), StftCase("sd", SMALL[1], _A, 8), StftCase("sd", SPLIT[2], _B, 40, aw=True),
       StftCase("sd", BIG[0], _A, 40)])
STFT_BY_NAME = {c.name: c for c in STFT_CASES}
assert len(STFT_BY_NAME) == len(STFT_CASES)


@functools.lru_cache(maxsize=None)
def stft_clean(name):
    """(input, target, reference) of a case's clean batch: computed once per process, shared and read-only."""
    case = STFT_BY_NAME[name]
    p, t = generic(case.shape, case.shape[-1] + case.res[0][0])
    ref = case.ref(p, t)
    for v in (p, t) + tuple(ref[1:]):
        v.flags.writeable = False
    return p, t, ref


# ---- silence and the eps clamp (STFT family) ------------------------------------------------------------------------------------------
SILENCE_KINDS = ("zeros", "identical", "below_eps", "straddle")
STRADDLE_SEED = 7


def window_gain(res):
    """sum of the periodic Hann window: the largest |X| of a frame of samples of magnitude <= 1."""
    return float(torch.hann_window(res[2], dtype=torch.float64).sum())


def silence_pair(case, kind):
    """(input, target) of one silence case. "below_eps": both scaled so that NO bin power can reach eps (|x| <= a with (a sum w)^2 =
    eps / 4, whatever the phases); "straddle": a level at which the bin powers lie on both sides of eps (the median power of white noise
    of variance s^2 under a window w is ~ s^2 sum w^2 ln 2: s is set so that this is eps)."""
    shape, res = case.shape, case.res[0]
    a, b = generic(shape, STRADDLE_SEED + shape[-1])
    if kind == "zeros":
        return np.zeros_like(a), np.zeros_like(b)
    if kind == "identical":
        return a, a.copy()
    if kind == "below_eps":
        peak = 0.5 * np.sqrt(EPS) / window_gain(res) / (2.0 if case.layout == "sd" else 1.0)       # (L + R doubles the level)
        scale = peak / max(np.abs(a).max(), np.abs(b).max())
        return (a * scale).astype(np.float32), (b * scale).astype(np.float32)
    w2 = float((torch.hann_window(res[2], dtype=torch.float64) ** 2).sum())
    s = np.sqrt(EPS / (w2 * np.log(2.0))) / 0.3
    return (a * s).astype(np.float32), (b * s).astype(np.float32)


def bin_powers(case, x):
    """The float64 bin powers re^2 + im^2 of every frame of x (items, chs, N), before the clamp (linear bins; for the stereo layout:
    of the sum and of the difference)."""
    v = torch.from_numpy(np.asarray(x, dtype=np.float64))
    sigs = sdr.sum_diff(v) if case.layout == "sd" else (v,)
    n_fft, hop, win = case.res[0]
    w = torch.hann_window(win, dtype=torch.float64)
    out = []
    for s in sigs:
        S = torch.stft(s.reshape(-1, s.shape[-1]), n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
        out.append((S.real ** 2 + S.imag ** 2).reshape(-1))
    return torch.cat(out).numpy()


# one case per kernel family (no A-weighting: the levels are set on the signals the transforms see); Part D runs each with (1, 1, 0) weights
SILENCE_CASES = [STFT_BY_NAME[n] for n in ("mono-256-sc+log", "mono-1024-sc+log", "mono-8192-sc+log", "sd-256-log+lin", "mono-64-sc+log-mel8")]


def silence_case(case):
    """The case with the weights (1, 1, 0) of Part D."""
    return StftCase(case.layout, case.res[0], "sc+log", case.n_bins)


# ---- the time-domain losses -----------------------------------------------------------------------------------------------------------
TD_SHAPE = (3, 2, 4099)
TD_MIX = {"esr": 1.0, "dc": 1.0, "mse": 100.0}                # tests/test_gpu_time_losses.py:23
TD_CASES = dict({name: {name: 1.0} for name in atr.TERMS}, mix=TD_MIX)
TD_LOSS_TOL, TD_GRAD_TOL = 2e-5, 1e-4


@functools.lru_cache(maxsize=None)
def td_draw():
    """The "generic" draw of tests/test_gpu_time_losses.py:37-43 at (3, 2, 4099)."""
    rng = np.random.default_rng([0, *TD_SHAPE, 0])
    t = (0.3 * rng.standard_normal(TD_SHAPE)).astype(np.float32)
    p = (t + 0.09 * rng.standard_normal(TD_SHAPE) + 0.05).astype(np.float32)
    p.flags.writeable = t.flags.writeable = False
    return p, t


def td_ref(p, t, case, zero_mean, reduction):
    return atr.loss_and_grads(p, t, TD_CASES[case], zero_mean=zero_mean, reduction=reduction)


def td_keywords(case, **more):
    return dict({"w_" + k: v for k, v in TD_CASES[case].items()}, **more)


# ---- freqdomain_fir -------------------------------------------------------------------------------------------------------------------
FDFIR_N = (64, 4096, 16384)                                  # the one-launch path, the 8192 boundary's side of it, the work-buffer path
FDFIR_LAYOUTS = {"per_row": (2, False), "shared2": (2, True), "shared3": (3, True)}      # name: (chs, H shared by the item's rows)
FDFIR_TOL = 2e-5


def fdfir_arrays(n, layout, seed=0):
    """x (3, chs, T), H (3, chs or 1, bins) complex64, w (3, chs, n): T = n - 3, ragged against every tile."""
    chs, shared = FDFIR_LAYOUTS[layout]
    gen = torch.Generator().manual_seed(1000 * n + seed + chs + 10 * shared)
    T, bins = n - 3, n // 2 + 1
    x = torch.randn(3, chs, T, generator=gen)
    H = torch.view_as_complex(torch.randn(3, 1 if shared else chs, bins, 2, generator=gen))
    w = torch.randn(3, chs, n, generator=gen)
    return x, H, w


def fdfir_ref(x, H, w, n):
    """float64 on the CPU: y, gx, gH of (y * w).sum() for y = irfft(rfft(x, n) * H, n) - every row transformed on its own."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    H64 = H.detach().cpu().to(torch.complex128).requires_grad_(True)
    y = torch.fft.irfft(torch.fft.rfft(x64, n) * H64, n)
    (y * w.detach().cpu().double()).sum().backward()
    return y.detach(), x64.grad, H64.grad


def fdfir_partner(layout, ch):
    """The channel that shares a complex transform with channel ch of its item (csrc/fdfir.hip: rows 2f and 2f + 1 of the chs rows that
    share a response; a response per row, and the odd row left over, travel alone), or None."""
    chs, shared = FDFIR_LAYOUTS[layout]
    if not shared:
        return None
    mate = ch ^ 1
    return mate if mate < chs else None


# ---- fft_freqz / fft_sosfreqz ---------------------------------------------------------------------------------------------------------
FREQZ_CASES = {"sos": "freqz_sos_eq_n999", "ba": "freqz_ba_k5"}      # the existing goldens whose shapes (and first three rows) are used


def freqz_arrays(kind):
    """b (3, S, Kb), a (3, S, Ka) float64, n_fft, W (3, bins) complex128, from the first three rows of an existing golden."""
    from tests.util import load_golden
    g = load_golden(FREQZ_CASES[kind])
    n = int(g["n_fft"])
    if kind == "sos":
        s = g["sos"][:3].astype(np.float64)
        b, a = s[..., :3].copy(), s[..., 3:].copy()
    else:
        b, a = g["b"][:3, None].astype(np.float64), g["a"][:3, None].astype(np.float64)
    return b, a, n, g["W"][:3].astype(np.complex128)
