"""The level ops (loudness, loudness_normalize, peak_normalize), stereo_mix and oversampled_distortion off their nominal domain: the case
table, the draws and the float64 references of tests/test_gpu_level_mix_input_domain.py (GPU) and
tests/test_level_mix_input_domain_cpu.py (the references' own behaviour, without a GPU). References: tests/bs1770_restated.py,
tests/oversampled_distortion_restated.py and tests/stereo_mix_ref.py, each run on the SAME off-domain input as the kernels.

The contract: an output is non-finite exactly where the reference's is; finite outputs hold the bound of the op's existing parity test;
a neighbouring batch item keeps its bits. Bounds, with the lines they come from:
  loudness              |L - L_ref| / max(1, |L_ref|) <= 2e-5, gradients 1e-4 in relative L2 and of the largest entry, per row
                        (tests/test_gpu_loudness.py:15, L_TOL and GRAD_TOL, imported by the GPU test)
  peak_normalize        y 3e-7 of the largest entry, gradient 1e-6 in relative L2 and 1e-5 of the largest entry (tests/test_gpu_loudness.py:255-256)
  stereo_mix            mix, send, grad x 2e-6 of the largest entry, control gradients 5e-5 (tests/test_gpu_stereo_mix.py:122)
  oversampled_distortion  4 x the error of the restatement's own float32 run (of the CLEAN batch), and never less than 2e-6 for y and
                        grad x, 1e-5 for grad drive_db (tests/test_gpu_oversampled_distortion.py:79-80)
Shapes are the smallest that reach each launch shape; the launch shapes are asserted through the library's size queries (which need no
GPU), not assumed."""
import functools
import warnings

import numpy as np
import torch

from tests import bs1770_restated as R
from tests import oversampled_distortion_restated as OSR
from tests import stereo_mix_ref as MR
from tests.loss_input_domain_cases import POSITIONS, items, position          # noqa: F401  (re-exported to the two test files)

NAN, INF, BIG = float("nan"), float("inf"), 1e30
VALUES = {"nan": NAN, "inf": INF, "1e30": BIG}
PEAK_TOL = dict(y=3e-7, gx_l2=1e-6, gx_max=1e-5)
MIX_VAL_TOL, MIX_CTL_TOL = 2e-6, 5e-5
OS_FLOORS = dict(y=2e-6, gx=2e-6, gdrive=1e-5)


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


def quiet(fn, *a, **k):
    """fn(*a, **k) with numpy's and scipy's complaints about non-finite arithmetic switched off: here they are results."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def split(got, ref):
    """(equal finite masks?, largest deviation on the finite entries, largest finite |ref|) of two arrays of one shape."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    gm, rm = np.isfinite(got), np.isfinite(ref)
    same = bool(np.array_equal(gm, rm))
    both = gm & rm
    if not both.any():
        return same, 0.0, 0.0
    return same, float(np.abs(got[both] - ref[both]).max()), float(np.abs(ref[both]).max())


# ---- loudness -------------------------------------------------------------------------------------------------------------------------
LOUD_RATES = (8000, 16000, 48000, 96000, 192000, 384000)      # the limits of the supported range and four rates between them
LOUD_POSITIONS = POSITIONS + ("block_end", "tail")            # + the last sample of the last complete block, and the first one after it


@functools.lru_cache(maxsize=None)
def loud_segmented_n():
    """The smallest N >= 44117 at which three rows are cut into segments (dasp_loudness_segments > 1)."""
    n = 44117
    while lib().dasp_loudness_segments(3, n) <= 1:
        n += 1
    return n


def loud_cases():
    """name -> (shape, sample rate, segmented?)."""
    return {"one_segment": ((3, 2, 9001), 8000, False), "segmented": ((3, 1, loud_segmented_n()), 44100, True),
            "five_channels": ((3, 5, 9001), 8000, False)}


LOUD_CASES = ("one_segment", "segmented", "five_channels")


def loud_position(pos, N, fs):
    H, T = R.block_sizes(fs)
    end = (R.num_blocks(N, fs) - 1) * H + T - 1
    assert end + 1 < N
    return {"block_end": end, "tail": end + 1}[pos] if pos in ("block_end", "tail") else position(pos, N)


@functools.lru_cache(maxsize=None)
def loud_draw(name):
    """(x float32, upstream gradient float32 with one value per item, sample rate), read-only."""
    shape, fs, _ = loud_cases()[name]
    rng = np.random.default_rng([21, *shape])
    x = (0.3 * rng.standard_normal(shape)).astype(np.float32)
    gL = (0.5 + rng.random(shape[0])).astype(np.float32)
    return frozen(x, gL) + (fs,)


def loud_ref(x, fs, gL):
    return quiet(R.loudness, x, fs, gL=gL)


@functools.lru_cache(maxsize=None)
def loud_clean_ref(name):
    x, gL, fs = loud_draw(name)
    r = loud_ref(x, fs, gL)
    frozen(*r.values())
    return r


def loud_poisoned(name, value, pos):
    """A copy of the case's batch with one sample of item 1 replaced; -> (x, channel, index)."""
    x, _, fs = loud_draw(name)
    x = np.array(x)
    ch = LOUD_POSITIONS.index(pos) % x.shape[1]
    j = loud_position(pos, x.shape[-1], fs)
    x[1, ch, j] = VALUES[value]
    return x, ch, j


LOUD_LEVELS = ("gates", "zeros", "zero_head", "zero_tail", "underflow")


@functools.lru_cache(maxsize=None)
def loud_level_draw(kind):
    """(2, 2, 20001) at 8 kHz, item 1 an ordinary signal in every case. Item 0 - "gates": 0.3 randn, 25 dB down from 0.8 s on and at
    1e-5 from sample 15300 on, so that there are blocks above the relative gate, between the two gates and below the absolute one; "zeros":
    exact zeros; "zero_head" / "zero_tail": exact zeros before / after sample 9600 (the boundaries are placed so that every block level
    of the float64 reference is at least 0.5 LU from either gate); "underflow": 1e-25 randn, whose squares are 0 in float32 and 1e-50
    in float64 (below the absolute gate either way)."""
    rng = np.random.default_rng(31)
    x = 0.3 * rng.standard_normal((2, 2, 20001))
    if kind == "gates":
        x[0, :, 6400:15300] *= 10.0 ** (-25.0 / 20.0)
        x[0, :, 15300:] *= 1e-5 / 0.3
    elif kind == "zeros":
        x[0] = 0.0
    elif kind == "zero_head":
        x[0, :, :9600] = 0.0
    elif kind == "zero_tail":
        x[0, :, 9600:] = 0.0
    elif kind == "underflow":
        x[0] *= 1e-25 / 0.3
    else:
        raise KeyError(kind)
    gL = np.array([0.75, 1.25], np.float32)
    return frozen(x.astype(np.float32), gL) + (8000,)


@functools.lru_cache(maxsize=None)
def loud_rate_draw(fs):
    """(2, 1, 5 H + 37): two blocks and a tail at every rate."""
    H, _ = R.block_sizes(fs)
    rng = np.random.default_rng([41, fs])
    x = (0.3 * rng.standard_normal((2, 1, 5 * H + 37)) + 0.1).astype(np.float32)
    return frozen(x, np.array([0.75, 1.25], np.float32)) + (fs,)


# ---- peak_normalize -------------------------------------------------------------------------------------------------------------------
PEAK_SHAPES = ((3, 2, 4097), (3, 1, 2 ** 18 + 3))
PEAK_DB, PEAK_EPS = -6.0, 1e-8
EPS32 = float(np.float32(1e-8))                              # an eps a float32 peak can equal


def peak_segments(shape):
    rows = shape[0] * shape[1]
    nd = lib().dasp_peaknorm_scratch_doubles(rows, shape[2])
    assert nd > 0 and nd % (2 * rows) == 0
    return nd // (2 * rows)


@functools.lru_cache(maxsize=None)
def peak_draw(shape):
    rng = np.random.default_rng([51, *shape])
    return frozen((0.3 * rng.standard_normal(shape)).astype(np.float32), rng.standard_normal(shape).astype(np.float32))


def peak_ref(x, gy, peak_db=PEAK_DB, eps=PEAK_EPS):
    return quiet(R.peak_normalize, x, peak_db, eps, gy=gy)


@functools.lru_cache(maxsize=None)
def peak_level_draw():
    """(4, 1, 4097): rows of level 0.3 eps whose largest sample (index 1000) is eps / 2, eps, one float32 ulp above eps - eps being
    EPS32 - and a row of exact zeros (for eps = 0)."""
    rng = np.random.default_rng(52)
    x = (0.3 * EPS32 * rng.uniform(-1.0, 1.0, (4, 1, 4097))).astype(np.float32)
    x[0, 0, 1000] = np.float32(0.5 * EPS32)
    x[1, 0, 1000] = -np.float32(EPS32)
    x[2, 0, 1000] = np.nextafter(np.float32(EPS32), np.float32(1.0))
    x[3] = 0.0
    assert float(np.abs(x[1]).max()) == EPS32 and float(np.abs(x[2]).max()) > EPS32 > float(np.abs(x[0]).max())
    return frozen(x, rng.standard_normal(x.shape).astype(np.float32))


# ---- oversampled_distortion -----------------------------------------------------------------------------------------------------------
OS_CASES = ((2, 12), (4, 12), (8, 12), (8, 16))              # (L, H)
OS_TILES = {2: 2016, 4: 992, 8: 480}
OS_POSITIONS = POSITIONS + ("tile_end", "tile_start")        # samples T - 1 and T: the footprint spans two workgroups
OS_LEVELS = ("zeros", "1e-7")


def os_shape(L):
    T = lib().dasp_osdist_tile(L)
    assert T == OS_TILES[L]
    return (3, 2, 2 * T + 5)


def os_position(pos, L):
    T, N = OS_TILES[L], os_shape(L)[-1]
    return {"tile_end": T - 1, "tile_start": T}[pos] if pos in ("tile_end", "tile_start") else position(pos, N)


@functools.lru_cache(maxsize=None)
def os_draw(L):
    """x, drive_db (one per row), w - as tests/test_gpu_oversampled_distortion.py draws them - float32 torch tensors."""
    B, C, N = os_shape(L)
    g = torch.Generator().manual_seed(61 + 7 * B + 3 * C + N)
    return torch.rand(B, C, N, generator=g) * 2 - 1, torch.rand(B * C, generator=g) * 30 - 6, torch.randn(B, C, N, generator=g)


def os_ref(x, drive, w, L, H, dtype=torch.float64):
    """dict(y, gx, gdrive) of the restatement as float64 numpy arrays."""
    out = quiet(OSR.forward_backward, x, drive, w, L, H, dtype=dtype)
    return dict(zip(("y", "gx", "gdrive"), (t.double().numpy() for t in out)))


@functools.lru_cache(maxsize=None)
def os_clean(L, H):
    """(reference, bound per output) of the clean batch: the bound is 4 x the float32 restatement's error, and at least the floor."""
    x, drive, w = os_draw(L)
    ref, f32 = os_ref(x, drive, w, L, H), os_ref(x, drive, w, L, H, torch.float32)
    tol = {k: max(4.0 * float(np.abs(f32[k] - ref[k]).max() / np.abs(ref[k]).max()), OS_FLOORS[k]) for k in ref}
    frozen(*ref.values())
    return ref, tol


def os_poisoned(L, target, value, pos):
    """Copies of (x, drive, w) with one entry of item 1 replaced: target "x" (a sample), "gy" (a sample of w) or "drive" (the row's
    drive_db); -> (x, drive, w, flat row, index)."""
    x, drive, w = (t.clone() for t in os_draw(L))
    ch = OS_POSITIONS.index(pos) % 2
    j = os_position(pos, L)
    if target == "drive":
        drive[2 + ch] = VALUES[value]
    else:
        (x if target == "x" else w)[1, ch, j] = VALUES[value]
    return x, drive, w, 2 + ch, j


def os_footprint(j, H, N):
    """The outputs a sample j reaches: [j - 2 H, j + 2 H], clipped to the row."""
    m = np.zeros(N, bool)
    m[max(0, j - 2 * H):j + 2 * H + 1] = True
    return m


# ---- stereo_mix -----------------------------------------------------------------------------------------------------------------------
MIX_SHAPES = ((3, 5, 1501), (3, 9, 8200), (3, 1, 7))          # (B, T, N): T on either side of the 4-track unroll and of its two buffers
MIX_KEYS = ("mix", "send", "gx", "ggain", "gpan", "gsend")
MIX_LEVELS = ("zeros", "muted")


def mix_special(T):
    """The hard-left and the muted track of every item (none where there is one track only); the muted one sits in the second register
    buffer where there are nine."""
    return dict(hard=1, muted=5 if T > 8 else T - 2) if T >= 5 else {}


def mix_tracks(T):
    """name -> track to poison: the first (a generic one), the last, the muted and the hard-panned one."""
    return dict({"first_track": 0, "last_track": T - 1}, **{k + "_track": t for k, t in mix_special(T).items()}) if T > 1 else {"first_track": 0}


@functools.lru_cache(maxsize=None)
def mix_draw(shape):
    x, gain_db, pan, send_db, w0, w1 = MR.draw(*shape)
    sp = mix_special(shape[1])
    if sp:
        pan[:, sp["hard"]] = 0.0
        gain_db[:, sp["muted"]] = -np.inf
    return frozen(x, gain_db, pan, send_db, w0, w1)


def mix_ref(x, gain_db, pan, send_db, w0, w1):
    """tests/stereo_mix_ref.compose with the convention of test_hard_pans_and_a_muted_track at a hard-left pan, where the oracle's pan
    gradient is 0 / 0: the vanishing right-channel term is dropped, d l / d pan = -1 / 2 (u_L = 1, u_L' = -2 / pi)."""
    out = quiet(MR.compose, x, gain_db, pan, send_db, w0, w1 if send_db is not None else None)
    B, T, N = x.shape
    with np.errstate(all="ignore"):
        g = 10.0 ** (np.asarray(gain_db, np.float64).reshape(B, T) / 20.0)
        gpan = np.array(out["gpan"], np.float64).reshape(B, T)
        for b, t in zip(*np.nonzero(np.asarray(pan).reshape(B, T) == 0.0)):
            xt = x[b, t].astype(np.float64)
            ml = np.dot(xt, w0[b, 0].astype(np.float64))
            if send_db is not None:
                ml = ml + 10.0 ** (float(np.asarray(send_db).reshape(B, T)[b, t]) / 20.0) * np.dot(xt, w1[b, 0].astype(np.float64))
            gpan[b, t] = g[b, t] * -0.5 * ml
    out["gpan"] = gpan.reshape(-1)
    out.setdefault("gsend", None)
    return out


@functools.lru_cache(maxsize=None)
def mix_clean_ref(shape, with_send):
    x, gain_db, pan, send_db, w0, w1 = mix_draw(shape)
    out = mix_ref(x, gain_db, pan, send_db if with_send else None, w0, w1)
    frozen(*out.values())
    return out


def mix_poisoned(shape, target, value, where):
    """Copies of the draw with one entry of item 1 replaced. target "x": `where` is a sample position (track 0) or a name of
    mix_tracks (the middle sample of that track); "gain_db" / "pan" / "send_db": track 0's control; "gy": the middle sample of the
    left channel of the upstream gradient of mix. -> (arrays, track, index)."""
    x, gain_db, pan, send_db, w0, w1 = (np.array(a) for a in mix_draw(shape))
    B, T, N = shape
    t, j = 0, N // 2
    if target == "x":
        if where in POSITIONS:
            j = position(where, N)
        else:
            t = mix_tracks(T)[where]
        x[1, t, j] = VALUES[value]
    elif target == "gy":
        w0[1, 0, j] = VALUES[value]
    else:
        {"gain_db": gain_db, "pan": pan, "send_db": send_db}[target].reshape(B, T)[1, 0] = VALUES[value]
    return (x, gain_db, pan, send_db, w0, w1), t, j
