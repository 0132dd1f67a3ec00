"""The level ops (loudness, loudness_normalize, peak_normalize), stereo_mix and oversampled_distortion off their nominal domain; the
table, the draws, the references and the bounds (with the lines of the existing tests they come from) are in
tests/level_mix_input_domain_cases.py:

  A  guard bands, alignment and dirty scratch: every caller tensor as a contiguous view inside a NaN-filled allocation (16-byte and
     4-byte aligned) and as a row slice of a wider NaN tensor - bit-identical to stand-alone tensors (stereo_mix does pick its 16-byte
     loads by alignment and by N % 4; the arithmetic per sample is the same chain of fmas, so the bits are held there too); every forward
     and backward entry point through the C ABI with each output, saved buffer and scratch buffer (ysave, cov, peak, partials, scratch)
     pre-filled with NaN, then with zeros, inside a sentinel-guarded allocation sized by the library's own queries: guard words survive,
     the two runs and the Python path agree bit for bit.
  B  poisoned item: NaN, +inf, 1e30 in one sample of item 1 (first, middle, last sample; for loudness the last sample of the last block
     and the first of the tail; for the oversampling samples T - 1 and T; for the mix the last, the muted and the hard-panned track), a
     NaN control and a NaN upstream gradient. Items 0 and 2 keep every bit, forward and backward; item 1 is non-finite exactly where the
     float64 reference is and holds the op's bound elsewhere; the clean batch afterwards equals the clean batch before.
  C  levels: blocks on both sides of both loudness gates, exact zeros, zero heads and tails, squares that underflow float32; peaks below,
     at and one ulp above eps, eps = 0 on a zero row; silent and muted tracks; silence into the oversampler.
  D  loudness at 8, 16, 48, 96, 192 and 384 kHz against the restatement at that rate.

What the kernels do with such input is documented in include/dasp_hip.h and DESIGN.md section 5."""
import numpy as np
import pytest
import torch

from tests import bs1770_restated as R
from tests import level_mix_input_domain_cases as C
from tests.input_domain_cases import DEV
from tests.test_gpu_input_domain import SENTINEL, dev, guarded, misaligned, row_slice
from tests.test_gpu_loss_input_domain import Scratch
from tests.test_gpu_loudness import GRAD_TOL, L_TOL
from tests.util import record

pytestmark = pytest.mark.gpu
NAN = float("nan")
PLACEMENTS = (("16-byte aligned view", guarded), ("4-byte aligned view", misaligned), ("row slice", row_slice))


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def npy(t):
    return t.detach().cpu().double().numpy()


def placed(place, a):
    """place(a); a vector (one value per item or per row) under row_slice becomes a column of a NaN matrix - a slice of it is contiguous."""
    if place is not row_slice or np.ndim(a) != 1:
        return place(a)
    wide = torch.full((np.size(a), 5), NAN, device=DEV)
    v = wide[:, 2]
    v.copy_(dev(a))
    assert not v.is_contiguous()
    return v


def bits(a, b):
    """Equal bit for bit (NaNs included), tensors or None."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_bits(what, got, base, keys=None):
    for k in keys or base:
        assert bits(got[k], base[k]), (what, k)


def rel2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def held(what, key, got, ref, tol, worst):
    """The contract for one array of item 1: non-finite exactly where the reference is, the finite entries within tol of the largest one."""
    same, err, peak = C.split(got, ref)
    assert same, (what, key, "non-finite entries: here", int((~np.isfinite(got)).sum()), "reference", int((~np.isfinite(ref)).sum()))
    if peak == 0.0:
        assert err == 0.0, (what, key, "the reference is exactly 0", err)
        return
    worst[key] = max(worst.get(key, 0.0), err / peak)
    assert err <= tol * peak, (what, key, err / peak, tol)


# ---- the four ops: one call each, device tensors out ------------------------------------------------------------------------------------

def run_loud(D, x, gL, fs, place=dev):
    xt = place(x).requires_grad_(True)
    L = D.loudness(xt, fs)
    L.backward(placed(place, gL))
    torch.cuda.synchronize()
    return dict(L=L.detach(), gx=xt.grad)


def run_loudnorm(D, x, fs, gy, target=-20.0):
    xt = dev(x).requires_grad_(True)
    y = D.loudness_normalize(xt, fs, target)
    y.backward(dev(gy))
    torch.cuda.synchronize()
    return dict(y=y.detach(), gx=xt.grad)


def run_peak(D, x, gy, peak_db=C.PEAK_DB, eps=C.PEAK_EPS, place=dev):
    xt = place(x).requires_grad_(True)
    y = D.peak_normalize(xt, 44100, peak_db, eps)
    y.backward(place(gy))
    torch.cuda.synchronize()
    return dict(y=y.detach(), gx=xt.grad)


def run_os(D, x, drive, w, L, H, place=dev):
    xt, dt = place(x.numpy()).requires_grad_(True), placed(place, drive.numpy()).requires_grad_(True)
    y = D.oversampled_distortion(xt, 44100, dt, oversample=L, half_width=H)
    y.backward(place(w.numpy()))
    torch.cuda.synchronize()
    return dict(y=y.detach(), gx=xt.grad, gdrive=dt.grad)


def run_mix(D, arrays, with_send, place=dev):
    x, gain_db, pan, send_db, w0, w1 = arrays
    xt = place(x).requires_grad_(True)
    ct = [place(c).requires_grad_(True) for c in ((gain_db, pan, send_db) if with_send else (gain_db, pan))]
    out = D.stereo_mix(xt, C.MR.SR, *ct)
    mix, send = out if with_send else (out, None)
    torch.autograd.backward([mix, send] if with_send else [mix], [place(w0), place(w1)] if with_send else [place(w0)])
    torch.cuda.synchronize()
    return dict(mix=mix.detach(), send=None if send is None else send.detach(), gx=xt.grad, ggain=ct[0].grad, gpan=ct[1].grad,
                gsend=ct[2].grad if with_send else None)


MIX_PARAMS = [(shape, send) for shape in C.MIX_SHAPES for send in (True, False)]
mix_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("send" if v else "plain")


# ---- A: views -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.LOUD_CASES)
def test_a_loudness_inputs_as_views(D, name):
    shape, fs, segmented = C.loud_cases()[name]
    assert (C.lib().dasp_loudness_segments(shape[0] * shape[1], shape[2]) > 1) == segmented
    x, gL, _ = C.loud_draw(name)
    base = run_loud(D, x, gL, fs)
    assert torch.isfinite(base["L"]).all() and torch.isfinite(base["gx"]).all()
    for what, place in PLACEMENTS:
        same_bits((name, what), run_loud(D, x, gL, fs, place), base)


@pytest.mark.parametrize("shape", C.PEAK_SHAPES, ids=mix_id)
def test_a_peak_normalize_inputs_as_views(D, shape):
    assert C.peak_segments(shape) > 1
    x, gy = C.peak_draw(shape)
    base = run_peak(D, x, gy)
    for what, place in PLACEMENTS:
        same_bits((shape, what), run_peak(D, x, gy, place=place), base)


@pytest.mark.parametrize("L,H", C.OS_CASES)
def test_a_oversampled_distortion_inputs_as_views(D, L, H):
    x, drive, w = C.os_draw(L)
    base = run_os(D, x, drive, w, L, H)
    for what, place in PLACEMENTS:
        same_bits((L, H, what), run_os(D, x, drive, w, L, H, place), base)


@pytest.mark.parametrize("shape,with_send", MIX_PARAMS, ids=mix_id)
def test_a_stereo_mix_inputs_as_views(D, shape, with_send):
    """(N = 8200 is a multiple of 4: the stand-alone tensors and the aligned view take the 16-byte loads, the other two the scalar ones.)"""
    arrays = C.mix_draw(shape)
    base = run_mix(D, arrays, with_send)
    for what, place in PLACEMENTS:
        same_bits((shape, with_send, what), run_mix(D, arrays, with_send, place), base)


# ---- A: dirty scratch and guard words, through the C ABI ------------------------------------------------------------------------------

def abi_loudness(D, name):
    from dasp_pytorch_amd._lib import call, ptr, stream
    x, gL, fs = C.loud_draw(name)
    bs, chs, N = x.shape
    xt, gt, fs = dev(x), dev(gL), float(fs)
    nd, nb = C.lib().dasp_loudness_scratch_doubles(bs, chs, N, fs), C.lib().dasp_loudness_blocks(N, fs)
    assert nd > 0 and nb == R.num_blocks(N, fs)

    def go(out):
        scratch, L = out("scratch", nd, torch.float64), out("L", bs)
        ysave, cov = out("ysave", bs * chs * N), out("cov", bs * chs * (nb + 3))
        call("dasp_loudness_forward", ptr(xt), ptr(scratch), ptr(L), ptr(ysave), ptr(cov), bs, chs, N, fs, stream())
        scratch_b, gx = out("scratch_backward", nd, torch.float64), out("gx", bs * chs * N)
        call("dasp_loudness_backward", ptr(ysave), ptr(cov), ptr(gt), ptr(scratch_b), ptr(gx), bs, chs, N, fs, stream())
        scratch_m, Lm = out("scratch_meter", nd, torch.float64), out("L_meter", bs)           # metering only: nothing saved
        call("dasp_loudness_forward", ptr(xt), ptr(scratch_m), ptr(Lm), ptr(None), ptr(None), bs, chs, N, fs, stream())
        return dict(L=L, ysave=ysave, cov=cov, gx=gx, L_meter=Lm)
    py = run_loud(D, x, gL, fs)
    return go, dict(L=py["L"], L_meter=py["L"], gx=py["gx"])


def abi_peak(D, shape):
    from dasp_pytorch_amd._lib import call, ptr, stream
    x, gy = C.peak_draw(shape)
    rows, N = shape[0] * shape[1], shape[2]
    xt, gt = dev(x), dev(gy)
    nd = C.lib().dasp_peaknorm_scratch_doubles(rows, N)

    def go(out):
        scratch, peak, y = out("scratch", nd, torch.float64), out("peak", 2 * rows, torch.float64), out("y", rows * N)
        call("dasp_peaknorm_forward", ptr(xt), ptr(scratch), ptr(peak), ptr(y), rows, N, C.PEAK_DB, C.PEAK_EPS, stream())
        scratch_b, gx = out("scratch_backward", nd, torch.float64), out("gx", rows * N)
        call("dasp_peaknorm_backward", ptr(xt), ptr(gt), ptr(peak), ptr(scratch_b), ptr(gx), rows, N, C.PEAK_DB, C.PEAK_EPS, stream())
        return dict(y=y, peak=peak, gx=gx)
    return go, run_peak(D, x, gy)


def abi_os(D, L, H):
    from dasp_pytorch_amd import functional
    from dasp_pytorch_amd._lib import call, ptr, stream
    x, drive, w = C.os_draw(L)
    B, Cc, N = x.shape
    xt, dt, wt = x.to(DEV), drive.to(DEV), w.to(DEV)
    taps = functional._oversampling_taps_f32(L, H, 8.0, 0.9)
    npart = C.lib().dasp_osdist_partial_floats(B * Cc, N, L)
    assert npart == 3 * B * Cc

    def go(out):
        y = out("y", B * Cc * N)
        call("dasp_osdist_forward", ptr(xt), ptr(dt), taps, ptr(y), B, Cc, N, L, H, stream())
        gx, gdrive, partials = out("gx", B * Cc * N), out("gdrive", B * Cc), out("partials", npart)
        call("dasp_osdist_backward", ptr(xt), ptr(dt), taps, ptr(wt), ptr(gx), ptr(gdrive), ptr(partials), B, Cc, N, L, H, stream())
        return dict(y=y, gx=gx, gdrive=gdrive)
    return go, run_os(D, x, drive, w, L, H)


def abi_mix(D, shape, with_send):
    from dasp_pytorch_amd._lib import call, ptr, stream
    arrays = C.mix_draw(shape)
    B, T, N = shape
    xt, gt, pt, st, w0, w1 = (dev(a) for a in arrays)
    if not with_send:
        st = w1 = None
    npart = C.lib().dasp_stereo_mix_partial_floats(B, T, N, int(with_send))
    assert npart > 0

    def go(out):
        mix, send = out("mix", B * 2 * N), (out("send", B * 2 * N) if with_send else None)
        call("dasp_stereo_mix_forward", ptr(xt), ptr(gt), ptr(pt), ptr(st), ptr(mix), ptr(send), B, T, N, stream())
        gx, ggain, gpan, partials = out("gx", B * T * N), out("ggain", B * T), out("gpan", B * T), out("partials", npart)
        gsend = out("gsend", B * T) if with_send else None
        call("dasp_stereo_mix_backward", ptr(xt), ptr(gt), ptr(pt), ptr(st), ptr(w0), ptr(w1), ptr(gx), ptr(ggain), ptr(gpan), ptr(gsend),
             ptr(partials), B, T, N, stream())
        res = dict(mix=mix, gx=gx, ggain=ggain, gpan=gpan)
        if with_send:
            res.update(send=send, gsend=gsend)
        return res
    return go, {k: v for k, v in run_mix(D, arrays, with_send).items() if v is not None}


ABI_CALLS = dict(
    [(f"loudness {n}", lambda D, n=n: abi_loudness(D, n)) for n in C.LOUD_CASES]
    + [(f"peak_normalize {mix_id(s)}", lambda D, s=s: abi_peak(D, s)) for s in C.PEAK_SHAPES]
    + [(f"oversampled_distortion L={L} H={H}", lambda D, L=L, H=H: abi_os(D, L, H)) for L, H in C.OS_CASES]
    + [(f"stereo_mix {mix_id(s)} {mix_id(w)}", lambda D, s=s, w=w: abi_mix(D, s, w)) for s, w in MIX_PARAMS])


@pytest.mark.parametrize("name", list(ABI_CALLS))
def test_a_dirty_scratch_and_guard_words(D, name):
    """Loudness has "nothing to zero" (csrc/loudness.hip): with its scratch full of NaN the gate must read no partial bin a wave did not
    write; likewise the peak partials, the per-tile partials of the oversampler's drive gradient and the mix's per-segment partials."""
    assert SENTINEL == 0x7FC0DEAD
    go, python_path = ABI_CALLS[name](D)
    runs = []
    for fill in (NAN, 0.0):
        out = Scratch(fill)
        res = go(out)
        torch.cuda.synchronize()
        out.check((name, fill))
        runs.append({k: v.clone() for k, v in res.items()})
    dirty, zeroed = runs
    for k, v in dirty.items():
        assert bool(torch.isfinite(v).all()), (name, k, "a slot that is read but never written, or an output left unwritten")
        assert bits(v, zeroed[k]), (name, k, "depends on what the buffers held before the call")
    for k, v in python_path.items():
        assert bits(dirty[k].view(v.shape), v), (name, k, "the C ABI and the Python path disagree")


# ---- B: a poisoned item ---------------------------------------------------------------------------------------------------------------

def check_loud_item(what, got, ref, worst, rows=None):
    """Item 1 of a loudness call against the reference: L, then every channel row of the gradient (`rows`: only these)."""
    L, Lr = float(npy(got["L"])[1]), float(ref["L"][1])
    assert np.isfinite(L) == np.isfinite(Lr), (what, "L", L, Lr)
    if np.isfinite(Lr):
        e = abs(L - Lr) / max(1.0, abs(Lr))
        worst["L"] = max(worst.get("L", 0.0), e)
        assert e <= L_TOL, (what, "L", L, Lr)
    else:
        assert L == Lr or (L != L and Lr != Lr), (what, "L", L, Lr)
    g, gr = npy(got["gx"])[1], ref["grad"][1]
    for ch in range(g.shape[0]) if rows is None else rows:
        held(what + (ch,), "grad", g[ch], gr[ch], GRAD_TOL, worst)
        if np.isfinite(gr[ch]).all() and gr[ch].any():
            e = rel2(g[ch], gr[ch])
            worst["grad_l2"] = max(worst.get("grad_l2", 0.0), e)
            assert e <= GRAD_TOL, (what, ch, "grad rel L2", e)


def neighbours_keep_their_bits(what, got, base, keys=None):
    for k in keys or base:
        if base[k] is not None:
            assert bits(got[k][0], base[k][0]) and bits(got[k][2], base[k][2]), (what, k, "items 0 and 2")


@pytest.mark.parametrize("value", list(C.VALUES))
@pytest.mark.parametrize("name", C.LOUD_CASES)
def test_b_loudness_poisoned_item(D, name, value):
    """L of item 1 and the gradient rows, as the restatement evaluated with IEEE comparisons has them: a NaN block fails every gate
    comparison (the masked mean of the docstring), so a NaN in the middle of an item leaves L finite and the row's gradient NaN; an item
    with no block past the gates has L = -inf and a gradient of exactly 0, whatever its samples. For 1e30 only L is held here: the
    gradient is in test_b_loudness_gradient_of_an_item_with_a_1e30_sample."""
    x, gL, fs = C.loud_draw(name)
    base = run_loud(D, x, gL, fs)
    worst = {}
    check_loud_item((name, "clean"), base, C.loud_clean_ref(name), worst)
    for pos in C.LOUD_POSITIONS:
        bad, ch, j = C.loud_poisoned(name, value, pos)
        got, ref = run_loud(D, bad, gL, fs), C.loud_ref(bad, fs, gL)
        what = (name, value, pos)
        neighbours_keep_their_bits(what, got, base)
        check_loud_item(what, got, ref, worst, rows=() if value == "1e30" else None)
    same_bits((name, value, "the clean batch afterwards"), run_loud(D, x, gL, fs), base)
    record(f"level_mix_input_domain_b_loudness[{name},{value}]", **worst)


# 1e30 in an item: L is 567 LUFS and dL/dx is 3e-31 at its largest - representable, but the coverage weights the backward pass reads are
# stored as float32 and (10 / ln 10) / (|J| P T) = 1e-61 is not: they are 0 and the kernel's gradient is exactly 0. The bound (1e-4 of
# the reference's largest entry, per row) stays as it is.
OVERFLOW_GRAD_MISSES = "1e30 sample: the float32 coverage weights underflow (1e-61) and the gradient is exactly 0 in both rows of the item, " \
                       "against a reference whose largest entry is 1.254e-29 in the row that holds the sample and 1.254e-59 in the other"


@pytest.mark.xfail(strict=True, reason=OVERFLOW_GRAD_MISSES)
def test_b_loudness_gradient_of_an_item_with_a_1e30_sample(D):
    """(3, 2, 9001) at 8 kHz, 1e30 at the middle sample of item 1. Measured on an MI355X: largest |gradient| per row here 0 and 0, in
    the float64 restatement 1.254e-59 and 1.254e-29 - an error of 100 % of the largest entry against a bound of 1e-4. L itself is held
    (test_b_loudness_poisoned_item: 567.174 LUFS to 5.2e-8)."""
    x, gL, fs = C.loud_draw("one_segment")
    bad, ch, j = C.loud_poisoned("one_segment", "1e30", "mid")
    got, ref = run_loud(D, bad, gL, fs), C.loud_ref(bad, fs, gL)
    g, gr = npy(got["gx"])[1], ref["grad"][1]
    record("level_mix_input_domain_b_loudness_1e30_gradient", ours_max=np.abs(g).max(1), reference_max=np.abs(gr).max(1))
    check_loud_item(("one_segment", "1e30", "mid"), got, ref, {})


@pytest.mark.parametrize("name", C.LOUD_CASES)
def test_b_loudness_nan_upstream_gradient_and_normalize(D, name):
    """A NaN upstream gradient of item 1 poisons that item's gradient only; loudness_normalize on a batch whose item 1 holds a NaN, a
    +inf or a 1e30 sample leaves items 0 and 2 at their clean bits, values and gradients."""
    x, gL, fs = C.loud_draw(name)
    base = run_loud(D, x, gL, fs)
    gb = np.array(gL)
    gb[1] = NAN
    got = run_loud(D, x, gb, fs)
    neighbours_keep_their_bits((name, "gL"), got, base)
    assert bits(got["L"], base["L"]) and bool(torch.isnan(got["gx"][1]).all())
    assert np.isnan(C.loud_ref(x, fs, gb)["grad"][1]).all()
    gy = np.random.default_rng(22).standard_normal(x.shape).astype(np.float32)
    clean = run_loudnorm(D, x, fs, gy)
    assert torch.isfinite(clean["y"]).all() and torch.isfinite(clean["gx"]).all()
    for value in C.VALUES:
        bad, ch, j = C.loud_poisoned(name, value, "mid")
        neighbours_keep_their_bits((name, value, "loudness_normalize"), run_loudnorm(D, bad, fs, gy), clean)
    same_bits((name, "the clean batch afterwards"), run_loudnorm(D, x, fs, gy), clean)


def check_peak_rows(what, got, ref, worst):
    for k, tol in (("y", C.PEAK_TOL["y"]), ("gx", C.PEAK_TOL["gx_max"])):
        g = npy(got[k])
        for row, (G, Rr) in enumerate(zip(g.reshape(-1, g.shape[-1]), ref[k].reshape(-1, g.shape[-1]))):
            held(what + (row,), k, G, Rr, tol, worst)
            if k == "gx" and np.isfinite(Rr).all() and Rr.any():
                e = rel2(G, Rr)
                worst["gx_l2"] = max(worst.get("gx_l2", 0.0), e)
                assert e <= C.PEAK_TOL["gx_l2"], (what, row, e)


@pytest.mark.parametrize("value", list(C.VALUES))
@pytest.mark.parametrize("shape", C.PEAK_SHAPES, ids=mix_id)
def test_b_peak_normalize_poisoned_row(D, shape, value):
    """A row that holds a NaN has a NaN peak (torch.max, and the docstring's expression): y and the gradient of the row are NaN
    throughout. +inf: y is 0 with a NaN at the sample, the gradient 0 with a NaN at the index of the maximum. 1e30: finite, at the bound."""
    x, gy = C.peak_draw(shape)
    base = run_peak(D, x, gy)
    worst = {}
    ref = dict(zip(("y", "gx"), C.peak_ref(x, gy)))
    check_peak_rows((shape, "clean"), base, ref, worst)
    for pos in C.POSITIONS:
        bad = np.array(x)
        ch = C.POSITIONS.index(pos) % shape[1]
        bad[1, ch, C.position(pos, shape[2])] = C.VALUES[value]
        got = run_peak(D, bad, gy)
        what = (shape, value, pos)
        neighbours_keep_their_bits(what, got, base)
        for k in base:
            for c in range(shape[1]):
                if c != ch:
                    assert bits(got[k][1, c], base[k][1, c]), (what, k, "the other row of item 1")
        check_peak_rows(what, got, dict(zip(("y", "gx"), C.peak_ref(bad, gy))), worst)
    gb = np.array(gy)
    gb[1, 0, shape[2] // 2] = NAN                            # a NaN upstream gradient: NaN there, and (sum g x) at the index of the maximum
    got = run_peak(D, x, gb)
    neighbours_keep_their_bits((shape, "gy"), got, base)
    assert bits(got["y"], base["y"])
    check_peak_rows((shape, "gy"), got, dict(zip(("y", "gx"), C.peak_ref(x, gb))), worst)
    same_bits((shape, value, "the clean batch afterwards"), run_peak(D, x, gy), base)
    record(f"level_mix_input_domain_b_peak[{mix_id(shape)},{value}]", **worst)


def check_os_item(what, got, ref, tol, worst):
    for k in ("y", "gx"):
        g, r = npy(got[k]), ref[k]
        peak = np.abs(r[np.isfinite(r)]).max()
        same, err, _ = C.split(g[1], r[1])
        assert same, (what, k, "non-finite outputs: here", int((~np.isfinite(g[1])).sum()), "reference", int((~np.isfinite(r[1])).sum()))
        worst[k] = max(worst.get(k, 0.0), err / peak)
        assert err <= tol[k] * peak, (what, k, err / peak, tol[k])
    held(what, "gdrive", npy(got["gdrive"]), ref["gdrive"], tol["gdrive"], worst)


@pytest.mark.parametrize("value", list(C.VALUES))
@pytest.mark.parametrize("L,H", C.OS_CASES)
def test_b_oversampled_distortion_poisoned_item(D, L, H, value):
    """One sample of a row of item 1. NaN: y and grad x are NaN on [j - 2 H, j + 2 H] and nowhere else; +inf and 1e30: tanh saturates,
    sech^2 is 0 - y and grad x are finite everywhere (a zero tap must not meet the sample: 0 x inf); grad drive_db of the row is NaN
    for NaN and +inf. Outside the footprint the row keeps the clean run's bits."""
    x, drive, w = C.os_draw(L)
    base = run_os(D, x, drive, w, L, H)
    ref, tol = C.os_clean(L, H)
    worst = {}
    check_os_item((L, H, "clean"), base, ref, tol, worst)
    N = x.shape[-1]
    for pos in C.OS_POSITIONS:
        xb, db, wb, row, j = C.os_poisoned(L, "x", value, pos)
        got, want = run_os(D, xb, db, wb, L, H), C.os_ref(xb, db, wb, L, H)
        what = (L, H, value, pos)
        neighbours_keep_their_bits(what, got, base, ("y", "gx"))
        keep = torch.arange(6) != row
        assert bits(got["gdrive"][keep], base["gdrive"][keep]), (what, "gdrive of the other rows")
        check_os_item(what, got, want, tol, worst)
        away = torch.from_numpy(~C.os_footprint(j, H, N)).to(DEV)
        for k in ("y", "gx"):
            assert bits(got[k].view(6, N)[row][away], base[k].view(6, N)[row][away]), (what, k, "outside the footprint")
            assert bits(got[k].view(6, N)[row ^ 1], base[k].view(6, N)[row ^ 1]), (what, k, "the other row of item 1")
    same_bits((L, H, value, "the clean batch afterwards"), run_os(D, x, drive, w, L, H), base)
    record(f"level_mix_input_domain_b_osdist[L={L},H={H},{value}]", **worst)


@pytest.mark.parametrize("L,H", C.OS_CASES)
def test_b_oversampled_distortion_nan_control_and_upstream_gradient(D, L, H):
    x, drive, w = C.os_draw(L)
    base = run_os(D, x, drive, w, L, H)
    _, tol = C.os_clean(L, H)
    N = x.shape[-1]
    worst = {}
    for target, pos in (("drive", "mid"), ("gy", "first"), ("gy", "tile_end"), ("gy", "tile_start"), ("gy", "last")):
        xb, db, wb, row, j = C.os_poisoned(L, target, "nan", pos)
        got, want = run_os(D, xb, db, wb, L, H), C.os_ref(xb, db, wb, L, H)
        what = (L, H, target, pos)
        neighbours_keep_their_bits(what, got, base, ("y", "gx"))
        check_os_item(what, got, want, tol, worst)
        if target == "gy":
            assert bits(got["y"], base["y"]), what
            away = torch.from_numpy(~C.os_footprint(j, H, N)).to(DEV)
            assert bits(got["gx"].view(6, N)[row][away], base["gx"].view(6, N)[row][away]), (what, "outside the footprint")
        else:
            assert bool(torch.isnan(got["y"].view(6, N)[row]).all()) and bool(torch.isnan(got["gx"].view(6, N)[row]).all())
    same_bits((L, H, "the clean batch afterwards"), run_os(D, x, drive, w, L, H), base)


def check_mix_item(what, got, ref, worst):
    for k in C.MIX_KEYS:
        if ref[k] is None:
            assert got[k] is None
            continue
        g, r = npy(got[k]), np.asarray(ref[k], np.float64)
        if k in ("mix", "send", "gx"):
            held(what, k, g[1], r[1], C.MIX_VAL_TOL, worst)
        else:
            B = g.shape[0]
            g, r = g.reshape(B, -1), r.reshape(B, -1)
            same, err, _ = C.split(g[1], r[1])
            assert same, (what, k, g[1], r[1])
            peak = np.abs(r[np.isfinite(r)]).max()
            worst[k] = max(worst.get(k, 0.0), err / peak)
            assert err <= C.MIX_CTL_TOL * peak, (what, k, err / peak)


@pytest.mark.parametrize("value", list(C.VALUES))
@pytest.mark.parametrize("shape,with_send", MIX_PARAMS, ids=mix_id)
def test_b_stereo_mix_poisoned_item(D, shape, with_send, value):
    """One sample of one track of item 1 - track 0 at the first, middle and last sample, then the last, the muted and the hard-panned
    track: it reaches that sample of both channels of the item's mix and send (0 x NaN for the muted and the hard-panned track) and
    nothing else; grad x does not see x and keeps every bit; only that track's control gradients move."""
    B, T, N = shape
    clean = C.mix_draw(shape)
    base = run_mix(D, clean, with_send)
    worst = {}
    check_mix_item((shape, with_send, "clean"), base, C.mix_clean_ref(shape, with_send), worst)
    for where in C.POSITIONS + tuple(k for k in C.mix_tracks(T) if k != "first_track"):
        arrays, t, j = C.mix_poisoned(shape, "x", value, where)
        got = run_mix(D, arrays, with_send)
        want = C.mix_ref(*arrays[:3], arrays[3] if with_send else None, *arrays[4:])
        what = (shape, with_send, value, where)
        neighbours_keep_their_bits(what, got, base)
        check_mix_item(what, got, want, worst)
        assert bits(got["gx"], base["gx"]), (what, "grad x")
        away = torch.ones(N, dtype=torch.bool, device=DEV)
        away[j] = False
        for k in ("mix", "send") if with_send else ("mix",):
            assert bits(got[k][1][:, away], base[k][1][:, away]), (what, k, "the other samples of item 1")
        others = torch.arange(T) != t
        for k in ("ggain", "gpan", "gsend") if with_send else ("ggain", "gpan"):
            assert bits(got[k].view(B, T)[1][others], base[k].view(B, T)[1][others]), (what, k, "the other tracks of item 1")
    same_bits((shape, with_send, value, "the clean batch afterwards"), run_mix(D, clean, with_send), base)
    record(f"level_mix_input_domain_b_mix[{mix_id(shape)},{mix_id(with_send)},{value}]", **worst)


@pytest.mark.parametrize("shape,with_send", MIX_PARAMS, ids=mix_id)
def test_b_stereo_mix_nan_control_and_upstream_gradient(D, shape, with_send):
    clean = C.mix_draw(shape)
    base = run_mix(D, clean, with_send)
    worst = {}
    for target in ("gain_db", "pan", "send_db", "gy") if with_send else ("gain_db", "pan", "gy"):
        arrays, t, j = C.mix_poisoned(shape, target, "nan", None)
        got = run_mix(D, arrays, with_send)
        want = C.mix_ref(*arrays[:3], arrays[3] if with_send else None, *arrays[4:])
        what = (shape, with_send, target)
        neighbours_keep_their_bits(what, got, base)
        check_mix_item(what, got, want, worst)
    same_bits((shape, with_send, "the clean batch afterwards"), run_mix(D, clean, with_send), base)


# ---- C: levels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", C.LOUD_LEVELS)
def test_c_loudness_levels(D, kind):
    x, gL, fs = C.loud_level_draw(kind)
    ref = C.loud_ref(x, fs, gL)
    assert ref["margin"].min() >= 0.5                        # the float32 and float64 gate sets cannot differ (tests/test_gpu_loudness.py:104)
    got = run_loud(D, x, gL, fs)
    L, g = npy(got["L"]), npy(got["gx"])
    worst = {}
    for i in range(2):
        assert np.isfinite(g[i]).all(), (kind, i)
        if np.isfinite(ref["L"][i]):
            e = abs(L[i] - ref["L"][i]) / max(1.0, abs(ref["L"][i]))
            e2, em = rel2(g[i], ref["grad"][i]), float(np.abs(g[i] - ref["grad"][i]).max() / np.abs(ref["grad"][i]).max())
            worst.update(L=max(worst.get("L", 0.0), e), grad_l2=max(worst.get("grad_l2", 0.0), e2), grad_max=max(worst.get("grad_max", 0.0), em))
            assert e <= L_TOL and max(e2, em) <= GRAD_TOL, (kind, i, e, e2, em)
        else:
            assert L[i] == -np.inf and not g[i].any(), (kind, i, L[i])
    record(f"level_mix_input_domain_c_loudness[{kind}]", **worst, blocks=ref["nb"][0], above_absolute=ref["nA"][0], above_relative=ref["nJ"][0])


def test_c_peak_normalize_at_the_eps_clamp(D):
    """Peaks of eps / 2, eps and one float32 ulp above eps with eps = float32(1e-8), then eps = 0 with a row of exact zeros (y NaN, the
    gradient +-inf, as the closed form has them)."""
    x, gy = C.peak_level_draw()
    worst = {}
    for eps in (C.EPS32, 0.0):
        got = run_peak(D, x, gy, 0.0, eps)
        ref = dict(zip(("y", "gx"), C.peak_ref(x, gy, 0.0, eps)))
        check_peak_rows(("eps", eps), got, ref, worst)
        if eps == 0.0:
            assert bool(torch.isnan(got["y"][3]).all()) and bool(torch.isinf(got["gx"][3]).all())
            assert np.array_equal(np.sign(npy(got["gx"])[3]), np.sign(ref["gx"][3]))
    record("level_mix_input_domain_c_peak", **worst)


@pytest.mark.parametrize("kind", C.OS_LEVELS)
@pytest.mark.parametrize("L,H", C.OS_CASES)
def test_c_oversampled_distortion_silence(D, L, H, kind):
    x, drive, w = C.os_draw(L)
    x = torch.zeros_like(x) if kind == "zeros" else x * 1e-7
    got, ref = run_os(D, x, drive, w, L, H), C.os_ref(x, drive, w, L, H)
    _, tol = C.os_clean(L, H)
    worst = {}
    for k in ("y", "gx", "gdrive"):
        held((L, H, kind), k, npy(got[k]), ref[k], tol[k], worst)
    if kind == "zeros":
        assert not got["y"].any() and not got["gdrive"].any()
    record(f"level_mix_input_domain_c_osdist[L={L},H={H},{kind}]", **worst)


@pytest.mark.parametrize("kind", C.MIX_LEVELS)
@pytest.mark.parametrize("shape,with_send", MIX_PARAMS, ids=mix_id)
def test_c_stereo_mix_silence(D, shape, with_send, kind):
    x, gain_db, pan, send_db, w0, w1 = (np.array(a) for a in C.mix_draw(shape))
    if kind == "zeros":
        x[:] = 0.0
    else:
        gain_db[:] = -np.inf
    arrays = (x, gain_db, pan, send_db, w0, w1)
    got = run_mix(D, arrays, with_send)
    want = C.mix_ref(x, gain_db, pan, send_db if with_send else None, w0, w1)
    worst = {}
    for k in C.MIX_KEYS:
        if want[k] is not None:
            held((shape, with_send, kind), k, npy(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1),
                 C.MIX_VAL_TOL if k in ("mix", "send", "gx") else C.MIX_CTL_TOL, worst)
    assert not got["mix"].any() and not got["ggain"].any() and not got["gpan"].any()
    assert (not got["gx"].any()) == (kind == "muted")


# ---- D: loudness at other sample rates ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", C.LOUD_RATES)
def test_d_loudness_at_every_rate(D, fs):
    """8 kHz and 384 kHz are the limits of the supported range; at 384 kHz the high-pass poles sit at radius 0.9997."""
    x, gL, _ = C.loud_rate_draw(fs)
    ref = C.loud_ref(x, fs, gL)
    assert ref["nb"][0] == 2 and ref["margin"].min() >= 0.5
    got = run_loud(D, x, gL, fs)
    L, g = npy(got["L"]), npy(got["gx"])
    el = float(np.max(np.abs(L - ref["L"]) / np.maximum(1.0, np.abs(ref["L"]))))
    e2, em = rel2(g, ref["grad"]), float(np.abs(g - ref["grad"]).max() / np.abs(ref["grad"]).max())
    record(f"level_mix_input_domain_d_loudness[{fs}]", L=el, grad_l2=e2, grad_max=em)
    assert np.isfinite(L).all() and np.isfinite(g).all()
    assert el <= L_TOL and max(e2, em) <= GRAD_TOL, (fs, el, e2, em)
