"""The losses and spectral ops off their nominal domain - the three STFT-loss layouts, the time-domain losses, the A-weighting FIR exports,
signal.freqdomain_fir and fft_freqz / fft_sosfreqz; the table, the references and the bounds (with the lines of the existing tests they
come from) are in tests/loss_input_domain_cases.py:

  A  non-finite input: one sample of item 1 set to NaN or +inf (first, middle and last sample; the input, then the target). The loss is
     non-finite exactly when the float64 restatement's is; gradient rows the restatement keeps finite match it, rows it poisons are
     poisoned; the neighbours of the time-domain losses, of freqdomain_fir and of freqz keep their clean values bit for bit (fixed
     summation order), those of the STFT gradients to the bound of two runs against each other (float atomics); the clean batch
     afterwards is bit-identical to the clean batch before. fmaxf(x, eps) in place of torch.clamp(min=eps) fails here: it reads a frame
     with a NaN in it as silence and returns a finite loss.
  B  dirty scratch and guard words through the C ABI: every output and scratch buffer pre-filled with NaN, then with zeros, inside a
     sentinel-filled allocation and sized by the library's own size queries; the guard words survive and the two runs agree.
  C  views: every signal input as a 4-byte-offset view in a NaN-filled allocation and as a row slice of a wider NaN tensor, through the
     public functions (the bindings' .contiguous() paths). No kernel of these ops picks a variant by alignment (scalar gathers in the
     STFT kernels, staged scalar loads in fdfir, fp64 coefficient loads in freqz), so every forward value is bit-identical to the
     stand-alone call; the STFT gradients are held to the atomics bound (1e-5, tests/test_gpu_mrstft_options.py:208).
  D  silence and the eps clamp (STFT family): zeros, identical signals, every bin below eps (gradient exactly 0), bins on both sides of eps."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_input_domain_cases as C
from tests.input_domain_cases import DEV, GUARD
from tests.test_gpu_input_domain import SENTINEL, OutBuf, dev, guarded, misaligned, row_slice
from tests.util import linf_peak, record

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def rel2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def npy(t):
    return t.detach().cpu().double().numpy()


# ---- A: the STFT losses ---------------------------------------------------------------------------------------------------------------

def run_stft(D, case, p, t, place_p=dev, place_t=dev):
    pt, tt = place_p(p).requires_grad_(True), place_t(t).requires_grad_(True)
    loss = case.loss_fn(D)(pt, tt)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), npy(pt.grad), npy(tt.grad)


def check_stft_rows(case, what, got, ref, worst):
    """loss at 2e-5; every gradient row of both arguments at the case's generic-input bounds."""
    assert abs(got[0] - ref[0]) <= C.LOSS_TOL * abs(ref[0]), (case.name, what, got[0], ref[0])
    worst["loss"] = max(worst["loss"], abs(got[0] - ref[0]) / abs(ref[0]))
    for g, r in zip(got[1:], ref[1:]):
        for G, R in zip(C.items(g), C.items(r)):
            check_grad_row(case, what, G, R, worst)


def check_grad_row(case, what, G, R, worst):
    l2, mx = case.grad_bounds()
    assert np.isfinite(G).all(), (case.name, what, "a finite row of the reference is not finite here")
    e2, em = rel2(G, R), relmax(G, R)
    worst["grad_l2"], worst["grad_max"] = max(worst["grad_l2"], e2), max(worst["grad_max"], em)
    assert e2 < l2, (case.name, what, e2)
    if mx is not None:
        assert em < mx, (case.name, what, em)


@pytest.mark.parametrize("case", C.STFT_CASES, ids=str)
def test_a_stft_loss_with_a_non_finite_sample(D, case):
    p, t, ref = C.stft_clean(case.name)
    worst = dict(loss=0.0, grad_l2=0.0, grad_max=0.0, run_to_run=0.0)
    base = run_stft(D, case, p, t)
    check_stft_rows(case, "clean", base, ref, worst)
    other_rows = []
    for poison in C.POISONS:
        pp, tp = C.poisoned(p, t, poison)
        want = case.ref(pp, tp)
        got = run_stft(D, case, pp, tp)
        assert np.isfinite(got[0]) == np.isfinite(want[0]), (case.name, poison, "loss", got[0], want[0])
        for k, arg in ((1, "input"), (2, "target")):
            for row, (G, R, B) in enumerate(zip(C.items(got[k]), C.items(want[k]), C.items(base[k]))):
                what = poison + (arg + ".grad", row)
                if row == 1 and arg != poison[0]:
                    # the poisoned item's row of the OTHER argument: the restatement's value goes through sign(NaN) = 0 (finite, and not
                    # the clean batch's, where w_sc = 0) - recorded only
                    other_rows.append((int((~np.isfinite(G)).sum()), int((~np.isfinite(R)).sum())))
                elif np.isfinite(R).all():
                    check_grad_row(case, what, G, R, worst)
                    if case.w_sc == 0:                   # no term couples the rows: the clean batch's row, up to the order of the atomics
                        e = float(np.abs(G - B).max() / np.abs(B).max())
                        worst["run_to_run"] = max(worst["run_to_run"], e)
                        assert e <= C.ATOMICS_TOL, (case.name, what, e)
                else:
                    assert not np.isfinite(G).all(), (case.name, what, "the reference's row is poisoned, this one is finite")
    again = run_stft(D, case, p, t)
    assert again[0] == base[0], (case.name, "the clean loss after the poisoned runs", again[0], base[0])
    for a, b in zip(again[1:], base[1:]):
        assert np.abs(a - b).max() <= C.ATOMICS_TOL * np.abs(b).max()
    record(f"loss_input_domain_stft[{case.name}]", **worst, other_argument_row_nonfinite_ours=[o[0] for o in other_rows],
           other_argument_row_nonfinite_reference=[o[1] for o in other_rows])


# ---- A: the time-domain losses --------------------------------------------------------------------------------------------------------

def run_td(D, p, t, **options):
    pt, tt = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
    loss = D.losses.time_domain_loss(pt, tt, **options)
    loss.backward(torch.ones_like(loss))
    torch.cuda.synchronize()
    return npy(loss), npy(pt.grad), npy(tt.grad)


def td_loss_error(l, lo, db):
    return float(np.max(np.abs(l - lo) / (np.maximum(1.0, np.abs(lo)) if db else np.abs(lo))))


@pytest.mark.parametrize("zero_mean", [True, False])
@pytest.mark.parametrize("name", list(C.TD_CASES))
def test_a_time_domain_losses_with_a_non_finite_sample(D, name, zero_mean):
    from tests.auraloss_time_restated import DB_TERMS
    p, t = C.td_draw()
    db = name in DB_TERMS
    rows = C.TD_SHAPE[0] * C.TD_SHAPE[1]
    flat = lambda a: np.asarray(a).reshape(rows, -1)
    worst = dict(loss=0.0, grad_l2=0.0, grad_max=0.0)
    for reduction in ("none", "mean"):
        opts = C.td_keywords(name, zero_mean=zero_mean, reduction=reduction)
        base = run_td(D, p, t, **opts)
        ref = C.td_ref(p, t, name, zero_mean, reduction)
        assert td_loss_error(base[0], ref[0], db) < C.TD_LOSS_TOL
        for poison in C.POISONS:
            pp, tp = C.poisoned(p, t, poison)
            bad = 1 * C.TD_SHAPE[1] + C.POSITIONS.index(poison[2]) % C.TD_SHAPE[1]          # the flat row that holds the sample
            want = C.td_ref(pp, tp, name, zero_mean, reduction)
            got = run_td(D, pp, tp, **opts)
            what = (name, zero_mean, reduction) + poison
            if reduction == "none":
                L, Lr, Lb = got[0].reshape(rows), want[0].reshape(rows), base[0].reshape(rows)
                keep = np.arange(rows) != bad
                assert np.array_equal(L[keep], Lb[keep]), (what, "a clean row's loss moved")               # "no atomics": bit for bit
                assert np.isfinite(L[bad]) == np.isfinite(Lr[bad]), (what, L[bad], Lr[bad])
                if np.isfinite(Lr[bad]):                                   # (snr of a +inf prediction with zero_mean=False: 80 dB)
                    e = td_loss_error(L[bad], Lr[bad], db)
                    worst["loss"] = max(worst["loss"], e)
                    assert e < C.TD_LOSS_TOL, (what, L[bad], Lr[bad])
            else:
                assert np.isfinite(got[0]) == np.isfinite(want[0]), (what, got[0], want[0])
            for k in (1, 2):
                for row, (G, R, B) in enumerate(zip(flat(got[k]), flat(want[k]), flat(base[k]))):
                    if row != bad:
                        assert np.array_equal(G, B), (what, k, row, "a clean row's gradient moved")
                    if np.isfinite(R).all():
                        assert np.isfinite(G).all(), (what, k, row)
                        if np.abs(R).max() == 0:
                            assert not G.any(), (what, k, row)
                            continue
                        e2, em = rel2(G, R), relmax(G, R)
                        worst["grad_l2"], worst["grad_max"] = max(worst["grad_l2"], e2), max(worst["grad_max"], em)
                        assert max(e2, em) < C.TD_GRAD_TOL, (what, k, row, e2, em)
                    else:
                        assert not np.isfinite(G).all(), (what, k, row, "the reference's row is poisoned, this one is finite")
        again = run_td(D, p, t, **opts)
        assert all(np.array_equal(a, b) for a, b in zip(again, base)), (name, zero_mean, reduction, "the clean batch after the poisoned ones")
    record(f"loss_input_domain_time[{name},zero_mean={zero_mean}]", **worst)


# ---- A: the A-weighting FIR exports ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", ["aw", "hp", "random7"])
@pytest.mark.parametrize("entry", ["dasp_fir_same_forward", "dasp_fir_same_adjoint"])
def test_a_fir_exports_with_a_non_finite_sample(D, entry, filt):
    """The 101 A-weighting taps, FIRFilter("hp")'s three (the last one 0) and 7 random ones on 3 rows of 5000 samples (three 2048-sample
    tiles): NaN / +inf at the first sample, on either side of a tile boundary, in the middle and at the last sample. Non-finite exactly in
    the ntaps-wide neighbourhood where float64 conv1d (conv_transpose1d for the adjoint) is, bit-identical to the clean run everywhere
    else. (The kernel keeps a short filter centred in 101 slots: walking the zero slots too spread a NaN over 101 outputs, 0 * NaN.)"""
    from dasp_pytorch_amd import losses
    from dasp_pytorch_amd._lib import call, ptr, stream
    from tests import auraloss_restated as ar
    h = {"aw": lambda: losses.a_weighting_taps(float(C.SR)), "hp": lambda: np.array([1.0, -0.85, 0.0], np.float32),
         "random7": lambda: np.random.default_rng(7).standard_normal(7).astype(np.float32)}[filt]()
    half = len(h) // 2
    taps = dev(h)
    rows, N = 3, 5000
    x0, x1 = C.generic((rows, N), 11)
    fn = ar.fir_same if entry.endswith("forward") else ar.fir_same_adjoint

    def go(a, b):
        ya, yb = torch.full((rows, N), NAN, device=DEV), torch.full((rows, N), NAN, device=DEV)
        call(entry, ptr(a), ptr(b), ptr(ya), ptr(yb), ptr(taps), len(h), rows, N, stream())
        torch.cuda.synchronize()
        return ya, yb
    base = go(dev(x0), dev(x1))
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()
    for value in (NAN, float("inf")):
        for pos in (0, 2047, 2048, N // 2, N - 1):
            bad = x0.copy()
            bad[1, pos] = value
            ya, yb = go(dev(bad), dev(x1))
            want = fn(torch.from_numpy(bad).double(), h.astype(np.float64))
            hit = ~torch.isfinite(want)
            assert int(hit.sum()) == min(pos, half) + 1 + min(N - 1 - pos, half) and not hit[0].any() and not hit[2].any()
            assert torch.equal(~torch.isfinite(ya).cpu(), hit), (entry, filt, value, pos, int((~torch.isfinite(ya)).sum()), int(hit.sum()))
            assert torch.equal(ya[~hit.to(DEV)], base[0][~hit.to(DEV)]) and torch.equal(yb, base[1]), (entry, filt, value, pos)
    again = go(dev(x0), dev(x1))
    assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])


# ---- A: freqdomain_fir ----------------------------------------------------------------------------------------------------------------

def run_fdfir(D, x, H, w, n, place=None):
    place = place or {}
    put = lambda k, v: place.get(k, lambda a: a.to(DEV))(v)
    xt, Ht = put("x", x).requires_grad_(True), put("H", H).requires_grad_(True)
    y = D.signal.freqdomain_fir(xt, Ht, n)
    y.backward(put("gy", w))
    torch.cuda.synchronize()
    return y.detach().cpu(), xt.grad.cpu(), Ht.grad.cpu()


def nonfinite(z):
    z = z.detach()
    return ~torch.isfinite(torch.view_as_real(z)).all(-1) if z.is_complex() else ~torch.isfinite(z)


@pytest.mark.parametrize("layout", list(C.FDFIR_LAYOUTS))
@pytest.mark.parametrize("n", C.FDFIR_N)
def test_a_fdfir_with_a_non_finite_sample(D, n, layout):
    """x (3, chs, n - 3): a NaN / +inf sample of x, then a NaN of the upstream gradient, in channel 0 of item 1. Items 0 and 2 keep every
    bit of y, gx and gH. Inside item 1 (include/dasp_hip.h): the poisoned row is non-finite wherever the float64 reference's is; the row
    that shares its complex transform (channel 1 where the item's rows share one response) is non-finite throughout; a row that travels
    alone (a response per row; the third of three channels) keeps every bit. gx does not depend on x, y not on gy."""
    chs, shared = C.FDFIR_LAYOUTS[layout]
    x, H, w = C.fdfir_arrays(n, layout)
    T = x.shape[-1]
    base = run_fdfir(D, x, H, w, n)
    ref = C.fdfir_ref(x, H, w, n)
    errs = [float(linf_peak(npy(torch.view_as_real(g) if g.is_complex() else g), npy(torch.view_as_real(r) if r.is_complex() else r)).max())
            for g, r in zip(base, ref)]
    record(f"loss_input_domain_fdfir[{n},{layout}]", y=errs[0], gx=errs[1], gH=errs[2])
    assert max(errs) < C.FDFIR_TOL, errs
    mate = C.fdfir_partner(layout, 0)
    for target, value, pos in (("x", NAN, 0), ("x", NAN, T // 2), ("x", NAN, T - 1), ("x", float("inf"), T // 2), ("gy", NAN, n // 2)):
        xb, wb = x.clone(), w.clone()
        (xb if target == "x" else wb)[1, 0, pos] = value
        got = run_fdfir(D, xb, H, wb, n)
        want = C.fdfir_ref(xb, H, wb, n)
        what = (n, layout, target, value, pos)
        for g, b in zip(got, base):
            assert torch.equal(g[0], b[0]) and torch.equal(g[2], b[2]), (what, "items 0 and 2")
        hit, same = (0, 1) if target == "x" else (1, 0)            # the output the poison reaches, and the one it cannot
        assert torch.equal(got[same], base[same]), what
        assert bool(nonfinite(got[hit][1, 0])[nonfinite(want[hit][1, 0])].all()), (what, "the poisoned row")
        assert bool(nonfinite(want[hit][1, 0]).all())
        for ch in range(1, chs):
            if ch == mate:
                assert bool(nonfinite(got[hit][1, ch]).all()), (what, ch, "the row that shares the transform")
            else:
                assert torch.equal(got[hit][1, ch], base[hit][1, ch]), (what, ch, "a row that travels alone")
        gH, gHr = got[2][1], want[2][1]
        assert bool(nonfinite(gH[0])[nonfinite(gHr[0])].all()) and bool(nonfinite(gHr[0]).any()), (what, "gH")
        if not shared:
            assert torch.equal(gH[1], base[2][1, 1]), (what, "gH of the clean row")
    again = run_fdfir(D, x, H, w, n)
    assert all(torch.equal(a, b) for a, b in zip(again, base))


def test_a_fdfir_cross_talk_of_a_packed_pair(D):
    """Channel 0 at peak 1 and channel 1 at peak 1e-4 share one response and so one complex transform x0 + i x1 (n_fft = 4096, a generic
    H): the quiet row's error is held to 2e-5 (test_sweep_against_torch_fft's bound at this size) of the ITEM's largest output peak - what
    the packing guarantees (include/dasp_hip.h) - and recorded relative to its own peak, which the loud row's rounding error dominates."""
    n = 4096
    x, H, w = C.fdfir_arrays(n, "shared2", seed=1)
    x = x / x.abs().amax(-1, keepdim=True)
    x[:, 1] *= 1e-4
    y, gx, gH = run_fdfir(D, x, H, w, n)
    yr, gxr, gHr = C.fdfir_ref(x, H, w, n)
    y, gx = y.double(), gx.double()
    item_peak = yr.abs().amax((1, 2))
    quiet = (y[:, 1] - yr[:, 1]).abs().amax(-1)
    loud = (y[:, 0] - yr[:, 0]).abs().amax(-1)
    record("loss_input_domain_fdfir_cross_talk", quiet_of_item_peak=(quiet / item_peak).numpy(), quiet_of_own_peak=(quiet / yr[:, 1].abs().amax(-1)).numpy(),
           loud_of_own_peak=(loud / yr[:, 0].abs().amax(-1)).numpy())
    assert bool((quiet <= C.FDFIR_TOL * item_peak).all()) and bool((loud <= C.FDFIR_TOL * item_peak).all())
    assert float(linf_peak(gx.numpy(), gxr.numpy()).max()) < C.FDFIR_TOL             # gx does not see x: both rows at the usual bound
    assert float(linf_peak(npy(torch.view_as_real(gH)), npy(torch.view_as_real(gHr))).max()) < C.FDFIR_TOL


# ---- A: fft_freqz / fft_sosfreqz ------------------------------------------------------------------------------------------------------

def run_freqz(D, kind, b, a, n, W, dtype, place=dev):
    if kind == "sos":
        leaves = [place(np.concatenate([b, a], -1)).to(dtype).requires_grad_(True)]
        H = D.signal.fft_sosfreqz(leaves[0], n)
    else:
        leaves = [place(b[:, 0]).to(dtype).requires_grad_(True), place(a[:, 0]).to(dtype).requires_grad_(True)]
        H = D.signal.fft_freqz(leaves[0], leaves[1], n)
    (torch.conj(dev(W).to(H.dtype)) * H).real.sum().backward()
    torch.cuda.synchronize()
    return [H.detach()] + [v.grad for v in leaves]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("kind", list(C.FREQZ_CASES))
def test_a_freqz_with_a_non_finite_coefficient(D, kind, dtype):
    """Three rows; a NaN / +inf coefficient of row 1 (numerator, then denominator). Rows 0 and 2 keep every bit of H and of the
    coefficient gradients (fixed summation order); with a NaN, H of row 1 is non-finite at every bin, as the extended-precision
    evaluation's is. (With +inf the two evaluations need not agree bin by bin - inf * 0 inside a complex product - so row 1 is recorded.)"""
    from tests.freqz_exact import exact_response
    b, a, n, W = C.freqz_arrays(kind)
    base = run_freqz(D, kind, b, a, n, W, dtype)
    assert all(bool(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all()) for v in base)
    for which in ("b", "a"):
        for value in (NAN, float("inf")):
            bb, ab = b.copy(), a.copy()
            (bb if which == "b" else ab)[1, 0, 1] = value
            got = run_freqz(D, kind, bb, ab, n, W, dtype)
            for g, v in zip(got, base):
                assert torch.equal(g[0], v[0]) and torch.equal(g[2], v[2]), (kind, dtype, which, value)
            bad = nonfinite(got[0][1])
            if value != value:
                assert not np.isfinite(exact_response(bb, ab, n)[1]).any() and bool(bad.all()), (kind, dtype, which)
            else:
                record(f"loss_input_domain_freqz_inf[{kind},{dtype},{which}]", nonfinite_bins_ours=int(bad.sum()),
                       nonfinite_bins_reference=int((~np.isfinite(exact_response(bb, ab, n)[1])).sum()))
    again = run_freqz(D, kind, b, a, n, W, dtype)
    assert all(torch.equal(x, y) for x, y in zip(again, base))


# ---- B: dirty scratch and guard words, through the C ABI ------------------------------------------------------------------------------

class Scratch:
    """Hands out buffers of a call, each a view GUARD words into its own sentinel-filled allocation and pre-filled with `fill`."""

    def __init__(self, fill):
        self.fill, self.bufs = fill, {}

    def __call__(self, key, n, dtype=torch.float32):
        words = int(n) * (2 if dtype == torch.float64 else 1)
        ob = OutBuf(words, GUARD)
        v = ob.view.view(dtype) if dtype != torch.float32 else ob.view
        assert v.numel() == int(n)
        v.fill_(self.fill)
        self.bufs[key] = ob
        return v

    def check(self, what):
        for key, ob in self.bufs.items():
            ob.payload((what, key))                          # asserts both guard bands, compared as int32


def _int_arrays(res):
    return [(ctypes.c_int * len(res))(*[int(r[i]) for r in res]) for i in range(3)]


def abi_stft(halves, units, N, res, wts, n_bins=0):
    from dasp_pytorch_amd import _lib, losses
    from dasp_pytorch_amd._lib import call, ptr, stream
    prefix = "dasp_mrstft_sd_" if halves == 2 else "dasp_mrstft_"
    arr, nres = _int_arrays(res), len(res)
    p, t = (dev(v) for v in C.generic((units * halves, N), N + nres))
    tw = torch.empty(2 * 4096, dtype=torch.float32, device=DEV)
    call("dasp_mrstft_table", ptr(tw), stream())
    tables = [losses._mel_table(C.SR, r[0], n_bins, torch.device(DEV)) for r in res] if n_bins else []
    tabs = (ctypes.c_void_p * nres)(*[tb.data_ptr() for tb in tables]) if n_bins else None
    gloss = torch.tensor([1.0, 0.5][:halves], device=DEV)

    def go(out):
        nfl = getattr(_lib.lib(), prefix + "partial_floats")(units, N, nres, *arr, n_bins)
        assert nfl > 0
        partials, stats, loss = out("partials", nfl), out("stats", 4 * halves * nres), out("loss", halves)
        call(prefix + "forward", ptr(p), ptr(t), ptr(tw), tabs, ptr(partials), ptr(stats), ptr(loss), units, N, nres, *arr, C.EPS, *wts, n_bins, stream())
        grads = []
        for wrt in (0, 1):
            grads.append(out(f"grad{wrt}", units * halves * N))
            call(prefix + "backward", ptr(p), ptr(t), ptr(tw), tabs, ptr(stats), ptr(gloss), ptr(grads[-1]), units, N, nres, *arr, C.EPS, *wts, n_bins,
                 wrt, stream())
        return dict(exact=dict(loss=loss, stats=stats), atomics=dict(grad0=grads[0], grad1=grads[1]))
    return go


def abi_fdfir(n, T, chs=3, h_rows=3):
    from dasp_pytorch_amd import _lib
    from dasp_pytorch_amd._lib import call, ptr, stream
    rows, bins = h_rows * chs, n // 2 + 1
    gen = torch.Generator().manual_seed(n + T)
    x, gy = torch.randn(rows, T, generator=gen).to(DEV), torch.randn(rows, n, generator=gen).to(DEV)
    H = torch.randn(h_rows, bins, 2, generator=gen).to(DEV)
    tw = torch.empty(2 * 4096, dtype=torch.float32, device=DEV)
    call("dasp_mrstft_table", ptr(tw), stream())

    def go(out):
        nw = _lib.lib().dasp_fdfir_work_floats(rows, T, n, h_rows)
        assert nw >= 0 and (nw == 0) == (n <= 8192)
        work = out("work", nw) if nw else None
        y, gx, gH = out("y", rows * n), out("gx", rows * T), out("gH", 2 * h_rows * bins)
        call("dasp_fdfir_forward", ptr(x), ptr(H), ptr(tw), ptr(y), ptr(work), nw, rows, T, n, h_rows, stream())
        call("dasp_fdfir_backward", ptr(x), ptr(H), ptr(gy), ptr(tw), ptr(gx), ptr(gH), ptr(work), nw, rows, T, n, h_rows, stream())
        return dict(exact=dict(y=y, gx=gx, gH=gH), atomics={})
    return go


def abi_freqz(kind, dtype):
    from dasp_pytorch_amd import _lib
    from dasp_pytorch_amd._lib import call, ptr, stream
    b, a, n, W = C.freqz_arrays(kind)
    rows, S, Kb = b.shape
    Ka, bins, f64 = a.shape[2], n // 2 + 1, int(dtype == torch.float64)
    bt, at = dev(b).to(dtype), dev(a).to(dtype)
    gH = torch.view_as_real(dev(W)).to(dtype).contiguous()

    def go(out):
        nw = _lib.lib().dasp_freqz_work_doubles(rows, S, Kb, Ka, n)
        assert nw > 0
        H, work = out("H", 2 * rows * bins, dtype), out("work", nw, torch.float64)
        gb, ga = out("gb", rows * S * Kb, dtype), out("ga", rows * S * Ka, dtype)
        call("dasp_freqz_forward", ptr(bt), ptr(at), rows, S, Kb, Ka, n, f64, ptr(H), stream())
        call("dasp_freqz_backward", ptr(bt), ptr(at), ptr(gH), rows, S, Kb, Ka, n, f64, ptr(work), nw, ptr(gb), ptr(ga), stream())
        return dict(exact=dict(H=H, gb=gb, ga=ga), atomics={})
    return go


def abi_tdloss(reduction):
    from dasp_pytorch_amd import _lib
    from dasp_pytorch_amd._lib import call, ptr, stream
    p, t = C.td_draw()
    rows, N = p.shape[0] * p.shape[1], p.shape[2]
    pt, tt = dev(p).reshape(rows, N), dev(t).reshape(rows, N)
    w = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 100.0)                 # every term: all six moments are written and read
    gl = torch.linspace(0.5, 1.5, rows if reduction == 0 else 1, device=DEV)

    def go(out):
        nd = _lib.lib().dasp_tdloss_scratch_doubles(rows, N)
        assert nd > 0
        scratch, moments = out("scratch", nd, torch.float64), out("moments", 6 * rows, torch.float64)
        row_loss, loss = out("row_loss", rows), (out("loss", 1) if reduction else None)
        gp, gt = out("gpred", rows * N), out("gtarget", rows * N)
        call("dasp_tdloss_forward", ptr(pt), ptr(tt), ptr(scratch), ptr(moments), ptr(row_loss), ptr(loss), rows, N, *w, 1.0, C.EPS, 1, reduction, stream())
        call("dasp_tdloss_backward", ptr(pt), ptr(tt), ptr(moments), ptr(gl), ptr(gp), ptr(gt), rows, N, *w, 1.0, C.EPS, 1, reduction, stream())
        exact = dict(moments=moments, row_loss=row_loss, gpred=gp, gtarget=gt)
        if reduction:
            exact["loss"] = loss
        return dict(exact=exact, atomics={})
    return go


# the multi-resolution call whose resolutions have different frame-group counts (tests/test_gpu_losses.py:29): spec.groups is the 4096-point
# resolution's, and the groups past a resolution's own count are never written - the reduce kernel must not read them
RAGGED_RES = ((4096, 1024, 4096), (8, 2, 8), (512, 128, 500))
DEFAULT_RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
ABI_CALLS = {
    "mrstft default resolutions": lambda: abi_stft(1, 3, 5000, DEFAULT_RES, (1.0, 1.0, 0.0)),
    "mrstft ragged group counts": lambda: abi_stft(1, 2, 9000, RAGGED_RES, (1.0, 1.0, 1.0)),
    "mrstft 8192 + mel": lambda: abi_stft(1, 2, 9000, ((8192, 2048, 8191), (256, 64, 256)), (1.0, 1.0, 0.0), 40),
    "mrstft_sd default resolutions": lambda: abi_stft(2, 3, 5000, DEFAULT_RES, (1.0, 1.0, 0.0)),
    "mrstft_sd ragged group counts": lambda: abi_stft(2, 2, 9000, RAGGED_RES, (0.0, 1.0, 1.0)),
    "mrstft_sd 8192 + mel": lambda: abi_stft(2, 2, 9000, ((8192, 2048, 8191), (256, 64, 256)), (1.0, 1.0, 0.0), 8),
    "fdfir 64": lambda: abi_fdfir(64, 61),
    "fdfir 64 cropped": lambda: abi_fdfir(64, 69),
    "fdfir 4096": lambda: abi_fdfir(4096, 4093),
    "fdfir 16384": lambda: abi_fdfir(16384, 16381),
    "fdfir 16384 cropped, a response per row": lambda: abi_fdfir(16384, 16389, chs=1, h_rows=3),
    "freqz sos float32": lambda: abi_freqz("sos", torch.float32),
    "freqz sos float64": lambda: abi_freqz("sos", torch.float64),
    "freqz ba float32": lambda: abi_freqz("ba", torch.float32),
    "freqz ba float64": lambda: abi_freqz("ba", torch.float64),
    "tdloss none": lambda: abi_tdloss(0),
    "tdloss mean": lambda: abi_tdloss(1),
}


@pytest.mark.parametrize("name", list(ABI_CALLS))
def test_b_dirty_scratch_and_guard_words(D, name):
    """Every output and scratch buffer of the forward and the backward entry point (partials, stats, loss, grad, work, scratch, moments,
    row_loss, y, gx, gH, H, gb, ga) pre-filled with NaN, then with zeros, each GUARD words into a sentinel-filled allocation and exactly as
    large as the library's size query says: both guard bands survive, every output is finite, and the two runs agree bit for bit (the STFT
    gradients, accumulated with float atomics into a buffer the library zeroes itself: to 1e-5 of the largest entry)."""
    assert SENTINEL == 0x7FC0DEAD
    go = ABI_CALLS[name]()
    runs = []
    for fill in (NAN, 0.0):
        out = Scratch(fill)
        res = go(out)
        torch.cuda.synchronize()
        out.check((name, fill))
        runs.append({kind: {k: v.clone() for k, v in d.items()} for kind, d in res.items()})
    dirty, zeroed = runs
    for k, v in dirty["exact"].items():
        assert bool(torch.isfinite(v).all()), (name, k, "a slot that is read but never written, or an output left unwritten")
        assert torch.equal(v, zeroed["exact"][k]), (name, k)
    for k, v in dirty["atomics"].items():
        z = zeroed["atomics"][k]
        assert bool(torch.isfinite(v).all()) and float(z.abs().max()) > 0, (name, k)
        assert float((v - z).abs().max()) <= C.ATOMICS_TOL * float(z.abs().max()), (name, k)


# ---- C: views -------------------------------------------------------------------------------------------------------------------------

VIEW_CASES = ["mono-256-log+lin", "mono-1024-sc+log-mel40", "mono-2048-sc+log", "mono-8192-sc+log-aw", "sd-512-sc+log", "sd-2048-log+lin-mel40-aw"]


@pytest.mark.parametrize("name", VIEW_CASES)
def test_c_stft_inputs_as_views(D, name):
    """input and target 4 bytes into NaN-filled allocations (both, then each alone), then as row slices of wider NaN tensors: the loss
    equals the stand-alone call's bit for bit (the kernels gather sample by sample: no alignment phase), the gradients to the atomics bound."""
    case = C.STFT_BY_NAME[name]
    p, t, _ = C.stft_clean(name)
    base = run_stft(D, case, p, t)
    for what, pp, pt in (("both misaligned", misaligned, misaligned), ("input misaligned", misaligned, dev), ("target misaligned", dev, misaligned),
                         ("aligned views", guarded, guarded), ("row slices", row_slice, row_slice), ("input a row slice", row_slice, dev)):
        got = run_stft(D, case, p, t, pp, pt)
        assert got[0] == base[0], (name, what, got[0], base[0])
        for g, b in zip(got[1:], base[1:]):
            assert np.isfinite(g).all() and np.abs(g - b).max() <= C.ATOMICS_TOL * np.abs(b).max(), (name, what)


def complex_offset(z):
    """A complex64 tensor one element (8 bytes: the closest a complex view gets to a 16-byte boundary) into a NaN-filled allocation."""
    flat = guarded(np.zeros(2 * z.numel(), np.float32), GUARD + 2)
    v = torch.view_as_complex(flat.view(*z.shape, 2))
    v.copy_(z.to(DEV))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def complex_slice(z):
    wide = torch.full(tuple(z.shape[:-1]) + (z.shape[-1] + 5,), complex(NAN, NAN), dtype=torch.complex64, device=DEV)
    v = wide[..., 3:3 + z.shape[-1]]
    v.copy_(z.to(DEV))
    assert not v.is_contiguous()
    return v


@pytest.mark.parametrize("layout", ["per_row", "shared3"])
@pytest.mark.parametrize("n", C.FDFIR_N)
def test_c_fdfir_inputs_as_views(D, n, layout):
    """x, H and the upstream gradient as offset views and as slices of wider NaN tensors: y, gx and gH bit for bit (fixed summation order,
    and loads that do not depend on the alignment)."""
    x, H, w = C.fdfir_arrays(n, layout)
    base = run_fdfir(D, x, H, w, n)
    f = lambda fn: (lambda a: fn(a.numpy()))
    for what, place in (("offset views", dict(x=f(misaligned), H=complex_offset, gy=f(misaligned))), ("x alone", dict(x=f(misaligned))),
                        ("slices", dict(x=f(row_slice), H=complex_slice, gy=f(row_slice)))):
        got = run_fdfir(D, x, H, w, n, place)
        for g, b, k in zip(got, base, ("y", "gx", "gH")):
            assert torch.equal(g, b), (n, layout, what, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("kind", list(C.FREQZ_CASES))
def test_c_freqz_coefficients_as_offset_views(D, kind, dtype):
    """b and a one element into NaN-filled allocations (float32: 4 bytes, float64: 8 bytes off a 16-byte boundary): bit for bit."""
    b, a, n, W = C.freqz_arrays(kind)
    base = run_freqz(D, kind, b, a, n, W, dtype)

    def offset(arr):
        buf = torch.full((arr.size + 2 * GUARD + 1,), NAN, dtype=dtype, device=DEV)
        v = buf[GUARD + 1:GUARD + 1 + arr.size].view(arr.shape)
        v.copy_(dev(arr).to(dtype))
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 if dtype == torch.float32 else 8)
        return v
    got = run_freqz(D, kind, b, a, n, W, dtype, place=offset)
    assert all(torch.equal(g, v) for g, v in zip(got, base))


# ---- D: silence and the eps clamp (STFT family) ---------------------------------------------------------------------------------------

# Identical signals miss the comparison with the restatement, on every kernel family (measured on an MI355X: loss / largest gradient entry):
#   mono-256 2.1e-7 / 1.8e-2    mono-1024 3.5e-7 / 1.1e-2    mono-8192 5.5e-7 / 1.8e-2    sd-256 2.1e-7 / 6.8e-3    mono-64-mel8 1.4e-7 / 8.2e-3
# against a reference of exactly 0 / 0. Both spectra come out of ONE packed transform, P = (Z[k] + conj Z[F-k]) / 2 and
# T = (Z[k] - conj Z[F-k]) / 2i of Z = FFT(p + i t), so for p == t they agree to float32 rounding (1e-7), not exactly: s1 is ~1e-7 s2 and
# not 0 (grad_consts' s1 == 0 branch is not reached), and sign(|T| - |P|) is the sign of that rounding, which the L1 log-magnitude term
# and the spectral convergence (a unit vector over s2, whatever the size of the difference) turn into a gradient of the usual size where
# autograd's |0|' = 0 and norm(0)' = 0 give exactly 0. A precision bound (2e-5 of a reference that is 0), kept as it was set for this file and
# marked as a strict xfail rather than loosened; test_d_identical_signals_stay_small_and_finite holds what the kernels do guarantee.
IDENTICAL_MISSES = "identical signals: the loss is 1.4e-7 .. 5.5e-7 and the largest gradient entry 6.8e-3 .. 1.8e-2 against a reference of " \
                   "exactly 0 (the two spectra leave one packed transform equal to float32 rounding only); bound: 2e-5 of the reference"


@pytest.mark.parametrize("case,kind", [pytest.param(c, k, marks=[pytest.mark.xfail(strict=True, reason=IDENTICAL_MISSES)] if k == "identical" else [])
                                       for c in C.SILENCE_CASES for k in C.SILENCE_KINDS], ids=str)
def test_d_silence_and_the_eps_clamp(D, case, kind):
    """(1, 1, 0) weights. zeros: both spectra clamp to sqrt(eps), the reference is finite (0); identical signals: the spectral
    convergence's numerator is 0 (grad_consts' s1 branch); below_eps: no bin reaches eps, the gradient is exactly 0; straddle: bins on
    both sides of eps - the loss only, at 2e-5 (a bin within float32 rounding of eps falls on either side of the clamp and the gradient
    jumps there; tests/test_loss_input_domain_cpu.py holds their share below 1 %)."""
    case = C.silence_case(case)
    p, t = C.silence_pair(case, kind)
    want = case.ref(p, t)
    got = run_stft(D, case, p, t)
    err = abs(got[0] - want[0]) / abs(want[0]) if want[0] else abs(got[0])
    record(f"loss_input_domain_silence[{case.name},{kind}]", loss=got[0], reference=want[0], error=err,
           grad_max=[float(np.abs(g).max()) for g in got[1:]], reference_grad_max=[float(np.abs(g).max()) for g in want[1:]])
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert abs(got[0] - want[0]) <= C.LOSS_TOL * abs(want[0]), (case.name, kind, got[0], want[0])
    if kind == "straddle":
        return
    if kind == "below_eps":
        assert not got[1].any() and not got[2].any()
    l2, mx = case.grad_bounds()
    for g, r in zip(got[1:], want[1:]):
        if not r.any():
            assert not g.any(), (case.name, kind, "the reference's gradient is exactly 0", float(np.abs(g).max()))
        else:
            assert rel2(g, r) < l2 and (mx is None or relmax(g, r) < mx), (case.name, kind)


@pytest.mark.parametrize("case", C.SILENCE_CASES, ids=str)
def test_d_identical_signals_stay_small_and_finite(D, case):
    """What holds for identical non-zero signals (see IDENTICAL_MISSES): the loss is below 1e-5 (tests/test_gpu_losses.py:85) and both
    gradients are finite - with s1 tiny and w_sc / (s1 s2) huge, nothing overflows."""
    case = C.silence_case(case)
    p, t = C.silence_pair(case, "identical")
    loss, gp, gt = run_stft(D, case, p, t)
    assert 0 <= loss < 1e-5 and np.isfinite(gp).all() and np.isfinite(gt).all(), (case.name, loss)
