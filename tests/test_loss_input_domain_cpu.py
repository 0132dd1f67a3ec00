"""The float64 references of tests/loss_input_domain_cases.py on off-domain input, without a GPU: what
tests/test_gpu_loss_input_domain.py expects of the kernels is pinned here as the references' own behaviour - which rows of a batch with
one NaN or +inf sample are non-finite, which keep their clean values bit for bit, the one finite exception (SNRLoss on a +inf prediction
with zero_mean=False is exactly 80 dB) - and the caps that make the silence cases mean something (how many bins of the straddling case
sit within rounding of eps)."""
import numpy as np
import pytest
import torch

from tests import auraloss_restated as ar
from tests import auraloss_time_restated as atr
from tests import loss_input_domain_cases as C

RES = ((256, 64, 256),)
VALUES = {"nan": C.NAN, "inf": C.INF}


def _batch(value):
    """3 rows of 3000 samples, NaN or +inf at sample 1500 of the prediction's row 1."""
    p, t = C.generic((3, 1, 3000), 3000)
    bad = p.copy()
    bad[1, 0, 1500] = VALUES[value]
    return p, bad, t


@pytest.mark.parametrize("value", list(VALUES))
def test_stft_reference_on_a_poisoned_prediction(value):
    p, bad, t = _batch(value)
    for w in ((1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        kw = dict(w_sc=w[0], w_log_mag=w[1], w_lin_mag=w[2])
        loss, gp, _ = ar.loss_and_grads(bad, t, RES, **kw)
        assert not np.isfinite(loss), (value, w, loss)                    # torch.clamp(min=eps) hands a NaN on
        finite = np.isfinite(C.items(gp)).all(1)
        if w[0]:
            assert not finite.any(), (value, w, finite)                   # the spectral convergence divides every row by one norm
        else:
            _, clean, _ = ar.loss_and_grads(p, t, RES, **kw)
            assert list(finite) == [True, False, True], (value, w, finite)
            assert np.array_equal(gp[0], clean[0]) and np.array_equal(gp[2], clean[2])      # bit-equal to the clean batch's rows


@pytest.mark.parametrize("value", list(VALUES))
def test_time_domain_reference_on_a_poisoned_prediction(value):
    p, bad, t = _batch(value)
    for term in atr.TERMS:
        for zero_mean in (True, False):
            clean = atr.loss_and_grads(p, t, {term: 1.0}, zero_mean=zero_mean, reduction="none")[0]
            got = atr.loss_and_grads(bad, t, {term: 1.0}, zero_mean=zero_mean, reduction="none")[0]
            assert got.shape == (3, 1)
            assert got[0, 0] == clean[0, 0] and got[2, 0] == clean[2, 0], (term, zero_mean)
            if (term, value, zero_mean) == ("snr", "inf", False):
                assert got[1, 0] == 80.0                                   # -10 log10(T / inf + 1e-8): the one finite value
            else:
                assert not np.isfinite(got[1, 0]), (term, value, zero_mean, got[1, 0])
            mean = atr.loss_and_grads(bad, t, {term: 1.0}, zero_mean=zero_mean, reduction="mean")[0]
            assert np.isfinite(mean) == np.isfinite(got[1, 0])


def test_case_table_covers_what_it_says():
    names = set(C.STFT_BY_NAME)
    for layout in ("mono", "sd"):
        for r in C.ALL_RES:
            assert any(c.layout == layout and c.res[0] == r and not c.n_bins for c in C.STFT_CASES), (layout, r)
    for r in C.ALL_RES:
        for m in C.MIXES:
            assert f"mono-{r[0]}-{m}" in names
    for layout in ("mono", "sd"):
        cs = [c for c in C.STFT_CASES if c.layout == layout]
        assert {c.n_bins for c in cs} == {None, 8, 40} and {c.aw for c in cs} == {False, True} and {c.mix for c in cs} == set(C.MIXES)
        assert {c.shape[-1] for c in cs} == {3000, 5000, 9000} and all(c.shape[:2] == (3, 2 if layout == "sd" else 1) for c in cs)
    assert len(C.POISONS) == 12 and C.TD_SHAPE == (3, 2, 4099) and set(C.TD_CASES) == set(atr.TERMS) | {"mix"}
    # the rows of an item that share a complex transform (csrc/fdfir.hip: rows 2f and 2f + 1 of the rows that share a response)
    assert [C.fdfir_partner("per_row", c) for c in (0, 1)] == [None, None]
    assert [C.fdfir_partner("shared2", c) for c in (0, 1)] == [1, 0]
    assert [C.fdfir_partner("shared3", c) for c in (0, 1, 2)] == [1, 0, None]


@pytest.mark.parametrize("case", [c for c in C.STFT_CASES if c.res[0][0] <= 256], ids=str)
def test_every_small_case_has_a_non_finite_reference_loss(case):
    """(the small-frame cases: the larger ones run the same restatement on more samples)"""
    p, t, ref = C.stft_clean(case.name)
    assert np.isfinite(ref[0]) and np.isfinite(ref[1]).all() and np.isfinite(ref[2]).all()
    for poison in (("input", "nan", "first"), ("target", "inf", "last")):
        loss, gp, gt = case.ref(*C.poisoned(p, t, poison))
        assert not np.isfinite(loss), (case.name, poison, loss)
        g, clean = (gp, ref[1]) if poison[0] == "input" else (gt, ref[2])
        finite = np.isfinite(C.items(g)).all(1)
        assert not finite[1]
        if case.w_sc == 0:
            assert finite[0] and finite[2] and np.array_equal(g[0], clean[0]) and np.array_equal(g[2], clean[2])


@pytest.mark.parametrize("case", C.SILENCE_CASES, ids=str)
def test_silence_levels_are_what_their_names_say(case):
    """zeros: a finite reference (both spectra clamp to sqrt(eps)); below_eps: every bin power below eps, so the reference's gradient is
    exactly 0; straddle: bins on both sides of eps, and fewer than 1 % of them within 1e-4 relative of eps - a bin within float32
    rounding of eps may fall on either side of the clamp, so the loss comparison (2e-5) only means something if they are few."""
    linear = C.silence_case(case)
    p, t = C.silence_pair(case, "zeros")
    loss, gp, gt = linear.ref(p, t)
    assert np.isfinite(loss) and loss == 0.0 and not gp.any() and not gt.any()
    p, t = C.silence_pair(case, "below_eps")
    assert np.abs(p).max() > 0 and max(C.bin_powers(case, p).max(), C.bin_powers(case, t).max()) < C.EPS
    loss, gp, gt = linear.ref(p, t)
    assert loss == 0.0 and not gp.any() and not gt.any()
    p, t = C.silence_pair(case, "straddle")
    pw = np.concatenate([C.bin_powers(case, p), C.bin_powers(case, t)])
    below, near = float((pw < C.EPS).mean()), float((np.abs(pw - C.EPS) <= 1e-4 * C.EPS).mean())
    print(f"{case.name}: {below:.3f} of the bins below eps, {near:.2e} within 1e-4 relative of it")
    assert 0.1 < below < 0.9 and near < 0.01
    p, t = C.silence_pair(case, "identical")
    loss, gp, gt = linear.ref(p, t)
    assert loss == 0.0 and not gp.any() and not gt.any()                  # norm(0) and |0| have gradient 0 in autograd


def test_fdfir_and_freqz_references_on_a_poisoned_item():
    x, H, w = C.fdfir_arrays(64, "shared3")
    clean = C.fdfir_ref(x, H, w, 64)
    for v in VALUES.values():
        bad = x.clone()
        bad[1, 0, 30] = v
        y, gx, gH = C.fdfir_ref(bad, H, w, 64)
        assert not torch.isfinite(y[1, 0]).any()                          # the poisoned row, every sample
        assert torch.equal(y[1, 1], clean[0][1, 1]) and torch.equal(y[1, 2], clean[0][1, 2])       # the reference transforms rows separately
        assert torch.equal(y[0], clean[0][0]) and torch.equal(y[2], clean[0][2]) and torch.equal(gx, clean[1])
        assert not torch.isfinite(torch.view_as_real(gH[1])).any() and torch.equal(gH[0], clean[2][0]) and torch.equal(gH[2], clean[2][2])
    from tests.freqz_exact import exact_response
    for kind in C.FREQZ_CASES:
        b, a, n, W = C.freqz_arrays(kind)
        assert b.shape[0] == a.shape[0] == W.shape[0] == 3
        Hc = exact_response(b, a, n)
        bad = b.copy()
        bad[1, 0, 1] = np.nan
        Hb = exact_response(bad, a, n)
        assert np.array_equal(Hb[0], Hc[0]) and np.array_equal(Hb[2], Hc[2]) and not np.isfinite(Hb[1]).any()
