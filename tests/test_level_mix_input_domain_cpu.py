"""The float64 references of tests/level_mix_input_domain_cases.py on off-domain input, without a GPU: what
tests/test_gpu_level_mix_input_domain.py expects of the kernels is pinned here as the references' own behaviour - where a NaN, a +inf or
a 1e30 sample of one item shows in the loudness and its gradient, in a peak-normalised row, in the output of the oversampled distortion
and on the mix bus - together with the margins that make the level cases mean something."""
import numpy as np
import pytest
import torch

from tests import bs1770_restated as R
from tests import level_mix_input_domain_cases as C


# ---- loudness -------------------------------------------------------------------------------------------------------------------------

def test_loudness_reference_with_a_nan_sample():
    """(3, 2, 9001) at 8 kHz, the NaN in item 1. At sample 0 every block is NaN, no comparison holds: L = -inf, gradient exactly 0. At
    sample 4500 the two blocks before it decide L (finite); the gradient of the poisoned ROW is NaN throughout (NaN x 0 in
    u = 2 y wsum, then filtered backwards over the row), the item's other row stays finite. At sample 9000, in the ignored tail, L is the
    clean value to 3e-4 and the row's gradient is NaN all the same."""
    x, gL, fs = C.loud_draw("one_segment")
    clean = C.loud_clean_ref("one_segment")
    assert clean["nb"][0] == 8 and np.isfinite(clean["L"]).all() and clean["margin"].min() >= 0.5
    for j, finite_L in ((0, False), (4500, True), (9000, True)):
        bad = np.array(x)
        bad[1, 0, j] = C.NAN
        r = C.loud_ref(bad, fs, gL)
        assert r["L"][0] == clean["L"][0] and r["L"][2] == clean["L"][2]
        assert np.array_equal(r["grad"][0], clean["grad"][0]) and np.array_equal(r["grad"][2], clean["grad"][2])
        if not finite_L:
            assert r["L"][1] == -np.inf and not r["grad"][1].any()
            continue
        assert np.isfinite(r["L"][1]) and r["nJ"][1] == (2 if j == 4500 else 8)
        assert np.isnan(r["grad"][1, 0]).all() and np.isfinite(r["grad"][1, 1]).all() and r["grad"][1, 1].any()
        if j == 9000:
            assert abs(r["L"][1] - clean["L"][1]) < 3e-4


def test_loudness_reference_with_an_overflowing_sample():
    """1e30 in item 1: its square (1e60) is far outside float32 and well inside float64 - the restatement reports a finite level of several
    hundred LUFS; +inf at the last sample of the last block makes that block's power inf, the relative gate inf, and L = -inf."""
    x, gL, fs = C.loud_draw("one_segment")
    bad, ch, j = C.loud_poisoned("one_segment", "1e30", "mid")
    r = C.loud_ref(bad, fs, gL)
    assert 500.0 < r["L"][1] < 600.0 and np.isfinite(r["grad"][1]).all() and 0 < np.abs(r["grad"][1]).max() < 1e-28
    bad, ch, j = C.loud_poisoned("one_segment", "inf", "block_end")
    assert j == 8799
    r = C.loud_ref(bad, fs, gL)
    assert r["L"][1] == -np.inf and not r["grad"][1].any()


@pytest.mark.parametrize("kind", C.LOUD_LEVELS)
def test_loudness_level_cases_sit_clear_of_the_gates(kind):
    x, gL, fs = C.loud_level_draw(kind)
    r = C.loud_ref(x, fs, gL)
    assert np.isfinite(r["L"][1]) and r["margin"].min() >= 0.5, (kind, r["margin"])
    nb = int(r["nb"][0])
    if kind == "gates":
        assert 0 < r["nJ"][0] < r["nA"][0] < nb, (r["nJ"], r["nA"], nb)           # blocks on both sides of both gates
    elif kind in ("zeros", "underflow"):
        assert r["L"][0] == -np.inf and r["nA"][0] == 0 and not r["grad"][0].any()
    else:
        assert 0 < r["nJ"][0] <= r["nA"][0] < nb and np.isfinite(r["L"][0])


def test_loudness_rate_cases_have_two_blocks_and_a_tail():
    for fs in C.LOUD_RATES:
        x, gL, _ = C.loud_rate_draw(fs)
        assert R.num_blocks(x.shape[-1], fs) == 2 and x.shape[-1] - 5 * R.block_sizes(fs)[0] == 37
    assert C.LOUD_RATES[0] == 8000 and C.LOUD_RATES[-1] == 384000


def test_loudness_launch_shapes():
    L = C.lib()
    cases = C.loud_cases()
    assert tuple(cases) == C.LOUD_CASES
    for name, (shape, fs, segmented) in cases.items():
        g = L.dasp_loudness_segments(shape[0] * shape[1], shape[2])
        assert (g > 1) == segmented, (name, g)
    n = C.loud_segmented_n()
    assert n >= 44117 and (n == 44117 or L.dasp_loudness_segments(3, n - 1) == 1)


# ---- peak_normalize -------------------------------------------------------------------------------------------------------------------

def torch_peak(x, gy, peak_db, eps):
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    y = xt * 10.0 ** (peak_db / 20.0) / xt.abs().amax(-1, keepdim=True).clamp(min=eps)
    y.backward(torch.tensor(np.asarray(gy), dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy()


def close(a, b, rtol=1e-12):
    return np.array_equal(np.isfinite(a), np.isfinite(b)) and np.allclose(a[np.isfinite(a)], b[np.isfinite(b)], rtol=rtol, atol=0.0)


def test_peak_reference_against_autograd_off_domain():
    """The restatement against autograd of x * s / x.abs().amax(-1, keepdim=True).clamp(min=eps). NaN: y and the gradient of the row are
    NaN throughout in both (the corrected restatement). 1e30: both finite and equal. +inf: y is 0 with a NaN at the sample in both; the
    gradient is non-finite at the sample in both - autograd spreads it over the row (amax's backward multiplies the NaN by a 0 / 1 mask),
    the closed form keeps it at the index of the maximum, which is what the kernel is held to. The rows next to it keep their bits."""
    x, gy = C.peak_draw(C.PEAK_SHAPES[0])
    y0, g0 = C.peak_ref(x, gy)
    yt, gt = torch_peak(x, gy, C.PEAK_DB, C.PEAK_EPS)
    assert close(y0, yt) and close(g0, gt)
    for value in C.VALUES:
        bad = np.array(x)
        bad[1, 0, 2048] = C.VALUES[value]
        y, g = C.peak_ref(bad, gy)
        yt, gt = torch_peak(bad, gy, C.PEAK_DB, C.PEAK_EPS)
        keep = np.ones(x.shape[:2], bool)
        keep[1, 0] = False
        assert np.array_equal(y[keep], y0[keep]) and np.array_equal(g[keep], g0[keep])
        assert close(y, yt), value
        if value == "nan":
            assert np.isnan(y[1, 0]).all() and np.isnan(g[1, 0]).all() and np.isnan(gt[1, 0]).all()
        elif value == "1e30":
            assert close(g, gt) and np.isfinite(g).all()
        else:
            hit = np.zeros(x.shape[-1], bool)
            hit[2048] = True
            assert np.array_equal(~np.isfinite(y[1, 0]), hit) and not y[1, 0][~hit].any()
            assert np.array_equal(~np.isfinite(g[1, 0]), hit) and not g[1, 0][~hit].any() and np.isnan(gt[1, 0]).all()


def test_peak_reference_at_the_eps_clamp():
    """Peaks of eps / 2, eps and one float32 ulp above eps: y agrees with autograd everywhere. The gradient agrees below and above; AT
    eps the clamp's backward passes the gradient on (>=) where the closed form (and the kernel) take the constant branch (>): they differ
    at the index of the maximum only - a choice between two subgradients. eps = 0 on a zero row: y is NaN in both, the gradient non-finite
    everywhere in both (s g / 0 = +-inf in the closed form, NaN from the tie-splitting of amax in autograd)."""
    x, gy = C.peak_level_draw()
    y, g = C.peak_ref(x, gy, 0.0, C.EPS32)
    yt, gt = torch_peak(x, gy, 0.0, C.EPS32)
    assert np.isfinite(y).all() and np.isfinite(g).all()
    assert close(y, yt) and close(g[0], gt[0]) and close(g[2], gt[2]) and close(g[3], gt[3])
    differ = g[1, 0] != gt[1, 0]
    assert differ[1000] and differ.sum() == 1
    y, g = C.peak_ref(x, gy, 0.0, 0.0)
    yt, gt = torch_peak(x, gy, 0.0, 0.0)
    assert np.isnan(y[3]).all() and np.isnan(yt[3]).all() and np.isinf(g[3]).all() and not np.isfinite(gt[3]).any()
    assert np.isfinite(y[:3]).all() and close(y[:3], yt[:3]) and close(g[:3], gt[:3])


def test_peak_launch_shapes():
    assert C.peak_segments(C.PEAK_SHAPES[0]) == 2 and C.peak_segments(C.PEAK_SHAPES[1]) > 2       # PK_MIN_SEG = 4096


# ---- oversampled_distortion -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,H", [(2, 12), (8, 12), (8, 16)])
def test_oversampling_reference_footprints(L, H):
    """One sample j of row 3 (item 1). NaN: y and grad x are NaN on [j - 2 H, j + 2 H] (4 H + 1 = 49 outputs at H = 12), finite and
    bit-equal to the clean run elsewhere, grad drive_db of the row is NaN. +inf and 1e30: tanh saturates and sech^2 is 0 - y and grad x
    are finite everywhere; grad drive_db of the row is NaN for +inf (0 x inf) and finite for 1e30."""
    ref, _ = C.os_clean(L, H)
    N = C.os_shape(L)[-1]
    for value in C.VALUES:
        x, drive, w, row, j = C.os_poisoned(L, "x", value, "tile_start")
        r = C.os_ref(x, drive, w, L, H)
        hit = C.os_footprint(j, H, N)
        assert int(hit.sum()) == 4 * H + 1 and row == 2
        for k in ("y", "gx"):
            a, b = r[k].reshape(6, N), ref[k].reshape(6, N)
            keep = np.arange(6) != row
            assert np.array_equal(a[keep], b[keep]), (value, k)
            if value == "nan":
                assert np.array_equal(~np.isfinite(a[row]), hit) and np.array_equal(a[row][~hit], b[row][~hit]), (value, k)
            else:
                assert np.isfinite(a[row]).all() and np.array_equal(a[row][~hit], b[row][~hit]), (value, k)
        keep = np.arange(6) != row
        assert np.array_equal(r["gdrive"][keep], ref["gdrive"][keep])
        assert np.isfinite(r["gdrive"][row]) == (value == "1e30"), (value, r["gdrive"][row])
    x, drive, w, row, j = C.os_poisoned(L, "gy", "nan", "mid")
    r = C.os_ref(x, drive, w, L, H)
    assert np.array_equal(r["y"], ref["y"]) and np.array_equal(~np.isfinite(r["gx"].reshape(6, N)[row]), C.os_footprint(j, H, N))
    assert np.isnan(r["gdrive"][row]) and np.isfinite(np.delete(r["gdrive"], row)).all()


def test_oversampling_shapes():
    for L, H in C.OS_CASES:
        B, Cc, N = C.os_shape(L)
        assert N == 2 * C.OS_TILES[L] + 5 and C.lib().dasp_osdist_partial_floats(B * Cc, N, L) == 3 * B * Cc       # three tiles per row
        assert C.os_position("tile_end", L) + 1 == C.os_position("tile_start", L) == C.OS_TILES[L]


# ---- stereo_mix -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_send", [True, False])
def test_mix_reference_with_a_nan_sample(with_send):
    """A NaN sample in one track of item 1 - a generic, the last, the muted or the hard-panned one (0 x NaN) - reaches that sample of both
    channels of the item's mix (and send) and nothing else there; grad x does not depend on x and keeps its bits; exactly that track's
    control gradients are NaN."""
    shape = C.MIX_SHAPES[0]
    B, T, N = shape
    clean = C.mix_clean_ref(shape, with_send)
    assert all(np.isfinite(clean[k]).all() for k in C.MIX_KEYS if clean[k] is not None)
    sp = C.mix_special(T)
    assert not clean["gx"][:, sp["muted"]].any()
    for where, t in C.mix_tracks(T).items():
        (x, gain_db, pan, send_db, w0, w1), tt, j = C.mix_poisoned(shape, "x", "nan", where)
        assert tt == t
        r = C.mix_ref(x, gain_db, pan, send_db if with_send else None, w0, w1)
        hit = np.zeros((B, 2, N), bool)
        hit[1, :, j] = True
        for k in ("mix", "send") if with_send else ("mix",):
            assert np.array_equal(np.isnan(r[k]), hit) and np.array_equal(r[k][~hit], clean[k][~hit]), (where, k)
        assert np.array_equal(r["gx"], clean["gx"])
        bad = np.zeros((B, T), bool)
        bad[1, t] = True
        for k in ("ggain", "gpan", "gsend") if with_send else ("ggain", "gpan"):
            a, b = r[k].reshape(B, T), clean[k].reshape(B, T)
            assert np.array_equal(np.isnan(a), bad) and np.array_equal(a[~bad], b[~bad]), (where, k)


def test_mix_table():
    assert C.mix_special(5) == dict(hard=1, muted=3) and C.mix_special(9) == dict(hard=1, muted=5) and C.mix_special(1) == {}
    for shape in C.MIX_SHAPES:
        x, gain_db, pan, send_db, w0, w1 = C.mix_draw(shape)
        sp = C.mix_special(shape[1])
        if sp:
            assert (pan[:, sp["hard"]] == 0).all() and np.isneginf(gain_db[:, sp["muted"]]).all()
        assert C.lib().dasp_stereo_mix_partial_floats(shape[0], shape[1], shape[2], 1) > 0
