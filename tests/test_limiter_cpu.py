"""CPU tests of limiter: the restatement (tests/limiter_restated.py) against autograd and central differences, the properties of its
definition (both forms of e agree, the winners never go back, the ceiling holds), the conditioning of the parity cases that the GPU
tests run (tests/limiter_cases.py), and what functional.limiter, modules.Limiter and the C ABI refuse before they touch a device."""
import inspect

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import limiter_cases as K
from tests import limiter_restated as R

INF = float("inf")


def draw(B, C, N, seed, sr=8000):
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(B, C, N, generator=g, dtype=torch.float64) * torch.exp(0.7 * torch.randn(B, 1, 1, generator=g, dtype=torch.float64))
    thr = torch.rand(B, generator=g, dtype=torch.float64) * 14 - 20
    rel = torch.exp(torch.rand(B, generator=g, dtype=torch.float64) * np.log(40.0)) * 0.5            # 0.5 .. 20 ms
    return x, thr, rel, torch.randn(B, C, N, generator=g, dtype=torch.float64)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 5, 64])
@pytest.mark.parametrize("N,C", [(1, 1), (7, 2), (150, 3), (700, 2)])
def test_restated_adjoint_equals_autograd_and_the_definition_holds(L, N, C):
    sr = 8000
    x, thr, rel, w = draw(3, C, N, 100 * L + N)
    xg, tg, rg = x.clone().requires_grad_(True), thr.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    y, e, G = R.limiter(xg, sr, tg, rg, lookahead=L)
    gx, gt, gr = torch.autograd.grad((y * w).sum(), [xg, tg, rg])
    r = R.forward_backward(x, sr, thr, rel, w, lookahead=L)
    assert r["gap"]["hold"] > 1e-9 and r["gap"]["release"] > 1e-9 and r["gap"]["channel"] > 1e-9       # no ties: autograd's rule is the stated one
    scale = lambda t: max(float(t.abs().max()), 1e-30)
    assert np.abs(r["y"] - y.detach().numpy()).max() <= 1e-14 * scale(y.detach())
    assert np.abs(r["gx"] - gx.numpy()).max() <= 1e-12 * max(scale(gx), scale(w))          # (one sample, one channel: gx cancels to zero)
    assert np.abs(r["gthr"] - gt.numpy()).max() <= 1e-12 * max(scale(gt), 1e-3)
    assert np.abs(r["grel"] - gr.numpy()).max() <= 1e-11 * max(scale(gr), 1e-6)
    # both forms of e
    if N <= 150:
        e2 = R.limiter(x, sr, thr, rel, lookahead=L, two_step=True)[1]
        assert (e.detach() - e2).abs().max() <= 1e-12 * scale(e2)
    assert np.abs(r["e"] - e.detach().numpy()).max() == 0
    # the winners never go back, and name the sample that e[m] comes from
    wn = r["w"]
    assert (np.diff(np.where(wn < 0, -1, wn), axis=1) >= 0).all()
    # the ceiling
    ceil = 10.0 ** (thr.clamp(-120, 40) / 20.0)
    assert (y.detach().abs().amax((1, 2)) <= ceil * (1 + 1e-12)).all()


@pytest.mark.parametrize("L", [0, 5, 64])
def test_restated_adjoint_equals_central_differences(L):
    sr, N = 8000, 300
    x, thr, rel, w = draw(2, 2, N, 7 + L)
    r = R.forward_backward(x, sr, thr, rel, w, lookahead=L)
    f = lambda xx, tt, rr: float((R.limiter(xx, sr, tt, rr, lookahead=L)[0] * w).sum())
    h = 1e-6
    for b in range(2):
        d = torch.zeros(2, dtype=torch.float64)
        d[b] = h
        assert abs((f(x, thr + d, rel) - f(x, thr - d, rel)) / (2 * h) - r["gthr"][b]) <= 1e-6 * max(abs(r["gthr"][b]), 1e-2)
        assert abs((f(x, thr, rel + d) - f(x, thr, rel - d)) / (2 * h) - r["grel"][b]) <= 1e-6 * max(abs(r["grel"][b]), 1e-2)
    g = torch.Generator().manual_seed(3)
    for _ in range(12):
        b, c, n = int(torch.randint(2, (1,), generator=g)), int(torch.randint(2, (1,), generator=g)), int(torch.randint(N, (1,), generator=g))
        d = torch.zeros_like(x)
        d[b, c, n] = h
        assert abs((f(x + d, thr, rel) - f(x - d, thr, rel)) / (2 * h) - r["gx"][b, c, n]) <= 1e-6 * max(abs(r["gx"][b, c, n]), 1e-2)


def test_clamped_controls_have_exactly_no_gradient_in_the_restatement():
    x, _, _, w = draw(5, 2, 200, 5)
    thr = torch.tensor([-130.0, 45.0, -12.0, -12.0, -12.0], dtype=torch.float64)
    rel = torch.tensor([5.0, 5.0, 0.05, 20000.0, 5.0], dtype=torch.float64)
    r = R.forward_backward(x, 8000, thr, rel, w, lookahead=5)
    assert r["gthr"][0] == 0 and r["gthr"][1] == 0 and r["gthr"][2] != 0 and r["gthr"][3] != 0
    assert r["grel"][2] == 0 and r["grel"][3] == 0 and r["grel"][4] != 0 and r["gthr"][4] != 0
    c = R.forward_backward(x, 8000, thr.clamp(-120, 40), rel.clamp(0.1, 10000), w, lookahead=5)
    assert np.array_equal(r["y"], c["y"]) and np.array_equal(r["gx"], c["gx"])


def test_ties_follow_the_stated_rules():
    """A square wave +-A above the threshold on two equal channels: the latest sample of a window wins, the lower channel has the peak."""
    N, L = 40, 3
    x = (0.8 * (-1.0) ** torch.arange(N, dtype=torch.float64)).expand(1, 2, N).contiguous()
    r = R.forward_backward(x, 8000, torch.tensor([-12.0]), torch.tensor([5.0]), torch.ones(1, 2, N, dtype=torch.float64), lookahead=L)
    assert (r["cs"] == 0).all()
    assert np.array_equal(r["w"][0], np.minimum(np.arange(N + L), N - 1))     # m < N: the sample itself; then the last one, held and released
    assert not r["gx"][0, 1].any() or np.abs(r["gx"][0, 1] - r["G"][0]).max() == 0   # channel 1 gets the direct term alone


# ---- the parity cases of the GPU tests are well conditioned --------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", K.CONFIGS, ids=lambda c: "sr%d-L%d-C%d" % c[:3])
def test_parity_cases_are_well_conditioned(cfg):
    """A condition on the inputs, not a measurement: the float32 and the float64 restatement take the same decision everywhere, the
    smallest relative gap of a float64 decision is at least 1e-4, and 20 - 90 % of the samples are limited."""
    sr, L, C, seed = cfg
    a, w64, w32 = K.reference(*cfg)
    for k in ("w", "cs", "limited"):
        assert np.array_equal(w64[k], w32[k]), k
    assert min(w64["gap"].values()) >= 1e-4, w64["gap"]
    Ls = K.lengths(L)
    frac = sum(w64["limited"][q, :n].sum() for q, n in enumerate(Ls)) / sum(Ls)
    assert 0.2 <= frac <= 0.9, frac


def test_parity_cases_cover_what_the_issue_lists():
    assert sorted({c[1] for c in K.CONFIGS}) == [0, 1, 63, 64, 65, 220, K.MAX_LOOKAHEAD]
    assert {c[2] for c in K.CONFIGS} == {1, 2, 3} and {c[0] for c in K.CONFIGS} == {8000, 44100, 192000}
    T = K.TILE
    assert K.lengths(220) == [1, 2, 220, 221, T - 221, T - 220, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]
    assert K.lengths(0) == [1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]
    assert R.lookahead_samples(44100, 5.0) == 220 == D.functional.limiter_lookahead(44100, 5.0)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------
def _controls(bs):
    return [torch.full((bs,), -6.0), torch.full((bs,), 50.0)]


@pytest.mark.parametrize("which,name", enumerate(R.CTL))
def test_wrong_control_count_names_the_control(which, name):
    ctl = _controls(2)
    ctl[which] = torch.zeros(5)
    with pytest.raises(RuntimeError, match=name):
        D.limiter(torch.zeros(2, 2, 64), 44100, *ctl)


@pytest.mark.parametrize("kw", [dict(sample_rate=0), dict(sample_rate=-8000), dict(sample_rate=float("nan")), dict(sample_rate=INF),
                                dict(lookahead_ms=-1.0), dict(lookahead_ms=float("nan")), dict(lookahead_ms=INF), dict(lookahead_ms=1024.6 / 44.1),
                                dict(sample_rate=192000, lookahead_ms=5.4), dict(eps=-1.0), dict(eps=float("nan")), dict(lookahead_ms="x")])
def test_bad_scalars_raise_value_error_before_the_device(kw):
    a = dict(sample_rate=44100, lookahead_ms=5.0, eps=1e-8)
    a.update(kw)
    with pytest.raises(ValueError, match="limiter"):
        D.limiter(torch.zeros(1, 1, 8), a["sample_rate"], *_controls(1), lookahead_ms=a["lookahead_ms"], eps=a["eps"])


def test_lookahead_in_samples():
    f = D.functional.limiter_lookahead
    assert f(44100, 5.0) == 220 and f(8000, 0.0) == 0 and f(192000, 5.0) == 960 and f(44100, 1024 / 44.1) == 1024
    assert D.functional.LIMITER_MAX_LOOKAHEAD == _lib.lib().dasp_limiter_max_lookahead() == K.MAX_LOOKAHEAD >= 1024
    assert _lib.lib().dasp_limiter_tile() == K.TILE


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.limiter(torch.zeros(2, 2, 64), 44100, *_controls(2))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.Limiter(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 2), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="limiter: float64"):
        D.limiter(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2))


def test_size_queries_and_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) and DASP_ERR_UNSUPPORTED (-2) before any launch; the non-null pointers are fakes, never read."""
    L = _lib.lib()
    assert L.dasp_limiter_state_floats(3, 1000) == 6000 == L.dasp_limiter_partial_floats(3, 1000)          # 8 bytes per sample of an item
    assert L.dasp_limiter_state_floats(0, 10) == -1 and L.dasp_limiter_partial_floats(3, 0) == -1
    f = 256
    ok = dict(B=2, C=2, N=1000, L=220, sr=44100.0, eps=1e-8)

    def fwd(x=f, ctl=f, y=f, gain=f, win=f, **kw):
        a = {**ok, **kw}
        return L.dasp_limiter_forward(x, ctl, y, gain, win, a["B"], a["C"], a["N"], a["L"], a["sr"], a["eps"], None)

    def bwd(x=f, ctl=f, gain=f, win=f, gy=f, gx=f, gctl=f, scr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_limiter_backward(x, ctl, gain, win, gy, gx, gctl, scr, a["B"], a["C"], a["N"], a["L"], a["sr"], a["eps"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(ctl=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1 and call(L=-1) == -1
        assert call(sr=0.0) == -1 and call(sr=-1.0) == -1 and call(sr=float("nan")) == -1 and call(sr=INF) == -1
        assert call(eps=-1.0) == -1 and call(eps=float("nan")) == -1 and call(eps=INF) == -1
        assert call(L=K.MAX_LOOKAHEAD + 1) == -2 and call(N=(1 << 31) - 4096) == -2
    assert fwd(y=None) == -1 and fwd(gain=None) == -1 and fwd(win=None) == -1         # gain and winner: both or neither
    assert bwd(gain=None) == -1 and bwd(win=None) == -1 and bwd(gy=None) == -1 and bwd(gctl=None) == -1 and bwd(scr=None) == -1


# ---- the module --------------------------------------------------------------------------------------------------------------------------
def test_module_tables_and_plumbing():
    names = list(inspect.signature(D.functional.limiter).parameters)
    assert names == ["x", "sample_rate", "threshold_db", "release_ms", "lookahead_ms", "eps"]
    m = D.Limiter(44100)
    assert m.num_params == 2 and list(m.param_ranges) == names[2:4]
    assert m.param_ranges == {"threshold_db": (-40.0, 0.0), "release_ms": (5.0, 500.0)}
    assert m.lookahead_ms == 5.0 and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.limiter and m.process_fn.keywords == {"lookahead_ms": 5.0}
    with pytest.raises(ValueError, match="limiter"):
        D.Limiter(192000, lookahead_ms=6.0)
    m = D.Limiter(48000, lookahead_ms=2.0, min_threshold_db=-24.0, max_release_ms=200.0)
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    p = torch.rand(3, 2, generator=torch.Generator().manual_seed(0))
    x = torch.zeros(3, 2, 16)
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and list(seen)[:2] == names[2:4]
    assert torch.allclose(seen["threshold_db"], p[:, 0] * 24.0 - 24.0) and torch.allclose(seen["release_ms"], p[:, 1] * 195.0 + 5.0)
    with pytest.raises(ValueError):
        m.process_normalized(x, torch.rand(3, 3))
    assert D.limiter is D.functional.limiter and D.Limiter is D.modules.Limiter
