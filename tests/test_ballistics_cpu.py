"""ballistics and sidechain_compressor without a GPU: the hand-written adjoint of tests/ballistics_restated.py against autograd, the
control gradients against central differences, the step's rise and fall times, attack == release against the linear one-pole, the
conditions on the parity cases of the GPU tests, the argument errors raised before the device is asked for and the C entry points'
refusals."""
import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import ballistics_cases as K
from tests import ballistics_restated as R


def _inputs(bs, F, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(P=K.curve(bs, F, g).double(), w=(0.5 + 0.5 * torch.randn(bs, F, generator=g)).double())


@pytest.mark.parametrize("sr,hop,F,att,rel", [(8000, 8, 203, (0.1, 3.0, 80.0), (50.0, 3.0, 1.0)), (44100, 64, 700, (0.05, 50.0, 2000.0), (2000.0, 5.0, 20000.0)),
                                              (192000, 2048, 100, (1.0, 50.0, 20000.0), (5.0, 500.0, 1.0)), (44100, 16, 1, (5.0, 5.0, 5.0), (50.0, 1.0, 5.0))])
def test_by_hand_adjoint_equals_autograd(sr, hop, F, att, rel):
    """The float64 form of by_hand (the saved E kept in float64 too) against the frame loop and autograd: 1e-12 of the peak."""
    a = _inputs(3, F, seed=hop + F)
    att, rel = torch.tensor(att), torch.tensor(rel)
    want = R.forward_backward(a["P"], sr, att, rel, a["w"], hop)
    got = R.by_hand(a["P"].float().numpy(), sr, att.numpy(), rel.numpy(), a["w"].numpy(), hop, np.float64)
    assert np.array_equal(got["up"], want["up"])
    for k in R.NAMES:
        assert K.per_item_err(got[k], want[k]) <= 1e-12, k
    for name, t in (("gatt", att), ("grel", rel)):
        clamped = ((t < 0.1) | (t > 10000.0)).numpy()
        assert (got[name][clamped] == 0).all() and (want[name][clamped] == 0).all()


def test_control_gradients_against_central_differences():
    """Four digits, as the issue measured them; the step is small enough that no branch flips between the two evaluations."""
    sr, hop, F = 44100, 64, 600
    a = _inputs(5, F, seed=5)
    att, rel = torch.tensor([1.0, 5.0, 50.0, 2000.0, 20.0]), torch.tensor([50.0, 5.0, 1.0, 100.0, 2000.0])
    got = R.by_hand(a["P"].float().numpy(), sr, att.numpy(), rel.numpy(), a["w"].numpy(), hop, np.float64)
    loss = lambda at, re: (R.ballistics(a["P"].float(), sr, at, re, hop)[0] * a["w"]).sum(1).numpy()
    for name, which in (("gatt", 0), ("grel", 1)):
        t = (att, rel)[which].double()
        h = 1e-6 * t
        hi, lo = ((t + s * h if which == 0 else att.double(), t + s * h if which == 1 else rel.double()) for s in (1, -1))
        assert all(np.array_equal(R.ballistics(a["P"].float(), sr, *c, hop)[1].numpy(), got["up"]) for c in (hi, lo))
        fd = (loss(*hi) - loss(*lo)) / (2 * h.numpy())
        assert np.abs(fd - got[name]).max() <= 1e-4 * np.abs(got[name]).max(), name


@pytest.mark.parametrize("sr,hop,att,rel", [(44100, 8, 5.0, 100.0), (44100, 64, 20.0, 200.0), (8000, 8, 100.0, 5.0)])
def test_step_rise_and_fall_times(sr, hop, att, rel):
    """The 10 - 90 % rise and fall times of a step are attack_ms and release_ms to within one hop (at hop 8 and 44.1 kHz one hop is 0.18 ms;
    the crossings are interpolated between frame points)."""
    split = int(6 * max(att, rel) * sr / 1000.0 / hop) + 2
    P = torch.cat([torch.ones(1, split), torch.zeros(1, split)], 1)
    E = R.by_hand(P.numpy(), sr, np.array([att]), np.array([rel]), np.ones((1, 2 * split)), hop)["E"][0]
    rise, fall = R.rise_and_fall_ms(np.concatenate([[0.0], E]), sr, hop, 0.0, 1.0, split + 1)
    one_hop = hop * 1000.0 / sr
    assert abs(rise - att) <= one_hop and abs(fall - rel) <= one_hop, (rise, fall)


def test_equal_times_are_the_linear_one_pole():
    sr, hop, F = 44100, 64, 500
    a = _inputs(3, F, seed=2)
    t = torch.tensor([0.5, 5.0, 300.0])
    E, _ = R.ballistics(a["P"], sr, t, t, hop)
    c = R.item_constants(sr, hop, t.numpy())[0]
    e, want = np.zeros(3), np.zeros((3, F))
    for j in range(F):
        e = (1.0 - c) * e + c * a["P"][:, j].numpy()
        want[:, j] = e
    assert K.per_item_err(E.numpy(), want) <= 1e-12


def test_ties_and_nan_frames_take_the_release_branch():
    P = torch.tensor([[1.0, 1.0, 1.0, float("nan"), 2.0]])
    r = R.by_hand(P.numpy(), 8000, np.array([0.1]), np.array([50.0]), np.ones((1, 5)), 2048)            # c_a = 1: E reaches P at once
    assert r["up"][0].tolist() == [True, False, False, False, False]
    assert r["E"][0, :3].tolist() == [1.0, 1.0, 1.0] and np.isnan(r["E"][0, 3:]).all()
    r = R.by_hand(np.ones((2, 4), np.float32), 8000, np.array([5.0, np.nan]), np.array([np.nan, 5.0]), np.ones((2, 4)), 64)
    assert all(np.isnan(r[k]).all() for k in R.NAMES)                          # a NaN control: the whole item


@pytest.mark.parametrize("cfg", K.BALLISTICS_CONFIGS, ids=lambda c: "sr%d-hop%d" % c[:2])
def test_conditions_on_the_parity_cases(cfg):
    """Both branches at least 5 % of the frames in every item with F >= 64, no bound above ten floors, the by-hand masks equal to the
    float64 ones, and no near-tie: the masks are what they are with both coefficients an ulp up or down (a coefficient that is exactly 1,
    where exp underflows by a wide margin, stays 1)."""
    sr, hop, att, rel, seed = cfg
    assert set(att) | set(rel) <= set(K.TIMES)
    for f, b, want, f32 in K.ballistics_calls(cfg):
        assert np.array_equal(want["up"], f32["up"]), (cfg, f)
        if f >= 64:
            up, down = K.branch_shares(want["up"])
            assert up.min() >= 0.05 and down.min() >= 0.05, (cfg, f, up, down)
        for k, (e32, bound) in K.bounds(want, f32, R.FLOOR).items():
            assert bound <= 10 * R.FLOOR[k], (cfg, f, k, e32)
    a, r64 = K.ballistics_reference(cfg)
    P = a["P"].double().numpy()
    ca, cr = (R.item_constants(sr, hop, a[k].numpy())[0] for k in R.CTL)
    for t in att + rel:                                                       # c is exactly 1 only where exp underflows in any library
        x = R.LN9 * hop / (sr * t / 1000.0)
        assert x < 30.0 or x > 100.0, (cfg, t, x)
    for s in (1.0, -1.0):
        e, up = np.zeros(len(P)), np.zeros(P.shape, bool)
        xa, xr = (np.where(c < 1.0, np.nextafter(c, c + s), c) for c in (ca, cr))
        for j in range(P.shape[1]):
            u = P[:, j] > e
            e = e + np.where(u, xa, xr) * (P[:, j] - e)
            up[:, j] = u
        assert np.array_equal(up, r64["up"]), (cfg, s)


def test_the_configurations_cover_the_orders_of_the_two_times():
    pairs = [(a, r) for c in K.BALLISTICS_CONFIGS for a, r in zip(c[2], c[3])]
    assert any(a > r for a, r in pairs) and any(a == r for a, r in pairs) and any(a < r for a, r in pairs)
    assert {t for p in pairs for t in p} == set(K.TIMES)
    assert K.frame_counts() == [1, 2, 3, K.CHUNK - 1, K.CHUNK, K.CHUNK + 1, 2 * K.CHUNK + 3, 16385] and _lib.lib().dasp_ballistics_chunk() == K.CHUNK


def test_bad_arguments_raise_before_the_device_is_asked_for():
    """The curve is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    P, one = torch.zeros(2, 9), torch.ones(2)
    with pytest.raises(RuntimeError, match=r"attack_ms: shape '\[2\]' is invalid for input of size 3"):
        D.ballistics(P, 44100, torch.ones(3), one)
    with pytest.raises(RuntimeError, match=r"release_ms: shape '\[2\]' is invalid for input of size 1"):
        D.ballistics(P, 44100, one, torch.ones(1))
    with pytest.raises(RuntimeError, match="curve: expected shape"):
        D.ballistics(torch.zeros(2, 1, 9), 44100, one, one)
    for sr in (0, -8000, float("nan"), float("inf"), "fast"):
        with pytest.raises(ValueError, match="ballistics: finite sample_rate"):
            D.ballistics(P, sr, one, one)
    for hop in (0, 4, 24, 4096, 64.0, True):
        with pytest.raises(ValueError, match="ballistics: hop"):
            D.ballistics(P, 44100, one, one, hop=hop)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.ballistics(P, 44100, one, one)


def test_float64_is_refused(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="ballistics: float64"):
        D.ballistics(torch.zeros(2, 9, dtype=torch.float64), 44100, torch.ones(2), torch.ones(2))


def test_sidechain_compressor_checks_its_arguments_before_the_device_is_asked_for():
    x, one = torch.zeros(2, 2, 100), torch.ones(2)
    ok = dict(threshold_db=-one, ratio=4 * one, attack_ms=one, release_ms=one, knee_db=one, makeup_gain_db=one)
    for name in ok:
        with pytest.raises(RuntimeError, match=name + r": shape '\[2\]' is invalid for input of size 3"):
            D.sidechain_compressor(x, 44100, **{**ok, name: torch.ones(3)})
    for key in (torch.zeros(2, 1, 99), torch.zeros(3, 1, 100), torch.zeros(2, 100)):
        with pytest.raises(RuntimeError, match="key: expected shape"):
            D.sidechain_compressor(x, 44100, **ok, key=key)
    with pytest.raises(ValueError, match="sidechain_compressor: finite sample_rate"):
        D.sidechain_compressor(x, 0, **ok)
    with pytest.raises(ValueError, match="block_level: hop"):
        D.sidechain_compressor(x, 44100, **ok, hop=24)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.sidechain_compressor(x, 44100, **ok)
    m = D.SidechainCompressor(44100, hop=8)
    assert list(m.param_ranges) == list(D.Compressor(44100).param_ranges) and m.param_ranges == D.Compressor(44100).param_ranges and m.hop == 8
    with pytest.raises(ValueError):
        D.SidechainCompressor(44100, hop=24)


def test_the_soft_knee_curve_and_its_gradients_at_knee_zero():
    from dasp_pytorch_amd.functional import _soft_knee_level
    l = torch.linspace(-60.0, 0.0, 241, dtype=torch.float64)[None].requires_grad_(True)
    T, Rt = torch.tensor([[-24.0]], dtype=torch.float64), torch.tensor([[4.0]], dtype=torch.float64)
    for W in (0.0, 6.0):
        Wt = torch.tensor([[W]], dtype=torch.float64, requires_grad=True)
        g = _soft_knee_level(l, T, Rt, Wt)
        lo, hi = l.detach() < -24.0 - W / 2, l.detach() > -24.0 + W / 2
        assert torch.equal(g[lo], l.detach()[lo]) and torch.allclose(g[hi], -24.0 + (l.detach()[hi] + 24.0) / 4.0, rtol=0, atol=1e-12)
        assert (l.detach() - g.detach()).min() >= 0 and (g[0, 1:] - g[0, :-1]).min() > 0          # the reduction is >= 0, the curve increases
        gl, gW = torch.autograd.grad(g.sum(), [l, Wt])
        assert torch.isfinite(gl).all() and torch.isfinite(gW).all()


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, impossible sizes and rates, DASP_ERR_UNSUPPORTED (-2) for a hop that is no power of two from
    8 to 2048 - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, F=1000, hop=64, sr=44100.0)

    def fwd(p=f, at=f, re=f, out=f, up=f, **kw):
        a = {**ok, **kw}
        return L.dasp_ballistics_forward(p, at, re, out, up, a["B"], a["F"], a["hop"], a["sr"], None)

    def bwd(p=f, at=f, re=f, out=f, up=f, go=f, gp=f, ga=f, gr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_ballistics_backward(p, at, re, out, up, go, gp, ga, gr, a["B"], a["F"], a["hop"], a["sr"], None)
    for call in (fwd, bwd):
        for kw in (dict(p=None), dict(at=None), dict(re=None), dict(out=None), dict(B=0), dict(F=0), dict(hop=0), dict(sr=0.0), dict(sr=float("nan")),
                   dict(sr=float("inf"))):
            assert call(**kw) == -1, (call.__name__, kw)
        for hop in (4, 24, 4096):
            assert call(hop=hop) == -2
    assert bwd(up=None) == -1 and bwd(go=None) == -1 and bwd(gp=None, ga=None, gr=None) == -1
