"""Host-side checks of time_varying_eq (no GPU): the restatement (tests/tveq_restated.py) against the RBJ peaking and shelving biquads on
constant curves, an oracle that shares no code with it; the adjoint that csrc/tveq.hip implements, written out by hand, against autograd
of the sample loop, down to the frame values of all three curves; what the definition says about zero gain, clamped and NaN frame values
and the last frame point; the size queries and argument checks of the C ABI; the errors of the Python layer and modules.TimeVaryingEQ.
(signal.biquad runs on the device: the RBJ helper is pinned to it in tests/test_gpu_time_varying_eq.py.)"""
import inspect
import math

import numpy as np
import pytest
import scipy.signal
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import tveq_restated as R


def _draw(B, C, N, hop, seed=0, sr=44100):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo
    F = R.control_frames(N, hop)
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g, dtype=torch.float64), gain_db=u(-18.0, 18.0, B, F),
                cutoff_hz=torch.exp(u(math.log(50.0), math.log(12000.0), B, F)) * sr / 44100, q=torch.exp(u(math.log(0.5), math.log(8.0), B, F)))


def _ctl(d):
    return [d[k] for k in R.CTL]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("f,Q,db", [(100.0, 0.7, 12.0), (1000.0, 4.0, -18.0), (8000.0, 1.0, 6.0), (44100 / 4096, 10.0, -24.0), (0.45 * 44100, 0.5, 24.0)])
def test_constant_curves_equal_the_rbj_biquad(mode, f, Q, db):
    sr, N, hop = 44100, 4000, 64
    x = torch.rand(1, 1, N, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 1
    F = R.control_frames(N, hop)
    y = R.time_varying_eq(x, sr, *[torch.full((1, F), v, dtype=torch.float64) for v in (db, f, Q)], hop, mode)
    want = scipy.signal.lfilter(*R.rbj(mode, f, Q, db, sr), x[0, 0].numpy())
    err = np.abs(y[0, 0].numpy() - want).max() / np.abs(want).max()
    print(f"RBJ {mode} f={f:.2f} Q={Q} dB={db}: {err:.3e}")
    assert err <= 1e-9


def test_rbj_helper_is_the_cookbook():
    """Against scipy-free closed forms at one point each: unit gain away from the band, the full gain inside it."""
    sr = 48000
    for mode, f_in, f_out in (("bell", 1000.0, 20.0), ("lowshelf", 20.0, 20000.0), ("highshelf", 20000.0, 20.0)):
        b, a = R.rbj(mode, 1000.0, 0.7071, 12.0, sr)
        H = lambda f: abs(np.polyval(b[::-1], np.exp(-2j * math.pi * f / sr)) / np.polyval(a[::-1], np.exp(-2j * math.pi * f / sr)))
        assert abs(20 * math.log10(H(f_in)) - 12.0) < 0.1 and abs(20 * math.log10(H(f_out))) < 0.1, mode


@pytest.mark.parametrize("mode", R.MODES)
def test_hand_adjoint_equals_autograd_of_the_sample_loop(mode):
    """(3, 2, 700) at hop 64, float64: gx and the gradients of every frame value of the three curves - through gg[n], gk[n] and gA[n], the
    halves of the intervals and the chain from (G, K, A) to (gain_db, cutoff_hz, q) - agree with autograd to rounding."""
    sr, N, hop = 44100, 700, 64
    d = _draw(3, 2, N, hop, seed=1)
    want = R.forward_backward(d["x"], sr, *_ctl(d), d["w"], hop, mode)
    G, K, A = R.frame_points(sr, *_ctl(d), mode)
    g, k, a = (R.interpolate(P, N, hop).repeat_interleave(2, 0).numpy() for P in (G, K, A))
    hx, hg, hk, ha = R.adjoint_by_hand(d["x"].reshape(6, -1), g, k, a, d["w"].reshape(6, -1), mode)
    F = R.control_frames(N, hop)
    gG, gK, gA = (R.frame_gradients(t, hop, F).reshape(3, 2, F).sum(1) for t in (hg, hk, ha))
    got = dict(zip(R.GRADS, R.curve_gradients(sr, *_ctl(d), gG, gK, gA, mode)))
    rel = lambda p, q: np.abs(p - q).max() / np.abs(q).max()
    assert rel(hx.reshape(3, 2, N), want["gx"]) < 1e-11
    for name in R.GRADS:
        assert rel(got[name], want[name]) < 1e-10, name


@pytest.mark.parametrize("mode", R.MODES)
def test_zero_gain_is_the_identity_and_its_gain_gradient_is_not_zero(mode):
    d = _draw(2, 2, 300, 64)
    z = torch.zeros_like(d["gain_db"])
    for arith in (torch.float64, torch.float32):
        y = R.time_varying_eq(d["x"], 44100, z, d["cutoff_hz"], d["q"], 64, mode, arith)
        assert torch.equal(y, d["x"].to(arith))
        r = R.forward_backward(d["x"], 44100, z, d["cutoff_hz"], d["q"], d["w"], 64, mode, arith)
        assert np.array_equal(r["gx"], d["w"].to(arith).double().numpy()) and r["ggain"].all() and not r["gcutoff"].any() and not r["gq"].any()


def test_bell_up_then_down_is_the_identity_up_to_rounding():
    d = _draw(2, 1, 600, 64, seed=3)
    up = R.time_varying_eq(d["x"], 44100, torch.full_like(d["gain_db"], 12.0), d["cutoff_hz"][:, :1].expand_as(d["q"]), d["q"][:, :1].expand_as(d["q"]), 64, "bell")
    back = R.time_varying_eq(up, 44100, torch.full_like(d["gain_db"], -12.0), d["cutoff_hz"][:, :1].expand_as(d["q"]), d["q"][:, :1].expand_as(d["q"]), 64, "bell")
    assert float((back - d["x"]).abs().max()) < 1e-12


@pytest.mark.parametrize("mode", R.MODES)
def test_clamped_frame_values_get_exactly_zero_and_only_they(mode):
    sr, N, hop = 44100, 300, 64
    d = _draw(2, 2, N, hop, seed=2)
    d["gain_db"][0, 0], d["gain_db"][1, 4], d["cutoff_hz"][0, 1], d["cutoff_hz"][1, 2], d["q"][0, 3], d["q"][1, 0] = 50.0, -41.0, 1.0, 30000.0, 0.01, 1000.0
    zero = {k: np.zeros((2, 6), bool) for k in R.GRADS}
    zero["ggain"][0, 0] = zero["ggain"][1, 4] = zero["gcutoff"][0, 1] = zero["gcutoff"][1, 2] = zero["gq"][0, 3] = zero["gq"][1, 0] = True
    for arith in (torch.float64, torch.float32):
        r = R.forward_backward(d["x"], sr, *_ctl(d), d["w"], hop, mode, arith)
        for k in R.GRADS:
            assert np.array_equal(r[k] == 0.0, zero[k]), (k, arith)
    e = {k: v.clone() for k, v in d.items()}
    e["gain_db"][0, 0], e["gain_db"][1, 4], e["cutoff_hz"][0, 1], e["cutoff_hz"][1, 2], e["q"][0, 3], e["q"][1, 0] = 40.0, -40.0, sr / 4096, 0.49 * sr, 0.1, 100.0
    y = [R.time_varying_eq(t["x"], sr, *_ctl(t), hop, mode) for t in (d, e)]
    assert torch.equal(*y)


def test_the_last_frame_point():
    """Frame point F - 1 is the end of the last interval: it takes t of that interval's samples. Its gradients are exactly zero when the
    only sample of the last interval sits on frame point F - 2 (seq_len = 1 mod hop: t = 0 there), and not when hop divides seq_len."""
    for N, zero in ((129, True), (128, False), (100, False), (1, True)):
        d = _draw(1, 1, N, 64, seed=N)
        r = R.forward_backward(d["x"], 44100, *_ctl(d), d["w"], 64, "lowshelf")
        for k in R.GRADS:
            assert (r[k][0, -1] == 0.0) == zero, (N, k)
            assert r[k][0, :-1].all(), (N, k)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("which", R.CTL)
def test_a_nan_frame_value_reaches_its_item_from_the_interval_before_it(which, mode):
    N, hop = 200, 8
    d = _draw(2, 1, N, hop)
    clean = R.time_varying_eq(d["x"], 44100, *_ctl(d), hop, mode)
    for j in (0, 1, 7, R.control_frames(N, hop) - 1):
        e = {k: v.clone() for k, v in d.items()}
        e[which][1, j] = float("nan")
        y = R.time_varying_eq(e["x"], 44100, *_ctl(e), hop, mode)
        n0 = max(j - 1, 0) * hop
        assert torch.isnan(y[1, 0, n0:]).all() and torch.equal(y[1, 0, :n0], clean[1, 0, :n0]) and torch.equal(y[0], clean[0]), j


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    T = L.dasp_tveq_tile()
    assert T == 2048 == L.dasp_tvfilter_tile()
    for rows in (1, 3, 128):
        for N, nt in ((1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (3 * T + 5, 4)):
            assert L.dasp_tveq_state_floats(rows, N) == rows * nt * 2
            for hop in (8, 64, 2048):
                assert L.dasp_tveq_scratch_floats(rows, N, hop) == rows * 3 * R.control_frames(N, hop)
    assert L.dasp_tveq_state_floats(0, 10) == -1 and L.dasp_tveq_state_floats(4, 0) == -1
    assert L.dasp_tveq_scratch_floats(0, 10, 64) == -1 and L.dasp_tveq_scratch_floats(4, 0, 64) == -1 and L.dasp_tveq_scratch_floats(4, 10, -8) == -1
    for hop in (4, 24, 4096):
        assert L.dasp_tveq_scratch_floats(4, 10, hop) == -2


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, impossible sizes and modes, DASP_ERR_UNSUPPORTED (-2) for a hop that is no power of two from 8
    to 2048 and a grid beyond 2^31 rows - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, hop=64, mode=0, sr=44100.0)

    def fwd(x=f, gain=f, cut=f, q=f, y=f, st=f, **kw):
        a = {**ok, **kw}
        return L.dasp_tveq_forward(x, gain, cut, q, y, st, a["B"], a["C"], a["N"], a["hop"], a["mode"], a["sr"], None)

    def bwd(x=f, gain=f, cut=f, q=f, st=f, gy=f, gx=f, ggain=f, gcut=f, gq=f, scr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_tveq_backward(x, gain, cut, q, st, gy, gx, ggain, gcut, gq, scr, a["B"], a["C"], a["N"], a["hop"], a["mode"], a["sr"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(gain=None) == -1 and call(cut=None) == -1 and call(q=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1 and call(hop=0) == -1 and call(hop=-64) == -1
        assert call(mode=-1) == -1 and call(mode=3) == -1
        assert call(sr=0.0) == -1 and call(sr=float("nan")) == -1 and call(sr=float("inf")) == -1
        assert call(hop=4) == -2 and call(hop=24) == -2 and call(hop=4096) == -2
        assert call(B=1 << 16, C=1 << 16) == -2
    assert fwd(y=None) == -1
    assert bwd(st=None) == -1 and bwd(gy=None) == -1 and bwd(ggain=None) == -1 and bwd(gcut=None) == -1 and bwd(gq=None) == -1 and bwd(scr=None) == -1


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def _controls(bs, N, hop=64):
    F = R.control_frames(N, hop)
    return [torch.full((bs, F), 3.0), torch.full((bs, F), 1000.0), torch.full((bs, F), 2.0)]


@pytest.mark.parametrize("which,name", list(enumerate(R.CTL)))
def test_wrong_frame_count_names_the_control_and_the_expected_count(which, name):
    for bad in (torch.zeros(2, 2), torch.zeros(2, 4), torch.zeros(2), torch.zeros(3, 3)):
        ctl = _controls(2, 100)
        ctl[which] = bad
        with pytest.raises(RuntimeError, match=rf"{name}: expected shape \[2, 3\]"):
            D.time_varying_eq(torch.zeros(2, 2, 100), 44100, *ctl)


def test_bad_scalars_raise_value_error_before_the_device_is_asked_for():
    """x is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    x = torch.zeros(1, 1, 8)
    for sr in (0, -8000, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="time_varying_eq"):
            D.time_varying_eq(x, sr, *_controls(1, 8))
    for hop in (0, 4, 24, 4096, 64.0, True):
        with pytest.raises(ValueError, match="hop"):
            D.time_varying_eq(x, 44100, *_controls(1, 8), hop=hop)
        with pytest.raises(ValueError, match="hop"):
            D.TimeVaryingEQ(44100, hop=hop)
    for mode in ("peaking", "low_shelf", "lowpass", 0, None):
        with pytest.raises(ValueError, match="mode"):
            D.time_varying_eq(x, 44100, *_controls(1, 8), mode=mode)
        with pytest.raises(ValueError, match="mode"):
            D.TimeVaryingEQ(44100, mode=mode)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.time_varying_eq(torch.zeros(2, 2, 64), 44100, *_controls(2, 64))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.TimeVaryingEQ(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 6), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="time_varying_eq: float64"):
        D.time_varying_eq(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2, 64))


def test_module_tables_and_denormalisation():
    names = list(inspect.signature(D.functional.time_varying_eq).parameters)
    assert names == ["x", "sample_rate", "gain_db", "cutoff_hz", "q", "hop", "mode"]
    m = D.TimeVaryingEQ(44100)
    assert list(m.param_ranges) == names[2:5] == list(R.CTL)
    assert m.param_ranges == {"gain_db": (-24.0, 24.0), "cutoff_hz": (50.0, 12000.0), "q": (0.5, 8.0)}
    assert m.hop == 64 and m.mode == "bell" and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.time_varying_eq and m.process_fn.keywords == {"hop": 64, "mode": "bell"}
    m = D.TimeVaryingEQ(48000, hop=8, mode="highshelf", min_gain_db=-12.0, max_gain_db=6.0, min_cutoff_hz=100.0, max_cutoff_hz=2100.0, max_q=4.5)
    assert m.process_fn.keywords == {"hop": 8, "mode": "highshelf"}
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    x = torch.zeros(3, 2, 20)
    F = 4                                                                  # ceil(20 / 8) + 1
    p = torch.rand(3, 3 * F, generator=torch.Generator().manual_seed(0))
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and list(seen)[:3] == names[2:5]
    assert all(seen[k].shape == (3, F) for k in R.CTL)
    assert torch.allclose(seen["gain_db"], p[:, :F] * 18 - 12) and torch.allclose(seen["cutoff_hz"], p[:, F:2 * F] * 2000 + 100)
    assert torch.allclose(seen["q"], p[:, 2 * F:] * 4 + 0.5)
    with pytest.raises(ValueError, match="12 parameters"):
        m.process_normalized(x, torch.rand(3, 3 * F + 1))
    q = p.clone()
    q[1, 2 * F + 1] = 1.5
    with pytest.raises(ValueError, match="Parameter q of is out of range"):
        m.process_normalized(x, q)
    m.validate_range = "deferred"                                          # a CPU tensor is looked at at once
    with pytest.raises(ValueError, match="Parameter q of is out of range"):
        m.process_normalized(x, q)
    m.validate_range = False
    assert m.process_normalized(x, q) is x
    assert D.time_varying_eq is D.functional.time_varying_eq and D.TimeVaryingEQ is D.modules.TimeVaryingEQ
    assert D.functional.TVEQ_MODES == R.MODES
