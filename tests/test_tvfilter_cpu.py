"""Host-side checks of time_varying_filter (no GPU): the restatement (tests/tvfilter_restated.py) against the RBJ biquads on constant
curves, an oracle that shares no code with it; the adjoint that csrc/tvfilter.hip implements, written out by hand, against autograd of
the sample loop, down to the frame values; what the definition says about clamped and NaN frame values and about the last frame point;
signal.control_frames; the size queries and argument checks of the C ABI; the errors of the Python layer and modules.TimeVaryingFilter."""
import inspect
import math

import numpy as np
import pytest
import scipy.signal
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import tvfilter_restated as R


def _draw(B, C, N, hop, seed=0, sr=44100):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo
    F = R.control_frames(N, hop)
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g, dtype=torch.float64),
                cutoff_hz=torch.exp(u(math.log(50.0), math.log(12000.0), B, F)) * sr / 44100, q=torch.exp(u(math.log(0.5), math.log(8.0), B, F)), mix=u(0.2, 1.0, B))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def rbj(kind, f, Q, sr):
    """The Audio EQ Cookbook's low_pass, high_pass and constant-peak band-pass, alpha = sin w0 / 2Q: (b, a)."""
    w0 = 2 * math.pi * f / sr
    al, c = math.sin(w0) / (2 * Q), math.cos(w0)
    b = {"lowpass": [(1 - c) / 2, 1 - c, (1 - c) / 2], "highpass": [(1 + c) / 2, -(1 + c), (1 + c) / 2], "bandpass": [al, 0.0, -al]}[kind]
    return np.array(b), np.array([1 + al, -2 * c, 1 - al])


@pytest.mark.parametrize("mode", ["lowpass", "highpass", "bandpass"])
@pytest.mark.parametrize("f_over_sr,Q", [(1 / 4096, 30.0), (1 / 4096, 0.5), (0.49, 30.0), (0.49, 0.5)])
def test_constant_curves_equal_the_rbj_biquad(mode, f_over_sr, Q):
    sr, N, hop = 44100, 3000, 64
    f = f_over_sr * sr
    x = torch.rand(1, 1, N, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 1
    F = R.control_frames(N, hop)
    y = R.time_varying_filter(x, sr, torch.full((1, F), f, dtype=torch.float64), torch.full((1, F), Q, dtype=torch.float64), torch.ones(1, dtype=torch.float64), hop, mode)
    b, a = rbj(mode, f, Q, sr)
    want = scipy.signal.lfilter(b, a, x[0, 0].numpy())
    assert np.abs(y[0, 0].numpy() - want).max() <= 1e-9 * max(np.abs(want).max(), 1.0)


def test_notch_is_lowpass_plus_highpass():
    d = _draw(2, 2, 400, 8)
    lp, hp, no = (R.time_varying_filter(d["x"], 44100, d["cutoff_hz"], d["q"], torch.ones(2, dtype=torch.float64), 8, m) for m in ("lowpass", "highpass", "notch"))
    assert (lp + hp - no).abs().max() < 1e-12


@pytest.mark.parametrize("mode", R.MODES)
def test_hand_adjoint_equals_autograd_of_the_sample_loop(mode):
    """(3, 2, 700) at hop 64, float64: gx, gmix and the gradients of every frame value of both curves - through gg[n] and gk[n], the
    halves of the intervals and dG / dcutoff, dK / dq - agree with autograd to rounding."""
    sr, N, hop = 44100, 700, 64
    d = _draw(3, 2, N, hop, seed=1)
    want = R.forward_backward(d["x"], sr, d["cutoff_hz"], d["q"], d["mix"], d["w"], hop, mode)
    G, K = R.frame_points(sr, d["cutoff_hz"], d["q"])
    g, k = (R.interpolate(P, N, hop).repeat_interleave(2, 0).numpy() for P in (G, K))
    hx, hg, hk, hm = R.adjoint_by_hand(d["x"].reshape(6, -1), g, k, d["mix"].repeat_interleave(2), d["w"].reshape(6, -1), mode)
    F = R.control_frames(N, hop)
    gG, gK = (R.frame_gradients(t, hop, F).reshape(3, 2, F).sum(1) for t in (hg, hk))
    hc, hq = R.curve_gradients(sr, d["cutoff_hz"], d["q"], gG, gK)
    rel = lambda p, q: np.abs(p - q).max() / np.abs(q).max()
    assert rel(hx.reshape(3, 2, N), want["gx"]) < 1e-11
    assert rel(hm.reshape(3, 2).sum(1), want["gmix"]) < 1e-11
    assert rel(hc, want["gcutoff"]) < 1e-10 and rel(hq, want["gq"]) < 1e-10


def test_mix_zero_is_the_identity():
    d = _draw(2, 2, 300, 64)
    for arith in (torch.float64, torch.float32):
        y = R.time_varying_filter(d["x"], 44100, d["cutoff_hz"], d["q"], torch.zeros(2, dtype=torch.float64), 64, "bandpass", arith)
        assert torch.equal(y, d["x"].to(arith))


def test_clamped_frame_values_get_exactly_zero_and_only_they():
    sr, N, hop = 44100, 300, 64
    d = _draw(2, 2, N, hop, seed=2)
    d["cutoff_hz"][0, 1], d["cutoff_hz"][1, 2], d["q"][0, 3], d["q"][1, 0] = 1.0, 30000.0, 0.01, 1000.0
    for arith in (torch.float64, torch.float32):
        r = R.forward_backward(d["x"], sr, d["cutoff_hz"], d["q"], d["mix"], d["w"], hop, "lowpass", arith)
        zc, zq = np.zeros((2, 6), bool), np.zeros((2, 6), bool)
        zc[0, 1] = zc[1, 2] = zq[0, 3] = zq[1, 0] = True
        assert np.array_equal(r["gcutoff"] == 0.0, zc) and np.array_equal(r["gq"] == 0.0, zq)
    e = {k: v.clone() for k, v in d.items()}
    e["cutoff_hz"][0, 1], e["cutoff_hz"][1, 2], e["q"][0, 3], e["q"][1, 0] = sr / 4096, 0.49 * sr, 0.1, 100.0
    y = [R.time_varying_filter(t["x"], sr, t["cutoff_hz"], t["q"], t["mix"], hop) for t in (d, e)]
    assert torch.equal(*y)


def test_the_last_frame_point():
    """Frame point F - 1 is the end of the last interval: it takes t gg of that interval's samples. Its gradient is exactly zero when the
    only sample of the last interval sits on frame point F - 2 (seq_len = 1 mod hop: t = 0 there), and not when hop divides seq_len."""
    for N, zero in ((129, True), (128, False), (100, False), (1, True)):
        d = _draw(1, 1, N, 64, seed=N)
        r = R.forward_backward(d["x"], 44100, d["cutoff_hz"], d["q"], d["mix"], d["w"], 64, "lowpass")
        assert (r["gcutoff"][0, -1] == 0.0) == zero and (r["gq"][0, -1] == 0.0) == zero, N
        assert r["gcutoff"][0, :-1].all()


@pytest.mark.parametrize("which", ["cutoff_hz", "q"])
def test_a_nan_frame_value_reaches_its_item_from_the_interval_before_it(which):
    N, hop = 200, 8
    d = _draw(2, 1, N, hop)
    clean = R.time_varying_filter(d["x"], 44100, d["cutoff_hz"], d["q"], d["mix"], hop)
    for j in (0, 1, 7, R.control_frames(N, hop) - 1):
        e = {k: v.clone() for k, v in d.items()}
        e[which][1, j] = float("nan")
        y = R.time_varying_filter(e["x"], 44100, e["cutoff_hz"], e["q"], e["mix"], hop)
        n0 = max(j - 1, 0) * hop
        assert torch.isnan(y[1, 0, n0:]).all() and torch.equal(y[1, 0, :n0], clean[1, 0, :n0]) and torch.equal(y[0], clean[0]), j


def test_control_frames():
    S = D.signal
    assert [S.control_frames(n, 64) for n in (0, 1, 63, 64, 65, 128, 129)] == [1, 2, 2, 2, 3, 3, 4]
    assert S.control_frames(7, 2048) == 2 and S.control_frames(6149, 8) == 770 and S.control_frames(6149, 2048) == 5
    for n in (1, 100, 2048, 6149):
        for hop in (8, 64, 2048):
            assert S.control_frames(n, hop) == R.control_frames(n, hop) == math.ceil(n / hop) + 1
    for hop in (0, 4, 7, 24, 4096, -8, 8.0, True, None):
        with pytest.raises(ValueError, match="hop"):
            S.control_frames(100, hop)
    for n in (-1, 2.5, None):
        with pytest.raises(ValueError, match="seq_len"):
            S.control_frames(n, 64)
    assert D.control_frames is S.control_frames


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    T = L.dasp_tvfilter_tile()
    assert T == 2048
    for rows in (1, 3, 128):
        for N, nt in ((1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (3 * T + 5, 4)):
            assert L.dasp_tvfilter_state_floats(rows, N) == rows * nt * 2
            for hop in (8, 64, 2048):
                assert L.dasp_tvfilter_frames(N, hop) == R.control_frames(N, hop)
                assert L.dasp_tvfilter_scratch_floats(rows, N, hop) == rows * (2 * R.control_frames(N, hop) + 1)
    assert L.dasp_tvfilter_state_floats(0, 10) == -1 and L.dasp_tvfilter_state_floats(4, 0) == -1
    assert L.dasp_tvfilter_frames(0, 64) == -1 and L.dasp_tvfilter_frames(10, 0) == -1
    assert L.dasp_tvfilter_scratch_floats(0, 10, 64) == -1 and L.dasp_tvfilter_scratch_floats(4, 0, 64) == -1 and L.dasp_tvfilter_scratch_floats(4, 10, -8) == -1
    for hop in (4, 24, 4096):
        assert L.dasp_tvfilter_frames(10, hop) == -2 and L.dasp_tvfilter_scratch_floats(4, 10, hop) == -2


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers, impossible sizes and modes, DASP_ERR_UNSUPPORTED (-2) for a hop that is no power of two from 8
    to 2048 and a grid beyond 2^31 rows - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, hop=64, mode=0, sr=44100.0)

    def fwd(x=f, cut=f, q=f, mix=f, y=f, st=f, **kw):
        a = {**ok, **kw}
        return L.dasp_tvfilter_forward(x, cut, q, mix, y, st, a["B"], a["C"], a["N"], a["hop"], a["mode"], a["sr"], None)

    def bwd(x=f, cut=f, q=f, mix=f, st=f, gy=f, gx=f, gcut=f, gq=f, gmix=f, scr=f, **kw):
        a = {**ok, **kw}
        return L.dasp_tvfilter_backward(x, cut, q, mix, st, gy, gx, gcut, gq, gmix, scr, a["B"], a["C"], a["N"], a["hop"], a["mode"], a["sr"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(cut=None) == -1 and call(q=None) == -1 and call(mix=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1 and call(hop=0) == -1 and call(hop=-64) == -1
        assert call(mode=-1) == -1 and call(mode=4) == -1
        assert call(sr=0.0) == -1 and call(sr=float("nan")) == -1 and call(sr=float("inf")) == -1
        assert call(hop=4) == -2 and call(hop=24) == -2 and call(hop=4096) == -2
        assert call(B=1 << 16, C=1 << 16) == -2
    assert fwd(y=None) == -1
    assert bwd(st=None) == -1 and bwd(gy=None) == -1 and bwd(gcut=None) == -1 and bwd(gq=None) == -1 and bwd(gmix=None) == -1 and bwd(scr=None) == -1


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def _controls(bs, N, hop=64):
    F = R.control_frames(N, hop)
    return [torch.full((bs, F), 1000.0), torch.full((bs, F), 2.0), torch.full((bs,), 0.5)]


@pytest.mark.parametrize("which,name", [(0, "cutoff_hz"), (1, "q")])
def test_wrong_frame_count_names_the_control_and_the_expected_count(which, name):
    for bad in (torch.zeros(2, 2), torch.zeros(2, 4), torch.zeros(2), torch.zeros(3, 3)):
        ctl = _controls(2, 100)
        ctl[which] = bad
        with pytest.raises(RuntimeError, match=rf"{name}: expected shape \[2, 3\]"):
            D.time_varying_filter(torch.zeros(2, 2, 100), 44100, *ctl)
    ctl = _controls(2, 100)
    ctl[2] = torch.zeros(5)
    with pytest.raises(RuntimeError, match="mix"):
        D.time_varying_filter(torch.zeros(2, 2, 100), 44100, *ctl)


def test_bad_scalars_raise_value_error_before_the_device_is_asked_for():
    """x is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    x = torch.zeros(1, 1, 8)
    for sr in (0, -8000, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="time_varying_filter"):
            D.time_varying_filter(x, sr, *_controls(1, 8))
    for hop in (0, 4, 24, 4096, 64.0, True):
        with pytest.raises(ValueError, match="hop"):
            D.time_varying_filter(x, 44100, *_controls(1, 8), hop=hop)
        with pytest.raises(ValueError, match="hop"):
            D.TimeVaryingFilter(44100, hop=hop)
    for mode in ("low_pass", "peak", 0, None):
        with pytest.raises(ValueError, match="mode"):
            D.time_varying_filter(x, 44100, *_controls(1, 8), mode=mode)
        with pytest.raises(ValueError, match="mode"):
            D.TimeVaryingFilter(44100, mode=mode)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.time_varying_filter(torch.zeros(2, 2, 64), 44100, *_controls(2, 64))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.TimeVaryingFilter(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 5), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="time_varying_filter: float64"):
        D.time_varying_filter(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2, 64))


def test_module_tables_and_denormalisation():
    names = list(inspect.signature(D.functional.time_varying_filter).parameters)
    assert names == ["x", "sample_rate", "cutoff_hz", "q", "mix", "hop", "mode"]
    m = D.TimeVaryingFilter(44100)
    assert list(m.param_ranges) == names[2:5]
    assert m.param_ranges == {"cutoff_hz": (50.0, 12000.0), "q": (0.5, 8.0), "mix": (0.0, 1.0)}
    assert m.hop == 64 and m.mode == "lowpass" and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.time_varying_filter and m.process_fn.keywords == {"hop": 64, "mode": "lowpass"}
    m = D.TimeVaryingFilter(48000, hop=8, mode="notch", min_cutoff_hz=100.0, max_cutoff_hz=2100.0, max_q=4.5, min_mix=0.5)
    assert m.process_fn.keywords == {"hop": 8, "mode": "notch"}
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    x = torch.zeros(3, 2, 20)
    F = 4                                                                  # ceil(20 / 8) + 1
    p = torch.rand(3, 2 * F + 1, generator=torch.Generator().manual_seed(0))
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and list(seen)[:3] == names[2:5]
    assert seen["cutoff_hz"].shape == (3, F) and seen["q"].shape == (3, F) and seen["mix"].shape == (3,)
    assert torch.allclose(seen["cutoff_hz"], p[:, :F] * 2000 + 100) and torch.allclose(seen["q"], p[:, F:2 * F] * 4 + 0.5)
    assert torch.allclose(seen["mix"], p[:, 2 * F] * 0.5 + 0.5)
    with pytest.raises(ValueError, match="9 parameters"):
        m.process_normalized(x, torch.rand(3, 2 * F))
    q = p.clone()
    q[1, F + 1] = 1.5
    with pytest.raises(ValueError, match="Parameter q of is out of range"):
        m.process_normalized(x, q)
    m.validate_range = "deferred"                                          # a CPU tensor is looked at at once
    with pytest.raises(ValueError, match="Parameter q of is out of range"):
        m.process_normalized(x, q)
    m.validate_range = False
    assert m.process_normalized(x, q) is x
    assert D.time_varying_filter is D.functional.time_varying_filter and D.TimeVaryingFilter is D.modules.TimeVaryingFilter
