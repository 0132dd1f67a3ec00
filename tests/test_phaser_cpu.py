"""Host-side checks of phaser (no GPU): the adjoint that csrc/phaser.hip implements, written out by hand, against autograd of the
restatement (tests/phaser_restated.py); the identities the restatement must satisfy (mix = 0, the K-sample shift at a = 0, the energy of
an all-pass); the exact zero that clamped samples contribute to the sweep gradients; the size queries and argument checks of the C ABI;
the errors of the Python layer and modules.Phaser."""
import inspect
import math

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import phaser_restated as R


def _draw(B, C, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g, dtype=torch.float64), rate_hz=u(-10.0, 10.0, B), center_hz=u(300.0, 3000.0, B),
                depth=u(0.5, 2.0, B), phase=u(0.0, 1.0, B), mix=u(0.2, 1.0, B))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_hand_adjoint_equals_autograd_of_the_sample_loop():
    """(3, 2, 1500), K = 4, float64: gx, the gradient of the coefficient sequence a and gmix agree to rounding."""
    sr, K = 44100, 4
    d = _draw(3, 2, 1500)
    _, a = R.sweep(sr, d["rate_hz"], d["center_hz"], d["depth"], d["phase"], 2, 1500)
    x = d["x"].clone().requires_grad_(True)
    al = a.detach().clone().requires_grad_(True)
    mix = d["mix"].clone().requires_grad_(True)
    m = mix[:, None, None]
    y = (1 - m) * x + m * R.cascade(x, al, K)
    gx, ga, gmix = torch.autograd.grad((y * d["w"]).sum(), [x, al, mix])
    hx, ha, hm = R.adjoint_by_hand(d["x"].reshape(6, -1), a.reshape(6, -1), d["mix"].repeat_interleave(2), d["w"].reshape(6, -1), K)
    rel = lambda p, q: np.abs(p - q).max() / np.abs(q).max()
    assert rel(hx, gx.reshape(6, -1).numpy()) < 1e-12
    assert rel(ha, ga.reshape(6, -1).numpy()) < 1e-12
    assert rel(hm.reshape(3, 2).sum(1), gmix.numpy()) < 1e-12


def test_mix_zero_is_the_identity():
    d = _draw(2, 2, 300)
    for arith in (torch.float64, torch.float32):
        y = R.phaser(d["x"], 44100, d["rate_hz"], d["center_hz"], d["depth"], d["phase"], torch.zeros(2, dtype=torch.float64), stages=4, arith=arith)
        assert torch.equal(y, d["x"].to(arith))


@pytest.mark.parametrize("K", [1, 4, 12])
def test_zero_coefficient_is_a_shift_by_the_number_of_stages(K):
    """depth = 0, center_hz = sample_rate / 4, mix = 1: t = tan(pi / 4), a = 0 to rounding, every stage is one sample of delay."""
    sr = 44100
    d = _draw(2, 2, 200)
    one, zero = torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    y = R.phaser(d["x"], sr, d["rate_hz"], one * sr / 4, zero, d["phase"], one, stages=K)
    assert not y[..., :K].abs().max() > 1e-14
    assert (y[..., K:] - d["x"][..., :-K]).abs().max() < 1e-13


def test_all_pass_keeps_the_energy():
    """depth = 0 (a constant coefficient), mix = 1, x zero over its last quarter: sum y^2 = sum x^2. With a = -0.41 (center_hz = sr / 8) what
    the 500 samples of silence cut off of the response is below 1e-150."""
    sr = 44100
    d = _draw(3, 2, 2000)
    d["x"][..., 1500:] = 0
    one, zero = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    y = R.phaser(d["x"], sr, d["rate_hz"], one * sr / 8, zero, d["phase"], one, stages=6)
    ex, ey = (d["x"] ** 2).sum(-1), (y ** 2).sum(-1)
    assert ((ey - ex).abs() / ex).max() < 1e-13


def test_clamped_samples_contribute_exactly_nothing_to_the_sweep_gradients():
    """Item 0 sits on the upper clamp all the time, item 1 on the lower one: exactly zero for rate_hz, center_hz, depth and phase, and
    a gradient for mix all the same. Item 2 sweeps through both clamps: its gradients equal those of the samples inside, taken alone."""
    sr, N = 44100, 600
    d = _draw(3, 2, N, seed=3)
    d["center_hz"] = torch.tensor([1e6, 1e-3, 1000.0], dtype=torch.float64)
    d["depth"] = torch.tensor([1.0, 1.0, 9.0], dtype=torch.float64)
    d["rate_hz"] = torch.tensor([3.0, -2.0, 200.0], dtype=torch.float64)
    for arith in (torch.float64, torch.float32):
        r = R.forward_backward(d["x"], sr, *[d[k] for k in R.CTL], d["w"], stages=4, arith=arith)
        for k in R.GRADS[:4]:
            assert r[k][0] == 0.0 and r[k][1] == 0.0 and r[k][2] != 0.0, (k, r[k])
        assert r["gmix"].all()
    raw, a = R.sweep(sr, d["rate_hz"], d["center_hz"], d["depth"], d["phase"], 2, N)
    lo, hi = R.clamp_bounds(sr)
    inside = ((raw >= lo) & (raw <= hi))[2]
    assert 0.1 * inside.numel() < inside.sum() < 0.9 * inside.numel() and (raw[2] < lo).any() and (raw[2] > hi).any()
    # the chain rule by hand over the samples inside: ga from the hand adjoint, da/df = 2 / (t + 1)^2 (pi / sr)(1 + t^2), f = raw there
    _, ga, _ = R.adjoint_by_hand(d["x"][2], a[2], d["mix"][2].repeat(2), d["w"][2], 4)
    t = torch.tan(math.pi * raw[2] / sr)
    dadf = (2 / (t + 1) ** 2 * (math.pi / sr) * (1 + t ** 2)).numpy()
    gcenter = (ga * dadf * (raw[2] / d["center_hz"][2]).numpy())[inside.numpy()].sum()
    want = R.forward_backward(d["x"], sr, *[d[k] for k in R.CTL], d["w"], stages=4)["gcenter"][2]
    assert abs(gcenter - want) <= 1e-10 * abs(want)


def test_nan_control_passes_the_clamp():
    d = _draw(2, 1, 50)
    for k in R.CTL:
        e = {q: v.clone() for q, v in d.items()}
        e[k][1] = float("nan")
        y = R.phaser(e["x"], 44100, *[e[q] for q in R.CTL], stages=2)
        assert torch.isnan(y[1]).all() and torch.isfinite(y[0]).all(), k


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    kmax = L.dasp_phaser_max_stages()
    assert kmax == 12
    for K in range(1, kmax + 1):
        T = L.dasp_phaser_tile(K)
        assert T >= 512 and T % 256 == 0
        assert (K + 4) * T * 4 + 2 * (T + T // 8) * 4 + 1024 <= 160 * 1024            # the backward kernel's rows and staging inside a workgroup's LDS
        for rows in (1, 3, 128):
            for N, nt in ((1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (2 * T + 5, 3)):
                assert L.dasp_phaser_state_floats(rows, N, K) == rows * nt * K
            assert L.dasp_phaser_state_floats(rows, 2 * T + 5, K) < (2 * T + 5) * rows / 8
            assert L.dasp_phaser_partial_floats(rows) == 5 * rows
    assert L.dasp_phaser_tile(0) == -1 and L.dasp_phaser_tile(kmax + 1) == -2
    assert L.dasp_phaser_state_floats(0, 10, 4) == -1 and L.dasp_phaser_state_floats(4, 0, 4) == -1 and L.dasp_phaser_state_floats(4, 10, 0) == -1
    assert L.dasp_phaser_state_floats(4, 10, kmax + 1) == -2 and L.dasp_phaser_partial_floats(0) == -1


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers and impossible sizes, DASP_ERR_UNSUPPORTED (-2) for too many stages and a grid beyond 2^31 rows -
    all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, K=4, sr=44100.0, spread=0.25)

    def fwd(x=f, ctl=f, y=f, st=f, **kw):
        a = {**ok, **kw}
        return L.dasp_phaser_forward(x, ctl, y, st, a["B"], a["C"], a["N"], a["K"], a["sr"], a["spread"], None)

    def bwd(x=f, ctl=f, st=f, gy=f, gx=f, gctl=f, part=f, **kw):
        a = {**ok, **kw}
        return L.dasp_phaser_backward(x, ctl, st, gy, gx, gctl, part, a["B"], a["C"], a["N"], a["K"], a["sr"], a["spread"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(ctl=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1 and call(K=0) == -1
        assert call(sr=0.0) == -1 and call(sr=float("nan")) == -1 and call(sr=float("inf")) == -1
        assert call(spread=float("nan")) == -1 and call(spread=float("inf")) == -1
        assert call(K=13) == -2
        assert call(B=1 << 16, C=1 << 16) == -2
    assert fwd(y=None) == -1
    assert bwd(st=None) == -1 and bwd(gy=None) == -1 and bwd(gctl=None) == -1 and bwd(part=None) == -1


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def _controls(bs):
    return [torch.full((bs,), 0.5), torch.full((bs,), 1000.0), torch.full((bs,), 1.0), torch.full((bs,), 0.0), torch.full((bs,), 0.5)]


@pytest.mark.parametrize("which,name", enumerate(R.CTL))
def test_wrong_control_count_names_the_control(which, name):
    ctl = _controls(2)
    ctl[which] = torch.zeros(5)
    with pytest.raises(RuntimeError, match=name):
        D.phaser(torch.zeros(2, 2, 64), 44100, *ctl)


def test_bad_scalars_raise_value_error_before_the_device_is_asked_for():
    """x is a CPU tensor: anything that got as far as the device would raise DaspHipError instead."""
    x = torch.zeros(1, 1, 8)
    for sr in (0, -8000, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="phaser"):
            D.phaser(x, sr, *_controls(1))
    for spread in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="phaser"):
            D.phaser(x, 44100, *_controls(1), stereo_spread=spread)
    for stages in (0, -1, 13, 2.5, True):
        with pytest.raises(ValueError, match="stages"):
            D.phaser(x, 44100, *_controls(1), stages=stages)
        with pytest.raises(ValueError, match="stages"):
            D.Phaser(44100, stages=stages)


def test_cpu_tensor_and_float64_are_refused(monkeypatch):
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.phaser(torch.zeros(2, 2, 64), 44100, *_controls(2))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.Phaser(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 5), 0.5))
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="phaser: float64"):
        D.phaser(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2))


def test_module_tables_and_plumbing():
    names = list(inspect.signature(D.functional.phaser).parameters)
    assert names == ["x", "sample_rate", "rate_hz", "center_hz", "depth", "phase", "mix", "stages", "stereo_spread"]
    m = D.Phaser(44100)
    assert m.num_params == 5 and list(m.param_ranges) == names[2:7]
    assert m.param_ranges == {"rate_hz": (0.05, 10.0), "center_hz": (200.0, 4000.0), "depth": (0.0, 2.0), "phase": (0.0, 1.0), "mix": (0.0, 1.0)}
    assert m.stages == 4 and m.sample_rate == 44100
    assert m.process_fn.func is D.functional.phaser and m.process_fn.keywords == {"stages": 4, "stereo_spread": 0.25}
    m = D.Phaser(48000, stages=8, max_center_hz=2200.0, stereo_spread=0.5)
    assert m.process_fn.keywords == {"stages": 8, "stereo_spread": 0.5}
    seen = {}

    def fake(x, sample_rate, **kw):
        seen.update(kw, sample_rate=sample_rate)
        return x
    m.process_fn = fake
    p = torch.rand(3, 5, generator=torch.Generator().manual_seed(0))
    x = torch.zeros(3, 2, 16)
    assert m.process_normalized(x, p) is x
    assert seen["sample_rate"] == 48000 and list(seen)[:5] == names[2:7]
    assert torch.allclose(seen["rate_hz"], p[:, 0] * 9.95 + 0.05) and torch.allclose(seen["center_hz"], p[:, 1] * 2000 + 200)
    assert torch.allclose(seen["depth"], p[:, 2] * 2) and torch.allclose(seen["mix"], p[:, 4])
    with pytest.raises(ValueError):
        m.process_normalized(x, torch.rand(3, 6))
    assert D.phaser is D.functional.phaser and D.Phaser is D.modules.Phaser
