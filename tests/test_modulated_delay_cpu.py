"""Host-side checks of modulated_delay (no GPU): the restatement (tests/modulated_delay_restated.py) against a direct double loop with
hand-derived gradients, the Catmull-Rom weights, the size queries and argument checks of the C ABI, the errors of the Python layer and
the parameter tables of modules.ModulatedDelay."""
import inspect

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests import modulated_delay_restated as R


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,clamped", [(1, False), (3, False), (2, True)])
def test_restatement_equals_the_direct_loop(V, clamped):
    """(2, 2, 40) at 8 kHz with delays of 0 - 2.5 ms, reads before the start of the signal included; `clamped`: max_delay_ms = 1, so that
    d sits on either bound for part of every LFO cycle. Both sides are float64: they agree to rounding, 1e-12 of each quantity's peak."""
    g = torch.Generator().manual_seed(11 + V)
    bs, chs, N, sr = 2, 2, 40, 8000
    x, gy = torch.randn(bs, chs, N, generator=g), torch.randn(bs, chs, N, generator=g)
    delay, depth = torch.rand(bs, V, generator=g) * 1.5, torch.rand(bs, V, generator=g)
    rate, phase, mix = torch.rand(bs, V, generator=g) * 300 + 50, torch.rand(bs, V, generator=g), torch.rand(bs, generator=g)
    mdm = 1.0 if clamped else 2.5
    a = R.forward_backward(x, sr, delay, depth, rate, phase, mix, gy, max_delay_ms=mdm)
    b = R.direct(x.numpy(), sr, delay.numpy(), depth.numpy(), rate.numpy(), phase.numpy(), mix.numpy(), gy.numpy(), max_delay_ms=mdm)
    if clamped:
        raw = sr / 1000.0 * (delay.double() + depth.double() * torch.tensor([-1.0, 1.0]).view(2, 1, 1))
        assert (raw < 0).any() and (raw > sr / 1000.0 * mdm).any()
    for k in R.NAMES:
        assert a[k].shape == b[k].shape, k
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * np.abs(b[k]).max(), k


def test_float32_position_is_what_the_kernel_avoids():
    """The figure behind the float64 position: at (2, 2, 20000), 44.1 kHz, three voices of 5 - 25 ms, a float32 position costs y more
    than 1e-4 of its peak; float32 arithmetic behind a float64 position stays under 1e-6."""
    g = torch.Generator().manual_seed(5)
    bs, chs, N, V, sr = 2, 2, 20000, 3, 44100
    x, gy = torch.rand(bs, chs, N, generator=g) * 2 - 1, torch.randn(bs, chs, N, generator=g)
    ctl = (torch.rand(bs, V, generator=g) * 15 + 8, torch.rand(bs, V, generator=g) * 3, torch.rand(bs, V, generator=g) * 5 + 0.1,
           torch.rand(bs, V, generator=g), torch.rand(bs, generator=g) * 0.5 + 0.5)
    ref = R.forward_backward(x, sr, *ctl, gy)["y"]
    e_arith = np.abs(R.forward_backward(x, sr, *ctl, gy, arith=torch.float32)["y"] - ref).max() / np.abs(ref).max()
    e_pos = np.abs(R.forward_backward(x, sr, *ctl, gy, pos=torch.float32, arith=torch.float32)["y"] - ref).max() / np.abs(ref).max()
    assert e_arith < 1e-6 and e_pos > 1e-4, (e_arith, e_pos)


def test_catmull_rom_weights():
    """The weights sum to 1, reproduce every quadratic (and so every line) exactly up to rounding, and at f = 0 pick x[i] alone."""
    f = torch.linspace(0, 1, 101, dtype=torch.float64)
    w = R.weights(f)
    assert torch.allclose(w.sum(-1), torch.ones_like(f), atol=1e-15)
    k = torch.tensor([-1.0, 0.0, 1.0, 2.0], dtype=torch.float64)
    for a, b, c in ((0.0, 1.0, 0.0), (1.0, -2.0, 0.5), (-0.3, 0.7, 2.0)):
        q = lambda t: a * t * t + b * t + c
        assert torch.allclose((w * q(k)).sum(-1), q(f), atol=1e-14)
    assert R.weights(torch.zeros(1, dtype=torch.float64)).abs().tolist() == [[0.0, 1.0, 0.0, 0.0]]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _lib.lib()
    vmax, hmax = L.dasp_moddelay_max_voices(), L.dasp_moddelay_max_delay_samples()
    assert vmax == 8 and hmax >= 8192
    tiles = [L.dasp_moddelay_tile(H) for H in range(1, hmax + 1, 97)] + [L.dasp_moddelay_tile(hmax)]
    assert all(t > 0 and t % 256 == 0 for t in tiles)
    assert all(a >= b for a, b in zip(tiles, tiles[1:]))                       # the tile shrinks or holds as H grows
    for H in (1, 320, 1764, hmax):
        T = L.dasp_moddelay_tile(H)
        assert (2 * T + H + 6) * 4 <= 160 * 1024                               # backward LDS inside a CU's 160 KiB
        for rows in (1, 3, 128):
            for N in (1, T - 1, T, T + 1, 5 * T + 1, 131072):
                for V in (1, 3, 8):
                    assert L.dasp_moddelay_partial_floats(rows, N, V, H) == rows * -(-N // T) * (4 * V + 1), (H, rows, N, V)
    assert L.dasp_moddelay_partial_floats(4, 1000, vmax + 1, 100) == -2        # nine voices
    assert L.dasp_moddelay_tile(hmax + 1) == -2 and L.dasp_moddelay_partial_floats(4, 1000, 1, hmax + 1) == -2
    assert L.dasp_moddelay_tile(0) == -1 and L.dasp_moddelay_partial_floats(0, 1000, 1, 100) == -1
    assert L.dasp_moddelay_partial_floats(4, 0, 1, 100) == -1 and L.dasp_moddelay_partial_floats(4, 1000, 0, 100) == -1


def test_entry_points_check_their_arguments_without_gpu():
    """DASP_ERR_ARG (-1) for null pointers and impossible sizes, DASP_ERR_UNSUPPORTED (-2) for nine voices, an H beyond the limit and a
    grid beyond 2^31 workgroups - all before any launch. The non-null device pointers are fakes, never read."""
    L = _lib.lib()
    f = 256
    ok = dict(B=2, C=2, N=1000, V=3, H=1764, sr=44100.0, mdm=40.0, spread=0.25)

    def fwd(x=f, ctl=f, mix=f, y=f, **kw):
        a = {**ok, **kw}
        return L.dasp_moddelay_forward(x, ctl, mix, y, a["B"], a["C"], a["N"], a["V"], a["H"], a["sr"], a["mdm"], a["spread"], None)

    def bwd(x=f, ctl=f, mix=f, gy=f, gx=f, gctl=f, gmix=f, part=f, **kw):
        a = {**ok, **kw}
        return L.dasp_moddelay_backward(x, ctl, mix, gy, gx, gctl, gmix, part, a["B"], a["C"], a["N"], a["V"], a["H"], a["sr"], a["mdm"],
                                        a["spread"], None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(ctl=None) == -1 and call(mix=None) == -1
        assert call(B=0) == -1 and call(C=-1) == -1 and call(N=0) == -1 and call(V=0) == -1 and call(H=0) == -1
        assert call(H=1763) == -1                                            # H below sr/1000 max_delay_ms = 1764
        assert call(sr=0.0) == -1 and call(sr=float("nan")) == -1 and call(mdm=-1.0) == -1 and call(mdm=float("nan")) == -1
        assert call(spread=float("inf")) == -1
        assert call(V=9) == -2
        assert call(H=L.dasp_moddelay_max_delay_samples() + 1) == -2
        assert call(B=1 << 15, C=1 << 15, N=1 << 20) == -2
    assert fwd(y=None) == -1
    assert bwd(gy=None) == -1 and bwd(gctl=None) == -1 and bwd(gmix=None) == -1 and bwd(part=None) == -1


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def _controls(bs, V):
    return [torch.full((bs, V), 10.0), torch.full((bs, V), 2.0), torch.full((bs, V), 1.0), torch.zeros(bs, V), torch.full((bs,), 0.5)]


@pytest.mark.parametrize("which,name", enumerate(("delay_ms", "depth_ms", "rate_hz", "phase", "mix")))
def test_wrong_control_count_names_the_control(which, name):
    x = torch.zeros(2, 2, 64)
    ctl = _controls(2, 3)
    ctl[which] = torch.zeros(5)
    with pytest.raises(RuntimeError, match=name):
        D.modulated_delay(x, 44100, *ctl)


def test_cpu_tensor_and_float64_are_refused():
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.modulated_delay(torch.zeros(2, 2, 64), 44100, *_controls(2, 1))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.ModulatedDelay(44100).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 5), 0.5))
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.ModulatedDelay(44100, voices=3).process_normalized(torch.zeros(2, 1, 64), torch.full((2, 13), 0.5))
    meta = torch.zeros(2, 2, 64, dtype=torch.float64, device="meta")             # is_cuda is False: the device check comes first
    with pytest.raises(_lib.DaspHipError):
        D.modulated_delay(meta, 44100, *_controls(2, 1))


def test_float64_message(monkeypatch):
    """float64 audio that passed the device check raises DaspHipError naming the op (the device check is stubbed: no GPU here)."""
    monkeypatch.setattr(_lib, "require_device", lambda t, name="x": None)
    with pytest.raises(_lib.DaspHipError, match="modulated_delay: float64"):
        D.modulated_delay(torch.zeros(2, 2, 64, dtype=torch.float64), 44100, *_controls(2, 1))


def test_bad_scalars_raise_value_error():
    x = torch.zeros(1, 1, 8)
    for kw in (dict(max_delay_ms=-1.0), dict(max_delay_ms=float("nan")), dict(max_delay_ms=float("inf")), dict(stereo_spread=float("nan"))):
        with pytest.raises(ValueError, match="modulated_delay"):
            D.modulated_delay(x, 44100, *_controls(1, 1), **kw)
    with pytest.raises(ValueError, match="modulated_delay"):
        D.modulated_delay(x, 0, *_controls(1, 1))


def test_module_tables():
    names = list(inspect.signature(D.functional.modulated_delay).parameters)
    assert names == ["x", "sample_rate", "delay_ms", "depth_ms", "rate_hz", "phase", "mix", "max_delay_ms", "stereo_spread"]
    m = D.ModulatedDelay(44100)
    assert m.num_params == 5 and list(m.param_ranges) == names[2:7]
    assert m.param_ranges == {"delay_ms": (0.0, 30.0), "depth_ms": (0.0, 5.0), "rate_hz": (0.05, 10.0), "phase": (0.0, 1.0), "mix": (0.0, 1.0)}
    assert m.max_delay_ms == 35.0 and m.sample_rate == 44100 and m.voices == 1
    for V in (2, 3, 8):
        m = D.ModulatedDelay(48000, voices=V, max_delay_ms=20.0, max_depth_ms=2.0)
        assert m.num_params == 4 * V + 1 and m.max_delay_ms == 22.0
        want = [f"voice{v}_{n}" for v in range(V) for n in names[2:6]] + ["mix"]
        assert list(m.param_ranges) == want
        assert m.param_ranges["voice1_delay_ms"] == (0.0, 20.0) and m.param_ranges[f"voice{V - 1}_rate_hz"] == (0.05, 10.0)
    with pytest.raises(ValueError, match="voices"):
        D.ModulatedDelay(44100, voices=0)
    assert D.modulated_delay is D.functional.modulated_delay and D.ModulatedDelay is D.modules.ModulatedDelay
