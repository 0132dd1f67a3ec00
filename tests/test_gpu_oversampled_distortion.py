"""GPU tests of oversampled_distortion (csrc/oversample.hip): parity of y, grad x and grad drive_db with the float64 restatement
(tests/oversampled_distortion_restated.py), the alias rejection it exists for, the interpolation property of the low-pass, and what the
fused form promises - bit-identical results run to run, alone or inside a batch, eager or replayed from a graph.

Parity bounds. The yardstick is the restatement itself run in float32 on the same inputs on the CPU: e32 = its error against float64,
relative to the peak of the float64 result. The kernel sums in another order, so it gets 4 x e32, and never less than the floors that
tests/test_gpu_elementwise.py uses for `distortion`: 2e-6 of the peak for y and grad x, 1e-5 for grad drive_db.
"""
import functools

import numpy as np
import pytest
import torch

from tests import oversampled_distortion_restated as R
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 44100


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def tile(L):
    from dasp_pytorch_amd import _lib
    return _lib.lib().dasp_osdist_tile(L)


def draw(B, C, N, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * C + N)
    x = torch.rand(B, C, N, generator=g) * 2 - 1
    drive = torch.rand(B * C, generator=g) * 30 - 6
    w = torch.randn(B, C, N, generator=g)
    return x, drive, w


def run_t(D, x, drive, w, L, H=12, **kw):
    xt = x.to(DEV).requires_grad_(True)
    dt = drive.to(DEV).requires_grad_(True)
    y = D.oversampled_distortion(xt, SR, dt, oversample=L, half_width=H, **kw)
    (y * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return dict(y=y.detach(), gx=xt.grad, gdrive=dt.grad)


def peak_err(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
def shapes(L, H=12):
    T = tile(L)
    return [(1, 1, 1), (2, 2, 5), (2, 3, T - 1), (2, 2, T), (1, 2, T + 1), (1, 1, 2 * T + 2 * H + 1), (3, 1, 10001), (64, 2, 8192)]


@functools.lru_cache(maxsize=4)
def reference(B, C, N, L, H):
    """Inputs, the float64 restatement and the error of its float32 run, once per case."""
    x, drive, w = draw(B, C, N)
    want = dict(zip(("y", "gx", "gdrive"), (t.numpy() for t in R.forward_backward(x, drive, w, L, H))))
    f32 = dict(zip(("y", "gx", "gdrive"), (t.numpy() for t in R.forward_backward(x, drive, w, L, H, dtype=torch.float32))))
    return (x, drive, w), want, {k: peak_err(f32[k], want[k]) for k in want}


def check_parity(D, name, B, C, N, L, H):
    (x, drive, w), want, e32 = reference(B, C, N, L, H)
    got = {k: v.cpu().numpy() for k, v in run_t(D, x, drive, w, L, H).items()}
    assert got["y"].shape == got["gx"].shape == (B, C, N) and got["gdrive"].shape == (B * C,)
    e = {k: peak_err(got[k], want[k]) for k in want}
    record(name, **e, **{"fp32_" + k: v for k, v in e32.items()})
    for k, floor in (("y", 2e-6), ("gx", 2e-6), ("gdrive", 1e-5)):
        assert e[k] <= max(4 * e32[k], floor), (name, k, e[k], e32[k])


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("L", [2, 4, 8])
def test_parity_with_the_float64_restatement(D, L, case):
    B, C, N = shapes(L)[case]
    check_parity(D, f"osdist_parity L={L} ({B},{C},{N})", B, C, N, L, 12)


@pytest.mark.parametrize("L,H", [(4, 1), (8, 16), (2, 16)])
def test_parity_at_other_half_widths(D, L, H):
    B, C, N = 2, 2, tile(L) + 2 * H + 3
    check_parity(D, f"osdist_parity L={L} H={H} ({B},{C},{N})", B, C, N, L, H)


# ---- 2. aliasing ---------------------------------------------------------------------------------------------------------------------------
TONE_N, TONE_BIN = 32768, 3603


def tone():
    return (0.5 * torch.sin(2 * np.pi * TONE_BIN * torch.arange(TONE_N, dtype=torch.float64) / TONE_N)).float().view(1, 1, -1)


@pytest.mark.parametrize("L", [4, 8])
def test_alias_rejection(D, L):
    """A 0.5-amplitude sine on bin 3603 of 32768 driven by 24 dB: the energy off the harmonics is what folded back. The kernel is within
    1 dB of the restatement's figure (-62.5 dB at 4x, -78.5 dB at 8x); tanh at the base rate leaves it above -20 dB (-13.7 dB)."""
    x, drive = tone(), torch.tensor([24.0])
    with torch.no_grad():
        y = D.oversampled_distortion(x.to(DEV), SR, drive.to(DEV), oversample=L).cpu().numpy().reshape(-1)
        base = D.distortion(x.to(DEV), SR, drive.to(DEV)).cpu().numpy().reshape(-1)
    got, want = R.inharmonic_share_db(y, TONE_BIN), R.inharmonic_share_db(R.forward(x, drive, L).numpy().reshape(-1), TONE_BIN)
    base_db = R.inharmonic_share_db(base, TONE_BIN)
    record(f"osdist_alias L={L}", kernel_db=got, restated_db=want, base_rate_db=base_db)
    assert abs(got - want) <= 1.0, (got, want)
    assert want < -60.0 if L == 4 else want < -75.0
    assert base_db > -20.0


# ---- 3. the low-pass interpolates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4, 8])
def test_small_signal_passes_unchanged(D, L):
    """At -80 dB of drive tanh is linear to 1e-8 and with cutoff = 1 the interpolator passes the base samples through: 10^4 y gives x back
    within 1e-4 of the peak, away from the ends where the zeros outside the signal are felt."""
    n = 8192
    x = torch.sin(2 * np.pi * 1000.0 * torch.arange(n, dtype=torch.float64) / SR).float().view(1, 1, -1)
    with torch.no_grad():
        y = D.oversampled_distortion(x.to(DEV), SR, torch.tensor([-80.0], device=DEV), oversample=L, cutoff=1.0).cpu()
    e = float((y * 1e4 - x)[..., 64:-64].abs().max() / x.abs().max())
    record(f"osdist_interpolation L={L}", err=e)
    assert e <= 1e-4


# ---- 4. identity and determinism -----------------------------------------------------------------------------------------------------------
def test_oversample_1_is_distortion(D):
    x, drive, w = draw(3, 2, 5000)
    xt, dt = x.to(DEV).requires_grad_(True), drive.to(DEV).requires_grad_(True)
    y = D.oversampled_distortion(xt, SR, dt, oversample=1)
    gx, gd = torch.autograd.grad((y * w.to(DEV)).sum(), (xt, dt))
    y0 = D.distortion(xt, SR, dt)
    gx0, gd0 = torch.autograd.grad((y0 * w.to(DEV)).sum(), (xt, dt))
    assert torch.equal(y, y0) and torch.equal(gx, gx0) and torch.equal(gd, gd0)


@pytest.mark.parametrize("L", [2, 4, 8])
def test_runs_are_bit_identical(D, L):
    d = draw(3, 2, 3 * tile(L) + 77)
    a, b = run_t(D, *d, L), run_t(D, *d, L)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_row_alone_and_inside_a_batch(D):
    L, item = 4, 5
    x, drive, w = draw(4, 3, 2 * tile(L) + 13)
    whole = run_t(D, x, drive, w, L)
    b, c = divmod(item, 3)
    alone = run_t(D, x[b:b + 1, c:c + 1], drive[item:item + 1], w[b:b + 1, c:c + 1], L)
    assert torch.equal(whole["y"][b, c], alone["y"][0, 0]) and torch.equal(whole["gx"][b, c], alone["gx"][0, 0])
    assert torch.equal(whole["gdrive"][item], alone["gdrive"][0])


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path, nothing to zero, fixed
    summation orders - every replay equals the eager step bit for bit."""
    L = 4
    x, drive, w = draw(3, 2, 2 * tile(L) + 500)
    eager = run_t(D, x, drive, w, L)
    xt, dt, wt = x.to(DEV).requires_grad_(True), drive.to(DEV).requires_grad_(True), w.to(DEV)

    def step():
        y = D.oversampled_distortion(xt, SR, dt, oversample=L)
        return (y,) + torch.autograd.grad((y * wt).sum(), (xt, dt))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in range(3):
        for o in outs:
            o.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, o in zip(("y", "gx", "gdrive"), outs):
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 5. interface ----------------------------------------------------------------------------------------------------------------------------
def test_wrong_drive_count_raises_as_distortion_does(D):
    x = torch.zeros(2, 2, 64, device=DEV)
    for n in (3, 8):
        with pytest.raises(RuntimeError) as want:
            D.distortion(x, SR, torch.zeros(n, device=DEV))
        with pytest.raises(RuntimeError) as got:
            D.oversampled_distortion(x, SR, torch.zeros(n, device=DEV))
        assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    from dasp_pytorch_amd import _lib
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.oversampled_distortion(x.double(), SR, torch.zeros(4, device=DEV))


@pytest.mark.parametrize("L", [4, 8])
def test_module_equals_functional(D, L):
    x, _, _ = draw(3, 1, 3000)
    p = torch.tensor([[0.0], [0.37], [1.0]], device=DEV)
    m = D.OversampledDistortion(-6.0, 18.0, SR, oversample=L)
    with torch.no_grad():
        got = m.process_normalized(x.to(DEV), p)
        want = D.oversampled_distortion(x.to(DEV), SR, p[:, 0] * 24.0 - 6.0, oversample=L)
    assert torch.equal(got, want)


def test_non_contiguous_input(D):
    x, drive, w = draw(3, 2, 2500)
    xt = x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)         # (3, 2, 2500) with the strides of (2, 3, 2500)
    assert not xt.is_contiguous() and torch.equal(xt, x.to(DEV))
    xt.requires_grad_(True)
    dt = drive.to(DEV).requires_grad_(True)
    y = D.oversampled_distortion(xt, SR, dt)
    gx, gd = torch.autograd.grad((y * w.to(DEV)).sum(), (xt, dt))
    want = run_t(D, x, drive, w, 4)
    assert torch.equal(y, want["y"]) and torch.equal(gx, want["gx"]) and torch.equal(gd, want["gdrive"])


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        d = torch.zeros(B * C, device=DEV, requires_grad=True)
        y = D.oversampled_distortion(x, SR, d)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and d.grad.shape == d.shape and not d.grad.any()
