"""signal.freqdomain_fir (csrc/fdfir.hip through torch.ops.dasp.freqdomain_fir) on the device: against the reference's own float64
outputs (tests/golden/fdfir_*.npz, made by tests/golden/make_golden_freqdomain_fir.py), against torch.fft in float64 on the CPU, and
against itself. Bound of every comparison with float64: the project's own for its FFT paths, L-inf / peak < 2e-5 (the reference's own
float32 run stays within 4.5e-7 of float64 on these shapes, so the bound hides nothing)."""
import math

import numpy as np
import pytest
import torch

import dasp_pytorch_amd as D
from tests.util import linf_peak, load_golden, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
TOL_PAR = 1e-4

GOLDENS = ["fdfir_b2c2_t700_n512", "fdfir_b2c3_t3000_n4096", "fdfir_b2c2_t6000_n16384"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ri(z):
    """complex (..., bins) -> real (..., bins, 2) as numpy: complex values are compared as re / im"""
    z = z.detach().cpu() if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z))
    if z.dim() == 1:
        z = z[None]
    return torch.view_as_real(z.resolve_conj()).numpy() if z.is_complex() else z.numpy()


def torch_fft_reference(x, H, n, w):
    """float64 on the CPU: y, gx, gH of (y * w).sum() for y = irfft(rfft(x, n) * H, n)"""
    x64 = x.detach().cpu().double().requires_grad_(True)
    H64 = H.detach().cpu()
    H64 = (H64.to(torch.complex128) if H64.is_complex() else H64.double()).requires_grad_(True)
    y = torch.fft.irfft(torch.fft.rfft(x64, n) * H64, n)
    (y * w.detach().cpu().double()).sum().backward()
    return y.detach(), x64.grad, H64.grad


def run(x, H, n, w):
    x = x.detach().clone().requires_grad_(True)
    H = H.detach().clone().requires_grad_(True)
    y = D.signal.freqdomain_fir(x, H, n)
    (y * w).sum().backward()
    return y.detach(), x.grad, H.grad


def errors(got, want):
    """L-inf / peak per batch item (tests/util.py linf_peak: the items are the first dimension) of y, gx and gH, the worst item of each"""
    out = []
    for g, w in zip(got, want):
        g, w = ri(g).astype(np.float64), ri(w).astype(np.float64)
        assert g.shape == w.shape, (g.shape, w.shape)
        out.append(float(linf_peak(g, w).max()))
    return out


# ---- 1. the reference's own outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_golden(name):
    g = load_golden(name)
    n = int(g["n_fft"])
    H = torch.complex(dev(g["H_re"]), dev(g["H_im"]))
    y, gx, gH = run(dev(g["x"]), H, n, dev(g["w"]))
    assert y.shape == g["y64"].shape and y.shape[-1] == n and y.dtype == torch.float32
    assert gH.dtype == torch.complex64 and gH.shape == H.shape
    ey, egx, egH = errors((y, gx, gH), (g["y64"], g["gx64"], np.stack([g["gH64_re"], g["gH64_im"]], -1)))
    record(f"freqdomain_fir golden {name}", y=ey, gx=egx, gH=egH)
    assert ey < TOL and egx < TOL and egH < TOL
    if g["x"].shape[-1] > n:                                  # samples cropped by the transform: gradient exactly 0
        assert torch.all(gx[..., n:] == 0)


# ---- 2. sweep against torch.fft in float64 --------------------------------------------------------------------------------------------
def _patterns():
    """(x leading shape, H leading shape, real H): rows 1, 3 and 4; H per row, shared per item, real-valued"""
    return [((1,), (1,), False), ((1, 3), (1, 1), False), ((2, 2), (2, 2), False), ((2, 2), (2, 1), True), ((3,), (3,), True)]


def _sweep_cases(n):
    if n == 1 << 19:
        return [((1, 2), (1, 1), False, n - 3), ((1, 2), (1, 1), True, n + 5)]
    if n == 1 << 20:
        return [((1,), (1,), False, n - 3), ((1,), (1,), True, 1)]
    Ts = [1, n - 3, n, n + 5]
    pats = _patterns()
    if n >= 131072:                                            # every T and every pattern once, not the full cross
        return [(*pats[i % len(pats)], T) for i, T in enumerate(Ts)] + [(*pats[4], n - 3)]
    return [(*p, T) for p in pats for T in Ts]


@pytest.mark.parametrize("n", [8, 64, 512, 4096, 8192, 16384, 131072, 1 << 19, 1 << 20])
def test_sweep_against_torch_fft(n):
    gen = torch.Generator().manual_seed(n)
    bins = n // 2 + 1
    worst = [0.0, 0.0, 0.0]
    for xl, hl, real, T in _sweep_cases(n):
        x = torch.randn(*xl, T, generator=gen)
        H = torch.randn(*hl, bins, generator=gen) if real else torch.view_as_complex(torch.randn(*hl, bins, 2, generator=gen))
        w = torch.randn(*xl, n, generator=gen)
        want = torch_fft_reference(x, H, n, w)
        got = run(x.to(DEV), H.to(DEV), n, w.to(DEV))
        assert got[0].shape == (*xl, n) and got[1].shape == x.shape and got[2].shape == H.shape
        assert got[2].dtype == (torch.float32 if real else torch.complex64)          # a real response gets a real gradient
        e = errors(got, want)
        assert max(e) < TOL, (n, xl, hl, real, T, e)
        if T > n:
            assert torch.all(got[1][..., n:] == 0)
        worst = [max(a, b) for a, b in zip(worst, e)]
    record(f"freqdomain_fir sweep n_fft={n}", y=worst[0], gx=worst[1], gH=worst[2])


# ---- 3. DC / Nyquist ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 16384])
def test_dc_and_nyquist_imaginary_parts(n):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 2, n - 7, generator=gen).to(DEV)
    H = torch.view_as_complex(torch.randn(2, 1, n // 2 + 1, 2, generator=gen)).to(DEV)
    w = torch.randn(2, 2, n, generator=gen).to(DEV)
    Hbig = H.clone()
    Hbig[..., 0] = Hbig[..., 0].real + 1e3j
    Hbig[..., -1] = Hbig[..., -1].real - 7e2j
    Hzero = H.clone()
    Hzero[..., 0] = Hzero[..., 0].real + 0j
    Hzero[..., -1] = Hzero[..., -1].real + 0j
    y1, gx1, gH1 = run(x, Hbig, n, w)
    y0, gx0, gH0 = run(x, Hzero, n, w)
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0) and torch.equal(gH1, gH0)
    assert torch.all(gH1.imag[..., 0] == 0) and torch.all(gH1.imag[..., -1] == 0)
    assert torch.all(gH1.real[..., 0] != 0)


# ---- 4. the reference's frequency-sampled sosfilt, composed ---------------------------------------------------------------------------
def test_reference_fsm_composed():
    """signal.py:136-166 of the reference: H = fft_sosfreqz(sos, n_fft), y = freqdomain_fir(x, H.unsqueeze(1), n_fft)[..., :T] with
    n_fft = 2^ceil(log2(2 T - 1)) = 16384 for T = 6000, against the golden the exact recurrence is tested with."""
    g = load_golden("sos_b2c2_n6000_s3")
    x = dev(g["x"]).requires_grad_(True)
    sos = dev(g["sos"]).requires_grad_(True)
    T = x.shape[-1]
    n = 2 ** math.ceil(math.log2(2 * T - 1))
    assert n == 16384
    y = D.signal.freqdomain_fir(x, D.signal.fft_sosfreqz(sos, n).unsqueeze(1), n)[..., :T]
    (y * dev(g["w"])).sum().backward()
    ey = linf_peak(y.detach().cpu().numpy(), g["y64"]).max()
    egx = linf_peak(x.grad.cpu().numpy(), g["gx64"]).max()
    egs = linf_peak(sos.grad.cpu().numpy(), g["gsos64"]).max()
    record("freqdomain_fir composed FSM sos_b2c2_n6000_s3", y=ey, gx=egx, gsos=egs)
    assert ey < TOL and egx < TOL
    assert egs < TOL_PAR


# ---- 5. algebra -------------------------------------------------------------------------------------------------------------------------
def _inputs(n, T, seed, xl=(2, 2), hl=(2, 1)):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*xl, T, generator=gen).to(DEV)
    H = torch.view_as_complex(torch.randn(*hl, n // 2 + 1, 2, generator=gen)).to(DEV)
    return x, H


@pytest.mark.parametrize("n", [512, 16384])
def test_linearity(n):
    x1, H1 = _inputs(n, n - 3, 1)
    x2, H2 = _inputs(n, n - 3, 2)
    f = D.signal.freqdomain_fir
    a, b = 0.75, -1.5
    ex = linf_peak(f(a * x1 + b * x2, H1, n).cpu().numpy(), (a * f(x1, H1, n) + b * f(x2, H1, n)).cpu().numpy()).max()
    eh = linf_peak(f(x1, a * H1 + b * H2, n).cpu().numpy(), (a * f(x1, H1, n) + b * f(x1, H2, n)).cpu().numpy()).max()
    record(f"freqdomain_fir linearity n_fft={n}", in_x=ex, in_H=eh)
    assert ex < TOL and eh < TOL


@pytest.mark.parametrize("n", [512, 16384])
def test_unit_response_returns_the_padded_input(n):
    x, _ = _inputs(n, n - 3, 3)
    y = D.signal.freqdomain_fir(x, torch.ones(2, 1, n // 2 + 1, dtype=torch.complex64, device=DEV), n)
    want = torch.nn.functional.pad(x, (0, 3))
    e = linf_peak(y.cpu().numpy(), want.cpu().numpy()).max()
    record(f"freqdomain_fir H=1 n_fft={n}", y=e)
    assert e < 1e-6


@pytest.mark.parametrize("n,d", [(64, 5), (4096, 1000), (16384, 9000)])
def test_linear_phase_is_a_circular_delay(n, d):
    x, _ = _inputs(n, n, 4)
    k = torch.arange(n // 2 + 1, dtype=torch.float64)
    H = torch.polar(torch.ones_like(k), -2 * math.pi * k * d / n).to(torch.complex64).to(DEV)
    y = D.signal.freqdomain_fir(x, H, n)                       # H (bins,): shared by every row
    e = linf_peak(y.cpu().numpy(), torch.roll(x, d, -1).cpu().numpy()).max()
    record(f"freqdomain_fir delay n_fft={n}", y=e)
    assert e < TOL


@pytest.mark.parametrize("n", [512, 16384])
def test_rows_are_independent(n):
    x, H = _inputs(n, n - 3, 6, xl=(4, 2), hl=(4, 1))
    w = torch.randn(4, 2, n, generator=torch.Generator().manual_seed(7)).to(DEV)
    y, gx, gH = run(x, H, n, w)
    ys, gxs, gHs = run(x[1:2], H[1:2], n, w[1:2])
    assert torch.equal(ys, y[1:2]) and torch.equal(gxs, gx[1:2]) and torch.equal(gHs, gH[1:2])


# ---- 6. determinism and plumbing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 16384])
@pytest.mark.parametrize("chs", [2, 3])
def test_bit_identical_runs(n, chs):
    x, H = _inputs(n, n - 3, 8, xl=(3, chs), hl=(3, 1))
    w = torch.randn(3, chs, n, generator=torch.Generator().manual_seed(9)).to(DEV)
    a, b = run(x, H, n, w), run(x, H, n, w)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # and the shared response's gradient is the sum over the item's channels of the per-row gradients
    per_row = run(x, H.expand(3, chs, -1).contiguous(), n, w)[2].sum(1, keepdim=True)
    assert linf_peak(ri(a[2]), ri(per_row)).max() < TOL


def test_only_the_requested_gradients():
    n = 512
    x, H = _inputs(n, 400, 10)
    w = torch.randn(2, 2, n, generator=torch.Generator().manual_seed(11)).to(DEV)
    _, gx, gH = run(x, H, n, w)
    x0, H0 = x.clone(), H.clone()
    xr = x.clone().requires_grad_(True)
    (D.signal.freqdomain_fir(xr, H, n) * w).sum().backward()
    assert torch.equal(xr.grad, gx)
    Hr = H.clone().requires_grad_(True)
    (D.signal.freqdomain_fir(x, Hr, n) * w).sum().backward()
    assert torch.equal(Hr.grad, gH)
    assert not D.signal.freqdomain_fir(x, H, n).requires_grad
    assert torch.equal(x, x0) and torch.equal(H, H0)          # inputs are not written to
    from dasp_pytorch_amd import _torch_ops
    assert _torch_ops.load()
    g0, g1 = torch.ops.dasp._freqdomain_fir_backward(x.reshape(4, -1), H.reshape(2, -1), w.reshape(4, -1), n, True, False)
    assert g1.numel() == 0 and torch.equal(g0.reshape(x.shape), gx)
    g0, g1 = torch.ops.dasp._freqdomain_fir_backward(x.reshape(4, -1), H.reshape(2, -1), w.reshape(4, -1), n, False, True)
    assert g0.numel() == 0 and torch.equal(g1.reshape(H.shape), gH)


@pytest.mark.parametrize("n", [512, 16384])
def test_non_default_stream(n):
    x, H = _inputs(n, n - 3, 12)
    w = torch.randn(2, 2, n, generator=torch.Generator().manual_seed(13)).to(DEV)
    want = run(x, H, n, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = run(x, H, n, w)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for u, v in zip(got, want):
        assert torch.equal(u, v)


@pytest.mark.parametrize("rows,h_rows,T,n", [(4, 2, 50, 64), (3, 3, 70, 64), (2, 1, 20000, 16384)])
def test_opcheck(rows, h_rows, T, n):
    from dasp_pytorch_amd import _torch_ops
    assert _torch_ops.load()
    gen = torch.Generator().manual_seed(14)
    x = torch.randn(rows, T, generator=gen).to(DEV).requires_grad_(True)
    H = torch.view_as_complex(torch.randn(h_rows, n // 2 + 1, 2, generator=gen)).to(DEV).requires_grad_(True)
    torch.library.opcheck(torch.ops.dasp.freqdomain_fir.default, (x, H, n))
    torch.library.opcheck(torch.ops.dasp.freqdomain_fir.default, (x.detach(), H.detach(), n))


def _loss(x, H):
    return D.signal.freqdomain_fir(x, H, 512)[..., :400].square().mean()


def test_compile_fullgraph():
    x, H = _inputs(512, 400, 15)
    x0, H0 = x.clone().requires_grad_(True), H.clone().requires_grad_(True)
    l0 = _loss(x0, H0)
    l0.backward()
    x1, H1 = x.clone().requires_grad_(True), H.clone().requires_grad_(True)
    l1 = torch.compile(_loss, fullgraph=True)(x1, H1)
    l1.backward()
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0)
    torch.testing.assert_close(x1.grad, x0.grad, rtol=1e-5, atol=1e-6 * x0.grad.abs().max().item())
    torch.testing.assert_close(H1.grad, H0.grad, rtol=1e-5, atol=1e-6 * H0.grad.abs().max().item())


def test_cuda_graph_replay():
    n = 16384
    x, H = _inputs(n, 6000, 16)
    w = torch.randn(2, 2, n, generator=torch.Generator().manual_seed(17)).to(DEV)
    x.requires_grad_(True)
    H.requires_grad_(True)

    def step():
        x.grad = None
        H.grad = None
        y = D.signal.freqdomain_fir(x, H, n)
        (y * w).sum().backward()
        return y

    y0 = step().detach().clone()
    gx0, gH0 = x.grad.clone(), H.grad.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    H.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y0) and torch.equal(x.grad, gx0) and torch.equal(H.grad, gH0)
