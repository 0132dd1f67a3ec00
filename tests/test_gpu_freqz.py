"""signal.fft_freqz / fft_sosfreqz (csrc/freqz.hip through torch.ops.dasp.freqz) and ParametricEQ.frequency_response on the device,
against the reference's own outputs (tests/golden/freqz_*.npz, made by tests/golden/make_golden_freqz.py) and against themselves."""
import glob
import os

import numpy as np
import pytest
import scipy.signal
import torch

import dasp_pytorch_amd as D
from dasp_pytorch_amd import _lib
from tests.freqz_exact import exact_for_golden, exact_response, fp64_bound
from tests.util import GOLDEN, load_golden, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 44100

SOS_FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "freqz_sos_*.npz")))
BA_FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "freqz_ba_*.npz")))


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x if dtype is None else x.to(dtype)


def run_golden(name, dtype):
    """-> (H, grads, golden) for one golden file at one precision; the loss is sum(Re(conj(W) H)) as in the golden's gradients."""
    g = load_golden(name)
    n = int(g["n_fft"])
    if "sos" in g:
        coefs = [t(g["sos"], dtype).requires_grad_(True)]
        H = D.signal.fft_sosfreqz(coefs[0], n) if n != 512 else D.signal.fft_sosfreqz(coefs[0])
        want = [g["gsos64"]]
    else:
        coefs = [t(g["b"], dtype).requires_grad_(True), t(g["a"], dtype).requires_grad_(True)]
        H = D.signal.fft_freqz(coefs[0], coefs[1], n)
        want = [g["gb64"], g["ga64"]]
    (torch.conj(t(g["W"]).to(H.dtype)) * H).real.sum().backward()
    return H.detach().cpu().numpy(), [c.grad.cpu().numpy() for c in coefs], want, g


@pytest.mark.parametrize("name", SOS_FILES + BA_FILES)
def test_values_float32(name):
    H, _, _, g = run_golden(name, torch.float32)
    assert H.dtype == np.complex64 and H.shape == g["H64"].shape
    H64, H32r = g["H64"], g["H32"]
    rows64, rows = H64.reshape(-1, H64.shape[-1]), H.reshape(-1, H.shape[-1]).astype(np.complex128)
    err = np.abs(rows - rows64)
    floor = 1e-7 * np.abs(rows64).max(1, keepdims=True)
    assert np.all(err <= 1e-6 * np.abs(rows64) + floor), (err / (np.abs(rows64) + floor / 1e-6)).max()
    # at least as accurate as the reference's own float32 FFTs, bin by bin
    ref_err = np.abs(H32r.reshape(rows.shape).astype(np.complex128) - rows64)
    assert np.all(err <= 4 * ref_err + 1e-6 * np.abs(rows64)), name
    record(f"freqz values f32 {name}", rel=(err / np.maximum(np.abs(rows64), floor)).max(), ref_rel=(ref_err / np.maximum(np.abs(rows64), floor)).max())


def _rows(x):
    x = np.asarray(x)
    return x.reshape(-1, x.shape[-1])


def _peak_rel(a, b):
    """per row: max |a - b| / max |b|"""
    a, b = _rows(a), _rows(b)
    return np.abs(a - b).max(1) / np.abs(b).max(1)


def _norm_rel(a, b):
    """per row: ||a - b|| / ||b||"""
    a, b = _rows(a).astype(np.float64), _rows(b)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


@pytest.mark.parametrize("name", SOS_FILES + BA_FILES)
def test_values_float64(name):
    """Within 1e-12 of the extended-precision evaluation (tests/freqz_exact.py), and of the reference's float64 response up to that
    response's own error (its FFTs lose up to ~5e-11 next to a pole close to the unit circle; measured against the same yardstick)."""
    H, _, _, g = run_golden(name, torch.float64)
    assert H.dtype == np.complex128
    Hx, _ = exact_for_golden(g)
    e_exact, e_ref, ref_own = _peak_rel(H, Hx), _peak_rel(H, g["H64"]), _peak_rel(g["H64"], Hx)
    # next to a pole on the unit circle no float64 evaluation gets within 1e-12: there the a-priori bound of tests/freqz_exact.py is the floor
    bound = _rows(fp64_bound(g))
    err = np.abs(_rows(H) - _rows(Hx))
    record(f"freqz values f64 {name}", vs_exact=e_exact, vs_ref=e_ref, ref_own=ref_own, err_over_bound=(err / (1e-12 * np.abs(_rows(Hx)) + bound)).max())
    assert np.all(err <= 1e-12 * np.abs(_rows(Hx)).max(1, keepdims=True) + bound)
    assert np.all(e_ref <= e_exact + ref_own + 1e-15)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float64, 1e-11)])
@pytest.mark.parametrize("name", SOS_FILES + BA_FILES)
def test_gradients_against_reference(name, dtype, tol):
    """Per row, normwise: within tol of the reference's float64 gradients plus their own error (against the extended-precision
    gradients of tests/freqz_exact.py), and within tol of the extended-precision gradients themselves."""
    _, got, want, g = run_golden(name, dtype)
    Hx, exact = exact_for_golden(g)
    # the conditioning floor of float64 (tests/freqz_exact.py fp64_bound), normwise per item, twice: the adjoint divides by A_s once more
    rho = 2 * np.linalg.norm(_rows(fp64_bound(g)), axis=1) / np.linalg.norm(_rows(Hx), axis=1)
    for gg, ww, xx in zip(got, want, exact):
        assert gg.shape == ww.shape == xx.shape
        e_ref, e_exact, ref_own = _norm_rel(gg, ww), _norm_rel(gg, xx), _norm_rel(ww, xx)
        floor = tol + (rho if len(rho) == len(e_exact) else rho.max())
        record(f"freqz grads {dtype} {name}", vs_ref=e_ref, vs_exact=e_exact, ref_own=ref_own, floor=floor)
        assert np.all(e_exact <= floor), (name, e_exact.max())
        assert np.all(e_ref <= floor + ref_own), (name, e_ref.max())


def _stable_sos(gen, bs, S, dtype=torch.float64):
    r = 0.3 + 0.6 * torch.rand(bs, S, generator=gen, dtype=dtype)
    th = 3.0 * torch.rand(bs, S, generator=gen, dtype=dtype)
    a0 = 0.5 + torch.rand(bs, S, generator=gen, dtype=dtype)
    a = torch.stack([torch.ones_like(r), -2 * r * torch.cos(th), r * r], -1) * a0[..., None]
    b = torch.randn(bs, S, 3, generator=gen, dtype=dtype)
    return torch.cat([b, a], -1)


def test_gradcheck_float64():
    gen = torch.Generator().manual_seed(3)
    sos = _stable_sos(gen, 2, 3).to(DEV)
    # section 1 a low pass (an exact zero of B at Nyquist: a bin at even n_fft), section 2 a high pass (zero at DC)
    b_lp, a_lp = D.signal.biquad(torch.tensor([0.0, 0.0], device=DEV, dtype=torch.float64), torch.tensor([3000.0, 9000.0], device=DEV, dtype=torch.float64),
                                 torch.tensor([0.7, 2.0], device=DEV, dtype=torch.float64), SR, "low_pass")
    b_hp, a_hp = D.signal.biquad(torch.tensor([0.0, 0.0], device=DEV, dtype=torch.float64), torch.tensor([50.0, 300.0], device=DEV, dtype=torch.float64),
                                 torch.tensor([0.7, 1.0], device=DEV, dtype=torch.float64), SR, "high_pass")
    one = torch.tensor([1.0, 2.0, 1.0], device=DEV, dtype=torch.float64)
    sos[:, 1] = torch.cat([b_lp[:, :1] * one, a_lp], -1).detach()                 # b0 [1, 2, 1]: B(-1) = 0 exactly
    sos[:, 2] = torch.cat([b_hp[:, :1] * one * one.new_tensor([1, -1, 1]), a_hp], -1).detach()   # b0 [1, -2, 1]: B(1) = 0 exactly
    for n in (16, 15):
        H = D.signal.fft_sosfreqz(sos, n)
        if n % 2 == 0:
            assert torch.all(H[:, -1] == 0) and torch.all(H[:, 0] == 0)
        assert torch.autograd.gradcheck(lambda s: D.signal.fft_sosfreqz(s, n), (sos.clone().requires_grad_(True),))
    b = torch.randn(3, 4, dtype=torch.float64, device=DEV, requires_grad=True)
    a = (_stable_sos(gen, 3, 1)[:, 0, 3:].to(DEV)).requires_grad_(True)
    for n in (9, 10, 2):
        assert torch.autograd.gradcheck(lambda b_, a_: D.signal.fft_freqz(b_, a_, n), (b, a))


def test_gradients_bit_identical():
    g = load_golden("freqz_sos_eq_n999")
    out = []
    for _ in range(2):
        s = t(g["sos"]).requires_grad_(True)
        H = D.signal.fft_sosfreqz(s, 4096)
        (torch.conj(torch.ones_like(H)) * H * 1.5).real.sum().backward()
        out.append(s.grad.clone())
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_opcheck(dtype):
    from dasp_pytorch_amd import _torch_ops
    assert _torch_ops.load()
    gen = torch.Generator().manual_seed(1)
    sos = _stable_sos(gen, 3, 2).to(DEV, dtype)
    b, a = sos[..., :3].contiguous().requires_grad_(True), sos[..., 3:].contiguous().requires_grad_(True)
    torch.library.opcheck(torch.ops.dasp.freqz.default, (b, a, 64))
    torch.library.opcheck(torch.ops.dasp.freqz.default, (b.detach(), a.detach(), 33))


def _db_loss(sos, target):
    H = D.signal.fft_sosfreqz(sos, 2048)
    return (20 * torch.log10(H.abs() + 1e-8) - target).square().mean()


def test_compile_fullgraph_db_loss():
    g = load_golden("freqz_sos_eq_n512")
    target = torch.zeros(1025, device=DEV)
    s0 = t(g["sos"]).requires_grad_(True)
    l0 = _db_loss(s0, target)
    l0.backward()
    s1 = t(g["sos"]).requires_grad_(True)
    l1 = torch.compile(_db_loss, fullgraph=True)(s1, target)
    l1.backward()
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0)
    torch.testing.assert_close(s1.grad, s0.grad, rtol=1e-5, atol=1e-6 * s0.grad.abs().max().item())


def test_cuda_graph_replay():
    g = load_golden("freqz_sos_eq_n512")
    sos = t(g["sos"]).requires_grad_(True)
    W = t(g["W"])

    def step():
        sos.grad = None
        H = D.signal.fft_sosfreqz(sos, 500)
        (torch.conj(W[:, :251]) * H).real.sum().backward()
        return H.detach().clone(), sos.grad.clone()

    H0, g0 = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    sos.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        H = D.signal.fft_sosfreqz(sos, 500)
        (torch.conj(W[:, :251]) * H).real.sum().backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(H, H0) and torch.equal(sos.grad, g0)


def _eq_params(seed, bs, dtype):
    gen = torch.Generator().manual_seed(seed)
    return (0.05 + 0.9 * torch.rand(bs, 18, generator=gen, dtype=torch.float64)).to(DEV, dtype)


def _eq_design(eq, p):
    """The six sections of the EQ, designed as the documentation of frequency_response says: de-normalised, then signal.biquad."""
    lo, span = eq._affine(p)
    d = p * span + lo
    secs = []
    for i, kind in enumerate(("low_shelf", "peaking", "peaking", "peaking", "peaking", "high_shelf")):
        b, a = D.signal.biquad(d[:, 3 * i], d[:, 3 * i + 1], d[:, 3 * i + 2], SR, kind)
        secs.append(torch.cat([b, a], -1))
    return torch.stack(secs, 1)


def test_frequency_response_is_sosfreqz_of_the_design():
    eq = D.ParametricEQ(SR)
    p = _eq_params(0, 3, torch.float32)
    H = eq.frequency_response(p, n_fft=4096)
    assert H.shape == (3, 2049) and H.dtype == torch.complex64
    assert torch.equal(H, D.signal.fft_sosfreqz(_eq_design(eq, p), 4096))
    with pytest.raises(ValueError):
        eq.frequency_response(p + 1.0)
    with pytest.raises(ValueError):
        eq.frequency_response(p[:, :17])


def test_frequency_response_gradient_central_differences():
    eq = D.ParametricEQ(SR)
    p = _eq_params(1, 2, torch.float64).requires_grad_(True)
    gen = torch.Generator().manual_seed(2)
    W = torch.randn(2, 257, 2, generator=gen, dtype=torch.float64)
    W = torch.view_as_complex(W).to(DEV)
    f = lambda q: (torch.conj(W) * eq.frequency_response(q, n_fft=512)).real.sum()
    f(p).backward()
    h = 1e-6
    num = torch.zeros_like(p)
    with torch.no_grad():
        for i in range(2):
            for j in range(18):
                e = torch.zeros_like(p)
                e[i, j] = h
                num[i, j] = (f(p + e) - f(p - e)) / (2 * h)
    err = (p.grad - num).norm() / num.norm()
    record("frequency_response grad vs central differences", rel=err.item())
    assert err < 1e-6


def test_frequency_response_against_the_filtered_impulse():
    """rFFT (numpy, host) of a 65,536-sample impulse through process_normalized (the EQ kernels) against frequency_response(65536).
    Per bin the two may differ by the float64 impulse response's tail beyond 65,536 samples (the truncation aliases it into every bin:
    at most sum |h[n >= N]|), plus the float32 filter's own deviation from that response (at most sum |h32 - h64|) and the rounding of
    H to complex64; all three are computed here, none is tuned."""
    N = 65536
    eq = D.ParametricEQ(SR)
    p = _eq_params(4, 3, torch.float32)
    x = torch.zeros(3, 1, N, device=DEV)
    x[:, :, 0] = 1.0
    h32 = eq.process_normalized(x, p)[:, 0].double().cpu().numpy()
    H = eq.frequency_response(p, n_fft=N).cpu().numpy().astype(np.complex128)
    Hy = np.fft.rfft(h32, N, axis=-1)
    # the float64 recursion on the very sections frequency_response evaluates (its float32 design, cast to float64)
    sos64 = _eq_design(eq, p).double().cpu().numpy()
    for r in range(3):
        imp = np.zeros(4 * N)
        imp[0] = 1.0
        h64 = scipy.signal.sosfilt(sos64[r], imp)
        tail = np.abs(h64[N:]).sum()
        dev32 = np.abs(h32[r] - h64[:N]).sum()
        tol = tail + dev32 + 1e-6 * np.abs(H[r])
        err = np.abs(Hy[r] - H[r])
        record("frequency_response vs filtered impulse", max_err=err.max(), tail=tail, dev32=dev32)
        assert np.all(err <= tol), (err - tol).max()


def test_broadcasting_and_shapes():
    gen = torch.Generator().manual_seed(5)
    b = torch.randn(3, 1, 4, generator=gen, dtype=torch.float64).to(DEV)
    a = _stable_sos(gen, 2, 1)[:, 0, 3:].to(DEV)                      # (2, 3)
    H = D.signal.fft_freqz(b, a, 100)
    assert H.shape == (3, 2, 51)
    want = torch.fft.rfft(b.expand(3, 2, 4), 100) / torch.fft.rfft(a.expand(3, 2, 3), 100)
    torch.testing.assert_close(H, want, rtol=1e-12, atol=1e-12)
    H1 = D.signal.fft_freqz(b[0, 0], a[0], torch.tensor(7))            # 1-D inputs, n_fft as a 0-dim tensor, odd
    assert H1.shape == (4,)
    torch.testing.assert_close(H1, torch.fft.rfft(b[0, 0], 7) / torch.fft.rfft(a[0], 7), rtol=1e-12, atol=1e-12)
    Hm = D.signal.fft_freqz(b.float(), a, 16)                          # float32 with float64 promotes to float64
    assert Hm.dtype == torch.complex128
    with pytest.raises(NotImplementedError, match="FFT"):
        D.signal.fft_freqz(torch.randn(2, 33, device=DEV), torch.ones(2, 1, device=DEV), 512)
    D.signal.fft_freqz(torch.randn(2, 33, device=DEV), torch.ones(2, 1, device=DEV), 32)    # cropped to 32 taps: fine
    with pytest.raises(NotImplementedError):
        D.signal.fft_sosfreqz(torch.randn(1, 17, 6, device=DEV), 64)
    with pytest.raises(AssertionError):
        D.signal.fft_sosfreqz(torch.randn(1, 2, 5, device=DEV), 64)
    with pytest.raises(_lib.DaspHipError):
        D.signal.fft_sosfreqz(torch.randn(1, 2, 6), 64)
    with pytest.raises(_lib.DaspHipError):
        D.signal.fft_freqz(torch.randn(2, 3), torch.randn(2, 3), 64)


@pytest.mark.parametrize("bs,n_fft", [(250, 16384), (64, 65536)])
def test_multi_row_multi_tile_plans(bs, n_fft):
    """Shapes where the kernels take their batched plans (csrc/freqz.hip fz_plan / fz_forward): the forward pass evaluates 4 rows per
    workgroup (250 rows: the last group holds 2), the backward pass covers 7 or 8 tiles of 64 bins per workgroup, advancing the twiddle by
    the rotation e^{-2 pi i 64 / n} from tile to tile, and its last workgroup stops at the last bin in the middle of its tiles. Values and
    gradients against the extended-precision evaluation (tests/freqz_exact.py), values also against torch.fft in float64; gradients
    bit-identical over two runs."""
    S, bins = 6, n_fft // 2 + 1
    tiles64 = -(-bins // 64)
    nwg = _lib.lib().dasp_freqz_work_doubles(bs, S, 3, 3, n_fft) // (bs * S * 6)
    assert -(-tiles64 // nwg) > 1 and tiles64 % -(-tiles64 // nwg) != 0     # several tiles per workgroup, the last one ragged
    gen = torch.Generator().manual_seed(bs)
    sos64 = _stable_sos(gen, bs, S)
    W = torch.view_as_complex(torch.randn(bs, bins, 2, generator=gen, dtype=torch.float64))
    Hx, gb, ga = exact_response(sos64[..., :3].numpy(), sos64[..., 3:].numpy(), n_fft, W.numpy())
    gx = np.concatenate([gb, ga], -1)
    Wd = W.to(DEV)
    grads = []
    for _ in range(2):
        s = sos64.to(DEV).requires_grad_(True)
        H = D.signal.fft_sosfreqz(s, n_fft)
        (torch.conj(Wd) * H).real.sum().backward()
        grads.append(s.grad)
    assert torch.equal(grads[0], grads[1])
    Hd = H.detach()
    e_exact = _peak_rel(Hd.cpu().numpy(), Hx)
    Hf = torch.fft.rfft(s.detach()[..., :3], n_fft) / torch.fft.rfft(s.detach()[..., 3:], n_fft)
    e_fft = _peak_rel(Hd.cpu().numpy(), Hf.prod(1).cpu().numpy())
    e_grad = _norm_rel(grads[0].reshape(bs, -1).cpu().numpy(), gx.reshape(bs, -1))
    record(f"freqz batched plans ({bs}, 6, {n_fft})", vs_exact=e_exact.max(), vs_torch_fft=e_fft.max(), grad_vs_exact=e_grad.max())
    assert np.all(e_exact <= 1e-12) and np.all(e_fft <= 1e-11) and np.all(e_grad <= 1e-11)
    # float32 in, same plans: per bin within the float32 rounding of the exact response
    s32 = sos64.float().to(DEV).requires_grad_(True)
    H32 = D.signal.fft_sosfreqz(s32, n_fft)
    (torch.conj(Wd.to(torch.complex64)) * H32).real.sum().backward()
    c32 = s32.detach().double().cpu().numpy()
    Hx32, gb32, ga32 = exact_response(c32[..., :3], c32[..., 3:], n_fft, W.numpy())
    err = np.abs(H32.detach().cpu().numpy().astype(np.complex128) - Hx32)
    assert np.all(err <= 1e-6 * np.abs(Hx32) + 1e-7 * np.abs(Hx32).max(1, keepdims=True))
    e32 = _norm_rel(s32.grad.reshape(bs, -1).cpu().numpy(), np.concatenate([gb32, ga32], -1).reshape(bs, -1))
    assert np.all(e32 <= 1e-5), e32.max()
