"""GPU parity of the options of the multi-resolution STFT loss (auraloss's term weights, the A-weighting FIR, 8192-point frames;
csrc/stftloss.hip) against tests/auraloss_restated.py (float64 CPU torch.stft + conv1d + autograd). Tolerances as in
tests/test_gpu_losses.py: 2e-5 relative on the loss; gradients 1e-2 in relative L2 norm on generic inputs, 1e-4 (L2 and largest entry) on
well-conditioned ones (prediction = 1.5 x target + a little noise, the draw checked so that every log-magnitude difference keeps its sign
and no predicted magnitude is tiny). With the A-weighting in front the low bins are 40 dB down, so those draws are held to the bound of
that file's test_gradient_for_both_arguments (2e-3) instead."""
import time

import numpy as np
import pytest
import torch

from tests import auraloss_restated as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def res_kw(res):
    return dict(fft_sizes=[r[0] for r in res], hop_sizes=[r[1] for r in res], win_lengths=[r[2] for r in res])


def gpu_loss(D, p, t, res, **opts):
    pt, tt = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
    loss = D.losses.MultiResolutionSTFTLoss(**res_kw(res), **opts)(pt, tt)
    loss.backward()
    return float(loss.detach()), pt.grad.cpu().double().numpy(), tt.grad.cpu().double().numpy()


def ref_loss(D, p, t, res, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, perceptual_weighting=False, sample_rate=None, **_):
    taps = D.losses.a_weighting_taps(sample_rate) if perceptual_weighting else None
    return ar.loss_and_grads(p, t, res, w_sc=w_sc, w_log_mag=w_log_mag, w_lin_mag=w_lin_mag, taps=taps)


def rel2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def generic(shape, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(shape) * 0.3).astype(np.float32)
    b = (0.6 * a + 0.2 * rng.standard_normal(shape)).astype(np.float32)
    return a, b


def check(name, got, want, gtol, both=True, maxtol=None, ttol=None):
    (l, gp, gt), (lo, gpo, gto) = got, want
    el, ep, et = abs(l - lo) / abs(lo), rel2(gp, gpo), rel2(gt, gto)
    em = relmax(gp, gpo)
    print(f"{name}: loss {el:.2e}, input.grad rel L2 {ep:.2e} (max {em:.2e}), target.grad rel L2 {et:.2e}")
    assert el < 2e-5, (name, el)
    assert ep < gtol, (name, ep)
    if both:
        assert et < (gtol if ttol is None else ttol), (name, et)
    if maxtol is not None:
        assert em < maxtol, (name, em)


@pytest.mark.parametrize("shape", [(2, 1, 32768), (1, 2, 20000)])
def test_example_configuration(D, shape):
    """The loss of examples/auto_eq.py:252-262 / virtual_analog.py:288-298 exactly: seven resolutions 128 .. 8192 at hop n_fft / 2,
    w_sc = 0, w_phs = 0, log + linear magnitude, A-weighting at 44.1 kHz - value, input.grad and target.grad on generic inputs."""
    a, b = generic(shape, shape[-1])
    opts = dict(ar.EXAMPLE_KW, perceptual_weighting=True, sample_rate=44100)
    # target.grad: 2e-2. Both spectra come out of one packed transform, T = (Z[k] - conj Z[F-k]) / 2i, so a bin where |T| << |P| carries an
    # error of ~eps |P| / |T|, and the log-magnitude gradient weighs it by 1 / |T|; the target (0.6 x input + noise) is the quieter signal.
    # Measured: input.grad 2.2e-3 / 2.7e-3, target.grad 1.4e-3 / 1.2e-2; the float32 restatement on the CPU 2.0e-3 .. 5.2e-3.
    check(f"example {shape}", gpu_loss(D, a, b, ar.EXAMPLE_RESOLUTIONS, w_phs=0.0, **opts), ref_loss(D, a, b, ar.EXAMPLE_RESOLUTIONS, **opts), 1e-2,
          ttol=2e-2)


TERMS = {"w_sc": dict(w_sc=1.0, w_log_mag=0.0, w_lin_mag=0.0), "w_log_mag": dict(w_sc=0.0, w_log_mag=1.0, w_lin_mag=0.0),
         "w_lin_mag": dict(w_sc=0.0, w_log_mag=0.0, w_lin_mag=1.0)}


def well_conditioned(N, res, taps=None, floor=1e-3, noise=1e-3):
    """test_gpu_losses.py's construction: prediction = 1.5 x target + noise, the first draw whose (weighted) spectra keep every
    log-magnitude difference above 0.1 and every predicted magnitude above `floor` of the largest."""
    for seed in range(40):
        rng = np.random.default_rng(1000 * N + seed)
        b = (rng.standard_normal((1, 1, N)) * 0.3).astype(np.float32)
        a = (1.5 * b + noise * rng.standard_normal((1, 1, N))).astype(np.float32)
        pa, pb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        if taps is not None:
            pa, pb = ar.fir_same(pa, taps), ar.fir_same(pb, taps)
        ok = True
        for n_fft, hop, win in res:
            pm, tm = ar.stft_mag(pa, n_fft, hop, win), ar.stft_mag(pb, n_fft, hop, win)
            ok = ok and float(pm.min()) > floor * float(pm.max()) and float((pm.log() - tm.log()).min()) > 0.1
        if ok:
            return a, b, True
    return a, b, False


@pytest.mark.parametrize("fs", [None, 44100, 48000])
@pytest.mark.parametrize("term", list(TERMS))
def test_each_term_alone(D, term, fs):
    """One weight at 1, the others at 0 (so those terms are not computed), with and without the A-weighting, against the restatement."""
    res = ((256, 64, 256), (64, 16, 64))
    opts = dict(TERMS[term], **({} if fs is None else dict(perceptual_weighting=True, sample_rate=fs)))
    taps = None if fs is None else D.losses.a_weighting_taps(fs)
    a, b, ok = well_conditioned(3000, res, taps)
    if fs is None:
        assert ok, "the unweighted draw of test_gpu_losses.py is well-conditioned"
        check(f"{term} alone", gpu_loss(D, a, b, res, **opts), ref_loss(D, a, b, res, **opts), 1e-4, maxtol=1e-4)
    else:
        check(f"{term} alone, A-weighted at {fs}", gpu_loss(D, a, b, res, **opts), ref_loss(D, a, b, res, **opts), 2e-3)


@pytest.mark.parametrize("N,res", [(20000, ((8192, 3000, 6000),)), (4097, ((8192, 2048, 8192), (128, 64, 128))),
                                   (30001, ((8192, 1000, 8191), (4096, 999, 4000), (2048, 333, 2048)))])
def test_8192_point_frames(D, N, res):
    """n_fft = 8192 (one frame per 1024-thread workgroup): windows shorter than the frame, hops that do not divide N, N just above
    4096 (the reflect-padding limit), beside other resolutions; default weights. Generic inputs
    at 1e-2, the 1.5x construction at 3e-4 (test_gpu_losses.py's bound for thousands of bins per frame)."""
    a, b = generic((2, 1, N), N)
    check(f"8192 generic N={N}", gpu_loss(D, a, b, res), ref_loss(D, a, b, res), 1e-2)
    rng = np.random.default_rng(N + 1)
    t = (rng.standard_normal((1, 1, N)) * 0.3).astype(np.float32)
    p = (1.5 * t + 1e-5 * rng.standard_normal(t.shape)).astype(np.float32)
    check(f"8192 1.5x N={N}", gpu_loss(D, p, t, res, w_lin_mag=1.0), ref_loss(D, p, t, res, w_lin_mag=1.0), 3e-4)


def test_silent_target_without_spectral_convergence(D):
    """w_sc = 0 leaves the spectral convergence (which divides by the target's norm) out: a silent target gives a finite loss and finite
    gradients, equal to the restatement's."""
    rng = np.random.default_rng(2)
    p = (rng.standard_normal((2, 1, 20000)) * 0.3).astype(np.float32)
    t = np.zeros_like(p)
    for opts in (dict(w_sc=0.0, w_log_mag=1.0, w_lin_mag=1.0), dict(ar.EXAMPLE_KW, perceptual_weighting=True, sample_rate=44100)):
        res = ar.EXAMPLE_RESOLUTIONS if "sample_rate" in opts else ((1024, 256, 1024), (8192, 4096, 8192))
        l, gp, gt = gpu_loss(D, p, t, res, **opts)
        assert np.isfinite(l) and np.isfinite(gp).all() and np.isfinite(gt).all()
        lo, gpo, _ = ref_loss(D, p, t, res, **opts)
        assert abs(l - lo) < 2e-5 * abs(lo) and rel2(gp, gpo) < 1e-2, (opts, l, lo, rel2(gp, gpo))


@pytest.mark.parametrize("ntaps", [101, 7])
@pytest.mark.parametrize("rows,N", [(3, 1), (2, 37), (2, 100), (2, 2047), (1, 2048), (2, 2049), (1, 4095), (2, 4097), (300, 3000)])
def test_fir_exports(D, rows, N, ntaps):
    """dasp_fir_same_forward / _adjoint through ctypes against float64 conv1d / conv_transpose1d on asymmetric taps (the adjoint is the
    true one, not the symmetric shortcut); outputs bit-identical run to run; the one-signal adjoint equals the first of the pair."""
    from dasp_pytorch_amd._lib import call, ptr, stream
    rng = np.random.default_rng(rows * 10007 + N + ntaps)
    h = rng.standard_normal(ntaps).astype(np.float32)
    x0, x1, g0, g1 = (dev(rng.standard_normal((rows, N)).astype(np.float32)) for _ in range(4))
    taps = dev(h)
    outs = [torch.empty_like(x0) for _ in range(6)]
    call("dasp_fir_same_forward", ptr(x0), ptr(x1), ptr(outs[0]), ptr(outs[1]), ptr(taps), ntaps, rows, N, stream())
    call("dasp_fir_same_adjoint", ptr(g0), ptr(g1), ptr(outs[2]), ptr(outs[3]), ptr(taps), ntaps, rows, N, stream())
    call("dasp_fir_same_adjoint", ptr(g0), ptr(None), ptr(outs[4]), ptr(None), ptr(taps), ntaps, rows, N, stream())
    call("dasp_fir_same_forward", ptr(x0), ptr(x1), ptr(outs[5]), ptr(outs[1]), ptr(taps), ntaps, rows, N, stream())
    torch.cuda.synchronize()
    scale = float(np.abs(h).sum())
    for got, src, fn in ((outs[0], x0, ar.fir_same), (outs[1], x1, ar.fir_same), (outs[2], g0, ar.fir_same_adjoint), (outs[3], g1, ar.fir_same_adjoint)):
        s = src.cpu().double()
        want = fn(s, h.astype(np.float64))
        err = float((got.cpu().double() - want).abs().max())
        assert err <= 1e-6 * scale * float(s.abs().max()), (rows, N, ntaps, err)
    assert torch.equal(outs[0], outs[5]) and torch.equal(outs[2], outs[4])


def test_graph_replay_of_the_example_loss(D):
    """The auto_eq configuration captured with its backward (taps and twiddles built inside the capture) and replayed with new inputs in
    the same buffers on an idle device equals eager calls (loss: the same fixed-order sums; gradients: float atomics, order only)."""
    fn = D.losses.MultiResolutionSTFTLoss(**res_kw(ar.EXAMPLE_RESOLUTIONS), **ar.EXAMPLE_KW, perceptual_weighting=True, sample_rate=44100)
    g = torch.Generator(device=DEV).manual_seed(11)
    mk = lambda: torch.randn(2, 1, 32768, device=DEV, generator=g) * 0.3
    xs, ts = mk().requires_grad_(True), mk()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn(xs, ts).backward()
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls = fn(xs, ts)
        ls.backward()
    for k in range(3):
        xn, tn = mk(), mk()
        with torch.no_grad():
            xs.copy_(xn); ts.copy_(tn)
        xs.grad.zero_()
        torch.cuda.synchronize()
        time.sleep(0.05)
        graph.replay()
        xe = xn.clone().requires_grad_(True)
        le = fn(xe, tn)
        le.backward()
        assert float(ls.detach()) == float(le.detach()), (k, float(ls), float(le))
        assert float((xs.grad - xe.grad).abs().max()) <= 1e-5 * float(xe.grad.abs().max()), k


def test_auto_eq_training_step(D):
    """The step of examples/auto_eq.py: ParametricEQ(44100, max_q_factor=1.0).process_normalized -> the example's loss -> backward at
    (16, 1, 131072): finite loss and parameter gradients; the loss and gradient of a two-row slice of the EQ output against the restatement."""
    torch.manual_seed(0)
    eq = D.ParametricEQ(44100, max_q_factor=1.0)
    x = torch.randn(16, 1, 131072, device=DEV) * 0.2
    target = torch.randn(16, 1, 131072, device=DEV) * 0.2
    params = torch.rand(16, eq.num_params, device=DEV).requires_grad_(True)
    fn = D.losses.MultiResolutionSTFTLoss(**res_kw(ar.EXAMPLE_RESOLUTIONS), **ar.EXAMPLE_KW, w_phs=0.0, perceptual_weighting=True, sample_rate=44100)
    y = eq.process_normalized(x, params)
    loss = fn(y, target)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(params.grad).all() and float(params.grad.abs().max()) > 0
    ys = y.detach()[:2].cpu().numpy()
    tsl = target[:2].cpu().numpy()
    opts = dict(ar.EXAMPLE_KW, perceptual_weighting=True, sample_rate=44100)
    check("auto_eq slice (2,1,131072)", gpu_loss(D, ys, tsl, ar.EXAMPLE_RESOLUTIONS, **opts), ref_loss(D, ys, tsl, ar.EXAMPLE_RESOLUTIONS, **opts), 1e-2)


def test_opts_none_is_unit_weights(D):
    """opts=None (what the modules carry for auraloss's defaults) and the explicit weights (1, 1, 0) with no sample rate are the same
    call of dasp_mrstft_forward: the same loss bit for bit."""
    from dasp_pytorch_amd import losses
    a, b = generic((2, 2, 20000), 4)
    res = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240), (256, 64, 256))
    l0 = losses.MultiResolutionSTFTLoss(**res_kw(res))(dev(a), dev(b))
    l1 = losses._MRSTFTFunction.apply(dev(a), dev(b), tuple(res), 1e-8, (1.0, 1.0, 0.0, None))
    assert float(l0) == float(l1)


def test_unsupported_sizes_raise(D):
    from dasp_pytorch_amd._lib import DaspHipError
    x, y = torch.rand(1, 1, 40000, device=DEV), torch.rand(1, 1, 40000, device=DEV)
    for res in (((16384, 4096, 16384),), ((1024, 256, 2048),), ((8192, 4096, 8192),)):
        for opts in ({}, dict(w_lin_mag=1.0, perceptual_weighting=True, sample_rate=44100)):
            n = 4000 if res[0][0] == 8192 else 40000           # 8192-point frames need more than 4096 samples
            with pytest.raises(DaspHipError):
                D.losses.MultiResolutionSTFTLoss(**res_kw(res), **opts)(x[..., :n], y[..., :n])
