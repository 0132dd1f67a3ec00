"""GPU parity of the mel-scaled STFT losses (scale="mel" / n_bins, MelSTFTLoss; mrstft_mel_fwd_kernel / mrstft_mel_bwd_kernel and the
per-resolution mel table of csrc/stftloss.hip) against tests/auraloss_mel_restated.py (float64 CPU torch.stft + matmul + autograd):
loss, input.grad and target.grad. Inputs and bounds are those of tests/test_gpu_mrstft_options.py: 2e-5 relative on the loss; gradients
1e-2 in relative L2 norm on generic inputs, 1e-4 (L2 and largest entry) on the well-conditioned draw (prediction = 1.5 x target + a
little noise, accepted on the mel magnitudes), 2e-3 on that draw behind the A-weighting. Sample rate 44100 throughout. The float32
restatement on the CPU sits at <= 1.1e-7 (loss), <= 2.8e-6 (gradients) and <= 8.1e-6 (gradients, A-weighted) at these shapes, so the
bounds are far from tight for the arithmetic; each test prints what it measured.

Measured on an MI355X (first run of this file; relative error of the loss, relative L2 of input.grad (largest entry) and of target.grad):
  case E  4.0e-8  1.5e-7 (1.7e-7)  2.7e-7        case A  2.9e-8  5.4e-7 (1.6e-6)  1.4e-6        case B  2.1e-8  2.5e-7 (3.2e-7)  3.9e-7
  case D  2.0e-8  2.7e-6 (2.7e-6)  3.3e-7        case C  3.2e-8  5.6e-6 (8.1e-6)  1.7e-5        11 empty filters  3.2e-8  3.1e-7 (4.3e-7)  4.2e-7
  w_sc alone       2.6e-8  2.8e-7 (5.6e-7)  2.0e-7     A-weighted  5.9e-8  3.3e-7 (5.4e-7)  2.5e-7
  w_log_mag alone  3.5e-8  5.0e-7 (8.6e-7)  4.7e-7     A-weighted  2.5e-8  2.9e-6 (5.6e-6)  1.6e-6
  w_lin_mag alone  7.7e-8  5.8e-7 (1.4e-6)  4.0e-7     A-weighted  6.0e-8  2.6e-7 (5.1e-7)  2.5e-7
  device tables: every entry of all six equal to losses.mel_filterbank bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import auraloss_mel_restated as amr
from tests import auraloss_restated as ar
from tests.test_gpu_mrstft_options import TERMS, check, dev, generic, rel2, res_kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 44100


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def gpu_loss(D, p, t, res, n_bins, **opts):
    pt, tt = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
    loss = D.losses.MultiResolutionSTFTLoss(**res_kw(res), scale="mel", n_bins=n_bins, sample_rate=SR, **opts)(pt, tt)
    loss.backward()
    return float(loss.detach()), pt.grad.cpu().double().numpy(), tt.grad.cpu().double().numpy()


def ref_loss(D, p, t, res, n_bins, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, perceptual_weighting=False):
    taps = D.losses.a_weighting_taps(SR) if perceptual_weighting else None
    return amr.loss_and_grads(p, t, res, SR, n_bins, w_sc=w_sc, w_log_mag=w_log_mag, w_lin_mag=w_lin_mag, taps=taps)


# name: shape, resolutions, n_bins, options - the smallest shapes at which each piece can go wrong
CASES = {
    "E": ((1, 1, 200), ((8, 4, 8),), 2, {}),                                                    # 512 frames per workgroup, one partial group
    "A": ((1, 3, 3000), ((64, 16, 64), (256, 64, 200)), 8, dict(w_lin_mag=0.5)),                # ragged last frame group, window shorter than the frame
    "B": ((2, 1, 6000), ((512, 128, 512), (1024, 256, 1024), (2048, 512, 2048)), 40, {}),       # the sizes whose default loss runs the split kernels
    "D": ((1, 1, 9000), ((4096, 1000, 3000),), 128, dict(w_sc=0.5, w_lin_mag=1.0)),             # one frame per workgroup in the 512-thread instance
    "C": ((1, 2, 20000), ((1024, 256, 1024), (2048, 512, 2048), (8192, 2048, 8192)), 128,       # auraloss's README loss, with the 1024-thread
          dict(perceptual_weighting=True)),                                                     # 8192-point instance
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case and the float64 reference, computed once and shared (read-only)."""
    import dasp_pytorch_amd as D
    shape, res, n_bins, opts = CASES[name]
    a, b = generic(shape, shape[-1])
    want = ref_loss(D, a, b, res, n_bins, **opts)
    for v in want[1:]:
        v.flags.writeable = False
    return a, b, want


@pytest.mark.parametrize("name", list(CASES))
def test_shapes(D, name):
    _, res, n_bins, opts = CASES[name]
    a, b, want = case_data(name)
    check(f"mel case {name}", gpu_loss(D, a, b, res, n_bins, **opts), want, 1e-2)


def well_conditioned_mel(N, res, n_bins, taps=None, floor=1e-3, noise=1e-3):
    """tests/test_gpu_mrstft_options.py's construction with the mel magnitudes in the acceptance check: prediction = 1.5 x target +
    noise, the first draw whose (weighted) mel spectra keep every log-magnitude difference above 0.1 and every predicted magnitude above
    `floor` of the largest. Returns the seed's offset as well."""
    for seed in range(40):
        rng = np.random.default_rng(1000 * N + seed)
        b = (rng.standard_normal((1, 1, N)) * 0.3).astype(np.float32)
        a = (1.5 * b + noise * rng.standard_normal((1, 1, N))).astype(np.float32)
        pa, pb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
        if taps is not None:
            pa, pb = ar.fir_same(pa, taps), ar.fir_same(pb, taps)
        ok = True
        for n_fft, hop, win in res:
            pm, tm = amr.mel_mag(pa, n_fft, hop, win, SR, n_bins), amr.mel_mag(pb, n_fft, hop, win, SR, n_bins)
            ok = ok and float(pm.min()) > floor * float(pm.max()) and float((pm.log() - tm.log()).min()) > 0.1
        if ok:
            return a, b, seed
    return a, b, None


@pytest.mark.parametrize("aw", [False, True])
@pytest.mark.parametrize("term", list(TERMS))
def test_each_term_alone(D, term, aw):
    """One weight at 1, the others at 0 (those terms are not computed), with and without the A-weighting, on the well-conditioned draw."""
    res, n_bins = ((256, 64, 256), (64, 16, 64)), 8
    opts = dict(TERMS[term], perceptual_weighting=aw)
    a, b, seed = well_conditioned_mel(3000, res, n_bins, D.losses.a_weighting_taps(SR) if aw else None)
    if not aw:
        assert seed == 0, "seed 0 of the construction is well-conditioned on the mel magnitudes"
        check(f"mel {term} alone", gpu_loss(D, a, b, res, n_bins, **opts), ref_loss(D, a, b, res, n_bins, **opts), 1e-4, maxtol=1e-4)
    else:
        assert seed is not None, "no well-conditioned draw behind the A-weighting"
        check(f"mel {term} alone, A-weighted", gpu_loss(D, a, b, res, n_bins, **opts), ref_loss(D, a, b, res, n_bins, **opts), 2e-3)


def test_empty_filters_without_the_log_term(D):
    """128 filters on 512-point frames at 44.1 kHz leave 11 rows of the filterbank empty: with w_log_mag = 0 they add 0 to the sums, still
    count in the mean, and reach no bin in the backward."""
    res, n_bins, opts = ((512, 128, 512),), 128, dict(w_sc=1.0, w_log_mag=0.0, w_lin_mag=1.0)
    a, b = generic((1, 2, 3000), 77)
    got = gpu_loss(D, a, b, res, n_bins, **opts)
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    check("mel with 11 empty filters, w_log_mag = 0", got, ref_loss(D, a, b, res, n_bins, **opts), 1e-2)


def test_gradient_paths(D):
    """Only the input, only the target, or both require a gradient: the gradient they share is the same bit for bit. The backward adds
    with float atomics, whose order is free, so the shape is one where the order cannot matter: one resolution with hop = n_fft, where a
    sample receives at most two contributions (its frame's, and a reflected one at either end) and a sum of two floats onto zero commutes."""
    a, b = generic((1, 2, 3000), 5)
    fn = D.losses.MultiResolutionSTFTLoss((64,), (64,), (64,), scale="mel", n_bins=8, sample_rate=SR, w_lin_mag=0.5)
    grads = {}
    for which in ("input", "target", "both"):
        pt, tt = dev(a).requires_grad_(which != "target"), dev(b).requires_grad_(which != "input")
        fn(pt, tt).backward()
        grads[which] = (pt.grad, tt.grad)
    assert grads["input"][1] is None and grads["target"][0] is None
    assert float(grads["both"][0].abs().max()) > 0 and float(grads["both"][1].abs().max()) > 0
    assert torch.equal(grads["input"][0], grads["both"][0])
    assert torch.equal(grads["target"][1], grads["both"][1])
    _, gp, gt = ref_loss(D, a, b, ((64, 64, 64),), 8, w_lin_mag=0.5)
    assert rel2(grads["both"][0].cpu().double().numpy(), gp) < 1e-2 and rel2(grads["both"][1].cpu().double().numpy(), gt) < 1e-2


def test_class_equivalence(D):
    """MelSTFTLoss(44100) is STFTLoss(scale="mel", n_bins=128, sample_rate=44100) is mrstft_loss(..., one resolution): the same bits."""
    a, b = (dev(v) for v in generic((2, 1, 6000), 8))
    l0 = D.losses.MelSTFTLoss(SR)(a, b)
    l1 = D.losses.STFTLoss(scale="mel", n_bins=128, sample_rate=SR)(a, b)
    l2 = D.losses.mrstft_loss(a, b, (1024,), (256,), (1024,), scale="mel", n_bins=128, sample_rate=SR)
    assert torch.isfinite(l0) and float(l0) > 0
    assert float(l0) == float(l1) == float(l2)
    want = amr.loss_and_grads(a.cpu().numpy(), b.cpu().numpy(), ((1024, 256, 1024),), SR, 128)[0]
    assert abs(float(l0) - want) < 2e-5 * abs(want)


def test_run_to_run(D):
    """The forward adds in a fixed order: two calls return the same bits. The backward's float atomics leave the order of the overlapping
    frames free: 1e-5 of the largest entry, as for the existing loss."""
    _, res, n_bins, opts = CASES["B"]
    a, b, _ = case_data("B")
    fn = D.losses.MultiResolutionSTFTLoss(**res_kw(res), scale="mel", n_bins=n_bins, sample_rate=SR, **opts)
    outs = []
    for _ in range(2):
        pt, tt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        loss = fn(pt, tt)
        loss.backward()
        outs.append((loss.detach().clone(), pt.grad, tt.grad))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in (1, 2):
        assert float((outs[0][k] - outs[1][k]).abs().max()) <= 1e-5 * float(outs[0][k].abs().max())


@pytest.mark.parametrize("sr,n_fft,n_bins", [(44100, 8, 2), (44100, 64, 8), (16000, 512, 40), (44100, 2048, 128), (48000, 1024, 128), (44100, 8192, 256)])
def test_device_table(D, sr, n_fft, n_bins):
    """dasp_mel_table_store + dasp_mel_table_dense against losses.mel_filterbank: both compute in fp64 from the same edges and round once,
    so every entry agrees within one float32 ulp of its row's maximum and the zero pattern is identical."""
    from dasp_pytorch_amd._lib import call, lib, ptr, stream
    nfl = lib().dasp_mel_table_floats(n_fft, n_bins)
    assert nfl == 3 * (n_fft // 2 + 1) + 2 * n_bins
    tab = torch.empty(nfl, dtype=torch.float32, device=DEV)
    dense = torch.full((n_bins, n_fft // 2 + 1), -1.0, dtype=torch.float32, device=DEV)
    edges = D.losses.mel_edges(float(sr), n_bins)
    call("dasp_mel_table_store", ptr(tab), edges.ctypes.data_as(ctypes.c_void_p), float(sr), n_fft, n_bins, stream())
    call("dasp_mel_table_dense", ptr(tab), ptr(dense), n_fft, n_bins, stream())
    got, want = dense.cpu().numpy(), D.losses.mel_filterbank(sr, n_fft, n_bins)
    assert np.array_equal(got > 0, want > 0) and (got >= 0).all()
    ulp = np.spacing(want.max(axis=1, keepdims=True))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"mel table ({sr}, {n_fft}, {n_bins}): largest deviation {float((err / ulp).max()):.2f} ulp of the row maximum, {int((got != want).sum())} entries differ")
    assert (err <= ulp).all()


def test_graph_replay(D):
    """Case B with its backward captured on one stream after an eager call (twiddles and mel tables are then built inside the capture, as
    kernel nodes) and replayed on new data in the same buffers: the loss equals the eager value (fixed-order sums), the gradients agree to
    1e-5 of the largest entry (float atomics: order only)."""
    shape, res, n_bins, opts = CASES["B"]
    fn = D.losses.MultiResolutionSTFTLoss(**res_kw(res), scale="mel", n_bins=n_bins, sample_rate=SR, **opts)
    g = torch.Generator(device=DEV).manual_seed(12)
    mk = lambda: torch.randn(*shape, device=DEV, generator=g) * 0.3
    xs, ts = mk().requires_grad_(True), mk().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(xs, ts).backward()
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = None; ts.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls = fn(xs, ts)
        ls.backward()
    for k in range(2):
        xn, tn = mk(), mk()
        with torch.no_grad():
            xs.copy_(xn); ts.copy_(tn)
        xs.grad.zero_(); ts.grad.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        xe, te = xn.clone().requires_grad_(True), tn.clone().requires_grad_(True)
        le = fn(xe, te)
        le.backward()
        assert float(ls.detach()) == float(le.detach()), (k, float(ls), float(le))
        assert float((xs.grad - xe.grad).abs().max()) <= 1e-5 * float(xe.grad.abs().max()), k
        assert float((ts.grad - te.grad).abs().max()) <= 1e-5 * float(te.grad.abs().max()), k
