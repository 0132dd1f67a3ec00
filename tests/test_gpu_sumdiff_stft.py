"""GPU parity of SumAndDifferenceSTFTLoss (the item-owned kernels mrstft_sd_* of csrc/stftloss.hip: both channels gathered once, the
sum and the difference half transformed in one workgroup, the backward through one packed inverse transform) against
tests/auraloss_sumdiff_restated.py (float64 CPU torch.stft + conv1d + matmul + autograd). Helpers and bounds are those of
tests/test_gpu_mrstft_options.py: 2e-5 relative on each of loss, sum_loss and diff_loss; gradients 1e-2 in relative L2 norm on `generic`
inputs, 1e-4 (L2 and largest entry) on the well-conditioned stereo draw, 2e-3 on that draw behind the A-weighting. Against the composition
of two calls of the existing loss on the device: 1e-6 on the loss, 1e-4 relative L2 on the gradients. w_sum = 0.7, w_diff = 1.3 throughout,
sample rate 44100. The float32 restatement on the CPU sits at <= 1.8e-7 (loss) and <= 1.9e-3 (gradients, case B) at these shapes, the two
mel cases at <= 1.8e-7 and <= 1.3e-6 - inside the bounds, which therefore stay as they are. Every test prints what it measured.

Measured on an MI355X (relative error of the loss, relative L2 of input.grad (largest entry) and of target.grad; sum_loss and diff_loss
<= 7.9e-8 everywhere but the A-weighted w_log_mag row, 1.0e-6):
  case E      5.6e-8  3.6e-6 (4.7e-6)  5.8e-6      case A  5.9e-8  1.3e-5 (1.3e-5)  3.8e-5      case B      2.2e-8  1.9e-4 (1.2e-4)  3.5e-4
  case D      1.1e-7  3.9e-3 (3.5e-3)  2.9e-3      case C  3.6e-8  1.2e-6 (6.0e-7)  1.5e-6      case C plain 4.5e-8  6.6e-4 (4.8e-4)  7.6e-5
  case mel A  6.7e-8  7.8e-7 (1.6e-6)  3.7e-7
  w_sc alone       4.0e-8  1.7e-7 (2.3e-7)  1.7e-7    8 mel bins  4.3e-9  1.8e-7 (2.9e-7)  1.8e-7    A-weighted  5.0e-8  3.8e-7 (5.1e-7)  2.9e-7
  w_log_mag alone  1.1e-8  1.8e-6 (2.0e-6)  2.0e-6    8 mel bins  6.0e-8  7.3e-7 (1.9e-6)  6.1e-7    A-weighted  1.0e-6  4.6e-4 (2.9e-4)  2.3e-4
  w_lin_mag alone  4.1e-8  1.5e-7 (2.3e-7)  1.6e-7    8 mel bins  4.9e-8  1.8e-7 (3.3e-7)  1.8e-7    A-weighted  1.0e-7  4.1e-7 (4.4e-7)  3.2e-7
  (A-weighted on 8 mel bins: <= 6.9e-8, <= 4.5e-7 (7.4e-7), <= 3.5e-7)
  sum_loss.backward() / diff_loss.backward() alone: case A 8.1e-6 / 9.6e-6 and 1.4e-5 / 6.1e-5, mel A <= 7.9e-7
  against the composition: loss equal bit for bit, gradients 1.8e-7 / 3.6e-7 (plain), 1.5e-7 / 1.8e-7 (mel)
  channel swap: loss equal bit for bit, gradients swapped to 1.3e-7 (plain) / 1.8e-7 (mel) of the largest entry."""
import functools

import numpy as np
import pytest
import torch

from tests import auraloss_restated as ar
from tests import auraloss_sumdiff_restated as sdr
from tests.test_gpu_mrstft_options import TERMS, check, dev, generic, rel2, res_kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 44100
W = dict(w_sum=0.7, w_diff=1.3)


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def split_opts(opts):
    """The package's keywords -> the restatement's (taps for perceptual_weighting, n_bins with the sample rate)."""
    from dasp_pytorch_amd import losses
    o = dict(opts)
    kw = {k: o[k] for k in ("w_sc", "w_log_mag", "w_lin_mag", "w_sum", "w_diff") if k in o}
    if o.get("perceptual_weighting"):
        kw["taps"] = losses.a_weighting_taps(SR)
    if o.get("n_bins") is not None:
        kw.update(sample_rate=SR, n_bins=o["n_bins"])
    return kw


def pkg_opts(opts):
    o = dict(opts)
    if o.get("n_bins") is not None:
        o.update(scale="mel", sample_rate=SR)
    if o.get("perceptual_weighting"):
        o["sample_rate"] = SR
    return o


def gpu_full(D, p, t, res, backward="loss", **opts):
    pt, tt = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
    out = D.losses.SumAndDifferenceSTFTLoss(**res_kw(res), output="full", **pkg_opts(opts))(pt, tt)
    out[("loss", "sum", "diff").index(backward)].backward()
    return tuple(float(v.detach()) for v in out) + (pt.grad.cpu().double().numpy(), tt.grad.cpu().double().numpy())


def ref_full(p, t, res, backward="loss", **opts):
    return sdr.loss_and_grads(p, t, res, backward=backward, **split_opts(opts))


def check_full(name, got, want, gtol, maxtol=None):
    """`check` on (loss, gradients), and sum_loss and diff_loss held to the loss's bound."""
    for which, g, w in (("sum_loss", got[1], want[1]), ("diff_loss", got[2], want[2])):
        e = abs(g - w) / abs(w)
        print(f"{name}: {which} {e:.2e}")
        assert e < 2e-5, (name, which, e)
    check(name, (got[0], got[3], got[4]), (want[0], want[3], want[4]), gtol, maxtol=maxtol)


R3 = ((1024, 256, 1024), (2048, 512, 2048), (8192, 2048, 8192))
# name: shape, resolutions, options - the smallest shapes at which each piece can go wrong
CASES = {
    "E": ((1, 2, 200), ((8, 4, 8),), {}),                                                        # 512 frames per workgroup, one partial group
    "A": ((2, 2, 3000), ((64, 16, 64), (256, 64, 200)), dict(w_lin_mag=0.5)),                    # two items, ragged last group, window < frame
    "B": ((1, 2, 6000), ((512, 128, 512), (1024, 256, 1024), (2048, 512, 2048)), {}),            # the sizes the mono loss sends to the split kernels
    "D": ((1, 2, 9000), ((4096, 1000, 3000),), dict(w_sc=0.5, w_lin_mag=1.0)),                   # one frame per workgroup
    "C": ((1, 2, 20000), R3, dict(n_bins=128, perceptual_weighting=True)),                       # auraloss's README loss: the 1024-thread mel instance
    "C plain": ((1, 2, 20000), R3, {}),                                                          # the 1024-thread instance of the plain kernels
    "mel A": ((2, 2, 3000), ((64, 16, 64), (256, 64, 200)), dict(w_lin_mag=0.5, n_bins=8)),
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case and the float64 reference, computed once and shared (read-only)."""
    shape, res, opts = CASES[name]
    a, b = generic(shape, shape[-1])
    want = ref_full(a, b, res, **W, **opts)
    for v in want[3:]:
        v.flags.writeable = False
    return a, b, want


@pytest.mark.parametrize("name", list(CASES))
def test_shapes(D, name):
    _, res, opts = CASES[name]
    a, b, want = case_data(name)
    check_full(f"sum/diff case {name}", gpu_full(D, a, b, res, **W, **opts), want, 1e-2)


def well_conditioned_stereo(N, res, taps=None, floor=1e-3, noise=1e-3):
    """tests/test_gpu_mrstft_options.py's construction on a stereo pair: prediction = 1.5 x target + noise, the first draw whose sum AND
    difference spectra keep every log-magnitude difference above 0.1 and every predicted magnitude above `floor` of the largest."""
    for seed in range(40):
        rng = np.random.default_rng(1000 * N + seed)
        b = (rng.standard_normal((1, 2, N)) * 0.3).astype(np.float32)
        a = (1.5 * b + noise * rng.standard_normal((1, 2, N))).astype(np.float32)
        ok = True
        for pa, pb in zip(sdr.sum_diff(torch.from_numpy(a).double()), sdr.sum_diff(torch.from_numpy(b).double())):
            if taps is not None:
                pa, pb = ar.fir_same(pa, taps), ar.fir_same(pb, taps)
            for n_fft, hop, win in res:
                pm, tm = ar.stft_mag(pa, n_fft, hop, win), ar.stft_mag(pb, n_fft, hop, win)
                ok = ok and float(pm.min()) > floor * float(pm.max()) and float((pm.log() - tm.log()).min()) > 0.1
        if ok:
            return a, b, seed
    return a, b, None


WC_RES = ((256, 64, 256), (64, 16, 64))


@functools.lru_cache(maxsize=None)
def wc_draw(aw):
    from dasp_pytorch_amd import losses
    a, b, seed = well_conditioned_stereo(2000, WC_RES, losses.a_weighting_taps(SR) if aw else None)
    return a, b, seed


@pytest.mark.parametrize("n_bins", [None, 8])
@pytest.mark.parametrize("aw", [False, True])
@pytest.mark.parametrize("term", list(TERMS))
def test_each_term_alone(D, term, aw, n_bins):
    """One weight at 1, the others at 0, with and without the A-weighting, plain and on 8 mel bins, on the well-conditioned stereo draw
    (accepted on the plain sum and difference spectra; behind the A-weighting no draw is, and the bound is the wider 2e-3, as in
    tests/test_gpu_mrstft_options.py)."""
    opts = dict(TERMS[term], perceptual_weighting=aw, n_bins=n_bins, **W)
    a, b, seed = wc_draw(aw)
    name = f"sum/diff {term} alone" + (", A-weighted" if aw else "") + (", 8 mel bins" if n_bins else "")
    if not aw:
        assert seed == 0, "seed 0 of the stereo construction is well-conditioned"
        check_full(name, gpu_full(D, a, b, WC_RES, **opts), ref_full(a, b, WC_RES, **opts), 1e-4, maxtol=1e-4)
    else:
        assert seed is None, "no draw of the construction is accepted behind the A-weighting: the last of the 40 is used, at the wider bound"
        check_full(name, gpu_full(D, a, b, WC_RES, **opts), ref_full(a, b, WC_RES, **opts), 2e-3)


@pytest.mark.parametrize("name", ["A", "mel A"])
def test_output_full_and_each_half_alone(D, name):
    """output="full": the three values; sum_loss.backward() alone and diff_loss.backward() alone give the restatement's gradients of that
    half - each half has its own element of the two-element gloss (the other is 0)."""
    _, res, opts = CASES[name]
    a, b, want = case_data(name)
    for which in ("sum", "diff"):
        got = gpu_full(D, a, b, res, backward=which, **W, **opts)
        ref = ref_full(a, b, res, backward=which, **W, **opts)
        for k in range(3):
            assert abs(got[k] - want[k]) < 2e-5 * abs(want[k]), (name, which, k)
        ep, et = rel2(got[3], ref[3]), rel2(got[4], ref[4])
        print(f"sum/diff case {name}, {which}_loss.backward(): input.grad rel L2 {ep:.2e}, target.grad rel L2 {et:.2e}")
        assert ep < 1e-2 and et < 1e-2, (name, which, ep, et)
    fn = D.losses.SumAndDifferenceSTFTLoss(**res_kw(res), **W, **pkg_opts(opts))
    only = fn(dev(a), dev(b))
    assert only.shape == () and abs(float(only) - want[0]) < 2e-5 * abs(want[0])
    fl = D.losses.sum_and_difference_stft_loss(dev(a), dev(b), **res_kw(res), **W, **pkg_opts(opts))
    assert float(fl) == float(only)


@pytest.mark.parametrize("opts", [dict(w_lin_mag=0.5), dict(w_lin_mag=0.5, n_bins=8)], ids=["plain", "mel"])
def test_against_the_composition_on_the_device(D, opts):
    """(w_sum mrstft_loss(s) + w_diff mrstft_loss(d)) / 2 with s and d formed by torch ops and the existing loss, on the well-conditioned
    draw: the same arithmetic up to the order of the sums and the packed inverse transform. (Not behind the A-weighting: the composition
    filters L + R where the fused loss adds the filtered channels, another rounding of every sample, and no draw is well-conditioned
    there - the A-weighted paths are held against the float64 restatement instead.)"""
    a, b, _ = wc_draw(False)
    o = pkg_opts(opts)
    pt, tt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    loss = D.losses.SumAndDifferenceSTFTLoss(**res_kw(WC_RES), **W, **o)(pt, tt)
    loss.backward()
    pc, tc = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    mono = D.losses.MultiResolutionSTFTLoss(**res_kw(WC_RES), **o)
    comp = (W["w_sum"] * mono(pc[:, 0:1] + pc[:, 1:2], tc[:, 0:1] + tc[:, 1:2])
            + W["w_diff"] * mono(pc[:, 0:1] - pc[:, 1:2], tc[:, 0:1] - tc[:, 1:2])) / 2
    comp.backward()
    el = abs(float(loss.detach()) - float(comp.detach())) / abs(float(comp.detach()))
    ep = rel2(pt.grad.cpu().double().numpy(), pc.grad.cpu().double().numpy())
    et = rel2(tt.grad.cpu().double().numpy(), tc.grad.cpu().double().numpy())
    print(f"fused against the composition ({opts}): loss {el:.2e}, input.grad rel L2 {ep:.2e}, target.grad rel L2 {et:.2e}")
    assert el < 1e-6 and ep < 1e-4 and et < 1e-4, (el, ep, et)


@pytest.mark.parametrize("n_bins", [None, 8])
def test_degenerate_stereo(D, n_bins):
    """L == R in both signals: the difference half is silent, diff_loss == 0.0 exactly and the gradients are finite; R == -L: sum_loss ==
    0.0. Swapping the channels of both signals leaves the loss (1e-6) and swaps the gradients (1e-5 of the largest entry)."""
    res, opts = CASES["A"][1], dict(w_lin_mag=0.5, n_bins=n_bins, **W)
    a, b, _ = case_data("A")
    for sign, zero in ((1.0, 2), (-1.0, 1)):
        a2, b2 = a.copy(), b.copy()
        a2[:, 1] = sign * a2[:, 0]; b2[:, 1] = sign * b2[:, 0]
        got = gpu_full(D, a2, b2, res, **opts)
        assert got[zero] == 0.0, (sign, got[:3])
        assert got[3 - zero] > 0 and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    got = gpu_full(D, a, b, res, **opts)
    swp = gpu_full(D, a[:, ::-1], b[:, ::-1], res, **opts)
    el = abs(got[0] - swp[0]) / abs(got[0])
    eg = max(float(np.abs(swp[k][:, ::-1] - got[k]).max() / np.abs(got[k]).max()) for k in (3, 4))
    print(f"channel swap (n_bins={n_bins}): loss {el:.2e}, gradients {eg:.2e} of the largest entry")
    assert el < 1e-6 and eg < 1e-5, (el, eg)


@pytest.mark.parametrize("n_bins", [None, 8])
def test_gradient_paths(D, n_bins):
    """Only the input, only the target, or both require a gradient: the gradient they share is the same bit for bit. One resolution with
    hop = n_fft, where a sample receives at most two contributions per channel, so the order of the float atomics cannot matter."""
    a, b = generic((2, 2, 3000), 5)
    fn = D.losses.SumAndDifferenceSTFTLoss((64,), (64,), (64,), **W, **pkg_opts(dict(w_lin_mag=0.5, n_bins=n_bins)))
    grads = {}
    for which in ("input", "target", "both"):
        pt, tt = dev(a).requires_grad_(which != "target"), dev(b).requires_grad_(which != "input")
        fn(pt, tt).backward()
        grads[which] = (pt.grad, tt.grad)
    assert grads["input"][1] is None and grads["target"][0] is None
    assert float(grads["both"][0].abs().max()) > 0 and float(grads["both"][1].abs().max()) > 0
    assert torch.equal(grads["input"][0], grads["both"][0])
    assert torch.equal(grads["target"][1], grads["both"][1])
    ref = ref_full(a, b, ((64, 64, 64),), w_lin_mag=0.5, n_bins=n_bins, **W)
    assert rel2(grads["both"][0].cpu().double().numpy(), ref[3]) < 1e-2 and rel2(grads["both"][1].cpu().double().numpy(), ref[4]) < 1e-2


@pytest.mark.parametrize("name", ["B", "C"])
def test_run_to_run(D, name):
    """The forward adds in a fixed order: two calls return the same bits of all three values. The backward's float atomics leave the order
    of the overlapping frames free: 1e-5 of the largest entry, as for the existing loss."""
    _, res, opts = CASES[name]
    a, b, _ = case_data(name)
    fn = D.losses.SumAndDifferenceSTFTLoss(**res_kw(res), output="full", **W, **pkg_opts(opts))
    outs = []
    for _ in range(2):
        pt, tt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        full = fn(pt, tt)
        full[0].backward()
        outs.append((torch.stack([v.detach() for v in full]), pt.grad, tt.grad))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in (1, 2):
        assert float((outs[0][k] - outs[1][k]).abs().max()) <= 1e-5 * float(outs[0][k].abs().max())


@pytest.mark.parametrize("name", ["B", "C"])
def test_graph_replay(D, name):
    """Forward and backward captured on one stream after an eager call (twiddles, taps and mel tables are then built inside the capture,
    as kernel nodes) and replayed on new data in the same buffers: the loss equals the eager value (fixed-order sums), the gradients agree
    to 1e-5 of the largest entry (float atomics: order only)."""
    shape, res, opts = CASES[name]
    fn = D.losses.SumAndDifferenceSTFTLoss(**res_kw(res), **W, **pkg_opts(opts))
    g = torch.Generator(device=DEV).manual_seed(13)
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


def test_errors(D):
    fn = D.losses.SumAndDifferenceSTFTLoss((64,), (16,), (64,))
    for chs in (1, 3):
        x = torch.rand(2, chs, 1000, device=DEV)
        with pytest.raises(ValueError, match=rf"Input must be stereo: {chs} channel\(s\)\."):
            fn(x, x)
    with pytest.raises(RuntimeError, match="same shape"):
        fn(torch.rand(2, 2, 1000, device=DEV), torch.rand(2, 2, 999, device=DEV))
    with pytest.raises(RuntimeError, match="same shape"):
        fn(torch.rand(2, 2, 1000, device=DEV), torch.rand(1, 2, 1000, device=DEV))
    from dasp_pytorch_amd._lib import DaspHipError
    with pytest.raises(DaspHipError):
        D.losses.SumAndDifferenceSTFTLoss((16384,), (4096,), (16384,))(torch.rand(1, 2, 40000, device=DEV), torch.rand(1, 2, 40000, device=DEV))
