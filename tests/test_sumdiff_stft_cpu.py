"""Host side of SumAndDifferenceSTFTLoss (dasp_pytorch_amd/losses.py): its signature and the options it takes and refuses, the size
queries and null-pointer refusals of the dasp_mrstft_sd_* exports, and three properties of the float64 restatement the GPU tests compare
against (tests/auraloss_sumdiff_restated.py) - no GPU needed."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from dasp_pytorch_amd import _lib, losses
from tests import auraloss_sumdiff_restated as sdr

R = dict(fft_sizes=(1024, 2048), hop_sizes=(256, 512), win_lengths=(1024, 2048))


def test_signature_and_defaults():
    sig = inspect.signature(losses.SumAndDifferenceSTFTLoss.__init__)
    names = list(sig.parameters)
    assert names == ["self", "fft_sizes", "hop_sizes", "win_lengths", "window", "w_sum", "w_diff", "output", "kwargs"]
    for n in ("fft_sizes", "hop_sizes", "win_lengths"):
        assert sig.parameters[n].default is inspect.Parameter.empty
    assert [sig.parameters[n].default for n in ("window", "w_sum", "w_diff", "output")] == ["hann_window", 1.0, 1.0, "loss"]
    with pytest.raises(TypeError):
        losses.SumAndDifferenceSTFTLoss()
    fn = losses.SumAndDifferenceSTFTLoss(**R)
    assert (fn.w_sum, fn.w_diff, fn.output, fn.eps) == (1.0, 1.0, "loss", 1e-8) and fn._opts is None and fn._mel is None
    assert fn.resolutions == ((1024, 256, 1024), (2048, 512, 2048))
    fsig = inspect.signature(losses.sum_and_difference_stft_loss)
    assert list(fsig.parameters) == ["input", "target", "fft_sizes", "hop_sizes", "win_lengths", "eps", "w_sum", "w_diff", "output", "options"]
    assert [fsig.parameters[n].default for n in ("eps", "w_sum", "w_diff", "output")] == [1e-8, 1.0, 1.0, "loss"]
    with pytest.raises(ValueError, match="same length"):
        losses.SumAndDifferenceSTFTLoss((1024,), (256, 512), (1024,))


def test_accepted_options_are_those_of_the_mono_loss():
    fn = losses.SumAndDifferenceSTFTLoss(**R, w_sum=0.7, w_diff=1.3, output="full", w_sc=0.0, w_log_mag=1.0, w_lin_mag=1.0,
                                         perceptual_weighting=True, sample_rate=44100, eps=1e-7, device="cpu")
    mono = losses.MultiResolutionSTFTLoss(**R, w_sc=0.0, w_log_mag=1.0, w_lin_mag=1.0, perceptual_weighting=True, sample_rate=44100)
    assert fn._opts == mono._opts == (0.0, 1.0, 1.0, 44100.0) and fn.eps == 1e-7 and fn.output == "full"
    fn = losses.SumAndDifferenceSTFTLoss(**R, scale="mel", n_bins=128, sample_rate=44100, perceptual_weighting=True)
    mono = losses.MultiResolutionSTFTLoss(**R, scale="mel", n_bins=128, sample_rate=44100, perceptual_weighting=True)
    assert fn._mel == mono._mel == (128, 44100.0) and fn._opts == mono._opts


@pytest.mark.parametrize("name,value", [("w_phs", 0.5), ("scale", "chroma"), ("n_bins", 64), ("scale_invariance", True), ("reduction", "sum"),
                                        ("mag_distance", "L2"), ("output", "bogus"), ("window", "hamming_window")])
def test_refused_options_name_themselves(name, value):
    x = torch.zeros(1, 2, 4096)
    for make in (lambda: losses.SumAndDifferenceSTFTLoss(**R, **{name: value}),
                 lambda: losses.sum_and_difference_stft_loss(x, x, **R, **{name: value})):
        with pytest.raises(NotImplementedError, match=name):
            make()


def test_option_errors_match_the_mono_loss():
    with pytest.raises(ValueError, match="sample_rate"):
        losses.SumAndDifferenceSTFTLoss(**R, perceptual_weighting=True)
    with pytest.raises(TypeError, match="no_such_option"):
        losses.SumAndDifferenceSTFTLoss(**R, no_such_option=1)
    with pytest.raises(ValueError, match="finite"):
        losses.SumAndDifferenceSTFTLoss(**R, w_sc=float("nan"))
    # mel validation: the same refusals as MultiResolutionSTFTLoss, for the same reasons
    for kw, exc in ((dict(scale="mel", n_bins=128), NotImplementedError),                       # no sample rate
                    (dict(scale="mel", sample_rate=44100), NotImplementedError),                # no n_bins
                    (dict(scale="mel", n_bins=257, sample_rate=44100), NotImplementedError),
                    (dict(scale="mel", n_bins=2.5, sample_rate=44100), NotImplementedError),
                    (dict(scale="mel", n_bins=128, sample_rate=-1.0), ValueError)):
        for cls in (losses.MultiResolutionSTFTLoss, losses.SumAndDifferenceSTFTLoss):
            with pytest.raises(exc):
                cls(**R, **kw)
    for cls in (losses.MultiResolutionSTFTLoss, losses.SumAndDifferenceSTFTLoss):
        with pytest.raises(ValueError, match="narrower than the bin spacing"):                  # 128 filters on 512-point frames: 11 empty rows
            cls((512,), (128,), (512,), scale="mel", n_bins=128, sample_rate=44100)
        cls((512,), (128,), (512,), scale="mel", n_bins=128, sample_rate=44100, w_log_mag=0.0)


def test_channel_count_and_shape_errors_come_before_the_device():
    fn = losses.SumAndDifferenceSTFTLoss(**R)
    for chs in (1, 3):
        with pytest.raises(ValueError, match=rf"Input must be stereo: {chs} channel\(s\)\."):
            fn(torch.zeros(2, chs, 4096), torch.zeros(2, chs, 4096))
    with pytest.raises(RuntimeError, match="same shape"):
        fn(torch.zeros(2, 2, 4096), torch.zeros(2, 2, 4095))
    with pytest.raises(_lib.DaspHipError):                                                      # stereo CPU tensors: no CPU path
        fn(torch.zeros(2, 2, 4096), torch.zeros(2, 2, 4096))


def _arr(v):
    return (ctypes.c_int * len(v))(*v)


def test_size_queries():
    """2 halves x nres x items x groups x 4, groups = the most frame groups of any resolution; 4096 / n_fft frames per group, one 8192-point frame."""
    L = _lib.lib()
    N = 20000
    fft, hop, win = (1024, 2048, 8192), (256, 512, 2048), (1024, 2048, 8192)
    groups = max(-(-(1 + N // 256) // 4), -(-(1 + N // 512) // 2), 1 + N // 2048)
    assert groups == 20
    q = L.dasp_mrstft_sd_partial_floats                         # the last argument: n_bins, 0 for linear bins
    assert q(3, N, 3, _arr(fft), _arr(hop), _arr(win), 0) == 2 * 3 * 3 * groups * 4
    assert q(3, N, 3, _arr(fft), _arr(hop), _arr(win), 128) == 2 * 3 * 3 * groups * 4
    assert q(1, 200, 1, _arr((8,)), _arr((4,)), _arr((8,)), 0) == 2 * 1 * 1 * 1 * 4          # 51 frames: one group of 512
    # twice the mono query for the 2 x items rows of the same signals
    assert q(3, N, 3, _arr(fft), _arr(hop), _arr(win), 0) == L.dasp_mrstft_partial_floats(6, N, 3, _arr(fft), _arr(hop), _arr(win), 0)
    for bad in ((3, N, 1, (1000,), (256,), (1000,)),            # not a power of two
                (3, N, 1, (16384,), (4096,), (16384,)),         # beyond 8192
                (3, N, 1, (1024,), (256,), (2048,)),            # window longer than the frame
                (3, 4000, 1, (8192,), (2048,), (8192,)),        # n_fft / 2 >= N
                (3, N, 1, (1024,), (0,), (1024,)),
                (0, N, 1, (1024,), (256,), (1024,))):
        items, n, nres, f, h, w = bad
        assert q(items, n, nres, _arr(f), _arr(h), _arr(w), 0) == -1, bad
        assert q(items, n, nres, _arr(f), _arr(h), _arr(w), 4) == -1, bad
    assert q(3, N, 9, _arr(fft * 3), _arr(hop * 3), _arr(win * 3), 0) == -1                  # more than 8 resolutions
    assert q(3, N, 1, None, None, None, 0) == -1
    assert q(3, N, 3, _arr(fft), _arr(hop), _arr(win), 257) == -1
    assert q(3, N, 1, _arr((64,)), _arr((16,)), _arr((64,)), 34) == -1               # n_bins > n_fft / 2 + 1
    assert q(3, N, 1, _arr((64,)), _arr((16,)), _arr((64,)), 33) == 2 * 3 * (-(-(1 + N // 16) // 64)) * 4


def test_null_pointers_are_refused_before_any_launch():
    """Argument order: pred, target, tw, mel_tables, then partials, stats, loss (forward) or stats, gloss, grad (backward), items, N, nres,
    fft, hop, win, eps, the three weights, n_bins, (backward: wrt_target,) stream."""
    L = _lib.lib()
    a = _arr((1024,)), _arr((256,)), _arr((1024,))
    tabs = (ctypes.c_void_p * 1)(8)
    for n_bins in (0, 8):
        assert L.dasp_mrstft_sd_forward(None, None, None, None, None, None, None, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, n_bins, None) == -1
        for wrt_target in (0, 1):
            assert L.dasp_mrstft_sd_backward(None, None, None, None, None, None, None, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, n_bins, wrt_target, None) == -1
    # non-null data pointers (never dereferenced on the host) but no table array / no items: still refused without a launch
    assert L.dasp_mrstft_sd_forward(8, 8, 8, None, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 8, None) == -1
    assert L.dasp_mrstft_sd_forward(8, 8, 8, None, 8, 8, 8, 0, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 0, None) == -1
    # for both layouts and directions: n_bins and mel_tables that disagree, and a wrt_target that is neither 0 nor 1
    for prefix in ("dasp_mrstft_", "dasp_mrstft_sd_"):
        fwd, bwd = getattr(L, prefix + "forward"), getattr(L, prefix + "backward")
        assert fwd(8, 8, 8, None, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 8, None) == -1, prefix
        assert fwd(8, 8, 8, tabs, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 0, None) == -1, prefix
        assert bwd(8, 8, 8, None, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 8, 0, None) == -1, prefix
        assert bwd(8, 8, 8, tabs, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 0, 0, None) == -1, prefix
        assert bwd(8, 8, 8, None, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 0, 2, None) == -1, prefix
        assert bwd(8, 8, 8, tabs, 8, 8, 8, 1, 4096, 1, *a, 1e-8, 1.0, 1.0, 0.0, 8, 2, None) == -1, prefix


def _draw(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape) * 0.3
    return a, 0.6 * a + 0.2 * rng.standard_normal(shape)


RES = ((64, 16, 64), (256, 64, 200))


@pytest.mark.parametrize("kw", [dict(w_lin_mag=0.5), dict(w_lin_mag=0.5, sample_rate=44100, n_bins=8)], ids=["plain", "mel"])
def test_restatement_properties(kw):
    """In float64: swapping the channels of both signals leaves the loss unchanged (the difference changes sign, the magnitudes do not);
    L == R gives diff_loss == 0.0 and R == -L gives sum_loss == 0.0 (a silent half: both magnitudes sit at the clamp)."""
    a, b = _draw((2, 2, 3000), 7)
    base = sdr.loss_and_grads(a, b, RES, w_sum=0.7, w_diff=1.3, **kw)
    swap = sdr.loss_and_grads(a[:, ::-1].copy(), b[:, ::-1].copy(), RES, w_sum=0.7, w_diff=1.3, **kw)
    assert base[0] == swap[0] and base[1] == swap[1] and base[2] == swap[2]
    assert np.array_equal(swap[3][:, ::-1], base[3]) and np.array_equal(swap[4][:, ::-1], base[4])
    assert abs(base[0] - (0.7 * base[1] + 1.3 * base[2]) / 2) < 1e-15
    same = (np.stack([a[:, 0], a[:, 0]], 1), np.stack([b[:, 0], b[:, 0]], 1))
    out = sdr.loss_and_grads(*same, RES, **kw)
    assert out[2] == 0.0 and out[1] > 0 and np.isfinite(out[3]).all()
    anti = (np.stack([a[:, 0], -a[:, 0]], 1), np.stack([b[:, 0], -b[:, 0]], 1))
    out = sdr.loss_and_grads(*anti, RES, **kw)
    assert out[1] == 0.0 and out[2] > 0 and np.isfinite(out[3]).all()
    with pytest.raises(ValueError, match=r"Input must be stereo: 3 channel\(s\)\."):
        sdr.losses(torch.zeros(1, 3, 3000), torch.zeros(1, 3, 3000), RES)


def test_restatement_halves_are_separate_losses():
    """backward="sum" differentiates sum_loss alone: its gradient is the same in both channels, that of diff_loss opposite in the two."""
    a, b = _draw((2, 2, 3000), 8)
    s = sdr.loss_and_grads(a, b, RES, backward="sum")
    d = sdr.loss_and_grads(a, b, RES, backward="diff")
    full = sdr.loss_and_grads(a, b, RES, w_sum=0.7, w_diff=1.3)
    assert np.allclose(s[3][:, 0], s[3][:, 1], rtol=0, atol=1e-18) and np.allclose(d[3][:, 0], -d[3][:, 1], rtol=0, atol=1e-18)
    assert np.allclose(full[3], (0.7 * s[3] + 1.3 * d[3]) / 2, rtol=1e-12, atol=1e-18)


def test_new_kernels_keep_their_registers_and_use_no_scratch(tmp_path):
    """The second half and the inverse transform of every mrstft_sd_* kernel run behind sd_next_phase (an empty asm dependency that keeps
    the compiler from carrying the first half's twiddles and addresses across): if a compiler change undoes that, nothing computes a
    wrong value - the kernels only lose occupancy or start to spill. So csrc/stftloss.hip is compiled to assembly with the build's flags
    and the kernels' resource records are held to the documented limits: no scratch, no spills; the 512-thread instances at most 80 VGPRs
    (three workgroups per CU), their mel backward at most 96 (two); the 1024-thread instances at most 128 (what a workgroup of 16 waves gets)."""
    import re
    import shutil
    import subprocess
    from dasp_pytorch_amd.csrc import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "stftloss.s"
    subprocess.check_call([hipcc] + build.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                                                         build.HERE + "/stftloss.hip", "-o", str(out)])
    recs = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        get = lambda key: re.search(rf"\.{key}:\s+(\S+)", block).group(1)
        recs[get("name")] = (int(get("vgpr_count")), int(get("private_segment_fixed_size")), int(get("vgpr_spill_count")))
    mine = {k: v for k, v in recs.items() if "mrstft_sd_" in k}
    assert len(mine) == 12 and len(recs) == 41, (len(mine), len(recs))
    for name, (vgprs, scratch, spills) in mine.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        if "ILi13E" in name:
            limit = 128
        elif "mel_bwd" in name:
            limit = 96
        else:
            limit = 80
        assert vgprs <= limit, (name, vgprs, limit)
