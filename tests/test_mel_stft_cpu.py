"""Host side of the mel-scaled STFT losses (scale="mel" / n_bins / MelSTFTLoss, dasp_pytorch_amd/losses.py): the filterbank against an
independent restatement of librosa.filters.mel and its structural properties (what the kernels' table relies on), the options and
their errors, and the size queries of the new exports - no GPU needed."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from dasp_pytorch_amd import _lib, losses

# every (sample_rate, n_fft, n_bins) the GPU tests of tests/test_gpu_mel_stft.py run or build a table for
GPU_CONFIGS = [(44100, 8, 2), (44100, 64, 8), (44100, 256, 8), (44100, 512, 40), (44100, 1024, 40), (44100, 2048, 40), (44100, 4096, 128),
               (44100, 1024, 128), (44100, 2048, 128), (44100, 8192, 128), (16000, 512, 40), (48000, 1024, 128), (44100, 8192, 256)]
LOOP_CONFIGS = [(44100, 8, 2), (44100, 64, 8), (16000, 512, 40), (48000, 1024, 128), (44100, 2048, 128), (22050, 512, 64)]


def _mel(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _hz(m):
    return (200.0 / 3.0) * m if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def _edges(sr, n_mels):
    top = _mel(sr / 2.0)
    return [_hz(top * n / (n_mels + 1)) for n in range(n_mels + 2)]


def _double_loop(sr, n_fft, n_mels):
    """librosa.filters.mel(sr, n_fft, n_mels) (fmin=0, fmax=sr/2, htk=False, norm="slaney") written out bin by bin with scalar math."""
    e = _edges(sr, n_mels)
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            up, down = (f - e[m]) / (e[m + 1] - e[m]), (e[m + 2] - f) / (e[m + 2] - e[m + 1])
            W[m, k] = max(0.0, min(up, down)) * 2.0 / (e[m + 2] - e[m])
    return W


@pytest.mark.parametrize("sr,n_fft,n_mels", LOOP_CONFIGS)
def test_filterbank_is_the_double_loop_restatement(sr, n_fft, n_mels):
    """Elementwise within one float32 ulp. The two sides round their fp64 edges independently (numpy against math, a linspace against
    n / (B + 1)): a few fp64 ulps of an edge frequency, < 1e-10 of a row's peak in a weight - far below a float32 ulp of the peak, but
    not of a weight that is itself tiny next to its filter's foot, so that much is allowed on top of the ulp."""
    W = losses.mel_filterbank(sr, n_fft, n_mels)
    want = _double_loop(sr, n_fft, n_mels)
    assert W.shape == (n_mels, n_fft // 2 + 1) and W.dtype == np.float32 and not W.flags.writeable
    assert (W >= 0).all()
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.maximum(W, w32))
    slack = 1e-10 * want.max(axis=1, keepdims=True)
    err = np.abs(W.astype(np.float64) - want)
    assert (err <= ulp + slack).all(), float((err - ulp - slack).max())
    assert np.array_equal(W > 0, w32 > 0) or float(np.abs(W - w32)[(W > 0) != (w32 > 0)].max()) < 1e-10 * float(want.max())
    assert losses.mel_filterbank(sr, n_fft, n_mels) is W                       # lru_cache


def test_mel_scale_anchors():
    assert float(losses.hz_to_mel(1000.0)) == 15.0 and float(losses.mel_to_hz(15.0)) == 1000.0
    assert abs(float(losses.hz_to_mel(6400.0)) - 42.0) < 1e-12 and abs(float(losses.mel_to_hz(42.0)) - 6400.0) < 1e-8
    assert float(losses.hz_to_mel(0.0)) == 0.0 and abs(float(losses.hz_to_mel(500.0)) - 7.5) < 1e-14
    for sr, n in ((44100, 128), (16000, 40)):
        e = losses.mel_edges(sr, n)
        assert e.shape == (n + 2,) and e.dtype == np.float64 and e[0] == 0.0 and abs(e[-1] - sr / 2) < 1e-9 * sr
        assert (np.diff(e) > 0).all()
        assert np.allclose(e, _edges(sr, n), rtol=1e-14, atol=0)


@pytest.mark.parametrize("sr,n_fft,n_mels", GPU_CONFIGS + [(44100, 512, 128)])
def test_filterbank_structure(sr, n_fft, n_mels):
    """What the device table relies on: every filter's support is one run of bins, every bin lies in at most two filters and those are
    neighbours, and no weight exceeds the Slaney peak 2 / (e[m+2] - e[m])."""
    W = losses.mel_filterbank(sr, n_fft, n_mels)
    e = losses.mel_edges(sr, n_mels)
    nz = W > 0
    for m in range(n_mels):
        k = np.flatnonzero(nz[m])
        assert k.size == 0 or k[-1] - k[0] + 1 == k.size, m
    per_bin = nz.sum(axis=0)
    assert per_bin.max() <= 2
    for k in np.flatnonzero(per_bin == 2):
        m = np.flatnonzero(nz[:, k])
        assert m[1] == m[0] + 1
    assert (W.max(axis=1).astype(np.float64) <= 2.0 / (e[2:] - e[:-2]) * (1 + 2.0 ** -23)).all()


def test_empty_filters():
    """A filter narrower than the bin spacing is an all-zero row: 11 of 128 at 44.1 kHz with 512-point frames, none with 1024; none in
    any configuration the GPU tests use."""
    assert int((~losses.mel_filterbank(44100, 512, 128).any(axis=1)).sum()) == 11
    assert losses.mel_filterbank(44100, 1024, 128).any(axis=1).all()
    for cfg in GPU_CONFIGS:
        assert losses.mel_filterbank(*cfg).any(axis=1).all(), cfg


def test_functional_combinations_construct():
    fn = losses.MultiResolutionSTFTLoss((1024, 2048, 8192), (256, 512, 2048), (1024, 2048, 8192), scale="mel", n_bins=128, sample_rate=44100,
                                        perceptual_weighting=True)
    assert fn._mel == (128, 44100.0) and fn._opts == (1.0, 1.0, 0.0, 44100.0)
    fn = losses.STFTLoss(scale="mel", n_bins=64, sample_rate=48000)
    assert fn._mel == (64, 48000.0) and fn._opts is None
    fn = losses.STFTLoss(512, 128, 512, scale="mel", n_bins=40, sample_rate=16000, w_sc=0.0, w_log_mag=0.5, w_lin_mag=2.0)
    assert fn._mel == (40, 16000.0) and fn._opts == (0.0, 0.5, 2.0, None)
    assert losses.MultiResolutionSTFTLoss()._mel is None and losses.MultiResolutionSTFTLoss(sample_rate=44100)._mel is None
    assert losses.STFTLoss(8, 4, 8, scale="mel", n_bins=5, sample_rate=44100, w_log_mag=0.0)._mel == (5, 44100.0)     # n_bins = n_fft / 2 + 1


def test_mel_stft_loss_signature():
    """auraloss.freq.MelSTFTLoss's parameters, in order, with its defaults."""
    sig = inspect.signature(losses.MelSTFTLoss.__init__)
    names = [n for n in sig.parameters if n != "self"]
    assert names == ["sample_rate", "fft_size", "hop_size", "win_length", "window", "w_sc", "w_log_mag", "w_lin_mag", "w_phs", "n_mels", "kwargs"]
    defaults = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(fft_size=1024, hop_size=256, win_length=1024, window="hann_window", w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, w_phs=0.0,
                            n_mels=128)
    assert sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    fn = losses.MelSTFTLoss(44100)
    assert isinstance(fn, losses.STFTLoss) and fn.resolutions == ((1024, 256, 1024),) and fn._mel == (128, 44100.0) and fn._opts is None
    fn = losses.MelSTFTLoss(48000, 2048, 512, 2048, "hann_window", 0.0, 1.0, 1.0, 0.0, 64, perceptual_weighting=True, eps=1e-7)
    assert fn.resolutions == ((2048, 512, 2048),) and fn._mel == (64, 48000.0) and fn._opts == (0.0, 1.0, 1.0, 48000.0) and fn.eps == 1e-7
    with pytest.raises(TypeError):
        losses.MelSTFTLoss()
    with pytest.raises(NotImplementedError, match="window"):
        losses.MelSTFTLoss(44100, window="hamming_window")
    with pytest.raises(NotImplementedError, match="w_phs"):
        losses.MelSTFTLoss(44100, w_phs=0.1)
    with pytest.raises(NotImplementedError, match="n_bins"):
        losses.MelSTFTLoss(44100, n_mels=300)


def _each_interface(**kw):
    yield lambda: losses.MultiResolutionSTFTLoss(**kw)
    yield lambda: losses.STFTLoss(**kw)
    yield lambda: losses.mrstft_loss(torch.zeros(1, 1, 4000), torch.zeros(1, 1, 4000), **kw)


@pytest.mark.parametrize("kw,name", [(dict(scale="mel"), "scale"), (dict(scale="mel", n_bins=64), "scale"), (dict(scale="mel", sample_rate=44100), "scale"),
                                     (dict(n_bins=64), "n_bins"), (dict(n_bins=64, sample_rate=44100), "n_bins"),
                                     (dict(scale="chroma", n_bins=12, sample_rate=44100), "scale"), (dict(scale="chroma"), "scale"),
                                     (dict(scale="mel", n_bins=64, sample_rate=44100, scale_invariance=True), "scale_invariance"),
                                     (dict(scale="mel", n_bins=64, sample_rate=44100, mag_distance="L2"), "mag_distance"),
                                     (dict(scale="mel", n_bins=64, sample_rate=44100, reduction="sum"), "reduction"),
                                     (dict(scale="mel", n_bins=64, sample_rate=44100, output="full"), "output"),
                                     (dict(scale="mel", n_bins=0, sample_rate=44100), "n_bins"), (dict(scale="mel", n_bins=257, sample_rate=44100), "n_bins"),
                                     (dict(scale="mel", n_bins=-3, sample_rate=44100), "n_bins"), (dict(scale="mel", n_bins=64.5, sample_rate=44100), "n_bins")])
def test_cases_that_raise_name_the_option(kw, name):
    for make in _each_interface(**kw):
        with pytest.raises(NotImplementedError, match=name):
            make()


def test_n_bins_above_the_bin_count_of_a_resolution():
    with pytest.raises(NotImplementedError, match="n_bins"):
        losses.MultiResolutionSTFTLoss((1024, 64), (256, 16), (1024, 64), scale="mel", n_bins=40, sample_rate=44100, w_log_mag=0.0)
    with pytest.raises(NotImplementedError, match="n_bins"):
        losses.STFTLoss(8, 4, 8, scale="mel", n_bins=6, sample_rate=44100, w_log_mag=0.0)


def test_empty_filters_are_refused_with_the_log_term():
    """auraloss's default resolutions with 128 bins at 44.1 kHz: the 512-point frames leave 11 filters empty (log 0 - log 0 = NaN in
    auraloss) - a ValueError at construction that names the n_fft and the count; allowed with w_log_mag = 0."""
    kw = dict(scale="mel", n_bins=128, sample_rate=44100)
    z = torch.zeros(1, 1, 4000)
    for make in (lambda: losses.MultiResolutionSTFTLoss(**kw), lambda: losses.mrstft_loss(z, z, **kw), lambda: losses.STFTLoss(512, 128, 512, **kw),
                 lambda: losses.MelSTFTLoss(44100, 512, 128, 512)):
        with pytest.raises(ValueError, match=r"n_fft=512.*11 of the 128.*NaN"):
            make()
    losses.STFTLoss(**kw)                                          # 1024-point frames: no empty filter
    fn = losses.MultiResolutionSTFTLoss(scale="mel", n_bins=128, sample_rate=44100, w_log_mag=0.0, w_lin_mag=1.0)
    assert fn._mel == (128, 44100.0) and fn._opts == (1.0, 0.0, 1.0, None)
    losses.STFTLoss(512, 128, 512, scale="mel", n_bins=128, sample_rate=44100, w_log_mag=0)


def test_size_queries_of_the_mel_exports():
    L = _lib.lib()
    arr = lambda *v: (ctypes.c_int * len(v))(*v)
    q = L.dasp_mrstft_partial_floats                                                    # the last argument: n_bins, 0 for linear bins
    assert q(4, 20000, 3, arr(1024, 2048, 8192), arr(256, 512, 2048), arr(1024, 2048, 8192), 128) == \
        q(4, 20000, 3, arr(1024, 2048, 8192), arr(256, 512, 2048), arr(1024, 2048, 8192), 0) > 0
    assert q(1, 200, 1, arr(8), arr(4), arr(8), 5) > 0                                  # n_bins = n_fft / 2 + 1
    assert q(1, 200, 1, arr(8), arr(4), arr(8), 6) == -1                                # more filters than bins
    assert q(1, 20000, 1, arr(1024), arr(256), arr(1024), -1) == -1                     # 0 filters is the linear-bin query; fewer are refused
    assert q(1, 20000, 1, arr(1024), arr(256), arr(1024), 257) == -1
    assert q(1, 20000, 2, arr(1024, 64), arr(256, 16), arr(1024, 64), 40) == -1         # one resolution too short for 40 filters
    assert q(1, 20000, 1, arr(1000), arr(256), arr(1000), 40) == -1                     # not a power of two
    assert q(1, 40000, 1, arr(16384), arr(4096), arr(16384), 40) == -1
    assert q(1, 20000, 1, arr(1024), arr(256), arr(2048), 40) == -1                     # win > fft
    assert q(1, 400, 1, arr(1024), arr(256), arr(1024), 40) == -1                       # fft / 2 >= N
    assert q(1, 20000, 9, arr(*[64] * 9), arr(*[16] * 9), arr(*[64] * 9), 8) == -1
    assert L.dasp_mel_table_floats(1024, 128) == 3 * 513 + 2 * 128
    assert L.dasp_mel_table_floats(8192, 256) == 3 * 4097 + 2 * 256
    for bad in ((1024, 0), (1024, 257), (8, 6), (1000, 40), (16384, 128), (4, 2)):
        assert L.dasp_mel_table_floats(*bad) == -1
    assert L.dasp_mrstft_forward(None, None, None, None, None, None, None, 1, 4096, 1, arr(1024), arr(256), arr(1024), 1e-8, 1.0, 1.0, 0.0, 64, None) == -1
    assert L.dasp_mel_table_store(None, None, 44100.0, 1024, 64, None) == -1
