"""Host side of the MR-STFT loss options (auraloss 0.4.0's keywords, dasp_pytorch_amd/losses.py): the A-weighting taps, the float64
restatement the GPU tests compare against (tests/auraloss_restated.py), and argument validation - no GPU needed."""
import numpy as np
import pytest
import scipy.signal
import torch

from dasp_pytorch_amd import losses
from oracle import dasp_oracle as orc
from tests import auraloss_restated as ar

RATES = (44100, 48000, 22050, 16000)


def _bilinear_a_weighting(fs):
    f1, f2, f3, f4 = 20.598997, 107.65265, 737.86223, 12194.217
    num = [(2 * np.pi * f4) ** 2 * (10 ** (1.9997 / 20)), 0, 0, 0, 0]
    den = np.polymul([1, 4 * np.pi * f4, (2 * np.pi * f4) ** 2], [1, 4 * np.pi * f1, (2 * np.pi * f1) ** 2])
    den = np.polymul(np.polymul(den, [1, 2 * np.pi * f3]), [1, 2 * np.pi * f2])
    return scipy.signal.bilinear(num, den, fs=fs)


@pytest.mark.parametrize("fs", RATES)
def test_a_weighting_taps_are_symmetric(fs):
    h = losses.a_weighting_taps(fs)
    assert h.dtype == np.float32 and h.shape == (losses.AW_TAPS,)
    assert np.array_equal(h, h[::-1])


@pytest.mark.parametrize("fs", RATES)
def test_a_weighting_fir_follows_the_analog_curve(fs):
    """|H_fir| within 0.5 dB of the bilinear A-weighting from 500 Hz to min(10 kHz, 0.4 fs), within 0.2 dB of 0 dB at 1 kHz."""
    h = losses.a_weighting_taps(fs).astype(np.float64)
    b, a = _bilinear_a_weighting(fs)
    f = np.linspace(500.0, min(10000.0, 0.4 * fs), 400)
    _, hf = scipy.signal.freqz(h, [1.0], worN=f, fs=fs)
    _, ha = scipy.signal.freqz(b, a, worN=f, fs=fs)
    dev = np.abs(20 * np.log10(np.abs(hf) / np.abs(ha)))
    _, h1k = scipy.signal.freqz(h, [1.0], worN=[1000.0], fs=fs)
    print(f"fs {fs}: FIR vs bilinear A-weighting max {dev.max():.3f} dB, 1 kHz {20 * np.log10(abs(h1k[0])):+.3f} dB")
    assert dev.max() < 0.5
    assert abs(20 * np.log10(abs(h1k[0]))) < 0.2


@pytest.mark.parametrize("res", [((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)), ((256, 64, 200), (64, 16, 64))])
def test_restatement_is_the_oracle_at_default_weights(res):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((2, 1, 3000)) * 0.3
    b = 0.6 * a + 0.2 * rng.standard_normal(a.shape)
    got = float(ar.mrstft_loss(torch.from_numpy(a), torch.from_numpy(b), res))
    want = orc.mrstft_loss(a, b, resolutions=res)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


def test_restatement_fir_adjoint():
    """<fir_same(x), g> = <x, fir_same_adjoint(g)> on asymmetric taps (the pair the GPU FIR exports are checked against)."""
    rng = np.random.default_rng(9)
    h = rng.standard_normal(11)
    x, g = torch.from_numpy(rng.standard_normal((3, 50))), torch.from_numpy(rng.standard_normal((3, 50)))
    lhs, rhs = float((ar.fir_same(x, h) * g).sum()), float((x * ar.fir_same_adjoint(g, h)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize("name,value", [("w_phs", 0.5), ("window", "hamming_window"), ("scale", "mel"), ("n_bins", 128),
                                        ("scale_invariance", True), ("reduction", "none"), ("mag_distance", "L2"), ("output", "full")])
def test_options_not_implemented_name_themselves(name, value):
    with pytest.raises(NotImplementedError, match=name):
        losses.MultiResolutionSTFTLoss(**{name: value})
    with pytest.raises(NotImplementedError, match=name):
        losses.STFTLoss(**{name: value})
    with pytest.raises(NotImplementedError, match=name):
        losses.mrstft_loss(torch.zeros(1, 1, 4000), torch.zeros(1, 1, 4000), **{name: value})


def test_perceptual_weighting_needs_a_sample_rate():
    with pytest.raises(ValueError, match="sample_rate"):
        losses.MultiResolutionSTFTLoss(perceptual_weighting=True)
    with pytest.raises(ValueError, match="sample_rate"):
        losses.STFTLoss(perceptual_weighting=True)
    with pytest.raises(ValueError, match="sample_rate"):
        losses.mrstft_loss(torch.zeros(1, 1, 4000), torch.zeros(1, 1, 4000), perceptual_weighting=True)


def test_unknown_keywords_and_extra_positionals_are_type_errors():
    with pytest.raises(TypeError, match="w_foo"):
        losses.MultiResolutionSTFTLoss(w_foo=1.0)
    with pytest.raises(TypeError):
        losses.STFTLoss(1024, 256, 1024, 1e-8, 1.0)
    with pytest.raises(TypeError):
        losses.MultiResolutionSTFTLoss((1024,), (256,), (1024,), 1e-8, "hann_window")


def test_keywords_and_their_defaults():
    """auraloss's defaults are carried as None (weights (1, 1, 0), no sample rate); `device` is accepted and ignored; the 4th positional
    argument is still eps; the examples' configuration is carried as (w_sc, w_log_mag, w_lin_mag, sample_rate)."""
    fn = losses.MultiResolutionSTFTLoss(w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, w_phs=0.0, sample_rate=None, scale=None, n_bins=None,
                                        perceptual_weighting=False, scale_invariance=False, window="hann_window", reduction="mean",
                                        mag_distance="L1", output="loss", device="cuda:3")
    assert fn._opts is None
    assert losses.MultiResolutionSTFTLoss(sample_rate=44100)._opts is None
    assert losses.MultiResolutionSTFTLoss((1024,), (256,), (1024,), 1e-7).eps == 1e-7
    ex = losses.MultiResolutionSTFTLoss(**ar.EXAMPLE_KW, w_phs=0.0, perceptual_weighting=True, sample_rate=44100)
    assert ex._opts == (0.0, 1.0, 1.0, 44100.0)
    assert losses.STFTLoss(w_lin_mag=2)._opts == (1.0, 1.0, 2.0, None)
    with pytest.raises(ValueError):
        losses.MultiResolutionSTFTLoss(w_sc=float("nan"))
