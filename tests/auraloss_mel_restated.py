"""auraloss 0.4.0's STFTLoss.forward with scale="mel" (and MelSTFTLoss, which is that call), restated in float64 on top of
tests/auraloss_restated.py: per resolution the magnitudes |X| = sqrt(max(re^2 + im^2, eps)) are projected with the mel filterbank,
M = W |X| (no clamp after the projection), and the three terms run over rows x frames x n_bins:
  w_sc ||M_T - M_P||_F / ||M_T||_F + w_log_mag mean|log M_P - log M_T| + w_lin_mag mean|M_P - M_T|,
a term with weight 0 not computed; the mean over resolutions; with taps, both signals through the A-weighting FIR first. W is the
package's float32 filterbank (losses.mel_filterbank, librosa.filters.mel restated) widened to float64 - the same convention as the
A-weighting taps. Autograd gives the gradients for both arguments."""
import numpy as np
import torch

from dasp_pytorch_amd import losses
from tests.auraloss_restated import fir_same, stft_mag


def mel_mag(v, n_fft, hop, win, sample_rate, n_bins, eps=1e-8):
    """(rows, n_bins, frames): W @ |STFT(v)|."""
    W = torch.from_numpy(np.asarray(losses.mel_filterbank(sample_rate, n_fft, n_bins), dtype=np.float64)).to(v.dtype)
    return torch.matmul(W, stft_mag(v, n_fft, hop, win, eps))


def mel_mrstft_loss(p, t, resolutions, sample_rate, n_bins, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, taps=None, eps=1e-8):
    if taps is not None:
        p, t = fir_same(p, taps), fir_same(t, taps)
    total = 0.0
    for n_fft, hop, win in resolutions:
        P, T = mel_mag(p, n_fft, hop, win, sample_rate, n_bins, eps), mel_mag(t, n_fft, hop, win, sample_rate, n_bins, eps)
        term = 0.0
        if w_sc:
            term = term + w_sc * torch.linalg.norm(T - P) / torch.linalg.norm(T)
        if w_log_mag:
            term = term + w_log_mag * (torch.log(P) - torch.log(T)).abs().mean()
        if w_lin_mag:
            term = term + w_lin_mag * (P - T).abs().mean()
        total = total + term
    return total / len(resolutions)


def loss_and_grads(p, t, resolutions, sample_rate, n_bins, **kw):
    """(loss, d loss / d p, d loss / d t) as float / numpy float64, p and t numpy arrays."""
    pc = torch.from_numpy(np.asarray(p, dtype=np.float64)).requires_grad_(True)
    tc = torch.from_numpy(np.asarray(t, dtype=np.float64)).requires_grad_(True)
    loss = mel_mrstft_loss(pc, tc, resolutions, sample_rate, n_bins, **kw)
    loss.backward()
    return float(loss.detach()), pc.grad.numpy(), tc.grad.numpy()
