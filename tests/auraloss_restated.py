"""auraloss 0.4.0's MultiResolutionSTFTLoss with the term weights w_sc / w_log_mag / w_lin_mag and perceptual_weighting, restated on
CPU torch.stft (center=True, reflect padding, periodic Hann window zero-padded to n_fft) + conv1d in float64, with autograd for both
arguments: the yardstick of tests/test_gpu_mrstft_options.py (auraloss is not a dependency; freq.py and perceptual.py of 0.4.0 restated).
Per resolution  w_sc ||T| - |P||_F / ||T||_F + w_log_mag mean|log|P| - log|T|| + w_lin_mag mean||P| - |T||, |.| = sqrt(max(re^2 + im^2,
eps)), a term with weight 0 not computed; the mean over resolutions. The A-weighting taps are the package's float32 taps widened to
float64, applied as conv1d(x, h, padding=50) to both signals row by row."""
import numpy as np
import torch
import torch.nn.functional as F


def fir_same(x, taps):
    """y[n] = sum_k h[k] x[n + k - K/2], zeros outside [0, N): conv1d with padding K // 2, over the last axis of x (in x's dtype)."""
    h = torch.as_tensor(np.asarray(taps, dtype=np.float64)).to(x.dtype)
    K = h.numel()
    v = x.reshape(-1, 1, x.shape[-1])
    return F.conv1d(v, h.view(1, 1, K), padding=K // 2).reshape(x.shape)


def fir_same_adjoint(g, taps):
    """The adjoint of fir_same: conv_transpose1d with the same taps and padding."""
    h = torch.as_tensor(np.asarray(taps, dtype=np.float64)).to(g.dtype)
    K = h.numel()
    v = g.reshape(-1, 1, g.shape[-1])
    return F.conv_transpose1d(v, h.view(1, 1, K), padding=K // 2).reshape(g.shape)


def stft_mag(v, n_fft, hop, win, eps=1e-8):
    w = torch.hann_window(win, dtype=v.dtype)
    S = torch.stft(v.reshape(-1, v.shape[-1]), n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
    return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=eps))


def mrstft_loss(p, t, resolutions, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, taps=None, eps=1e-8):
    """p, t: (..., N) float64 tensors (requires_grad as the caller wishes); taps: None or the A-weighting taps."""
    if taps is not None:
        p, t = fir_same(p, taps), fir_same(t, taps)
    total = 0.0
    for n_fft, hop, win in resolutions:
        P, T = stft_mag(p, n_fft, hop, win, eps), stft_mag(t, n_fft, hop, win, eps)
        term = 0.0
        if w_sc:
            term = term + w_sc * torch.linalg.norm(T - P) / torch.linalg.norm(T)
        if w_log_mag:
            term = term + w_log_mag * (torch.log(P) - torch.log(T)).abs().mean()
        if w_lin_mag:
            term = term + w_lin_mag * (P - T).abs().mean()
        total = total + term
    return total / len(resolutions)


def loss_and_grads(p, t, resolutions, **kw):
    """(loss, d loss / d p, d loss / d t) as float / numpy float64, p and t numpy arrays."""
    pc = torch.from_numpy(np.asarray(p, dtype=np.float64)).requires_grad_(True)
    tc = torch.from_numpy(np.asarray(t, dtype=np.float64)).requires_grad_(True)
    loss = mrstft_loss(pc, tc, resolutions, **kw)
    loss.backward()
    return float(loss.detach()), pc.grad.numpy(), tc.grad.numpy()


# the loss of the reference's examples/auto_eq.py:252-262 and examples/virtual_analog.py:288-298 (identical arguments)
EXAMPLE_RESOLUTIONS = tuple((1 << k, 1 << (k - 1), 1 << k) for k in range(7, 14))
EXAMPLE_KW = dict(w_sc=0.0, w_log_mag=1.0, w_lin_mag=1.0)
