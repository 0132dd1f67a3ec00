"""auraloss 0.4.0's SumAndDifferenceSTFTLoss restated in float64 on top of tests/auraloss_restated.py and tests/auraloss_mel_restated.py
(auraloss is not a dependency): for (bs, 2, N) signals
  s(x) = x[:, 0] + x[:, 1],  d(x) = x[:, 0] - x[:, 1]                       each (bs, 1, N)
  sum_loss = MRSTFT(s(input), s(target)),  diff_loss = MRSTFT(d(input), d(target)),  loss = (w_sum sum_loss + w_diff diff_loss) / 2,
two separate multi-resolution losses: each has its own spectral-convergence ratio and its own means over the bs rows of its half. With
taps, the A-weighting FIR is applied inside each MRSTFT, to the sum and the difference signals, as auraloss does. n_bins selects the
mel-scaled form. Autograd gives the gradients for both arguments; `backward` picks the value that is differentiated ("loss", "sum",
"diff"), for the check that each half has its own upstream gradient. `dtype` float32 runs the same statement in single precision (the
float32 restatement error quoted by the GPU tests)."""
import numpy as np
import torch

from tests import auraloss_mel_restated as amr
from tests import auraloss_restated as ar


def sum_diff(x):
    return x[:, 0:1] + x[:, 1:2], x[:, 0:1] - x[:, 1:2]


def losses(p, t, resolutions, w_sum=1.0, w_diff=1.0, sample_rate=None, n_bins=None, **kw):
    """(loss, sum_loss, diff_loss) as tensors; p, t: (bs, 2, N) tensors. kw: w_sc, w_log_mag, w_lin_mag, taps, eps."""
    if p.dim() != 3 or p.shape[1] != 2:
        raise ValueError(f"Input must be stereo: {p.shape[1]} channel(s).")
    (ps, pd), (ts, td) = sum_diff(p), sum_diff(t)
    if n_bins is None:
        sum_loss, diff_loss = ar.mrstft_loss(ps, ts, resolutions, **kw), ar.mrstft_loss(pd, td, resolutions, **kw)
    else:
        sum_loss = amr.mel_mrstft_loss(ps, ts, resolutions, sample_rate, n_bins, **kw)
        diff_loss = amr.mel_mrstft_loss(pd, td, resolutions, sample_rate, n_bins, **kw)
    return (w_sum * sum_loss + w_diff * diff_loss) / 2, sum_loss, diff_loss


def loss_and_grads(p, t, resolutions, backward="loss", dtype=torch.float64, **kw):
    """(loss, sum_loss, diff_loss, d/d input, d/d target) as floats / numpy float64 arrays, p and t numpy arrays; the gradients are those
    of `backward`: "loss", "sum" or "diff"."""
    pc = torch.from_numpy(np.asarray(p, dtype=np.float64)).to(dtype).requires_grad_(True)
    tc = torch.from_numpy(np.asarray(t, dtype=np.float64)).to(dtype).requires_grad_(True)
    out = losses(pc, tc, resolutions, **kw)
    out[("loss", "sum", "diff").index(backward)].backward()
    zero = lambda x: (x.grad if x.grad is not None else torch.zeros_like(x)).double().numpy()
    return float(out[0].detach()), float(out[1].detach()), float(out[2].detach()), zero(pc), zero(tc)
