"""auraloss.time 0.4.0 restated in float64 torch on the CPU, with autograd for the gradients: the reference of tests/test_gpu_time_losses.py
(auraloss is not installed with the project). Formulas per row - one (batch, channel) pair of N samples, sums over the last axis, input p,
target t:

    esr       sum (t - p)^2 / (sum t^2 + eps)
    dc        mean(t - p)^2 / (mean(t^2) + eps)
    log_cosh  mean(log(cosh(a (p - t)) + eps) / a)
    snr       -10 log10(sum t^2 / (sum (p - t)^2 + eps) + eps)
    si_sdr    alpha = sum p t / (sum t^2 + eps);  -10 log10(sum (alpha t)^2 / (sum (p - alpha t)^2 + eps) + eps)
    sd_sdr    same alpha;                         -10 log10(sum (alpha t)^2 / (sum (p - t)^2 + eps) + eps)
    mse       mean (p - t)^2

snr, si_sdr and sd_sdr with zero_mean=True: both signals minus their row means first. reduction "mean" / "sum" over the rows, "none" the
per-row values shaped input.shape[:-1]."""
import numpy as np
import torch

TERMS = ("esr", "dc", "log_cosh", "snr", "si_sdr", "sd_sdr", "mse")
DB_TERMS = ("snr", "si_sdr", "sd_sdr")


def _centre(p, t, zero_mean):
    if zero_mean:
        return p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    return p, t


def esr(p, t, eps=1e-8, **_):
    return ((t - p) ** 2).sum(-1) / ((t ** 2).sum(-1) + eps)


def dc(p, t, eps=1e-8, **_):
    return (t - p).mean(-1) ** 2 / ((t ** 2).mean(-1) + eps)


def log_cosh(p, t, a=1.0, eps=1e-8, **_):
    return (torch.log(torch.cosh(a * (p - t)) + eps) / a).mean(-1)


def snr(p, t, zero_mean=True, eps=1e-8, **_):
    p, t = _centre(p, t, zero_mean)
    return -10.0 * torch.log10((t ** 2).sum(-1) / (((p - t) ** 2).sum(-1) + eps) + eps)


def si_sdr(p, t, zero_mean=True, eps=1e-8, **_):
    p, t = _centre(p, t, zero_mean)
    alpha = ((p * t).sum(-1) / ((t ** 2).sum(-1) + eps)).unsqueeze(-1)
    return -10.0 * torch.log10(((alpha * t) ** 2).sum(-1) / (((p - alpha * t) ** 2).sum(-1) + eps) + eps)


def sd_sdr(p, t, zero_mean=True, eps=1e-8, **_):
    p, t = _centre(p, t, zero_mean)
    alpha = ((p * t).sum(-1) / ((t ** 2).sum(-1) + eps)).unsqueeze(-1)
    return -10.0 * torch.log10(((alpha * t) ** 2).sum(-1) / (((p - t) ** 2).sum(-1) + eps) + eps)


def mse(p, t, **_):
    return ((p - t) ** 2).mean(-1)


_FN = {"esr": esr, "dc": dc, "log_cosh": log_cosh, "snr": snr, "si_sdr": si_sdr, "sd_sdr": sd_sdr, "mse": mse}


def rows_loss(p, t, weights, a=1.0, zero_mean=True, eps=1e-8):
    """The weighted per-row loss, shaped p.shape[:-1]. weights: {term: weight}; a term with weight 0 is not evaluated."""
    out = 0.0
    for name, w in weights.items():
        if w != 0:
            out = out + w * _FN[name](p, t, a=a, zero_mean=zero_mean, eps=eps)
    return out


def reduce(v, reduction):
    return v.mean() if reduction == "mean" else v.sum() if reduction == "sum" else v


def loss_and_grads(p, t, weights, a=1.0, zero_mean=True, eps=1e-8, reduction="mean", upstream=None):
    """(loss, d/d input, d/d target) as float64 numpy arrays. upstream: the gradient handed to backward (default: ones)."""
    pt = torch.from_numpy(np.asarray(p, dtype=np.float64)).clone().requires_grad_(True)
    tt = torch.from_numpy(np.asarray(t, dtype=np.float64)).clone().requires_grad_(True)
    loss = reduce(rows_loss(pt, tt, weights, a=a, zero_mean=zero_mean, eps=eps), reduction)
    up = torch.ones_like(loss) if upstream is None else torch.from_numpy(np.asarray(upstream, dtype=np.float64)).reshape(loss.shape)
    loss.backward(up)
    return loss.detach().numpy(), pt.grad.numpy(), tt.grad.numpy()
