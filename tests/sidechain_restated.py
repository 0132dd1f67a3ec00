"""Restatement of functional.sidechain_compressor on the CPU: the whole chain, in two forms.

    L = block_level(key or x, "peak");   l_db = 20 log10(L + eps);   r = l_db - soft_knee(l_db);   r_s = ballistics(r)
    y = gain_curve(x, makeup_gain_db - r_s)

arith=torch.float64: the float64 definitions of tests/block_level_restated.py, tests/ballistics_restated.py and
tests/gain_curve_restated.py around the product's own static curve (functional._soft_knee_level, plain torch, here in float64), one
autograd graph - the oracle. arith=torch.float32: the composition at the kernels' arithmetic - the by-hand stages of the same files
(peak exact; the smoother's float64 recurrence rounded once; the gain in float32) joined by float32 torch for the dB stage, the adjoints
chained by hand. Its error against the float64 chain is the yardstick e32 of the composed bounds max(4 e32, floor).
"""
import numpy as np
import torch

from dasp_pytorch_amd.functional import _soft_knee_level
from tests import ballistics_restated as BR
from tests import block_level_restated as LR
from tests import gain_curve_restated as GR

CTL = ("threshold_db", "ratio", "attack_ms", "release_ms", "knee_db", "makeup_gain_db")
FLOOR = dict(y=2e-6, gx=2e-6, gkey=2e-6, **{"g_" + k: 1e-5 for k in CTL})


def _reduction(L, c, eps):
    col = lambda k: c[k].reshape(-1, 1)
    l_db = 20.0 * torch.log10(L + eps)
    return l_db - _soft_knee_level(l_db, col("threshold_db"), col("ratio"), col("knee_db"))


def forward_backward(x, sr, ctl, w, key=None, hop=64, eps=1e-5, arith=torch.float64):
    """y, gx, gkey (with a key), the six control gradients and the branch mask `up`, as numpy arrays (float64 but for the mask)."""
    if arith is torch.float64:
        xl = x.detach().double().clone().requires_grad_(True)
        kl = None if key is None else key.detach().double().clone().requires_grad_(True)
        c = {k: ctl[k].detach().float().double().reshape(-1).clone().requires_grad_(True) for k in CTL}
        r = _reduction(LR.block_level(xl if kl is None else kl, hop, "peak"), c, eps)
        r_s, up = BR.ballistics(r, sr, c["attack_ms"], c["release_ms"], hop)
        y = GR.gain_curve(xl, c["makeup_gain_db"][:, None] - r_s, hop)
        leaves = [xl] + ([] if kl is None else [kl]) + [c[k] for k in CTL]
        grads = [g.numpy() for g in torch.autograd.grad((y * w.double()).sum(), leaves)]
        out = dict(y=y.detach().numpy(), gx=grads[0], up=up.numpy(), **{"g_" + k: g for k, g in zip(CTL, grads[-6:])})
        if kl is not None:
            out["gkey"] = grads[1]
        return out
    side = (x if key is None else key).detach().float()
    c = {k: ctl[k].detach().float().reshape(-1).clone().requires_grad_(True) for k in CTL}
    F = LR.control_frames(x.shape[-1], hop)
    hand = LR.by_hand(side.numpy(), np.zeros((len(x), F)), hop, "peak")
    L = torch.from_numpy(hand["L"]).float().requires_grad_(True)
    r = _reduction(L, c, eps)
    sm = BR.by_hand(r.detach().numpy(), sr, c["attack_ms"].detach().numpy(), c["release_ms"].detach().numpy(), np.zeros((len(x), F)), hop)
    E = torch.from_numpy(sm["E"]).float().requires_grad_(True)
    xl = x.detach().float().clone().requires_grad_(True)
    y = GR.gain_curve(xl, c["makeup_gain_db"][:, None] - E, hop, torch.float32)
    gx, gE, gmk = torch.autograd.grad((y * w.float()).sum(), [xl, E, c["makeup_gain_db"]])
    back = BR.by_hand(r.detach().numpy(), sr, c["attack_ms"].detach().numpy(), c["release_ms"].detach().numpy(), gE.numpy(), hop)
    gL, gthr, grat, gknee = torch.autograd.grad(r, [L, c["threshold_db"], c["ratio"], c["knee_db"]], torch.from_numpy(back["gP"]).float())
    gside = LR.by_hand(side.numpy(), gL.numpy(), hop, "peak")["gx"]
    f = lambda v: np.asarray(v, np.float64)
    out = dict(y=f(y.detach()), up=sm["up"], g_threshold_db=f(gthr), g_ratio=f(grat), g_attack_ms=back["gatt"], g_release_ms=back["grel"],
               g_knee_db=f(gknee), g_makeup_gain_db=f(gmk))
    if key is None:
        out["gx"] = f((gx + torch.from_numpy(gside).float()))
    else:
        out["gx"], out["gkey"] = f(gx), gside
    return out
