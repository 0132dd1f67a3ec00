"""Restatement of functional.ballistics on the CPU, in two forms.

`ballistics` is the definition as a loop over the frames, in torch float64, differentiable by autograd (torch.where branches) - the
oracle. For item b over the F values of a curve P, with E_{-1} = 0:

    t_a = clamp(attack_ms, 0.1, 10000);   c_a = -expm1(-ln 9 hop / (sr t_a / 1000));   c_r likewise from release_ms
    up_j = P_j > E_{j-1};   c_j = c_a if up_j else c_r;   E_j = E_{j-1} + c_j (P_j - E_{j-1})

A NaN control makes its whole item NaN.

`by_hand` is the forward pass and the adjoint without autograd, in numpy at the kernel's arithmetic: the constants in float64 from the
float32 controls, the recurrence in float64 with the products and sums rounded as written, E rounded once to float32; the branch mask
as the forward pass decided it; then

    Lambda_j = gE_j + (1 - c_{j+1}) Lambda_{j+1};   gP_j = c_j Lambda_j
    g_attack = (dc_a/dt_a) sum_{j: up_j} Lambda_j (P_j - E_{j-1});   g_release over the other frames;   dc/dt = -(1-c) ln 9 hop 1000 / (sr t^2)

in float64 in the order j = F-1 .. 0 with E_{j-1} the saved float32 value, every result rounded once to float32. Its error against the
float64 form is the yardstick e32 of the GPU tests.
"""
import numpy as np
import torch

from tests import envelope_restated as ER

CTL = ("attack_ms", "release_ms")
NAMES = ("E", "gP", "gatt", "grel")
FLOOR = dict(E=ER.FLOOR["E"], gP=ER.FLOOR["gx"], gatt=ER.FLOOR["gsm"], grel=ER.FLOOR["gsm"])
LN9, T_LO, T_HI = ER.LN9, ER.T_LO, ER.T_HI


def coefficient(t_ms, sr, hop):
    """c of a clamped time in ms, torch."""
    return -torch.expm1(-LN9 * hop / (sr * t_ms / 1000.0))


def ballistics(P, sr, attack_ms, release_ms, hop=64):
    """E (bs, F) float64 and the branch mask (bs, F) bool: the frame loop."""
    bs, F = P.shape
    P = P.double()
    ca, cr = (coefficient(ER._clamp(c.double().reshape(bs), T_LO, T_HI), sr, hop) for c in (attack_ms, release_ms))
    bad = torch.isnan(ca) | torch.isnan(cr)
    pois = torch.where(bad, torch.full_like(ca, float("nan")), torch.zeros_like(ca))
    e = torch.zeros(bs, dtype=torch.float64)
    out, ups = [], []
    for j in range(F):
        up = P[:, j] > e
        e = e + torch.where(up, ca, cr) * (P[:, j] - e)
        out.append(e + pois)
        ups.append(up)
    return torch.stack(out, -1), torch.stack(ups, -1)


def item_constants(sr, hop, t_ms):
    """c, t and whether t was clamped, float64 numpy (bs,), from the control as the kernel reads it (float32)."""
    s = np.asarray(t_ms, np.float32).astype(np.float64).reshape(-1)
    clamped = (s < T_LO) | (s > T_HI)
    t = np.where(s < T_LO, T_LO, np.where(s > T_HI, T_HI, s))
    return -np.expm1(-LN9 * hop / (sr * t / 1000.0)), t, clamped


def by_hand(P, sr, attack_ms, release_ms, w, hop=64, dt=np.float32):
    """E, up, gP, gatt and grel for the upstream gradient w (bs, F); float64 arrays of values held in dt (up: bool)."""
    P = np.asarray(P, dt).astype(np.float64)
    bs, F = P.shape
    (ca, ta, cla), (cr, tr, clr) = item_constants(sr, hop, attack_ms), item_constants(sr, hop, release_ms)
    pois = np.where(np.isnan(ca) | np.isnan(cr), np.nan, 0.0)
    E, up = np.zeros((bs, F)), np.zeros((bs, F), bool)
    e = np.zeros(bs)
    with np.errstate(invalid="ignore"):
        for j in range(F):
            u = P[:, j] > e
            e = e + np.where(u, ca, cr) * (P[:, j] - e)
            E[:, j], up[:, j] = e, u
        E = (E.astype(dt) + pois[:, None].astype(dt)).astype(np.float64)
        gE = np.asarray(w, dt).astype(np.float64)
        prev = np.concatenate([np.zeros((bs, 1)), E[:, :-1]], 1)
        gP, carry, sa, sr_ = np.zeros((bs, F)), np.zeros(bs), np.zeros(bs), np.zeros(bs)
        for j in range(F - 1, -1, -1):
            lam = gE[:, j] + carry
            carry = np.where(up[:, j], 1.0 - ca, 1.0 - cr) * lam
            gP[:, j] = np.where(up[:, j], ca, cr) * lam
            d = lam * (P[:, j] - prev[:, j])
            sa, sr_ = sa + np.where(up[:, j], d, 0.0), sr_ + np.where(up[:, j], 0.0, d)
        k = -LN9 * hop * 1000.0 / sr
        gatt = np.where(cla, 0.0, ((1.0 - ca) * k / (ta * ta) * sa).astype(dt)) + pois
        grel = np.where(clr, 0.0, ((1.0 - cr) * k / (tr * tr) * sr_).astype(dt)) + pois
        gP = (gP.astype(dt) + pois[:, None].astype(dt)).astype(np.float64)
    return dict(E=E, up=up, gP=gP, gatt=gatt.astype(np.float64), grel=grel.astype(np.float64))


def forward_backward(P, sr, attack_ms, release_ms, w, hop=64, arith=torch.float64):
    """E, up, gP, gatt and grel for the upstream gradient w (bs, F), as numpy arrays. arith=torch.float64: the frame loop and autograd;
    arith=torch.float32: `by_hand` at the kernel's arithmetic."""
    if arith is torch.float32:
        return by_hand(P.detach().numpy(), sr, attack_ms.detach().numpy(), release_ms.detach().numpy(), w.detach().numpy(), hop, np.float32)
    Pl = P.detach().float().double().clone().requires_grad_(True)
    a, r = (c.detach().float().double().reshape(-1).clone().requires_grad_(True) for c in (attack_ms, release_ms))
    E, up = ballistics(Pl, sr, a, r, hop)
    gP, ga, gr = torch.autograd.grad((E * w.double()).sum(), [Pl, a, r])
    return dict(E=E.detach().numpy(), up=up.numpy(), gP=gP.numpy(), gatt=ga.numpy(), grel=gr.numpy())


def rise_and_fall_ms(E, sr, hop, lo, hi, split):
    """10 - 90 % rise time of E[:split] from lo to hi and 90 - 10 % fall time of E[split:] back to lo, in ms, the crossings
    interpolated between frame points."""
    E = np.asarray(E, np.float64)
    a, b = lo + 0.1 * (hi - lo), lo + 0.9 * (hi - lo)

    def crossing(seg, level, rising):
        k = int(np.argmax(seg >= level if rising else seg <= level))
        if k == 0:
            return 0.0
        return k - 1 + (level - seg[k - 1]) / (seg[k] - seg[k - 1])
    up, down = E[:split], E[split - 1:]
    rise = crossing(up, b, True) - crossing(up, a, True)
    fall = crossing(down, a, False) - crossing(down, b, False)
    return rise * hop * 1000.0 / sr, fall * hop * 1000.0 / sr
