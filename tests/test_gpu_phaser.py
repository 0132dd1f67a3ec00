"""GPU tests of phaser (csrc/phaser.hip): parity of y, grad x and the five control gradients with the float64 restatement
(tests/phaser_restated.py), exact identities, the adjoint, bit-for-bit reproducibility, what happens off the nominal domain, what the
forward pass leaves behind, the refused
double backward and the module. The autograd and call-state contracts run on the op's entry in tests/autograd_contract_cases.py.

Parity bounds, as for feedback_delay. The yardstick is the restatement with a float64 phase and float32 arithmetic on the same inputs on
the CPU: e32 = its error against float64 throughout, relative to the peak of the float64 result. The kernel's scan orders its sums
differently, so it gets 4 x e32, and never less than the floors of the other fused effects: 2e-6 of the peak for y and grad x, 1e-5 for
the control gradients. The op has no atomics: wherever two results are compared, every quantity is compared bit for bit.

The restatement is a Python loop over samples and stages, so it runs once per (rate, stages): one batch of 2 T + 5 samples that holds
every length of the parity cases as an item group. An item of length L has its upstream gradient zero from L on; the op is causal, so
its y, grad x and control gradients over [0, L) are those of the signal cut to L samples, which is what the kernel is given. The
control gradients are taken per (item, channel) row, so that the same run serves one channel (row 0) and two (the sum).
"""
import functools

import numpy as np
import pytest
import torch

from tests import phaser_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTL = R.CTL
GRADS = R.GRADS
FLOOR = R.FLOOR
LANE, WAVE = 8, 512                        # samples of a lane's run and of a wave's 64 runs (csrc/phaser.hip PH_SPT)
SETS = 4                                   # control sets per length


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def tile(K):
    T = lib().dasp_phaser_tile(K)
    assert T == 4 * WAVE                   # four waves: the thresholds below are the kernel's
    return T


def lengths(K):
    T = tile(K)
    return [1, 2, LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1, 2 * T + 5]


def controls(sr, groups, seed):
    """SETS items per group. 0: rate 0 (a constant coefficient), mix 0.5, no clamp. 1: a negative rate, mix 1, no clamp. 2: 10 Hz over 20
    octaves around the middle of the clamp's range from phase 0.4 on - sin theta falls from 0.59 through zero, through both clamps - mix 0.5.
    3: a sweep whose top third is above the upper clamp, mix 1. Every value jittered from group to group."""
    g = torch.Generator().manual_seed(seed)
    j = lambda lo, hi: float(torch.rand((), generator=g)) * (hi - lo) + lo
    rows = []
    for _ in range(groups):
        rows += [(0.0, sr * j(0.02, 0.04), j(1.0, 1.5), j(0.0, 1.0), 0.5),
                 (-j(2.0, 9.0), sr * j(0.04, 0.06), j(1.0, 2.0), j(0.0, 1.0), 1.0),
                 (10.0, sr * (0.49 / 4096) ** 0.5 * j(0.9, 1.1), 20.0, 0.4, 0.5),
                 (j(1.0, 10.0), sr * 0.2, j(1.8, 2.2), j(0.15, 0.35), 1.0)]              # sin theta >= 0.8 at the start: above the clamp there
    t = torch.tensor(rows, dtype=torch.float32)
    return {k: t[:, q].contiguous() for q, k in enumerate(CTL)}


def plain(B, C, N, seed=0, sr=44100):
    """Everything inside its range: 0.05 - 10 Hz either way, centres of 200 - 4000 Hz at 44.1 kHz, up to 2 octaves, mix 0.2 - 1."""
    g = torch.Generator().manual_seed(91 * seed + 7 * B + 3 * C + N)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    return dict(x=u(-1.0, 1.0, B, C, N), w=torch.randn(B, C, N, generator=g), rate_hz=u(0.05, 10.0, B) * torch.sign(u(-1.0, 3.0, B)),
                center_hz=torch.exp(u(np.log(200.0), np.log(4000.0), B)) * sr / 44100, depth=u(0.0, 2.0, B), phase=u(0.0, 1.0, B), mix=u(0.2, 1.0, B))


def run_t(D, a, sr, K, need_gx=True, **kw):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    y = D.phaser(x, sr, *ctl, stages=K, **kw)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + ctl)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + GRADS, (y.detach(),) + grads))


@functools.lru_cache(maxsize=None)
def reference(sr, K):
    """The restatement's two runs for one (rate, stages): inputs, float64 results and float32-arithmetic results, control gradients per
    row. Computed once, read by the parity cases of both channel counts, never modified."""
    Ls = lengths(K)
    N, B = Ls[-1], SETS * len(Ls)
    g = torch.Generator().manual_seed(sr + K)
    a = dict(x=torch.rand(B, 2, N, generator=g) * 2 - 1, w=torch.randn(B, 2, N, generator=g), **controls(sr, len(Ls), sr + 31 * K))
    for q, L in enumerate(Ls):
        a["w"][SETS * q:SETS * (q + 1), :, L:] = 0
    args = [a["x"], sr] + [a[k] for k in CTL] + [a["w"]]
    want = R.forward_backward(*args, stages=K, per_row=True)
    f32 = R.forward_backward(*args, stages=K, per_row=True, arith=torch.float32)
    return a, want, f32


def cut(r, q, L, C):
    """Group q of a restated result as the op with C channels and L samples would give it."""
    s = slice(SETS * q, SETS * (q + 1))
    out = {"y": r["y"][s, :C, :L], "gx": r["gx"][s, :C, :L]}
    for k in GRADS:
        out[k] = r[k][s, :C].sum(1)
    return out


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 4, 12])
@pytest.mark.parametrize("sr", [8000, 44100, 192000])
def test_parity_with_the_float64_restatement(D, sr, K):
    a, want64, want32 = reference(sr, K)
    lo, hi = R.clamp_bounds(sr)
    raw, _ = R.sweep(sr, *[a[k].double() for k in CTL[:4]], 2, a["x"].shape[-1])
    below, above = (raw < lo).reshape(-1, SETS, *raw.shape[1:]), (raw > hi).reshape(-1, SETS, *raw.shape[1:])
    assert below[-1, 2].any() and above[-1, 2].any() and above[-1, 3].any() and not (below | above)[:, :2].any()     # the sweeps are what controls() says
    worst = {k: 0.0 for k in R.NAMES}
    for q, L in enumerate(lengths(K)):
        s = slice(SETS * q, SETS * (q + 1))
        for C in (1, 2):
            b = {k: v[s] for k, v in a.items()}
            b["x"], b["w"] = b["x"][:, :C, :L].contiguous(), b["w"][:, :C, :L].contiguous()
            got = {k: v.cpu().numpy() for k, v in run_t(D, b, sr, K).items()}
            want, f32 = cut(want64, q, L, C), cut(want32, q, L, C)
            e32 = {k: peak_err(f32[k], want[k]) for k in R.NAMES}
            e = {k: peak_err(got[k], want[k]) for k in R.NAMES}
            share = {k: e[k] / max(4 * e32[k], FLOOR[k]) for k in R.NAMES}
            record(f"phaser_parity sr={sr} K={K} ({SETS},{C},{L})", **e, **{"fp32_" + k: v for k, v in e32.items()}, **{"share_" + k: v for k, v in share.items()})
            for k in R.NAMES:
                assert got[k].shape == want[k].shape, (L, C, k)
                assert e[k] <= max(4 * e32[k], FLOOR[k]), (sr, K, L, C, k, e[k], e32[k])
                worst[k] = max(worst[k], share[k])
    record(f"phaser_parity_worst sr={sr} K={K}", **{"share_" + k: v for k, v in worst.items()})


# ---- 2. exact identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 12])
def test_mix_zero_is_the_identity(D, K):
    a = plain(4, 2, 2 * tile(K) + 5)
    a["mix"] = torch.zeros(4)
    with torch.no_grad():
        y = D.phaser(a["x"].to(DEV), 44100, *[a[k].to(DEV) for k in CTL], stages=K)
    assert torch.equal(y.cpu(), a["x"])


@pytest.mark.parametrize("K", [1, 4, 12])
def test_zero_coefficient_is_a_shift_by_the_number_of_stages(D, K):
    """depth = 0, center_hz = sample_rate / 4, mix = 1: a = 0 to float32 rounding, y is x delayed by K samples within the parity floor."""
    sr = 44100
    a = plain(2, 2, 2 * tile(K) + 5)
    a["center_hz"], a["depth"], a["mix"] = torch.full((2,), sr / 4), torch.zeros(2), torch.ones(2)
    with torch.no_grad():
        y = D.phaser(a["x"].to(DEV), sr, *[a[k].to(DEV) for k in CTL], stages=K).cpu()
    assert y[..., :K].abs().max() <= FLOOR["y"]
    assert (y[..., K:] - a["x"][..., :-K]).abs().max() <= FLOOR["y"] * a["x"].abs().max()


# ---- 3. adjoint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 12])
def test_adjoint(D, K):
    """The op is linear in x: <w, J v> = <J^T w, v> at 2 T + 5 samples, both sums taken in float64 on the host from the kernel's float32
    outputs. The relative difference, the largest over four draws of w, is within 4 x that of the float32-arithmetic restatement (taken
    at 700 samples, where the loop is quick: its rounding does not shrink with the length) and never above 1e-5."""
    sr = 44100
    a = plain(4, 2, 2 * tile(K) + 5)
    small = plain(4, 2, 700)
    g = torch.Generator().manual_seed(77)

    def rel(x, y, gx, w):
        yw = (np.float64(y) * np.float64(w)).sum()
        return abs(float(yw - (np.float64(x) * np.float64(gx)).sum())) / abs(float(yw))
    got, want = [], []
    for _ in range(4):
        a["w"], small["w"] = torch.randn(a["x"].shape, generator=g), torch.randn(small["x"].shape, generator=g)
        k = run_t(D, a, sr, K)
        got.append(rel(a["x"].numpy(), k["y"].cpu().numpy(), k["gx"].cpu().numpy(), a["w"].numpy()))
        r = R.forward_backward(small["x"], sr, *[small[c] for c in CTL], small["w"], stages=K, arith=torch.float32)
        want.append(rel(small["x"].numpy(), r["y"].astype(np.float32), r["gx"].astype(np.float32), small["w"].numpy()))
    record(f"phaser_adjoint K={K}", kernel=max(got), restated_fp32=max(want))
    assert max(got) <= 4 * max(want) and max(got) <= 1e-5, (got, want)


# ---- 4. reproducibility: everything bit for bit ------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(D):
    a = plain(6, 2, 2 * tile(4) + 5)
    p, q = run_t(D, a, 44100, 4), run_t(D, a, 44100, 4)
    for k in R.NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, 4, need_gx=False)         # x needs no gradient: gx is not written, nothing else changes
    for k in ("y",) + GRADS:
        assert torch.equal(p[k], r[k]), k


def test_item_alone_and_inside_a_batch(D):
    a = plain(5, 2, 2 * tile(4) + 5)
    whole = run_t(D, a, 44100, 4)
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, 4)
        for k in R.NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path, nothing to zero, and the LDS
    limit of the backward kernel was raised when the library was loaded."""
    sr, K = 44100, 4
    a = plain(4, 2, 2 * tile(K) + 5)
    eager = run_t(D, a, sr, K)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.phaser(xt, sr, *ctl, stages=K)
        return (y,) + torch.autograd.grad((y * wt).sum(), [xt] + ctl)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in range(3):
        for o in outs:
            o.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, o in zip(R.NAMES, outs):
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 5. off the nominal domain -----------------------------------------------------------------------------------------------------------
def _item0_unchanged(clean, dirty):
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_audio_and_controls_stay_in_their_item(D, value):
    N = 2 * tile(4) + 5
    a = plain(2, 2, N)
    clean = run_t(D, a, 44100, 4)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    for k in CTL:
        b[k][1] = float("nan")
    dirty = run_t(D, b, 44100, 4)
    _item0_unchanged(clean, dirty)
    assert torch.isnan(dirty["y"][1]).all() and torch.isnan(dirty["gx"][1]).all() and all(torch.isnan(dirty[k][1]) for k in GRADS)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_audio_alone_stays_in_its_item(D, value):
    """Bad samples under clean controls, the first of them at sample 0: every y of the item is NaN or inf (a bad sample stays in the
    stages' states), and so is every control gradient; grad x, which holds no x, keeps its bits, and so does all of item 0."""
    a = plain(2, 2, 2 * tile(4) + 5)
    clean = run_t(D, a, 44100, 4)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    dirty = run_t(D, b, 44100, 4)
    _item0_unchanged(clean, dirty)
    assert not torch.isfinite(dirty["y"][1]).any() and not any(torch.isfinite(dirty[k][1]) for k in GRADS)
    assert torch.equal(dirty["gx"][1], clean["gx"][1])


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_upstream_gradient_stays_in_its_item(D, value):
    a = plain(2, 2, 2 * tile(4) + 5)
    clean = run_t(D, a, 44100, 4)
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = value
    dirty = run_t(D, b, 44100, 4)
    _item0_unchanged(clean, dirty)
    assert torch.equal(clean["y"], dirty["y"]) and not any(torch.isfinite(dirty[k][1]) for k in GRADS)


@pytest.mark.parametrize("n0", [0, 3000, 4100])
def test_one_nan_sample_reaches_every_later_sample_of_its_row_and_nothing_else(D, n0):
    """What the restatement says (a NaN stays in the stages' states): y of row (0, 1) is NaN from n0 on and finite before it, every other
    row keeps its bits; the restatement itself is asked at 700 samples, where the loop is quick."""
    K, N = 4, 2 * tile(4) + 5
    a = plain(2, 2, N)
    clean = run_t(D, a, 44100, K)
    a["x"][0, 1, n0] = float("nan")
    got = run_t(D, a, 44100, K)
    bad = torch.isnan(got["y"]).cpu()
    want = torch.zeros(2, 2, N, dtype=torch.bool)
    want[0, 1, n0:] = True
    assert torch.equal(bad, want)
    for r in ((0, 0), (1, 0), (1, 1)):
        assert torch.equal(got["y"][r], clean["y"][r]) and torch.equal(got["gx"][r], clean["gx"][r]), r
    assert torch.equal(got["y"][0, 1, :n0], clean["y"][0, 1, :n0])
    for k in GRADS:
        assert torch.equal(got[k][1], clean[k][1]), k
    s = plain(1, 2, 700)
    m0 = 350
    s["x"][0, 1, m0] = float("nan")
    y = R.phaser(s["x"].double(), 44100, *[s[k].double() for k in CTL], stages=K)
    assert torch.isnan(y[0, 1, m0:]).all() and torch.isfinite(y[0, 1, :m0]).all() and torch.isfinite(y[0, 0]).all()


@pytest.mark.parametrize("which", CTL)
def test_nan_control_gives_a_nan_item(D, which):
    a = plain(3, 2, 2 * tile(4) + 5)
    clean = run_t(D, a, 44100, 4)
    a[which][1] = float("nan")
    dirty = run_t(D, a, 44100, 4)
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
        assert torch.isnan(dirty[k][1]).all(), k


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * tile(4) + 5
    a = plain(3, 2, N)
    want = run_t(D, a, 44100, 4)
    x = a["x"].to(DEV)
    if view == "offset":
        xv = torch.cat([torch.zeros(5, device=DEV), x.reshape(-1)])[5:].view(3, 2, N)
    elif view == "strided":
        xv = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not xv.is_contiguous()
    else:
        xv = torch.cat([x, torch.ones(3, 2, 40, device=DEV)], -1)[..., :N]
        assert not xv.is_contiguous()
    assert torch.equal(xv, x)
    xv.requires_grad_(True)
    ctl = [torch.stack([a[k], a[k]], -1).to(DEV)[:, 1].requires_grad_(True) for k in CTL]            # strided controls
    y = D.phaser(xv, 44100, *ctl, stages=4)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    for k, g in zip(R.NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


@pytest.mark.parametrize("K", [4, 12])
def test_c_abi_keeps_guard_words_and_ignores_dirty_scratch(D, K):
    """Through the C ABI: y, the states, gx, gctl and the partials written inside NaN-filled guard words leave the guards NaN, NaN-filled
    state and partials buffers give the same bits as zero-filled ones, and states = NULL / gx = NULL change nothing else."""
    from dasp_pytorch_amd._lib import call, ptr, stream
    sr, spread, G = 44100, 0.25, 64
    B, C = 3, 2
    N = 2 * tile(K) + 5
    a = plain(B, C, N)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    ctl = torch.stack([a[k] for k in CTL], -1).contiguous().to(DEV)
    nstate, npart = lib().dasp_phaser_state_floats(B * C, N, K), lib().dasp_phaser_partial_floats(B * C)
    assert nstate == B * C * 3 * K and npart == 5 * B * C

    def guarded(n, fill=float("nan")):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        buf[G:G + n] = fill
        return buf, buf[G:G + n]

    def run(fill, save=True, want_gx=True):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("gx", B * C * N), ("gctl", B * 5))}
        bufs["states"], bufs["partials"] = guarded(nstate, fill), guarded(npart, fill)
        call("dasp_phaser_forward", ptr(x), ptr(ctl), ptr(bufs["y"][1]), ptr(bufs["states"][1] if save else None), B, C, N, K, float(sr), spread, stream())
        if not save:
            call("dasp_phaser_forward", ptr(x), ptr(ctl), ptr(torch.empty_like(x)), ptr(bufs["states"][1]), B, C, N, K, float(sr), spread, stream())
        call("dasp_phaser_backward", ptr(x), ptr(ctl), ptr(bufs["states"][1]), ptr(gy), ptr(bufs["gx"][1] if want_gx else None), ptr(bufs["gctl"][1]),
             ptr(bufs["partials"][1]), B, C, N, K, float(sr), spread, stream())
        torch.cuda.synchronize()
        for k, (buf, inner) in bufs.items():
            assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
            assert torch.isfinite(inner).all() or (k == "gx" and not want_gx and torch.isnan(inner).all()), k
        return {k: inner.clone() for k, (buf, inner) in bufs.items()}

    zero, dirty, lean = run(0.0), run(float("nan")), run(0.0, save=False, want_gx=False)
    for k in ("y", "states", "gx", "gctl", "partials"):
        assert torch.equal(zero[k], dirty[k]), k
    for k in ("y", "states", "gctl", "partials"):
        assert torch.equal(zero[k], lean[k]), k
    ref = run_t(D, a, sr, K)
    assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"])
    for q, k in enumerate(GRADS):
        assert torch.equal(zero["gctl"].view(B, 5)[:, q], ref[k]), k


def test_silence_in_silence_out(D):
    a = plain(2, 2, 2 * tile(4) + 5)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100, 4)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS)


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        ctl = [torch.ones(B, device=DEV, requires_grad=True) for _ in range(5)]
        y = D.phaser(x, 44100, *ctl)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


# ---- 6. what the forward pass leaves behind ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 12])
def test_forward_saves_the_tile_states_and_nothing_of_the_signals_length(D, K):
    """Beyond x and the packed controls the forward pass keeps dasp_phaser_state_floats(rows, N, K) floats for backward - K per tile and
    row, below N rows / 8 at N = 2 T + 5 - and nothing at all when no input needs a gradient."""
    B, C = 3, 2
    N = 2 * tile(K) + 5
    a = plain(B, C, N)
    x = a["x"].to(DEV).requires_grad_(True)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = D.phaser(x, 44100, *ctl, stages=K)
    nstate = lib().dasp_phaser_state_floats(B * C, N, K)
    assert nstate == B * C * 3 * K and nstate < N * B * C / 8
    sizes = sorted(t.numel() for t in saved)
    assert sizes == sorted([B * C * N, B * 5, nstate]), sizes
    assert any(t.data_ptr() == x.data_ptr() for t in saved)                     # x itself, not a copy
    y.sum().backward()
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.phaser(x.detach(), 44100, *[c.detach() for c in ctl], stages=K)
    assert not saved


# ---- 7. double backward ------------------------------------------------------------------------------------------------------------------
def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.phaser(x, 44100, *[a[k].to(DEV) for k in CTL])
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 8. module ---------------------------------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    sr = 44100
    x = plain(3, 2, 3000)["x"].to(DEV)
    p = torch.rand(3, 5, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = D.Phaser(sr, stages=6, stereo_spread=0.1)
    lo = torch.tensor([0.05, 200.0, 0.0, 0.0, 0.0], device=DEV)
    span = torch.tensor([9.95, 3800.0, 2.0, 1.0, 1.0], device=DEV)
    with torch.no_grad():
        got = m.process_normalized(x, p)
        d = p * span + lo
        want = D.phaser(x, sr, d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], stages=6, stereo_spread=0.1)
    assert torch.equal(got, want)
