"""GPU tests of time_varying_filter (csrc/tvfilter.hip): parity of y, grad x and the three control gradients with the float64 restatement
(tests/tvfilter_restated.py), the static case against the RBJ biquads, exact identities, clamped frame values, the last frame point, a
frame point on a tile boundary, the adjoint, bit-for-bit reproducibility, NaN frame values, views and guard words, the errors of the C
ABI, the refused
double backward and the module. The autograd and call-state contracts run on the op's entry in tests/autograd_contract_cases.py.

Parity bounds, as for phaser. The yardstick is the restatement with float64 frame points and float32 arithmetic on the same inputs on the
CPU: e32 = its error against float64 throughout, relative to the peak of the float64 result. The kernel's scan orders its products
differently, so it gets 4 x e32, and never less than the floors of the other fused effects: 2e-6 of the peak for y and grad x, 1e-5 for
the control gradients. As in tests/test_gpu_phaser.py an error is the largest difference over a case's items against the largest value
over them: gmix is one number per item and gq at hop 2048 two or three, and the float32 restatement's error in a single number is one
draw of its rounding, anywhere between nothing and its scale, which no kernel can be held to four times of. (Measured over some 530 items
of the parity cases: the kernel's error in gmix is 0.1 - 0.5 of the restatement's in the geometric mean and never above its largest,
yet 146 times a single draw of it.) The op has no atomics: wherever two results are compared, every quantity is compared bit for bit.

The restatement is a Python loop over samples, so it runs once per (rate, hop, mode): one batch of 6149 samples that holds every length
of the parity cases as an item group. An item of length L has its upstream gradient zero from L on; the op is causal and a curve's first
ceil(L / hop) + 1 frame points are all that L samples read, so its y, grad x and control gradients over [0, L) are those of the signal
and the curves cut to L samples, which is what the kernel is given. The control gradients are taken per (item, channel) row, so that the
same run serves one channel (row 0) and two (the sum).
"""
import functools
import math

import numpy as np
import pytest
import scipy.signal
import torch

from tests import tvfilter_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTL = R.CTL
GRADS = R.GRADS
FLOOR = R.FLOOR
LANE, WAVE, TILE = 8, 512, 2048            # samples of a lane's run, of a wave's 64 runs and of a tile (csrc/tvfilter.hip TV_SPT, TV_TILE)
LENGTHS = (1, 7, 8, 9, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5)
SETS = 3                                   # control sets per length: two draws of the main sweep, the hard set
MODE_INDEX = {m: i for i, m in enumerate(R.MODES)}


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    assert lib().dasp_tvfilter_tile() == TILE
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def curves(sr, B, F, g, hard=False):
    """The main sweep: log-uniform cutoff 50 Hz - 12 kHz, q 0.5 - 8, a draw per frame point. The hard set: cutoff sr/4096 - 200 Hz, q 20 - 100."""
    u = lambda lo, hi: torch.exp(torch.rand(B, F, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))
    return (u(sr / 4096, 200.0), u(20.0, 100.0)) if hard else (u(50.0, 12000.0), u(0.5, 8.0))


def plain(B, C, N, hop=64, seed=0, sr=44100, hard=False):
    g = torch.Generator().manual_seed(91 * seed + 7 * B + 3 * C + N + hop)
    cut, q = curves(sr, B, R.control_frames(N, hop), g, hard)
    return dict(x=torch.rand(B, C, N, generator=g) * 2 - 1, w=torch.randn(B, C, N, generator=g), cutoff_hz=cut, q=q, mix=torch.rand(B, generator=g) * 0.8 + 0.2)


def run_t(D, a, sr, hop=64, mode="lowpass", need_gx=True):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    y = D.time_varying_filter(x, sr, *ctl, hop=hop, mode=mode)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + ctl)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + GRADS, (y.detach(),) + grads))


def restated(a, sr, hop, mode, **kw):
    return R.forward_backward(a["x"], sr, a["cutoff_hz"], a["q"], a["mix"], a["w"], hop, mode, **kw)


def held(got, want, f32, what):
    """Every quantity within max(4 e32, floor) of its peak over the case's items; returns the share of its bound per quantity."""
    share = {}
    for k in R.NAMES:
        assert got[k].shape == want[k].shape, (what, k)
        e32, e = peak_err(f32[k], want[k]), peak_err(got[k], want[k])
        bound = max(4 * e32, FLOOR[k])
        share[k] = e / bound
        print(f"PARITY {what} {k}: kernel {e:.3e} fp32 {e32:.3e} bound {bound:.3e}")
        assert e <= bound, (what, k, e, e32)
    return share


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(sr, hop, mode):
    """The restatement's two runs for one (rate, hop, mode): inputs, float64 results and float32-arithmetic results, control gradients
    per row. Computed once, read by the parity cases of both channel counts, never modified."""
    N, B = LENGTHS[-1], SETS * len(LENGTHS)
    F = R.control_frames(N, hop)
    g = torch.Generator().manual_seed(sr + 31 * hop + MODE_INDEX[mode])
    cut, q = curves(sr, B, F, g)
    hc, hq = curves(sr, B, F, g, hard=True)
    cut[2::SETS], q[2::SETS] = hc[2::SETS], hq[2::SETS]
    mix = torch.rand(B, generator=g) * 0.8 + 0.2
    mix[1::SETS] = 1.0
    a = dict(x=torch.rand(B, 2, N, generator=g) * 2 - 1, w=torch.randn(B, 2, N, generator=g), cutoff_hz=cut, q=q, mix=mix)
    for i, L in enumerate(LENGTHS):
        a["w"][SETS * i:SETS * (i + 1), :, L:] = 0
    return a, restated(a, sr, hop, mode, per_row=True), restated(a, sr, hop, mode, per_row=True, arith=torch.float32)


def cut_to(r, i, L, C, hop):
    """Group i of a restated result as the op with C channels, L samples and their frame points would give it."""
    s, F = slice(SETS * i, SETS * (i + 1)), R.control_frames(L, hop)
    return {"y": r["y"][s, :C, :L], "gx": r["gx"][s, :C, :L], "gcutoff": r["gcutoff"][s, :C, :F].sum(1), "gq": r["gq"][s, :C, :F].sum(1),
            "gmix": r["gmix"][s, :C].sum(1)}


@pytest.mark.parametrize("sr,hop,mode", [(44100, 64, "lowpass"), (44100, 8, "bandpass"), (44100, 2048, "highpass"), (44100, 64, "notch"),
                                         (8000, 8, "lowpass"), (8000, 2048, "bandpass"), (192000, 64, "highpass"), (192000, 2048, "notch")])
def test_parity_with_the_float64_restatement(D, sr, hop, mode):
    a, want64, want32 = reference(sr, hop, mode)
    assert float(a["cutoff_hz"][2::SETS].max()) <= 200.0 and float(a["q"][2::SETS].min()) >= 20.0              # the hard set is what curves() says
    worst = {k: 0.0 for k in R.NAMES}
    for i, L in enumerate(LENGTHS):
        s, F = slice(SETS * i, SETS * (i + 1)), R.control_frames(L, hop)
        for C in (1, 2):
            b = dict(x=a["x"][s, :C, :L].contiguous(), w=a["w"][s, :C, :L].contiguous(), cutoff_hz=a["cutoff_hz"][s, :F].contiguous(),
                     q=a["q"][s, :F].contiguous(), mix=a["mix"][s])
            got = {k: v.cpu().numpy() for k, v in run_t(D, b, sr, hop, mode).items()}
            share = held(got, cut_to(want64, i, L, C, hop), cut_to(want32, i, L, C, hop), f"sr={sr} hop={hop} {mode} ({SETS},{C},{L})")
            record(f"tvfilter_parity sr={sr} hop={hop} mode={mode} ({SETS},{C},{L})", **{"share_" + k: v for k, v in share.items()})
            worst = {k: max(worst[k], share[k]) for k in R.NAMES}
    record(f"tvfilter_parity_worst sr={sr} hop={hop} mode={mode}", **{"share_" + k: v for k, v in worst.items()})


def test_four_items(D):
    """bs = 4 with two channels at three tiles and a ragged tail, the restatement asked at that size directly."""
    a = plain(4, 2, 4097 + 40, hop=64, seed=3)
    a["w"][..., 700:] = 0                                   # the loop is quick where the gradient is short; y is compared over all samples
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, 44100, 64, "bandpass").items()}
    share = held(got, restated(a, 44100, 64, "bandpass"), restated(a, 44100, 64, "bandpass", arith=torch.float32), "four items")
    record("tvfilter_four_items", **{"share_" + k: v for k, v in share.items()})


# ---- 2. the static case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lowpass", "highpass", "bandpass"])
def test_constant_curves_equal_the_float64_biquad(D, mode):
    """Constant curves against the RBJ biquad of scipy in float64 (tests/test_tvfilter_cpu.py holds the restatement to it at 1e-9): within
    max(4 e32, 2e-6) of the peak, e32 the float32-arithmetic restatement's error against the same biquad."""
    from tests.test_tvfilter_cpu import rbj
    sr, N, hop = 44100, 2 * TILE + 5, 64
    F = R.control_frames(N, hop)
    x = torch.rand(4, 1, N, generator=torch.Generator().manual_seed(11)) * 2 - 1
    fq = [(sr / 4096, 30.0), (300.0, 0.5), (2500.0, 4.0), (0.49 * sr, 0.5)]
    cut, q = (torch.tensor([[v[i]] * F for v in fq], dtype=torch.float32) for i in (0, 1))
    with torch.no_grad():
        y = D.time_varying_filter(x.to(DEV), sr, cut.to(DEV), q.to(DEV), torch.ones(4, device=DEV), hop=hop, mode=mode).cpu().numpy()
        y32 = R.time_varying_filter(x, sr, cut, q, torch.ones(4), hop, mode, torch.float32).numpy()
    for b in range(4):
        want = scipy.signal.lfilter(*rbj(mode, float(cut[b, 0]), float(q[b, 0]), sr), x[b, 0].double().numpy())
        e, e32 = peak_err(y[b, 0], want), peak_err(y32[b, 0], want)
        record(f"tvfilter_static {mode} f={float(cut[b, 0]):.1f} q={float(q[b, 0])}", kernel=e, restated_fp32=e32)
        assert e <= max(4 * e32, FLOOR["y"]), (mode, b, e, e32)


# ---- 3. exact identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_mix_zero_is_the_identity(D, mode):
    a = plain(4, 2, 2 * TILE + 5)
    with torch.no_grad():
        y = D.time_varying_filter(a["x"].to(DEV), 44100, a["cutoff_hz"].to(DEV), a["q"].to(DEV), torch.zeros(4, device=DEV), mode=mode)
    assert torch.equal(y.cpu(), a["x"])


@pytest.mark.parametrize("mode", ["lowpass", "bandpass"])
def test_curves_with_equal_neighbours_give_the_same_bits_at_every_hop(D, mode):
    """Constant curves: G_{j+1} - G_j = 0, so g and k are the frame values whatever t and hop are - y, gx and gmix agree bit for bit
    between the hops, and the frame gradients of either hop add up to the same total within the floor."""
    N = 2 * TILE + 5
    base = plain(3, 2, N, hop=8)
    out = {}
    for hop in (8, 64, 2048):
        F = R.control_frames(N, hop)
        a = dict(base, cutoff_hz=base["cutoff_hz"][:, :1].expand(3, F).contiguous(), q=base["q"][:, :1].expand(3, F).contiguous())
        out[hop] = run_t(D, a, 44100, hop, mode)
    for hop in (64, 2048):
        for k in ("y", "gx", "gmix"):
            assert torch.equal(out[8][k], out[hop][k]), (hop, k)
        for k in ("gcutoff", "gq"):
            p, q = out[8][k].double().sum(1), out[hop][k].double().sum(1)
            assert ((p - q).abs() <= 1e-5 * out[8][k].double().abs().sum(1)).all(), (hop, k)


# ---- 4. clamping, the last frame point, the tile boundary -----------------------------------------------------------------------------------
def test_clamped_frame_values_give_the_clamped_result_and_exactly_zero_gradients_there_and_only_there(D):
    sr, hop, N = 44100, 64, TILE + 300
    a = plain(2, 2, N, seed=5)
    F = R.control_frames(N, hop)
    lo, hi = R.clamp_bounds(sr)
    out_c, out_q = torch.zeros(2, F, dtype=torch.bool), torch.zeros(2, F, dtype=torch.bool)
    out_c[0, 3], out_c[0, 32], out_c[1, 0], out_c[1, F - 1] = True, True, True, True            # frame point 32 is sample 2048
    out_q[0, 5], out_q[1, 32], out_q[1, 33] = True, True, True
    b = {k: v.clone() for k, v in a.items()}
    b["cutoff_hz"][out_c] = torch.tensor([1.0, 30000.0, 1e9, -5.0])
    b["q"][out_q] = torch.tensor([0.01, 1e4, 0.0])
    c = {k: v.clone() for k, v in a.items()}
    c["cutoff_hz"][out_c] = torch.tensor([lo, hi, hi, lo], dtype=torch.float64).float()
    c["q"][out_q] = torch.tensor([0.1, 100.0, 0.1])
    got, edge = run_t(D, b, sr, hop), run_t(D, c, sr, hop)
    assert torch.equal((got["gcutoff"] == 0).cpu(), out_c) and torch.equal((got["gq"] == 0).cpu(), out_q)
    # float32(lo), float32(hi) may sit a rounding outside the float64 bounds and be clamped themselves: the same G, K either way
    for k in ("y", "gx", "gmix"):
        assert torch.equal(got[k], edge[k]), k
    assert torch.equal(got["gcutoff"][~out_c.to(DEV)], edge["gcutoff"][~out_c.to(DEV)]) and torch.equal(got["gq"][~out_q.to(DEV)], edge["gq"][~out_q.to(DEV)])


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_the_last_frame_point(D, hop):
    """Frame point F - 1 ends the last interval and takes t gg of its samples (tests/test_tvfilter_cpu.py): exactly zero when that interval
    holds one sample, the one on frame point F - 2 (seq_len = 1 mod hop), and the oracle's value when hop divides seq_len."""
    for N in (2 * TILE + 1, 1):
        got = run_t(D, plain(2, 2, N, hop=hop, seed=2), 44100, hop)
        assert not got["gcutoff"][:, -1].any() and not got["gq"][:, -1].any() and got["gcutoff"][:, :-1].all(), N
    a = plain(2, 2, TILE, hop=hop, seed=2)
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, 44100, hop).items()}
    want, f32 = restated(a, 44100, hop, "lowpass"), restated(a, 44100, hop, "lowpass", arith=torch.float32)
    held(got, want, f32, f"last frame point hop={hop}")
    assert got["gcutoff"][:, -1].all() and got["gq"][:, -1].all()
    for k in ("gcutoff", "gq"):
        assert np.abs(got[k][:, -1] - want[k][:, -1]).max() <= max(4 * peak_err(f32[k], want[k]), FLOOR[k]) * np.abs(want[k]).max(), k


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_a_frame_point_on_a_tile_boundary_matches_the_oracle(D, hop):
    """The upstream gradient lives on [1900, 2200): the frame point at sample 2048 takes a half from either tile."""
    N = TILE + 600
    a = plain(2, 2, N, hop=hop, seed=4)
    a["w"][..., :1900] = 0
    a["w"][..., 2200:] = 0
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, 44100, hop, "bandpass").items()}
    want, f32 = restated(a, 44100, hop, "bandpass"), restated(a, 44100, hop, "bandpass", arith=torch.float32)
    held(got, want, f32, f"tile boundary hop={hop}")
    j = TILE // hop
    for k in ("gcutoff", "gq"):
        assert want[k][:, j].all() and got[k][:, j].all()
        assert np.abs(got[k][:, j] - want[k][:, j]).max() <= max(4 * peak_err(f32[k], want[k]), FLOOR[k]) * np.abs(want[k]).max(), k


# ---- 5. adjoint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_adjoint(D, mode):
    """The op is linear in x: <u, J x> = <J^T u, x> at three tiles and a tail, both sums taken in float64 on the host from the kernel's
    float32 outputs, four draws of u. The difference is held against ||y|| ||u||, not against <y, u> itself, which a draw can bring near
    zero. Bound: y and gx leave the kernel rounded to float32, which alone moves either inner product by up to 2^-24 sum |y u| <= 2^-24
    ||y|| ||u||, so 2^-23 for the two; the kernel's own rounding inside is of that size per sample and without a common sign, so it adds
    1 / sqrt(samples) of it. A wrong coupling of one sample per tile shows at 1e-5. The float32-arithmetic restatement's figure (at 700
    samples, where the loop is quick) is recorded beside it."""
    sr = 44100
    a, small = plain(4, 2, 3 * TILE + 5), plain(4, 2, 700)
    g = torch.Generator().manual_seed(77)

    def rel(x, y, gx, w):
        x, y, gx, w = (np.float64(t) for t in (x, y, gx, w))
        return abs(float((y * w).sum() - (x * gx).sum())) / float(np.sqrt((y * y).sum() * (w * w).sum()))
    got, want = [], []
    for _ in range(4):
        a["w"], small["w"] = torch.randn(a["x"].shape, generator=g), torch.randn(small["x"].shape, generator=g)
        k = run_t(D, a, sr, 64, mode)
        got.append(rel(a["x"].numpy(), k["y"].cpu().numpy(), k["gx"].cpu().numpy(), a["w"].numpy()))
        r = restated(small, sr, 64, mode, arith=torch.float32)
        want.append(rel(small["x"].numpy(), r["y"].astype(np.float32), r["gx"].astype(np.float32), small["w"].numpy()))
    record(f"tvfilter_adjoint {mode}", kernel=max(got), restated_fp32=max(want))
    assert max(got) <= 2.0 ** -23, (got, want)


# ---- 6. reproducibility: everything bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [8, 2048])
def test_runs_are_bit_identical(D, hop):
    a = plain(6, 2, 3 * TILE + 5, hop=hop)
    p, q = run_t(D, a, 44100, hop), run_t(D, a, 44100, hop)
    for k in R.NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, hop, need_gx=False)       # x needs no gradient: gx is not written, nothing else changes
    for k in ("y",) + GRADS:
        assert torch.equal(p[k], r[k]), k


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_item_alone_and_inside_a_batch(D, hop):
    a = plain(4, 2, 3 * TILE + 5, hop=hop)
    whole = run_t(D, a, 44100, hop, "highpass")
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, hop, "highpass")
        for k in R.NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path and nothing to zero."""
    sr, hop = 44100, 64
    a = plain(4, 2, 3 * TILE + 5)
    eager = run_t(D, a, sr, hop, "notch")
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.time_varying_filter(xt, sr, *ctl, hop=hop, mode="notch")
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


# ---- 7. off the nominal domain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cutoff_hz", "q"])
@pytest.mark.parametrize("hop,j", [(64, 0), (64, 1), (64, 40), (8, 300), (2048, 1), (2048, 2), (64, -1)])
def test_one_nan_frame_value_reaches_its_item_from_the_interval_before_it_and_nothing_else(D, which, hop, j):
    """A NaN at frame point j: y of item 1 is NaN from sample (j - 1) hop on and keeps its bits before it; items 0 and 2 keep every bit of
    every result (tests/test_tvfilter_cpu.py shows the same reach for the restatement)."""
    N = 2 * TILE + 5
    a = plain(3, 2, N, hop=hop)
    clean = run_t(D, a, 44100, hop)
    j = j % R.control_frames(N, hop)
    a[which][1, j] = float("nan")
    got = run_t(D, a, 44100, hop)
    n0 = max(j - 1, 0) * hop
    bad = torch.isnan(got["y"]).cpu()
    want = torch.zeros(3, 2, N, dtype=torch.bool)
    want[1, :, n0:] = True
    assert torch.equal(bad, want)
    assert torch.equal(got["y"][1, :, :n0], clean["y"][1, :, :n0])
    for k in R.NAMES:
        assert torch.equal(got[k][0], clean[k][0]) and torch.equal(got[k][2], clean[k][2]), k


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_poisoned_audio_and_upstream_gradient_stay_in_their_item(D, value):
    a = plain(2, 2, 2 * TILE + 5)
    clean = run_t(D, a, 44100)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    dirty = run_t(D, b, 44100)
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k
    assert not torch.isfinite(dirty["y"][1]).any() and not torch.isfinite(dirty["gmix"][1])
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = value
    dirty = run_t(D, b, 44100)
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k
    assert torch.equal(clean["y"], dirty["y"]) and not torch.isfinite(dirty["gmix"][1])


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * TILE + 5
    a = plain(3, 2, N)
    want = run_t(D, a, 44100)
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
    F = a["q"].shape[1]
    if view == "offset":
        ctl = [torch.cat([torch.zeros(3, device=DEV), a[k].to(DEV).reshape(-1)])[3:].view(a[k].shape).requires_grad_(True) for k in CTL]
    elif view == "strided":
        ctl = [torch.stack([a[k], a[k]], -1).to(DEV)[..., 1].requires_grad_(True) for k in CTL]
        assert not ctl[0].is_contiguous()
    else:
        ctl = [torch.cat([a[k].to(DEV), torch.ones(3, 7, device=DEV)], -1)[:, :F].requires_grad_(True) for k in CTL[:2]] + [a["mix"].to(DEV).requires_grad_(True)]
        assert not ctl[0].is_contiguous()
    y = D.time_varying_filter(xv, 44100, *ctl)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    for k, g in zip(R.NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


@pytest.mark.parametrize("hop,mode", [(8, "lowpass"), (2048, "highpass")])
def test_c_abi_keeps_guard_words_and_ignores_dirty_scratch(D, hop, mode):
    """Through the C ABI: y, the states, gx, gcutoff, gq, gmix and the scratch written inside NaN-filled guard words leave the guards
    NaN, NaN-filled state and scratch buffers give the same bits as zero-filled ones, and states = NULL / gx = NULL change nothing else."""
    from dasp_pytorch_amd._lib import call, ptr, stream
    sr, G = 44100, 64
    B, C = 3, 2
    N = 2 * TILE + 5
    m = MODE_INDEX[mode]
    a = plain(B, C, N, hop=hop)
    F = R.control_frames(N, hop)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    cut, q, mix = (a[k].to(DEV) for k in CTL)
    nstate, nscr = lib().dasp_tvfilter_state_floats(B * C, N), lib().dasp_tvfilter_scratch_floats(B * C, N, hop)
    assert nstate == B * C * 3 * 2 and nscr == B * C * (2 * F + 1) and lib().dasp_tvfilter_frames(N, hop) == F

    def guarded(n, fill=float("nan")):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        buf[G:G + n] = fill
        return buf, buf[G:G + n]

    def run(fill, save=True, want_gx=True):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("gx", B * C * N), ("gcutoff", B * F), ("gq", B * F), ("gmix", B))}
        bufs["states"], bufs["scratch"] = guarded(nstate, fill), guarded(nscr, fill)
        call("dasp_tvfilter_forward", ptr(x), ptr(cut), ptr(q), ptr(mix), ptr(bufs["y"][1]), ptr(bufs["states"][1] if save else None), B, C, N, hop, m, float(sr), stream())
        if not save:
            call("dasp_tvfilter_forward", ptr(x), ptr(cut), ptr(q), ptr(mix), ptr(torch.empty_like(x)), ptr(bufs["states"][1]), B, C, N, hop, m, float(sr), stream())
        call("dasp_tvfilter_backward", ptr(x), ptr(cut), ptr(q), ptr(mix), ptr(bufs["states"][1]), ptr(gy), ptr(bufs["gx"][1] if want_gx else None),
             ptr(bufs["gcutoff"][1]), ptr(bufs["gq"][1]), ptr(bufs["gmix"][1]), ptr(bufs["scratch"][1]), B, C, N, hop, m, float(sr), stream())
        torch.cuda.synchronize()
        for k, (buf, inner) in bufs.items():
            assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
            assert torch.isfinite(inner).all() or (k == "gx" and not want_gx and torch.isnan(inner).all()), k
        return {k: inner.clone() for k, (buf, inner) in bufs.items()}

    zero, dirty, lean = run(0.0), run(float("nan")), run(0.0, save=False, want_gx=False)
    for k in zero:
        assert torch.equal(zero[k], dirty[k]), k
        assert k == "gx" or torch.equal(zero[k], lean[k]), k
    ref = run_t(D, a, sr, hop, mode)
    assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"])
    assert torch.equal(zero["gcutoff"].view(B, F), ref["gcutoff"]) and torch.equal(zero["gq"].view(B, F), ref["gq"]) and torch.equal(zero["gmix"], ref["gmix"])


def test_c_abi_errors_launch_nothing(D):
    """DASP_ERR_ARG / DASP_ERR_UNSUPPORTED with real device buffers: every output keeps its NaN fill, and the device has no error."""
    from dasp_pytorch_amd._lib import ptr, stream
    L = lib()
    B, C, N, hop = 2, 2, 300, 64
    a = plain(B, C, N)
    F = R.control_frames(N, hop)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    cut, q, mix = (a[k].to(DEV) for k in CTL)
    nan = lambda n: torch.full((n,), float("nan"), device=DEV)
    y, st, gx, gc, gq, gm, scr = nan(B * C * N), nan(B * C * 2), nan(B * C * N), nan(B * F), nan(B * F), nan(B), nan(B * C * (2 * F + 1))
    P = ptr

    def fwd(x_=x, y_=y, B_=B, hop_=hop, mode_=0, sr_=44100.0):
        return L.dasp_tvfilter_forward(P(x_), P(cut), P(q), P(mix), P(y_), P(st), B_, C, N, hop_, mode_, sr_, stream())

    def bwd(gy_=gy, scr_=scr, B_=B, hop_=hop, mode_=0, sr_=44100.0):
        return L.dasp_tvfilter_backward(P(x), P(cut), P(q), P(mix), P(st), P(gy_), P(gx), P(gc), P(gq), P(gm), P(scr_), B_, C, N, hop_, mode_, sr_, stream())
    assert fwd(x_=None) == -1 and fwd(y_=None) == -1 and fwd(B_=0) == -1 and fwd(hop_=0) == -1 and fwd(mode_=4) == -1 and fwd(sr_=float("nan")) == -1
    assert fwd(hop_=4) == -2 and fwd(hop_=48) == -2 and fwd(hop_=4096) == -2
    assert bwd(gy_=None) == -1 and bwd(scr_=None) == -1 and bwd(B_=-1) == -1 and bwd(mode_=-1) == -1 and bwd(sr_=0.0) == -1
    assert bwd(hop_=4) == -2 and bwd(hop_=4096) == -2
    torch.cuda.synchronize()
    for t in (y, st, gx, gc, gq, gm, scr):
        assert torch.isnan(t).all()
    assert L.dasp_device_error() == 0


def test_silence_in_silence_out(D):
    a = plain(2, 2, 2 * TILE + 5)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS)


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        F = R.control_frames(N, 64)
        ctl = [torch.ones(B, F, device=DEV, requires_grad=True), torch.ones(B, F, device=DEV, requires_grad=True), torch.ones(B, device=DEV, requires_grad=True)]
        y = D.time_varying_filter(x, 44100, *ctl)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


# ---- 8. what the forward pass leaves behind ------------------------------------------------------------------------------------------------
def test_forward_saves_the_tile_states_and_nothing_of_the_signals_length(D):
    """Beyond x, the curves and mix the forward pass keeps dasp_tvfilter_state_floats(rows, N) floats for backward - two per tile and
    row - and nothing at all when no input needs a gradient."""
    B, C, hop = 3, 2, 64
    N = 2 * TILE + 5
    a = plain(B, C, N)
    F = R.control_frames(N, hop)
    x = a["x"].to(DEV).requires_grad_(True)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = D.time_varying_filter(x, 44100, *ctl)
    nstate = lib().dasp_tvfilter_state_floats(B * C, N)
    assert nstate == B * C * 3 * 2
    assert sorted(t.numel() for t in saved) == sorted([B * C * N, B * F, B * F, B, nstate])
    assert any(t.data_ptr() == x.data_ptr() for t in saved)                     # x itself, not a copy
    y.sum().backward()
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.time_varying_filter(x.detach(), 44100, *[c.detach() for c in ctl])
    assert not saved


# ---- 9. double backward ------------------------------------------------------------------------------------------------------------------
def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.time_varying_filter(x, 44100, *[a[k].to(DEV) for k in CTL])
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 10. module --------------------------------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    sr, hop = 44100, 8
    x = plain(3, 2, 3000)["x"].to(DEV)
    F = R.control_frames(3000, hop)
    p = torch.rand(3, 2 * F + 1, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = D.TimeVaryingFilter(sr, hop=hop, mode="notch")
    with torch.no_grad():
        got = m.process_normalized(x, p)
        want = D.time_varying_filter(x, sr, p[:, :F] * 11950.0 + 50.0, p[:, F:2 * F] * 7.5 + 0.5, p[:, 2 * F], hop=hop, mode="notch")
    assert torch.equal(got, want)
