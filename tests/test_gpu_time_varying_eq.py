"""GPU tests of time_varying_eq (csrc/tveq.hip): parity of y, grad x and the three curve gradients with the float64 restatement
(tests/tveq_restated.py), the static case against the RBJ peaking and shelving biquads, a bell undone by its inverse, exact identities
(zero gain, equal neighbours, reproducibility, clamped frame values), the last frame point, a frame point on a tile boundary, NaN frame
values, views and guard words, the errors of the C ABI, what the forward pass saves, the refused double backward, the module, the
autograd and call-state batteries on a private spec, and the two compositions of the README.

Parity bounds, as for time_varying_filter (tests/test_gpu_tvfilter.py, whose reasoning applies word for word). The yardstick is the
restatement with float64 frame points and float32 arithmetic on the same inputs on the CPU: e32 = its error against float64 throughout,
relative to the peak of the float64 result over the case's items. The kernel's scan orders its products differently, so it gets 4 x e32,
and never less than the floors of tests/tvfilter_restated.py: 2e-6 of the peak for y and grad x, 1e-5 for the curve gradients. The op has
no atomics: wherever two results are compared, every quantity is compared bit for bit.

The restatement is a Python loop over samples, so it runs once per (rate, hop, mode): one batch of 6149 samples that holds every length
of the parity cases as an item group, cut as in tests/test_gpu_tvfilter.py. The curve gradients are taken per (item, channel) row, so that
the same run serves one channel (row 0) and two (the sum).
"""
import functools
import math

import numpy as np
import pytest
import scipy.signal
import torch

from tests import tveq_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTL = R.CTL
GRADS = R.GRADS
FLOOR = R.FLOOR
LANE, WAVE, TILE = 8, 512, 2048            # samples of a lane's run, of a wave's 64 runs and of a tile (csrc/tv_scan.hpp TV_SPT, TV_TILE)
LENGTHS = (1, 7, 8, 9, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5)
SETS = 3                                   # control sets per length: two draws of the main sweep, the hard set
MODE_INDEX = {m: i for i, m in enumerate(R.MODES)}


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    assert lib().dasp_tveq_tile() == TILE
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def curves(sr, B, F, g, hard=False):
    """The main sweep: gain uniform +-18 dB, log-uniform cutoff 50 Hz - 12 kHz, q 0.5 - 8, a draw per frame point. The hard set: gain
    +-24 dB, cutoff sr/4096 - 200 Hz, q 20 - 100. In the order of CTL."""
    u = lambda lo, hi: torch.exp(torch.rand(B, F, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))
    db = lambda a: torch.rand(B, F, generator=g) * 2 * a - a
    return (db(24.0), u(sr / 4096, 200.0), u(20.0, 100.0)) if hard else (db(18.0), u(50.0, 12000.0), u(0.5, 8.0))


def plain(B, C, N, hop=64, seed=0, sr=44100, hard=False):
    g = torch.Generator().manual_seed(91 * seed + 7 * B + 3 * C + N + hop)
    gain, cut, q = curves(sr, B, R.control_frames(N, hop), g, hard)
    return dict(x=torch.rand(B, C, N, generator=g) * 2 - 1, w=torch.randn(B, C, N, generator=g), gain_db=gain, cutoff_hz=cut, q=q)


def run_t(D, a, sr, hop=64, mode="bell", need_gx=True):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    y = D.time_varying_eq(x, sr, *ctl, hop=hop, mode=mode)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + ctl)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + GRADS, (y.detach(),) + grads))


def restated(a, sr, hop, mode, **kw):
    return R.forward_backward(a["x"], sr, a["gain_db"], a["cutoff_hz"], a["q"], a["w"], hop, mode, **kw)


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
    """The restatement's two runs for one (rate, hop, mode): inputs, float64 results and float32-arithmetic results, curve gradients per
    row. Computed once, read by the parity cases of both channel counts, never modified."""
    N, B = LENGTHS[-1], SETS * len(LENGTHS)
    F = R.control_frames(N, hop)
    g = torch.Generator().manual_seed(sr + 31 * hop + MODE_INDEX[mode])
    ctl = dict(zip(CTL, curves(sr, B, F, g)))
    for k, h in zip(CTL, curves(sr, B, F, g, hard=True)):
        ctl[k][2::SETS] = h[2::SETS]
    a = dict(ctl, x=torch.rand(B, 2, N, generator=g) * 2 - 1, w=torch.randn(B, 2, N, generator=g))
    for i, L in enumerate(LENGTHS):
        a["w"][SETS * i:SETS * (i + 1), :, L:] = 0
    return a, restated(a, sr, hop, mode, per_row=True), restated(a, sr, hop, mode, per_row=True, arith=torch.float32)


def cut_to(r, i, L, C, hop):
    """Group i of a restated result as the op with C channels, L samples and their frame points would give it."""
    s, F = slice(SETS * i, SETS * (i + 1)), R.control_frames(L, hop)
    return dict({"y": r["y"][s, :C, :L], "gx": r["gx"][s, :C, :L]}, **{k: r[k][s, :C, :F].sum(1) for k in GRADS})


@pytest.mark.parametrize("sr,hop,mode", [(44100, 64, "bell"), (44100, 8, "lowshelf"), (44100, 2048, "highshelf"), (8000, 2048, "bell"),
                                         (192000, 64, "lowshelf"), (8000, 8, "highshelf")])
def test_parity_with_the_float64_restatement(D, sr, hop, mode):
    a, want64, want32 = reference(sr, hop, mode)
    assert float(a["cutoff_hz"][2::SETS].max()) <= 200.0 and float(a["q"][2::SETS].min()) >= 20.0              # the hard set is what curves() says
    assert float(a["gain_db"][2::SETS].abs().max()) > 18.0 >= float(a["gain_db"][0::SETS].abs().max())
    worst = {k: 0.0 for k in R.NAMES}
    for i, L in enumerate(LENGTHS):
        s, F = slice(SETS * i, SETS * (i + 1)), R.control_frames(L, hop)
        for C in (1, 2):
            b = dict({k: a[k][s, :F].contiguous() for k in CTL}, x=a["x"][s, :C, :L].contiguous(), w=a["w"][s, :C, :L].contiguous())
            got = {k: v.cpu().numpy() for k, v in run_t(D, b, sr, hop, mode).items()}
            share = held(got, cut_to(want64, i, L, C, hop), cut_to(want32, i, L, C, hop), f"sr={sr} hop={hop} {mode} ({SETS},{C},{L})")
            record(f"tveq_parity sr={sr} hop={hop} mode={mode} ({SETS},{C},{L})", **{"share_" + k: v for k, v in share.items()})
            worst = {k: max(worst[k], share[k]) for k in R.NAMES}
    record(f"tveq_parity_worst sr={sr} hop={hop} mode={mode}", **{"share_" + k: v for k, v in worst.items()})


# ---- 2. the static case ------------------------------------------------------------------------------------------------------------------
STATIC = lambda sr: [(sr / 4096, 10.0, -24.0), (100.0, 0.7, 12.0), (1000.0, 4.0, -18.0), (0.45 * sr, 0.5, 24.0)]      # (f, Q, dB)


def constant(vals, F):
    """(gain_db, cutoff_hz, q) constant curves, one item per (f, Q, dB)."""
    return [torch.tensor([[v[i]] * F for v in vals], dtype=torch.float32) for i in (2, 0, 1)]


@pytest.mark.parametrize("mode", R.MODES)
def test_constant_curves_equal_the_float64_biquad(D, mode):
    """Constant curves against the RBJ biquad of scipy in float64 (tests/test_time_varying_eq_cpu.py holds the restatement to it at 1e-9):
    within max(4 e32, 2e-6) of the peak, e32 the float32-arithmetic restatement's error against the same biquad."""
    sr, N, hop = 44100, 2 * TILE + 5, 64
    F = R.control_frames(N, hop)
    x = torch.rand(4, 1, N, generator=torch.Generator().manual_seed(11)) * 2 - 1
    ctl = constant(STATIC(sr), F)
    with torch.no_grad():
        y = D.time_varying_eq(x.to(DEV), sr, *[c.to(DEV) for c in ctl], hop=hop, mode=mode).cpu().numpy()
        y32 = R.time_varying_eq(x, sr, *ctl, hop, mode, torch.float32).numpy()
    for b in range(4):
        db, f, q = (float(c[b, 0]) for c in ctl)
        want = scipy.signal.lfilter(*R.rbj(mode, f, q, db, sr), x[b, 0].double().numpy())
        e, e32 = peak_err(y[b, 0], want), peak_err(y32[b, 0], want)
        print(f"STATIC {mode} f={f:.1f} q={q:g} dB={db:g}: kernel {e:.3e} fp32 {e32:.3e}")
        record(f"tveq_static {mode} f={f:.1f} q={q:g} dB={db:g}", kernel=e, restated_fp32=e32)
        assert e <= max(4 * e32, FLOOR["y"]), (mode, b, e, e32)


def test_the_rbj_helper_is_signal_biquad(D):
    """The cookbook formulas of tests/tveq_restated.py rbj() against signal.biquad, the design parametric_eq is built from."""
    sr = 44100
    for mode, kind in zip(R.MODES, ("peaking", "low_shelf", "high_shelf")):
        for f, q, db in STATIC(sr)[1:]:
            b, a = D.signal.biquad(*[torch.tensor([v], dtype=torch.float64, device=DEV) for v in (db, f, q)], sr, kind)
            wb, wa = R.rbj(mode, f, q, db, sr)
            assert np.allclose(b[0].cpu().numpy(), wb / wa[0], rtol=1e-9, atol=1e-12) and np.allclose(a[0].cpu().numpy(), wa / wa[0], rtol=1e-9, atol=1e-12), (mode, f)


def test_a_bell_and_its_inverse_are_the_identity(D):
    """bell(+12 dB) then bell(-12 dB) with the same f and Q against x itself: within 4 x the error of the float32-arithmetic restatement's
    same two passes. Either error is measured against x, never against the other."""
    sr, N, hop = 44100, 2 * TILE + 5, 64
    F = R.control_frames(N, hop)
    x = torch.rand(4, 1, N, generator=torch.Generator().manual_seed(12)) * 2 - 1
    _, cut, q = constant(STATIC(sr), F)
    up, down = torch.full((4, F), 12.0), torch.full((4, F), -12.0)
    with torch.no_grad():
        dev = [t.to(DEV) for t in (cut, q)]
        y = D.time_varying_eq(D.time_varying_eq(x.to(DEV), sr, up.to(DEV), *dev, hop=hop), sr, down.to(DEV), *dev, hop=hop).cpu()
        mid = R.time_varying_eq(x, sr, up, cut, q, hop, "bell", torch.float32)
        y32 = R.time_varying_eq(mid, sr, down, cut, q, hop, "bell", torch.float32)
    e, e32 = peak_err(y.numpy(), x.numpy()), peak_err(y32.numpy(), x.numpy())
    print(f"BELL ROUND TRIP: kernel {e:.3e} fp32 {e32:.3e}")
    record("tveq_bell_round_trip", kernel=e, restated_fp32=e32)
    assert e <= 4 * e32, (e, e32)


# ---- 3. exact identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_zero_gain_is_the_identity_in_both_directions(D, mode):
    """A = 1 exactly: y = x and gx = gy bit for bit, while the gradient of gain_db is not zero."""
    a = plain(4, 2, 2 * TILE + 5)
    a["gain_db"] = torch.zeros_like(a["gain_db"])
    got = run_t(D, a, 44100, 64, mode)
    assert torch.equal(got["y"].cpu(), a["x"]) and torch.equal(got["gx"].cpu(), a["w"])
    assert got["ggain"].ne(0).float().mean() > 0.9 and torch.isfinite(got["ggain"]).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_curves_with_equal_neighbours_give_the_same_bits_at_every_hop(D, mode):
    """Constant curves: G_{j+1} - G_j = 0, so g, k and A are the frame values whatever t and hop are - y and gx agree bit for bit between
    the hops, and the frame gradients of either hop add up to the same total within the floor."""
    N = 2 * TILE + 5
    base = plain(3, 2, N, hop=8)
    out = {}
    for hop in (8, 64, 2048):
        F = R.control_frames(N, hop)
        out[hop] = run_t(D, dict(base, **{k: base[k][:, :1].expand(3, F).contiguous() for k in CTL}), 44100, hop, mode)
    for hop in (64, 2048):
        for k in ("y", "gx"):
            assert torch.equal(out[8][k], out[hop][k]), (hop, k)
        for k in GRADS:
            p, q = out[8][k].double().sum(1), out[hop][k].double().sum(1)
            assert ((p - q).abs() <= 1e-5 * out[8][k].double().abs().sum(1)).all(), (hop, k)


@pytest.mark.parametrize("hop", [8, 2048])
def test_runs_are_bit_identical(D, hop):
    a = plain(6, 2, 3 * TILE + 5, hop=hop)
    p, q = run_t(D, a, 44100, hop, "lowshelf"), run_t(D, a, 44100, hop, "lowshelf")
    for k in R.NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, hop, "lowshelf", need_gx=False)       # x needs no gradient: gx is not written, nothing else changes
    for k in ("y",) + GRADS:
        assert torch.equal(p[k], r[k]), k


@pytest.mark.parametrize("hop,mode", [(8, "bell"), (64, "lowshelf"), (2048, "highshelf")])
def test_item_alone_and_inside_a_batch(D, hop, mode):
    a = plain(4, 2, 3 * TILE + 5, hop=hop)
    whole = run_t(D, a, 44100, hop, mode)
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, hop, mode)
        for k in R.NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path and nothing to zero."""
    sr, hop = 44100, 64
    a = plain(4, 2, 3 * TILE + 5)
    eager = run_t(D, a, sr, hop, "highshelf")
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.time_varying_eq(xt, sr, *ctl, hop=hop, mode="highshelf")
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


# ---- 4. clamping, the last frame point, the tile boundary -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_clamped_frame_values_give_the_clamped_result_and_exactly_zero_gradients_there_and_only_there(D, mode):
    sr, hop, N = 44100, 64, TILE + 300
    a = plain(2, 2, N, seed=5)
    F = R.control_frames(N, hop)
    lo, hi = R.clamp_bounds(sr)
    out = {k: torch.zeros(2, F, dtype=torch.bool) for k in CTL}
    for k, cells in (("gain_db", [(0, 2), (0, 32), (1, 1), (1, F - 1)]), ("cutoff_hz", [(0, 3), (0, 32), (1, 0), (1, F - 1)]), ("q", [(0, 5), (1, 32), (1, 33)])):
        for c in cells:
            out[k][c] = True                                                    # frame point 32 is sample 2048
    b, c = ({k: v.clone() for k, v in a.items()} for _ in range(2))
    b["gain_db"][out["gain_db"]] = torch.tensor([41.0, -1e6, -40.5, 400.0])
    b["cutoff_hz"][out["cutoff_hz"]] = torch.tensor([1.0, 30000.0, 1e9, -5.0])
    b["q"][out["q"]] = torch.tensor([0.01, 1e4, 0.0])
    c["gain_db"][out["gain_db"]] = torch.tensor([40.0, -40.0, -40.0, 40.0])
    c["cutoff_hz"][out["cutoff_hz"]] = torch.tensor([lo, hi, hi, lo], dtype=torch.float64).float()
    c["q"][out["q"]] = torch.tensor([0.1, 100.0, 0.1])
    got, edge = run_t(D, b, sr, hop, mode), run_t(D, c, sr, hop, mode)
    for k, gk in zip(CTL, GRADS):
        assert torch.equal((got[gk] == 0).cpu(), out[k]), gk
    # float32(lo), float32(hi) may sit a rounding outside the float64 bounds and be clamped themselves: the same G, K, A either way
    for k in ("y", "gx"):
        assert torch.equal(got[k], edge[k]), k
    for k, gk in zip(CTL, GRADS):
        keep = ~out[k].to(DEV)
        assert torch.equal(got[gk][keep], edge[gk][keep]), gk


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_the_last_frame_point(D, hop):
    """Frame point F - 1 ends the last interval and takes t of its samples (tests/test_time_varying_eq_cpu.py): exactly zero when that
    interval holds one sample, the one on frame point F - 2 (seq_len = 1 mod hop), and the oracle's value when hop divides seq_len."""
    mode = {8: "bell", 64: "lowshelf", 2048: "highshelf"}[hop]
    for N in (2 * TILE + 1, 1):
        got = run_t(D, plain(2, 2, N, hop=hop, seed=2), 44100, hop, mode)
        for k in GRADS:
            assert not got[k][:, -1].any() and got[k][:, :-1].all(), (N, k)
    a = plain(2, 2, TILE, hop=hop, seed=2)
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, 44100, hop, mode).items()}
    want, f32 = restated(a, 44100, hop, mode), restated(a, 44100, hop, mode, arith=torch.float32)
    held(got, want, f32, f"last frame point hop={hop}")
    for k in GRADS:
        assert got[k][:, -1].all()
        assert np.abs(got[k][:, -1] - want[k][:, -1]).max() <= max(4 * peak_err(f32[k], want[k]), FLOOR[k]) * np.abs(want[k]).max(), k


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_a_frame_point_on_a_tile_boundary_matches_the_oracle(D, hop):
    """N = 4097: the upstream gradient lives on [1900, 2200) and [4000, 4097), so that the frame points at samples 2048 and 4096 take a half
    from either tile - the second tile boundary with a single sample beyond it."""
    N = 2 * TILE + 1
    mode = {8: "lowshelf", 64: "highshelf", 2048: "bell"}[hop]
    a = plain(2, 2, N, hop=hop, seed=4)
    a["w"][..., :1900] = 0
    a["w"][..., 2200:4000] = 0
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, 44100, hop, mode).items()}
    want, f32 = restated(a, 44100, hop, mode), restated(a, 44100, hop, mode, arith=torch.float32)
    held(got, want, f32, f"tile boundary hop={hop}")
    for j in (TILE // hop, 2 * TILE // hop):
        for k in GRADS:
            assert want[k][:, j].all() and got[k][:, j].all()
            assert np.abs(got[k][:, j] - want[k][:, j]).max() <= max(4 * peak_err(f32[k], want[k]), FLOOR[k]) * np.abs(want[k]).max(), (k, j)


# ---- 5. off the nominal domain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("which", CTL)
@pytest.mark.parametrize("hop,j", [(64, 0), (64, 1), (64, 40), (8, 300), (2048, 1), (2048, 2), (64, -1)])
def test_one_nan_frame_value_reaches_its_item_from_the_interval_before_it_and_nothing_else(D, which, hop, j, mode):
    """A NaN at frame point j of any curve: y of item 1 is NaN from sample (j - 1) hop on and keeps its bits before it; items 0 and 2 keep
    every bit of every result (tests/test_time_varying_eq_cpu.py shows the same reach for the restatement)."""
    N = 2 * TILE + 5
    a = plain(3, 2, N, hop=hop)
    clean = run_t(D, a, 44100, hop, mode)
    j = j % R.control_frames(N, hop)
    a[which][1, j] = float("nan")
    got = run_t(D, a, 44100, hop, mode)
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
    assert not torch.isfinite(dirty["y"][1]).any() and not torch.isfinite(dirty["ggain"][1]).any()
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = value
    dirty = run_t(D, b, 44100)
    for k in R.NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k
    assert torch.equal(clean["y"], dirty["y"]) and not torch.isfinite(dirty["ggain"][1, :-1]).any()       # (the last sample poisoned is 4074)


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * TILE + 5
    a = plain(3, 2, N)
    want = run_t(D, a, 44100, 64, "lowshelf")
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
        ctl = [torch.cat([a[k].to(DEV), torch.ones(3, 7, device=DEV)], -1)[:, :F].requires_grad_(True) for k in CTL]
        assert not ctl[0].is_contiguous()
    y = D.time_varying_eq(xv, 44100, *ctl, mode="lowshelf")
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    for k, g in zip(R.NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


@pytest.mark.parametrize("hop,mode", [(8, "bell"), (64, "lowshelf"), (2048, "highshelf")])
def test_c_abi_keeps_guard_words_and_ignores_dirty_scratch(D, hop, mode):
    """Through the C ABI: y, the states, gx, the three curve gradients and the scratch written inside NaN-filled guard words leave the
    guards NaN, NaN-filled state and scratch buffers give the same bits as zero-filled ones, and states = NULL / gx = NULL change nothing
    else."""
    from dasp_pytorch_amd._lib import call, ptr, stream
    sr, G = 44100, 64
    B, C = 3, 2
    N = 2 * TILE + 5
    m = MODE_INDEX[mode]
    a = plain(B, C, N, hop=hop)
    F = R.control_frames(N, hop)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    gain, cut, q = (a[k].to(DEV) for k in CTL)
    nstate, nscr = lib().dasp_tveq_state_floats(B * C, N), lib().dasp_tveq_scratch_floats(B * C, N, hop)
    assert nstate == B * C * 3 * 2 and nscr == B * C * 3 * F

    def guarded(n, fill=float("nan")):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        buf[G:G + n] = fill
        return buf, buf[G:G + n]

    def run(fill, save=True, want_gx=True):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("gx", B * C * N), ("ggain", B * F), ("gcutoff", B * F), ("gq", B * F))}
        bufs["states"], bufs["scratch"] = guarded(nstate, fill), guarded(nscr, fill)
        call("dasp_tveq_forward", ptr(x), ptr(gain), ptr(cut), ptr(q), ptr(bufs["y"][1]), ptr(bufs["states"][1] if save else None), B, C, N, hop, m, float(sr), stream())
        if not save:
            call("dasp_tveq_forward", ptr(x), ptr(gain), ptr(cut), ptr(q), ptr(torch.empty_like(x)), ptr(bufs["states"][1]), B, C, N, hop, m, float(sr), stream())
        call("dasp_tveq_backward", ptr(x), ptr(gain), ptr(cut), ptr(q), ptr(bufs["states"][1]), ptr(gy), ptr(bufs["gx"][1] if want_gx else None),
             ptr(bufs["ggain"][1]), ptr(bufs["gcutoff"][1]), ptr(bufs["gq"][1]), ptr(bufs["scratch"][1]), B, C, N, hop, m, float(sr), stream())
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
    for k in GRADS:
        assert torch.equal(zero[k].view(B, F), ref[k]), k


def test_c_abi_errors_launch_nothing(D):
    """DASP_ERR_ARG / DASP_ERR_UNSUPPORTED with real device buffers: every output keeps its NaN fill, and the device has no error."""
    from dasp_pytorch_amd._lib import ptr, stream
    L = lib()
    B, C, N, hop = 2, 2, 300, 64
    a = plain(B, C, N)
    F = R.control_frames(N, hop)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    gain, cut, q = (a[k].to(DEV) for k in CTL)
    nan = lambda n: torch.full((n,), float("nan"), device=DEV)
    y, st, gx, gg, gc, gq, scr = nan(B * C * N), nan(B * C * 2), nan(B * C * N), nan(B * F), nan(B * F), nan(B * F), nan(B * C * 3 * F)
    P = ptr

    def fwd(x_=x, y_=y, B_=B, hop_=hop, mode_=0, sr_=44100.0):
        return L.dasp_tveq_forward(P(x_), P(gain), P(cut), P(q), P(y_), P(st), B_, C, N, hop_, mode_, sr_, stream())

    def bwd(gy_=gy, scr_=scr, B_=B, hop_=hop, mode_=0, sr_=44100.0):
        return L.dasp_tveq_backward(P(x), P(gain), P(cut), P(q), P(st), P(gy_), P(gx), P(gg), P(gc), P(gq), P(scr_), B_, C, N, hop_, mode_, sr_, stream())
    assert fwd(x_=None) == -1 and fwd(y_=None) == -1 and fwd(B_=0) == -1 and fwd(hop_=0) == -1 and fwd(mode_=3) == -1 and fwd(sr_=float("nan")) == -1
    assert fwd(hop_=4) == -2 and fwd(hop_=48) == -2 and fwd(hop_=4096) == -2
    assert bwd(gy_=None) == -1 and bwd(scr_=None) == -1 and bwd(B_=-1) == -1 and bwd(mode_=-1) == -1 and bwd(sr_=0.0) == -1
    assert bwd(hop_=4) == -2 and bwd(hop_=4096) == -2
    torch.cuda.synchronize()
    for t in (y, st, gx, gg, gc, gq, scr):
        assert torch.isnan(t).all()
    assert L.dasp_device_error() == 0


@pytest.mark.parametrize("mode", R.MODES)
def test_silence_in_silence_out(D, mode):
    a = plain(2, 2, 2 * TILE + 5)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100, 64, mode)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS)


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        F = R.control_frames(N, 64)
        ctl = [torch.ones(B, F, device=DEV, requires_grad=True) for _ in CTL]
        y = D.time_varying_eq(x, 44100, *ctl)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_and_bfloat16_are_converted(D, dtype):
    a = plain(2, 2, 700)
    x = a["x"].to(DEV).to(dtype)
    ctl = [a[k].to(DEV) for k in CTL]
    with torch.no_grad():
        y = D.time_varying_eq(x, 44100, *ctl)
        want = D.time_varying_eq(x.float(), 44100, *ctl)
    assert y.dtype is dtype and torch.equal(y, want.to(dtype))


# ---- 6. what the forward pass leaves behind ------------------------------------------------------------------------------------------------
def test_forward_saves_the_tile_states_and_nothing_of_the_signals_length(D):
    """Beyond x and the curves the forward pass keeps dasp_tveq_state_floats(rows, N) floats for backward - two per tile and row - and
    nothing at all when no input needs a gradient."""
    B, C, hop = 3, 2, 64
    N = 2 * TILE + 5
    a = plain(B, C, N)
    F = R.control_frames(N, hop)
    x = a["x"].to(DEV).requires_grad_(True)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = D.time_varying_eq(x, 44100, *ctl)
    nstate = lib().dasp_tveq_state_floats(B * C, N)
    assert nstate == B * C * 3 * 2
    assert sorted(t.numel() for t in saved) == sorted([B * C * N, B * F, B * F, B * F, nstate])
    assert any(t.data_ptr() == x.data_ptr() for t in saved)                     # x itself, not a copy
    y.sum().backward()
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.time_varying_eq(x.detach(), 44100, *[c.detach() for c in ctl])
    assert not saved


def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.time_varying_eq(x, 44100, *[a[k].to(DEV) for k in CTL])
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


def test_module_equals_functional(D):
    sr, hop = 44100, 8
    x = plain(3, 2, 3000)["x"].to(DEV)
    F = R.control_frames(3000, hop)
    p = torch.rand(3, 3 * F, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = D.TimeVaryingEQ(sr, hop=hop, mode="lowshelf")
    with torch.no_grad():
        got = m.process_normalized(x, p)
        want = D.time_varying_eq(x, sr, p[:, :F] * 48.0 - 24.0, p[:, F:2 * F] * 11950.0 + 50.0, p[:, 2 * F:] * 7.5 + 0.5, hop=hop, mode="lowshelf")
    assert torch.equal(got, want)


# ---- 7. the autograd and call-state contracts -----------------------------------------------------------------------------------------------
def _spec():
    """The op's entry for the contract batteries, in the form of the entries of tests/autograd_contract_cases.py (that table is closed:
    tests/test_call_state_cpu.py pins its size). What is watched is TimeVaryingEQKernels, the class that holds the forward / backward
    pair that TimeVaryingEQFunction binds to autograd."""
    from dasp_pytorch_amd._ctypes_ops import TimeVaryingEQKernels
    from tests import autograd_contract_cases as A
    sr, hop, N, mode = 8000, 64, 1501, "lowshelf"
    F = R.control_frames(N, hop)

    def arrays(seed):
        g = A.gen(seed, 181)
        u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
        return dict(x=u(-1.0, 1.0, 3, 2, N), gain_db=u(-18.0, 18.0, 3, F), cutoff_hz=u(100.0, 3000.0, 3, F), q=u(0.5, 8.0, 3, F))

    def call(t):
        import dasp_pytorch_amd
        return dasp_pytorch_amd.time_varying_eq(t["x"], sr, *[t[k] for k in CTL], hop=hop, mode=mode)

    names = dict(zip(R.NAMES, ("y0", "g_x") + tuple("g_" + k for k in CTL)))

    def ref(a, gys):
        w = torch.from_numpy(gys[0])
        r64 = R.forward_backward(a["x"], sr, *[a[k] for k in CTL], w, hop, mode)
        r32 = R.forward_backward(a["x"], sr, *[a[k] for k in CTL], w, hop, mode, arith=torch.float32)
        bound = {names[k]: max(4.0 * peak_err(r32[k], r64[k]), FLOOR[k]) for k in names}
        return dict({names[k]: r64[k] for k in names}, _bound=bound)
    spec = A.measured_bound("time_varying_eq", arrays, call, ("x",) + CTL, ("x",), ("TimeVaryingEQKernels",), ref, {names[k]: FLOOR[k] for k in names},
                            forms={k: "matrix" for k in CTL}, lowp=("x",), cite="tests/test_gpu_time_varying_eq.py test_parity_with_the_float64_restatement")
    spec.functions = lambda: [TimeVaryingEQKernels]
    return spec


def _contract(checks, check):
    spec, rec = _spec(), []
    try:
        find = checks[check](spec, rec)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in time_varying_eq {check}: {e}", returncode=3)        # nothing more runs on a device that has faulted
        raise
    torch.cuda.synchronize()
    assert lib().dasp_device_error() == 0
    assert not find, "\n".join(find)


@pytest.mark.parametrize("check", ["C1_subsets", "C2_repeat", "C3_interleave", "C4_upstream_forms", "C5_leaf_forms", "C6_mutation", "C7_streams"])
def test_autograd_contract(D, check):
    from tests import autograd_contract_checks as C
    _contract(C.CHECKS, check)


@pytest.mark.parametrize("check", ["S1_arguments", "S4_memory"])
def test_call_state(D, check):
    from tests import call_state_checks as S
    _contract(S.CHECKS, check)


# ---- 8. the compositions of the README -------------------------------------------------------------------------------------------------------
def band_db(t, sr, lo, hi):
    """Energy of t (..., N) between lo and hi Hz, in dB, per leading index."""
    S = torch.fft.rfft(t.double(), dim=-1).abs().pow(2)
    f = torch.fft.rfftfreq(t.shape[-1], 1.0 / sr).to(t.device)
    return 10 * torch.log10(S[..., (f >= lo) & (f <= hi)].sum(-1))


def test_de_esser_composition(D):
    """README "Dynamic EQ": high-pass x, follow its envelope, turn the level above a threshold into a cut, apply it as a bell at 6.5 kHz.
    Two items that differ only in the level of their sibilance (noise between 5 and 8 kHz over a 200 Hz tone): the louder one's 5 - 8 kHz
    band is reduced by more dB. Finite gradients reach the audio and smoothing_ms."""
    sr, hop, N = 44100, 64, 8192
    g = torch.Generator().manual_seed(21)
    n = torch.arange(N) / sr
    S = torch.fft.rfft(torch.randn(N, generator=g))
    f = torch.fft.rfftfreq(N, 1.0 / sr)
    S[(f < 5000) | (f > 8000)] = 0
    ess = torch.fft.irfft(S, n=N)
    ess = ess / ess.abs().max()
    voice = 0.3 * torch.sin(2 * math.pi * 200.0 * n)
    x = torch.stack([voice + 0.1 * ess, voice + 0.4 * ess])[:, None, :].to(DEV).requires_grad_(True)
    sm = torch.tensor([5.0, 5.0], device=DEV, requires_grad=True)
    F = D.control_frames(N, hop)
    const = lambda v: torch.full((2, F), v, device=DEV)
    thr, r = -40.0, 0.75

    side = D.time_varying_filter(x, sr, const(5000.0), const(0.707), torch.ones(2, device=DEV), hop=hop, mode="highpass")
    level_db = 20 * torch.log10(D.envelope_follower(side, sr, sm, hop=hop) + 1e-5)
    cut_db = -r * torch.relu(level_db - thr)
    y = D.time_varying_eq(x, sr, cut_db, const(6500.0), const(2.0), hop=hop, mode="bell")

    gx, gs = torch.autograd.grad(y.pow(2).sum(), [x, sm])
    assert y.shape == x.shape and all(torch.isfinite(t).all() for t in (y, gx, gs)) and gs.ne(0).all()
    depth = cut_db.detach()
    assert float(depth.max()) <= 0.0 and float(depth[1].min()) < float(depth[0].min()) < 0.0
    cut = band_db(x.detach()[:, 0], sr, 5000, 8000) - band_db(y.detach()[:, 0], sr, 5000, 8000)
    low = band_db(x.detach()[:, 0], sr, 100, 400) - band_db(y.detach()[:, 0], sr, 100, 400)
    record("tveq_de_esser", cut_db_quiet=float(cut[0]), cut_db_loud=float(cut[1]), low_band_change_db=float(low.abs().max()))
    assert float(cut[1]) > float(cut[0]) + 1.0 > 1.0 and float(low.abs().max()) < 0.1


def test_eq_automation_composition(D):
    """README "EQ automation": a high shelf whose gain ramps from 0 to -12 dB over the clip. The start is untouched to rounding, the end has
    lost 12 dB above the shelf, and finite gradients reach the audio and every frame value of the ramp."""
    sr, hop, N = 44100, 64, 16384
    g = torch.Generator().manual_seed(22)
    x = (0.3 * torch.randn(2, 2, N, generator=g)).to(DEV).requires_grad_(True)
    F = D.control_frames(N, hop)
    ramp = torch.linspace(0.0, -12.0, F, device=DEV).expand(2, -1).clone().requires_grad_(True)
    const = lambda v: torch.full((2, F), v, device=DEV)
    y = D.time_varying_eq(x, sr, ramp, const(4000.0), const(0.707), hop=hop, mode="highshelf")
    gx, gr = torch.autograd.grad(y.pow(2).sum(), [x, ramp])
    assert y.shape == x.shape and all(torch.isfinite(t).all() for t in (y, gx, gr)) and gr[:, :-1].ne(0).all()
    head, tail = slice(0, 2048), slice(N - 2048, N)
    lost = band_db(x.detach()[..., tail], sr, 10000, 20000) - band_db(y.detach()[..., tail], sr, 10000, 20000)
    kept = band_db(x.detach()[..., head], sr, 10000, 20000) - band_db(y.detach()[..., head], sr, 10000, 20000)
    record("tveq_eq_automation", lost_db_tail=float(lost.mean()), lost_db_head=float(kept.mean()))
    assert float((lost - 11.0).abs().max()) < 1.5 and float(kept.abs().max()) < 1.5 and float(kept.max()) < float(lost.min())
