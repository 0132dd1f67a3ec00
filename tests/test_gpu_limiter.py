"""GPU tests of limiter (csrc/limiter.hip): parity of y, grad x, both control gradients and the saved winners with the float64
restatement (tests/limiter_restated.py) on the cases of tests/limiter_cases.py, the ceiling, exact identities, closed forms of one
impulse, ties, the link of the channels, clamped controls, the adjoint, bit-for-bit reproducibility, what happens off the nominal
domain, what the forward pass leaves behind, the refused
double backward and the module. The autograd and call-state contracts run on the op's entry in tests/autograd_contract_cases.py.

Parity bounds, the house rule of the phaser and the swept filter: the yardstick is the restatement in float32 arithmetic on the same
inputs, e32 = its error against float64 relative to the peak of the float64 result, per case over its items; the kernel gets 4 x e32
and never less than 2e-6 of the peak for y and grad x and 1e-5 for the control gradients. The winners are compared exactly: the
cases are chosen (tests/test_limiter_cpu.py) so that no decision is closer than 1e-4. The op has no atomics: wherever two results are
compared, every quantity is compared bit for bit.

The restatement is a Python loop over samples, so it runs once per case on one batch that holds every length as an item, zero from
its length on - the definition's own padding.
"""
import numpy as np
import pytest
import torch

from tests import limiter_cases as K
from tests import limiter_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTL, GRADS, NAMES = R.CTL, R.GRADS, R.NAMES
FLOOR = R.FLOOR
T = K.TILE


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    assert lib().dasp_limiter_tile() == T and lib().dasp_limiter_max_lookahead() == K.MAX_LOOKAHEAD
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def run_t(D, a, sr, L, need_gx=True, saved=None):
    x = a["x"].to(DEV).requires_grad_(need_gx)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    if saved is None:
        y = D.limiter(x, sr, *ctl, lookahead_ms=K.lookahead_ms(sr, L))
    else:
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            y = D.limiter(x, sr, *ctl, lookahead_ms=K.lookahead_ms(sr, L))
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), ([x] if need_gx else []) + ctl)
    torch.cuda.synchronize()
    return dict(zip(("y",) + (("gx",) if need_gx else ()) + GRADS, (y.detach(),) + grads))


def winners(saved):
    (w,) = [t for t in saved if t.dtype == torch.int32]
    return w.cpu().numpy()


def plain(B, C, N, seed=0, sr=44100):
    """Noise under a log-normal envelope, thresholds of -20 .. -8 dB, releases of 30 .. 4000 samples: about half of the samples limited."""
    g = torch.Generator().manual_seed(97 * seed + 7 * B + 3 * C + N)
    env = torch.exp(0.8 * torch.randn(B, 1, (N + 47) // 48, generator=g)).repeat_interleave(48, -1)[..., :N]
    u = lambda lo, hi: torch.rand(B, generator=g) * (hi - lo) + lo
    return dict(x=0.35 * torch.randn(B, C, N, generator=g) * env, w=torch.randn(B, C, N, generator=g), threshold_db=u(-20.0, -8.0),
                release_ms=torch.exp(u(np.log(30.0), np.log(4000.0))) / sr * 1000.0)


def ceiling(thr):
    return 10.0 ** (np.clip(np.asarray(thr, np.float64), -120.0, 40.0) / 20.0)


def case_results(D, cfg):
    """The kernel on every item of a case, each cut to its length: what it gives, what both restatements give, the winners."""
    sr, L, C, seed = cfg
    a, want64, want32 = K.reference(*cfg)
    rows = []
    for q, n in enumerate(K.lengths(L)):
        b = {k: v[q:q + 1] for k, v in a.items()}
        b["x"], b["w"] = b["x"][:, :, :n].contiguous(), b["w"][:, :, :n].contiguous()
        saved = []
        got = {k: v.cpu().numpy() for k, v in run_t(D, b, sr, L, saved=saved).items()}
        cut = lambda r: dict(y=r["y"][q:q + 1, :, :n], gx=r["gx"][q:q + 1, :, :n], gthr=r["gthr"][q:q + 1], grel=r["grel"][q:q + 1])
        rows.append(dict(n=n, got=got, want=cut(want64), f32=cut(want32), w=winners(saved)[0], w_want=want64["w"][q, L:L + n],
                         thr=float(a["threshold_db"][q])))
    return rows


_RESULTS = {}


def results(D, cfg):
    if cfg not in _RESULTS:
        _RESULTS[cfg] = case_results(D, cfg)
    return _RESULTS[cfg]


IDS = lambda c: "sr%d-L%d-C%d" % c[:3]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", K.CONFIGS, ids=IDS)
def test_parity_with_the_float64_restatement(D, cfg):
    rows = results(D, cfg)
    cat = lambda key, k: np.concatenate([np.asarray(r[key][k], np.float64).reshape(-1) for r in rows])
    e, e32, share = {}, {}, {}
    for k in NAMES:
        e[k], e32[k] = peak_err(cat("got", k), cat("want", k)), peak_err(cat("f32", k), cat("want", k))
        share[k] = e[k] / max(4 * e32[k], FLOOR[k])
    record("limiter_parity sr=%d L=%d C=%d" % cfg[:3], **e, **{"fp32_" + k: v for k, v in e32.items()}, **{"share_" + k: v for k, v in share.items()})
    for r in rows:
        assert r["got"]["y"].shape == r["want"]["y"].shape and r["got"]["gx"].shape == r["want"]["gx"].shape
        assert np.array_equal(r["w"], r["w_want"]), (cfg, r["n"], np.flatnonzero(r["w"] != r["w_want"])[:5])
    for k in NAMES:
        assert e[k] <= max(4 * e32[k], FLOOR[k]), (cfg, k, e[k], e32[k])


# ---- 2. the ceiling ------------------------------------------------------------------------------------------------------------------------
def test_ceiling(D):
    """max|y| <= 10^(thr/20) (1 + m) over all parity inputs and a full-scale square wave; m is 4 x the float32 restatement's own
    overshoot on the same inputs and never less than 2^-20."""
    over = over32 = 0.0
    for cfg in K.CONFIGS:
        for r in results(D, cfg):
            c = ceiling(np.float32(r["thr"]))
            over = max(over, float(np.abs(r["got"]["y"]).max() / c - 1))
            over32 = max(over32, float(np.abs(r["f32"]["y"]).max() / c - 1))
    sr, L, N = 8000, 64, T + 5
    sq = dict(x=((-1.0) ** torch.arange(N)).expand(2, 2, N).contiguous(), w=torch.ones(2, 2, N), threshold_db=torch.tensor([-0.1, -18.0]),
              release_ms=torch.tensor([50.0, 5.0]))
    y = run_t(D, sq, sr, L)["y"].cpu().numpy()
    y32 = R.forward_backward(sq["x"], sr, sq["threshold_db"], sq["release_ms"], sq["w"], lookahead=L, arith=torch.float32)["y"]
    c = ceiling(sq["threshold_db"].numpy())[:, None, None]
    over, over32 = max(over, float((np.abs(y) / c).max() - 1)), max(over32, float((np.abs(y32) / c).max() - 1))
    m = max(4 * over32, 2.0 ** -20)
    record("limiter_ceiling", overshoot=over, restated_fp32=over32, margin=m)
    assert over <= m, (over, over32)
    assert float((np.abs(y) / c).min()) >= 1 - 2e-6                       # a square wave above its threshold sits on the ceiling


# ---- 3. identities -------------------------------------------------------------------------------------------------------------------------
def test_item_below_its_threshold_comes_back_bit_for_bit(D):
    a = plain(4, 2, 2 * T + 5)
    a["x"][2] = a["x"][2].clamp(-0.2, 0.2)
    a["threshold_db"][2] = -12.0                                          # 0.2 < 10^(-12/20) = 0.251
    got = run_t(D, a, 44100, 220)
    assert torch.equal(got["y"][2].cpu(), a["x"][2]) and torch.equal(got["gx"][2].cpu(), a["w"][2])
    assert got["gthr"][2] == 0 and got["grel"][2] == 0
    assert not torch.equal(got["y"][1].cpu(), a["x"][1])


def test_silence_in_silence_out(D):
    a = plain(2, 2, 2 * T + 5)
    a["x"] = torch.zeros_like(a["x"])
    got = run_t(D, a, 44100, 220)
    assert not got["y"].any() and all(torch.isfinite(v).all() for v in got.values())
    assert not any(got[k].any() for k in GRADS) and torch.equal(got["gx"].cpu(), a["w"])


def test_empty_input(D):
    for B, C, N in ((2, 2, 0), (0, 2, 16)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        ctl = [torch.ones(B, device=DEV, requires_grad=True) for _ in range(2)]
        y = D.limiter(x, 44100, *ctl)
        assert y.shape == (B, C, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)


# ---- 4. one impulse in silence: closed forms -------------------------------------------------------------------------------------------------
def closed_gain(N, L, n0, r0, rho):
    """G[n + L] for one sample of required reduction r0 at n0: e is r0 over [n0, n0 + L] and r0 rho^k after it, s the box."""
    m = np.arange(-L, N + L, dtype=np.float64)
    e = np.where(m < n0, 0.0, np.where(m <= n0 + L, r0, r0 * rho ** np.maximum(m - n0 - L, 0.0)))
    c = np.concatenate([[0.0], np.cumsum(e)])
    s = (c[L + 1:] - c[:-L - 1]) / (L + 1)                                # s[m], m = 0 .. N + L - 1
    return 10.0 ** (-s[L:] / 20.0), s[L:]


def impulse_case(D, N, L, n0, sr, rel_ms, probe):
    """Channel 0: the impulse, 1.0 over a threshold of -12 dB. Channel 1: `probe`, below the threshold, which reads the gain out."""
    x = torch.zeros(1, 2, N)
    x[0, 0, n0] = 1.0
    x[0, 1] = probe
    x[0, 1, n0] = 0.0
    a = dict(x=x, w=torch.ones(1, 2, N), threshold_db=torch.tensor([-12.0]), release_ms=torch.tensor([rel_ms]))
    saved = []
    got = run_t(D, a, sr, L, saved=saved)
    rho = float(np.exp(-R.LN9 / (sr * float(np.float32(rel_ms)) / 1000.0)))
    G, s = closed_gain(N, L, n0, 12.0, rho)
    return got["y"][0].cpu().numpy().astype(np.float64), winners(saved)[0], G, s, x[0].numpy().astype(np.float64)


@pytest.mark.parametrize("L", [0, 1, 64, 220])
@pytest.mark.parametrize("where", ["first", "tile_end", "tile_start", "last", "hold_j0", "hold_j1", "hold_jL-1", "hold_jL"])
def test_one_impulse_in_silence(D, where, L):
    """A linear-in-dB ramp over L samples, the peak at exactly the ceiling, a hold of L and a release as rho^k - where the look-ahead
    reaches before sample 0 (first) or into the padding (last), and where the hold window lies across a tile boundary (a peak at
    T - 1 - j). 2e-6 of the gain: r, e and G are each rounded once to float32 (1e-7 each at 12 dB), the product once more."""
    N = 2 * T + 5
    n0 = {"first": 0, "tile_end": T - 1, "tile_start": T, "last": N - 1, "hold_j0": T - 1, "hold_j1": T - 2, "hold_jL-1": T - 1 - max(L - 1, 0),
          "hold_jL": T - 1 - L}[where]
    y, w, G, s, x = impulse_case(D, N, L, n0, 8000, 20.0, 2.0 ** -7)
    assert abs(y[0, n0] / ceiling(-12.0) - 1) <= 2e-6 and abs(G[n0] / ceiling(-12.0) - 1) <= 1e-14
    assert np.abs(y[1] - x[1] * G).max() <= 2e-6 * 2.0 ** -7
    assert np.array_equal(y[1, :max(n0 - L, 0)], x[1, :max(n0 - L, 0)])    # before the ramp: untouched, bit for bit
    if L and n0 >= L:                                                      # the ramp is linear in dB: s rises by 12 / (L + 1) a sample
        got_s = -20.0 * np.log10(y[1, n0 - L:n0] * 2.0 ** 7)
        assert np.abs(got_s - 12.0 * np.arange(1, L + 1) / (L + 1)).max() <= 2e-5
    want_w = np.where(np.arange(N) + L >= n0, n0, -1)
    assert np.array_equal(w, want_w)


def test_release_across_three_tiles(D):
    """One impulse, then noise below the threshold for more than 3 T samples under a release of one second: every winner is the impulse
    and the gain is the closed form."""
    sr, L, N, n0 = 8000, 40, 3 * T + 300, 10
    g = torch.Generator().manual_seed(5)
    probe = (torch.rand(N, generator=g) * 2 - 1) * 0.2
    y, w, G, s, x = impulse_case(D, N, L, n0, sr, 1000.0, probe)
    assert np.array_equal(w, np.where(np.arange(N) + L >= n0, n0, -1))
    assert np.abs(y - x * G).max() <= 2e-6
    assert 0.5 < s[-1] < 6.0                                                # still releasing at the end


# ---- 5. ties and the link ------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_latest_sample_and_the_lowest_channel(D):
    sr, L, N = 8000, 5, T + 37
    x = (0.8 * (-1.0) ** torch.arange(N)).expand(2, 2, N).contiguous().clone()
    x[1, 1] *= 0.5                                                          # item 1: channel 0 alone has the peak
    g = torch.Generator().manual_seed(2)
    a = dict(x=x, w=torch.randn(2, 2, N, generator=g), threshold_db=torch.tensor([-12.0, -9.0]), release_ms=torch.tensor([20.0, 5.0]))
    saved = []
    got = run_t(D, a, sr, L, saved=saved)
    w = winners(saved)
    assert np.array_equal(w, np.broadcast_to(np.minimum(np.arange(N) + L, N - 1), (2, N)))
    args = (a["x"], sr, a["threshold_db"], a["release_ms"], a["w"])
    r64, r32 = R.forward_backward(*args, lookahead=L), R.forward_backward(*args, lookahead=L, arith=torch.float32)
    assert (r64["cs"] == 0).all() and np.array_equal(r64["w"][:, L:], w)
    for k in NAMES:
        assert peak_err(got[k].cpu().numpy(), r64[k]) <= max(4 * peak_err(r32[k], r64[k]), FLOOR[k]), k
    G = got["y"][0, 1].cpu().double() / a["x"][0, 1].double()
    assert (got["gx"][0, 1].cpu().double() - a["w"][0, 1].double() * G).abs().max() <= 2e-6 * float(a["w"].abs().max())     # channel 1: the direct term alone


def test_channels_are_linked(D):
    """A peak in channel 1 alone gives the same gain on every channel: the probes 2^-7 and 2^-6 come back in the ratio 2, bit for bit."""
    a = plain(2, 3, 2 * T + 5)
    a["x"][:, 0], a["x"][:, 2] = 2.0 ** -7, 2.0 ** -6
    a["x"][:, 1] = a["x"][:, 1] + 0.05 * torch.sign(a["x"][:, 1])
    got = run_t(D, a, 44100, 220)
    y = got["y"].cpu()
    assert torch.equal(y[:, 2], 2 * y[:, 0]) and (y[:, 0] < 2.0 ** -7).any()
    r = R.forward_backward(a["x"], 44100, a["threshold_db"], a["release_ms"], a["w"], lookahead=220)
    assert np.abs(y[:, 0].double().numpy() * 2.0 ** 7 - r["G"]).max() <= 2e-6


# ---- 6. clamped controls -------------------------------------------------------------------------------------------------------------------
def test_clamped_controls(D):
    a = plain(7, 2, T + 300, sr=8000)
    a["threshold_db"] = torch.tensor([-130.0, 45.0, -12.0, -12.0, -12.0, -120.0, 40.0])
    a["release_ms"] = torch.tensor([50.0, 50.0, 0.05, 20000.0, 50.0, 0.1, 10000.0])
    got = run_t(D, a, 8000, 40)
    b = dict(a, threshold_db=a["threshold_db"].clamp(-120, 40), release_ms=a["release_ms"].clamp(0.1, 10000))
    want = run_t(D, b, 8000, 40)
    for k in ("y", "gx"):
        assert peak_err(got[k].cpu().numpy(), want[k].cpu().numpy()) <= FLOOR[k], k
    assert torch.equal(got["y"][:2], want["y"][:2]) and torch.equal(got["y"][4:], want["y"][4:])
    gt, gr = got["gthr"].cpu().numpy(), got["grel"].cpu().numpy()
    assert gt[0] == 0 and gt[1] == 0 and all(gt[q] != 0 for q in (2, 3, 4, 5))          # exactly zero where clamped - and only there
    assert gr[2] == 0 and gr[3] == 0 and gr[4] != 0 and want["grel"][3] != 0
    assert gt[5] == want["gthr"][5] and gr[6] == want["grel"][6]                          # on the edge of the range: not clamped


# ---- 7. adjoint ----------------------------------------------------------------------------------------------------------------------------
def test_adjoint(D):
    """The dot-product test in the form this op admits. It is not linear in x, but limiter(a x; thr + 20 log10 a) = a limiter(x; thr), and
    the derivative of that at a = 1 is <gx, x> + (20 / ln 10) g_threshold_db = <w, y> per item: y, gx and the control gradient of one
    call against each other, all sums in float64 on the host. The relative difference is within 4 x that of the float32 restatement
    (at 700 samples, where the loop is quick) and never above 1e-5."""
    sr, L = 44100, 220
    a, small = plain(4, 2, 2 * T + 5), plain(4, 2, 700)
    g = torch.Generator().manual_seed(77)

    def rel(x, w, y, gx, gthr):
        f = lambda t: np.asarray(t, np.float64)
        lhs = (f(gx) * f(x)).sum((1, 2)) + 20.0 / np.log(10.0) * f(gthr)
        rhs = (f(w) * f(y)).sum((1, 2))
        return float((np.abs(lhs - rhs) / np.abs(f(w) * f(y)).sum((1, 2))).max())
    got, want = [], []
    for _ in range(4):
        a["w"], small["w"] = torch.randn(a["x"].shape, generator=g), torch.randn(small["x"].shape, generator=g)
        k = {n: v.cpu().numpy() for n, v in run_t(D, a, sr, L).items()}
        got.append(rel(a["x"], a["w"], k["y"], k["gx"], k["gthr"]))
        r = R.forward_backward(small["x"], sr, small["threshold_db"], small["release_ms"], small["w"], lookahead=L, arith=torch.float32)
        want.append(rel(small["x"], small["w"], r["y"].astype(np.float32), r["gx"].astype(np.float32), r["gthr"].astype(np.float32)))
    record("limiter_adjoint", kernel=max(got), restated_fp32=max(want))
    assert max(got) <= max(4 * max(want), 1e-6) and max(got) <= 1e-5, (got, want)


# ---- 8. reproducibility: everything bit for bit ----------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(D):
    a = plain(6, 2, 2 * T + 5)
    p, q = run_t(D, a, 44100, 220), run_t(D, a, 44100, 220)
    for k in NAMES:
        assert torch.equal(p[k], q[k]), k
    r = run_t(D, a, 44100, 220, need_gx=False)       # x needs no gradient: gx is not written, nothing else changes
    for k in ("y",) + GRADS:
        assert torch.equal(p[k], r[k]), k
    with torch.no_grad():                            # nothing saved: the same y
        y = D.limiter(a["x"].to(DEV), 44100, a["threshold_db"].to(DEV), a["release_ms"].to(DEV))
    assert torch.equal(y, p["y"])


def test_item_alone_and_inside_a_batch(D):
    a = plain(5, 2, 2 * T + 5)
    whole = run_t(D, a, 44100, 220)
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, 220)
        for k in NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


def test_graph_replay_equals_eager(D):
    """One forward + backward step captured on a single stream: no host synchronisation in the call path, the scratch zeroed by a kernel
    of the call, and the LDS limit raised when the library was loaded."""
    sr = 44100
    a = plain(4, 2, 2 * T + 5)
    eager = run_t(D, a, sr, 220)
    xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]

    def step():
        y = D.limiter(xt, sr, *ctl)
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
        for key, o in zip(NAMES, outs):
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 9. off the nominal domain -------------------------------------------------------------------------------------------------------------
def _item0_unchanged(clean, dirty):
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]), k


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e30])
def test_poisoned_audio_stays_in_its_item(D, value):
    a = plain(2, 2, 2 * T + 5)
    clean = run_t(D, a, 44100, 220)
    b = {k: v.clone() for k, v in a.items()}
    b["x"][1, :, ::97] = value
    dirty = run_t(D, b, 44100, 220)
    _item0_unchanged(clean, dirty)
    if value == 1e30:                                  # finite: the ceiling holds for it too (half an ulp of r at 600 dB is 3e-5 dB: 3.5e-6)
        assert torch.isfinite(dirty["y"][1]).all() and float(dirty["y"][1].abs().max()) <= float(ceiling(b["threshold_db"][1])) * (1 + 1e-5)


def test_nan_controls_and_upstream_gradients_stay_in_their_item(D):
    a = plain(3, 2, 2 * T + 5)
    clean = run_t(D, a, 44100, 220)
    for which in CTL:
        b = {k: v.clone() for k, v in a.items()}
        b[which][1] = float("nan")
        dirty = run_t(D, b, 44100, 220)
        for k in NAMES:
            assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), (which, k)
            assert torch.isnan(dirty[k][1]).all(), (which, k)
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, :, ::97] = float("nan")
    dirty = run_t(D, b, 44100, 220)
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
    assert torch.equal(clean["y"], dirty["y"]) and not any(torch.isfinite(dirty[k][1]) for k in GRADS)


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * T + 5
    a = plain(3, 2, N)
    want = run_t(D, a, 44100, 220)
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
    y = D.limiter(xv, 44100, *ctl)
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), [xv] + ctl)
    for k, g in zip(NAMES, (y,) + grads):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_ignores_dirty_scratch_and_refuses_before_it_launches(D):
    """Through the C ABI: every output written inside NaN-filled guard words leaves the guards NaN, a NaN-filled scratch gives the same
    bits as a zero-filled one, gain = winner = NULL / gx = NULL change nothing else, and a refused call writes nothing."""
    from dasp_pytorch_amd._lib import ptr, stream
    sr, L, G = 44100.0, 220, 64
    B, C, N = 3, 2, 2 * T + 5
    a = plain(B, C, N)
    x, gy = a["x"].to(DEV), a["w"].to(DEV)
    ctl = torch.stack([a[k] for k in CTL], -1).contiguous().to(DEV)
    nstate, nscr = lib().dasp_limiter_state_floats(B, N), lib().dasp_limiter_partial_floats(B, N)
    assert nstate == 2 * B * N == nscr
    Lb = lib()

    def guarded(n, fill=float("nan"), dtype=torch.float32):
        buf = torch.full((n + 2 * G,), float("nan"), device=DEV)
        buf[G:G + n] = fill
        return buf, buf[G:G + n]

    def run(fill, save=True, want_gx=True, L=L, expect=0):
        bufs = {k: guarded(n) for k, n in (("y", B * C * N), ("gain", B * N), ("win", B * N), ("gx", B * C * N), ("gctl", B * 2))}
        bufs["scr"] = guarded(nscr, fill)
        rc = Lb.dasp_limiter_forward(ptr(x), ptr(ctl), ptr(bufs["y"][1]), ptr(bufs["gain"][1] if save else None), ptr(bufs["win"][1] if save else None),
                                     B, C, N, L, sr, 1e-8, stream())
        assert rc == expect
        if not save and not expect:
            assert Lb.dasp_limiter_forward(ptr(x), ptr(ctl), ptr(torch.empty_like(x)), ptr(bufs["gain"][1]), ptr(bufs["win"][1]), B, C, N, L, sr, 1e-8,
                                           stream()) == 0
        rc = Lb.dasp_limiter_backward(ptr(x), ptr(ctl), ptr(bufs["gain"][1]), ptr(bufs["win"][1]), ptr(gy), ptr(bufs["gx"][1] if want_gx else None),
                                      ptr(bufs["gctl"][1]), ptr(bufs["scr"][1]), B, C, N, L, sr, 1e-8, stream())
        assert rc == expect
        torch.cuda.synchronize()
        for k, (buf, inner) in bufs.items():
            assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all(), k
        return {k: inner.clone() for k, (buf, inner) in bufs.items()}

    zero, dirty, lean = run(0.0), run(float("nan")), run(0.0, save=False, want_gx=False)
    for k in ("y", "gain", "win", "gx", "gctl", "scr"):
        assert torch.equal(zero[k].view(torch.int32), dirty[k].view(torch.int32)), k
    for k in ("y", "gain", "win", "gctl", "scr"):
        assert torch.equal(zero[k].view(torch.int32), lean[k].view(torch.int32)), k
    assert torch.isnan(lean["gx"]).all()
    ref = run_t(D, a, sr, L)
    assert torch.equal(zero["y"].view(B, C, N), ref["y"]) and torch.equal(zero["gx"].view(B, C, N), ref["gx"])
    for q, k in enumerate(GRADS):
        assert torch.equal(zero["gctl"].view(B, 2)[:, q], ref[k]), k
    refused = run(float("nan"), L=K.MAX_LOOKAHEAD + 1, expect=-2)             # nothing launched: every word is still NaN
    assert all(torch.isnan(v).all() for v in refused.values())
    assert lib().dasp_device_error() == 0


# ---- 10. what the forward pass leaves behind -------------------------------------------------------------------------------------------------
def test_forward_saves_eight_bytes_per_item_sample_and_nothing_without_a_gradient(D):
    B, C, N = 3, 2, 2 * T + 5
    a = plain(B, C, N)
    x = a["x"].to(DEV).requires_grad_(True)
    ctl = [a[k].to(DEV).requires_grad_(True) for k in CTL]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = D.limiter(x, 44100, *ctl)
    assert any(t.data_ptr() == x.data_ptr() for t in saved)                     # x itself, not a copy
    extra = [t for t in saved if t.data_ptr() != x.data_ptr() and t.numel() != 2 * B]
    assert sum(t.numel() * t.element_size() for t in extra) == 8 * B * N == 4 * lib().dasp_limiter_state_floats(B, N)
    assert sorted(t.numel() for t in saved) == sorted([B * C * N, 2 * B, B * N, B * N])
    y.sum().backward()
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.limiter(x.detach(), 44100, *[c.detach() for c in ctl])
    assert not saved


# ---- 11. double backward -----------------------------------------------------------------------------------------------------------------
def test_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    x = a["x"].to(DEV).requires_grad_(True)
    y = D.limiter(x, 44100, a["threshold_db"].to(DEV), a["release_ms"].to(DEV))
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 12. module ----------------------------------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    sr = 44100
    x = plain(3, 2, 3000)["x"].to(DEV)
    p = torch.rand(3, 2, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = D.Limiter(sr, lookahead_ms=2.0)
    with torch.no_grad():
        got = m.process_normalized(x, p)
        want = D.limiter(x, sr, p[:, 0] * 40.0 - 40.0, p[:, 1] * 495.0 + 5.0, lookahead_ms=2.0)
    assert torch.equal(got, want) and not torch.equal(got, x)


def test_half_and_bfloat16_are_converted_and_float64_is_refused(D):
    from dasp_pytorch_amd import _lib
    a = plain(2, 2, 3000)
    ctl = [a[k].to(DEV) for k in CTL]
    for dt in (torch.float16, torch.bfloat16):
        xl = a["x"].to(DEV).to(dt)
        with torch.no_grad():
            y = D.limiter(xl, 44100, *ctl)
            want = D.limiter(xl.float(), 44100, *ctl).to(dt)
        assert y.dtype == dt and torch.equal(y, want)
    with pytest.raises(_lib.DaspHipError, match="limiter: float64"):
        D.limiter(a["x"].to(DEV).double(), 44100, *ctl)
