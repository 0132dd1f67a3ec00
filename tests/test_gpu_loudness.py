"""functional.loudness / loudness_normalize / peak_normalize on the GPU (csrc/loudness.hip) against the float64 restatement
tests/bs1770_restated.py. Bounds: the project's own for dB-valued quantities (tests/test_gpu_time_losses.py) - |L - L_ref| / max(1, |L_ref|)
<= 2e-5, gradients within 1e-4 in relative L2 and in max|delta| / max|ref|. The reference of a case is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

from dasp_pytorch_amd import _lib
from tests import bs1770_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TOL, GRAD_TOL = 2e-5, 1e-4


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def draw(name):
    """-> (x float32, sample rate)."""
    if name.startswith("edge"):
        N = int(name[4:])
        return _frozen((0.3 * np.random.default_rng(N).standard_normal((1, 1, N))).astype(np.float32)), 8000
    if name == "gated":
        return _frozen(R.gated_draw()), 8000
    if name == "channels":
        return _frozen((0.3 * np.random.default_rng(5).standard_normal((3, 5, 9001))).astype(np.float32)), 8000
    if name == "generic":
        return _frozen((0.3 * np.random.default_rng(7).standard_normal((2, 2, 44117)) + 0.2).astype(np.float32)), 44100
    if name == "lowfreq":
        t = np.arange(66150) / 44100.0
        x = 0.5 * np.sin(2 * np.pi * 30.0 * t) + 1e-3 * np.random.default_rng(8).standard_normal(66150)
        return _frozen(x.reshape(1, 1, -1).astype(np.float32)), 44100
    if name == "rows":
        return _frozen((0.3 * np.random.default_rng(9).standard_normal((40, 2, 12000))).astype(np.float32)), 8000
    if name == "segmented":
        return _frozen((0.3 * np.random.default_rng(10).standard_normal((1, 1, 2 ** 18 + 3)) + 0.1).astype(np.float32)), 44100
    if name == "silence":
        x = (0.3 * np.random.default_rng(11).standard_normal((2, 2, 9001))).astype(np.float32)
        x[0] = 1e-6
        return _frozen(x), 8000
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def upstream(name):
    bs = draw(name)[0].shape[0]
    return _frozen((0.5 + np.random.default_rng(12).random(bs)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(name):
    x, fs = draw(name)
    r = R.loudness(x, fs, gL=upstream(name))
    for v in r.values():
        v.flags.writeable = False
    return r


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def offset_view(a):
    """`a` on the device as a contiguous view one float into a larger buffer: a base pointer that is only 4-byte aligned."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(dev(a).reshape(-1))
    v = buf[1:].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def run(D, name, make=dev):
    x, fs = draw(name)
    xt = make(x).requires_grad_(True)
    L = D.loudness(xt, fs)
    L.backward(dev(upstream(name)))
    return L.detach().cpu().double().numpy(), xt.grad.cpu().double().numpy()


def rel2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def check(name, L, g, min_margin=0.5):
    ref = reference(name)
    assert ref["margin"].min() >= min_margin, (name, ref["margin"])        # the float32 and float64 gate sets cannot differ
    el = float(np.max(np.abs(L - ref["L"]) / np.maximum(1.0, np.abs(ref["L"]))))
    errs = (rel2(g, ref["grad"]), relmax(g, ref["grad"]))
    print(f"{name}: L {L} ref {ref['L']} err {el:.2e}; grad rel L2 {errs[0]:.2e} max {errs[1]:.2e}; blocks {ref['nb'][0]} A {ref['nA']} J {ref['nJ']} "
          f"margin {ref['margin']}")
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(g)), name
    assert el <= L_TOL, (name, el)
    assert max(errs) <= GRAD_TOL, (name, errs)


def segments(name):
    x, _ = draw(name)
    return _lib.lib().dasp_loudness_segments(x.shape[0] * x.shape[1], x.shape[2])


@pytest.mark.parametrize("N", [3200, 3999, 4000])
def test_block_edges(D, N):
    """One block; one block with an ignored tail; two blocks."""
    name = f"edge{N}"
    assert reference(name)["nb"][0] == (2 if N == 4000 else 1)
    check(name, *run(D, name))


def test_both_gates_and_the_fixed_gate_gradient(D):
    ref = reference("gated")
    assert ref["nb"][0] == 27 and ref["nA"][0] == 20 and ref["nJ"][0] == 10
    check("gated", *run(D, "gated"))


def test_channel_weights(D):
    check("channels", *run(D, "channels"))


def test_generic_parity(D):
    assert segments("generic") > 1
    check("generic", *run(D, "generic"))


def test_low_frequency_tone(D):
    """A 30 Hz tone under the high-pass's double pole: a float32 sequential recurrence misses the bound here."""
    check("lowfreq", *run(D, "lowfreq"))


@pytest.mark.parametrize("channels, want", [((0,), -3.01), ((0, 1), 0.0)])
def test_997_hz_anchor(D, channels, want):
    x = R.sine_997(channels).astype(np.float32)
    L = float(D.loudness(dev(x), 48000)[0])
    print(f"997 Hz in channels {channels}: {L} LUFS")
    assert abs(L - want) <= 0.1                                            # EBU Tech 3341
    assert abs(L - R.loudness(x, 48000)["L"][0]) <= L_TOL * max(1.0, abs(want))


def test_row_per_workgroup_path(D):
    assert segments("rows") == 1
    check("rows", *run(D, "rows"))


def test_segmented_path(D):
    assert segments("segmented") > 1
    check("segmented", *run(D, "segmented"))


def test_silence_next_to_a_normal_item(D):
    x, fs = draw("silence")
    ref = reference("silence")
    assert ref["L"][0] == -np.inf and np.isfinite(ref["L"][1])
    L, g = run(D, "silence")
    print("silence:", L, ref["L"])
    assert L[0] == -np.inf and not np.isnan(g).any() and not np.isnan(L).any()
    assert np.all(g[0] == 0.0)
    assert abs(L[1] - ref["L"][1]) <= L_TOL * max(1.0, abs(ref["L"][1]))
    assert rel2(g[1], ref["grad"][1]) <= GRAD_TOL and relmax(g[1], ref["grad"][1]) <= GRAD_TOL
    alone = D.loudness(dev(x[1:]), fs)
    assert float(alone[0]) == float(np.float32(L[1]))                     # the other item is unaffected
    xt = dev(x).requires_grad_(True)
    y = D.loudness_normalize(xt, fs, -20.0)
    y.backward(torch.ones_like(y))
    assert torch.equal(y[0], xt.detach()[0])                               # unchanged, 0 dB
    assert torch.isfinite(y).all() and torch.isfinite(xt.grad).all()
    assert torch.equal(xt.grad[0], torch.ones_like(xt.grad[0]))


def test_two_runs_and_permuted_items_are_bit_identical(D):
    x, fs = draw("gated")
    up = upstream("gated")

    def once(xa, ua):
        xt = dev(xa).requires_grad_(True)
        L = D.loudness(xt, fs)
        L.backward(dev(ua))
        return L.detach().clone(), xt.grad.clone()

    L1, g1 = once(x, up)
    L2, g2 = once(x, up)
    assert torch.equal(L1, L2) and torch.equal(g1, g2)
    Lp, gp = once(x[::-1], up[::-1])
    assert torch.equal(Lp.flip(0), L1) and torch.equal(gp.flip(0), g1)
    xs, _ = draw("segmented")
    a = D.loudness(dev(xs), 44100)
    b = D.loudness(dev(xs), 44100)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["channels", "generic"])
def test_views_equal_their_contiguous_copies(D, name):
    x, fs = draw(name)
    L0, g0 = run(D, name)
    L1, g1 = run(D, name, make=offset_view)
    assert np.array_equal(L0, L1) and np.array_equal(g0, g1)

    def strided(a):                                                        # every other sample of a buffer twice as long
        buf = torch.zeros(a.shape[:-1] + (2 * a.shape[-1],), dtype=torch.float32, device=DEV)
        buf[..., ::2] = dev(a)
        v = buf[..., ::2]
        assert not v.is_contiguous()
        return v.detach()

    L2, g2 = run(D, name, make=strided)
    assert np.array_equal(L0, L2) and np.array_equal(g0, g2)


def test_loudness_normalize_reaches_the_target_and_its_gradient(D):
    x, fs = draw("generic")
    target = np.array([-23.0, -14.0])
    gy = _frozen((np.random.default_rng(13).standard_normal(x.shape)).astype(np.float32))
    y_ref, gx_ref = R.loudness_normalize(x, fs, target, gy=gy)
    xt = dev(x).requires_grad_(True)
    y = D.loudness_normalize(xt, fs, torch.tensor(target, dtype=torch.float32))
    y.backward(dev(gy))
    yn, gn = y.detach().cpu().double().numpy(), xt.grad.cpu().double().numpy()
    reached = R.loudness(yn, fs)["L"]
    print("normalize: reached", reached, "target", target, "value rel L2", rel2(yn, y_ref), "grad rel L2", rel2(gn, gx_ref), "max", relmax(gn, gx_ref))
    assert np.abs(reached - target).max() <= 1e-3
    assert rel2(yn, y_ref) <= GRAD_TOL and rel2(gn, gx_ref) <= GRAD_TOL and relmax(gn, gx_ref) <= GRAD_TOL
    y2 = D.loudness_normalize(dev(x), fs)                                  # the default target, a float
    assert np.abs(R.loudness(y2.cpu().double().numpy(), fs)["L"] + 23.0).max() <= 1e-3


@pytest.mark.parametrize("shape", [(3, 2, 4097), (1, 1, 2 ** 18 + 3)])
@pytest.mark.parametrize("peak_db", [0.0, -6.0])
def test_peak_normalize_against_the_formula(D, shape, peak_db):
    rng = np.random.default_rng([14, *shape])
    x = (0.3 * rng.standard_normal(shape)).astype(np.float32)
    gy = rng.standard_normal(shape).astype(np.float32)
    y_ref, gx_ref = R.peak_normalize(x, peak_db, 1e-8, gy=gy)
    xt = dev(x).requires_grad_(True)
    y = D.peak_normalize(xt, 44100, peak_db)
    y.backward(dev(gy))
    yn, gn = y.detach().cpu().double().numpy(), xt.grad.cpu().double().numpy()
    print(f"peak {shape} {peak_db} dB: value max {relmax(yn, y_ref):.2e}; grad rel L2 {rel2(gn, gx_ref):.2e} max {relmax(gn, gx_ref):.2e}")
    # float32 arithmetic on float64-exact inputs: one rounding of the factor and one of the product (2^-23 each), a few more in sum g x
    assert relmax(yn, y_ref) <= 3e-7
    assert rel2(gn, gx_ref) <= 1e-6 and relmax(gn, gx_ref) <= 1e-5
    assert abs(np.abs(yn).max(-1) - 10.0 ** (peak_db / 20.0)).max() <= 3e-7


def test_peak_normalize_ties_zeros_and_plain_division(D):
    x = np.zeros((2, 1, 4097), np.float32)
    x[0, 0, 7], x[0, 0, 900] = 0.5, -0.5                                   # an explicit tie: the correction goes to index 7
    x[0, 0, 100] = 0.25
    gy = np.random.default_rng(15).standard_normal(x.shape).astype(np.float32)
    y_ref, gx_ref = R.peak_normalize(x, 0.0, 1e-8, gy=gy)
    xt = dev(x).requires_grad_(True)
    y = D.peak_normalize(xt, 44100)
    y.backward(dev(gy))
    yn, gn = y.detach().cpu().double().numpy(), xt.grad.cpu().double().numpy()
    plain = 2.0 * gy[0, 0].astype(np.float64)                              # s g / p without the correction
    assert abs(gn[0, 0, 900] - plain[900]) <= 1e-6 * abs(plain[900]) and abs(gn[0, 0, 7] - plain[7]) > 1e-3
    assert np.abs(gn[0] - gx_ref[0]).max() <= 1e-5 * np.abs(gx_ref[0]).max()
    assert np.all(yn[1] == 0.0) and np.all(np.isfinite(gn[1]))             # the all-zero row with the default eps
    assert np.abs(gn[1] - gx_ref[1]).max() <= 1e-6 * np.abs(gx_ref[1]).max()
    x0 = dev(x[:1])
    y0 = D.peak_normalize(x0, 44100, 0.0, eps=0.0)                         # eps = 0 on a non-zero row: the plain division
    want = x0 / x0.abs().amax(-1, keepdim=True)
    assert (y0 - want).abs().max() <= 1.2e-7 * float(want.abs().max())


def test_graph_replay_equals_eager(D):
    """loudness_normalize forward and backward captured in one graph and replayed on new input: no host synchronisation in the call path
    (a capture would fail on one), nothing to zero, fixed summation orders - the replay equals eager bit for bit."""
    xa, fs = draw("generic")
    xb = _frozen(xa[::-1] * np.float32(0.5))
    xs = dev(xa).requires_grad_(True)
    gy = dev(np.random.default_rng(16).standard_normal(xa.shape).astype(np.float32))
    fn = lambda t: D.loudness_normalize(t, fs, -18.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn(xs).backward(gy)
    torch.cuda.current_stream().wait_stream(s)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = fn(xs)
        ys.backward(gy)
    for k, xn in enumerate((xb, xa)):
        with torch.no_grad():
            xs.copy_(dev(xn))
        xs.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        xe = dev(xn).requires_grad_(True)
        ye = fn(xe)
        ye.backward(gy)
        print(f"replay {k}: max |delta| value {float((ys - ye).detach().abs().max())} grad {float((xs.grad - xe.grad).abs().max())}")
        assert torch.equal(ys, ye) and torch.equal(xs.grad, xe.grad)
