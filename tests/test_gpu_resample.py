"""GPU tests of resample (csrc/resample.hip): parity of y and grad x with the float64 restatement (tests/resample_restated.py), exact
identities, the adjoint, bit-for-bit reproducibility, what happens off the nominal domain, host refusals, the refused
double backward and the module. The autograd and call-state contracts run on the op's entry in tests/autograd_contract_cases.py.

Parity bounds. The yardstick is the restatement with the same float32 taps and float32 arithmetic on the same inputs on the CPU:
e32 = its error against float64 arithmetic, relative to the peak of the float64 result. The kernel sums an output's products in another
order than conv1d does, so it gets 4 x e32, and never less than the floor of the other fused effects, 2e-6 of the peak (DESIGN 3.12 -
3.14). The op has no atomics: wherever two results are compared, they are compared bit for bit.

Lengths. T = dasp_resample_tile(...) is what one workgroup computes: outputs in the forward direction, inputs in the backward one. When
upsampling not every output length exists (M = ceil(n N / o) moves in steps); "the N that gives M" is then the shortest N with at least
M outputs, which crosses the same tile boundary.
"""
import numpy as np
import pytest
import torch

from tests import resample_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = R.FLOOR
NAMES = ("y", "gx")
RATIOS = [(147, 160), (160, 147), (441, 160), (80, 441), (640, 147), (2, 1), (1, 2), (3, 2), (2, 3)]
HANN = dict(resampling_method="sinc_interp_hann")
KAISER = dict(resampling_method="sinc_interp_kaiser")
DESIGNS = {"hann": HANN, "kaiser": KAISER, "kaiser_fast": R.KAISER_FAST}
# the two default windows at every ratio; the kaiser_fast setting (width 16, rolloff 0.85, beta 8.5555) at the ratios whose tables fit
# (at 441:160, 80:441 and 640:147 they hold more than dasp_resample_table_limit() taps: test_too_large_a_design_...)
CASES = [(o, n, d) for o, n in RATIOS for d in ("hann", "kaiser")] + [(o, n, "kaiser_fast") for o, n in ((147, 160), (160, 147), (2, 1), (1, 2))]


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def host_design(o, n, kw):
    from dasp_pytorch_amd import _resample_design
    a = dict(lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None)
    a.update(kw)
    return _resample_design.Design(o, n, a["lowpass_filter_width"], a["rolloff"], a["resampling_method"], a["beta"])


def tiles(o, n, kw):
    """(outputs per workgroup forward, inputs per workgroup backward), from the size query."""
    d = host_design(o, n, kw)
    T = tuple(lib().dasp_resample_tile(t.A, t.B, t.P, t.span) for t in (d.fwd, d.bwd))
    assert T[0] > 0 and T[0] % n == 0 and T[1] > 0 and T[1] % o == 0
    return T


def n_for(o, n, M):
    """The shortest N with ceil(n N / o) >= M."""
    N = (M - 1) * o // n + 1
    assert R.out_len(o, n, N) >= M > R.out_len(o, n, N - 1)
    return N


def draw(shape_x, o, n, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * o + 3 * n + sum(shape_x))
    M = R.out_len(o, n, shape_x[-1])
    return torch.rand(*shape_x, generator=g) * 2 - 1, torch.randn(*shape_x[:-1], M, generator=g)


def run_t(D, x, w, o, n, **kw):
    xt = x.to(DEV).requires_grad_(True)
    y = D.resample(xt, o, n, **kw)
    (gx,) = torch.autograd.grad((y * w.to(DEV)).sum(), xt)
    torch.cuda.synchronize()
    return dict(y=y.detach(), gx=gx)


def check_parity(D, name, x, w, o, n, kw):
    want = R.forward_backward(x, w, o, n, **kw)
    f32 = R.forward_backward(x, w, o, n, arith=torch.float32, **kw)
    got = {k: v.cpu().numpy() for k, v in run_t(D, x, w, o, n, **kw).items()}
    e32 = {k: peak_err(f32[k], want[k]) for k in NAMES}
    e = {k: peak_err(got[k], want[k]) for k in NAMES}
    record(name, **e, **{"fp32_" + k: v for k, v in e32.items()}, **{"share_" + k: e[k] / max(4 * e32[k], FLOOR) for k in NAMES})
    for k in NAMES:
        assert got[k].shape == want[k].shape, (name, k)
        assert e[k] <= max(4 * e32[k], FLOOR), (name, k, e[k], e32[k])


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
def lengths(o, n, kw):
    """N = 1, o - 1, o, o + 1; the N that give M = T - 1, T, T + 1 and 2 T + 1 outputs; and N = Tb - 1, Tb, Tb + 1, 2 Tb + 1, the same
    thresholds of the backward kernel, whose workgroups own Tb inputs."""
    T, Tb = tiles(o, n, kw)
    ns = {1, o - 1, o, o + 1} | {n_for(o, n, M) for M in (T - 1, T, T + 1, 2 * T + 1)} | {Tb - 1, Tb, Tb + 1, 2 * Tb + 1}
    return sorted(N for N in ns if N >= 1)


@pytest.mark.parametrize("o,n,design", CASES, ids=[f"{o}:{n}-{d}" for o, n, d in CASES])
def test_parity_with_the_float64_restatement(D, o, n, design):
    """Every length of lengths(), one channel and two in turn (rows = C, the shape (1, C, N))."""
    kw = DESIGNS[design]
    for q, N in enumerate(lengths(o, n, kw)):
        C = 1 + q % 2
        x, w = draw((1, C, N), o, n)
        check_parity(D, f"resample_parity {o}:{n} {design} (1,{C},{N})", x, w, o, n, kw)


def test_parity_of_a_training_batch(D):
    """(64, 2, 8192) at 44.1 -> 48 kHz: 128 rows of three forward tiles and three backward tiles each."""
    x, w = draw((64, 2, 8192), 147, 160)
    assert w.shape == (64, 2, 8917)
    check_parity(D, "resample_parity 147:160 hann (64,2,8192)", x, w, 44100, 48000, HANN)


# ---- 2. exact cases, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,n,design", [(147, 160, "hann"), (441, 160, "kaiser"), (2, 3, "hann"), (3, 2, "kaiser")])
def test_unit_impulse_gives_the_float32_taps(D, o, n, design):
    """An impulse at sample 0, at N - 1 and at the two input samples either side of the first forward tile boundary (the last sample
    of frame F - 1 and the first of frame F): y[q n + r] is the float32 tap h[r][i + width - q o] where that is a tap, else 0."""
    kw = DESIGNS[design]
    taps, width = D.signal.resample_taps(o, n, **kw)
    h32 = taps.float()
    K = h32.shape[1]
    F = tiles(o, n, kw)[0] // n
    N = 2 * F * o + 3
    M = R.out_len(o, n, N)
    where = [0, N - 1, F * o - 1, F * o]
    x = torch.zeros(len(where), N)
    for b, i in enumerate(where):
        x[b, i] = 1.0
    with torch.no_grad():
        y = D.resample(x.to(DEV), o, n, **kw).cpu()
    j = torch.arange(M)
    q, r = j // n, j % n
    for b, i in enumerate(where):
        k = i + width - q * o
        ok = (k >= 0) & (k < K)
        want = torch.where(ok, h32[r, k.clamp(0, K - 1)], torch.zeros(()))
        assert want.count_nonzero() >= 2 and torch.equal(y[b], want), (b, i)


@pytest.mark.parametrize("o,n", [(147, 160), (441, 160), (1, 2)])
def test_prepended_frames_of_zeros_shift_the_output(D, o, n):
    """k o zeros in front of x move y by k n samples, bit for bit; k = F + 1 frames, so every output changes its place in its tile and
    the shift crosses a tile."""
    F = tiles(o, n, HANN)[0] // n
    k = F + 1
    x, _ = draw((2, F * o + 77), o, n)
    x2 = torch.cat([torch.zeros(2, k * o), x], -1)
    with torch.no_grad():
        y, y2 = D.resample(x.to(DEV), o, n), D.resample(x2.to(DEV), o, n)
    assert y2.shape[-1] == y.shape[-1] + k * n and torch.equal(y2[:, k * n:], y) and y.abs().max() > 0.1


def test_equal_rates_return_x_and_reduced_rates_the_same_bits(D):
    x, w = draw((2, 2, 5000), 147, 160)
    xd = x.to(DEV)
    assert D.resample(xd, 48000, 48000) is xd
    a, b = run_t(D, x, w, 44100, 48000), run_t(D, x, w, 147, 160)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


# ---- 3. adjoint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,n", [(147, 160), (441, 160)])
def test_adjoint(D, o, n):
    """The op is linear: <y, w> = <x, gx>, both sums taken in float64 on the host from float32 results. The relative difference, the
    largest over four draws of w, is within 4 x that of the float32-arithmetic restatement."""
    x, _ = draw((3, 2, 9000), o, n)
    g = torch.Generator().manual_seed(o)
    rel = lambda y, gx, w: abs(float((np.float64(y) * w).sum() - (x.double().numpy() * np.float64(gx)).sum())) / abs(float((np.float64(y) * w).sum()))
    got, want = [], []
    for _ in range(4):
        w = torch.randn(3, 2, R.out_len(o, n, 9000), generator=g)
        k = run_t(D, x, w, o, n)
        got.append(rel(k["y"].cpu().numpy(), k["gx"].cpu().numpy(), w.double().numpy()))
        r = R.forward_backward(x, w, o, n, arith=torch.float32)
        want.append(rel(r["y"].astype(np.float32), r["gx"].astype(np.float32), w.double().numpy()))
    record(f"resample_adjoint {o}:{n}", kernel=max(got), restated_fp32=max(want))
    assert max(got) <= 4 * max(want), (got, want)


# ---- 4. reproducibility: everything bit for bit ------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(D):
    x, w = draw((6, 2, 9000), 160, 147)
    p, q = run_t(D, x, w, 160, 147), run_t(D, x, w, 160, 147)
    for k in NAMES:
        assert torch.equal(p[k], q[k]), k


def test_item_alone_and_inside_a_batch(D):
    x, w = draw((5, 2, 9000), 147, 160)
    whole = run_t(D, x, w, 147, 160)
    for b in (0, 3):
        alone = run_t(D, x[b:b + 1], w[b:b + 1], 147, 160)
        for k in NAMES:
            assert torch.equal(whole[k][b], alone[k][0]), (b, k)


@pytest.mark.parametrize("cold", [False, True])
def test_graph_replay_equals_eager(D, cold):
    """One forward + backward step captured on a single stream. cold: a design that no call has used before is first used inside the
    capture (rolloff 0.97 in this test only) - its tables are then filled by kernel nodes of the graph, not copied from the host."""
    kw = dict(rolloff=0.97) if cold else {}
    x, w = draw((4, 2, 9000), 147, 160)
    xt, wt = x.to(DEV).requires_grad_(True), w.to(DEV)

    def step():
        y = D.resample(xt, 147, 160, **kw)
        return (y,) + torch.autograd.grad((y * wt).sum(), [xt])

    if not cold:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    eager = run_t(D, x, w, 147, 160, **kw)
    for k in range(3):
        for o in outs:
            o.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, o in zip(NAMES, outs):
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 5. off the nominal domain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e30])
def test_poisoned_neighbour_leaves_other_items_alone(D, value):
    x, w = draw((3, 2, 9000), 147, 160)
    clean = run_t(D, x, w, 147, 160)
    x2, w2 = x.clone(), w.clone()
    x2[1, :, ::97] = value
    w2[1, :, ::89] = value
    dirty = run_t(D, x2, w2, 147, 160)
    for k in NAMES:
        assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), k
        assert not (dirty[k][1].abs() < 1e20).all(), k                           # the poisoned item itself shows it


@pytest.mark.parametrize("o,n", [(147, 160), (441, 160)])
@pytest.mark.parametrize("where", ["x", "w"])
def test_one_nan_reaches_exactly_the_span_that_covers_it(D, o, n, where):
    """A NaN in x at sample i makes NaN exactly the outputs whose compact span holds i; a NaN in the upstream gradient at output j
    exactly the inputs inside j's span. The spans are where signal.resample_taps is not zero (first to last per phase); everything
    else keeps its bits. In the conv1d form the whole 2 width + o window would be NaN."""
    taps, width = D.signal.resample_taps(o, n)
    nz = (taps != 0).numpy()
    first = nz.argmax(1)
    last = nz.shape[1] - 1 - nz[:, ::-1].argmax(1)
    T = tiles(o, n, HANN)[0]
    N = n_for(o, n, T) + 3 * o                               # the sample sits at the first tile boundary
    M = R.out_len(o, n, N)
    j = np.arange(M)
    lo, hi = (j // n) * o + first[j % n] - width, (j // n) * o + last[j % n] - width + 1
    rlo, rhi = R.spans(o, n, N)
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi)
    x, w = draw((2, N), o, n)
    clean = run_t(D, x, w, o, n)
    x2, w2 = x.clone(), w.clone()
    if where == "x":
        i0 = n_for(o, n, T)
        x2[0, i0] = float("nan")
        key, want = "y", (lo <= i0) & (i0 < hi)
    else:
        j0 = T
        w2[0, j0] = float("nan")
        key, want = "gx", (np.arange(N) >= lo[j0]) & (np.arange(N) < hi[j0])
    dirty = run_t(D, x2, w2, o, n)
    bad = torch.isnan(dirty[key][0]).cpu().numpy()
    assert np.array_equal(bad, want) and 2 <= want.sum() < want.size // 4
    keep = torch.from_numpy(~want).to(DEV)
    assert torch.equal(dirty[key][0][keep], clean[key][0][keep]) and torch.equal(dirty[key][1], clean[key][1])
    other = "gx" if key == "y" else "y"
    if where == "w":
        assert torch.equal(dirty[other], clean[other])


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_views_of_x_and_of_the_upstream_gradient(D, view):
    o, n, N = 147, 160, 4500
    x, w = draw((3, 2, N), o, n)
    want = run_t(D, x, w, o, n)
    xd, wd = x.to(DEV), w.to(DEV)

    def as_view(t):
        if view == "offset":
            v = torch.cat([torch.zeros(5, device=DEV), t.reshape(-1)])[5:].view(t.shape)
            assert v.storage_offset() == 5
        elif view == "strided":
            v = t.transpose(0, 1).contiguous().transpose(0, 1)
            assert not v.is_contiguous()
        else:
            v = torch.cat([t, torch.ones(*t.shape[:-1], 40, device=DEV)], -1)[..., :t.shape[-1]]
            assert not v.is_contiguous()
        assert torch.equal(v, t)
        return v
    xv = as_view(xd).requires_grad_(True)
    y = D.resample(xv, o, n)
    (gx,) = torch.autograd.grad(y, xv, grad_outputs=as_view(wd))
    assert torch.equal(y, want["y"]) and torch.equal(gx, want["gx"])


def test_c_abi_keeps_guard_words_and_overwrites_its_outputs(D):
    """Through the C ABI: y and gx written inside NaN-filled guard words leave the guards NaN, and NaN-filled output buffers are
    fully overwritten with the bits of the Python path."""
    from dasp_pytorch_amd import _ctypes_ops
    from dasp_pytorch_amd._lib import call, ptr, stream
    o, n, G = 441, 160, 64
    rows, N = 3, 2 * tiles(o, n, HANN)[1] + 11
    x, w = draw((rows, N), o, n)
    M = w.shape[-1]
    d = _ctypes_ops.resample_design(o, n, 6, 0.99, "sinc_interp_hann", None)
    dev = torch.device(DEV)
    xd, wd = x.to(DEV), w.to(DEV)

    def guarded(count):
        buf = torch.full((count + 2 * G,), float("nan"), device=DEV)
        return buf, buf[G:G + count]
    ybuf, y = guarded(rows * M)
    gbuf, gx = guarded(rows * N)
    f, b = d.fwd, d.bwd
    call("dasp_resample_forward", ptr(xd), ptr(_ctypes_ops._resample_table(d, "fwd", dev)), ptr(y), rows, N, M, o, n, f.P, f.lo, f.span, stream())
    call("dasp_resample_backward", ptr(wd), ptr(_ctypes_ops._resample_table(d, "bwd", dev)), ptr(gx), rows, N, M, o, n, b.P, b.lo, b.span, stream())
    torch.cuda.synchronize()
    for buf, inner in ((ybuf, y), (gbuf, gx)):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all() and torch.isfinite(inner).all()
    ref = run_t(D, x, w, o, n)
    assert torch.equal(y.view(rows, M), ref["y"]) and torch.equal(gx.view(rows, N), ref["gx"])


def test_silence_in_silence_out(D):
    x, w = draw((2, 2, 5000), 441, 160)
    got = run_t(D, torch.zeros_like(x), w, 441, 160)
    assert not got["y"].any() and torch.isfinite(got["gx"]).all()
    got = run_t(D, x, torch.zeros_like(w), 441, 160)
    assert not got["gx"].any()


def test_empty_input_and_one_dimension(D):
    for shape in ((2, 2, 0), (0, 2, 16), (0,)):
        x = torch.zeros(*shape, device=DEV, requires_grad=True)
        y = D.resample(x, 147, 160)
        assert y.shape == shape[:-1] + (R.out_len(147, 160, shape[-1]),)
        y.sum().backward()
        assert x.grad.shape == x.shape
    x, w = draw((1, 300), 3, 2)
    a = run_t(D, x, w, 3, 2)
    b = run_t(D, x[0], w[0], 3, 2)
    assert b["y"].shape == (200,) and torch.equal(a["y"][0], b["y"]) and torch.equal(a["gx"][0], b["gx"])


# ---- 6. host refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,n,kw", [(2049, 2048, HANN), (441, 160, R.KAISER_FAST), (80, 441, R.KAISER_FAST), (640, 147, R.KAISER_FAST)],
                         ids=["2049:2048", "441:160-kaiser_fast", "80:441-kaiser_fast", "640:147-kaiser_fast"])
def test_too_large_a_design_is_refused_before_any_launch(D, o, n, kw):
    d = host_design(o, n, kw)
    assert max(d.fwd.floats, d.bwd.floats) > lib().dasp_resample_table_limit()
    x = torch.zeros(1, 64, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match=f"resample {o}:{n}"):
        D.resample(x, o, n, **kw)
    torch.cuda.synchronize()
    assert lib().dasp_device_error() == 0


def test_double_backward_is_refused(D):
    x = draw((2, 600), 3, 2)[0].to(DEV).requires_grad_(True)
    y = D.resample(x, 3, 2)
    (gx,) = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)          # the upstream gradient 2 y depends on x
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 7. double backward, the module ------------------------------------------------------------------------------------------------------
def test_module_equals_functional(D):
    x = draw((3, 2, 3000), 147, 160)[0].to(DEV)
    m = D.Resample(44100, 48000, resampling_method="sinc_interp_kaiser", lowpass_filter_width=8, rolloff=0.9, beta=10.0)
    assert not list(m.parameters())
    with torch.no_grad():
        got = m(x)
        want = D.resample(x, 44100, 48000, lowpass_filter_width=8, rolloff=0.9, resampling_method="sinc_interp_kaiser", beta=10.0)
    assert got.shape == (3, 2, R.out_len(147, 160, 3000)) and torch.equal(got, want)
    assert torch.equal(D.Resample(48000, 44100)(x), D.resample(x, 160, 147))
