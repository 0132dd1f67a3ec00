"""GPU parity of stereo_mix (csrc/stereo.hip mix_fwd_kernel / mix_bwd_kernel / mix_finalize_kernel): the reference-generated golden,
the float64 oracle composition stereo_bus(stereo_panner(.)) at other shapes, the two existing ops composed on the device, and the
properties the fused form promises - a mix that does not depend on the send, on the layout of x or on the batch around an item, results
that are bit-identical run to run and under graph replay, and the edges of the pan law.
Bounds are those of tests/test_gpu_stereo.py: values and grad x within 2e-6 of the peak (1e-6 on the golden), the reduced control
gradients within 5e-5 of the largest entry (2e-5 on the golden), 1e-4 against the reference's float32 run."""
import functools

import numpy as np
import pytest
import torch

from tests.stereo_mix_ref import SR, compose, draw
from tests.util import linf_peak, load_golden, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("mix", "send", "gx", "ggain", "gpan", "gsend")


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_t(D, x, gain_db, pan, send_db, w0, w1, x_grad=True, make=dev):
    """stereo_mix and the gradients of <mix, w0> + <send, w1> as device tensors (None where there is no send / no gradient)."""
    xt = make(x).requires_grad_(x_grad)
    ct = [dev(c).requires_grad_(True) if c is not None else None for c in (gain_db, pan, send_db)]
    out = D.stereo_mix(xt, SR, *ct)
    if send_db is None:
        assert isinstance(out, torch.Tensor)
        mix, send = out, None
        loss = (mix * dev(w0)).sum()
    else:
        assert isinstance(out, tuple) and len(out) == 2
        mix, send = out
        loss = (mix * dev(w0)).sum() + (send * dev(w1)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return dict(mix=mix.detach(), send=None if send is None else send.detach(), gx=xt.grad, ggain=ct[0].grad, gpan=ct[1].grad,
                gsend=None if ct[2] is None else ct[2].grad)


def run(*a, **k):
    return {key: None if v is None else v.cpu().numpy() for key, v in run_t(*a, **k).items()}


def errors(got, want):
    """Largest deviation over the largest reference entry, per quantity; control gradients flat."""
    e = {}
    for key in KEYS:
        if want.get(key) is None:
            assert got[key] is None
            continue
        a, b = np.asarray(got[key], np.float64).reshape(-1), np.asarray(want[key], np.float64).reshape(-1)
        assert a.shape == b.shape, key
        e[key] = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    return e


def check(name, e, val_tol, ctl_tol):
    record(name, **e)
    for key, v in e.items():
        assert v <= (val_tol if key in ("mix", "send", "gx") else ctl_tol), (name, key, v)


def same_bits(a, b, keys):
    for key in keys:
        assert (a[key] is None) == (b[key] is None), key
        if a[key] is not None:
            assert torch.equal(a[key], b[key]) if isinstance(a[key], torch.Tensor) else np.array_equal(a[key], b[key]), key


# ---- 1. the reference's own run -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_send", [True, False])
def test_golden(D, with_send):
    g = load_golden("stereo_mix_b2t3_n1501")
    got = run(D, g["x"], g["gain_db"], g["pan"], g["send_db"] if with_send else None, g["w0"], g["w1"])
    pre = "" if with_send else "ns_"
    want = dict(mix=g["mix64"], gx=g[pre + "gx64"], ggain=g[pre + "ggain64"], gpan=g[pre + "gpan64"])
    want32 = dict(mix=g["mix32"], gx=g[pre + "gx32"], ggain=g[pre + "ggain32"], gpan=g[pre + "gpan32"])
    if with_send:
        want.update(send=g["send64"], gsend=g["gsend64"])
        want32.update(send=g["send32"], gsend=g["gsend32"])
    assert got["mix"].shape == (2, 2, 1501) and got["gx"].shape == (2, 3, 1501) and got["ggain"].shape == got["gpan"].shape == (2, 3)
    e = errors(got, want)
    for key in ("mix", "send", "gx"):                    # per item, as the sibling's golden test measures
        if key in want:
            e[key] = linf_peak(got[key], want[key]).max()
    check(f"stereo_mix_golden send={int(with_send)}", e, 1e-6, 2e-5)
    e32 = errors(got, want32)
    record(f"stereo_mix_golden_vs_fp32_run send={int(with_send)}", **e32)
    assert max(e32.values()) < 1e-4


# ---- 2. shapes: a single sample, the scalar path, a segment boundary, boundary + ragged tail, many tracks, the track limit with a
# ragged tail, one training-sized N ------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 3, 7), (1, 5, 4096), (3, 2, 4099), (2, 64, 8192), (1, 256, 4100), (4, 8, 131072)]


@functools.lru_cache(maxsize=2)
def oracle_case(B, T, N):
    """Inputs and both float64 references (with and without the send) of one shape, computed once for its two test cases."""
    d = draw(B, T, N)
    x, gain_db, pan, send_db, w0, w1 = d
    return d, compose(x, gain_db, pan, send_db, w0, w1), compose(x, gain_db, pan, None, w0)


@pytest.mark.parametrize("with_send", [True, False])
@pytest.mark.parametrize("B,T,N", SHAPES)
def test_shapes_vs_oracle(D, B, T, N, with_send):
    (x, gain_db, pan, send_db, w0, w1), want_send, want_plain = oracle_case(B, T, N)
    got = run(D, x, gain_db, pan, send_db if with_send else None, w0, w1)
    assert got["mix"].shape == (B, 2, N) and got["gx"].shape == (B, T, N) and got["ggain"].shape == gain_db.shape and got["gpan"].shape == pan.shape
    check(f"stereo_mix_shapes ({B},{T},{N}) send={int(with_send)}", errors(got, want_send if with_send else want_plain), 2e-6, 5e-5)


# ---- 3. drop-in for the composition of the two existing ops --------------------------------------------------------------------------
def test_equals_composed_ops_on_device(D):
    """Against D.stereo_bus(D.stereo_panner(.)) itself: each op is within 2e-6 of the peak of the exact result, so the two forms are
    within 4e-6 of each other; the control gradients within 2 x 5e-5 likewise."""
    x, gain_db, pan, send_db, w0, w1 = draw(3, 5, 4099)
    got = run(D, x, gain_db, pan, send_db, w0, w1)
    xt = dev(x).requires_grad_(True)
    gt, pt, st = (dev(c).requires_grad_(True) for c in (gain_db, pan, send_db))
    panned = D.stereo_panner(xt, SR, pt)
    mix = D.stereo_bus(panned, SR, gt)
    send = D.stereo_bus(panned, SR, gt + st)
    ((mix * dev(w0)).sum() + (send * dev(w1)).sum()).backward()
    want = dict(mix=mix.detach(), send=send.detach(), gx=xt.grad, ggain=gt.grad, gpan=pt.grad, gsend=st.grad)
    check("stereo_mix_vs_composed_ops", errors(got, {k: v.cpu().numpy() for k, v in want.items()}), 4e-6, 1e-4)


# ---- 4. the mix does not know about the send -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,N", [(2, 3, 7), (2, 9, 8200)])
def test_mix_is_bit_identical_with_and_without_send(D, B, T, N):
    x, gain_db, pan, send_db, w0, w1 = draw(B, T, N)
    with torch.no_grad():
        plain = D.stereo_mix(dev(x), SR, dev(gain_db), dev(pan))
        both = D.stereo_mix(dev(x), SR, dev(gain_db), dev(pan), dev(send_db))
    assert isinstance(plain, torch.Tensor) and isinstance(both, tuple)
    assert torch.equal(plain, both[0]) and both[1].shape == plain.shape


# ---- 5. layout of x ------------------------------------------------------------------------------------------------------------------
def offset_view(a):
    """`a` on the device as a contiguous view one float into a larger buffer: a base pointer that is only 4-byte aligned."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(dev(a).reshape(-1))
    v = buf[1:].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.detach()


def sliced_view(a):
    """`a` as a slice of a wider tensor: not contiguous."""
    buf = torch.zeros(a.shape[:-1] + (a.shape[-1] + 9,), dtype=torch.float32, device=DEV)
    buf[..., 5:5 + a.shape[-1]] = dev(a)
    v = buf[..., 5:5 + a.shape[-1]]
    assert not v.is_contiguous()
    return v.detach()


@pytest.mark.parametrize("make", [offset_view, sliced_view])
def test_layout_of_x(D, make):
    B, T, N = 2, 3, 4100                                  # N % 4 == 0: the aligned call takes the 16-byte path, the offset one cannot
    d = draw(B, T, N)
    base = run(D, *d)
    got = run(D, *d, make=make)
    same_bits(base, got, ("mix", "send", "gx"))
    want = compose(*d)
    e = errors(got, want)
    check(f"stereo_mix_layout {make.__name__}", {k: e[k] for k in ("ggain", "gpan", "gsend")}, 2e-6, 5e-5)


# ---- 6. an item does not know about its batch ------------------------------------------------------------------------------------------
def test_item_alone_and_inside_a_batch(D):
    from dasp_pytorch_amd import _lib
    B, T, N, item = 40, 3, 24581, 17
    L = _lib.lib()
    assert L.dasp_stereo_mix_segment(1, N) != L.dasp_stereo_mix_segment(B, N)        # the two calls cut the signal differently
    d = draw(B, T, N)
    whole = run(D, *d)
    alone = run(D, *[a[item:item + 1] for a in d])
    for key in ("mix", "send", "gx"):
        assert np.array_equal(whole[key][item], alone[key][0]), key
    e = {}
    for key in ("ggain", "gpan", "gsend"):
        a, b = alone[key].reshape(-1).astype(np.float64), whole[key].reshape(B, T)[item].astype(np.float64)
        e[key] = np.abs(a - b).max() / np.abs(b).max()
    check("stereo_mix_item_alone_vs_batch", e, 2e-6, 5e-5)


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------------
def test_eager_runs_are_bit_identical(D):
    d = draw(3, 7, 20000)
    a, b = run_t(D, *d), run_t(D, *d)
    same_bits(a, b, KEYS)


def test_graph_replay_equals_eager(D):
    """Forward and backward captured in one graph and replayed: no host synchronisation in the call path (a capture would fail on one),
    nothing to zero, fixed summation orders - every replay equals the eager run bit for bit."""
    x, gain_db, pan, send_db, w0, w1 = draw(3, 7, 20000)
    eager = run_t(D, x, gain_db, pan, send_db, w0, w1)
    leaves = [dev(a).requires_grad_(True) for a in (x, gain_db, pan, send_db)]
    w0t, w1t = dev(w0), dev(w1)

    def step():
        mix, send = D.stereo_mix(leaves[0], SR, *leaves[1:])
        return (mix, send) + torch.autograd.grad((mix * w0t).sum() + (send * w1t).sum(), leaves)

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
        for key, o in zip(KEYS, (outs[0], outs[1], outs[2], outs[3], outs[4], outs[5])):
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 8. edges ----------------------------------------------------------------------------------------------------------------------------
def test_hard_pans_and_a_muted_track(D):
    """pan exactly 0 / 1: the silent channel is exactly 0 and the vanishing term of the pan gradient is dropped (the convention of the
    panner's finalize kernel); gain_db = -inf: the track contributes nothing and receives nothing."""
    B, T, N = 1, 4, 5000
    x, gain_db, pan, send_db, w0, w1 = draw(B, T, N)
    pan = np.array([[0.0, 1.0, 0.3, 0.6]], np.float32)
    gain_db = gain_db.copy()
    gain_db[0, 3] = -np.inf
    got = run(D, x, gain_db, pan, send_db, w0, w1)
    for key in KEYS:
        assert np.all(np.isfinite(got[key])), key
    assert np.all(got["gx"][0, 3] == 0) and got["ggain"].reshape(-1)[3] == 0 and got["gpan"].reshape(-1)[3] == 0 and got["gsend"].reshape(-1)[3] == 0
    # the formula of the issue in float64, the term whose u is 0 left out
    g = 10.0 ** (gain_db.astype(np.float64).reshape(T) / 20)
    s = 10.0 ** (send_db.astype(np.float64).reshape(T) / 20)
    th = pan.astype(np.float64).reshape(T) * (np.pi / 2)
    hp, ip = np.pi / 2, 2 / np.pi
    uL, uR = (hp - th) * ip * np.cos(th), th * ip * np.sin(th)
    duL, duR = ip * (-np.cos(th) - (hp - th) * np.sin(th)), ip * (np.sin(th) + th * np.cos(th))
    assert uR[0] == 0 and uL[1] == 0
    l, r = np.sqrt(uL), np.sqrt(uR)
    with np.errstate(divide="ignore", invalid="ignore"):
        dl = np.where(uL > 0, hp * duL / (2 * np.sqrt(uL)), 0.0)
        dr = np.where(uR > 0, hp * duR / (2 * np.sqrt(uR)), 0.0)
    x64 = x[0].astype(np.float64)
    AL, AR, SL, SR_ = x64 @ w0[0, 0].astype(np.float64), x64 @ w0[0, 1].astype(np.float64), x64 @ w1[0, 0].astype(np.float64), x64 @ w1[0, 1].astype(np.float64)
    ML, MR = AL + s * SL, AR + s * SR_
    c = np.log(10.0) / 20
    want = dict(mix=np.stack([(g * l) @ x64, (g * r) @ x64])[None], send=np.stack([(s * g * l) @ x64, (s * g * r) @ x64])[None],
                gpan=g * (dl * ML + dr * MR), ggain=c * g * (l * ML + r * MR), gsend=c * s * g * (l * SL + r * SR_))
    want["gx"] = ((g * l)[:, None] * (w0[0, 0] + s[:, None] * w1[0, 0]) + (g * r)[:, None] * (w0[0, 1] + s[:, None] * w1[0, 1]))[None]
    check("stereo_mix_hard_pans_muted", errors(got, want), 2e-6, 5e-5)
    # the silent channel of a hard pan shows on a single track: exactly 0 in the mix and in the send
    for p, silent in ((0.0, 1), (1.0, 0)):
        with torch.no_grad():
            mix, send = D.stereo_mix(dev(x[:, :1]), SR, dev(gain_db[:, :1]), torch.full((1, 1), p, device=DEV), dev(send_db[:, :1]))
        assert torch.all(mix[:, silent] == 0) and torch.all(send[:, silent] == 0) and float(mix[:, 1 - silent].abs().max()) > 0


def test_controls_gradients_do_not_depend_on_x_requiring_grad(D):
    d = draw(2, 5, 9000)
    a, b = run_t(D, *d), run_t(D, *d, x_grad=False)
    assert b["gx"] is None
    same_bits(a, b, ("mix", "send", "ggain", "gpan", "gsend"))
    x = dev(d[0])
    x0 = x.clone()
    D.stereo_mix(x, SR, dev(d[1]), dev(d[2]), dev(d[3]))
    assert torch.equal(x, x0)                                     # input not mutated


def test_empty_inputs(D):
    for B, T, N in ((2, 3, 0), (0, 3, 16)):
        x = torch.zeros(B, T, N, device=DEV, requires_grad=True)
        ctl = [torch.zeros(B, T, device=DEV, requires_grad=True) for _ in range(3)]
        mix, send = D.stereo_mix(x, SR, *ctl)
        assert mix.shape == send.shape == (B, 2, N)
        (mix.sum() + send.sum()).backward()
        assert x.grad.shape == x.shape and all(c.grad.shape == c.shape and not c.grad.any() for c in ctl)
        mix = D.stereo_mix(x, SR, ctl[0], ctl[1])
        assert isinstance(mix, torch.Tensor) and mix.shape == (B, 2, N)


def test_refusals(D):
    from dasp_pytorch_amd import _lib
    tmax = _lib.lib().dasp_stereo_mix_max_tracks()
    x = torch.zeros(1, tmax + 1, 64, device=DEV)
    c = torch.zeros(1, tmax + 1, device=DEV)
    with pytest.raises(_lib.DaspHipError, match="unsupported"):
        D.stereo_mix(x, SR, c, c)
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.stereo_mix(torch.zeros(1, 2, 64, device=DEV, dtype=torch.float64), SR, torch.zeros(1, 2, device=DEV), torch.zeros(1, 2, device=DEV))
    with pytest.raises(RuntimeError, match="invalid for input of size"):
        D.stereo_mix(torch.zeros(2, 3, 64, device=DEV), SR, torch.zeros(2, 3, device=DEV), torch.zeros(5, device=DEV))
