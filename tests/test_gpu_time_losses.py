"""GPU parity of the time-domain losses (losses.time_domain_loss, ESRLoss .. SDSDRLoss, FIRFilter; csrc/tdloss.hip) against
tests/auraloss_time_restated.py (float64 torch on the CPU, autograd for the gradients).

Bounds, those of tests/test_gpu_mrstft_options.py: 2e-5 on the loss (relative for esr / dc / log_cosh / mse and their mixes,
|delta| / max(1, |ref|) for the dB losses), 1e-4 on the gradients of both arguments in relative L2 norm and in the largest entry. The same
formulas in float32 torch on the CPU sit at <= 4.4e-7 and <= 5.9e-5 over these shapes and draws, except float32 log-cosh on the converged
draw, which is 30 .. 100 % off (cosh + 1e-8 rounds to 1): the kernel's form keeps eps and is held to 2e-5 there too.

Draws (t = 0.3 randn): generic p = t + 0.09 randn + 0.05; converged p = t + 3e-4 randn + 1e-4 (a moment expansion in p, t or an lc that
drops eps fails here); big DC p = t + 0.09 randn + 0.5 with zero_mean True and False."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import auraloss_time_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 2e-5, 1e-4
MIX = {"esr": 1.0, "dc": 1.0, "mse": 100.0}
CASES = {name: {name: 1.0} for name in R.TERMS}
CASES["mix"] = MIX
DRAWS = (("generic", True), ("converged", True), ("big_dc", True), ("big_dc", False))


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


@functools.lru_cache(maxsize=None)
def draw(shape, kind, seed=0):
    rng = np.random.default_rng([seed, *shape, ("generic", "converged", "big_dc").index(kind)])
    t = (0.3 * rng.standard_normal(shape)).astype(np.float32)
    n = rng.standard_normal(shape)
    p = (t + {"generic": 0.09 * n + 0.05, "converged": 3e-4 * n + 1e-4, "big_dc": 0.09 * n + 0.5}[kind]).astype(np.float32)
    p.flags.writeable = t.flags.writeable = False
    return p, t


@functools.lru_cache(maxsize=None)
def reference(shape, kind, case, zero_mean, a=1.0, reduction="mean"):
    """The float64 restatement of one case, computed once and shared."""
    p, t = draw(shape, kind)
    out = R.loss_and_grads(p, t, CASES[case], a=a, zero_mean=zero_mean, reduction=reduction)
    for o in out:
        o.flags.writeable = False
    return out


def kw(weights, **more):
    return dict({"w_" + k: v for k, v in weights.items()}, **more)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)            # (a copy: the shared draws are read-only)


def offset_view(a):
    """`a` on the device as a contiguous view one float into a larger buffer: a base pointer that is only 4-byte aligned."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(dev(a).reshape(-1))
    v = buf[1:].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def run(D, p, t, make_p=dev, make_t=dev, upstream=None, **options):
    pt, tt = make_p(p).requires_grad_(True), make_t(t).requires_grad_(True)
    loss = D.losses.time_domain_loss(pt, tt, **options)
    loss.backward(None if upstream is None else torch.from_numpy(np.asarray(upstream)).to(DEV).reshape(loss.shape))
    return loss.detach().cpu().double().numpy(), pt.grad.cpu().double().numpy(), tt.grad.cpu().double().numpy()


def rel2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def check(name, got, want, db):
    (l, gp, gt), (lo, gpo, gto) = got, want
    el = float(np.max(np.abs(l - lo) / (np.maximum(1.0, np.abs(lo)) if db else np.abs(lo))))
    errs = (rel2(gp, gpo), relmax(gp, gpo), rel2(gt, gto), relmax(gt, gto))
    print(f"{name}: loss {el:.2e}; input.grad rel L2 {errs[0]:.2e} max {errs[1]:.2e}; target.grad rel L2 {errs[2]:.2e} max {errs[3]:.2e}")
    assert np.all(np.isfinite(l)) and np.all(np.isfinite(gp)) and np.all(np.isfinite(gt)), name
    assert el < LOSS_TOL, (name, el)
    assert max(errs) < GRAD_TOL, (name, errs)


SHAPES = [(2, 1, 1), (1, 1, 5), (33, 1, 257), (3, 2, 4099), (1, 1, 70001)]


@pytest.mark.parametrize("shape", SHAPES + ["view", "views"], ids=str)
def test_every_term_and_the_mix_against_float64(D, shape):
    """(2,1,1): esr, dc, log_cosh, mse and the mix only - the dB losses are degenerate at N = 1, where auraloss itself gives NaN gradients.
    "view": (3,2,4099) with the input a view one float into a larger buffer; "views": both signals."""
    make_p = make_t = dev
    if shape in ("view", "views"):
        make_p, make_t, shape = offset_view, (offset_view if shape == "views" else dev), (3, 2, 4099)
    for kind, zero_mean in DRAWS:
        for case in CASES:
            if case in R.DB_TERMS and shape[-1] == 1:
                continue
            if not zero_mean and case not in R.DB_TERMS:
                continue                                             # zero_mean only enters the dB losses
            p, t = draw(shape, kind)
            got = run(D, p, t, make_p, make_t, zero_mean=zero_mean, **kw(CASES[case]))
            check(f"{case} {shape} {kind} zero_mean={zero_mean}", got, reference(shape, kind, case, zero_mean), case in R.DB_TERMS)


@pytest.mark.parametrize("reduction", ["none", "sum"])
def test_reductions_with_a_non_uniform_upstream_gradient(D, reduction):
    shape = (3, 2, 4099)
    p, t = draw(shape, "generic")
    up = np.asarray(np.random.default_rng(5).standard_normal(shape[:-1] if reduction == "none" else ()), dtype=np.float32)
    for case in ("mix", "si_sdr", "log_cosh"):
        want = R.loss_and_grads(p, t, CASES[case], reduction=reduction, upstream=up)
        got = run(D, p, t, upstream=up, reduction=reduction, **kw(CASES[case]))
        assert got[0].shape == want[0].shape == (shape[:-1] if reduction == "none" else ())
        check(f"{case} reduction={reduction}", got, want, case in R.DB_TERMS)


def test_backward_of_one_argument_only(D):
    p, t = draw((3, 2, 4099), "generic")
    opts = kw(MIX, w_log_cosh=0.5, w_si_sdr=0.1)
    _, gp, gt = run(D, p, t, **opts)
    pt = dev(p).requires_grad_(True)
    D.losses.time_domain_loss(pt, dev(t), **opts).backward()
    tt = dev(t).requires_grad_(True)
    D.losses.time_domain_loss(dev(p), tt, **opts).backward()
    print("one-sided gradients: max |delta| input", float(np.abs(pt.grad.cpu().numpy() - gp).max()), "target", float(np.abs(tt.grad.cpu().numpy() - gt).max()))
    assert np.array_equal(pt.grad.cpu().double().numpy(), gp) and np.array_equal(tt.grad.cpu().double().numpy(), gt)


def test_zero_weight_term_with_an_infinite_value_stays_out(D):
    """a d = 200: cosh overflows float32. With w_log_cosh = 0 nothing of it reaches the value or the gradients (no 0 * inf)."""
    t = draw((3, 2, 4099), "generic")[1]
    p = (t + 200.0).astype(np.float32)
    got = run(D, p, t, w_esr=1.0, w_log_cosh=0.0, w_mse=1.0, a=1.0)
    want = R.loss_and_grads(p, t, {"esr": 1.0, "mse": 1.0})
    check("esr + mse beside an overflowing log-cosh", got, want, False)


def test_log_cosh_at_large_arguments(D):
    """a = 3, |a d| up to 100: float32 cosh overflows from |z| = 89 on; the kernel's |z| - log 2 + log1p(...) form does not."""
    shape = (3, 2, 4099)
    t = draw(shape, "generic")[1]
    d = np.random.default_rng(9).uniform(-100.0 / 3.0, 100.0 / 3.0, shape)
    p = (t + d).astype(np.float32)
    got = run(D, p, t, w_log_cosh=1.0, a=3.0)
    want = R.loss_and_grads(p, t, {"log_cosh": 1.0}, a=3.0)
    print("largest |a d|:", float(np.abs(3.0 * (p.astype(np.float64) - t)).max()))
    check("log_cosh a=3 wide", got, want, False)
    # and on the converged draw with a = 3: the small-argument branch
    p, t = draw(shape, "converged")
    check("log_cosh a=3 converged", run(D, p, t, w_log_cosh=1.0, a=3.0), R.loss_and_grads(p, t, {"log_cosh": 1.0}, a=3.0), False)


def test_two_runs_are_bit_identical(D):
    for shape in ((1, 1, 70001), (33, 1, 257)):
        p, t = draw(shape, "generic")
        opts = kw(MIX, w_log_cosh=1.0, w_snr=0.3)
        a, b = run(D, p, t, **opts), run(D, p, t, **opts)
        print(shape, "loss", float(a[0]), float(b[0]))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_bf16_in_bf16_out(D):
    p, t = draw((3, 2, 4099), "generic")
    pb, tb = dev(p).bfloat16().requires_grad_(True), dev(t).bfloat16().requires_grad_(True)
    loss = D.losses.time_domain_loss(pb, tb, **kw(MIX))
    loss.backward()
    assert loss.dtype == pb.grad.dtype == tb.grad.dtype == torch.bfloat16
    pf, tf = pb.detach().float().requires_grad_(True), tb.detach().float().requires_grad_(True)
    lf = D.losses.time_domain_loss(pf, tf, **kw(MIX))
    lf.backward()
    print("bf16 loss", float(loss.detach()), "float32 on the same values", float(lf.detach()))
    assert torch.equal(loss, lf.bfloat16()) and torch.equal(pb.grad, pf.grad.bfloat16()) and torch.equal(tb.grad, tf.grad.bfloat16())
    none = D.losses.time_domain_loss(pb.detach().half(), tb.detach().half(), w_esr=1.0, reduction="none")
    assert none.dtype == torch.float16 and none.shape == (3, 2)


def test_non_contiguous_input_equals_its_contiguous_copy(D):
    p, t = draw((3, 2, 4099), "generic")
    wide = torch.zeros(3, 2, 2 * 4099, device=DEV)
    wide[..., ::2] = dev(p)
    pn = wide[..., ::2].requires_grad_(True)
    tn = dev(t).transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    assert not pn.is_contiguous() and not tn.is_contiguous()
    loss = D.losses.time_domain_loss(pn, tn, **kw(MIX))
    loss.backward()
    want = run(D, p, t, **kw(MIX))
    print("non-contiguous loss", float(loss.detach()), "contiguous", float(want[0]))
    assert float(loss.detach()) == float(want[0])
    assert np.array_equal(pn.grad.cpu().double().numpy(), want[1]) and np.array_equal(tn.grad.cpu().double().numpy(), want[2])


MODULES = {"ESRLoss": "w_esr", "DCLoss": "w_dc", "LogCoshLoss": "w_log_cosh", "SNRLoss": "w_snr", "SISDRLoss": "w_si_sdr", "SDSDRLoss": "w_sd_sdr"}


@pytest.mark.parametrize("name", sorted(MODULES))
def test_module_equals_the_functional_form(D, name):
    p, t = draw((3, 2, 4099), "generic")
    for reduction in ("mean", "none"):
        pm, tm = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
        lm = getattr(D.losses, name)(reduction=reduction)(pm, tm)
        lm.sum().backward()
        pf, tf = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
        lf = D.losses.time_domain_loss(pf, tf, reduction=reduction, **{MODULES[name]: 1.0})
        lf.sum().backward()
        print(name, reduction, lm.flatten()[:2].tolist())
        assert torch.equal(lm, lf) and torch.equal(pm.grad, pf.grad) and torch.equal(tm.grad, tf.grad)


def conv_same(x, taps):
    return torch.nn.functional.conv1d(x.reshape(-1, 1, x.shape[-1]), taps.reshape(1, 1, -1), padding=taps.numel() // 2).reshape(x.shape)


@pytest.mark.parametrize("filter_type", ["hp", "fd", "aw"])
def test_fir_filter_against_float64_conv1d(D, filter_type):
    """Outputs and, through autograd with random upstream gradients on both outputs, input gradients against conv1d(padding=len // 2) in
    float64. Bounds: 2e-5 of the peak on the outputs (fp32 sums of at most 101 products: ~101 x 6e-8 of sum |taps| |x| at the very worst),
    the project's 1e-4 on the gradients."""
    shape = (2, 1, 300)
    p, t = draw(shape, "generic")
    fir = D.losses.FIRFilter(filter_type, coef=0.85, fs=44100)
    rng = np.random.default_rng(11)
    wp, wt = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    pt, tt = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
    yp, yt = fir(pt, tt)
    assert yp.shape == yt.shape == shape
    (yp * dev(wp)).sum().add((yt * dev(wt)).sum()).backward()
    taps = torch.from_numpy(np.asarray(fir._taps, dtype=np.float64))
    p64, t64 = torch.from_numpy(p.astype(np.float64)).requires_grad_(True), torch.from_numpy(t.astype(np.float64)).requires_grad_(True)
    rp, rt = conv_same(p64, taps), conv_same(t64, taps)
    ((rp * torch.from_numpy(wp.astype(np.float64))).sum() + (rt * torch.from_numpy(wt.astype(np.float64))).sum()).backward()
    ey = max(relmax(yp.detach().cpu().double().numpy(), rp.detach().numpy()), relmax(yt.detach().cpu().double().numpy(), rt.detach().numpy()))
    eg = [f(g.grad.cpu().double().numpy(), r.grad.numpy()) for g, r in ((pt, p64), (tt, t64)) for f in (rel2, relmax)]
    print(f"FIRFilter {filter_type}: outputs {ey:.2e} of the peak; gradients (rel L2, max) input {eg[0]:.2e} {eg[1]:.2e} target {eg[2]:.2e} {eg[3]:.2e}")
    assert ey < 2e-5 and max(eg) < GRAD_TOL
    # one argument only: the adjoint of the one gradient that exists
    p1 = dev(p).requires_grad_(True)
    y1, _ = fir(p1, dev(t))
    (y1 * dev(wp)).sum().backward()
    assert torch.equal(p1.grad, pt.grad)


def test_esr_behind_the_pre_emphasis_filter(D):
    shape = (2, 1, 300)
    p, t = draw(shape, "generic")
    pt, tt = dev(p).requires_grad_(True), dev(t).requires_grad_(True)
    loss = D.losses.ESRLoss()(*D.losses.FIRFilter("hp")(pt, tt))
    loss.backward()
    taps = torch.tensor([1.0, -0.85, 0.0], dtype=torch.float64)
    p64, t64 = torch.from_numpy(p.astype(np.float64)).requires_grad_(True), torch.from_numpy(t.astype(np.float64)).requires_grad_(True)
    ref = R.esr(conv_same(p64, taps), conv_same(t64, taps)).mean()
    ref.backward()
    check("ESRLoss()(*FIRFilter('hp')(p, t))", (loss.detach().cpu().double().numpy(), pt.grad.cpu().double().numpy(), tt.grad.cpu().double().numpy()),
          (ref.detach().numpy(), p64.grad.numpy(), t64.grad.numpy()), False)


def test_graph_replay_on_an_idle_device_equals_eager(D):
    """Forward + backward of the mix captured on a side stream (one stream, no parallel branches), replayed after a synchronise and a short
    sleep with new data in the same buffers: the launch sequence has no memset node and no counter, and the sums have a fixed order, so the
    replay equals eager bit for bit."""
    shape = (3, 2, 4099)
    opts = kw(MIX, w_log_cosh=0.5)
    fn = lambda p_, t_: D.losses.time_domain_loss(p_, t_, **opts)
    ps, ts = dev(draw(shape, "generic")[0]).requires_grad_(True), dev(draw(shape, "generic")[1]).requires_grad_(True)
    w = torch.ones((), device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn(ps, ts).backward(w)
    torch.cuda.current_stream().wait_stream(s)
    ps.grad = ts.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = fn(ps, ts)
        ys.backward(w)
    for k, kind in enumerate(("converged", "big_dc")):
        pn, tn = (dev(a) for a in draw(shape, kind))
        with torch.no_grad():
            ps.copy_(pn); ts.copy_(tn); w.fill_(1.0 + k)
        ps.grad.zero_(); ts.grad.zero_()
        torch.cuda.synchronize()
        time.sleep(0.05)                       # the device is idle when the replay starts
        graph.replay()
        torch.cuda.synchronize()
        pe, te = pn.clone().requires_grad_(True), tn.clone().requires_grad_(True)
        ye = fn(pe, te)
        ye.backward(w)
        print(f"replay {k} ({kind}): loss {float(ys.detach())} eager {float(ye.detach())}; max |delta| grads {float((ps.grad - pe.grad).abs().max())} {float((ts.grad - te.grad).abs().max())}")
        assert torch.equal(ys, ye) and torch.equal(ps.grad, pe.grad) and torch.equal(ts.grad, te.grad)
