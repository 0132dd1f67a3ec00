"""GPU tests of block_level (csrc/ballistics.hip): peak exact - L, grad x and the saved winners bit for bit what
tests/block_level_restated.py gives - power within max(4 e32, 2e-6) of the float64 restatement per item, on the cases of
tests/ballistics_cases.py; bit-for-bit reproducibility (runs, item alone or in a batch, graph replay), where a NaN sample reaches,
views, the C ABI inside guard words, the autograd and call-state contracts, dtypes and the empty signal."""
import numpy as np
import pytest
import torch

from tests import ballistics_cases as K
from tests import block_level_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES, FLOOR = R.NAMES, R.FLOOR
T = K.TILE


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    assert lib().dasp_envelope_tile() == T
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def run_t(D, a, hop=64, det="peak", saved=None):
    x = a["x"].to(DEV).requires_grad_(True)
    if saved is None:
        L = D.block_level(x, 44100, hop=hop, detector=det)
    else:
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            L = D.block_level(x, 44100, hop=hop, detector=det)
    (gx,) = torch.autograd.grad((L * a["w"].to(DEV)).sum(), [x])
    torch.cuda.synchronize()
    return dict(L=L.detach(), gx=gx)


def plain(B, C, N, hop=64, seed=0, ties=False):
    g = torch.Generator().manual_seed(137 * seed + 7 * B + 3 * C + N)
    env = torch.exp(0.8 * torch.randn(B, 1, (N + 255) // 256, generator=g)).repeat_interleave(256, -1)[..., :N]
    x = 0.3 * torch.randn(B, C, N, generator=g) * env
    return dict(x=torch.round(4 * x) / 4 if ties else x, w=0.5 + 0.5 * torch.randn(B, R.control_frames(N, hop), generator=g))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", K.BLOCK_LEVEL_CONFIGS, ids=lambda c: "hop%d-C%d-%s-ties%d" % c[:4])
def test_parity_with_the_restatement(D, cfg):
    hop, chs, det, ties, seed = cfg
    worst = {k: (0.0, 0.0, 0.0, 0) for k in NAMES}
    fails = []
    for n, b, want, hand in K.block_level_calls(cfg):
        saved = []
        got = {k: v.cpu().numpy() for k, v in run_t(D, b, hop, det, saved).items()}
        if det == "peak":                                                    # exact, and x itself is not saved
            assert [tuple(t.shape) for t in saved] == [(K.BS, R.control_frames(n, hop))] and saved[0].dtype == torch.int32, n
            assert np.array_equal(saved[0].cpu().numpy(), hand["win"]), (cfg, n)
            for k in NAMES:
                assert np.array_equal(got[k].astype(np.float64), hand[k]), (cfg, n, k)
                assert np.array_equal(hand[k], want[k]), (cfg, n, k)
            continue
        assert len(saved) == 1 and saved[0].shape == b["x"].shape
        for k, (e32, bound) in K.bounds(want, hand, FLOOR).items():
            assert got[k].shape == want[k].shape and bound <= 10 * FLOOR[k], (cfg, n, k, e32)
            e = K.per_item_err(got[k], want[k])
            if e / bound >= worst[k][0]:
                worst[k] = (e / bound, e, e32, n)
            if not e <= bound:
                fails.append((n, k, e, e32))
    if det == "power":
        record("block_level_parity hop=%d C=%d %s" % cfg[:3], **{k: worst[k][1] for k in NAMES}, **{"fp32_" + k: worst[k][2] for k in NAMES},
               **{"share_" + k: worst[k][0] for k in NAMES}, **{"n_" + k: worst[k][3] for k in NAMES})
    assert not fails, (cfg, fails)


def test_repeated_maxima_go_to_the_earliest_sample_and_the_lowest_channel(D):
    hop, N = 8, 41
    x = torch.zeros(1, 3, N)
    x[0, 1, 3], x[0, 2, 3], x[0, 0, 5], x[0, 1, 8] = -0.5, 0.5, 0.5, 0.5          # block 1 = samples 1 .. 8: four equal maxima
    x[0, 2, 16] = 0.25                                                            # block 2: its last sample
    a = dict(x=x, w=torch.arange(1.0, R.control_frames(N, hop) + 1)[None])
    got = run_t(D, a, hop)
    gx = got["gx"][0].cpu()
    assert got["L"][0, :3].tolist() == [0.0, 0.5, 0.25]
    want = torch.zeros(3, N)
    want[1, 3], want[2, 16] = -2.0, 3.0
    assert torch.equal(gx, want)


def test_silence_gives_zero_and_a_written_zero_gradient(D):
    for det in R.DETECTORS:
        a = plain(2, 2, T + 70)
        a["x"] = torch.zeros_like(a["x"])
        got = run_t(D, a, 64, det)
        assert not got["L"].any() and not got["gx"].any() and torch.isfinite(got["gx"]).all()


# ---- 2. reproducibility ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,det", [(8, "power"), (64, "peak"), (2048, "peak"), (2048, "power")])
def test_runs_and_items_are_bit_identical(D, hop, det):
    a = plain(3, 2, 2 * T + 5, hop, ties=det == "peak")
    p, q = run_t(D, a, hop, det), run_t(D, a, hop, det)
    for k in NAMES:
        assert torch.equal(p[k], q[k]), k
    for b in (0, 2):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, hop, det)
        for k in NAMES:
            assert torch.equal(p[k][b], alone[k][0]), (b, k)
    with torch.no_grad():
        assert torch.equal(D.block_level(a["x"].to(DEV), 44100, hop=hop, detector=det), p["L"])


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_graph_replay_equals_eager(D, hop):
    for det in R.DETECTORS:
        a = plain(4, 2, 2 * T + 5, hop)
        eager = run_t(D, a, hop, det)
        xt, wt = a["x"].to(DEV).requires_grad_(True), a["w"].to(DEV)

        def step():
            L = D.block_level(xt, 44100, hop=hop, detector=det)
            return (L,) + torch.autograd.grad((L * wt).sum(), [xt])

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        for k in range(2):
            for o in outs:
                o.detach().zero_()
            graph.replay()
            torch.cuda.synchronize()
            for key, o in zip(NAMES, outs):
                assert torch.equal(o.detach(), eager[key]), (hop, det, k, key)


# ---- 3. off the nominal domain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", R.DETECTORS)
def test_a_nan_sample_reaches_its_own_frame_only(D, det):
    hop, N = 64, 2 * T + 5
    a = plain(3, 2, N)
    clean = run_t(D, a, hop, det)
    for m0 in (0, 1, hop, hop + 1, T, T + 1, N - 1):
        b = {k: v.clone() for k, v in a.items()}
        b["x"][1, 1, m0] = float("nan")
        dirty = run_t(D, b, hop, det)
        for k in NAMES:
            assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), (m0, k)
        j0 = -(-m0 // hop)
        hit = torch.arange(clean["L"].shape[1], device=DEV) == j0
        assert torch.isnan(dirty["L"][1][hit]).all() and torch.equal(dirty["L"][1][~hit], clean["L"][1][~hit]), m0
        lo, hi = (0, 1) if m0 == 0 else ((j0 - 1) * hop + 1, min(j0 * hop + 1, N))      # gx changes inside the sample's block at most
        keep = torch.ones(N, dtype=torch.bool, device=DEV)
        keep[lo:hi] = False
        assert torch.equal(dirty["gx"][1][:, keep], clean["gx"][1][:, keep]), m0
        if det == "peak":                                                    # the NaN sample is the winner: the rest of its block is zero
            blk = dirty["gx"][1][:, lo:hi]
            assert torch.isnan(blk[1, m0 - lo]) and torch.isnan(blk).sum() == 1 and not torch.nan_to_num(blk).any(), m0


def test_a_nan_upstream_gradient_stays_in_its_frame(D):
    hop, N = 64, T + 70
    a = plain(2, 2, N)
    clean = run_t(D, a, hop, "power")
    b = {k: v.clone() for k, v in a.items()}
    b["w"][1, 5] = float("nan")
    dirty = run_t(D, b, hop, "power")
    blk = slice(4 * hop + 1, 5 * hop + 1)
    assert torch.equal(clean["gx"][0], dirty["gx"][0]) and torch.isnan(dirty["gx"][1][:, blk]).all()
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[blk] = False
    assert torch.equal(dirty["gx"][1][:, keep], clean["gx"][1][:, keep])


@pytest.mark.parametrize("view", ["offset", "strided", "sliced"])
def test_input_views(D, view):
    N = 2 * T + 5
    a = plain(3, 2, N)
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
    for det in R.DETECTORS:
        want = run_t(D, a, 64, det)
        xl = xv.detach().requires_grad_(True)
        L = D.block_level(xl, 44100, detector=det)
        (gx,) = torch.autograd.grad((L * a["w"].to(DEV)).sum(), [xl])
        assert torch.equal(L, want["L"]) and torch.equal(gx, want["gx"]), det


def test_c_abi_keeps_guard_words_and_refuses_before_it_launches(D):
    from dasp_pytorch_amd._lib import ptr, stream
    G = 64
    B, C, N = 3, 2, 2 * T + 5
    Lb = lib()
    for hop in (8, 2048):
        F = R.control_frames(N, hop)
        a = plain(B, C, N, hop)
        x, gL = a["x"].to(DEV), a["w"].to(DEV)

        def guarded(n, dtype=torch.float32):
            buf = torch.full((n + 2 * G,), float("nan"), device=DEV).view(dtype) if dtype is torch.float32 else torch.full((n + 2 * G,), -7, dtype=dtype, device=DEV)
            return buf, buf[G:G + n]

        def intact(buf, dtype):
            edge = torch.cat([buf[:G], buf[-G:]])
            return torch.isnan(edge).all() if dtype is torch.float32 else (edge == -7).all()

        for det in (0, 1):
            def run(hop=hop, expect=0):
                bufs = dict(L=guarded(B * F), win=guarded(B * F, torch.int32), gx=guarded(B * C * N))
                assert Lb.dasp_blocklevel_forward(ptr(x), ptr(bufs["L"][1]), ptr(bufs["win"][1]), B, C, N, hop, det, stream()) == expect
                assert Lb.dasp_blocklevel_backward(ptr(x if det else None), ptr(None if det else bufs["win"][1]), ptr(gL), ptr(bufs["gx"][1]), B, C, N,
                                                   hop, det, stream()) == expect
                torch.cuda.synchronize()
                for k, (buf, inner) in bufs.items():
                    assert intact(buf, inner.dtype), (k, det)
                return {k: inner.clone() for k, (buf, inner) in bufs.items()}

            got = run()
            ref = run_t(D, a, hop, R.DETECTORS[det])
            assert torch.equal(got["L"].view(B, F), ref["L"]) and torch.equal(got["gx"].view(B, C, N), ref["gx"])
            refused = run(hop=24, expect=-2)                                  # nothing launched: every word is as it was
            assert torch.isnan(refused["L"]).all() and torch.isnan(refused["gx"]).all() and (refused["win"] == -7).all()
    assert lib().dasp_device_error() == 0


# ---- 4. the autograd and call-state contracts -------------------------------------------------------------------------------------------------
def _spec(det="power"):
    """The op's entry for the contract batteries, in the form of the entries of tests/autograd_contract_cases.py (that table is closed).
    What is watched is BlockLevelKernels, the class that holds the forward / backward pair that BlockLevelFunction binds to autograd."""
    from dasp_pytorch_amd._ctypes_ops import BlockLevelKernels
    from tests import autograd_contract_cases as A
    hop, N = 64, 1501
    F = R.control_frames(N, hop)

    def arrays(seed):
        g = A.gen(seed, 181)
        return dict(x=0.5 * torch.randn(3, 2, N, generator=g))

    def call(t):
        import dasp_pytorch_amd
        return dasp_pytorch_amd.block_level(t["x"], 8000, hop=hop, detector=det)

    names = dict(L="y0", gx="g_x")

    def ref(a, gys):
        w = torch.from_numpy(gys[0])
        r64 = R.forward_backward(a["x"], w, hop, det)
        r32 = R.forward_backward(a["x"], w, hop, det, arith=torch.float32)
        bound = {names[k]: max(4.0 * peak_err(r32[k], r64[k]), FLOOR[k]) for k in names}
        return dict({names[k]: r64[k] for k in names}, _bound=bound)
    spec = A.measured_bound("block_level", arrays, call, ("x",), ("x",), ("BlockLevelKernels",), ref, {names[k]: FLOOR[k] for k in names},
                            lowp=("x",), outs=lambda a: [(3, F)], cite="tests/test_gpu_block_level.py test_parity_with_the_restatement")
    spec.functions = lambda: [BlockLevelKernels]
    return spec


def _contract(checks, check, det):
    spec, rec = _spec(det), []
    try:
        find = checks[check](spec, rec)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in block_level {check}: {e}", returncode=3)          # nothing more runs on a device that has faulted
        raise
    torch.cuda.synchronize()
    assert lib().dasp_device_error() == 0
    assert not find, "\n".join(find)


@pytest.mark.parametrize("det", R.DETECTORS)
@pytest.mark.parametrize("check", ["C1_subsets", "C2_repeat", "C3_interleave", "C4_upstream_forms", "C5_leaf_forms", "C6_mutation", "C7_streams"])
def test_autograd_contract(D, check, det):
    from tests import autograd_contract_checks as C
    _contract(C.CHECKS, check, det)


@pytest.mark.parametrize("check", ["S1_arguments", "S4_memory"])
def test_call_state(D, check):
    from tests import call_state_checks as S
    _contract(S.CHECKS, check, "peak")


def test_no_gradient_saves_nothing_and_double_backward_is_refused(D):
    a = plain(2, 1, 600)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.block_level(a["x"].to(DEV), 44100)
    assert not saved
    x = a["x"].to(DEV).requires_grad_(True)
    L = D.block_level(x, 44100, detector="power")
    (gx,) = torch.autograd.grad(L.pow(2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 5. dtypes and the empty signal ---------------------------------------------------------------------------------------------------------
def test_empty_input(D):
    for B, C, N, F in ((2, 2, 0, 1), (0, 2, 16, 3)):
        x = torch.zeros(B, C, N, device=DEV, requires_grad=True)
        L = D.block_level(x, 44100, hop=8)
        assert L.shape == (B, F) and not L.any()
        L.sum().backward()
        assert x.grad.shape == x.shape


def test_half_and_bfloat16_are_converted_and_float64_is_refused(D):
    from dasp_pytorch_amd import _lib
    a = plain(2, 2, 3000)
    for dt in (torch.float16, torch.bfloat16):
        xl = a["x"].to(DEV).to(dt)
        with torch.no_grad():
            L = D.block_level(xl, 44100)
            want = D.block_level(xl.float(), 44100).to(dt)
        assert L.dtype == dt and torch.equal(L, want)
    with pytest.raises(_lib.DaspHipError, match="block_level: float64"):
        D.block_level(a["x"].to(DEV).double(), 44100)
