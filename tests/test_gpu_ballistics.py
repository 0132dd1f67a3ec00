"""GPU tests of ballistics (csrc/ballistics.hip): parity of E, grad P and both control gradients with the float64 restatement
(tests/ballistics_restated.py) on the cases of tests/ballistics_cases.py, per item within max(4 e32, floor) of the item's float64 peak
(floors 2e-6 for curves, 1e-5 for control gradients; e32 the error of the restatement at the kernel's arithmetic; no bound exceeds ten
floors, tests/test_ballistics_cpu.py); the branch masks exactly; the all-zero curve exactly; the step's rise and fall times;
bit-for-bit reproducibility (runs, item alone or in a batch, graph replay); where non-finite input reaches; views; the C ABI inside
guard words; the autograd and call-state contracts; dtypes."""
import numpy as np
import pytest
import torch

from tests import ballistics_cases as K
from tests import ballistics_restated as R
from tests.autograd_contract_cases import peak_err
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES, FLOOR = R.NAMES, R.FLOOR
CH = K.CHUNK


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    assert lib().dasp_ballistics_chunk() == CH
    return D


def lib():
    from dasp_pytorch_amd import _lib
    return _lib.lib()


def run_t(D, a, sr, hop=64, need=(True, True, True), saved=None):
    leaves = [a[k].to(DEV).requires_grad_(n) for k, n in zip(("P", "attack_ms", "release_ms"), need)]
    if saved is None:
        E = D.ballistics(leaves[0], sr, leaves[1], leaves[2], hop=hop)
    else:
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            E = D.ballistics(leaves[0], sr, leaves[1], leaves[2], hop=hop)
    grads = torch.autograd.grad((E * a["w"].to(DEV)).sum(), [l for l, n in zip(leaves, need) if n])
    torch.cuda.synchronize()
    return dict(zip(["E"] + [k for k, n in zip(NAMES[1:], need) if n], (E.detach(),) + grads))


def plain(B, F, seed=0):
    g = torch.Generator().manual_seed(139 * seed + 7 * B + F)
    t = lambda: torch.tensor(K.TIMES)[torch.randint(0, len(K.TIMES), (B,), generator=g)] * (0.5 + torch.rand(B, generator=g))
    return dict(P=K.curve(B, F, g), w=0.5 + 0.5 * torch.randn(B, F, generator=g), attack_ms=t(), release_ms=t())


def mask_of(saved):
    (up,) = [t for t in saved if t.dtype is torch.uint8]
    return up.cpu().numpy().astype(bool)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", K.BALLISTICS_CONFIGS, ids=lambda c: "sr%d-hop%d" % c[:2])
def test_parity_with_the_float64_restatement(D, cfg):
    sr, hop = cfg[:2]
    worst = {k: (0.0, 0.0, 0.0, 0) for k in NAMES}
    fails = []
    for f, b, want, f32 in K.ballistics_calls(cfg):
        saved = []
        got = {k: v.cpu().numpy() for k, v in run_t(D, b, sr, hop, saved=saved).items()}
        assert np.array_equal(mask_of(saved), want["up"]), (cfg, f)                  # the branch masks: exact
        for k, (e32, bound) in K.bounds(want, f32, FLOOR).items():
            assert got[k].shape == want[k].shape and bound <= 10 * FLOOR[k], (cfg, f, k, e32)
            e = K.per_item_err(got[k], want[k])
            if e / bound >= worst[k][0]:
                worst[k] = (e / bound, e, e32, f)
            if not e <= bound:
                fails.append((f, k, e, e32))
    record("ballistics_parity sr=%d hop=%d" % cfg[:2], **{k: worst[k][1] for k in NAMES}, **{"fp32_" + k: worst[k][2] for k in NAMES},
           **{"share_" + k: worst[k][0] for k in NAMES}, **{"F_" + k: worst[k][3] for k in NAMES})
    assert not fails, (cfg, fails)


def test_an_all_zero_curve_is_all_release_and_exact(D):
    sr, hop, F = 44100, 64, 2 * CH + 3
    a = plain(3, F)
    a["P"] = torch.zeros_like(a["P"])
    saved = []
    got = run_t(D, a, sr, hop, saved=saved)
    want = R.by_hand(a["P"].numpy(), sr, a["attack_ms"].numpy(), a["release_ms"].numpy(), a["w"].numpy(), hop)
    assert not got["E"].any() and not mask_of(saved).any()
    assert np.array_equal(got["gP"].cpu().numpy().astype(np.float64), want["gP"]) and got["gP"].any()          # gP = c_r Lambda, as restated
    assert not got["gatt"].any() and not got["grel"].any()


def test_equal_times_are_the_linear_one_pole(D):
    sr, hop, F = 44100, 64, CH + 7
    a = plain(3, F)
    a["release_ms"] = a["attack_ms"].clone()
    E = run_t(D, a, sr, hop)["E"].cpu().double().numpy()
    c = R.item_constants(sr, hop, a["attack_ms"].numpy())[0]
    e, want = np.zeros(3), np.zeros((3, F))
    P = a["P"].double().numpy()
    for j in range(F):
        e = (1.0 - c) * e + c * P[:, j]
        want[:, j] = e
    assert K.per_item_err(E, want) <= FLOOR["E"]


@pytest.mark.parametrize("sr,hop,att,rel", [(44100, 8, 5.0, 100.0), (44100, 64, 20.0, 200.0), (8000, 8, 100.0, 5.0)])
def test_step_rise_and_fall_times(D, sr, hop, att, rel):
    """The 10 - 90 % rise and fall times of a step are attack_ms and release_ms to within one hop."""
    split = int(6 * max(att, rel) * sr / 1000.0 / hop) + 2
    P = torch.cat([torch.ones(1, split), torch.zeros(1, split)], 1)
    with torch.no_grad():
        E = D.ballistics(P.to(DEV), sr, torch.tensor([att], device=DEV), torch.tensor([rel], device=DEV), hop=hop)[0].cpu().numpy()
    rise, fall = R.rise_and_fall_ms(np.concatenate([[0.0], E]), sr, hop, 0.0, 1.0, split + 1)
    one_hop = hop * 1000.0 / sr
    assert abs(rise - att) <= one_hop and abs(fall - rel) <= one_hop, (rise, fall)


def test_clamped_times_have_exactly_zero_gradient(D):
    a = plain(4, CH + 7)
    a["attack_ms"] = torch.tensor([0.01, 20000.0, 5.0, 50.0])
    a["release_ms"] = torch.tensor([5.0, 50.0, 0.05, 10001.0])
    got = run_t(D, a, 44100)
    ga, gr = got["gatt"].cpu().numpy(), got["grel"].cpu().numpy()
    assert ga[0] == 0 and ga[1] == 0 and ga[2] != 0 and ga[3] != 0 and gr[0] != 0 and gr[1] != 0 and gr[2] == 0 and gr[3] == 0


# ---- 2. reproducibility ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_runs_items_and_subsets_are_bit_identical(D, hop):
    a = plain(5, 2 * CH + 3, seed=hop)
    p, q = run_t(D, a, 44100, hop), run_t(D, a, 44100, hop)
    for k in NAMES:
        assert torch.equal(p[k], q[k]), k
    for b in (0, 3):
        alone = run_t(D, {k: v[b:b + 1] for k, v in a.items()}, 44100, hop)
        for k in NAMES:
            assert torch.equal(p[k][b], alone[k][0]), (b, k)
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):      # the skipped outputs change nothing
        r = run_t(D, a, 44100, hop, need)
        for k in r:
            assert torch.equal(p[k], r[k]), (need, k)
    with torch.no_grad():
        assert torch.equal(D.ballistics(a["P"].to(DEV), 44100, a["attack_ms"].to(DEV), a["release_ms"].to(DEV), hop=hop), p["E"])


@pytest.mark.parametrize("hop", [8, 64, 2048])
def test_graph_replay_equals_eager(D, hop):
    sr = 44100
    a = plain(4, 2 * CH + 3, seed=hop)
    eager = run_t(D, a, sr, hop)
    leaves = [a[k].to(DEV).requires_grad_(True) for k in ("P", "attack_ms", "release_ms")]
    wt = a["w"].to(DEV)

    def step():
        E = D.ballistics(leaves[0], sr, leaves[1], leaves[2], hop=hop)
        return (E,) + torch.autograd.grad((E * wt).sum(), leaves)

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
            assert torch.equal(o.detach(), eager[key]), (k, key)


# ---- 3. off the nominal domain -----------------------------------------------------------------------------------------------------------
def test_a_nan_frame_makes_its_item_nan_from_there_on(D):
    F = 2 * CH + 3
    a = plain(3, F)
    clean = run_t(D, a, 44100)
    for j0 in (0, 1, CH - 1, CH, F - 1):
        b = {k: v.clone() for k, v in a.items()}
        b["P"][1, j0] = float("nan")
        dirty = run_t(D, b, 44100)
        for k in NAMES:
            assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), (j0, k)
        assert torch.isnan(dirty["E"][1, j0:]).all() and torch.equal(dirty["E"][1, :j0], clean["E"][1, :j0]), j0


def test_a_nan_control_poisons_its_own_item_only(D):
    a = plain(3, CH + 7)
    clean = run_t(D, a, 44100)
    for name in R.CTL:
        b = {k: v.clone() for k, v in a.items()}
        b[name][1] = float("nan")
        dirty = run_t(D, b, 44100)
        for k in NAMES:
            assert torch.equal(clean[k][0], dirty[k][0]) and torch.equal(clean[k][2], dirty[k][2]), (name, k)
            assert torch.isnan(dirty[k][1]).all(), (name, k)


@pytest.mark.parametrize("view", ["offset", "strided"])
def test_input_views(D, view):
    B, F = 3, 2 * CH + 3
    a = plain(B, F)
    want = run_t(D, a, 44100)
    P = a["P"].to(DEV)
    if view == "offset":
        Pv = torch.cat([torch.zeros(3, device=DEV), P.reshape(-1)])[3:].view(B, F)
    else:
        Pv = P.t().contiguous().t()
        assert not Pv.is_contiguous()
    assert torch.equal(Pv, P)
    Pv.requires_grad_(True)
    att, rel = (torch.stack([a[k], a[k]], -1).to(DEV)[:, 1].requires_grad_(True) for k in R.CTL)                # strided controls
    E = D.ballistics(Pv, 44100, att, rel)
    grads = torch.autograd.grad((E * a["w"].to(DEV)).sum(), [Pv, att, rel])
    for k, g in zip(NAMES, (E,) + grads):
        assert torch.equal(g, want[k]), k


def test_c_abi_keeps_guard_words_and_refuses_before_it_launches(D):
    from dasp_pytorch_amd._lib import ptr, stream
    sr, hop, G = 44100.0, 64, 64
    Lb = lib()
    for B, F in ((3, 1), (3, CH + 1), (2, 2 * CH + 3)):
        a = plain(B, F)
        P, w, att, rel = (a[k].to(DEV) for k in ("P", "w", "attack_ms", "release_ms"))

        def guarded(n, dtype=torch.float32):
            buf = torch.full((n + 2 * G,), float("nan"), device=DEV) if dtype is torch.float32 else torch.full((n + 2 * G,), 7, dtype=dtype, device=DEV)
            return buf, buf[G:G + n]

        def run(sr=sr, expect=0, want=(True, True, True)):
            bufs = dict(E=guarded(B * F), up=guarded(B * F, torch.uint8), gP=guarded(B * F), ga=guarded(B), gr=guarded(B))
            assert Lb.dasp_ballistics_forward(ptr(P), ptr(att), ptr(rel), ptr(bufs["E"][1]), ptr(bufs["up"][1]), B, F, hop, sr, stream()) == expect
            outs = [ptr(bufs[k][1] if on else None) for k, on in zip(("gP", "ga", "gr"), want)]
            assert Lb.dasp_ballistics_backward(ptr(P), ptr(att), ptr(rel), ptr(bufs["E"][1]), ptr(bufs["up"][1]), ptr(w), *outs, B, F, hop, sr,
                                               stream()) == expect
            torch.cuda.synchronize()
            for k, (buf, inner) in bufs.items():
                edge = torch.cat([buf[:G], buf[-G:]])
                assert (edge == 7).all() if inner.dtype is torch.uint8 else torch.isnan(edge).all(), k
            return {k: inner.clone() for k, (buf, inner) in bufs.items()}

        got, ref = run(), run_t(D, a, sr, hop)
        assert torch.equal(got["E"].view(B, F), ref["E"]) and torch.equal(got["gP"].view(B, F), ref["gP"])
        assert torch.equal(got["ga"], ref["gatt"]) and torch.equal(got["gr"], ref["grel"])
        part = run(want=(False, True, False))
        assert torch.equal(part["ga"], got["ga"]) and torch.isnan(part["gP"]).all() and torch.isnan(part["gr"]).all()
        refused = run(sr=float("nan"), expect=-1)
        assert all(torch.isnan(refused[k]).all() for k in ("E", "gP", "ga", "gr")) and (refused["up"] == 7).all()
    assert lib().dasp_device_error() == 0


# ---- 4. the autograd and call-state contracts -------------------------------------------------------------------------------------------------
def _spec():
    """The op's entry for the contract batteries, in the form of the entries of tests/autograd_contract_cases.py (that table is closed).
    What is watched is BallisticsKernels, the class that holds the forward / backward pair that BallisticsFunction binds to autograd."""
    from dasp_pytorch_amd._ctypes_ops import BallisticsKernels
    from tests import autograd_contract_cases as A
    sr, hop, F = 8000, 64, CH + 70

    def arrays(seed):
        g = A.gen(seed, 191)
        return dict(curve=K.curve(3, F, g), attack_ms=torch.rand(3, generator=g) * 45.0 + 5.0, release_ms=torch.rand(3, generator=g) * 400.0 + 20.0)

    def call(t):
        import dasp_pytorch_amd
        return dasp_pytorch_amd.ballistics(t["curve"], sr, t["attack_ms"], t["release_ms"], hop=hop)

    names = dict(E="y0", gP="g_curve", gatt="g_attack_ms", grel="g_release_ms")

    def ref(a, gys):
        w = torch.from_numpy(gys[0])
        r64 = R.forward_backward(a["curve"], sr, a["attack_ms"], a["release_ms"], w, hop)
        r32 = R.forward_backward(a["curve"], sr, a["attack_ms"], a["release_ms"], w, hop, arith=torch.float32)
        bound = {names[k]: max(4.0 * peak_err(r32[k], r64[k]), FLOOR[k]) for k in names}
        return dict({names[k]: r64[k] for k in names}, _bound=bound)
    spec = A.measured_bound("ballistics", arrays, call, ("curve", "attack_ms", "release_ms"), ("curve",), ("BallisticsKernels",), ref,
                            {names[k]: FLOOR[k] for k in names}, forms={"attack_ms": "vector", "release_ms": "vector"}, lowp=("curve",),
                            outs=lambda a: [(3, F)], cite="tests/test_gpu_ballistics.py test_parity_with_the_float64_restatement")
    spec.functions = lambda: [BallisticsKernels]
    return spec


def _contract(checks, check):
    spec, rec = _spec(), []
    try:
        find = checks[check](spec, rec)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in ballistics {check}: {e}", returncode=3)          # nothing more runs on a device that has faulted
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


def test_what_the_forward_pass_saves(D):
    B, F = 3, CH + 7
    a = plain(B, F)
    saved = []
    run_t(D, a, 44100, saved=saved)
    assert sorted((t.numel(), str(t.dtype)) for t in saved) == sorted([(B * F, "torch.float32")] * 2 + [(B * F, "torch.uint8")] + [(B, "torch.float32")] * 2)
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        D.ballistics(a["P"].to(DEV), 44100, a["attack_ms"].to(DEV), a["release_ms"].to(DEV))
    assert not saved


# ---- 5. dtypes and the empty batch ------------------------------------------------------------------------------------------------------------
def test_half_and_bfloat16_are_converted_and_float64_is_refused(D):
    from dasp_pytorch_amd import _lib
    a = plain(2, 300)
    att, rel = a["attack_ms"].to(DEV), a["release_ms"].to(DEV)
    for dt in (torch.float16, torch.bfloat16):
        Pl = a["P"].to(DEV).to(dt)
        with torch.no_grad():
            E = D.ballistics(Pl, 44100, att, rel)
            want = D.ballistics(Pl.float(), 44100, att, rel).to(dt)
        assert E.dtype == dt and torch.equal(E, want)
    with pytest.raises(_lib.DaspHipError, match="ballistics: float64"):
        D.ballistics(a["P"].to(DEV).double(), 44100, att, rel)
    E = D.ballistics(torch.zeros(0, 5, device=DEV, requires_grad=True), 44100, torch.ones(0, device=DEV), torch.ones(0, device=DEV))
    assert E.shape == (0, 5)
    E.sum().backward()
