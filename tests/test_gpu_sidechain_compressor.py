"""GPU tests of functional.sidechain_compressor and modules.SidechainCompressor: the composition equals its three ops called by hand
bit for bit; against the float64 restatement of the whole chain (tests/sidechain_restated.py) on (3, 2, 2 * 4096 + 3) it stays within the
composed bounds max(4 e32, floor), e32 the error of the chain at the kernels' arithmetic on the CPU; every gradient is finite, also at
knee_db == 0, and the release_ms gradient is real; with a key the gradient of x flows through the gain alone; the module round-trips
process_normalized."""
import numpy as np
import pytest
import torch

from tests import ballistics_cases as K
from tests import sidechain_restated as R
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, N = 44100, 2 * K.TILE + 3


def inputs(B=3, C=2, n=N, hop=64, key_chs=0, seed=0):
    """Bursts with a decay: noise under an envelope that jumps up every 2048 samples and falls off exponentially between."""
    g = torch.Generator().manual_seed(151 * seed + n + hop)
    env = torch.exp(-(torch.arange(n) % 2048) / 500.0) * (0.2 + torch.rand(B, 1, (n + 2047) // 2048, generator=g)).repeat_interleave(2048, -1)[..., :n]
    a = dict(x=torch.randn(B, C, n, generator=g) * env, w=torch.randn(B, C, n, generator=g))
    if key_chs:
        a["key"] = torch.randn(B, key_chs, n, generator=g) * env.flip(-1)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, generator=g)
    a["ctl"] = dict(threshold_db=u(-30.0, -12.0), ratio=u(2.0, 8.0), attack_ms=u(1.0, 10.0), release_ms=u(30.0, 120.0), knee_db=u(2.0, 10.0),
                    makeup_gain_db=u(0.0, 6.0))
    return a


def run_t(D, a, hop=64):
    x = a["x"].to(DEV).requires_grad_(True)
    key = a["key"].to(DEV).requires_grad_(True) if "key" in a else None
    c = {k: v.to(DEV).requires_grad_(True) for k, v in a["ctl"].items()}
    y = D.sidechain_compressor(x, SR, **c, key=key, hop=hop)
    leaves = [x] + ([key] if key is not None else []) + [c[k] for k in R.CTL]
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), leaves)
    torch.cuda.synchronize()
    out = dict(y=y.detach(), gx=grads[0], **{"g_" + k: g for k, g in zip(R.CTL, grads[-6:])})
    if key is not None:
        out["gkey"] = grads[1]
    return out


@pytest.fixture(scope="module")
def D():
    assert torch.cuda.is_available()
    import dasp_pytorch_amd as D
    return D


@pytest.mark.parametrize("key_chs", [0, 1])
def test_the_composition_is_its_three_ops_called_by_hand(D, key_chs):
    from dasp_pytorch_amd.functional import _soft_knee_level
    a = inputs(key_chs=key_chs)
    got = run_t(D, a)
    x = a["x"].to(DEV).requires_grad_(True)
    key = a["key"].to(DEV).requires_grad_(True) if key_chs else None
    c = {k: v.to(DEV).requires_grad_(True) for k, v in a["ctl"].items()}
    col = lambda k: c[k].reshape(-1, 1)
    L = D.block_level(x if key is None else key, SR, 64, "peak")
    l_db = 20.0 * torch.log10(L + 1e-5)
    r = l_db - _soft_knee_level(l_db, col("threshold_db"), col("ratio"), col("knee_db"))
    y = D.gain_curve(x, SR, col("makeup_gain_db") - D.ballistics(r, SR, c["attack_ms"], c["release_ms"], 64), 64)
    leaves = [x] + ([key] if key is not None else []) + [c[k] for k in R.CTL]
    grads = torch.autograd.grad((y * a["w"].to(DEV)).sum(), leaves)
    assert torch.equal(y, got["y"]) and torch.equal(grads[0], got["gx"])
    for k, g in zip(R.CTL, grads[-6:]):
        assert torch.equal(g, got["g_" + k]), k
    if key_chs:
        assert torch.equal(grads[1], got["gkey"])


@pytest.mark.parametrize("key_chs,hop", [(0, 64), (1, 8), (3, 2048)])
def test_parity_with_the_float64_chain(D, key_chs, hop):
    a = inputs(key_chs=key_chs, hop=hop)
    want = R.forward_backward(a["x"], SR, a["ctl"], a["w"], a.get("key"), hop)
    f32 = R.forward_backward(a["x"], SR, a["ctl"], a["w"], a.get("key"), hop, arith=torch.float32)
    assert np.array_equal(want["up"], f32["up"])                              # the yardstick walks the branches of the oracle
    got = {k: v.cpu().numpy() for k, v in run_t(D, a, hop).items()}
    names = [k for k in R.FLOOR if k in want]
    meas, fails = {}, []
    for k, (e32, bound) in K.bounds(want, f32, {k: R.FLOOR[k] for k in names}).items():
        e = K.per_item_err(got[k], want[k])
        meas[k], meas["fp32_" + k] = e, e32
        if not e <= bound:
            fails.append((k, e, e32, bound))
    record("sidechain_parity key_chs=%d hop=%d" % (key_chs, hop), **meas)
    assert not fails, fails


def test_gradients_are_finite_and_release_is_real(D):
    for knee in (6.0, 0.0):
        a = inputs(key_chs=1, seed=1)
        a["ctl"]["knee_db"] = torch.full((3,), knee)
        got = run_t(D, a)
        assert all(torch.isfinite(v).all() for v in got.values()), knee
        assert (got["g_release_ms"] != 0).all() and (got["g_attack_ms"] != 0).all() and got["gkey"].any()
    b = {**a, "ctl": dict(a["ctl"], release_ms=2.0 * a["ctl"]["release_ms"])}
    assert not torch.equal(run_t(D, b)["y"], got["y"])                        # and release_ms changes the output


def test_with_a_key_the_gradient_of_x_flows_through_the_gain_alone(D):
    a = inputs(key_chs=2)
    got = run_t(D, a)
    x, key = a["x"].to(DEV), a["key"].to(DEV)
    with torch.no_grad():
        G = D.sidechain_compressor(torch.ones_like(x), SR, **{k: v.to(DEV) for k, v in a["ctl"].items()}, key=key)
    assert torch.equal(got["gx"], a["w"].to(DEV) * G)                         # gx = w G, G the gain that the key alone decides
    solo = run_t(D, {k: v for k, v in a.items() if k != "key"})
    assert not torch.equal(solo["gx"], got["gx"])


def test_the_module_round_trips_process_normalized(D):
    a = inputs()
    m = D.SidechainCompressor(SR, hop=64)
    lo = torch.tensor([r[0] for r in m.param_ranges.values()])
    span = torch.tensor([r[1] - r[0] for r in m.param_ranges.values()])
    p = torch.rand(3, 6, generator=torch.Generator().manual_seed(3))
    x = a["x"].to(DEV)
    y = m.process_normalized(x, p.to(DEV))
    d = (p * span + lo).to(DEV)
    want = D.sidechain_compressor(x, SR, *[d[:, i] for i in range(6)], hop=64)
    assert y.shape == x.shape and torch.equal(y, want)
    with pytest.raises(ValueError, match="parameters"):
        m.process_normalized(x, p[:, :5].to(DEV))
    key = torch.randn(3, 1, N, device=DEV)
    assert torch.equal(m.process_fn(x, SR, *[d[:, i] for i in range(6)], key=key), D.sidechain_compressor(x, SR, *[d[:, i] for i in range(6)], key=key, hop=64))
