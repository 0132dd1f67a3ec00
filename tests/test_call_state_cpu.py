"""The call-state battery without a GPU (tests/call_state_checks.py, tests/call_state_cases.py):

* the battery catches what it claims: pure-torch toy ops, one correct and one planted defect per row of the table below; S1 - S4 pass
  the correct toy, and every defect is flagged by its own check and by no other (S5 - S7 need a device);
* every added entry's float64 reference evaluates once on the entry's own shape; the ones that need the device are listed;
* the jump table of the random-stream reproduction (dasp_pytorch_amd/_mt19937.py) is used only when it is this module's table: a
  flipped bit, another JUMP, the old format and a truncated file are rebuilt, a read-only directory is no error;
* _PendingState.finish() notices a draw from the global CPU generator between the device draw and itself;
* a private torch.Generator has the global generator's state layout, stream and states (what the self-check now relies on)."""
import os
import warnings

import numpy as np
import pytest
import torch

from dasp_pytorch_amd import _mt19937 as mt

from tests import autograd_contract_cases as T
from tests import autograd_contract_checks as K
from tests import call_state_cases as C
from tests import call_state_checks as S
from tests.autograd_contract_checks import Spec

CPU_CHECKS = ("S1_arguments", "S2_rng", "S3_ambient", "S4_memory")
_KEPT = []


def _toy(defect=None):
    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            if defect == "writes_through_data":
                a.data.add_(1.0)                                     # bits change, the version does not
            if defect == "bumps_version":
                a.detach().mul_(1)                                   # the version changes, bits do not
            ctx.save_for_backward(a.detach().clone(), b.detach().clone())
            y = a.detach() * b.detach().view(-1, 1, 1)
            if defect == "module_list":
                _KEPT.append(y)
            if defect == "output_on_ctx":
                ctx.y = y                                            # y -> grad_fn -> ctx -> y
            return y

        @staticmethod
        def backward(ctx, g):
            a, b = ctx.saved_tensors
            return g * b.view(-1, 1, 1), (g * a).sum((1, 2))

    def call(t):
        y = Toy.apply(t["a"], t["b"])
        if defect == "manual_seed":
            torch.manual_seed(7)
        if defect == "draws_one_value":
            torch.rand(1)
        if defect == "grad_mode_off":
            torch.set_grad_enabled(False)
        if defect == "default_dtype":
            torch.set_default_dtype(torch.float64)
        return y
    return call


def toy_spec(defect=None):
    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return dict(a=torch.randn(3, 2, 7, generator=g), b=torch.rand(3, generator=g) + 0.5)
    return Spec("toy_" + (defect or "correct"), make, _toy(defect), ("a", "b"), audio=("a",), forms={"b": "vector"})


DEFECTS = {"writes_through_data": "S1_arguments", "bumps_version": "S1_arguments", "manual_seed": "S2_rng", "draws_one_value": "S2_rng",
           "grad_mode_off": "S3_ambient", "default_dtype": "S3_ambient", "module_list": "S4_memory", "output_on_ctx": "S4_memory"}


@pytest.fixture(autouse=True)
def put_back():
    state, grad, dt = torch.get_rng_state(), torch.is_grad_enabled(), torch.get_default_dtype()
    yield
    torch.set_rng_state(state)
    torch.set_grad_enabled(grad)
    torch.set_default_dtype(dt)
    _KEPT.clear()


def findings(check, spec, rec=None):
    rec = [] if rec is None else rec
    kw = {"counter": S.live_tensor_bytes} if check == "S4_memory" else {}
    with S.isolated():
        return S.CHECKS[check](spec, rec, **kw)


@pytest.mark.parametrize("check", CPU_CHECKS)
def test_the_correct_toy_passes(check):
    rec = []
    assert findings(check, toy_spec(), rec) == []
    assert rec, "the check measured nothing"


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_planted_defect_is_flagged_by_its_own_check_only(defect):
    flagged = {check: findings(check, toy_spec(defect)) for check in CPU_CHECKS}
    assert {c for c, f in flagged.items() if f} == {DEFECTS[defect]}, (defect, flagged)


def test_every_cpu_check_owns_two_defects():
    assert sorted(DEFECTS.values()) == sorted(CPU_CHECKS * 2)


def test_a_documented_draw_is_the_only_draw_allowed():
    """S2 on an entry that is documented to draw: passes where the CPU generator is left exactly where that draw leaves it, flags a draw of
    another size, and flags a documented draw that is not made."""
    def spec(n_drawn, n_documented):
        s = Spec("toy_draws", lambda seed: dict(a=torch.ones(3)), lambda t: (t["a"] * 2 + 0 * torch.randn(n_drawn).sum() if n_drawn else t["a"] * 2), ("a",))
        s.draws = (lambda: torch.randn(n_documented)) if n_documented else None
        return s
    assert findings("S2_rng", spec(32, 32)) == []
    assert findings("S2_rng", spec(48, 32)) and findings("S2_rng", spec(0, 32)) and findings("S2_rng", spec(32, 0))


# ---- the added entries ----------------------------------------------------------------------------------------------------------------------------

ON_DEVICE = sorted(e.name for e in C.extras() if e.on_device)
NO_REFERENCE = sorted(e.name for e in C.extras() if e.reference_at is None and not e.on_device)


def test_the_added_entries_are_the_ones_the_contract_table_cannot_hold():
    names = [e.name for e in C.extras()]
    assert len(names) == 9 and not set(names) & {e.name for e in T.table()}
    assert ON_DEVICE == ["reverb_device_noise_unseeded[ctypes]", "reverb_device_noise_unseeded[torch_ops]", "reverb_noise_stream"]
    assert NO_REFERENCE == []
    drawing = sorted(e.name for e in C.extras() if e.draws is not None)
    assert drawing == sorted(n for n in names if n != "reverb_noise_stream")
    for check, out in C.EXEMPT.items():
        assert len(out) <= 5 and set(out) <= {e.name for e in C.entries()}, check


@pytest.mark.parametrize("name", [e.name for e in C.extras() if e.reference_at is not None and not e.on_device])
def test_every_added_reference_evaluates_on_the_entry_shape(name):
    spec = C.by_name()[name]
    state = torch.get_rng_state()
    shapes = spec.outs(0)
    gys = K.upstream([torch.zeros(s, dtype=torch.float64) for s, _ in shapes], 0)
    ref = spec.reference_at(state, 0, gys)
    assert torch.equal(torch.get_rng_state(), state), "the reference drew from the global generator"
    t = spec.make(0, "cpu")
    for i, (shape, _) in enumerate(shapes):
        y = T.as_np(ref["y%d" % i])
        assert np.isfinite(y).all() and y.shape == tuple(shape), (name, y.shape, shape)
    for leaf in spec.leaves:
        g = T.as_np(ref["g_" + leaf])
        assert np.isfinite(g).all() and g.size == t[leaf].numel(), (name, leaf, g.shape)
    # the reference is the documented draw: the same values the global generator hands out from that state
    if name.startswith("randn_cpu_stream"):
        spec.draws()
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        assert np.array_equal(T.as_np(ref["y0"]), torch.randn(shapes[0][0]).double().numpy()) and torch.equal(torch.get_rng_state(), after)


def test_the_contract_table_is_unchanged_by_the_added_entries():
    assert len(T.table()) == 112 and len(C.entries()) == 112 + 9
    reached = {r for e in T.table() for r in e.reaches}
    assert set(T.package_functions()) <= reached and set(T.registered_ops()) <= reached


# ---- a private generator is the global one -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,burn,n", [(20240601, 0, 16387), (7, 100, 4096)])
def test_a_private_generator_has_the_global_generators_layout_and_stream(seed, burn, n):
    g = torch.Generator()
    g.manual_seed(seed)
    torch.manual_seed(seed)
    if burn:
        assert torch.equal(torch.rand(burn, generator=g), torch.rand(burn))
    s0 = g.get_state()
    assert s0.numel() == mt.STATE_BYTES and torch.equal(s0, torch.get_rng_state())
    words, left = mt.parse_state(s0)
    assert torch.equal(torch.randn(n, generator=g), torch.randn(n))
    assert torch.equal(g.get_state(), torch.get_rng_state())
    w1, l1 = mt.parse_state(g.get_state())
    assert torch.equal(mt.format_state(s0, w1, l1), g.get_state()) and mt.plan(left, n)[2] == l1


def test_the_self_check_touches_no_global_generator(monkeypatch):
    """_run_self_check with the device draw replaced by the layout model (oracle/mt_stream.py): it passes, and torch's, numpy's and
    random's global generators are where they were."""
    from oracle import mt_stream as ms

    def fake(words, left, out, max_piece=None):
        vals, cur, left_new = ms.randn(words, left, out.numel())
        out.copy_(torch.from_numpy(np.asarray(vals, np.float32)))
        return torch.from_numpy(np.asarray(cur, np.uint32).view(np.int32).copy()), left_new
    monkeypatch.setattr(mt, "_randn_from_state", fake)
    monkeypatch.setattr(torch, "manual_seed", lambda *a: pytest.fail("torch.manual_seed reseeds every device generator"))
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    spec = Spec("self_check", lambda seed: {}, lambda t: (), ())
    before = S.rng_states(spec)
    assert mt._run_self_check("cpu") is True
    after = S.rng_states(spec)
    assert all(S._equal(before[k], after[k]) for k in before)


# ---- the jump table ------------------------------------------------------------------------------------------------------------------------------

REAL_POLYNOMIALS = mt.jump_polynomials
_POLYS, _CALLS = [], []


def _polynomials_once():
    """jump_polynomials() takes five seconds; a rebuild under test gets the values of the first call, and is counted."""
    _CALLS.append(1)
    if not _POLYS:
        _POLYS.extend(REAL_POLYNOMIALS())
    return list(_POLYS)


@pytest.fixture()
def rebuilds(monkeypatch):
    monkeypatch.setattr(mt, "jump_polynomials", _polynomials_once)
    del _CALLS[:]
    return _CALLS


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("jump") / "table.npy")
    mt.jump_polynomials = _polynomials_once
    try:
        t = mt.build_table(path=path, force=True)
    finally:
        mt.jump_polynomials = REAL_POLYNOMIALS
    return path, t, open(path, "rb").read()


def _file(tmp_path, raw):
    path = str(tmp_path / "table.npy")
    with open(path, "wb") as f:
        f.write(raw)
    return path


def _forbid_rebuild(monkeypatch):
    monkeypatch.setattr(mt, "jump_polynomials", lambda: pytest.fail("the table was recomputed"))


def test_a_correct_file_is_loaded_without_recomputing(good, tmp_path, monkeypatch):
    _, table, raw = good
    _forbid_rebuild(monkeypatch)
    got = mt.build_table(path=_file(tmp_path, raw))
    assert got.shape == (mt.N_BABY + mt.N_GIANT, mt.ROW) and got.dtype == np.uint16 and np.array_equal(got, table)


def _flipped(raw, row, word, bit):
    """The file with one bit of one row flipped (the rows are the file's last (262 + 1) * ROW uint16)."""
    data = bytearray(raw)
    off = len(raw) - 2 * mt.ROW * (mt.N_BABY + mt.N_GIANT + 1) + 2 * (row * mt.ROW + word)
    data[off + bit // 8] ^= 1 << (bit % 8)
    return bytes(data)


# rows: a corner row and a row no corner check recomputes, for the baby and for the giant steps; the last: the key row itself
@pytest.mark.parametrize("row,word,bit", [(0, 5, 3), (100, 1246, 0), (254, 700, 15), (255, 0, 0), (258, 999, 7), (261, 12, 9), (262, 9, 1)],
                         ids=["baby_first", "baby_100", "baby_last", "giant_first", "giant_3", "giant_last", "key_row"])
def test_one_flipped_bit_is_rebuilt(good, tmp_path, rebuilds, row, word, bit):
    _, table, raw = good
    bad = _flipped(raw, row, word, bit)
    assert bad != raw and len(bad) == len(raw)
    if row < 262:
        assert not np.array_equal(np.load(_file(tmp_path, bad))[:-1], table)          # (the flip did land in that row)
        assert np.array_equal(np.delete(np.load(_file(tmp_path, bad))[:-1], row, 0), np.delete(table, row, 0))
    path = _file(tmp_path, bad)
    assert np.array_equal(mt.build_table(path=path), table) and len(rebuilds) == 1
    assert open(path, "rb").read() == raw, "the rewritten file is not the computed table"


def test_a_table_built_with_another_jump_is_rebuilt(good, tmp_path, monkeypatch):
    """A file that is right in itself (key, checksum, shape) for JUMP / 2: stale for this module."""
    _, table, raw = good
    path = str(tmp_path / "table.npy")
    with monkeypatch.context() as m:
        m.setattr(mt, "JUMP", mt.JUMP // 2)
        other = mt.build_table(path=path, force=True)             # (the one real build of this file: five seconds)
        assert mt._load_table(path) is not None                     # self-consistent under the constants it was built with
    assert other.shape == table.shape and not np.array_equal(other, table)
    assert mt._load_table(path) is None
    monkeypatch.setattr(mt, "jump_polynomials", _polynomials_once)
    assert np.array_equal(mt.build_table(path=path), table) and open(path, "rb").read() == raw
    # the same rows under a key forged for this module's constants: caught by the corner rows, which are recomputed
    forged = np.concatenate([other, mt._key_row(other)[None]])
    np.save(path, forged)
    assert mt._load_table(path) is None


def test_the_old_format_is_stale(good, tmp_path, rebuilds):
    _, table, raw = good
    path = str(tmp_path / "table.npy")
    np.save(path, table)                                             # shape and dtype right, no key: what the parent commit wrote
    assert mt._load_table(path) is None
    assert np.array_equal(mt.build_table(path=path), table) and open(path, "rb").read() == raw


@pytest.mark.parametrize("keep", [0, 64, 0.5, -1])
def test_a_truncated_file_is_rebuilt(good, tmp_path, rebuilds, keep):
    _, table, raw = good
    n = int(len(raw) * keep) if isinstance(keep, float) else (len(raw) + keep if keep < 0 else keep)
    path = _file(tmp_path, raw[:n])
    assert np.array_equal(mt.build_table(path=path), table) and open(path, "rb").read() == raw


def test_a_read_only_directory_is_no_error(good, tmp_path, rebuilds):
    """Nowhere to write: the correct table in memory, no exception, nothing left behind. (A directory without write permission, and -
    for a user whom permissions do not stop - a path whose directory does not exist.)"""
    _, table, raw = good
    ro = tmp_path / "ro"
    ro.mkdir()
    stale = ro / "table.npy"
    np.save(str(stale), table)
    os.chmod(ro, 0o555)
    try:
        assert np.array_equal(mt.build_table(path=str(stale)), table)
        assert [p.name for p in ro.iterdir()] == ["table.npy"]
    finally:
        os.chmod(ro, 0o755)
    assert np.array_equal(mt.build_table(path=str(tmp_path / "missing" / "table.npy")), table)
    assert not (tmp_path / "missing").exists()


# ---- finish() and an interloper ------------------------------------------------------------------------------------------------------------------

def _pending(n):
    """A pending state as randn_cpu_stream leaves one behind, the device draw replaced by the layout model."""
    from oracle import mt_stream as ms
    state = torch.get_rng_state()
    words, left = mt.parse_state(state)
    _, cur, left_after = ms.randn(words, left, n)
    return mt._PendingState(state, np.asarray(cur, np.uint32), left_after, None)


def test_finish_installs_the_state_without_a_warning():
    torch.manual_seed(11)
    ref = torch.randn(1000)
    want = torch.get_rng_state()
    torch.manual_seed(11)
    p = _pending(1000)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        p.finish()
        p.finish()                                                   # (a second finish does nothing)
    assert torch.equal(torch.get_rng_state(), want) and ref.numel() == 1000


def test_finish_notices_a_draw_made_in_between():
    torch.manual_seed(11)
    torch.randn(1000)
    want = torch.get_rng_state()
    torch.manual_seed(11)
    p = _pending(1000)
    stolen = torch.rand(3)                                           # the interloper: a hook, another thread
    with pytest.warns(RuntimeWarning, match="will repeat"):
        p.finish()
    assert torch.equal(torch.get_rng_state(), want)                  # the device draw's state is installed all the same ...
    assert stolen.numel() == 3
