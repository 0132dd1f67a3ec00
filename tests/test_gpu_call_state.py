"""What a call leaves behind in the process that made it: arguments, random-number state, ambient settings, memory, caches, error words
and host threads - over the table of the autograd-contract battery (tests/autograd_contract_cases.py: every Function and every
torch.ops.dasp op at the smallest shape per launch shape) plus the entries that table cannot hold (tests/call_state_cases.py). The checks
are tests/call_state_checks.py; tests/test_call_state_cpu.py proves on toy Functions that S1 - S4 catch the defect they are there for.

  S1  arguments and upstream gradients keep their bits and versions (also as offset views and row slices of NaN-filled allocations)
  S2  the CPU generator, every device generator, numpy's and random's: untouched, or where the ONE documented draw leaves the CPU
      generator; the first default-noise reverb of a process in a child process of its own
  S3  device, stream, default dtype, grad mode, autocast and config.plan: untouched, also by a refused call
  S4  no byte more after a step than after warm-up, with the garbage collector off; nothing for a collection to find
  S5  33 streams / nine keys cross the limit of every Python cache
  S6  hipPeekAtLastError() == 0 and dasp_device_error() == 0
  S7  four host threads per config.plan

All inputs are finite and all shapes valid. Bounds are the ops' existing ones; run against run is bit for bit unless the table documents
otherwise. Every measured figure is recorded."""
import subprocess
import sys
import os

import pytest
import torch

from dasp_pytorch_amd import config

from tests import call_state_cases as C
from tests import call_state_checks as S
from tests.util import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_PLAN = {"torch_ops": True, "sos_segment": True, "sos_segment_tiles": None, "dyn_segment": True, "dyn_segment_tiles": None}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from dasp_pytorch_amd import _lib, _torch_ops
    assert _torch_ops.load(), "csrc/libdasp_torch.so missing or not loadable: __graft_entry__.build() builds it"
    return _lib.lib()


def configure(monkeypatch, spec):
    for k, v in dict(DEFAULT_PLAN, **spec.plan).items():
        monkeypatch.setattr(config.plan, k, v)


def guarded(name, rec, fn):
    """fn() -> findings; a GPU fault ends the session (nothing more runs on a device that has faulted); the figures are recorded."""
    try:
        return fn()
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in {name}: {e}", returncode=3)
        raise
    finally:
        worst = {}
        for what, key, e in rec:
            k = f"{what.split('[')[0]}:{key}"
            worst[k] = max(worst.get(k, 0.0), e)
        if worst:
            record(f"call_state {name}", **worst)


@pytest.mark.parametrize("check", sorted(S.CHECKS))
@pytest.mark.parametrize("name", [e.name for e in C.entries()])
def test_call_state(lib, monkeypatch, name, check):
    if name in C.EXEMPT.get(check, {}):
        return                                    # left out by name: the reason is in tests/call_state_cases.py (EXEMPT)
    spec = C.by_name()[name]
    configure(monkeypatch, spec)
    rec = []
    kw = {"refusal": C.REFUSALS.get(name)} if check == "S3_ambient" else {}
    find = guarded(f"{check} {name}", rec, lambda: S.CHECKS[check](spec, rec, **kw))
    torch.cuda.synchronize()
    assert lib.dasp_device_error() == 0
    assert not find, "\n".join([f"{name} ({spec.cite}):"] + find)


def test_exemptions_are_few_and_named():
    names = {e.name for e in C.entries()}
    for check, out in C.EXEMPT.items():
        assert check in S.CHECKS and set(out) <= names and len(out) <= 5 and all(out.values()), (check, out)
    assert set(C.REFUSALS) <= names


@pytest.mark.parametrize("name", [e.name for e in C.extras()])
def test_the_added_entries_compute_what_they_document(lib, monkeypatch, name):
    """The entries beside the table are held to a reference too: the float64 reference with the noise the documented draw hands out from
    the CPU generator's state at the call, at the reverb's / the random stream's existing bounds; and, from the same generator state, a
    second run returns what the first did by the entry's `same` rule (the written-out noise stream: that alone)."""
    spec = C.by_name()[name]
    configure(monkeypatch, spec)
    rec = []

    def run():
        torch.manual_seed(1234)                  # the noise these entries draw, and with it their error, is the same in every session
        state = torch.get_rng_state()
        first = S.step(spec, 0)
        after = torch.get_rng_state()
        ref = S.reference_of(spec, 0, first.get("_gys") or [], state)
        torch.set_rng_state(state)
        second = S.step(spec, 0, gys=first.get("_gys"))
        assert torch.equal(torch.get_rng_state(), after)
        return S.held(spec, "extras", second, first, ref, rec, "")
    find = guarded(f"extras {name}", rec, run)
    assert lib.dasp_device_error() == 0
    assert not find, "\n".join([f"{name} ({spec.cite}):"] + find)


# ---- S2: the first default-noise reverb of a process ------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
import dasp_pytorch_amd as D
from tests import call_state_cases as C
spec = C.by_name()["reverb_default_noise[ctypes]"]
t = spec.make(0)
cols = [t[k][:, i] for k in ("gains", "decays") for i in range(12)]
for run in ("default", "explicit"):
    torch.manual_seed(1234)
    s0, seed0 = [s.clone() for s in torch.cuda.get_rng_state_all()], torch.cuda.initial_seed()
    kw = {} if run == "default" else {"noise": torch.randn(4, 12, C.ROW).to(C.DEV)}
    D.noise_shaped_reverberation(t["x"], C.SR, *cols, t["mix"], num_samples=C.L, num_bandpass_taps=C.TAPS, **kw)
    torch.cuda.synchronize()
    s1, seed1 = torch.cuda.get_rng_state_all(), torch.cuda.initial_seed()
    same = len(s0) == len(s1) and all(torch.equal(a, b) for a, b in zip(s0, s1))
    print("RUN", run, "device_state_kept", same, "seed_before", seed0, "seed_after", seed1, "rand", torch.rand(4, device="cuda").tolist(),
          "cpu_next", torch.rand(2).tolist())
"""


def test_first_default_noise_call_of_a_process_leaves_the_device_generators_alone(lib):
    """The once-per-process self-check of the random-stream reproduction runs inside the first default-noise reverb: in a fresh child
    process (the parent has long made that call), seeded with torch.manual_seed(1234), the device generators' states and seed are the
    same before and after, and torch.rand(4, device="cuda") afterwards - and the CPU generator's next values - are those of the same run
    with noise= passed explicitly (drawn by the caller with torch.randn, as the reference draws it)."""
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    runs = {ln.split()[1]: ln.split(None, 2)[2] for ln in out.stdout.splitlines() if ln.startswith("RUN ")}
    print(out.stdout)
    assert set(runs) == {"default", "explicit"}, out.stdout
    assert "device_state_kept True seed_before 1234 seed_after 1234" in runs["explicit"], runs["explicit"]
    assert runs["default"] == runs["explicit"], f"first default-noise call:\n  {runs['default']}\nwith noise= passed:\n  {runs['explicit']}"


# ---- S5: cache eviction ---------------------------------------------------------------------------------------------------------------------------

FAMILIES = ["counters[ctypes]", "counters[torch_ops]", "mrstft_linear", "mrstft_mel", "mrstft_aw", "filter_spectrum", "filterbank", "fdfir_twiddles", "affine"]


@pytest.mark.parametrize("family", FAMILIES)
def test_cache_eviction(lib, monkeypatch, family):
    specs, caches, mode = C.families()[family]
    configure(monkeypatch, specs[0])
    rec = []
    find = guarded(f"S5_eviction {family}", rec, lambda: S.check_eviction(specs, caches, mode, rec))
    torch.cuda.synchronize()
    assert lib.dasp_device_error() == 0
    assert not find, "\n".join([f"{family}:"] + find[:40])


def test_the_families_are_the_ones_listed():
    assert sorted(C.families()) == sorted(FAMILIES)


# ---- S7: host threads ---------------------------------------------------------------------------------------------------------------------------

def plan_of(spec):
    return tuple(sorted(dict(DEFAULT_PLAN, **spec.plan).items(), key=lambda kv: kv[0]))


def plan_groups():
    groups = {}
    for e in C.T.table():
        groups.setdefault(plan_of(e), []).append(e)
    return groups


def group_id(plan):
    return ",".join(f"{k}={v}" for k, v in plan if DEFAULT_PLAN[k] != v) or "default"


@pytest.mark.parametrize("plan", sorted(plan_groups(), key=str), ids=group_id)
def test_host_threads(lib, monkeypatch, plan):
    specs = plan_groups()[plan]
    configure(monkeypatch, specs[0])
    for e in specs:
        e.global_generator = e.name.startswith("reverb_cpu_generator")        # its call() seeds and draws from the process-global generator
    rec = []
    find = guarded(f"S7_threads {group_id(plan)}", rec, lambda: S.check_threads(specs, rec))
    torch.cuda.synchronize()
    assert lib.dasp_device_error() == 0
    assert not find, "\n".join([f"{group_id(plan)} ({len(specs)} entries):"] + find[:40])


def test_every_entry_is_in_a_thread_group():
    assert sum(len(g) for g in plan_groups().values()) == len(C.T.table())
