"""The autograd contract of every differentiable op, through both bindings: the layer between torch.autograd and the C ABI (the
autograd.Functions of _ctypes_ops.py, ops64.py, losses.py and functional.py, and their C++ twins in csrc/torch_ext). The table is
tests/autograd_contract_cases.py, the seven checks tests/autograd_contract_checks.py; tests/test_autograd_contract_cpu.py proves on toy
Functions that each check catches the defect it is there for.

  C1  subsets of leaves: a leaf that needs no gradient gets None (also from backward() itself), a requested gradient holds the op's
      existing bound against the float64 reference and against the all-leaves run; the plain forward (no leaf, or no_grad) returns the
      bits of the forward that saves
  C2  four backward passes over one graph: nothing a backward reads is consumed by the one before
  C3  two forwards, then the two backwards in the other order
  C4  upstream gradients with stride 0, as slices and transposes, of exact zeros, and for one output only
  C5  dtype / shape / device of every gradient; bfloat16 and float16 audio; controls as (bs,), (bs, 1), (bs, 1, 1), expanded, strided and
      float64; one leaf passed twice
  C6  every caller's tensor overwritten between forward and backward: autograd's in-place error, or the gradient of what the forward saw
  C7  forward on a side stream, backward started from the default stream

All inputs are finite and all shapes valid. Bounds are the ops' existing ones (cited per entry in the table); run against run is bit for
bit except where an existing test documents a sum whose order is not fixed (the table's docstring). Every comparison is recorded."""
import pytest
import torch

from dasp_pytorch_amd import config

from tests import autograd_contract_cases as T
from tests import autograd_contract_checks as K
from tests.util import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from dasp_pytorch_amd import _lib, _torch_ops
    assert _torch_ops.load(), "csrc/libdasp_torch.so missing or not loadable: __graft_entry__.build() builds it"
    return _lib.lib()


def configure(monkeypatch, spec):
    for k, v in dict({"torch_ops": True, "sos_segment": True, "sos_segment_tiles": None, "dyn_segment": True, "dyn_segment_tiles": None}, **spec.plan).items():
        monkeypatch.setattr(config.plan, k, v)


@pytest.mark.parametrize("check", sorted(K.CHECKS))
@pytest.mark.parametrize("name", [e.name for e in T.table()])
def test_contract(lib, monkeypatch, name, check):
    spec = T.by_name()[name]
    configure(monkeypatch, spec)
    rec = []
    try:
        find = K.CHECKS[check](spec, rec)
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU fault in {name} {check}: {e}", returncode=3)        # nothing more runs on a device that has faulted
        raise
    finally:
        worst = {}
        for what, key, e in rec:
            k = f"{what.split('[')[0]}:{key}"
            worst[k] = max(worst.get(k, 0.0), e)
        if worst:
            record(f"autograd_contract {check} {name}", **worst)
    torch.cuda.synchronize()
    assert lib.dasp_device_error() == 0
    assert not find, "\n".join([f"{name} ({spec.cite}):"] + find)


# (SosFiltFunction through lfilter_via_fsm with K = 2: sosfilt_via_fsm's own reshape(bs, -1, 0) is ambiguous for an empty signal and raises
# before any Function; the per-sample distortion's drive_db has one value per sample, so it is empty with x and no control is left)
EMPTY = ["gain[ctypes]", "lfilter_k2", "parametric_eq[ctypes]", "compressor[ctypes]", "compressor_matrix", "compressor_ctl[ctypes]",
         "stereo_bus", "stereo_mix_send", "oversampled_distortion_x4", "modulated_delay", "reverb_matrices[ctypes]", "lfilter_k11", "gain_f64",
         "parametric_eq_f64", "compressor_f64", "lfilter_k11_f64"]


@pytest.mark.parametrize("name", EMPTY)
def test_backward_of_an_empty_signal_returns_only_what_is_needed(lib, monkeypatch, name):
    """seq_len = 0: no kernel runs, the Python Functions answer from their recorded shapes. Also then: None for a leaf that needs no
    gradient, the leaf's own dtype and shape otherwise (float64 controls beside a float32 x included), zeros for the controls."""
    spec = T.by_name()[name]
    configure(monkeypatch, spec)

    def empty(t, f64=False):
        t["x"] = t["x"][..., :0].contiguous()
        for n in spec.controls if f64 else ():
            t[n] = t[n].double()
    for need in K.subsets(spec):
        for f64 in (False, True) if spec.f64_controls and "_f64" not in name else (False,):
            log = []
            with K.watched(spec, log):
                got = K.run(spec, 0, need=need, change=lambda t: empty(t, f64), node_log=log)
            assert not [m for k, m in log if k != "entered"], (name, need, f64, log)
            for n in spec.leaves:
                g, leaf = got["g_" + n], got["_t"][n]
                assert (g is None) == (n not in need), (name, need, n)
                if g is not None:
                    assert g.dtype == leaf.dtype and g.shape == leaf.shape and g.device == leaf.device and not g.any(), (name, need, n, f64)
    assert lib.dasp_device_error() == 0
