"""stereo_mix without a device: the public interface, the golden file against the oracle composition that the GPU tests use as their
reference, the host-side size queries of the C ABI and the argument checks that come before any launch."""
import inspect

import numpy as np
import pytest
import torch

from dasp_pytorch_amd import _lib
from tests.stereo_mix_ref import compose
from tests.util import load_golden

GOLDEN = "stereo_mix_b2t3_n1501"


def test_api_presence():
    import dasp_pytorch_amd as D
    assert D.stereo_mix is D.functional.stereo_mix
    sig = inspect.signature(D.stereo_mix)
    assert list(sig.parameters) == ["x", "sample_rate", "gain_db", "pan", "send_db"]
    assert sig.parameters["send_db"].default is None
    assert all(p.default is inspect.Parameter.empty for n, p in sig.parameters.items() if n != "send_db")
    from dasp_pytorch_amd import ops
    assert issubclass(ops.StereoMixFunction, torch.autograd.Function)


def test_golden_matches_oracle_composition():
    """The oracle's stereo_bus(stereo_panner(.)) and its chained VJPs reproduce the reference's float64 run to 1e-12 relative, the send
    bus as the same composition at gain_db + send_db; the second run (no send) likewise."""
    g = load_golden(GOLDEN)
    assert g["x"].shape == (2, 3, 1501) and g["mix64"].dtype == np.float64
    assert 0.05 <= g["pan"].min() and g["pan"].max() <= 0.95
    for c in (g["gain_db"], g["send_db"]):
        assert -24 <= c.min() and c.max() <= 12

    def close(a, b):
        assert a.shape == b.shape
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()

    o = compose(g["x"], g["gain_db"], g["pan"], g["send_db"], g["w0"], g["w1"])
    for key in ("mix", "send", "gx"):
        close(o[key], g[key + "64"])
    for key in ("ggain", "gpan", "gsend"):
        close(o[key], g[key + "64"].reshape(-1))
    o = compose(g["x"], g["gain_db"], g["pan"], None, g["w0"])
    close(o["mix"], g["mix64"])
    close(o["gx"], g["ns_gx64"])
    close(o["ggain"], g["ns_ggain64"].reshape(-1))
    close(o["gpan"], g["ns_gpan64"].reshape(-1))
    assert o["send"] is None
    # the float32 run is the same computation: it agrees with the float64 one to float32 accuracy
    assert np.abs(g["mix32"] - g["mix64"]).max() <= 1e-5 * np.abs(g["mix64"]).max()


def _rule(B, N):
    """The stated rule: 4096 samples per workgroup, halved down to 1024 while B * segments is below two workgroups per CU (512)."""
    seg = 4096
    while seg > 1024 and B * -(-N // seg) < 512:
        seg //= 2
    return seg


def test_size_queries():
    L = _lib.lib()
    assert L.dasp_stereo_mix_max_tracks() >= 256
    assert L.dasp_stereo_mix_segment(1, 131072) == 1024
    assert L.dasp_stereo_mix_segment(16, 131072) == 4096
    assert L.dasp_stereo_mix_segment(256, 131072) == 4096
    for B in (1, 2, 3, 7, 16, 40, 64, 100, 256, 1000):
        for N in (1, 1000, 4096, 4097, 24581, 131072, 262144, 1 << 22):
            seg = L.dasp_stereo_mix_segment(B, N)
            assert seg == _rule(B, N) and 1024 <= seg <= 4096 and seg % 1024 == 0
            nseg = -(-N // seg)
            for T in (1, 8, 256):
                assert L.dasp_stereo_mix_partial_floats(B, T, N, 0) == B * nseg * T * 2
                assert L.dasp_stereo_mix_partial_floats(B, T, N, 1) == B * nseg * T * 4
    assert L.dasp_stereo_mix_segment(1, 131072) != L.dasp_stereo_mix_segment(40, 24581) != L.dasp_stereo_mix_segment(1, 24581)


def test_argument_errors_without_gpu():
    """Refusals come before any launch; the pointers are never dereferenced on the host (8 stands for a non-null address)."""
    L = _lib.lib()
    P, ARG, UNSUPPORTED = 8, -1, -2
    tmax = L.dasp_stereo_mix_max_tracks()
    fwd, bwd = L.dasp_stereo_mix_forward, L.dasp_stereo_mix_backward
    assert fwd(None, P, P, None, P, None, 1, 2, 64, None) == ARG
    assert fwd(P, None, P, None, P, None, 1, 2, 64, None) == ARG
    assert fwd(P, P, None, None, P, None, 1, 2, 64, None) == ARG
    assert fwd(P, P, P, None, None, None, 1, 2, 64, None) == ARG
    assert fwd(P, P, P, None, P, None, 1, 0, 64, None) == ARG                 # T = 0
    assert fwd(P, P, P, None, P, None, 0, 2, 64, None) == ARG and fwd(P, P, P, None, P, None, 1, 2, 0, None) == ARG
    assert fwd(P, P, P, None, P, P, 1, 2, 64, None) == ARG                    # send without send_db
    assert fwd(P, P, P, P, P, None, 1, 2, 64, None) == ARG                    # send_db without send
    assert fwd(P, P, P, None, P, None, 1, tmax + 1, 64, None) == UNSUPPORTED
    assert fwd(P, P, P, P, P, P, 1, tmax + 1, 64, None) == UNSUPPORTED
    assert fwd(P, P, P, None, P, None, 1, 2, 1 << 44, None) == UNSUPPORTED    # more than 2^31 - 1 workgroups
    assert bwd(None, P, P, None, P, None, P, P, P, None, P, 1, 2, 64, None) == ARG
    assert bwd(P, P, P, None, None, None, P, P, P, None, P, 1, 2, 64, None) == ARG       # gmix
    assert bwd(P, P, P, None, P, None, P, None, P, None, P, 1, 2, 64, None) == ARG       # ggain
    assert bwd(P, P, P, None, P, None, P, P, None, None, P, 1, 2, 64, None) == ARG       # gpan
    assert bwd(P, P, P, None, P, None, P, P, P, None, None, 1, 2, 64, None) == ARG       # partials
    assert bwd(P, P, P, None, P, None, P, P, P, None, P, 1, 0, 64, None) == ARG          # T = 0
    assert bwd(P, P, P, None, P, P, P, P, P, None, P, 1, 2, 64, None) == ARG             # gsend without send_db
    assert bwd(P, P, P, P, P, P, P, P, P, None, P, 1, 2, 64, None) == ARG                # send_db without gsend_db
    assert bwd(P, P, P, None, P, None, None, P, P, None, P, 1, tmax + 1, 64, None) == UNSUPPORTED   # (gx may be null)
    assert bwd(P, P, P, None, P, None, P, P, P, None, P, 1, 2, 1 << 44, None) == UNSUPPORTED


def test_python_layer_refusals():
    import dasp_pytorch_amd as D
    x = torch.zeros(2, 3, 64)
    ok = torch.zeros(2, 3)
    # a control with the wrong number of values: RuntimeError before the device is looked at (these are CPU tensors)
    for kw in (dict(gain_db=torch.zeros(2, 2), pan=ok), dict(gain_db=ok, pan=torch.zeros(7)), dict(gain_db=ok, pan=ok, send_db=torch.zeros(2, 3, 2))):
        with pytest.raises(RuntimeError, match="invalid for input of size") as e:
            D.stereo_mix(x, 44100, **kw)
        assert not isinstance(e.value, _lib.DaspHipError)
    with pytest.raises(ValueError):                                           # wrong rank of x: the siblings' unpacking error
        D.stereo_mix(torch.zeros(2, 64), 44100, ok, ok)
    with pytest.raises(ValueError):
        D.stereo_panner(torch.zeros(2, 64), 44100, ok)
    # CPU tensors are refused as the siblings refuse them: no CPU path
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.stereo_mix(x, 44100, ok, ok)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.stereo_mix(x, 44100, ok, ok, ok)
    with pytest.raises(_lib.DaspHipError, match="no CPU path"):
        D.stereo_panner(x, 44100, ok)
    with pytest.raises(_lib.DaspHipError, match="float64"):
        D.stereo_mix(x.double(), 44100, ok, ok)
