"""Expected values for the stereo_mix tests: the existing oracle functions composed in float64, exactly as the reference composes its own
stereo_bus(stereo_panner(.)) - no restated definition. The effects send is the same bus at gain_db + send_db (the sum taken in float64)."""
import numpy as np

from oracle import dasp_oracle as orc

SR = 44100


def compose(x, gain_db, pan, send_db=None, w0=None, w1=None):
    """mix, send (None without send_db) and, when w0 is given, the gradients of <mix, w0> + <send, w1> w.r.t. x, gain_db, pan, send_db
    by chaining the oracle's VJPs: dict of float64 arrays, the control gradients flat."""
    B, T, N = x.shape
    g = np.asarray(gain_db, np.float64).reshape(B, T)
    panned = orc.stereo_panner(x, SR, pan)                                    # (B, 2, T, N)
    out = {"mix": orc.stereo_bus(panned, SR, g), "send": None}
    if send_db is not None:
        gs = g + np.asarray(send_db, np.float64).reshape(B, T)
        out["send"] = orc.stereo_bus(panned, SR, gs)
    if w0 is None:
        return out
    gpanned, ggain = orc.stereo_bus_vjp(panned, SR, g, w0)
    if send_db is not None:
        gp2, gsum = orc.stereo_bus_vjp(panned, SR, gs, w1)                    # d/d(gain_db + send_db): flows to both controls
        gpanned = gpanned + gp2
        ggain = ggain + gsum
        out["gsend"] = gsum.reshape(-1)
    gx, gpan = orc.stereo_panner_vjp(x, SR, np.asarray(pan).reshape(B, T), gpanned)
    out.update(gx=gx, ggain=ggain.reshape(-1), gpan=gpan.reshape(-1))
    return out


def draw(B, T, N):
    """Inputs as tests/test_gpu_stereo.py::test_stereo_shapes_vs_oracle draws them."""
    rng = np.random.default_rng(7 * B + T + N)
    x = (rng.random((B, T, N)) * 2 - 1).astype(np.float32)
    pan = (rng.random((B, T)) * 0.9 + 0.05).astype(np.float32)
    gain_db = (rng.random((B, T, 1)) * 36 - 24).astype(np.float32)
    send_db = (rng.random((B, T, 1)) * 36 - 24).astype(np.float32)
    w0 = rng.standard_normal((B, 2, N)).astype(np.float32)
    w1 = rng.standard_normal((B, 2, N)).astype(np.float32)
    return x, gain_db, pan, send_db, w0, w1
