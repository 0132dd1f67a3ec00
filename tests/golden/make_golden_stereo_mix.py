"""Golden vectors for stereo_mix, made by running the *reference itself* (csteinmetz1/dasp-pytorch v0.0.1, imported from /root/reference)
on the CPU, in the manner of make_golden.py: the composition stereo_bus(stereo_panner(x, sr, pan), sr, gain_db) that stereo_mix fuses,
and the effects send as stereo_bus(stereo_panner(x, sr, pan), sr, gain_db + send_db). Run in the build container only:

    python tests/golden/make_golden_stereo_mix.py

tests/golden/stereo_mix_b2t3_n1501.npz (deflated) holds
  x (2, 3, 1501), gain_db, pan, send_db (2, 3), w0, w1 (2, 2, 1501)               float32 inputs and loss weights
  mix64, send64, gx64, ggain64, gpan64, gsend64                                      the reference's float64 run on those inputs: outputs and
                                                                                     the gradients of <mix, w0> + <send, w1>, kept as float64
  mix32, send32, gx32, ggain32, gpan32, gsend32                                      the same from its float32 run
  ns_gx64, ns_ggain64, ns_gpan64 and ns_gx32, ns_ggain32, ns_gpan32                  a second run without the send: gradients of <mix, w0>
                                                                                     (its mix is mix64 / mix32)
Seeds are fixed and the archive is written with fixed member timestamps, so re-running the script reproduces the file bit for bit.
"""
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import dasp_pytorch.functional as RF  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 44100


def save(name, **arrays):
    """np.savez with a fixed timestamp on every member (np.savez stamps the current time)."""
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(arrays[key]), allow_pickle=False)
    print(name, {k: (v.shape, v.dtype.name) for k, v in arrays.items()}, f"{os.path.getsize(path) / 1024:.0f} KiB")


def run(x, gain_db, pan, send_db, w0, w1, dt, with_send):
    x, gain_db, pan, send_db = (t.to(dt).clone().requires_grad_(True) for t in (x, gain_db, pan, send_db))
    panned = RF.stereo_panner(x, SR, pan)
    mix = RF.stereo_bus(panned, SR, gain_db)
    loss = (mix * w0.to(dt)).sum()
    send = None
    if with_send:
        send = RF.stereo_bus(panned, SR, gain_db + send_db)
        loss = loss + (send * w1.to(dt)).sum()
    loss.backward()
    return mix, send, x.grad, gain_db.grad, pan.grad, send_db.grad


def case(name, B, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, T, N, generator=g) * 2 - 1
    pan = torch.rand(B, T, generator=g) * 0.9 + 0.05           # away from 0 / 1, where the reference's sqrt has an infinite slope
    gain_db = torch.rand(B, T, generator=g) * 36 - 24
    send_db = torch.rand(B, T, generator=g) * 36 - 24
    # loss weights on a grid of 1/8 in [-2, 2]: as good a cotangent as any, and they deflate well
    w0 = torch.randint(-16, 17, (B, 2, N), generator=g).to(torch.float32) / 8.0
    w1 = torch.randint(-16, 17, (B, 2, N), generator=g).to(torch.float32) / 8.0
    out = dict(x=x.numpy(), gain_db=gain_db.numpy(), pan=pan.numpy(), send_db=send_db.numpy(), w0=w0.numpy(), w1=w1.numpy())
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        keep = lambda t: t.detach().numpy()                      # float64 results stay float64: the CPU test pins the oracle to 1e-12
        mix, send, gx, gg, gp, gs = run(x, gain_db, pan, send_db, w0, w1, dt, True)
        for key, v in (("mix", mix), ("send", send), ("gx", gx), ("ggain", gg), ("gpan", gp), ("gsend", gs)):
            out[key + tag] = keep(v)
        mix_ns, _, gx, gg, gp, gs = run(x, gain_db, pan, send_db, w0, w1, dt, False)
        assert torch.equal(mix_ns, mix) and gs is None
        for key, v in (("ns_gx", gx), ("ns_ggain", gg), ("ns_gpan", gp)):
            out[key + tag] = keep(v)
    save(name, **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    case("stereo_mix_b2t3_n1501", 2, 3, 1501, seed=140)
