"""Golden vectors of the reference's fft_freqz / fft_sosfreqz (dasp_pytorch/signal.py:7-32), made by running the *reference itself*
(csteinmetz1/dasp-pytorch v0.0.1, imported from /root/reference) on the CPU, in the manner of make_golden.py. Run in the build
container only:

    python tests/golden/make_golden_freqz.py

Every file holds the coefficients as float32; the reference's float32 response H32; its float64 response H64 computed on those float32
coefficients cast to float64; a random complex cotangent W (complex64); and the reference's float64 gradients of sum(Re(conj(W) H)) w.r.t.
the coefficients (W cast to complex128). Seeds are fixed and the archives are written with fixed member timestamps, so re-running the
script reproduces the files bit for bit.
"""
import math
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import dasp_pytorch  # noqa: E402
import dasp_pytorch.signal as RS  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 44100


def save(name, **arrays):
    """np.savez with a fixed timestamp on every member (np.savez stamps the current time)."""
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(arrays[key]), allow_pickle=False)
    print(name, {k: (v.shape, v.dtype.name) for k, v in arrays.items()}, f"{os.path.getsize(path) / 1024:.0f} KiB")


def cotangent(g, shape):
    return (torch.randn(shape, generator=g, dtype=torch.float64) + 1j * torch.randn(shape, generator=g, dtype=torch.float64)).to(torch.complex64)


def run(fn, coefs32, W, n_arg):
    """-> H32, H64, gradients (float64) of sum(Re(conj(W) H64)) for every coefficient tensor."""
    H32 = fn(*[torch.from_numpy(c) for c in coefs32], n_arg)
    c64 = [torch.from_numpy(c).to(torch.float64).requires_grad_(True) for c in coefs32]
    H64 = fn(*c64, n_arg)
    (torch.conj(W.to(torch.complex128)) * H64).real.sum().backward()
    return H32.detach().numpy(), H64.detach().numpy(), [c.grad.numpy() for c in c64]


def sos_file(name, sos32, n_fft, seed, n_arg=None):
    g = torch.Generator().manual_seed(seed)
    n = int(n_fft)
    W = cotangent(g, (sos32.shape[0], n // 2 + 1))
    if n_arg is None:                                       # the reference's default n_fft (512)
        H32, H64, (gs,) = run(lambda s, _: RS.fft_sosfreqz(s), [sos32], W, None)
    else:
        H32, H64, (gs,) = run(RS.fft_sosfreqz, [sos32], W, n_arg)
    save(name, sos=sos32, n_fft=np.int64(n), H32=H32, H64=H64, W=W.numpy(), gsos64=gs)


def ba_file(name, b32, a32, n_fft, seed):
    g = torch.Generator().manual_seed(seed)
    lead = np.broadcast_shapes(b32.shape[:-1], a32.shape[:-1])
    W = cotangent(g, tuple(lead) + (n_fft // 2 + 1,))
    H32, H64, (gb, ga) = run(RS.fft_freqz, [b32, a32], W, n_fft)
    save(name, b=b32, a=a32, n_fft=np.int64(n_fft), H32=H32, H64=H64, W=W.numpy(), gb64=gb, ga64=ga)


def eq_sos(params):
    """(bs, 18) physical EQ parameters -> (bs, 6, 6) float32 sections from the reference's own signal.biquad (float32 design)."""
    kinds = ("low_shelf", "peaking", "peaking", "peaking", "peaking", "high_shelf")
    p = torch.from_numpy(params.astype(np.float32))
    rows = []
    for i, kind in enumerate(kinds):
        b, a = RS.biquad(p[:, 3 * i], p[:, 3 * i + 1], p[:, 3 * i + 2], SR, kind)
        rows.append(torch.cat([b, a], -1))
    return torch.stack(rows, 1).numpy().astype(np.float32)


def eq_params(seed, n_random):
    mod = dasp_pytorch.ParametricEQ(SR)
    ranges = list(mod.param_ranges.values())
    lo = np.array([r[0] for r in ranges], np.float64)
    hi = np.array([r[1] for r in ranges], np.float64)
    rng = np.random.default_rng(seed)
    rows = [lo + rng.random(18) * (hi - lo) for _ in range(n_random)]
    top = hi[13]                                            # band3 / high shelf cutoff range ends 1 kHz below Nyquist
    # the corners: 20 Hz low shelf at Q 0.1 and at Q 6, +-20 dB, band3 and the high shelf at the top of their range
    c = lo + 0.5 * (hi - lo)
    for gain, q in ((20.0, 0.1), (-20.0, 6.0), (20.0, 6.0), (-20.0, 0.1)):
        r = c.copy()
        r[0:3] = (gain, 20.0, q)
        r[12:15] = (-gain, top, q)
        r[15:18] = (gain, top, 6.0 if q == 0.1 else 0.1)
        rows.append(r)
    return np.stack(rows)


def lphp_sos(seed, bs):
    """Three sections: RBJ low pass, high pass (exact zeros of B at Nyquist / DC) and a peaking band, from the reference's biquad."""
    rng = np.random.default_rng(seed)
    f = lambda lo, hi: torch.from_numpy(rng.uniform(lo, hi, bs).astype(np.float32))
    rows = []
    for kind, fc in (("low_pass", (2000, 20000)), ("high_pass", (20, 500)), ("peaking", (100, 10000))):
        b, a = RS.biquad(f(-12, 12), f(*fc), f(0.3, 4.0), SR, kind)
        rows.append(torch.cat([b, a], -1))
    return torch.stack(rows, 1).numpy().astype(np.float32)


def stable_poly(rng, rows, K):
    """Denominators of K taps with every root inside |z| < 0.95 and an unnormalised leading coefficient a0 in [0.5, 2]."""
    out = []
    for _ in range(rows):
        roots = []
        while len(roots) < K - 1:
            if K - 1 - len(roots) >= 2 and rng.random() < 0.7:
                r, th = rng.uniform(0.3, 0.95), rng.uniform(0, math.pi)
                roots += [r * np.exp(1j * th), r * np.exp(-1j * th)]
            else:
                roots.append(rng.uniform(-0.95, 0.95))
        poly = np.real(np.poly(roots)) if roots else np.ones(1)
        out.append(poly * rng.uniform(0.5, 2.0))
    return np.stack(out).astype(np.float32)


def main():
    torch.set_num_threads(1)
    eq = eq_sos(eq_params(7, 4))                             # 4 random + 4 corner rows
    sos_file("freqz_sos_eq_n512", eq, 512, 1)                # the default n_fft
    sos_file("freqz_sos_eq_n999", eq, 999, 2, 999)           # odd
    sos_file("freqz_sos_eq_n16384", eq[4:6], 16384, 3, 16384)
    lp = lphp_sos(11, 4)
    sos_file("freqz_sos_lphp_n1024", lp, 1024, 4, torch.tensor(1024))   # n_fft as a 0-dim tensor, as sosfilt_via_fsm passes it
    rng = np.random.default_rng(5)
    ba_file("freqz_ba_k2", rng.standard_normal((4, 2)).astype(np.float32), stable_poly(rng, 4, 2), 512, 6)
    ba_file("freqz_ba_k3_bcast", rng.standard_normal((3, 1, 3)).astype(np.float32), stable_poly(rng, 2, 3), 777, 7)   # (3, 1) x (2,)
    ba_file("freqz_ba_k5", rng.standard_normal((4, 5)).astype(np.float32), stable_poly(rng, 4, 5), 64, 8)
    ba_file("freqz_ba_k5_crop", rng.standard_normal((2, 5)).astype(np.float32), stable_poly(rng, 2, 5), 3, 9)        # n_fft < K


if __name__ == "__main__":
    main()
