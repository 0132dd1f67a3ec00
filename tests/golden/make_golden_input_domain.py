"""Golden vectors for tests/test_gpu_input_domain.py / tests/test_input_domain_cpu.py, made by running the *reference itself*
(csteinmetz1/dasp-pytorch v0.0.1, imported from /root/reference) on the CPU, in the manner of make_golden_freqz.py. Run in the build
container only:

    python tests/golden/make_golden_input_domain.py

  biquad_rates_b6           signal.biquad at 16 / 22.05 / 32 / 48 / 88.2 / 96 kHz, all five filter types: coefficients (float32 and float64
                            runs) and the float64 gradients of a random linear functional of them (as biquad_types_b6 at 44.1 kHz);
                            cutoffs below 0.45 x the lowest rate, so every row is a valid design at every rate
  comp_sr48000_b2c1_n6000,  compressor at 48 and 96 kHz with attack <= 12 ms, so that the wrap term of the reference's circular smoothing
  comp_sr96000_b2c1_n6000   filter, alpha^(n_fft - N), is below 1e-8: x, params, w, y32, y64, gx64, gp64
  comp_silence_b2c2_n6000   compressor at 44.1 kHz on a cancelling stereo pair (item 0: R = -L, side chain exactly zero) and a zero tail
                            (item 1: exact zeros from sample 1500 on): pins the reference's conventions on silence - no gradient through
                            the clamp below eps, sign(0) = 0

Seeds are fixed and the archives are written with fixed member timestamps, so re-running the script reproduces the files bit for bit."""
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import dasp_pytorch  # noqa: E402
import dasp_pytorch.functional as RF  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = (16000, 22050, 32000, 48000, 88200, 96000)
BIQUAD_TYPES = ["peaking", "low_shelf", "high_shelf", "low_pass", "high_pass"]


def save(name, **arrays):
    """np.savez with a fixed timestamp on every member (np.savez stamps the current time)."""
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(arrays[key]), allow_pickle=False)
    print(name, f"{len(arrays)} arrays", f"{os.path.getsize(path) / 1024:.0f} KiB")


def f32(t):
    return t.detach().to(torch.float32).numpy()


def biquad_rates(name, B, seed):
    g = torch.Generator().manual_seed(seed)
    gain = torch.rand(B, 1, generator=g) * 40 - 20
    fc = 20 + torch.rand(B, 1, generator=g) ** 2 * (0.45 * min(RATES) - 20)
    fc[0, 0] = 20.0                                           # the module's lowest cutoff with its highest Q: the pole nearest z = 1
    q = 0.1 + torch.rand(B, 1, generator=g) * 5.9
    q[0, 0] = 6.0
    wb, wa = torch.randn(B, 3, generator=g), torch.randn(B, 3, generator=g)
    out = dict(gain_db=f32(gain), cutoff_freq=f32(fc), q_factor=f32(q), wb=f32(wb), wa=f32(wa), rates=np.asarray(RATES, np.int64))
    for sr in RATES:
        for t in BIQUAD_TYPES:
            for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                ins = [v.to(torch.float32).to(dt).clone().requires_grad_(True) for v in (gain, fc, q)]
                b, a = dasp_pytorch.signal.biquad(*ins, sr, t)
                ((b * wb.to(dt)).sum() + (a * wa.to(dt)).sum()).backward()
                # the float64 coefficients are kept as float64: at 96 kHz and 20 Hz, 1 - a2 is 1e-4 and float32 storage would cost 6e-4 of it
                keep = (lambda v: v.detach().numpy().astype(np.float64)) if tag == "64" else f32
                out[f"sr{sr}_{t}_b{tag}"], out[f"sr{sr}_{t}_a{tag}"] = keep(b), keep(a)
                if tag == "64":     # (B, 3): d/d gain_db, cutoff_freq, q_factor; low_pass / high_pass do not depend on gain_db: stored as 0
                    out[f"sr{sr}_{t}_g64"] = torch.cat([v.grad if v.grad is not None else torch.zeros_like(v) for v in ins], 1).numpy()
    save(name, **out)


COMP_KEYS = ["threshold_db", "ratio", "attack_ms", "release_ms", "knee_db", "makeup_gain_db"]


def run_comp(x, params, w, sr):
    out = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        xx = x.to(dt).clone().requires_grad_(True)
        cols = [params[:, i].to(dt).clone().requires_grad_(True) for i in range(6)]
        y = RF.compressor(xx, sr, *cols)
        (y * w.to(dt)).sum().backward()
        gp = torch.stack([c.grad if c.grad is not None else torch.zeros_like(c) for c in cols], 1)
        out["y" + tag] = f32(y)
        if tag == "64":
            out["gx64"], out["gp64"] = f32(xx.grad), f32(gp)
    return out


def speechlike(g, B, C, N):
    x = torch.rand(B, C, N, generator=g) * 2 - 1
    env_db = torch.nn.functional.interpolate(torch.rand(B, 1, N // 500 + 2, generator=g) * 60 - 60, size=N, mode="linear")
    return x * 10 ** (env_db / 20)


def comp_params(g, B, sr, attack_hi):
    pn = torch.rand(B, 6, generator=g)
    pn[:, 4] = pn[:, 4].clamp_min(1e-3 / 12)
    mod = dasp_pytorch.Compressor(sr)
    d = mod.denormalize_param_dict(mod.extract_param_dict(pn))
    p = torch.stack([d[k] for k in COMP_KEYS], 1)
    p[:, 2] = 5.0 + (attack_hi - 5.0) * pn[:, 2]
    return p.to(torch.float32)


def comp_rate_case(name, sr, seed):
    B, C, N = 2, 1, 6000
    g = torch.Generator().manual_seed(seed)
    x = speechlike(g, B, C, N).to(torch.float32)
    p = comp_params(g, B, sr, 12.0)
    p[0, 2] = 12.0
    w = torch.randn(B, C, N, generator=g)
    save(name, x=f32(x), params=f32(p), w=f32(w), sample_rate=np.int64(sr), **run_comp(x, p, w, sr))


def comp_silence_case(name, seed):
    sr, B, C, N = 44100, 2, 2, 6000
    g = torch.Generator().manual_seed(seed)
    x = speechlike(g, B, C, N).to(torch.float32)
    x[0, 1] = -x[0, 0]
    x[1, :, 1500:] = 0
    p = comp_params(g, B, sr, 12.0)
    w = torch.randn(B, C, N, generator=g)
    save(name, x=f32(x), params=f32(p), w=f32(w), sample_rate=np.int64(sr), **run_comp(x, p, w, sr))


def main():
    torch.set_num_threads(1)
    biquad_rates("biquad_rates_b6", 6, 201)
    comp_rate_case("comp_sr48000_b2c1_n6000", 48000, 202)
    comp_rate_case("comp_sr96000_b2c1_n6000", 96000, 203)
    comp_silence_case("comp_silence_b2c2_n6000", 204)


if __name__ == "__main__":
    main()
