"""Forward + backward of the MR-STFT loss with auraloss's options (dasp_pytorch_amd.losses, csrc/stftloss.hip) against the same loss
written as torch.stft + conv1d on the GPU, timed with device events after warm-up. One JSON line per workload:
  auto_eq         the loss of examples/auto_eq.py:252-262 (seven resolutions 128 .. 8192, hop n_fft / 2, w_sc = 0, log + linear
                  magnitude, A-weighting at 44.1 kHz) at (16,1,131072) and (16,2,131072)
  virtual_analog  the same arguments (examples/virtual_analog.py:288-298) at (32,1,32768)
  default         auraloss's default loss at (16,2,131072) (no torch leg; `--only default` for same-box A/B runs, `--root DIR` imports
                  dasp_pytorch_amd from another checkout)
The target does not require a gradient (as in the examples). Also printed: the relative difference of the two losses' values."""
import argparse
import json
import os
import sys

import numpy as np

EXAMPLE_RES = tuple((1 << k, 1 << (k - 1), 1 << k) for k in range(7, 14))
DEFAULT_RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def torch_loss(res, w_sc, w_log, w_lin, taps, device, eps=1e-8):
    import torch
    import torch.nn.functional as F
    wins = {w: torch.hann_window(w, device=device) for _, _, w in res}
    h = None if taps is None else torch.tensor(np.array(taps), device=device).view(1, 1, -1)

    def fn(p, t):
        N = p.shape[-1]
        p, t = p.reshape(-1, N), t.reshape(-1, N)
        if h is not None:
            p = F.conv1d(p.unsqueeze(1), h, padding=h.shape[-1] // 2).squeeze(1)
            t = F.conv1d(t.unsqueeze(1), h, padding=h.shape[-1] // 2).squeeze(1)
        total = 0.0
        for n_fft, hop, win in res:
            mag = lambda v: torch.sqrt(torch.clamp(torch.view_as_real(torch.stft(v, n_fft, hop, win, wins[win], return_complex=True)).pow(2).sum(-1), min=eps))
            P, T = mag(p), mag(t)
            if w_sc:
                total = total + w_sc * torch.linalg.norm(T - P) / torch.linalg.norm(T)
            if w_log:
                total = total + w_log * F.l1_loss(torch.log(P), torch.log(T))
            if w_lin:
                total = total + w_lin * F.l1_loss(P, T)
        return total / len(res)
    return fn


def time_fwd_bwd(fn, x, t, iters, warmup):
    import torch
    for _ in range(warmup):
        x.grad = None
        fn(x, t).backward()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        x.grad = None
        fn(x, t).backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("all", "default", "hip"), default="all", help="hip: the HIP legs only (for a rocprofv3 run)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    work = [] if args.only == "default" else [("auto_eq", (16, 1, 131072)), ("auto_eq", (16, 2, 131072)), ("virtual_analog", (32, 1, 32768))]
    for name, shape in work:
        x = (torch.randn(*shape, device=dev, generator=g) * 0.3).requires_grad_(True)
        t = torch.randn(*shape, device=dev, generator=g) * 0.3
        kw = dict(fft_sizes=[r[0] for r in EXAMPLE_RES], hop_sizes=[r[1] for r in EXAMPLE_RES], win_lengths=[r[2] for r in EXAMPLE_RES])
        hip = D.losses.MultiResolutionSTFTLoss(**kw, w_sc=0.0, w_phs=0.0, w_lin_mag=1.0, w_log_mag=1.0, perceptual_weighting=True, sample_rate=44100)
        out = {"workload": name, "shape": list(shape), "hip_ms": round(time_fwd_bwd(hip, x, t, args.iters, args.warmup), 4)}
        if args.only == "all":
            ref = torch_loss(EXAMPLE_RES, 0.0, 1.0, 1.0, D.losses.a_weighting_taps(44100), dev)
            out["torch_ms"] = round(time_fwd_bwd(ref, x, t, args.iters, args.warmup), 4)
            out["speedup"] = round(out["torch_ms"] / out["hip_ms"], 2)
            with torch.no_grad():
                lh, lr = float(hip(x, t)), float(ref(x, t))
            out["loss_rel_diff"] = abs(lh - lr) / abs(lr)
        print(json.dumps(out), flush=True)
    x = (torch.randn(16, 2, 131072, device=dev, generator=g) * 0.3).requires_grad_(True)
    t = torch.randn(16, 2, 131072, device=dev, generator=g) * 0.3
    fn = D.losses.MultiResolutionSTFTLoss()
    print(json.dumps({"workload": "default", "shape": [16, 2, 131072], "root": os.path.abspath(args.root),
                      "hip_ms": round(time_fwd_bwd(fn, x, t, args.iters, args.warmup), 4),
                      "loss": float(fn(x, t).detach())}), flush=True)


if __name__ == "__main__":
    main()
