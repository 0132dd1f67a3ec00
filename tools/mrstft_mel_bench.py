"""Forward + backward of the mel-scaled STFT losses (dasp_pytorch_amd.losses with scale="mel" / MelSTFTLoss, csrc/stftloss.hip) against the
same loss written as torch.stft + matmul (+ conv1d for the A-weighting) on the GPU, timed with device events after warm-up, the median
of --repeats timed blocks. One JSON line per workload:
  readme_mel      auraloss's README loss - fft 1024 / 2048 / 8192 at hop n_fft / 4, scale="mel", n_bins=128, perceptual_weighting=True at
                  44.1 kHz - at (16,2,131072)
  mel_stft        MelSTFTLoss(44100) (fft 1024, hop 256, 128 bins) at (16,2,131072)
  default         auraloss's default loss at (16,2,131072) (no torch leg; `--only default` for same-box A/B runs, `--root DIR` imports
                  dasp_pytorch_amd from another checkout)
The target does not require a gradient. Also printed: the relative difference of the two losses' values."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

README_RES = ((1024, 256, 1024), (2048, 512, 2048), (8192, 2048, 8192))
MEL_RES = ((1024, 256, 1024),)


def torch_mel_loss(res, sample_rate, n_bins, filterbank, taps, device, w_sc=1.0, w_log=1.0, w_lin=0.0, eps=1e-8):
    import torch
    import torch.nn.functional as F
    wins = {w: torch.hann_window(w, device=device) for _, _, w in res}
    fbs = {n: torch.tensor(np.array(filterbank(sample_rate, n, n_bins)), device=device) for n, _, _ in res}
    h = None if taps is None else torch.tensor(np.array(taps), device=device).view(1, 1, -1)

    def fn(p, t):
        N = p.shape[-1]
        p, t = p.reshape(-1, N), t.reshape(-1, N)
        if h is not None:
            p = F.conv1d(p.unsqueeze(1), h, padding=h.shape[-1] // 2).squeeze(1)
            t = F.conv1d(t.unsqueeze(1), h, padding=h.shape[-1] // 2).squeeze(1)
        total = 0.0
        for n_fft, hop, win in res:
            mag = lambda v: torch.matmul(fbs[n_fft], torch.sqrt(torch.clamp(
                torch.view_as_real(torch.stft(v, n_fft, hop, win, wins[win], return_complex=True)).pow(2).sum(-1), min=eps)))
            P, T = mag(p), mag(t)
            if w_sc:
                total = total + w_sc * torch.linalg.norm(T - P) / torch.linalg.norm(T)
            if w_log:
                total = total + w_log * F.l1_loss(torch.log(P), torch.log(T))
            if w_lin:
                total = total + w_lin * F.l1_loss(P, T)
        return total / len(res)
    return fn


def time_fwd_bwd(fn, x, t, iters, warmup, repeats):
    import torch
    for _ in range(warmup):
        x.grad = None
        fn(x, t).backward()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            x.grad = None
            fn(x, t).backward()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("all", "default", "hip"), default="all", help="hip: the HIP legs of the two mel workloads only, no torch leg and no default loss (for a rocprofv3 run)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (16, 2, 131072)
    x = (torch.randn(*shape, device=dev, generator=g) * 0.3).requires_grad_(True)
    t = torch.randn(*shape, device=dev, generator=g) * 0.3
    work = [] if args.only == "default" else [("readme_mel", README_RES, True), ("mel_stft", MEL_RES, False)]
    for name, res, aw in work:
        if name == "mel_stft":
            hip = D.losses.MelSTFTLoss(44100)
        else:
            hip = D.losses.MultiResolutionSTFTLoss([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], scale="mel", n_bins=128,
                                                   sample_rate=44100, perceptual_weighting=True)
        out = {"workload": name, "shape": list(shape), "hip_ms": round(time_fwd_bwd(hip, x, t, args.iters, args.warmup, args.repeats), 4)}
        if args.only == "all":
            ref = torch_mel_loss(res, 44100, 128, D.losses.mel_filterbank, D.losses.a_weighting_taps(44100) if aw else None, dev)
            out["torch_ms"] = round(time_fwd_bwd(ref, x, t, args.iters, args.warmup, args.repeats), 4)
            out["speedup"] = round(out["torch_ms"] / out["hip_ms"], 2)
            with torch.no_grad():
                lh, lr = float(hip(x, t)), float(ref(x, t))
            out["loss_rel_diff"] = abs(lh - lr) / abs(lr)
        print(json.dumps(out), flush=True)
    if args.only == "hip":
        return
    fn = D.losses.MultiResolutionSTFTLoss()
    print(json.dumps({"workload": "default", "shape": list(shape), "root": os.path.abspath(args.root),
                      "hip_ms": round(time_fwd_bwd(fn, x, t, args.iters, args.warmup, args.repeats), 4),
                      "loss": float(fn(x, t).detach())}), flush=True)


if __name__ == "__main__":
    main()
