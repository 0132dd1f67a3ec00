"""Forward + backward of SumAndDifferenceSTFTLoss (dasp_pytorch_amd.losses, the item-owned kernels mrstft_sd_* of csrc/stftloss.hip) against
the composition it replaces - s = L + R and d = L - R formed with torch ops and MultiResolutionSTFTLoss called on each, (sum + diff) / 2 -
timed with device events after warm-up, the median of --repeats timed blocks of --iters steps. One JSON line per workload and leg:
  readme          auraloss's README loss - fft 1024 / 2048 / 8192 at hop n_fft / 4, scale="mel", n_bins=128, perceptual_weighting=True at
                  44.1 kHz - at (16,2,131072)
  default_16      auraloss's default three resolutions at (16,2,131072)
  default_8       the same at (8,2,262144)
Legs (--only): fused (needs this checkout), composition (the public API of any checkout that has the mel options: `--root DIR` imports
dasp_pytorch_amd from there, for a same-box comparison with the parent commit, the two alternated by the caller), torch (the README
loss as torch.stft + conv1d + matmul on the sum and difference signals, once), hip (fused only, 5 steps after 2 in 2 blocks unless given otherwise: for a rocprofv3 run).
The target does not require a gradient. The fused and composition legs print their loss value, which must agree."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrstft_mel_bench import README_RES, time_fwd_bwd, torch_mel_loss  # noqa: E402

DEFAULT_RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
WORKLOADS = {"readme": ((16, 2, 131072), README_RES, dict(scale="mel", n_bins=128, sample_rate=44100, perceptual_weighting=True)),
             "default_16": ((16, 2, 131072), DEFAULT_RES, {}),
             "default_8": ((8, 2, 262144), DEFAULT_RES, {})}


def composition(mono):
    def fn(p, t):
        return (mono(p[:, 0:1] + p[:, 1:2], t[:, 0:1] + t[:, 1:2]) + mono(p[:, 0:1] - p[:, 1:2], t[:, 0:1] - t[:, 1:2])) / 2
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("all", "fused", "composition", "torch", "hip"), default="all")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    if args.only == "hip":
        given = {a.split("=")[0] for a in sys.argv[1:]}
        args.iters, args.warmup, args.repeats = (args.iters if "--iters" in given else 5, args.warmup if "--warmup" in given else 2,
                                                 args.repeats if "--repeats" in given else 2)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    legs = {"all": ("fused", "composition", "torch"), "hip": ("fused",)}.get(args.only, (args.only,))
    for name in args.workloads.split(","):
        shape, res, opts = WORKLOADS[name]
        g = torch.Generator(device=dev).manual_seed(0)
        x = (torch.randn(*shape, device=dev, generator=g) * 0.3).requires_grad_(True)
        t = torch.randn(*shape, device=dev, generator=g) * 0.3
        kw = dict(fft_sizes=[r[0] for r in res], hop_sizes=[r[1] for r in res], win_lengths=[r[2] for r in res])
        for leg in legs:
            if leg == "fused":
                fn = D.losses.SumAndDifferenceSTFTLoss(**kw, **opts)
            elif leg == "composition":
                fn = composition(D.losses.MultiResolutionSTFTLoss(**kw, **opts))
            elif name == "readme":
                fn = composition(torch_mel_loss(res, 44100, 128, D.losses.mel_filterbank, D.losses.a_weighting_taps(44100), dev))
            else:
                continue
            ms = time_fwd_bwd(fn, x, t, args.iters, args.warmup, 1 if leg == "torch" else args.repeats)
            with torch.no_grad():
                loss = float(fn(x, t))
            print(json.dumps({"workload": name, "leg": leg, "shape": list(shape), "root": os.path.abspath(args.root), "ms": round(ms, 4),
                              "loss": loss}), flush=True)


if __name__ == "__main__":
    main()
