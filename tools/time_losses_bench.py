"""Forward + backward (input gradient only) of the time-domain losses (dasp_pytorch_amd.losses.time_domain_loss and SISDRLoss, the fused
moment kernels of csrc/tdloss.hip) against the same formulas written as torch ops on the same device, timed with device events after
warm-up: the median of --repeats timed blocks of --iters steps. One JSON line per workload, shape and leg:
  mix       w_esr=1, w_dc=1, w_mse=100 - the amp-modelling pair plus the MSE term of the reference's examples/virtual_analog.py
  si_sdr    SISDRLoss()
at (16,2,131072) and (256,2,131072).
Legs (--only): hip (the library), torch (the composition), all (both; for a comparison alternate `--only hip` and `--only torch` runs). Both
legs print their loss value, which must agree."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrstft_mel_bench import time_fwd_bwd  # noqa: E402

SHAPES = {"16": (16, 2, 131072), "256": (256, 2, 131072)}


def torch_mix(p, t, eps=1e-8):
    d = t - p
    t2 = (t ** 2).sum(-1)
    esr = (d ** 2).sum(-1) / (t2 + eps)
    dc = d.mean(-1) ** 2 / ((t ** 2).mean(-1) + eps)
    mse = ((p - t) ** 2).mean(-1)
    return (esr + dc + 100.0 * mse).mean()


def torch_si_sdr(p, t, eps=1e-8):
    import torch
    p = p - p.mean(-1, keepdim=True)
    t = t - t.mean(-1, keepdim=True)
    alpha = ((p * t).sum(-1) / ((t ** 2).sum(-1) + eps)).unsqueeze(-1)
    st = alpha * t
    return (-10.0 * torch.log10((st ** 2).sum(-1) / (((p - st) ** 2).sum(-1) + eps) + eps)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("all", "hip", "torch"), default="all")
    ap.add_argument("--workloads", default="mix,si_sdr")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    hip = {"mix": lambda p, t: D.losses.time_domain_loss(p, t, w_esr=1.0, w_dc=1.0, w_mse=100.0), "si_sdr": D.losses.SISDRLoss()}
    ref = {"mix": torch_mix, "si_sdr": torch_si_sdr}
    for key in args.shapes.split(","):
        shape = SHAPES[key]
        g = torch.Generator(device=dev).manual_seed(0)
        t = torch.randn(*shape, device=dev, generator=g) * 0.3
        x = (t + 0.09 * torch.randn(*shape, device=dev, generator=g) + 0.05).requires_grad_(True)
        for name in args.workloads.split(","):
            for leg in ("hip", "torch") if args.only == "all" else (args.only,):
                fn = (hip if leg == "hip" else ref)[name]
                ms = time_fwd_bwd(fn, x, t, args.iters, args.warmup, args.repeats)
                with torch.no_grad():
                    loss = float(fn(x, t))
                print(json.dumps({"workload": name, "leg": leg, "shape": list(shape), "ms": round(ms, 4), "loss": loss}), flush=True)


if __name__ == "__main__":
    main()
