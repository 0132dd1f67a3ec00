"""Timing of signal.freqdomain_fir (csrc/fdfir.hip through torch.ops.dasp.freqdomain_fir) against the same function written with
torch.fft on the same device - irfft(rfft(x, n) * H, n), the reference's own lines (dasp_pytorch/signal.py:35-39; hipFFT / rocFFT
underneath) - forward and forward + backward, float32.

    python tools/freqdomain_fir_bench.py [--reps 20 --blocks 7 --shape fsm|rows|all] [--hip-only] [--steps N]

Two shapes: `fsm`, the reference's frequency-sampled sosfilt at a training batch (x (16, 2, 131072), n_fft = 262144, H (16, 1, 131073)
shared by the two channels), and `rows`, many short rows (x (256, 2, 4096), n_fft = 8192, a response per row).

Device events around `reps` calls; the two forms ALTERNATE block by block on the same device (A B A B ...), after a warm-up that runs
both for --warm-seconds so that the clocks have left idle; the median over `blocks` blocks of each is reported, with the spread
(min, max). Both forms' outputs and gradients are compared once before timing (they must agree to float32 rounding, else the timing
is of two different things). Beside each time: the algorithmic byte count - per row forward 4 T (x) + 8 (n/2 + 1) h_rows / rows (H)
+ 4 n (y); backward reads gy (4 n), x (4 T) and H again and writes gx (4 T) and gH (8 (n/2 + 1) h_rows / rows) - and the fraction of
--hbm-tbs (8 TB/s) that count over the measured time comes to. `--hip-only --steps N` runs N forward + backward steps of the HIP
form alone (the target of a `rocprofv3 --kernel-trace --stats` run); `--torch-only` the same for the torch.fft form."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dasp_pytorch_amd as D  # noqa: E402

SHAPES = {
    "fsm": dict(x=(16, 2, 131072), n=262144, h=(16, 1)),
    "rows": dict(x=(256, 2, 4096), n=8192, h=(256, 2)),
}


def torch_fft_form(x, H, n):
    return torch.fft.irfft(torch.fft.rfft(x, n) * H, n)


def byte_model(xs, n, hl):
    rows = xs[0] * xs[1]
    h_rows = hl[0] * hl[1]
    T, bins = xs[2], n // 2 + 1
    fwd = rows * (4 * T + 4 * n) + 8 * bins * h_rows
    bwd = rows * (4 * n + 4 * T + 4 * T) + 2 * 8 * bins * h_rows
    return fwd, bwd


def block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, reps, blocks, warm_seconds):
    """{name: [ms per call, one per block]}: the forms take turns block by block"""
    t0 = time.time()
    while time.time() - t0 < warm_seconds:
        for f in fns.values():
            block(f, reps)
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            out[k].append(block(f, reps))
    return out


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth of the byte model, TB/s")
    ap.add_argument("--shape", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="with --steps: run the HIP form alone (kernel-trace runs)")
    ap.add_argument("--torch-only", action="store_true", help="with --steps: run the torch.fft form alone (kernel-trace runs)")
    ap.add_argument("--steps", type=int, default=0, help="plain forward + backward steps instead of the timed comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freqdomain_fir_bench: no ROCm device (timings are taken on the GPU only)")
    dev = "cuda:0"
    for name in (list(SHAPES) if args.shape == "all" else [args.shape]):
        sh = SHAPES[name]
        xs, n, hl = sh["x"], sh["n"], sh["h"]
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(*xs, generator=gen).to(dev).requires_grad_(True)
        H = torch.view_as_complex(torch.randn(*hl, n // 2 + 1, 2, generator=gen)).to(dev).requires_grad_(True)
        w = torch.randn(*xs[:-1], n, generator=gen).to(dev)
        hip = lambda: D.signal.freqdomain_fir(x, H, n)
        ref = lambda: torch_fft_form(x, H, n)
        grad = lambda f: torch.autograd.grad(f(), (x, H), w)
        if args.steps:
            f = ref if args.torch_only else hip
            for _ in range(args.steps):
                grad(f)
            torch.cuda.synchronize()
            print(json.dumps({"shape": name, "form": "torch_fft" if args.torch_only else "hip", "steps": args.steps}), flush=True)
            continue
        # the two forms compute the same thing
        with torch.no_grad():
            ya, yb = hip(), ref()
        ga, gb = grad(hip), grad(ref)
        agree = {"y": ((ya - yb).abs().max() / yb.abs().max()).item(), "gx": ((ga[0] - gb[0]).abs().max() / gb[0].abs().max()).item(),
                 "gH": ((ga[1] - gb[1]).abs().max() / gb[1].abs().max()).item()}
        assert max(agree.values()) < 2e-5, agree
        del ya, yb, ga, gb

        def nograd(f):
            def g():
                with torch.no_grad():
                    f()
            return g

        fwd = alternate({"hip": nograd(hip), "torch_fft": nograd(ref)}, args.reps, args.blocks, args.warm_seconds)
        both = alternate({"hip": lambda: grad(hip), "torch_fft": lambda: grad(ref)}, args.reps, args.blocks, args.warm_seconds)
        fb, bb = byte_model(xs, n, hl)
        row = {"shape": name, "x": list(xs), "n_fft": n, "H": list(hl) + [n // 2 + 1], "max_rel_diff_vs_torch_fft": agree}
        for k in ("hip", "torch_fft"):
            row[f"{k}_fwd_ms"] = med(fwd[k])
            row[f"{k}_fwd_ms_min_max"] = [min(fwd[k]), max(fwd[k])]
            row[f"{k}_fwd_bwd_ms"] = med(both[k])
            row[f"{k}_fwd_bwd_ms_min_max"] = [min(both[k]), max(both[k])]
        row["model_fwd_bytes"], row["model_fwd_bwd_bytes"] = fb, fb + bb
        row["hip_fwd_fraction_of_hbm"] = fb / (args.hbm_tbs * 1e12) / (row["hip_fwd_ms"] * 1e-3)
        row["hip_fwd_bwd_fraction_of_hbm"] = (fb + bb) / (args.hbm_tbs * 1e12) / (row["hip_fwd_bwd_ms"] * 1e-3)
        row["speedup_fwd_vs_torch_fft"] = row["torch_fft_fwd_ms"] / row["hip_fwd_ms"]
        row["speedup_fwd_bwd_vs_torch_fft"] = row["torch_fft_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]

        def rnd(v):
            if isinstance(v, float):
                return float(f"{v:.4g}")
            if isinstance(v, list):
                return [rnd(e) for e in v]
            if isinstance(v, dict):
                return {k: rnd(e) for k, e in v.items()}
            return v

        print(json.dumps(rnd(row)), flush=True)


if __name__ == "__main__":
    main()
