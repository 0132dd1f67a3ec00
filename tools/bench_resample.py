"""functional.resample (csrc/resample.hip) against the composition of torch ops that torchaudio.functional.resample is made of, in float32
on the same device and build: pad, a strided conv1d with the full (n, 1, 2 width + o) kernel, transpose / reshape, crop, autograd for its
backward pass. It is the yardstick for time and memory, not for accuracy.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the two legs run in alternation (fused, composed,
fused, composed ...) and each leg's median is over its own blocks. The workload is forward + backward (gradient for x) as a replayed
graph - the device's time without the host's. One JSON line per shape, ratio and leg with the time and the peak of
torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
--kernels adds the fused C entry points' own times (device events around each call) against the HBM limit at 8 TB/s on 4 (N + M) bytes
per row, forward and backward each, and the multiply-adds per second. DASP_HIP_LIB selects a variant build of the library.
"""
import argparse
import json
import os
import statistics
import sys

SHAPES = [(16, 2, 131072), (256, 2, 131072)]
RATIOS = [(44100, 48000), (48000, 44100), (44100, 16000)]
HBM = 8.0e12


def timed_block(step, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="'all' or B,C,N;B,C,N;...")
    ap.add_argument("--ratios", default="all", help="'all' or orig:new,orig:new,...")
    ap.add_argument("--method", default="sinc_interp_hann")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--no-composed", action="store_true", help="time the fused op only")
    ap.add_argument("--tag", default="", help="a label copied into every line (a variant build's name)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib, ops
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    ratios = RATIOS if args.ratios == "all" else [tuple(int(v) for v in s.split(":")) for s in args.ratios.split(",")]
    for B, C, N in shapes:
        for orig, new in ratios:
            o, n = D.signal.check_resampling(orig, new)
            gen = torch.Generator(device=dev).manual_seed(0)
            x = (torch.rand(B, C, N, device=dev, generator=gen) * 2 - 1).requires_grad_(True)
            taps, width = D.signal.resample_taps(o, n, resampling_method=args.method)
            kernel = taps.float().to(dev)[:, None]
            M = -(-n * N // o)
            w = torch.randn(B, C, M, device=dev, generator=gen)
            d = ops.resample_design(o, n, 6, 0.99, args.method, None)
            products = int(d.fwd.cnt.sum())                    # per frame of n outputs; the transposed table holds the same ones

            def fused():
                return D.resample(x, orig, new, resampling_method=args.method)

            def composed():
                xp = torch.nn.functional.pad(x.reshape(B * C, 1, N), (width, width + o))
                y = torch.nn.functional.conv1d(xp, kernel, stride=o)
                return y.transpose(1, 2).reshape(B * C, -1)[..., :M].reshape(B, C, M)

            tag = {"shape": [B, C, N], "ratio": f"{o}:{n}", "M": M, "taps_per_output": round(products / n, 2), "conv_taps": int(taps.shape[1]),
                   **({"build": args.tag} if args.tag else {})}
            forms = [("fused", fused)] + ([] if args.no_composed else [("composed", composed)])
            if not args.no_composed:
                with torch.no_grad():        # the two forms agree (a wrong benchmark is worse than none)
                    y0, y1 = fused(), composed()
                    dy = float((y0 - y1).abs().max() / y1.abs().max())
                    assert y0.shape == y1.shape and dy < 1e-5, dy
                print(json.dumps({**tag, "fused_vs_composed_y": dy}), flush=True)
                del y0, y1

            def body(fn):
                return torch.autograd.grad(fn(), [x], w)

            steps, peak, keep = {}, {}, []
            for leg, fn in forms:
                for _ in range(args.warmup):
                    body(fn)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                body(fn)
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body(fn)
                torch.cuda.current_stream().wait_stream(side)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    keep.append(body(fn))                        # the graph's outputs stay alive with it
                steps[leg] = gr.replay
                for _ in range(args.warmup):
                    gr.replay()
            torch.cuda.synchronize()
            times = {leg: [] for leg in steps}
            for _ in range(args.repeats):
                for leg, step in steps.items():
                    times[leg].append(timed_block(step, args.iters))
            ms = {leg: statistics.median(times[leg]) for leg in steps}
            for leg in steps:
                print(json.dumps({**tag, "workload": "fwd_bwd_graph", "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4),
                                  "max_ms": round(max(times[leg]), 4), "peak_alloc_MB": round(peak[leg] / 1e6, 1)}), flush=True)
            if "composed" in ms:
                print(json.dumps({**tag, "composed_over_fused": round(ms["composed"] / ms["fused"], 2)}), flush=True)
            del steps, keep
            if args.kernels:
                body(fused)
                _lib.timers.start()
                for _ in range(args.iters):
                    body(fused)
                per = _lib.timers.stop()
                nbytes = 4 * (N + M) * B * C
                fma = B * C * (M / n) * products
                for entry in ("dasp_resample_forward", "dasp_resample_backward"):
                    t = statistics.median(per[entry])
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "hbm_floor_ms": round(nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(nbytes / HBM / (t * 1e-3), 4), "rows": B * C,
                                      "gfma_per_s": round(fma / (t * 1e-3) / 1e9, 1), "note": "device events around the C call"}), flush=True)
            del x, w, kernel


if __name__ == "__main__":
    main()
