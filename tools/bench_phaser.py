"""functional.phaser (csrc/phaser.hip) against the composition of torch ops that computes the same thing in float32 on the same device:
the recurrence of tests/phaser_restated.py as a Python loop over samples and stages, every stage signal kept for autograd, at a length
that loop can finish (--composed-samples; the fused op is timed at that length too, beside its full shapes). It is the yardstick for time
and memory, not for accuracy.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the two legs run in alternation (fused, composed,
fused, composed ...) and each leg's median is over its own blocks. The workload is forward + backward (gradients for x and the five
controls); the fused op as a replayed graph - the device's time without the host's -, the composition issued eagerly (its graph would
hold hundreds of thousands of nodes) and says so in its line. One JSON line per shape, stage count and leg with the time and the peak of
torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
--kernels adds the fused C entry points' own times (device events around each call) against the HBM limit at 8 TB/s: 8 B per sample
forward (read x, write y), 12 B backward (read x and gy, write gx), and the time per tile of a row.
"""
import argparse
import json
import math
import os
import statistics
import sys

SHAPES = [(16, 2, 131072), (256, 2, 131072)]
SR = 44100
HBM = 8.0e12
CUS = 256


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="'all' or B,C,N;B,C,N;...")
    ap.add_argument("--stages", default="4,12")
    ap.add_argument("--composed-samples", type=int, default=2048, help="length of the torch composition's leg; 0: none")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    Nc = args.composed_samples
    runs = [(B, C, N, False) for B, C, N in shapes] + ([(B, C, Nc, True) for B, C, _ in shapes] if Nc else [])
    for K in (int(v) for v in args.stages.split(",")):
        T = _lib.lib().dasp_phaser_tile(K)
        for B, C, N, with_composed in runs:
            gen = torch.Generator(device=dev).manual_seed(0)
            u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo).requires_grad_(True)      # noqa: E731
            x = u(-1.0, 1.0, B, C, N)
            ctl = [u(0.1, 5.0, B), u(300.0, 3000.0, B), u(0.5, 2.0, B), u(0.0, 1.0, B), u(0.2, 1.0, B)]
            w = torch.randn(B, C, N, device=dev, generator=gen)
            leaves = [x] + ctl

            def fused():
                return D.phaser(x, SR, *ctl, stages=K)

            def composed():
                ex = lambda t: t.view(B, 1, 1)          # noqa: E731
                n = torch.arange(N, device=dev, dtype=torch.float64)
                c = torch.arange(C, device=dev, dtype=torch.float64).view(1, C, 1)
                turns = ex(ctl[0]).double() * n / SR + (ex(ctl[3]).double() + 0.25 * c)
                th = (turns - torch.round(turns)).float()
                f = torch.clamp(ex(ctl[1]) * torch.exp2(ex(ctl[2]) * torch.sin(2 * math.pi * th)), SR / 4096.0, 0.49 * SR)
                t = torch.tan(f * (math.pi / SR))
                a = (t - 1) / (t + 1)
                prev = [torch.zeros(B, C, device=dev) for _ in range(K + 1)]
                out = []
                for i in range(N):
                    an, cur = a[..., i], x[..., i]
                    new = [cur]
                    for k in range(1, K + 1):
                        cur = torch.addcmul(prev[k - 1], an, cur - prev[k])
                        new.append(cur)
                    prev = new
                    out.append(cur)
                m = ex(ctl[4])
                return (1 - m) * x + m * torch.stack(out, -1)

            tag = {"shape": [B, C, N], "stages": K, "tile": T, "tiles_per_row": -(-N // T)}
            forms = [("fused", fused)] + ([("composed", composed)] if with_composed else [])
            if with_composed:
                with torch.no_grad():        # the two forms agree (a wrong benchmark is worse than none)
                    y0, y1 = fused(), composed()
                    dy = float((y0 - y1).abs().max() / y1.abs().max())
                    assert dy < 1e-3, dy
                print(json.dumps({**tag, "fused_vs_composed_y": dy}), flush=True)
                del y0, y1

            def body(fn):
                return torch.autograd.grad(fn(), leaves, w)

            steps, peak, keep, how = {}, {}, [], {}
            for leg, fn in forms:
                for _ in range(args.warmup if leg == "fused" else 1):
                    body(fn)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                body(fn)
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                if leg == "composed":
                    steps[leg], how[leg] = (lambda fn=fn: body(fn)), "fwd_bwd_eager"           # noqa: E731
                    continue
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body(fn)
                torch.cuda.current_stream().wait_stream(side)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    keep.append(body(fn))                        # the graph's outputs stay alive with it
                steps[leg], how[leg] = gr.replay, "fwd_bwd_graph"
                for _ in range(args.warmup):
                    gr.replay()
            torch.cuda.synchronize()
            times = {leg: [] for leg in steps}
            for r in range(args.repeats):
                for leg, step in steps.items():
                    if leg == "composed" and r >= 2:             # seconds per step: two blocks of one
                        continue
                    times[leg].append(timed_block(step, args.iters if how[leg] == "fwd_bwd_graph" else 1))
            ms = {leg: statistics.median(times[leg]) for leg in steps}
            for leg in steps:
                print(json.dumps({**tag, "workload": how[leg], "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4),
                                  "max_ms": round(max(times[leg]), 4), "peak_alloc_MB": round(peak[leg] / 1e6, 2)}), flush=True)
            if "composed" in ms:
                print(json.dumps({**tag, "composed_over_fused": round(ms["composed"] / ms["fused"], 1)}), flush=True)
            del steps, keep
            if args.kernels and not with_composed:
                body(fused)
                _lib.timers.start()
                for _ in range(args.iters):
                    body(fused)
                per = _lib.timers.stop()
                n = B * C * N
                for entry, nbytes in (("dasp_phaser_forward", 8), ("dasp_phaser_backward", 12)):
                    t = statistics.median(per[entry])
                    # a row is one workgroup: up to 256 rows every row has a CU to itself and the time of a tile can be read off
                    per_tile = {"us_per_tile": round(t * 1e3 / tag["tiles_per_row"], 3)} if B * C <= CUS else {}
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(n * nbytes / HBM / (t * 1e-3), 4), "rows": B * C, **per_tile,
                                      "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")}),
                          flush=True)


if __name__ == "__main__":
    main()
