"""functional.time_varying_filter (csrc/tvfilter.hip) against the composition of torch ops that computes the same thing in float32 on the
same device: the recurrence of tests/tvfilter_restated.py as a Python loop over samples, every state kept for autograd, at a length that
loop can finish (--composed-samples; the fused op is timed at that length too, beside its full shapes). It is the yardstick for time and
memory, not for accuracy.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the legs run in alternation (fused, composed, fused,
composed ...) and each leg's median is over its own blocks. The workload is forward + backward (gradients for x, both curves and mix);
the fused op as a replayed graph - the device's time without the host's -, the composition issued eagerly (its graph would hold hundreds
of thousands of nodes) and says so in its line. One JSON line per shape, hop and leg with the time and the peak of
torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
--phaser adds functional.phaser at 1 and 4 stages at the same shapes in the same session: the same walk of a row with a scalar scan and a
per-sample LFO. --kernels adds the fused C entry points' own times (device events around each call) against the HBM limit at 8 TB/s: 8 B
per sample forward (read x, write y), 12 B backward (read x and gy, write gx), and the time per tile of a row.
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
    ap.add_argument("--hops", default="64,2048")
    ap.add_argument("--mode", default="lowpass")
    ap.add_argument("--composed-samples", type=int, default=2048, help="length of the torch composition's leg; 0: none")
    ap.add_argument("--phaser", action="store_true")
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
    T = _lib.lib().dasp_tvfilter_tile()
    ops = [("time_varying_filter", {"hop": int(h)}) for h in args.hops.split(",")] + ([("phaser", {"stages": 1}), ("phaser", {"stages": 4})] if args.phaser else [])
    for op, cfg in ops:
        runs = [(B, C, N, False) for B, C, N in shapes] + ([(B, C, Nc, True) for B, C, _ in shapes] if Nc and op != "phaser" else [])
        for B, C, N, with_composed in runs:
            gen = torch.Generator(device=dev).manual_seed(0)
            u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo)      # noqa: E731
            x = u(-1.0, 1.0, B, C, N).requires_grad_(True)
            if op == "phaser":
                ctl = [u(0.1, 5.0, B), u(300.0, 3000.0, B), u(0.5, 2.0, B), u(0.0, 1.0, B), u(0.2, 1.0, B)]
                entries = ("dasp_phaser_forward", "dasp_phaser_backward")
            else:
                hop = cfg["hop"]
                F = D.signal.control_frames(N, hop)
                ctl = [torch.exp(u(math.log(50.0), math.log(12000.0), B, F)), torch.exp(u(math.log(0.5), math.log(8.0), B, F)), u(0.2, 1.0, B)]
                entries = ("dasp_tvfilter_forward", "dasp_tvfilter_backward")
            ctl = [c.requires_grad_(True) for c in ctl]
            w = torch.randn(B, C, N, device=dev, generator=gen)
            leaves = [x] + ctl

            def fused():
                if op == "phaser":
                    return D.phaser(x, SR, *ctl, stages=cfg["stages"])
                return D.time_varying_filter(x, SR, *ctl, hop=hop, mode=args.mode)

            def composed():
                G = torch.tan(torch.clamp(ctl[0].double(), SR / 4096.0, 0.49 * SR) * (math.pi / SR)).float()
                K = (1.0 / torch.clamp(ctl[1].double(), 0.1, 100.0)).float()
                n = torch.arange(N, device=dev)
                j, t = n // hop, (n % hop).float() / hop
                g, k = (P[:, j] + t * (P[:, j + 1] - P[:, j]) for P in (G, K))
                a1 = 1 / (1 + g * (g + k))
                a2 = g * a1
                a3 = g * a2
                ic1 = ic2 = torch.zeros(B, C, device=dev)
                out = []
                for i in range(N):
                    xn, kn, p1, p2, p3 = x[..., i], k[:, None, i], a1[:, None, i], a2[:, None, i], a3[:, None, i]
                    v3 = xn - ic2
                    v1 = p1 * ic1 + p2 * v3
                    v2 = ic2 + p2 * ic1 + p3 * v3
                    ic1, ic2 = 2 * v1 - ic1, 2 * v2 - ic2
                    out.append({"lowpass": v2, "bandpass": kn * v1, "highpass": xn - kn * v1 - v2, "notch": xn - kn * v1}[args.mode])
                m = ctl[2].view(B, 1, 1)
                return (1 - m) * x + m * torch.stack(out, -1)

            tag = {"op": op, **cfg, "shape": [B, C, N], "tile": T, "tiles_per_row": -(-N // T)}
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
                for entry, nbytes in zip(entries, (8, 12)):
                    t = statistics.median(per[entry])
                    # a row is one workgroup: up to 256 rows every row has a CU to itself and the time of a tile can be read off
                    per_tile = {"us_per_tile": round(t * 1e3 / tag["tiles_per_row"], 3)} if B * C <= CUS else {}
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(n * nbytes / HBM / (t * 1e-3), 4), "rows": B * C, **per_tile,
                                      "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")}),
                          flush=True)


if __name__ == "__main__":
    main()
