"""functional.modulated_delay (csrc/moddelay.hip) against the composition of torch ops that computes the same thing in float32 on the same
device: an index tensor, four gathers and four weight tensors per voice, autograd for its backward pass (the formulas of
tests/modulated_delay_restated.py; its position is float32 too, which is what a user would write - it is the yardstick for time and
memory, not for accuracy).
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the two legs run in alternation (fused, composed,
fused, composed ...) and each leg's median is over its own blocks. The workload is forward + backward (gradients for x and the five
controls) as a replayed graph - the device's time without the host's - or issued eagerly with --eager. One JSON line per shape, voice
count and leg with the time and the peak of torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
--kernels adds the fused C entry points' own times (device events around each call) against the HBM limit: 8 B per sample forward
(read x, write y), 12 B backward (read x and gy, write gx), at 8 TB/s.
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="'all' or B,C,N;B,C,N;...")
    ap.add_argument("--voices", default="1,3")
    ap.add_argument("--max-delay-ms", type=float, default=40.0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--eager", action="store_true", help="issue the steps eagerly instead of replaying a graph")
    ap.add_argument("--no-composed", action="store_true", help="time the fused op only")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    mdm, spread = args.max_delay_ms, 0.25
    H = max(1, math.ceil(SR / 1000.0 * mdm))
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    for B, C, N in shapes:
        for V in (int(v) for v in args.voices.split(",")):
            gen = torch.Generator(device=dev).manual_seed(0)
            u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo).requires_grad_(True)      # noqa: E731
            x = u(-1.0, 1.0, B, C, N)
            ctl = [u(5.0, 25.0, B, V), u(0.0, 4.0, B, V), u(0.1, 8.0, B, V), u(0.0, 1.0, B, V), u(0.2, 1.0, B)]
            w = torch.randn(B, C, N, device=dev, generator=gen)
            leaves = [x] + ctl

            def fused():
                return D.modulated_delay(x, SR, *ctl, max_delay_ms=mdm, stereo_spread=spread)

            def composed():
                dl, dp, rt, ph = (t.view(B, 1, V, 1) for t in ctl[:4])
                n = torch.arange(N, device=dev, dtype=torch.float32).view(1, 1, 1, N)
                c = torch.arange(C, device=dev, dtype=torch.float32).view(1, C, 1, 1)
                k = SR / 1000.0
                d = torch.clamp(k * (dl + dp * torch.sin(2 * math.pi * (rt * n / SR + ph + c * spread))), 0.0, k * mdm)
                p = n - d
                i = torch.floor(p).detach()
                f = p - i
                f2, f3 = f * f, f * f * f
                wts = ((-f3 + 2 * f2 - f) / 2, (3 * f3 - 5 * f2 + 2) / 2, (-3 * f3 + 4 * f2 + f) / 2, (f3 - f2) / 2)
                xe = torch.nn.functional.pad(x, (H + 2, 3)).unsqueeze(2).expand(B, C, V, N + H + 5)
                idx = i.long() + (H + 2)
                wet = sum(wk * torch.gather(xe, 3, idx + kk) for kk, wk in zip((-1, 0, 1, 2), wts)).sum(2) / V
                m = ctl[4].view(B, 1, 1)
                return (1 - m) * x + m * wet

            tag = {"shape": [B, C, N], "V": V, "H": H, "tile": _lib.lib().dasp_moddelay_tile(H)}
            forms = [("fused", fused)] + ([] if args.no_composed else [("composed", composed)])
            if not args.no_composed:
                with torch.no_grad():        # the two forms agree (a wrong benchmark is worse than none) - over the first 4096 samples: the
                    y0, y1 = fused(), composed()        # composition's float32 position loses a bit per doubling of n (1 / 128 sample at n = 65536)
                    dy = float((y0 - y1)[..., :4096].abs().max() / y1.abs().max())
                    dy_all = float((y0 - y1).abs().max() / y1.abs().max())
                    assert dy < 1e-2, dy
                print(json.dumps({**tag, "fused_vs_composed_y_first_4096": dy, "fused_vs_composed_y": dy_all}), flush=True)
                del y0, y1

            def body(fn):
                return torch.autograd.grad(fn(), leaves, w)

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
                if args.eager:
                    steps[leg] = lambda fn=fn: body(fn)           # noqa: E731
                    continue
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
            workload = "fwd_bwd" if args.eager else "fwd_bwd_graph"
            for leg in steps:
                print(json.dumps({**tag, "workload": workload, "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4),
                                  "max_ms": round(max(times[leg]), 4), "peak_alloc_MB": round(peak[leg] / 1e6, 1)}), flush=True)
            if "composed" in ms:
                print(json.dumps({**tag, "workload": workload, "composed_over_fused": round(ms["composed"] / ms["fused"], 2)}), flush=True)
            del steps, keep
            if args.kernels:
                body(fused)
                _lib.timers.start()
                for _ in range(args.iters):
                    body(fused)
                per = _lib.timers.stop()
                n = B * C * N
                for entry, nbytes in (("dasp_moddelay_forward", 8), ("dasp_moddelay_backward", 12)):
                    t = statistics.median(per[entry])
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(n * nbytes / HBM / (t * 1e-3), 3),
                                      "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")}),
                          flush=True)


if __name__ == "__main__":
    main()
