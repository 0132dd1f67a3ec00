"""functional.envelope_follower and functional.gain_curve (csrc/envelope.hip) against their compositions from existing ops on the same
device and build, in alternated blocks:
  envelope     abs -> amax over the channels -> zero padding to the last frame point -> signal.lfilter_via_fsm (b = [1 - a, 0],
               a = [1, -a]) -> strided slice, with autograd through all of it;
  gain_curve   the interpolation as index arithmetic (two gathers of the curve and a lerp), 10^(g / 20), a multiply, with autograd.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; every leg's median is over its own blocks. The
workload is forward + backward (gradients for x and the control) as a replayed graph at 44.1 kHz. One JSON line per shape, hop and leg
with the time and the peak of torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
--kernels adds the C entry points' own times (device events around each call) against the HBM limit at 8 TB/s on the ops' algorithmic
bytes per sample and channel: envelope forward 4 (read x), backward 8 (read x, write gx); gain_curve forward 8, backward 12.
"""
import argparse
import json
import math
import os
import statistics
import sys

SHAPES = [(16, 2, 131072), (256, 2, 131072)]
HOPS = [64, 2048]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="'all' or B,C,N;B,C,N;...")
    ap.add_argument("--hops", default="all", help="'all' or 64,2048")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import torch.nn.functional as TF
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    hops = HOPS if args.hops == "all" else [int(h) for h in args.hops.split(",")]
    for B, C, N in shapes:
        for hop in hops:
            F = D.control_frames(N, hop)
            gen = torch.Generator(device=dev).manual_seed(0)
            x = (0.3 * torch.randn(B, C, N, device=dev, generator=gen)).requires_grad_(True)
            sm = (torch.rand(B, device=dev, generator=gen) * 45.0 + 5.0).requires_grad_(True)
            P = (torch.rand(B, F, device=dev, generator=gen) * 36.0 - 24.0).requires_grad_(True)
            wE = torch.randn(B, F, device=dev, generator=gen)
            wy = torch.randn(B, C, N, device=dev, generator=gen)
            n = torch.arange(N, device=dev)
            jj, tt = n // hop, (n % hop).float() / hop

            def env_fused():
                return D.envelope_follower(x, SR, sm, hop=hop)

            def env_composed():
                a = torch.exp(-math.log(9.0) / (SR * sm.clamp(0.1, 10000.0) / 1000.0))
                p = TF.pad(x.abs().amax(1, keepdim=True), (0, (F - 1) * hop + 1 - N))
                e = D.signal.lfilter_via_fsm(p, torch.stack([1 - a, torch.zeros_like(a)], -1), torch.stack([torch.ones_like(a), -a], -1))
                return e[:, 0, ::hop]

            def gc_fused():
                return D.gain_curve(x, SR, P, hop=hop)

            def gc_composed():
                p0 = P[:, jj]
                g = p0 + tt * (P[:, jj + 1] - p0)
                return x * torch.pow(10.0, g / 20.0).unsqueeze(1)

            tag = {"shape": [B, C, N], "sample_rate": SR, "hop": hop, "frames": F}
            with torch.no_grad():            # the two forms agree (a wrong benchmark is worse than none)
                dE = float((env_fused() - env_composed()).abs().max() / env_composed().abs().max())
                dy = float((gc_fused() - gc_composed()).abs().max() / gc_composed().abs().max())
                assert dE < 1e-3 and dy < 1e-4, (dE, dy)
            print(json.dumps({**tag, "envelope_fused_vs_composed": dE, "gain_curve_fused_vs_composed": dy}), flush=True)
            forms = [("envelope", "fused", env_fused, [x, sm], wE), ("envelope", "composed", env_composed, [x, sm], wE),
                     ("gain_curve", "fused", gc_fused, [x, P], wy), ("gain_curve", "composed", gc_composed, [x, P], wy)]

            def body(fn, lv, w):
                return torch.autograd.grad(fn(), lv, w)

            steps, peak, keep = {}, {}, []
            for op, leg, fn, lv, w in forms:
                for _ in range(args.warmup):
                    body(fn, lv, w)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                body(fn, lv, w)
                torch.cuda.synchronize()
                peak[op, leg] = torch.cuda.max_memory_allocated() - base
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body(fn, lv, w)
                torch.cuda.current_stream().wait_stream(side)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    keep.append(body(fn, lv, w))                 # the graph's outputs stay alive with it
                steps[op, leg] = gr.replay
                for _ in range(args.warmup):
                    gr.replay()
            torch.cuda.synchronize()
            times = {k: [] for k in steps}
            for _ in range(args.repeats):
                for k, step in steps.items():
                    times[k].append(timed_block(step, args.iters))
            ms = {k: statistics.median(v) for k, v in times.items()}
            for (op, leg) in steps:
                print(json.dumps({**tag, "op": op, "workload": "fwd_bwd_graph", "leg": leg, "ms": round(ms[op, leg], 4), "min_ms": round(min(times[op, leg]), 4),
                                  "max_ms": round(max(times[op, leg]), 4), "peak_alloc_MB": round(peak[op, leg] / 1e6, 1)}), flush=True)
            for op, nbytes in (("envelope", 12 * C), ("gain_curve", 20 * C)):
                floor = B * N * nbytes / HBM * 1e3
                print(json.dumps({**tag, "op": op, "composed_over_fused": round(ms[op, "composed"] / ms[op, "fused"], 2),
                                  "fwd_bwd_bytes_per_item_sample": nbytes, "hbm_floor_ms": round(floor, 4),
                                  "hbm_fraction": round(floor / ms[op, "fused"], 4)}), flush=True)
            del steps, keep
            if args.kernels:
                for fn, lv, w in ((env_fused, [x, sm], wE), (gc_fused, [x, P], wy)):
                    body(fn, lv, w)
                _lib.timers.start()
                for _ in range(args.iters):
                    body(env_fused, [x, sm], wE)
                    body(gc_fused, [x, P], wy)
                per = _lib.timers.stop()
                for entry, nbytes in (("dasp_envelope_forward", 4 * C), ("dasp_envelope_backward", 8 * C), ("dasp_gaincurve_forward", 8 * C),
                                      ("dasp_gaincurve_backward", 12 * C)):
                    t = statistics.median(per[entry])
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "bytes_per_item_sample": nbytes,
                                      "hbm_floor_ms": round(B * N * nbytes / HBM * 1e3, 4), "hbm_fraction": round(B * N * nbytes / HBM / (t * 1e-3), 4),
                                      "workgroups_per_sample_pass": B * -(-N // _lib.lib().dasp_envelope_tile()),
                                      "note": "device events around the C call: every launch of the call"}), flush=True)


if __name__ == "__main__":
    main()
