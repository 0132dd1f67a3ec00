"""functional.time_varying_eq (csrc/tveq.hip) beside functional.time_varying_filter (bandpass) at the same shapes in the same session: the
sibling is the yardstick - the same walk of a row with one curve fewer.
Device events after warm-up; the workload is forward + backward (gradients for x and every curve, and mix for the sibling) as a replayed
graph - the device's time without the host's. The legs of a shape and hop (the sibling, then the three modes) run in alternated blocks of
--iters steps, --repeats blocks per leg, and each leg's figure is the median over its own blocks. One JSON line per shape, hop and leg
with the time, its ratio to the sibling's and the peak of torch.cuda.max_memory_allocated over one eager step above what was allocated
before it.
--kernels adds the C entry points' own times (device events around each call) against the HBM limit at 8 TB/s: 8 B per sample forward
(read x, write y), 12 B backward (read x and gy, write gx), and the time per tile of a row.
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
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    from dasp_pytorch_amd.functional import TVEQ_MODES
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    T = _lib.lib().dasp_tveq_tile()
    for hop in (int(h) for h in args.hops.split(",")):
        for B, C, N in shapes:
            gen = torch.Generator(device=dev).manual_seed(0)
            u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo)      # noqa: E731
            x = u(-1.0, 1.0, B, C, N).requires_grad_(True)
            F = D.signal.control_frames(N, hop)
            cut, q = (torch.exp(u(math.log(lo), math.log(hi), B, F)).requires_grad_(True) for lo, hi in ((50.0, 12000.0), (0.5, 8.0)))
            gain, mix = u(-18.0, 18.0, B, F).requires_grad_(True), u(0.2, 1.0, B).requires_grad_(True)
            w = torch.randn(B, C, N, device=dev, generator=gen)
            legs = {"time_varying_filter": (lambda: D.time_varying_filter(x, SR, cut, q, mix, hop=hop, mode="bandpass"), [x, cut, q, mix],
                                            ("dasp_tvfilter_forward", "dasp_tvfilter_backward"))}
            for mode in TVEQ_MODES:
                legs["time_varying_eq " + mode] = (lambda mode=mode: D.time_varying_eq(x, SR, gain, cut, q, hop=hop, mode=mode), [x, gain, cut, q],
                                                   ("dasp_tveq_forward", "dasp_tveq_backward"))
            tag = {"hop": hop, "shape": [B, C, N], "tile": T, "tiles_per_row": -(-N // T)}

            def body(leg):
                fn, leaves, _ = legs[leg]
                return torch.autograd.grad(fn(), leaves, w)

            steps, peak, keep = {}, {}, []
            for leg in legs:
                for _ in range(args.warmup):
                    body(leg)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                body(leg)
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body(leg)
                torch.cuda.current_stream().wait_stream(side)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    keep.append(body(leg))                       # the graph's outputs stay alive with it
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
                                  "max_ms": round(max(times[leg]), 4), "over_sibling": round(ms[leg] / ms["time_varying_filter"], 3),
                                  "peak_alloc_MB": round(peak[leg] / 1e6, 2)}), flush=True)
            del steps, keep
            if args.kernels:
                n = B * C * N
                for leg, (_, _, entries) in legs.items():
                    body(leg)
                    _lib.timers.start()
                    for _ in range(args.iters):
                        body(leg)
                    per = _lib.timers.stop()
                    for entry, nbytes in zip(entries, (8, 12)):
                        t = statistics.median(per[entry])
                        # a row is one workgroup: up to 256 rows every row has a CU to itself and the time of a tile can be read off
                        per_tile = {"us_per_tile": round(t * 1e3 / tag["tiles_per_row"], 3)} if B * C <= CUS else {}
                        print(json.dumps({**tag, "leg": leg, "entry": entry, "ms": round(t, 4), "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                          "hbm_fraction": round(n * nbytes / HBM / (t * 1e-3), 4), "rows": B * C, **per_tile,
                                          "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")}),
                              flush=True)


if __name__ == "__main__":
    main()
