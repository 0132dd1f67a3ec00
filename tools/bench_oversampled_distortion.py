"""functional.oversampled_distortion (csrc/oversample.hip) against the composition of torch ops that computes the same thing on the
same device: conv_transpose1d (interpolation by L) -> tanh -> conv1d (low-pass and decimation by L), autograd for its backward pass.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the two legs of a workload run in alternation (fused,
composed, fused, composed ...) and each leg's median is over its own blocks. Workloads: forward under no_grad, forward + backward
(gradients for x and drive_db) issued eagerly, and forward + backward as a replayed graph (the device's time without the host's). One JSON
line per shape, factor, workload and leg with the time and the peak of torch.cuda.max_memory_allocated over one step above what was
allocated before it. --kernels adds the fused C entry points' own times (device events around each call) against the two limits:
  HBM     8 B per base sample forward (read x, write y), 12 B backward (read x and gy, write gx), at 8 TB/s
  issue   2 L (2 H + 1) fused multiply-adds per base sample forward (interpolator + decimator), 3 L (2 H + 1) backward (x and gy are
          interpolated, s is decimated), at the fp32 vector peak of 157.3 TFLOP/s = 78.6e12 multiply-adds per second; tanh / sech^2,
          the LDS accesses and the loop's own instructions come on top
--distortion times functional.distortion alone (to compare this tree with another: --root).

Bytes per base sample of the composition, fp32, counted from its ops (the L-times-longer tensors dominate):
  forward   4 + 4 L (conv_transpose1d) + 4 L + 4 L (the scale by g) + 4 L + 4 L (tanh) + 4 L + 4 (conv1d)            = 8 + 24 L
  backward  conv1d's input gradient 4 + 4 L, tanh's 4 L + 4 L + 4 L, the scale's 4 L + 4 L + 4 L (x) and 4 L + 4 L (g),
            conv_transpose1d's 4 L + 4                                                                            = 8 + 44 L
"""
import argparse
import json
import os
import statistics
import sys

SHAPES = [(16, 2, 131072), (256, 2, 131072)]
SR = 44100
HBM = 8.0e12
FMA_PEAK = 157.3e12 / 2


def model_bytes(form, direction, rows, N, L):
    if form == "fused":
        fwd, bwd = 8, 12
    else:
        fwd, bwd = 8 + 24 * L, 8 + 44 * L
    return rows * N * (fwd if direction == "fwd" else fwd + bwd)


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="'all' or B,C,N;B,C,N;...")
    ap.add_argument("--factors", default="4,8")
    ap.add_argument("--half-width", type=int, default=12)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--no-composed", action="store_true", help="time the fused op only")
    ap.add_argument("--distortion", action="store_true", help="time functional.distortion (forward, forward + backward) and nothing else")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import torch.nn.functional as TF
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    H = args.half_width
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    for B, C, N in shapes:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = (torch.rand(B, C, N, device=dev, generator=gen) * 2 - 1).requires_grad_(True)
        drive = (torch.rand(B * C, device=dev, generator=gen) * 30 - 6).requires_grad_(True)
        w = torch.randn(B, C, N, device=dev, generator=gen)
        leaves = (x, drive)

        def fwd_only(fn):
            def step():
                with torch.no_grad():
                    fn()
            return step

        def fwd_bwd(fn):
            def step():
                for t in leaves:
                    t.grad = None
                fn().backward(w)
            return step

        def measure(legs, tag, model=None):
            """legs: [(name, step)]; alternated blocks, medians, peak allocation of one step."""
            peak = {}
            for leg, step in legs:
                for _ in range(args.warmup):
                    step()
                torch.cuda.synchronize()
                for t in leaves:
                    t.grad = None
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                step()
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
            times = {leg: [] for leg, _ in legs}
            for _ in range(args.repeats):
                for leg, step in legs:
                    times[leg].append(timed_block(step, args.iters))
            ms = {leg: statistics.median(times[leg]) for leg, _ in legs}
            for leg, _ in legs:
                row = {**tag, "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4), "max_ms": round(max(times[leg]), 4),
                       "peak_alloc_MB": round(peak[leg] / 1e6, 1)}
                if model:
                    row["model_MB"] = round(model(leg) / 1e6, 1)
                print(json.dumps(row), flush=True)
            return ms

        if args.distortion:
            fn = lambda: D.distortion(x, SR, drive)          # noqa: E731
            measure([("distortion", fwd_only(fn))], {"shape": [B, C, N], "workload": "fwd"})
            measure([("distortion", fwd_bwd(fn))], {"shape": [B, C, N], "workload": "fwd_bwd"})
            continue

        for L in (int(v) for v in args.factors.split(",")):
            h32 = D.signal.oversampling_taps(L, H).to(device=dev, dtype=torch.float32).view(1, 1, -1)

            def fused():
                return D.oversampled_distortion(x, SR, drive, oversample=L, half_width=H)

            def composed():
                g = (10.0 ** (drive / 20.0)).view(B * C, 1, 1)
                u = TF.conv_transpose1d(x.view(B * C, 1, N), h32, stride=L)[..., H * L:H * L + L * N]
                return TF.conv1d(torch.tanh(g * u), h32 / L, stride=L, padding=H * L).view(B, C, N)

            tag = {"shape": [B, C, N], "L": L, "H": H}
            if not args.no_composed:
                with torch.no_grad():        # the two forms agree (a wrong benchmark is worse than none)
                    y0, y1 = fused(), composed()
                    dy = float((y0 - y1).abs().max() / y1.abs().max())
                    assert dy < 1e-5, dy
                print(json.dumps({**tag, "tile": _lib.lib().dasp_osdist_tile(L), "fused_vs_composed_y": dy,
                                  "model_ratio_fwd": round(model_bytes("composed", "fwd", B * C, N, L) / model_bytes("fused", "fwd", B * C, N, L), 2),
                                  "model_ratio_fwd_bwd": round(model_bytes("composed", "fwd_bwd", B * C, N, L) / model_bytes("fused", "fwd_bwd", B * C, N, L), 2)}),
                      flush=True)
                del y0, y1
            forms = [("fused", fused)] + ([] if args.no_composed else [("composed", composed)])
            for direction, wrap in (("fwd", fwd_only), ("fwd_bwd", fwd_bwd)):
                ms = measure([(leg, wrap(fn)) for leg, fn in forms], {**tag, "workload": direction},
                             model=lambda leg: model_bytes(leg, direction, B * C, N, L))
                if "composed" in ms:
                    print(json.dumps({**tag, "workload": direction, "composed_over_fused": round(ms["composed"] / ms["fused"], 2)}), flush=True)
            if args.graph:
                graphs = {}
                for leg, fn in forms:
                    def body(fn=fn):
                        return torch.autograd.grad(fn(), leaves, w)
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(2):
                            body()
                    torch.cuda.current_stream().wait_stream(side)
                    gr = torch.cuda.CUDAGraph()
                    try:
                        with torch.cuda.graph(gr):
                            keep = body()       # noqa: F841 (the graph's outputs stay alive with it)
                    except RuntimeError as err:     # a library call that cannot be captured: report it and time the other leg
                        print(json.dumps({**tag, "workload": "fwd_bwd_graph", "leg": leg, "capture_failed": str(err).splitlines()[0][:200]}), flush=True)
                        continue
                    graphs[leg] = gr
                    for _ in range(args.warmup):
                        gr.replay()
                torch.cuda.synchronize()
                times = {leg: [] for leg in graphs}
                for _ in range(args.repeats):
                    for leg, gr in graphs.items():
                        times[leg].append(timed_block(gr.replay, args.iters))
                ms = {leg: statistics.median(times[leg]) for leg in graphs}
                for leg in graphs:
                    print(json.dumps({**tag, "workload": "fwd_bwd_graph", "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4),
                                      "max_ms": round(max(times[leg]), 4)}), flush=True)
                if "composed" in ms:
                    print(json.dumps({**tag, "workload": "fwd_bwd_graph", "composed_over_fused": round(ms["composed"] / ms["fused"], 2)}), flush=True)
                del graphs
            if args.kernels:
                step = fwd_bwd(fused)
                step()
                _lib.timers.start()
                for _ in range(args.iters):
                    step()
                per = _lib.timers.stop()
                for entry, nbytes, fmas in (("dasp_osdist_forward", 8, 2 * L * (2 * H + 1)), ("dasp_osdist_backward", 12, 3 * L * (2 * H + 1))):
                    ms = statistics.median(per[entry])
                    n = B * C * N
                    print(json.dumps({**tag, "entry": entry, "ms": round(ms, 4), "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(n * nbytes / HBM / (ms * 1e-3), 3), "fma_per_sample": fmas,
                                      "issue_floor_ms": round(n * fmas / FMA_PEAK * 1e3, 4), "issue_fraction": round(n * fmas / FMA_PEAK / (ms * 1e-3), 3),
                                      "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")}),
                          flush=True)


if __name__ == "__main__":
    main()
