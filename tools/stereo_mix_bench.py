"""functional.stereo_mix (csrc/stereo.hip mix_fwd_kernel / mix_bwd_kernel) against the composition it fuses,
stereo_bus(stereo_panner(x, sr, pan), sr, gain_db), on the same device and build (the composition's kernels are the parent's, unchanged).
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the two legs of a workload run in alternation (fused,
composed, fused, composed ...) and each leg's median is over its own blocks. Workloads: forward under no_grad and forward + backward
(gradients for x and every control), each without and with the effects send - the composition then runs the bus a second time at
gain_db + send_db on the same panned tracks. One JSON line per shape, workload and leg with the time, the GB/s of that leg's own byte
model (below) and the peak of torch.cuda.max_memory_allocated over one step, above what was allocated before it.
--graph adds forward + backward as a replayed graph (an eager step of either form costs the host about 0.2 ms, more than the device needs
at the smaller shapes). --kernels adds the fused C entry points' own times (device events around each call) and their share of the 8 TB/s HBM roofline.

Bytes per item (T tracks, N samples, s = 1 with the send else 0), counted from the kernels, fp32:
  fused     forward  4 T N + 8 (1 + s) N                       backward  8 T N + 8 (1 + s) N
  composed  forward  12 T N + (1 + s) (8 T N + 8 N)            backward  (1 + s) (16 T N + 8 N) + 24 s T N + 16 T N
            (panner: read x, write 2 rows per track; bus: read them, write 2 rows.  Backward: each bus reads the panned tracks and its
            upstream rows and writes their gradient, autograd adds the two gradients when there are two buses, the panner reads x and the
            gradient and writes gx.)"""
import argparse
import json
import os
import statistics
import sys

SHAPES = [(16, 8, 131072), (16, 16, 131072), (64, 8, 131072), (1, 16, 262144)]
SR = 44100
HBM = 8.0e12


def model_bytes(form, direction, B, T, N, s):
    if form == "fused":
        fwd, bwd = 4 * T * N + 8 * (1 + s) * N, 8 * T * N + 8 * (1 + s) * N
    else:
        fwd = 12 * T * N + (1 + s) * (8 * T * N + 8 * N)
        bwd = (1 + s) * (16 * T * N + 8 * N) + 24 * s * T * N + 16 * T * N
    return B * (fwd if direction == "fwd" else fwd + bwd)


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="all", help="'all' or B,T,N;B,T,N;...")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--graph", action="store_true", help="also time forward + backward as a replayed graph: the device's time without the host's")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    for B, T, N in shapes:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = (torch.rand(B, T, N, device=dev, generator=gen) * 2 - 1).requires_grad_(True)
        pan = (torch.rand(B, T, device=dev, generator=gen) * 0.9 + 0.05).requires_grad_(True)
        gain_db = (torch.rand(B, T, device=dev, generator=gen) * 36 - 24).requires_grad_(True)
        send_db = (torch.rand(B, T, device=dev, generator=gen) * 36 - 24).requires_grad_(True)
        w0, w1 = torch.randn(B, 2, N, device=dev, generator=gen), torch.randn(B, 2, N, device=dev, generator=gen)
        leaves = (x, pan, gain_db, send_db)

        def fused(s):
            return D.stereo_mix(x, SR, gain_db, pan, send_db) if s else (D.stereo_mix(x, SR, gain_db, pan), None)

        def composed(s):
            panned = D.stereo_panner(x, SR, pan)
            return D.stereo_bus(panned, SR, gain_db), (D.stereo_bus(panned, SR, gain_db + send_db) if s else None)

        def fwd_only(fn, s):
            def step():
                with torch.no_grad():
                    fn(s)
            return step

        def fwd_bwd(fn, s):
            def step():
                for t in leaves:
                    t.grad = None
                mix, send = fn(s)
                torch.autograd.backward([mix, send], [w0, w1]) if s else mix.backward(w0)
            return step

        with torch.no_grad():        # the two forms agree (a wrong benchmark is worse than none)
            (m0, s0), (m1, s1) = fused(1), composed(1)
            dm, ds = float((m0 - m1).abs().max() / m1.abs().max()), float((s0 - s1).abs().max() / s1.abs().max())
            assert dm < 4e-6 and ds < 4e-6, (dm, ds)
        print(json.dumps({"shape": [B, T, N], "segment": _lib.lib().dasp_stereo_mix_segment(B, N), "fused_vs_composed_mix": dm, "send": ds,
                          "model_ratio_fwd_bwd_no_send": round(model_bytes("composed", "fwd_bwd", B, T, N, 0) / model_bytes("fused", "fwd_bwd", B, T, N, 0), 3)}), flush=True)
        del m0, s0, m1, s1
        for direction, wrap in (("fwd", fwd_only), ("fwd_bwd", fwd_bwd)):
            for s in (0, 1):
                legs = [("fused", wrap(fused, s)), ("composed", wrap(composed, s))]
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
                    nbytes = model_bytes(leg, direction, B, T, N, s)
                    print(json.dumps({"shape": [B, T, N], "workload": direction, "send": s, "leg": leg, "ms": round(ms[leg], 4),
                                      "min_ms": round(min(times[leg]), 4), "max_ms": round(max(times[leg]), 4), "model_MB": round(nbytes / 1e6, 1),
                                      "model_GBps": round(nbytes / (ms[leg] * 1e-3) / 1e9, 1), "peak_alloc_MB": round(peak[leg] / 1e6, 1)}), flush=True)
                print(json.dumps({"shape": [B, T, N], "workload": direction, "send": s, "composed_over_fused": round(ms["composed"] / ms["fused"], 3)}),
                      flush=True)
        if args.graph:
            for s in (0, 1):
                graphs = {}
                for leg, fn in (("fused", fused), ("composed", composed)):
                    def body(fn=fn):
                        mix, send = fn(s)
                        return torch.autograd.grad([mix, send] if s else [mix], leaves if s else leaves[:3], [w0, w1] if s else [w0])
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(2):
                            body()
                    torch.cuda.current_stream().wait_stream(side)
                    graphs[leg] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[leg]):
                        keep = body()           # noqa: F841 (the graph's outputs stay alive with it)
                    for _ in range(args.warmup):
                        graphs[leg].replay()
                torch.cuda.synchronize()
                times = {leg: [] for leg in graphs}
                for _ in range(args.repeats):
                    for leg, gr in graphs.items():
                        times[leg].append(timed_block(gr.replay, args.iters))
                ms = {leg: statistics.median(times[leg]) for leg in graphs}
                for leg in graphs:
                    nbytes = model_bytes(leg, "fwd_bwd", B, T, N, s)
                    print(json.dumps({"shape": [B, T, N], "workload": "fwd_bwd_graph", "send": s, "leg": leg, "ms": round(ms[leg], 4),
                                      "min_ms": round(min(times[leg]), 4), "max_ms": round(max(times[leg]), 4),
                                      "model_GBps": round(nbytes / (ms[leg] * 1e-3) / 1e9, 1)}), flush=True)
                print(json.dumps({"shape": [B, T, N], "workload": "fwd_bwd_graph", "send": s,
                                  "composed_over_fused": round(ms["composed"] / ms["fused"], 3)}), flush=True)
                del graphs, keep
        if args.kernels:
            for s in (0, 1):
                step = fwd_bwd(fused, s)
                step()
                _lib.timers.start()
                for _ in range(args.iters):
                    step()
                per = _lib.timers.stop()
                for entry, direction in (("dasp_stereo_mix_forward", "fwd"), ("dasp_stereo_mix_backward", "bwd")):
                    ms = statistics.median(per[entry])
                    nbytes = model_bytes("fused", "fwd", B, T, N, s)
                    if direction == "bwd":
                        nbytes = model_bytes("fused", "fwd_bwd", B, T, N, s) - nbytes
                    print(json.dumps({"entry": entry, "shape": [B, T, N], "send": s, "ms": round(ms, 4), "model_MB": round(nbytes / 1e6, 1),
                                      "roofline_fraction": round(nbytes / (ms * 1e-3) / HBM, 3),
                                      "note": "device events around the C call" + (": both backward launches" if direction == "bwd" else "")}), flush=True)


if __name__ == "__main__":
    main()
