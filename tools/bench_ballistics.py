"""functional.block_level, functional.ballistics and functional.sidechain_compressor (csrc/ballistics.hip) on one card at 44.1 kHz,
forward + backward as a replayed graph, in alternated blocks: device events after warm-up, the median of --repeats timed blocks of
--iters steps, every leg's median over its own blocks. One JSON line per shape, hop and leg.
  block_level   both detectors against abs -> amax(1) -> pad -> view(bs, F - 1, hop).amax(-1) (mean of the squares for power) with
                autograd, beside envelope_follower in the same session; its share of the HBM limit at 8 TB/s on the byte model per
                sample and channel: forward 4 (read x), peak backward 4 (write gx), power backward 8 (read x, write gx).
  ballistics    alone at F = 65, 2049 and 16385 (the frame counts of 131072 samples at hop 2048, 64 and 8), as time per frame of the
                forward and backward walks (device events around the C calls); as the torch yardstick the same recurrence as an eager
                Python loop at F = 2049.
  sidechain_compressor   beside compressor on the same shape, with the C entry points' own times, which say which stage the time is.
"""
import argparse
import json
import os
import statistics
import sys

SHAPES = [(16, 2, 131072), (256, 2, 131072)]
HOPS = [8, 64, 2048]
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
    ap.add_argument("--hops", default="all", help="'all' or 8,64,2048")
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

    def body(fn, lv, w):
        return torch.autograd.grad(fn(), lv, w)

    def graphs(forms):
        """{name: replay} of forward + backward steps, each captured after warm-up."""
        steps, keep = {}, []
        for name, fn, lv, w in forms:
            for _ in range(args.warmup):
                body(fn, lv, w)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body(fn, lv, w)
            torch.cuda.current_stream().wait_stream(side)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                keep.append(body(fn, lv, w))
            steps[name] = gr.replay
            for _ in range(args.warmup):
                gr.replay()
        torch.cuda.synchronize()
        return steps, keep

    def alternated(steps):
        times = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, step in steps.items():
                times[k].append(timed_block(step, args.iters))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}

    def entries(forms, names):
        """Median device time of each C entry point over --iters eager steps of the forms."""
        for name, fn, lv, w in forms:
            body(fn, lv, w)
        _lib.timers.start()
        for _ in range(args.iters):
            for name, fn, lv, w in forms:
                body(fn, lv, w)
        per = _lib.timers.stop()
        return {n: statistics.median(per[n]) for n in names if n in per}

    for B, C, N in shapes:
        for hop in hops:
            F = D.control_frames(N, hop)
            gen = torch.Generator(device=dev).manual_seed(0)
            x = (0.3 * torch.randn(B, C, N, device=dev, generator=gen)).requires_grad_(True)
            sm = (torch.rand(B, device=dev, generator=gen) * 45.0 + 5.0).requires_grad_(True)
            wL = torch.randn(B, F, device=dev, generator=gen)
            wy = torch.randn(B, C, N, device=dev, generator=gen)
            ctl = [(lo + (hi - lo) * torch.rand(B, device=dev, generator=gen)).requires_grad_(True)
                   for lo, hi in ((-30.0, -12.0), (2.0, 8.0), (1.0, 10.0), (30.0, 120.0), (2.0, 10.0), (0.0, 6.0))]
            tag = {"shape": [B, C, N], "sample_rate": SR, "hop": hop, "frames": F}
            pad = (F - 1) * hop - (N - 1)

            def composed(det):
                p = x.abs().amax(1) if det == "peak" else (x * x).mean(1)
                blocks = TF.pad(p[:, 1:], (0, pad)).view(B, F - 1, hop)
                return torch.cat([p[:, :1], blocks.amax(-1) if det == "peak" else blocks.mean(-1)], 1)

            with torch.no_grad():            # the two forms agree (a wrong benchmark is worse than none)
                for det in ("peak", "power"):
                    d = float((D.block_level(x, SR, hop, det) - composed(det)).abs().max() / composed(det).abs().max())
                    assert d < 1e-5, (det, d)
            forms = [("block_level_peak fused", lambda: D.block_level(x, SR, hop, "peak"), [x], wL),
                     ("block_level_peak composed", lambda: composed("peak"), [x], wL),
                     ("block_level_power fused", lambda: D.block_level(x, SR, hop, "power"), [x], wL),
                     ("block_level_power composed", lambda: composed("power"), [x], wL),
                     ("envelope_follower fused", lambda: D.envelope_follower(x, SR, sm, hop=hop), [x, sm], wL),
                     ("sidechain_compressor fused", lambda: D.sidechain_compressor(x, SR, *ctl, hop=hop), [x] + ctl, wy),
                     ("compressor fused", lambda: D.compressor(x, SR, *ctl), [x] + ctl, wy)]
            steps, keep = graphs(forms)
            ms = alternated(steps)
            for name, (med, lo, hi) in ms.items():
                op, leg = name.split()
                print(json.dumps({**tag, "op": op, "workload": "fwd_bwd_graph", "leg": leg, "ms": round(med, 4), "min_ms": round(lo, 4),
                                  "max_ms": round(hi, 4)}), flush=True)
            for det, nbytes in (("peak", 8 * C), ("power", 12 * C)):
                floor = B * N * nbytes / HBM * 1e3
                fused = ms[f"block_level_{det} fused"][0]
                print(json.dumps({**tag, "op": f"block_level_{det}", "composed_over_fused": round(ms[f"block_level_{det} composed"][0] / fused, 2),
                                  "fwd_bwd_bytes_per_item_sample": nbytes, "hbm_floor_ms": round(floor, 4), "hbm_fraction": round(floor / fused, 4),
                                  "envelope_follower_over_fused": round(ms["envelope_follower fused"][0] / fused, 2)}), flush=True)
            print(json.dumps({**tag, "op": "sidechain_compressor", "over_compressor": round(ms["sidechain_compressor fused"][0] / ms["compressor fused"][0], 3)}),
                  flush=True)
            del steps, keep
            names = ("dasp_blocklevel_forward", "dasp_blocklevel_backward", "dasp_ballistics_forward", "dasp_ballistics_backward",
                     "dasp_gaincurve_forward", "dasp_gaincurve_backward")
            per = entries([forms[5]], names)
            total = sum(per.values())
            print(json.dumps({**tag, "op": "sidechain_compressor", "workload": "eager entry points, device events around each C call",
                              **{n: round(t, 4) for n, t in per.items()}, "ballistics_share_of_entry_time": round(
                                  (per["dasp_ballistics_forward"] + per["dasp_ballistics_backward"]) / total, 3)}), flush=True)

    # ballistics alone: the serial walk, per frame
    for B in sorted({s[0] for s in shapes}):
        for F in (65, 2049, 16385):
            gen = torch.Generator(device=dev).manual_seed(1)
            P = (6.0 * torch.rand(B, F, device=dev, generator=gen)).requires_grad_(True)
            att = (1.0 + 9.0 * torch.rand(B, device=dev, generator=gen)).requires_grad_(True)
            rel = (30.0 + 90.0 * torch.rand(B, device=dev, generator=gen)).requires_grad_(True)
            w = torch.randn(B, F, device=dev, generator=gen)
            tag = {"op": "ballistics", "items": B, "frames": F, "sample_rate": SR, "hop": 64}
            form = ("ballistics fused", lambda: D.ballistics(P, SR, att, rel, 64), [P, att, rel], w)
            steps, keep = graphs([form])
            med, lo, hi = alternated(steps)["ballistics fused"]
            per = entries([form], ("dasp_ballistics_forward", "dasp_ballistics_backward"))
            print(json.dumps({**tag, "workload": "fwd_bwd_graph", "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                              "forward_ms": round(per["dasp_ballistics_forward"], 4), "backward_ms": round(per["dasp_ballistics_backward"], 4),
                              "forward_ns_per_frame": round(per["dasp_ballistics_forward"] * 1e6 / F, 2),
                              "backward_ns_per_frame": round(per["dasp_ballistics_backward"] * 1e6 / F, 2)}), flush=True)
            del steps, keep
            if F == 2049:                    # the torch yardstick: the same recurrence as an eager Python loop over the frames
                def loop():
                    ca, cr = (-torch.expm1(-2.1972245773362196 * 64 / (SR * c.clamp(0.1, 10000.0) / 1000.0)) for c in (att, rel))
                    e, out = torch.zeros(B, device=dev), []
                    for j in range(F):
                        p = P[:, j]
                        e = e + torch.where(p > e, ca, cr) * (p - e)
                        out.append(e)
                    return torch.stack(out, -1)
                body(loop, [P, att, rel], w)
                t = [timed_block(lambda: body(loop, [P, att, rel], w), 1) for _ in range(3)]
                print(json.dumps({**tag, "workload": "fwd_bwd eager python loop (torch yardstick)", "ms": round(statistics.median(t), 2),
                                  "over_fused": round(statistics.median(t) / med, 1)}), flush=True)


if __name__ == "__main__":
    main()
