"""functional.limiter (csrc/limiter.hip) against two things on the same device, in alternated blocks:
  compressor   functional.compressor at the same shape (the same bytes in and out: the natural yardstick of a dynamics op);
  composed     the same definition as torch ops in float32 on --composed-samples samples (2048): max_pool1d for the hold, a Python loop
               over samples for the release, avg_pool1d for the box, autograd for the backward pass; issued eagerly - the yardstick for
               time, not for accuracy.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; every leg's median is over its own blocks. The
workload is forward + backward (gradients for x and every control) as a replayed graph at 44.1 kHz with 5 ms of look-ahead. One JSON
line per shape and leg with the time and the peak of torch.cuda.max_memory_allocated over one eager step above what was allocated
before it.
--kernels adds the C entry points' own times (device events around each call) against the HBM limit at 8 TB/s on the op's algorithmic
bytes per item sample: forward 8 C + 8 (read x, write y, G and the winners), backward 12 C + 8 (read x, gy, G and the winners, write
gx); and the time per tile of an item - an item is one workgroup on one compute unit, so B items use B of the 256.
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
    ap.add_argument("--legs", default="fused,compressor,composed")
    ap.add_argument("--lookahead-ms", type=float, default=5.0)
    ap.add_argument("--composed-samples", type=int, default=2048)
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
    legs = args.legs.split(",")
    L = D.functional.limiter_lookahead(SR, args.lookahead_ms)
    T = _lib.lib().dasp_limiter_tile()
    for B, C, N in shapes:
        gen = torch.Generator(device=dev).manual_seed(0)
        u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo).requires_grad_(True)      # noqa: E731
        env = torch.exp(0.8 * torch.randn(B, 1, (N + 47) // 48, device=dev, generator=gen)).repeat_interleave(48, -1)[..., :N]
        x = (0.35 * torch.randn(B, C, N, device=dev, generator=gen) * env).requires_grad_(True)
        ctl = [u(-20.0, -8.0, B), u(20.0, 200.0, B)]
        cmp_ctl = [u(-20.0, -8.0, B), u(2.0, 8.0, B), u(1.0, 30.0, B), u(20.0, 200.0, B), u(1.0, 6.0, B), u(0.0, 3.0, B)]
        w = torch.randn(B, C, N, device=dev, generator=gen)
        Nc = min(N, args.composed_samples)
        xc = x.detach()[..., :Nc].clone().requires_grad_(True)

        def fused():
            return D.limiter(x, SR, *ctl, lookahead_ms=args.lookahead_ms)

        def compressor():
            return D.compressor(x, SR, *cmp_ctl)

        def composed():
            thr = ctl[0].clamp(-120.0, 40.0).view(B, 1)
            rho = torch.exp(-math.log(9.0) / (SR * ctl[1].clamp(0.1, 10000.0) / 1000.0))
            p = xc.abs().amax(1)
            r = (20.0 * torch.log10(p.clamp(min=1e-8)) - thr).clamp(min=0.0)
            r = TF.pad(r, (L, L))                                            # L zeros before 0, the timeline's L samples after N
            h = TF.max_pool1d(r.unsqueeze(1), L + 1, 1).squeeze(1)           # h[m], m in [0, Nc + L)
            e, prev = [], torch.zeros(B, device=dev)
            for m in range(Nc + L):
                prev = torch.maximum(h[:, m], rho * prev)
                e.append(prev)
            e = TF.pad(torch.stack(e, 1), (L, 0))
            s = TF.avg_pool1d(e.unsqueeze(1), L + 1, 1).squeeze(1)           # s[m], m in [0, Nc + L)
            return xc * (10.0 ** (-s[:, L:] / 20.0)).unsqueeze(1)

        tag = {"shape": [B, C, N], "sample_rate": SR, "lookahead": L, "tiles_per_item": -(-(N + L) // T)}
        forms = [(leg, fn, lv) for leg, fn, lv in (("fused", fused, [x] + ctl), ("compressor", compressor, [x] + cmp_ctl),
                                                   ("composed", composed, [xc] + ctl)) if leg in legs]
        if "composed" in legs and "fused" in legs:
            with torch.no_grad():            # the two forms agree (a wrong benchmark is worse than none)
                y0, y1 = D.limiter(xc, SR, *ctl, lookahead_ms=args.lookahead_ms), composed()
                dy = float((y0 - y1).abs().max() / y1.abs().max())
                assert dy < 1e-3, dy
            print(json.dumps({**tag, "fused_vs_composed_y": dy, "composed_samples": Nc}), flush=True)
            del y0, y1

        def body(fn, lv):
            y = fn()
            return torch.autograd.grad(y, lv, w[..., :y.shape[-1]])

        steps, peak, keep, how = {}, {}, [], {}
        for leg, fn, lv in forms:
            for _ in range(args.warmup if leg != "composed" else 1):
                body(fn, lv)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            body(fn, lv)
            torch.cuda.synchronize()
            peak[leg] = torch.cuda.max_memory_allocated() - base
            if leg == "composed":
                steps[leg], how[leg] = (lambda fn=fn, lv=lv: body(fn, lv)), "fwd_bwd_eager"           # noqa: E731
                continue
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body(fn, lv)
            torch.cuda.current_stream().wait_stream(side)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                keep.append(body(fn, lv))                    # the graph's outputs stay alive with it
            steps[leg], how[leg] = gr.replay, "fwd_bwd_graph"
            for _ in range(args.warmup):
                gr.replay()
        torch.cuda.synchronize()
        times = {leg: [] for leg in steps}
        for _ in range(args.repeats):
            for leg, step in steps.items():
                times[leg].append(timed_block(step, args.iters if how[leg] == "fwd_bwd_graph" else 1))
        ms = {leg: statistics.median(times[leg]) for leg in steps}
        for leg in steps:
            print(json.dumps({**tag, "workload": how[leg], "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4),
                              "max_ms": round(max(times[leg]), 4), "peak_alloc_MB": round(peak[leg] / 1e6, 1),
                              **({"composed_samples": Nc} if leg == "composed" else {})}), flush=True)
        if "compressor" in ms and "fused" in ms:
            print(json.dumps({**tag, "fused_over_compressor": round(ms["fused"] / ms["compressor"], 3)}), flush=True)
        if "composed" in ms and "fused" in ms:
            print(json.dumps({**tag, "composed_per_sample_over_fused_per_sample": round(ms["composed"] / Nc / (ms["fused"] / N), 1)}), flush=True)
        del steps, keep
        if args.kernels and "fused" in legs:
            body(fused, [x] + ctl)
            _lib.timers.start()
            for _ in range(args.iters):
                body(fused, [x] + ctl)
            per = _lib.timers.stop()
            rounds = -(-B // CUS)                      # an item is one workgroup on one CU: items beyond 256 wait for a free one
            for entry, nbytes in (("dasp_limiter_forward", 8 * C + 8), ("dasp_limiter_backward", 12 * C + 8)):
                t = statistics.median(per[entry])
                print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "bytes_per_item_sample": nbytes,
                                  "hbm_floor_ms": round(B * N * nbytes / HBM * 1e3, 4), "hbm_fraction": round(B * N * nbytes / HBM / (t * 1e-3), 4),
                                  "items": B, "compute_units_used": min(B, CUS), "us_per_tile": round(t * 1e3 / (tag["tiles_per_item"] * rounds), 3),
                                  "note": "device events around the C call" + (": the zeroing kernel and the backward kernel" if entry.endswith("backward") else "")
                                          + f"; us_per_tile = ms / (tiles_per_item x {rounds} round(s) of items over {CUS} CUs)"}), flush=True)


if __name__ == "__main__":
    main()
