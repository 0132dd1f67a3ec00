"""functional.feedback_delay (csrc/fbdelay.hip) against the composition of torch ops that computes the same thing in float32 on the same
device: a Python loop over blocks of at most one delay length (the formulas of tests/feedback_delay_restated.py: four weighted slices of
the line's history, the one-pole as a triangular matrix of powers of a, blocks capped at 512 samples to bound that matrix), autograd for
its backward pass. It is the yardstick for time and memory, not for accuracy.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; the two legs run in alternation (fused, composed,
fused, composed ...) and each leg's median is over its own blocks. The workload is forward + backward (gradients for x and the four
controls) as a replayed graph - the device's time without the host's. A composed leg of more than --graph-max-blocks blocks is issued
eagerly instead (its graph would hold tens of thousands of nodes) and says so in its line. One JSON line per shape, delay and leg with the
time and the peak of torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
--kernels adds the fused C entry points' own times (device events around each call) against the HBM limit at 8 TB/s: 12 B per sample
forward (read x, write y and v), 16 B backward (read x, v and gy, write gx), and the time per sequential step of a row.
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
    ap.add_argument("--delays-ms", default="2,50,350")
    ap.add_argument("--max-delay-ms", type=float, default=500.0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--graph-max-blocks", type=int, default=100)
    ap.add_argument("--no-composed", action="store_true", help="time the fused op only")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    mdm = args.max_delay_ms
    H = math.ceil(SR / 1000.0 * mdm)
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    for B, C, N in shapes:
        for delay in (float(v) for v in args.delays_ms.split(",")):
            gen = torch.Generator(device=dev).manual_seed(0)
            u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo).requires_grad_(True)      # noqa: E731
            x = u(-1.0, 1.0, B, C, N)
            # one delay for the whole batch (within a tenth of a sample), so that the composition can take all items in one loop
            ctl = [u(delay + 0.02 / 44.1, delay + 0.1 / 44.1, B), u(0.3, 0.8, B), u(2000.0, 12000.0, B), u(0.2, 1.0, B)]
            w = torch.randn(B, C, N, device=dev, generator=gen)
            leaves = [x] + ctl
            i = int(math.floor(SR / 1000.0 * delay))
            assert int(math.floor(SR / 1000.0 * (delay + 0.11 / 44.1))) == i == int(math.floor(SR / 1000.0 * (delay + 0.01 / 44.1))) and 2 <= i < H
            S_fused = _lib.lib().dasp_fbdelay_block(H, i - 1)
            S = min(i - 1, 512)
            blocks = -(-N // S)

            def fused():
                return D.feedback_delay(x, SR, *ctl, max_delay_ms=mdm)

            def composed():
                f = (SR / 1000.0 * ctl[0].double() - i).float().view(B, 1, 1)          # (a float32 product would cost 1e-3 samples at 350 ms)
                fb, m = ctl[1].view(B, 1, 1), ctl[3].view(B, 1, 1)
                a = torch.exp(-2 * math.pi * torch.clamp(ctl[2], min=0.0) / SR).view(B, 1, 1)
                f2, f3 = f * f, f * f * f
                wrev = torch.stack(((f3 - f2) / 2, (-3 * f3 + 4 * f2 + f) / 2, (3 * f3 - 5 * f2 + 2) / 2, (-f3 + 2 * f2 - f) / 2), -1)
                j = torch.arange(S, device=dev)
                e = j.view(S, 1) - j.view(1, S)
                T = torch.where(e >= 0, a ** e.clamp(min=0).float(), torch.zeros((), device=dev))
                decay = a ** (j + 1).float()
                na = 1 - a
                hist = torch.zeros(B, C, i + 2, device=dev)
                rs = []
                for n0 in range(0, N, S):
                    s = min(S, N - n0)
                    r = (hist.unfold(-1, 4, 1)[..., :s, :] * wrev).sum(-1)
                    v = torch.einsum("gjm,gcm->gcj", T[:, :s, :s], na * (x[..., n0:n0 + s] + fb * r)) + decay[..., :s] * hist[..., -1:]
                    hist = torch.cat([hist[..., s:], v], -1)
                    rs.append(r)
                return (1 - m) * x + m * torch.cat(rs, -1)

            tag = {"shape": [B, C, N], "delay_ms": delay, "H": H, "step": S_fused, "steps_per_row": -(-N // S_fused)}
            forms = [("fused", fused)] + ([] if args.no_composed else [("composed", composed)])
            if not args.no_composed:
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
                for _ in range(args.warmup):
                    body(fn)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                body(fn)
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                if leg == "composed" and blocks > args.graph_max_blocks:
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
            for _ in range(args.repeats):
                for leg, step in steps.items():
                    times[leg].append(timed_block(step, args.iters if how[leg] == "fwd_bwd_graph" else 1))
            ms = {leg: statistics.median(times[leg]) for leg in steps}
            for leg in steps:
                print(json.dumps({**tag, "workload": how[leg], "leg": leg, "ms": round(ms[leg], 4), "min_ms": round(min(times[leg]), 4),
                                  "max_ms": round(max(times[leg]), 4), "peak_alloc_MB": round(peak[leg] / 1e6, 1),
                                  **({"composed_blocks": blocks} if leg == "composed" else {})}), flush=True)
            if "composed" in ms:
                print(json.dumps({**tag, "composed_over_fused": round(ms["composed"] / ms["fused"], 2)}), flush=True)
            del steps, keep
            if args.kernels:
                body(fused)
                _lib.timers.start()
                for _ in range(args.iters):
                    body(fused)
                per = _lib.timers.stop()
                n = B * C * N
                rounds = -(-B * C // CUS)              # a row is one workgroup on one CU: rows beyond 256 wait for a free one
                for entry, nbytes in (("dasp_fbdelay_forward", 12), ("dasp_fbdelay_backward", 16)):
                    t = statistics.median(per[entry])
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(n * nbytes / HBM / (t * 1e-3), 4), "rows": B * C,
                                      "us_per_step": round(t * 1e3 / (tag["steps_per_row"] * rounds), 3),
                                      "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")
                                              + f"; us_per_step = ms / (steps_per_row x {rounds} round(s) of rows over {CUS} CUs)"}), flush=True)


if __name__ == "__main__":
    main()
