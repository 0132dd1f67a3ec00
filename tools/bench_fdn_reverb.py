"""functional.fdn_reverb (csrc/fdn.hip) against three things on the same device, in alternated blocks:
  feedback_delay   functional.feedback_delay at a delay equal to the network's shortest line (the same steps per row, one line): the
                   cost per step and per line is read from the two;
  noise_reverb     functional.noise_shaped_reverberation at the same shape (device noise, a fixed seed), for orientation only;
  composed         the recurrence as torch ops in float32 (the formulas of tests/fdn_reverb_restated.py: a Python loop over blocks of at
                   most the shortest line, 512 samples at the most, the one-pole as a triangular matrix of powers of a), autograd for its
                   backward pass - the yardstick for time and memory, not for accuracy; issued eagerly beyond --graph-max-blocks blocks.
Device events after warm-up, the median of --repeats timed blocks of --iters steps; every leg's median is over its own blocks. The
workload is forward + backward (gradients for x and every control) as a replayed graph. One JSON line per shape, delay set and leg with
the time and the peak of torch.cuda.max_memory_allocated over one eager step above what was allocated before it.
Delay sets (--sets): k8 = signal.fdn_delay_lengths(44100), eight primes from 23 to 83 ms; k4 the same range with four lines; k16 sixteen
lines from 23 to 36 ms (what fits the LDS at K = 16); short = eight lines from 2 to 83 ms (88-sample steps).
--kernels adds the fused C entry points' own times (device events around each call) against the HBM limit at 8 TB/s: 8 + 4 K B per
sample forward (read x, write y and the K line signals), 12 + 4 K B backward (read x, gy and the line signals, write gx), and the time
per sequential step of a row.
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
SETS = {"k8": (8, 23.0, 83.0), "k4": (4, 23.0, 83.0), "k16": (16, 23.0, 36.0), "short": (8, 2.0, 83.0)}


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
    ap.add_argument("--sets", default="k8", help="comma-separated names of " + ", ".join(SETS))
    ap.add_argument("--legs", default="fused,feedback_delay,noise_reverb,composed")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--graph-max-blocks", type=int, default=100)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dasp_pytorch_amd as D
    from dasp_pytorch_amd import _lib
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = "cuda:0"
    shapes = SHAPES if args.shapes == "all" else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    legs = args.legs.split(",")
    for B, C, N in shapes:
        for name in args.sets.split(","):
            lines = D.fdn_delay_lengths(SR, *SETS[name])
            K = len(lines)
            gen = torch.Generator(device=dev).manual_seed(0)
            u = lambda lo, hi, *s: (torch.rand(*s, device=dev, generator=gen) * (hi - lo) + lo).requires_grad_(True)      # noqa: E731
            x = u(-1.0, 1.0, B, C, N)
            ctl = [u(0.5, 4.0, B), u(2000.0, 12000.0, B), u(0.2, 1.0, B)]
            w = torch.randn(B, C, N, device=dev, generator=gen)
            S_fused = _lib.lib().dasp_fdn_block(K, min(lines))
            S = min(min(lines), 512)
            blocks = -(-N // S)
            # feedback_delay: D = shortest line + 0.5 samples, so that its smallest lag and hence its step is the network's shortest line
            fb_ctl = [u((min(lines) + 1.4) / 44.1, (min(lines) + 1.6) / 44.1, B), u(0.3, 0.8, B), u(2000.0, 12000.0, B), u(0.2, 1.0, B)]
            rv_ctl = [u(0.1, 1.0, B) for _ in range(25)]

            def fused():
                return D.fdn_reverb(x, SR, *ctl, lines)

            def feedback_delay():
                return D.feedback_delay(x, SR, *fb_ctl, max_delay_ms=500.0)

            def noise_reverb():
                return D.noise_shaped_reverberation(x, SR, *rv_ctl, noise_seed=1234)

            def composed():
                Tc = torch.clamp(ctl[0].double(), 0.01, 100.0).view(B, 1)
                g = (10.0 ** (-3.0 * torch.tensor(lines, device=dev, dtype=torch.float64).view(1, K) / (SR * Tc))).float()
                a = torch.exp(-2 * math.pi * torch.clamp(ctl[1], min=0.0) / SR).view(B, 1, 1)
                m = ctl[2].view(B, 1, 1)
                j = torch.arange(S, device=dev)
                e = j.view(S, 1) - j.view(1, S)
                T = torch.where(e >= 0, a ** e.clamp(min=0).float(), torch.zeros((), device=dev))
                decay = a ** (j + 1).float()
                na = 1 - a
                sg = torch.tensor([[(-1.0) ** (k * c) for k in range(K)] for c in range(C)], device=dev)
                hist = [torch.zeros(B, C, mk, device=dev) for mk in lines]
                wets = []
                for n0 in range(0, N, S):
                    s = min(S, N - n0)
                    r = torch.stack([h[..., :s] for h in hist], 2)                                       # (B, C, K, s)
                    uu = g.view(B, 1, K, 1) * r
                    wk = x[..., n0:n0 + s].unsqueeze(2) + uu - (2.0 / K) * uu.sum(2, keepdim=True)
                    v = torch.einsum("bjm,bckm->bckj", T[:, :s, :s], na.unsqueeze(-1) * wk) + decay[..., :s].unsqueeze(2) * torch.stack([h[..., -1:] for h in hist], 2)
                    hist = [torch.cat([h[..., s:], v[:, :, k]], -1) for k, h in enumerate(hist)]
                    wets.append((sg.view(1, C, K, 1) * r).sum(2) / math.sqrt(K))
                return (1 - m) * x + m * torch.cat(wets, -1)

            tag = {"shape": [B, C, N], "set": name, "K": K, "shortest": min(lines), "sum": sum(lines), "step": S_fused, "steps_per_row": -(-N // S_fused)}
            forms = [(leg, fn, lv) for leg, fn, lv in (("fused", fused, [x] + ctl), ("feedback_delay", feedback_delay, [x] + fb_ctl),
                                                       ("noise_reverb", noise_reverb, [x] + rv_ctl), ("composed", composed, [x] + ctl)) if leg in legs]
            if "composed" in legs and "fused" in legs:
                with torch.no_grad():        # the two forms agree (a wrong benchmark is worse than none)
                    y0, y1 = fused(), composed()
                    dy = float((y0 - y1).abs().max() / y1.abs().max())
                    assert dy < 1e-3, dy
                print(json.dumps({**tag, "fused_vs_composed_y": dy}), flush=True)
                del y0, y1

            def body(fn, lv):
                y = fn()
                return torch.autograd.grad(y, lv, w if y.shape == w.shape else torch.ones_like(y))

            steps, peak, keep, how = {}, {}, [], {}
            for leg, fn, lv in forms:
                for _ in range(args.warmup):
                    body(fn, lv)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                body(fn, lv)
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                if leg == "composed" and blocks > args.graph_max_blocks:
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
                                  **({"composed_blocks": blocks} if leg == "composed" else {})}), flush=True)
            for other in ("feedback_delay", "noise_reverb", "composed"):
                if other in ms and "fused" in ms:
                    print(json.dumps({**tag, other + "_over_fused": round(ms[other] / ms["fused"], 3)}), flush=True)
            del steps, keep
            if args.kernels and "fused" in legs:
                body(fused, [x] + ctl)
                _lib.timers.start()
                for _ in range(args.iters):
                    body(fused, [x] + ctl)
                per = _lib.timers.stop()
                n = B * C * N
                rounds = -(-B * C // CUS)              # a row is one workgroup on one CU: rows beyond 256 wait for a free one
                for entry, nbytes in (("dasp_fdn_forward", 8 + 4 * K), ("dasp_fdn_backward", 12 + 4 * K)):
                    t = statistics.median(per[entry])
                    print(json.dumps({**tag, "entry": entry, "ms": round(t, 4), "bytes_per_sample": nbytes, "hbm_floor_ms": round(n * nbytes / HBM * 1e3, 4),
                                      "hbm_fraction": round(n * nbytes / HBM / (t * 1e-3), 4), "rows": B * C,
                                      "us_per_step": round(t * 1e3 / (tag["steps_per_row"] * rounds), 3),
                                      "note": "device events around the C call" + (": both backward launches" if entry.endswith("backward") else "")
                                              + f"; us_per_step = ms / (steps_per_row x {rounds} round(s) of rows over {CUS} CUs)"}), flush=True)


if __name__ == "__main__":
    main()
