"""Timing of signal.fft_sosfreqz (csrc/freqz.hip through torch.ops.dasp.freqz) against the same function written with torch.fft on the
same device (the reference's algorithm, dasp_pytorch/signal.py:7-32), forward and forward + backward, float32.

    python tools/freqz_bench.py [--reps 20 --blocks 7]

Device events around `reps` calls, median over `blocks` blocks after a warm-up block. Beside each time: the byte model (8 B per complex64
output value; backward also reads 8 B per cotangent value) and the fp64 operation model of the kernels (per (row, bin): the Horner
evaluations, products and divisions written out in csrc/freqz.hip, counted from the source), each as the time it would take at the HBM
rate of --hbm-tbs and the fp64 rate of --fp64-lane-ops: lane operations per second, an FMA counting as one, by default the device-wide
v_fma_f64 rate tools/ubench8.hip measured on the MI355X (3.19e13/s; the datasheet's 78.6 TFLOP/s counts an FMA as two FLOPs and
assumes a rate this part did not show). The instructions the kernels actually issue are counted by rocprofv3 --pmc runs of
`--shapes 256,6,262144 --hip-only` (profiles/r07/freqz/)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dasp_pytorch_amd as D  # noqa: E402

SHAPES = ((16, 6, 16384), (256, 6, 65536), (256, 6, 262144))


def torch_fft_sosfreqz(sos, n):
    H = None
    for s in range(sos.shape[1]):
        Hs = torch.fft.rfft(sos[:, s, :3], n) / torch.fft.rfft(sos[:, s, 3:], n)
        H = Hs if H is None else H * Hs
    return H


def timed(fn, reps, blocks):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out = sorted(out[1:])
    return out[len(out) // 2]


def fp64_ops(S, K=3):
    """fp64 lane operations per (row, bin), forward / backward, for S sections of K + K taps (counted from csrc/freqz.hip: a complex
    multiply is 4 operations (2 mul + 2 fma), a Horner step 5, a complex reciprocal ~12 (one fp64 division ~8), the twiddle amortised)."""
    horner = 5 * (K - 1)
    fwd = S * (2 * horner + 8) + 12 + 4
    # backward: both passes evaluate every section (4 Horner), suffix / prefix products, per section a reciprocal and 2 (K) term updates
    # of a complex power (4) and a real part (2), plus the LDS read-modify-write of 2 K accumulators
    bwd = S * (4 * horner + 4 * 4 + 12 + 2 * K * 6) + 12 + 3 * 4
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth of the byte model, TB/s")
    ap.add_argument("--fp64-lane-ops", type=float, default=31.9, help="fp64 lane operations (FMA = 1) per second of the model, T/s")
    ap.add_argument("--shapes", default=None, help="bs,S,n_fft[;bs,S,n_fft...] instead of the three default shapes")
    ap.add_argument("--hip-only", action="store_true", help="skip the torch.fft form (counter runs)")
    args = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    shapes = [tuple(int(v) for v in sh.split(",")) for sh in args.shapes.split(";")] if args.shapes else SHAPES
    for bs, S, n in shapes:
        r = 0.3 + 0.69 * torch.rand(bs, S, generator=gen)
        th = 3.1 * torch.rand(bs, S, generator=gen)
        a = torch.stack([torch.ones_like(r), -2 * r * torch.cos(th), r * r], -1)
        sos = torch.cat([torch.randn(bs, S, 3, generator=gen), a], -1).to(dev).requires_grad_(True)
        bins = n // 2 + 1
        W = torch.randn(bs, bins, dtype=torch.complex64, device=dev)
        row = {"shape": [bs, S, n]}
        forms = [("hip", lambda s: D.signal.fft_sosfreqz(s, n))] + ([] if args.hip_only else [("torch_fft", lambda s: torch_fft_sosfreqz(s, n))])
        for name, f in forms:
            with torch.no_grad():
                row[f"{name}_fwd_ms"] = timed(lambda: f(sos), args.reps, args.blocks)
            row[f"{name}_fwd_bwd_ms"] = timed(lambda: torch.autograd.grad(f(sos), sos, W), args.reps, args.blocks)
        fo, bo = fp64_ops(S)
        vals = bs * bins
        row["model_fwd_bytes"] = 8 * vals
        row["model_bwd_bytes"] = 8 * vals
        row["model_fwd_hbm_ms"] = 8 * vals / (args.hbm_tbs * 1e12) * 1e3
        row["model_fwd_bwd_hbm_ms"] = 16 * vals / (args.hbm_tbs * 1e12) * 1e3
        row["model_fp64_ops_per_value"] = [fo, bo]
        row["model_fwd_fp64_ms"] = vals * fo / (args.fp64_lane_ops * 1e12) * 1e3
        row["model_fwd_bwd_fp64_ms"] = vals * (fo + bo) / (args.fp64_lane_ops * 1e12) * 1e3
        if not args.hip_only:
            row["speedup_fwd_bwd_vs_torch_fft"] = row["torch_fft_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
