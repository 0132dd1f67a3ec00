#!/usr/bin/env python3
"""Mnemonic counts of one kernel of csrc/sosfilt.hip from its cross-compiled gfx950 assembly (developer aid, needs no GPU).

    python scripts/isa_histogram.py sos_bwd_gram_kernelILi6ELi16ELi4ELi0ELi0          (a substring of the mangled name)
    python scripts/isa_histogram.py --all                                             (registers / occupancy / scratch of every kernel)
    python scripts/isa_histogram.py --asm FILE.s ...                                  (an assembly file made earlier instead of compiling)
    python scripts/isa_histogram.py --keep FILE.s -DFLAG=1 ...                        (keep the assembly; further -D flags go to hipcc)

The source is compiled with the flags of csrc/build.py. Printed: the kernel's VGPR count, occupancy and scratch size, the mnemonic
histogram of the whole kernel and that of its main loop - the longest run of instructions from a label to a later branch back to it
(the tile loop of the scan kernels; one iteration = one 1024-sample tile of one wave)."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dasp_pytorch_amd.csrc.build import HERE, HIPCC_FLAGS  # noqa: E402


def compile_asm(out, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc] + HIPCC_FLAGS + list(extra) + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                                                                  "-o", out, os.path.join(HERE, "sosfilt.hip")])


def functions(path):
    """name -> (instruction lines with labels, {property: value}) for every function of the assembly file"""
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name, body, i = m.group(1), [], i + 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            body.append(lines[i])
            i += 1
        props = {}
        while i < len(lines) and not re.match(r"^_Z\w+:", lines[i]):
            p = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", lines[i])
            if p:
                props.setdefault(p.group(1), int(p.group(2)))
            i += 1
        out[name] = (body, props)
    return out


def instructions(body):
    """[(label or None, mnemonic or None, operand text)] in program order"""
    seq = []
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.L\w+):", s)
            if m:
                seq.append((m.group(1), None, ""))
            continue
        m = re.match(r"^(\w+):$", s)
        if m:
            seq.append((m.group(1), None, ""))
            continue
        parts = s.split(None, 1)
        seq.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return seq


def main_loop(seq):
    """the instructions of the longest label .. backward-branch span"""
    pos = {lab: i for i, (lab, _, _) in enumerate(seq) if lab}
    best = (0, 0, 0)
    for i, (_, mn, ops) in enumerate(seq):
        if mn and "branch" in mn:
            tgt = ops.strip().split()[-1] if ops.strip() else ""
            if tgt in pos and pos[tgt] < i:
                n = sum(1 for _, m, _ in seq[pos[tgt]:i + 1] if m)
                if n > best[0]:
                    best = (n, pos[tgt], i + 1)
    return seq[best[1]:best[2]]


def histogram(seq, split_operand_of=()):
    c = collections.Counter()
    for _, mn, ops in seq:
        if mn:
            c[mn + (" " + ops.strip() if mn in split_operand_of else "")] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="?", help="substring of the kernel's mangled name")
    ap.add_argument("--all", action="store_true", help="one line per kernel: VGPRs, occupancy, scratch, instructions")
    ap.add_argument("--asm", help="read this assembly file, compile nothing")
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("--operands", action="append", default=[], metavar="MNEMONIC", help="count this mnemonic per operand text (repeatable)")
    ap.add_argument("--top", type=int, default=0, help="print only the N most frequent mnemonics")
    args, extra = ap.parse_known_args()
    if not args.all and not args.kernel:
        ap.error("a kernel name substring or --all")
    if args.asm:
        path = args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="isa_"), "sosfilt.s")
        compile_asm(path, extra)
    fns = functions(path)
    if args.all:
        print(f"{'VGPR':>5} {'AGPR':>5} {'occ':>4} {'scratch':>8} {'instr':>7}  kernel")
        for name, (body, p) in fns.items():
            n = sum(1 for _, m, _ in instructions(body) if m)
            print(f"{p.get('NumVgprs', -1):5d} {p.get('NumAgprs', -1):5d} {p.get('Occupancy', -1):4d} {p.get('ScratchSize', -1):8d} {n:7d}  {name}")
        bad = [n for n, (_, p) in fns.items() if p.get("ScratchSize", 0)]
        print("kernels with scratch:", bad if bad else "none")
        if not args.kernel:
            return 0
    hits = [n for n in fns if args.kernel in n]
    if len(hits) != 1:
        print(f"{len(hits)} kernels match {args.kernel!r}:", *hits, sep="\n  ", file=sys.stderr)
        return 1
    body, p = fns[hits[0]]
    seq = instructions(body)
    loop = main_loop(seq)
    print("kernel:", hits[0])
    print("VGPRs %d  AGPRs %d  SGPRs %d  occupancy %d  scratch %d B  LDS %d B" % tuple(
        p.get(k, -1) for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "Occupancy", "ScratchSize", "LDSByteSize")))
    hk, hl = histogram(seq, args.operands), histogram(loop, args.operands)
    print(f"instructions: kernel {sum(hk.values())}, main loop {sum(hl.values())}")
    print(f"{'mnemonic':<34} {'kernel':>7} {'loop':>7}")
    rows = sorted(hk.items(), key=lambda kv: (-kv[1], kv[0]))
    for mn, n in rows[:args.top] if args.top else rows:
        print(f"{mn:<34} {n:7d} {hl.get(mn, 0):7d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
