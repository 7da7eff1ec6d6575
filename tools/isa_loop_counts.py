#!/usr/bin/env python3
"""Counts vector-ALU instruction classes inside the loops of one kernel's gfx950 assembly (hipcc --cuda-device-only -S).
A loop is the span from a label to the last backward branch to it; loops are reported outermost first with their line span, so the
innermost loops that hold a kernel's tile work are the ones with the large counts that contain no other large loop.
usage: isa_loop_counts.py <file.s> [kernel-name substring] [min VALU to report, default 300]"""
import re
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    floor = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    lines = open(path).read().split("\n")
    # the kernel's body: from its label to .Lfunc_end
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and want in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    loops = {}
    for i, l in enumerate(body):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)|\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] < i:
                loops[tgt] = max(loops.get(tgt, 0), i)
    classes = [("VALU", lambda op, l: op.startswith("v_") and not op.startswith(("v_accvgpr", "v_readfirstlane", "v_readlane", "v_writelane"))),
               ("pk_math_f32", lambda op, l: op in ("v_pk_add_f32", "v_pk_fma_f32", "v_pk_mul_f32")),
               ("v_mov_b32 reg", lambda op, l: op.startswith("v_mov_b32") and re.search(r"v_mov_b32\w*\s+v\d+,\s*v\d+", l) is not None),
               ("v_pk_mov_b32", lambda op, l: op == "v_pk_mov_b32"),
               ("v_xor sign", lambda op, l: op.startswith("v_xor_b32") and "0x80000000" in l),
               ("v_cndmask", lambda op, l: op.startswith("v_cndmask_b32")),
               ("v_accvgpr", lambda op, l: op.startswith("v_accvgpr")),
               ("scratch", lambda op, l: op.startswith("scratch_")),
               ("global_load", lambda op, l: op.startswith("global_load")),
               ("global_store", lambda op, l: op.startswith("global_store")),
               ("ds", lambda op, l: op.startswith("ds_")),
               ("s_barrier", lambda op, l: op == "s_barrier"),
               ("s_waitcnt", lambda op, l: op == "s_waitcnt")]
    print(f"# {body[0].rstrip(':')}")
    print("# loop(label: first..last line of the body) " + " | ".join(n for n, _ in classes))
    for tgt, last in sorted(loops.items(), key=lambda kv: labels[kv[0]]):
        counts = [0] * len(classes)
        for l in body[labels[tgt]:last + 1]:
            m = re.match(r"\s+([a-z_0-9]+)", l)
            if not m:
                continue
            op = m.group(1)
            for k, (_, f) in enumerate(classes):
                if f(op, l):
                    counts[k] += 1
        if counts[0] >= floor:
            print(f"{tgt}: {labels[tgt]}..{last} " + " | ".join(str(c) for c in counts))


if __name__ == "__main__":
    main()
