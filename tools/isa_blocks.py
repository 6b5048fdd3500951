#!/usr/bin/env python3
"""Basic blocks of one kernel in the compiler's assembly (the .s that tools/isa_table.py reads), with their instruction counts.

    python tools/isa_blocks.py candidate.s 'k_align8_fwd_xq<16, 4, 1, true, 3, false, true, true>' [--grep v_pk_mov_b32] [--show LABEL ...]

Prints one line per block in layout order: its label, instructions, vector instructions (v_), f64 ones among them, and how it ends (a branch's target or "falls
through").  --grep marks the blocks that hold a pattern, --show prints the text of the named blocks.  The every-row path of a loop is read off this list by hand:
the blocks that no conditional branch skips; tools/isa_table.py has the kernel's totals."""
import argparse
import re
import subprocess
import sys


def kernel_body(path, want):
    names, body, cur = {}, {}, None
    for line in open(path):
        m = re.match(r"(_Z\w+):\s", line)
        if m and cur is None:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                body[cur].append(line.rstrip("\n"))
    dem = subprocess.run(["c++filt"], input="\n".join(body), capture_output=True, text=True, check=True).stdout.split("\n")
    for sym, d in zip(body, dem):
        names[d] = sym
    hits = [d for d in names if want in d]
    if len(hits) != 1:
        sys.exit("%d kernels match %r: %s" % (len(hits), want, hits[:5]))
    return body[names[hits[0]]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--grep", action="append", default=[])
    ap.add_argument("--show", nargs="*", default=[])
    a = ap.parse_args()
    blocks, cur = [], {"label": "entry", "lines": []}
    for line in kernel_body(a.asm, a.kernel):
        m = re.match(r"(\.LBB\d+_\d+):", line) or re.match(r"; %bb\.(\d+):", line)
        if m:
            blocks.append(cur)
            cur = {"label": m.group(1) if line.startswith(".L") else "bb." + m.group(1), "lines": []}
        elif line.startswith("\t") and not line.startswith(("\t.", "\t;")):
            cur["lines"].append(line.strip())
    blocks.append(cur)
    for b in blocks:
        ins = b["lines"]
        v = [x for x in ins if x.startswith("v_")]
        f64 = [x for x in v if re.match(r"v_\w+_f64", x) or "_f64_" in x.split()[0]]
        br = [x for x in ins if x.startswith(("s_cbranch", "s_branch"))]
        marks = [g for g in a.grep if any(g in x for x in ins)]
        print("%-14s %4d ins %4d v_ %3d f64   %s%s" % (b["label"], len(ins), len(v), len(f64), "; ".join(br) if br else "falls through",
                                                      ("   <-- " + ", ".join(marks)) if marks else ""))
        if b["label"] in a.show:
            print("\n".join("        " + x for x in ins))


if __name__ == "__main__":
    main()
