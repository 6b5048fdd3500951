#!/usr/bin/env python3
"""Per-kernel resource table of two builds of one .hip file, from the compiler's assembly.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S parent/bsa_align8_x.hip -o parent.s      (the same for the candidate)
    python tools/isa_table.py parent.s candidate.s [-o profiles/x_shared_isa.json] [--rename REGEX REPL ...]

Either side may be several assembly files joined by commas (a.s,b.s), for a change that moves kernels between files: their kernels form one table.

Reads the registers, scratch, LDS and spill count of every kernel from the assembly's metadata, counts each kernel's instruction lines (all, and those
that begin with v_) and hashes its instruction text (labels without the function's number, so that kernels added before it do not change it).  --rename
rewrites the candidate's mangled kernel names before they are matched (the first pattern that matches a name decides), for a change that adds a template parameter: the kernels keep their rows.  Prints the kernels whose figures differ; exit status 1 when the sets of kernels differ or scratch, LDS, a spill count or the
occupancy (waves per SIMD that the vector registers allow) of some kernel changed."""
import argparse
import hashlib
import json
import re
import subprocess
import sys

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def read_asm(path, renames=()):
    kernels, cur, body, meta = {}, None, None, False
    counts, text = {}, {}
    for line in open(path):
        if line.startswith("amdhsa.kernels:"):
            meta = True
        elif meta:
            m = re.match(r"  (?:- |  )\.(\w+):\s*(\S*)", line)          # an entry's own keys ("  - ." opens one); deeper lines are its arguments
            if m and line.startswith("  - "):
                cur = {}
            if m and cur is not None:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == "wavefront_size":          # (the last key of an entry: keys are sorted)
                    kernels[cur["name"]] = {k: int(cur[k]) for k in KEYS}
        elif body is None:
            m = re.match(r"(\w+):\s", line)
            if m and not line.startswith(".L"):
                body = m.group(1)
                counts[body] = [0, 0]
                text[body] = hashlib.sha1()
        elif line.startswith(".Lfunc_end"):
            body = None
        elif line.startswith("\t") and not line.startswith(("\t.", "\t;")):
            counts[body][0] += 1
            counts[body][1] += line.startswith("\tv_")
            text[body].update(re.sub(r"\.LBB\d+_", ".LBB_", line.replace(body, "@")).encode())
    for name, k in kernels.items():
        k["instructions"], k["v_instructions"] = counts[name]
        k["text_sha1"] = text[name].hexdigest()[:16]
    out = {}
    for name, k in kernels.items():
        for pat, repl in renames:          # the first pattern that matches decides
            if re.search(pat, name):
                name = re.sub(pat, repl, name)
                break
        out[name] = k
    return out


def waves(k):
    """waves per SIMD that the unified register file of 512 allows (allocation in steps of 8)"""
    regs = (k["vgpr_count"] + 7) // 8 * 8 + (k["agpr_count"] + 7) // 8 * 8
    return min(8, 512 // max(regs, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("candidate")
    ap.add_argument("-o", "--out")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    a = ap.parse_args()
    par, cand = {}, {}
    for path in a.parent.split(","):
        par.update(read_asm(path))
    for path in a.candidate.split(","):
        cand.update(read_asm(path, a.rename))
    names = demangle(sorted(set(par) | set(cand)))
    bad = set(par) != set(cand)
    table = {}
    for sym in sorted(names):
        p, c = par.get(sym), cand.get(sym)
        table[names[sym]] = {"parent": p, "candidate": c}
        if p is None or c is None:
            print("only in one build:", names[sym])
            continue
        if p != c:
            print(names[sym] + ": " + ", ".join("%s %s -> %s" % (k, p[k], c[k]) for k in p if p[k] != c[k]))
        if any(p[k] != c[k] for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")) or waves(p) != waves(c):
            print("  ^ scratch, LDS, spills or occupancy changed")
            bad = True
    same = sum(1 for v in table.values() if v["parent"] == v["candidate"])
    print("%d kernels, %d with equal figures" % (len(table), same))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"kernels": len(table), "equal": same, "table": table}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
