#!/usr/bin/env python3
"""= / X CIGAR words (BSA_MODE_CIGAR_EQX) against plain M / I / D words, device-resident (one process, one GPU).

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), 8-bit aligner, global, bandwidth 128, default scoring.
C3: 32 768 pairs of 100 kbp, edit aligner, global, bandwidth 256.
Both as device-resident plans on the same staged blob: `--warmup` steps of each form, then plain and flagged steps ALTERNATING, `--steps`
of each (at least five), timed between two synchronisations as bench.py times its step.  Ranges, not means.

Checked on EVERY pair of the last step of each form: records and status identical, the flagged words collapsed (runs of = / X merged into
M) equal the plain words, the = lengths sum to the record's mat and the X lengths to its mis, no word of length 0, no two neighbouring
words with the same op.

--flagged-only runs the flagged plan alone (for a kernel trace: rocprofv3 --kernel-trace --stats in a run of its own); --stats CSV folds
the rows of such a trace that matter (the traceback kernel and the three kernels of the pass) into the JSON line.  --only c2|c3 runs one
configuration.  Prints ONE JSON line."""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20240611
KERNELS = ("k_cigar_eqx_count", "k_cigar_collect_eqx", "k_cigar_final_direct_eqx", "k_cigar_final_direct", "k_cigar_final", "k_cigar_collect",
           "k_align8_trace_codes_wave", "k_edit_trace_wave", "k_edit_trace")


def kernel_stats(path):
    """the rows of a rocprofv3 --stats kernel table that the comparison is about: calls, average and total ms"""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            short = name.split("(")[0].split("<")[0].replace("void ", "").strip()
            if short in KERNELS:
                e = rows.setdefault(short, {"calls": 0, "total_ms": 0.0})
                e["calls"] += int(r["Calls"])
                e["total_ms"] += float(r["TotalDurationNs"]) / 1e6
    for e in rows.values():
        e["avg_ms"] = round(e["total_ms"] / max(e["calls"], 1), 4)
        e["total_ms"] = round(e["total_ms"], 3)
    return rows


def segment_sums(vals, off):
    """sum of vals[off[k]:off[k + 1]] for every k (empty segments give 0)"""
    cs = np.concatenate([[0], np.cumsum(vals, dtype=np.int64)])
    return cs[off[1:]] - cs[off[:-1]]


def check(plain, flagged):
    """(records, offsets, words, status) of the two forms -> dict of what holds on every pair"""
    po, poff, pw, pst = plain
    fo, foff, fw, fst = flagged
    n = len(po)
    fop, flen = fw & np.uint32(15), (fw >> np.uint32(4)).astype(np.int64)
    iseq, isx = fop == 7, fop == 8
    # collapse: a run of = / X words becomes one M word -- a word starts a collapsed word unless it and its predecessor in the same pair are both = / X
    ex = iseq | isx
    first = np.zeros(len(fw), dtype=bool)
    first[foff[:-1][foff[:-1] < foff[1:]]] = True
    head = ~ex | first | ~np.concatenate([[False], ex[:-1]])
    gid = np.cumsum(head) - 1
    clen = np.bincount(gid, weights=flen, minlength=int(head.sum())).astype(np.int64)
    cop = np.where(ex[head], 0, fop[head]).astype(np.uint32)
    collapsed = (clen.astype(np.uint32) << np.uint32(4)) | cop
    coff = np.concatenate([[0], np.cumsum(head, dtype=np.int64)])[foff]
    inner = np.ones(len(fw), dtype=bool)
    inner[0:1] = False
    inner[foff[:-1][foff[:-1] < foff[1:]]] = False             # a pair's first word has no neighbour in front
    return {
        "records_identical": bool(np.array_equal(po, fo)), "status_identical": bool(np.array_equal(pst, fst)),
        "collapsed_equals_plain": bool(np.array_equal(coff, poff) and np.array_equal(collapsed, pw)),
        "eq_sums_to_mat": bool(np.array_equal(segment_sums(np.where(iseq, flen, 0), foff), fo[:, 5].astype(np.int64))),
        "x_sums_to_mis": bool(np.array_equal(segment_sums(np.where(isx, flen, 0), foff), fo[:, 6].astype(np.int64))),
        "no_zero_length": bool((flen > 0).all()), "no_equal_neighbours": bool(not (inner[1:] & (fop[1:] == fop[:-1])).any()),
        "no_m_words": bool(not (fop == 0).any()),
        "pairs": int(n), "flagged_status": int((fst != 0).sum()),
        "words_per_pair": {"plain": round(len(pw) / n, 1), "eqx": round(len(fw) / n, 1)},
        "mis_per_pair": round(float(fo[:, 6].mean()), 1),
    }


def run(cfg, args, torch, B, ctx):
    dev = torch.device("cuda:0")
    lib = B.lib()
    n, L, bw, edit = cfg["pairs"], cfg["length"], cfg["bw"], cfg["edit"]
    stride = lib.bsa_synth_stride(L)
    nb = 2 * n * stride
    d_seqs = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    torch.cuda.synchronize()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
    cig_cap = n * max(L // 4, 64)                  # (expanded words at 10 % errors: about L / 5.5 a pair)
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(cig_cap, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)

    def plan_of(flag):
        if edit:
            return B.EditPlan(ctx, qoff, qlen, toff, tlen, B.MODE_GLOBAL | flag, bw)
        return B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL | flag, bw, 2, -6, -3, -2, 0, 0))
    forms = ["eqx"] if args.flagged_only else ["plain", "eqx"]
    plans = {name: plan_of(B.MODE_CIGAR_EQX if name == "eqx" else 0) for name in forms}
    times = {name: [] for name in forms}
    outs, names = {}, {}

    def step(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[name].run(d_seqs, d_out, d_cig, d_off, d_st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(args.warmup):
        for name in forms:
            step(name)
    for i in range(args.steps):
        for name in forms:
            times[name].append(round(step(name), 3))
            if i == args.steps - 1:
                off = d_off.cpu().numpy()
                assert int(off[n]) <= cig_cap, "CIGAR arena too small"
                outs[name] = (d_out.cpu().numpy().reshape(n, 10), off, d_cig[:int(off[n])].cpu().numpy().view(np.uint32), d_st.cpu().numpy().view(np.uint32))
                names[name] = ctx.last_kernel_names()
    for p in plans.values():
        p.close()
    res = {"config": {"pairs": n, "length": L, "bandwidth": bw, "aligner": "edit" if edit else "align8", "steps": args.steps, "warmup": args.warmup},
           "kernels": {k: list(v) for k, v in names.items()},
           "ms_per_step": {name: {"min": min(v), "max": max(v), "all": v} for name, v in times.items()}}
    if not args.flagged_only:
        res["check"] = check(outs["plain"], outs["eqx"])
        res["added_ms"] = {"min": round(min(times["eqx"]) - max(times["plain"]), 3), "max": round(max(times["eqx"]) - min(times["plain"]), 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed steps of each form, alternating (at least five)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", choices=["", "c2", "c3"])
    ap.add_argument("--c2-pairs", type=int, default=100000)
    ap.add_argument("--c3-pairs", type=int, default=32768)
    ap.add_argument("--flagged-only", action="store_true")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel_stats.csv of a --flagged-only run")
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()
    if args.steps < 5 and not args.flagged_only:
        ap.error("--steps must be at least 5")
    import torch
    import bsalign_amd as B
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    res = {}
    if args.only in ("", "c2"):
        res["C2"] = run({"pairs": args.c2_pairs, "length": 10000, "bw": 128, "edit": False}, args, torch, B, ctx)
    if args.only in ("", "c3"):
        res["C3"] = run({"pairs": args.c3_pairs, "length": 100000, "bw": 256, "edit": True}, args, torch, B, ctx)
    if args.stats:
        res["kernel_trace_of_the_flagged_run"] = kernel_stats(args.stats)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(all(v for k, v in r["check"].items() if isinstance(v, bool)) for r in res.values() if isinstance(r, dict) and "check" in r)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
