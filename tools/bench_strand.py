#!/usr/bin/env python3
"""Per-pair reverse-complement queries (BSA_MODE_QSTRAND) against the plain plan, at C2, device-resident (one process, one GPU).

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring.  Forms, all on the
same pairs at the same offsets:

  plain           the unflagged plan on the blob as the generator made it (1 B/base);
  strand          every second query reverse-complemented IN PLACE in the blob (3 - flip, a torch expression) and marked with
                  BSA_QOFF_REVCOMP, the plan with BSA_MODE_QSTRAND -- the aligner therefore sees the very sequences of `plain`;
  plain2b         the unflagged BSA_MODE_SEQ2BIT plan on the packed original blob;
  strand2b        the flagged BSA_MODE_SEQ2BIT plan on the packed modified blob.

Each form: `--warmup` steps, then `--steps` steps timed one by one between two synchronisations (as bench.py times its step); the JSON
line has the median and the spread.  `identical`: records, CIGAR offsets, CIGAR words and status of every form equal those of `plain`,
for every pair.  --plain-only measures `plain` alone (a library built from a commit without the flag: BSA_LIB_PATH).

The staging kernels' own time comes from a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_strand.py ...);
--stats CSV folds the k_stage / k_stage2b rows of that run's kernel table into the JSON line, one row per instantiation (the ones
with `true` as their second template argument are the flagged plans').  Prints ONE JSON line."""
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


def staging_stats(path):
    """the align staging kernels' rows of a rocprofv3 --stats kernel table, by instantiation"""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "k_stage" in name and "k_edit" not in name:
                rows[name.split("(")[0].replace("void ", "")] = {"calls": int(r["Calls"]), "avg_ms": round(float(r["AverageNs"]) / 1e6, 4)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel_stats.csv of an earlier run of this tool")
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = B.lib()
    n, L, bw = args.pairs, args.length, args.bw
    stride = lib.bsa_synth_stride(L)
    nb = 2 * n * stride
    d_seqs = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    torch.cuda.synchronize()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)          # (one byte a base: byte offsets are base offsets)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
    cells = float(L) * bw * n
    cig_cap = n * max(L // 4, 64)
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(cig_cap, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    res = {"config": {"pairs": n, "length": L, "bandwidth": bw, "scoring": "2,-6,-3,-2,0,0", "steps": args.steps, "warmup": args.warmup,
                      "library": os.path.relpath(B.LIB_PATH, ROOT)}}

    def pack(d):
        d_bits = torch.zeros((nb + 31) // 32, dtype=torch.int64, device=dev)
        ctx.seq_pack2bit(d, d_bits)
        torch.cuda.synchronize()
        return d_bits

    def measure(flags, d, qo):
        plan = B.AlignPlan(ctx, qo, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL | flags, bw, 2, -6, -3, -2, 0, 0))

        def step():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan.run(d, d_out, d_cig, d_off, d_st)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(args.warmup):
            step()
        ms = [step() for _ in range(args.steps)]
        kms, _, _ = ctx.last_kernel_ms()
        off = d_off.cpu().numpy()
        outs = (d_out.cpu().numpy().reshape(n, 10), off, d_cig[:int(off[n])].cpu().numpy().view(np.uint32), d_st.cpu().numpy().view(np.uint32))
        plan.close()
        med = float(np.median(ms))
        return {"ms_per_step": round(med, 3), "steps_ms": [round(x, 3) for x in ms], "gcups": round(cells / med / 1e6, 1),
                "forward_ms": round(kms, 3), "forward_kernel": ctx.last_kernel_names()[0]}, outs

    timing, outs = {}, {}
    timing["plain"], outs["plain"] = measure(0, d_seqs, qoff)
    if not args.plain_only:
        d_bits = pack(d_seqs)
        timing["plain2b"], outs["plain2b"] = measure(B.MODE_SEQ2BIT, d_bits, qoff)
        del d_bits
        # every second query reverse-complemented where it lies, and marked
        marked = qoff.copy()
        for k in range(0, n, 2):
            a, b = int(qoff[k]), int(qoff[k]) + int(qlen[k])
            d_seqs[a:b] = 3 - d_seqs[a:b].flip(0)
            marked[k] |= np.uint64(B.QOFF_REVCOMP)
        torch.cuda.synchronize()
        timing["strand"], outs["strand"] = measure(B.MODE_QSTRAND, d_seqs, marked)
        d_bits = pack(d_seqs)
        timing["strand2b"], outs["strand2b"] = measure(B.MODE_QSTRAND | B.MODE_SEQ2BIT, d_bits, marked)
        res["marked_pairs"] = int((n + 1) // 2)
    res["device_resident"] = timing
    res["identical"] = bool(all(np.array_equal(x, y) for name in outs for x, y in zip(outs["plain"], outs[name])))
    res["flagged"] = int((outs["plain"][3] != 0).sum())
    if args.stats:
        res["staging_kernels"] = staging_stats(args.stats)
    print(json.dumps(res))
    return 0 if res["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
