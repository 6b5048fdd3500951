#!/usr/bin/env python3
"""What BSA_MODE_BAND_MARGIN costs and what it tells, at C2, device-resident (one process, one GPU).

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, default scoring.  At bandwidth 128 and again at 64, on
the same pairs: the plain plan and the plan with the flag, each `--warmup` steps and then `--steps` steps timed one by one between two
synchronisations (as bench.py times its step), so the flagged step is compared with the plain step of the same process.  Per bandwidth the JSON
line has both medians, the pass's own kernel time (HIP events around its launches: bsa_ctx_last_margin_ms), whether records, CIGAR words,
offsets and the low status half are identical, the histogram of the margins (by eighths of the band) and the two shares a user picks a
bandwidth by: pairs with margin 0 -- the path ran on an edge of its band -- and pairs with a margin of at most 8.

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 600 python tools/bench_band_margin.py && ...
Prints ONE JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20240611


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--bw", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = B.lib()
    n, L = args.pairs, args.length
    stride = lib.bsa_synth_stride(L)
    d_seqs = torch.zeros(2 * n * stride, dtype=torch.uint8, device=dev)
    d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    torch.cuda.synchronize()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
    cig_cap = n * max(L // 4, 64)
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(cig_cap, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    res = {"config": {"pairs": n, "length": L, "scoring": "2,-6,-3,-2,0,0", "steps": args.steps, "warmup": args.warmup,
                      "library": os.path.relpath(B.LIB_PATH, ROOT)}, "bandwidths": {}}

    def measure(flags, bw):
        plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL | flags, bw, 2, -6, -3, -2, 0, 0))

        def step():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan.run(d_seqs, d_out, d_cig, d_off, d_st)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(args.warmup):
            step()
        ms = [step() for _ in range(args.steps)]
        kms, _, _ = ctx.last_kernel_ms()
        tms, _ = ctx.last_trace_ms()
        mms, mlaunches = ctx.last_margin_ms()
        off = d_off.cpu().numpy()
        outs = (d_out.cpu().numpy().reshape(n, 10), off, d_cig[:int(off[n])].cpu().numpy().view(np.uint32), d_st.cpu().numpy().view(np.uint32))
        plan.close()
        med = float(np.median(ms))
        return {"ms_per_step": round(med, 3), "steps_ms": [round(x, 3) for x in ms], "forward_ms": round(kms, 3), "traceback_ms": round(tms, 3),
                "margin_pass_ms": round(mms, 3), "margin_pass_launches": int(mlaunches), "forward_kernel": ctx.last_kernel_names()[0]}, outs

    ok = True
    for bw in args.bw:
        plain, po = measure(0, bw)
        flagged, fo = measure(B.MODE_BAND_MARGIN, bw)
        same = bool(np.array_equal(po[0], fo[0]) and np.array_equal(po[1], fo[1]) and np.array_equal(po[2], fo[2])
                    and np.array_equal(po[3], fo[3] & np.uint32(0xFFFF)) and not (po[3] >> np.uint32(16)).any())
        ok = ok and same
        m = (fo[3] >> np.uint32(B.ST_MARGIN_SHIFT)).astype(np.int64)
        have = m != B.ST_MARGIN_NONE
        eighth = max(bw // 8, 1)
        hist = {"%d-%d" % (k * eighth, (k + 1) * eighth - 1): int(((m >= k * eighth) & (m < (k + 1) * eighth) & have).sum()) for k in range(8)}
        hist[">=%d" % (8 * eighth)] = int(((m >= 8 * eighth) & have).sum())
        hist["none"] = int((~have).sum())
        res["bandwidths"][str(bw)] = {
            "plain": plain, "flagged": flagged, "identical": same,
            "step_cost_percent": round(100.0 * (flagged["ms_per_step"] - plain["ms_per_step"]) / plain["ms_per_step"], 2),
            "margin_histogram": hist,
            "share_margin_0": round(float((m == 0).sum()) / n, 5), "share_margin_le_8": round(float(((m <= 8) & have).sum()) / n, 5),
            "flagged_pairs": int((po[3] != 0).sum()),
        }
    res["identical"] = ok
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
