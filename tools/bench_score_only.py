#!/usr/bin/env python3
"""Score-only against full alignment on the same device-resident batch (one process, one GPU).

Default: C2's shape -- 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring --
once with BSA_MODE_SCORE_ONLY and once without, plus one overlap-mode line.  Each path: a plan, `--warmup` runs, then `--steps` runs of
plan.run between two synchronisations, timed on the host clock as bench.py times its step.  Prints ONE JSON line: ms per step, GCUPS, the
forward kernel's own time and the workspace of both paths, and whether score, qe and te agree on every pair.

--workload edit: the edit aligner (bsa_edit_plan_create / bsa_edit_run).  Default: C3's shape -- 32 768 pairs of 100 kbp, global, bandwidth
256, bench.py's synthetic pairs and seed -- plus one extend-mode line on whole-read bands (4 096 pairs of 10 kbp, bandwidth 0)."""
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
    ap.add_argument("--workload", default="align8", choices=["align8", "edit"])
    ap.add_argument("--pairs", type=int, default=0, help="default: 100 000 (align8), 32 768 (edit)")
    ap.add_argument("--length", type=int, default=0, help="default: 10 000 (align8), 100 000 (edit)")
    ap.add_argument("--bw", type=int, default=-1, help="default: 128 (align8), 256 (edit)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--overlap-pairs", type=int, default=20000, help="align8: pairs of the overlap-mode line (0: none)")
    ap.add_argument("--extend-pairs", type=int, default=4096, help="edit: pairs of the extend-mode line, bandwidth 0 (0: none)")
    ap.add_argument("--extend-length", type=int, default=10000, help="edit: read length of the extend-mode line")
    ap.add_argument("--score-only-run", action="store_true", help="only the score-only global line, no comparison (for a kernel trace of that path alone)")
    args = ap.parse_args()
    edit = args.workload == "edit"
    args.pairs = args.pairs or (32768 if edit else 100000)
    args.length = args.length or (100000 if edit else 10000)
    args.bw = args.bw if args.bw >= 0 else (256 if edit else 128)
    if edit:
        return main_edit(args)
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = B.lib()
    n, L = args.pairs, args.length
    stride = lib.bsa_synth_stride(L)
    d_seqs = torch.empty(2 * n * stride, dtype=torch.uint8, device=dev)
    d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
    assert lib.bsa_synth_pairs_dev(ctx.h, SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    torch.cuda.synchronize()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)

    def slot_bytes(score_only, mode, m):
        # workspace of the plan's slots (bsa_common.h: bsa_score_rec_bytes, bsa_code_slot_bytes; slots start at multiples of 256 bytes)
        up = lambda b: (b + 255) & ~255
        if score_only:
            rec = 4 if mode == B.MODE_GLOBAL else 200 + args.bw
            return m * up(rec)
        begs = up((L + 2) * 4)
        rows = (L + 3) // 4 * 4 + 7
        return m * up(begs + rows * 64 * max(1, args.bw // 128))

    def run(mode, score_only, m):
        par = B.make_params(mode, args.bw, 2, -6, -3, -2, 0, 0)
        if score_only:
            par.mode |= B.MODE_SCORE_ONLY
        plan = B.AlignPlan(ctx, qoff[:m], qlen[:m], toff[:m], tlen[:m], par)
        cells = plan.cells()
        d_out = torch.zeros(m * 10, dtype=torch.int32, device=dev)
        d_st = torch.zeros(m, dtype=torch.int32, device=dev)
        d_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        d_cig = None if score_only else torch.empty(m * max(L // 4, 64), dtype=torch.int32, device=dev)
        for _ in range(args.warmup):
            plan.run(d_seqs, d_out, d_cig, d_off, d_st)
        ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            plan.run(d_seqs, d_out, d_cig, d_off, d_st)
        ctx.sync()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        fwd_ms, launches, _ = ctx.last_kernel_ms()
        names = ctx.last_kernel_names()
        out = d_out.cpu().numpy().view(B.RESULT_DTYPE).reshape(m)
        st = d_st.cpu().numpy()
        plan.close()
        del d_cig
        torch.cuda.empty_cache()
        return out, st, {"ms_per_step": round(ms, 3), "gcups": round(cells / (ms * 1e-3) / 1e9, 1), "forward_ms": round(fwd_ms, 3),
                         "forward_launches": launches, "workspace_bytes": slot_bytes(score_only, mode, m), "forward_kernel": names[0], "finish_kernel": names[1],
                         "flagged": int((st != 0).sum())}

    res = {"config": {"pairs": n, "length": L, "bandwidth": args.bw, "scoring": "2,-6,-3,-2,0,0", "steps": args.steps, "warmup": args.warmup}}
    if args.score_only_run:
        _, _, res["global"] = run(B.MODE_GLOBAL, True, n)
        print(json.dumps(res))
        ctx.close()
        return 0
    for mode, m, key in ((B.MODE_GLOBAL, n, "global"), (B.MODE_OVERLAP, min(args.overlap_pairs, n), "overlap")):
        if m == 0:
            continue
        fo, fs, full = run(mode, False, m)
        so, ss, score = run(mode, True, m)
        same = all(np.array_equal(so[f], fo[f]) for f in ("score", "qe", "te")) and np.array_equal(ss, fs)
        minus = all((so[f] == -1).all() for f in ("qb", "tb", "mat", "mis", "ins", "del", "aln"))
        res[key] = {"pairs": m, "full": full, "score_only": score, "scores_identical": bool(same), "trace_fields_minus_one": bool(minus),
                    "step_saving": round(1.0 - score["ms_per_step"] / full["ms_per_step"], 4)}
    res["scores_identical"] = all(res[k]["scores_identical"] for k in ("global", "overlap") if k in res)
    print(json.dumps(res))
    ctx.close()
    return 0 if res["scores_identical"] else 1


def edit_bw_eff(qlen, tlen, mode, bandwidth):
    """bsa_edit_bw_eff (csrc/bsa_common.h): the effective band of one edit pair"""
    qround = (qlen + 63) // 64 * 64
    if mode != 0:
        return qround
    bw = (bandwidth + 63) // 64 * 64
    if bw == 0 or bw > qlen:
        bw = qround
    if bw < qlen:
        step = (qlen + tlen - 1) // tlen + 1
        if bw < step:
            bw = (step + 63) // 64 * 64
    return bw


def main_edit(args):
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = B.lib()

    def synth(n, L):
        stride = lib.bsa_synth_stride(L)
        d_seqs = torch.empty(2 * n * stride, dtype=torch.uint8, device=dev)
        d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
        assert lib.bsa_synth_pairs_dev(ctx.h, SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
        torch.cuda.synchronize()
        qlen = d_qlen.cpu().numpy().astype(np.uint32)
        tlen = np.full(n, L, dtype=np.uint32)
        toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
        return d_seqs, qoff, qlen, toff, tlen

    def slot_bytes(score_only, mode, bw, qlen, tlen):
        # workspace of the plan's slots (bsa_edit_plan_create: (tlen + 1 + 12 spare rows) x NW x 16 bytes a pair, score only one row -- two for
        # the generic kernel's pairs, moving bands above 1024 columns; slots start at multiples of 256 bytes)
        up = lambda b: (b + 255) & ~255
        tot = 0
        for q, t in zip(qlen.tolist(), tlen.tolist()):
            b = edit_bw_eff(q, t, mode, bw)
            nw = b // 64
            if score_only:
                gen = b > 1024 and (b != (q + 63) // 64 * 64 or nw > 512)
                tot += up((2 if gen else 1) * nw * 16)
            else:
                tot += up((t + 13) * nw * 16)
        return tot

    def run(data, mode, bw, score_only):
        d_seqs, qoff, qlen, toff, tlen = data
        m, L = len(qlen), int(tlen.max())
        plan = B.EditPlan(ctx, qoff, qlen, toff, tlen, mode | (B.MODE_SCORE_ONLY if score_only else 0), bw)
        cells = plan.cells()
        d_out = torch.zeros(m * 10, dtype=torch.int32, device=dev)
        d_st = torch.zeros(m, dtype=torch.int32, device=dev)
        d_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        d_cig = None if score_only else torch.empty(m * max(L // 4, 64), dtype=torch.int32, device=dev)      # (bench.py's arena)
        for _ in range(args.warmup):
            plan.run(d_seqs, d_out, d_cig, d_off, d_st)
        ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            plan.run(d_seqs, d_out, d_cig, d_off, d_st)
        ctx.sync()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        fwd_ms, launches, _ = ctx.last_kernel_ms()
        names = ctx.last_kernel_names()
        out = d_out.cpu().numpy().view(B.RESULT_DTYPE).reshape(m)
        st = d_st.cpu().numpy()
        plan.close()
        del d_cig
        torch.cuda.empty_cache()
        return out, st, {"ms_per_step": round(ms, 3), "gcups": round(cells / (ms * 1e-3) / 1e9, 1), "forward_ms": round(fwd_ms, 3),
                         "forward_launches": launches, "workspace_bytes": slot_bytes(score_only, mode, bw, qlen, tlen), "forward_kernel": names[0],
                         "finish_kernel": names[1], "flagged": int((st != 0).sum())}

    res = {"workload": "edit", "config": {"pairs": args.pairs, "length": args.length, "bandwidth": args.bw, "steps": args.steps, "warmup": args.warmup,
                                          "extend_pairs": args.extend_pairs, "extend_length": args.extend_length}}
    main_data = synth(args.pairs, args.length)
    if args.score_only_run:
        _, _, res["global"] = run(main_data, B.MODE_GLOBAL, args.bw, True)
        print(json.dumps(res))
        ctx.close()
        return 0
    lines = [("global", B.MODE_GLOBAL, args.bw, main_data)]
    if args.extend_pairs:
        lines.append(("extend", B.MODE_EXTEND, 0, None))
    for key, mode, bw, data in lines:
        if data is None:
            data = synth(args.extend_pairs, args.extend_length)
        fo, fs, full = run(data, mode, bw, False)
        so, ss, score = run(data, mode, bw, True)
        same = all(np.array_equal(so[f], fo[f]) for f in ("score", "qe", "te")) and np.array_equal(ss, fs)
        minus = all((so[f] == -1).all() for f in ("qb", "tb", "mat", "mis", "ins", "del", "aln"))
        res[key] = {"pairs": len(data[2]), "bandwidth": bw, "full": full, "score_only": score, "scores_identical": bool(same),
                    "trace_fields_minus_one": bool(minus), "step_saving": round(1.0 - score["ms_per_step"] / full["ms_per_step"], 4)}
    res["scores_identical"] = all(res[k]["scores_identical"] for k in ("global", "extend") if k in res)
    print(json.dumps(res))
    ctx.close()
    return 0 if res["scores_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
