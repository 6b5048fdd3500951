#!/usr/bin/env python3
"""What bsa_cigar_windows_run costs beside the align step it follows, at C2, device-resident (one process, one GPU).

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring, windows of 500 target
bases.  After a warm-up, `reps` rounds; every round times, each between two synchronisations and one after the other (interleaved, so that
all of them see the same device state):
  - the plain align step (bsa_align_run);
  - the step followed by the pass (bsa_align_run, bsa_cigar_windows_run);
  - the pass alone, on the records and words the step left;
  - a step with BSA_MODE_BAND_MARGIN, for bsa_ctx_last_margin_ms: the margin pass reads the same words, one wave a pair;
  - the device-to-host copy of the CIGAR arena, and that of the windows, into pinned memory: what the host route pays and what this one does.
The JSON line has the median of each over the rounds, the sizes, and whether the windows of the first pairs equal the Python statement of the
definition (tests/cigar_windows_cases.windows_ref).

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 600 python tools/bench_cigar_windows.py --out profiles/cigar_windows_bench_line.json && ...
Prints ONE JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20240611


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=100000)
    ap.add_argument("length", type=int, nargs="?", default=10000)
    ap.add_argument("window", type=int, nargs="?", default=500)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--check", type=int, default=16, help="pairs whose windows are compared with the Python reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import cigar_windows_cases as W
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = B.lib()
    n, L, w = args.pairs, args.length, args.window
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
    win_cap = B.cigar_windows_bound(tlen, w)
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(cig_cap, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    d_win = torch.zeros(max(win_cap, 1) * 4, dtype=torch.int32, device=dev)
    d_woff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    sc = (2, -6, -3, -2, 0, 0)
    plain = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL, args.bw, *sc))
    flagged = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL | B.MODE_BAND_MARGIN, args.bw, *sc))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def step():
        plain.run(d_seqs, d_out, d_cig, d_off, d_st)

    def windows():
        ctx.cigar_windows_run(d_out, d_cig, d_off, n, w, d_win, win_cap, d_woff)

    def both():
        step()
        windows()

    def flagged_step():
        flagged.run(d_seqs, d_out, d_cig, d_off, d_st)

    for _ in range(args.warmup):
        timed(both)
        timed(flagged_step)
    words, records = int(d_off.cpu().numpy()[n]), int(d_woff.cpu().numpy()[n])
    assert words <= cig_cap and records <= win_cap
    h_cig = torch.empty(max(words, 1), dtype=torch.int32).pin_memory()
    h_win = torch.empty(max(records, 1) * 4, dtype=torch.int32).pin_memory()
    t = {k: [] for k in ("step", "step_and_windows", "windows", "margin_pass", "flagged_step", "cigar_d2h", "windows_d2h")}
    for _ in range(args.reps):
        t["step"].append(timed(step))
        t["step_and_windows"].append(timed(both))
        t["windows"].append(timed(windows))
        t["flagged_step"].append(timed(flagged_step))
        t["margin_pass"].append(ctx.last_margin_ms()[0])
        t["cigar_d2h"].append(timed(lambda: h_cig[:words].copy_(d_cig[:words], non_blocking=True)))
        t["windows_d2h"].append(timed(lambda: h_win[:records * 4].copy_(d_win[:records * 4], non_blocking=True)))
    med = {k: round(float(np.median(v)), 3) for k, v in t.items()}
    # the first pairs against the definition
    timed(both)
    off, woff = d_off.cpu().numpy(), d_woff.cpu().numpy()
    out = d_out.cpu().numpy().reshape(n, 10)
    nchk = min(args.check, n)
    cig = d_cig[:int(off[nchk])].cpu().numpy().view(np.uint32)
    win = d_win[:int(woff[nchk]) * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)
    same = all(np.array_equal(win[int(woff[k]):int(woff[k + 1])], W.windows_ref(out[k], cig[int(off[k]):int(off[k + 1])], w)) for k in range(nchk))
    none = int((d_win[:records * 4].view(-1, 4)[:, 0] == -1).sum().item())
    res = {"config": {"pairs": n, "length": L, "window": w, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps, "warmup": args.warmup,
                      "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "pass_cost_percent_of_step": round(100.0 * (med["step_and_windows"] - med["step"]) / med["step"], 2) if med["step"] else None,
           "cigar_words": words, "cigar_words_per_pair": round(words / max(n, 1), 1), "cigar_bytes": 4 * words,
           "window_records": records, "window_records_per_pair": round(records / max(n, 1), 2), "window_bytes": 16 * records, "records_none": none,
           "checked_pairs": nchk, "identical": bool(same), "flagged_pairs": int((d_st.cpu().numpy() & 0xFFFF != 0).sum())}
    plain.close()
    flagged.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
