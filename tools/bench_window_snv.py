#!/usr/bin/env python3
"""What bsa_window_snv_run costs at C2's shape, device-resident (one process, one GPU), against what it is to be judged by: a device-to-device copy
of the column bytes it reads, bsa_window_stitch_run (which reads the same bytes once), and the MSA's copy to pinned host memory -- the route the pass
replaces for anyone who wants the heterozygous sites.

C2 as in tools/bench_window_stitch.py: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default
scoring, windows of 500 target bases, `--depth` pairs in a row on one draft, vote 0.  One align step and the five passes leave every window's MSA
with its consensus bytes on the device; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see the
same device state):
  - the pass (bsa_window_snv_run, default parameters, snv_cap its own need) and bsa_window_stitch_run, each alone between two synchronisations;
  - each of the pass's three steps (prepare; the count -- both readings of the columns and the estimate -- with its scan; the fill) alone, launched
    once more on what the pass left, between two events;
  - a device-to-device copy of the column bytes, between two events;
  - the columns and records to pinned host memory, between two synchronisations.
The JSON line has median, min and max of each over the rounds, the sizes, the number of calls and sites, the distribution of the estimated rates,
and whether the first windows equal the Python statement of the definition (tests/snv_cases.snv_ref).  The synthetic pairs share no draft: the
number of calls is not a result.

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 900 python tools/bench_window_snv.py 100000 10000 500 7 --out profiles/window_snv_bench_line.json && ...
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
STEPS = ("prepare", "count", "fill")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=100000)
    ap.add_argument("length", type=int, nargs="?", default=10000)
    ap.add_argument("window", type=int, nargs="?", default=500)
    ap.add_argument("reps", type=int, nargs="?", default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--depth", type=int, default=40, help="pairs in a row that share a draft: the pieces a window holds")
    ap.add_argument("--min-cov", type=int, default=1, help="of the stitch pass beside it")
    ap.add_argument("--check", type=int, default=16, help="windows compared with the Python reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import window_cns_cases as WC
    import snv_cases as SC
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())                 # a stream of its own: the events below are recorded on the stream the library launches on
    stream = torch.cuda.current_stream().cuda_stream
    assert stream
    ctx.set_stream(stream)
    lib = B.lib()
    n, L, w, depth, min_cov = args.pairs, args.length, args.window, max(args.depth, 1), args.min_cov
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
    wpt = (L + w - 1) // w                                     # windows a draft
    gbase = (np.arange(n, dtype=np.uint64) // np.uint64(depth)) * np.uint64(wpt)
    nwin = int((n + depth - 1) // depth) * wpt
    cig_cap = n * max(L // 4, 64)
    win_cap = B.cigar_windows_bound(tlen, w)
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(cig_cap, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    d_win = torch.zeros(max(win_cap, 1) * 4, dtype=torch.int32, device=dev)
    d_woff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_qoff = torch.from_numpy(qoff.view(np.int64)).to(dev)
    d_gbase = torch.from_numpy(gbase.view(np.int64)).to(dev)
    sc = (2, -6, -3, -2, 0, 0)
    plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL, args.bw, *sc))
    plan.run(d_seqs, d_out, d_cig, d_off, d_st)
    ctx.cigar_windows_run(d_out, d_cig, d_off, n, w, d_win, win_cap, d_woff)
    torch.cuda.synchronize()
    plan.close()
    coff = d_off.cpu().numpy().view(np.uint64)
    assert int(coff[n]) <= cig_cap, "the align run was not complete"
    records = int(d_woff.cpu().numpy()[n])
    assert records <= win_cap
    piece_cap, bases_cap = records, int(qlen.astype(np.int64).sum())
    pcig_cap = B.piece_cigars_bound(coff, piece_cap)
    d_piece = torch.zeros(max(piece_cap, 1) * 4, dtype=torch.int64, device=dev)
    d_bases = torch.zeros(max(bases_cap, 1), dtype=torch.uint8, device=dev)
    d_poff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    d_boff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    d_pcig = torch.zeros(max(pcig_cap, 1), dtype=torch.int32, device=dev)
    d_pcoff = torch.zeros(piece_cap + 1, dtype=torch.int64, device=dev)
    d_pst = torch.zeros(max(piece_cap, 1), dtype=torch.int32, device=dev)
    d_np = d_poff[nwin:]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def by_events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def windows():
        ctx.cigar_windows_run(d_out, d_cig, d_off, n, w, d_win, win_cap, d_woff)

    def pieces():
        ctx.window_pieces_run(d_seqs, d_qoff, d_qlen, d_win, d_woff, n, w, d_gbase, nwin, 0, d_piece, piece_cap, d_poff, d_bases, bases_cap, d_boff)

    def cigars():
        ctx.piece_cigars_run(d_out, d_cig, d_off, n, d_piece, d_np, piece_cap, d_pcig, pcig_cap, d_pcoff, d_pst)

    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    doff, dlen = B.window_drafts(toff[::depth], tlen[::depth], w)
    assert len(doff) == nwin
    d_doff = torch.from_numpy(doff.view(np.int64)).to(dev)
    d_dlen = torch.from_numpy(dlen.view(np.int32)).to(dev)
    d_coff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    d_cwin = torch.zeros(max(nwin, 1) * 5, dtype=torch.int64, device=dev)
    timed(windows)
    timed(pieces)
    timed(cigars)
    npieces = int(d_poff.cpu().numpy()[nwin])
    assert npieces <= piece_cap
    state = {"cols": None, "cap": 0}

    def msa():
        ctx.window_msa_run(d_piece, d_poff, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w, 0, 0,
                           state["cols"], state["cap"], d_coff, d_cwin)

    timed(msa)                                                 # count only: what the columns take
    need = int(d_coff.cpu().numpy()[nwin])
    assert need > 0
    state["cols"], state["cap"] = torch.zeros(need, dtype=torch.uint8, device=dev), need
    d_cols = state["cols"]
    timed(msa)
    cwin = d_cwin.cpu().numpy().view(B.CNS_WINDOW_DTYPE)[:nwin].copy()
    out_cap, max_rows = int(cwin["mlen"].astype(np.int64).sum()), int(cwin["nseq"].max())
    model = ctx.cns_model(WC.PAR7)
    d_cns, d_qlt, d_alt, d_seq, d_sq, d_sa = (torch.zeros(max(out_cap, 1), dtype=torch.uint8, device=dev) for _ in range(6))
    d_clen = torch.zeros(nwin, dtype=torch.int32, device=dev)
    d_status = torch.zeros(nwin, dtype=torch.int32, device=dev)
    d_soff, d_goff = (torch.zeros(nwin + 1, dtype=torch.int64, device=dev) for _ in range(2))
    d_words = torch.zeros(max(out_cap, 1), dtype=torch.int32, device=dev)
    d_rec = torch.zeros(nwin * 8, dtype=torch.int32, device=dev)

    def cns():                                                 # as a caller of the stitch runs it: no compaction
        ctx.window_cns_run(model, d_cols, need, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, None, d_status)

    def stitch():
        ctx.window_stitch_run(d_cols, need, d_cwin, nwin, d_status, min_cov, d_seq, d_sq, d_sa, out_cap, d_soff, d_words, out_cap, d_goff, d_rec)

    timed(cns)
    status = d_status.cpu().numpy()
    assert not status.any(), "a window of the MSA pass's own output was dead"
    timed(stitch)
    snv_model = ctx.snv_model(max_rows)
    par = B.snv_params()
    d_snv_off = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    d_snv_rec = torch.zeros(nwin * 4, dtype=torch.int32, device=dev)
    snv_state = {"snv": None, "cap": 0}

    def snv():
        ctx.window_snv_run(snv_model, d_cols, need, d_cwin, nwin, d_status, par, snv_state["snv"], snv_state["cap"], d_snv_off, d_snv_rec)

    def snv_step(i):
        def fn():
            assert lib.bsa_window_snv_step_internal(ctx.h, i, snv_model.h, p(d_cols), need, p(d_cwin), nwin, p(d_status), B._p(par), p(snv_state["snv"]), snv_state["cap"],
                                                    p(d_snv_off), p(d_snv_rec)) == 0
        return fn

    timed(snv)                                                 # count only: what the records take
    snv_need = int(d_snv_off.cpu().numpy()[nwin])
    snv_state["snv"], snv_state["cap"] = torch.zeros(max(snv_need, 1) * 6, dtype=torch.int32, device=dev), snv_need
    timed(snv)
    d_copy = torch.empty(need, dtype=torch.uint8, device=dev)
    h_cols = torch.empty(need, dtype=torch.uint8).pin_memory()
    h_cwin = torch.empty(max(nwin, 1) * 5, dtype=torch.int64).pin_memory()

    def cols_copy():
        d_copy.copy_(d_cols, non_blocking=True)

    def msa_to_host():
        h_cols.copy_(d_cols, non_blocking=True)
        h_cwin.copy_(d_cwin, non_blocking=True)

    rounds = (("window_stitch", timed, stitch), ("pass", timed, snv)) \
        + tuple((k + "_step", by_events, snv_step(i)) for i, k in enumerate(STEPS)) \
        + (("cols_copy_d2d", by_events, cols_copy), ("msa_d2h", timed, msa_to_host))
    for _ in range(args.warmup):
        for _, how, fn in rounds:
            how(fn)
    t = {k: [] for k, _, _ in rounds}
    for _ in range(args.reps):
        for k, how, fn in rounds:
            t[k].append(how(fn))
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the first windows against the definition, on the columns as they lie on the device
    timed(snv)
    rec = d_snv_rec.cpu().numpy().view(B.SNV_WINDOW_DTYPE)[:nwin]
    off = d_snv_off.cpu().numpy().view(np.uint64)
    assert int(off[nwin]) == snv_need
    got = snv_state["snv"].cpu().numpy().view(B.SNV_DTYPE)[:snv_need]
    nchk = min(args.check, nwin)
    same = True
    for g in range(nchk):
        r = cwin[g]
        o, m, a = int(r["cols_off"]), int(r["mlen"]), int(r["nall"])
        ref, pexp, nsites, _ = SC.snv_ref(d_cols[o:o + m * (a + 3)].cpu().numpy().reshape(m, a + 3), a, int(r["nseq"]), par)
        same = same and got[int(off[g]):int(off[g + 1])].tobytes() == ref.tobytes() and rec[g].tolist() == (0, len(ref), nsites, float(pexp))
    rates, counts = np.unique(rec["pexp"], return_counts=True)
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "vote": 0, "snv_params": [int(par[0][0]), float(par[0][1]), int(par[0][2]), int(par[0][3])],
                      "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "cols_bytes": need, "columns": out_cap, "max_rows": max_rows, "calls": snv_need,
           "sites": int(rec["nsites"].astype(np.int64).sum()), "windows_with_calls": int((rec["nsnv"] > 0).sum()),
           "rates": {"%.4f" % float(x): int(c) for x, c in zip(rates, counts)}, "scratch_bytes": 32 * nwin,
           "result_bytes": 24 * snv_need + 8 * (nwin + 1) + 16 * nwin, "mlen_mean": round(float(cwin["mlen"].mean()), 1),
           "cols_GBps": round(need / med["pass"] / 1e6, 1) if med["pass"] else None,
           "pass_over_cols_copy": round(med["pass"] / med["cols_copy_d2d"], 3) if med["cols_copy_d2d"] else None,
           "pass_over_stitch": round(med["pass"] / med["window_stitch"], 3) if med["window_stitch"] else None,
           "checked_windows": nchk, "identical": same}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
