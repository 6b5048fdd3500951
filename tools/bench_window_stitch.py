#!/usr/bin/env python3
"""What bsa_window_stitch_run costs at C2's shape, device-resident (one process, one GPU), against what it is to be judged by: a device-to-device copy
of the column bytes it reads, the consensus pass's pack step that a caller of this pass skips, and the MSA's copy to pinned host memory -- the route
the pass replaces for anyone who wants the differences to the draft.

C2 as in tools/bench_window_cns.py: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default
scoring, windows of 500 target bases, `--depth` pairs in a row on one draft, vote 0.  One align step and the five passes leave every window's MSA
with its consensus bytes on the device; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see the
same device state):
  - bsa_cigar_windows_run, bsa_window_pieces_run, bsa_piece_cigars_run, bsa_window_msa_run, bsa_window_cns_run (without its compaction) and the
    pass (bsa_window_stitch_run, min_cov `--min-cov`, both caps the sum of mlen), each alone between two synchronisations;
  - each of the pass's three steps (prepare with its scan; the columns with the two scans; the fill) alone, launched once more on what the pass
    left, between two events;
  - a device-to-device copy of the column bytes, between two events;
  - the consensus pass's pack step (its scan and k_window_cns_pack) behind a run of that pass, between two events;
  - the columns and records to pinned host memory, between two synchronisations.
The JSON line has median, min and max of each over the rounds, the sizes, the totals eq, x, ins, del, kept over all windows, and whether the first
windows equal the Python statement of the definition (tests/window_stitch_cases.window_stitch_ref).

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 900 python tools/bench_window_stitch.py 100000 10000 500 7 --out profiles/window_stitch_bench_line.json && ...
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
STEPS = ("prepare", "cols", "fill")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=100000)
    ap.add_argument("length", type=int, nargs="?", default=10000)
    ap.add_argument("window", type=int, nargs="?", default=500)
    ap.add_argument("reps", type=int, nargs="?", default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--depth", type=int, default=40, help="pairs in a row that share a draft: the pieces a window holds")
    ap.add_argument("--min-cov", type=int, default=1)
    ap.add_argument("--check", type=int, default=16, help="windows compared with the Python reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import window_cns_cases as WC
    import window_stitch_cases as WS
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
    d_cns, d_qlt, d_alt, d_seq, d_sq, d_sa, d_pseq, d_psq, d_psa = (torch.zeros(max(out_cap, 1), dtype=torch.uint8, device=dev) for _ in range(9))
    d_clen = torch.zeros(nwin, dtype=torch.int32, device=dev)
    d_status = torch.zeros(nwin, dtype=torch.int32, device=dev)
    d_soff, d_psoff, d_goff = (torch.zeros(nwin + 1, dtype=torch.int64, device=dev) for _ in range(3))
    d_words = torch.zeros(max(out_cap, 1), dtype=torch.int32, device=dev)
    d_rec = torch.zeros(nwin * 8, dtype=torch.int32, device=dev)

    def cns():                                                 # as a caller of the stitch runs it: no compaction
        ctx.window_cns_run(model, d_cols, need, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, None, d_status)

    cns_args = lambda: (model.h, p(d_cols), need, p(d_cwin), nwin, max_rows, p(d_cns), p(d_qlt), p(d_alt), out_cap, p(d_clen), None, p(d_status), p(d_pseq), p(d_psq), p(d_psa),
                        out_cap, p(d_psoff))

    def cns_pack_step():
        """the pack step alone, on the scratch a run of the consensus pass has just left (this pass uses the same scratch)"""
        assert lib.bsa_window_cns_step_internal(ctx.h, 0, *cns_args()) == 0            # the records again: a few microseconds, not timed
        return by_events(lambda: lib.bsa_window_cns_step_internal(ctx.h, 3, *cns_args()))

    def stitch():
        ctx.window_stitch_run(d_cols, need, d_cwin, nwin, d_status, min_cov, d_seq, d_sq, d_sa, out_cap, d_soff, d_words, out_cap, d_goff, d_rec)

    def step(i):
        def fn():
            assert lib.bsa_window_stitch_step_internal(ctx.h, i, p(d_cols), need, p(d_cwin), nwin, p(d_status), min_cov, p(d_seq), p(d_sq), p(d_sa), out_cap, p(d_soff),
                                                       p(d_words), out_cap, p(d_goff), p(d_rec)) == 0
        return fn

    timed(cns)
    status = d_status.cpu().numpy()
    assert not status.any(), "a window of the MSA pass's own output was dead"
    timed(stitch)
    d_copy = torch.empty(need, dtype=torch.uint8, device=dev)
    h_cols = torch.empty(need, dtype=torch.uint8).pin_memory()
    h_cwin = torch.empty(max(nwin, 1) * 5, dtype=torch.int64).pin_memory()

    def cols_copy():
        d_copy.copy_(d_cols, non_blocking=True)

    def msa_to_host():
        h_cols.copy_(d_cols, non_blocking=True)
        h_cwin.copy_(d_cwin, non_blocking=True)

    direct = lambda fn: fn()
    rounds = (("cigar_windows", timed, windows), ("window_pieces", timed, pieces), ("piece_cigars", timed, cigars), ("window_msa", timed, msa), ("window_cns", timed, cns),
              ("cns_pack_step", direct, cns_pack_step), ("pass", timed, stitch)) \
        + tuple((s + "_step", by_events, step(i)) for i, s in enumerate(STEPS)) \
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
    timed(stitch)
    rec = d_rec.cpu().numpy().view(B.STITCH_DTYPE)[:nwin]
    soff, goff = d_soff.cpu().numpy().view(np.uint64), d_goff.cpu().numpy().view(np.uint64)
    seq_bytes, words = int(soff[nwin]), int(goff[nwin])
    assert 0 < seq_bytes <= out_cap and 0 < words <= out_cap
    nchk = min(args.check, nwin)
    cend = int(cwin[nchk - 1]["cols_off"]) + int(cwin[nchk - 1]["mlen"]) * (int(cwin[nchk - 1]["nall"]) + 3)
    send, gend = int(soff[nchk]), int(goff[nchk])
    ref = WS.window_stitch_ref(d_cols[:cend].cpu().numpy(), cwin[:nchk], cend, status[:nchk], min_cov, send, gend)
    same = bool(np.array_equal(ref.rec, rec[:nchk]) and np.array_equal(ref.seq_off, soff[:nchk + 1]) and np.array_equal(ref.cig_off, goff[:nchk + 1])
                and np.array_equal(ref.seq, d_seq[:send].cpu().numpy()) and np.array_equal(ref.seq_qlt, d_sq[:send].cpu().numpy())
                and np.array_equal(ref.seq_alt, d_sa[:send].cpu().numpy()) and np.array_equal(ref.cig, d_words[:gend].cpu().numpy().view(np.uint32)))
    total = {k: int(rec[k].astype(np.int64).sum()) for k in ("eq", "x", "ins", "del", "kept")}
    clen_sum = int(d_clen.cpu().numpy().view(np.uint32).astype(np.int64).sum())
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "min_cov": min_cov, "vote": 0, "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "cols_bytes": need, "columns": out_cap, "max_rows": max_rows, "seq_bytes": seq_bytes, "words": words,
           "consensus_clen_sum": clen_sum, "totals": total, "scratch_bytes": 44 * nwin + 4 * min(need // 4, out_cap),
           "result_bytes": 3 * seq_bytes + 4 * words + 16 * (nwin + 1) + 32 * nwin,
           "mlen_mean": round(float(cwin["mlen"].mean()), 1), "slen_mean": round(float(rec["slen"].mean()), 1), "ncig_mean": round(float(rec["ncig"].mean()), 1),
           "cols_GBps": round(need / med["pass"] / 1e6, 1) if med["pass"] else None,
           "pass_over_cols_copy": round(med["pass"] / med["cols_copy_d2d"], 3) if med["cols_copy_d2d"] else None,
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
