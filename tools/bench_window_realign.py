#!/usr/bin/env python3
"""What bsa_window_realign_run costs at C2's shape, device-resident (one process, one GPU), against what it is to be judged by: the passes of the
round it opens (bsa_window_msa_run, bsa_window_cns_run, bsa_window_stitch_run on the re-aligned pieces) beside their round-1 times in the same
process, and the copy to pinned host memory of what the host route would need (piece records, codes, the stitched sequence and its words).

C2 as in tools/bench_window_stitch.py: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default
scoring, windows of 500 target bases, `--depth` pairs in a row on one draft, vote 0.  One align step and the passes of round 1 leave every window's
stitched sequence and words on the device; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see
the same device state):
  - bsa_window_msa_run, bsa_window_cns_run (without its compaction) and bsa_window_stitch_run of round 1, each alone between two synchronisations;
  - the pass (bsa_window_realign_run, window2 `--window2`, max_len `--max-len`, the arena of the words it needs), alone between two synchronisations;
  - each of the pass's four steps (the lift; the DP with its traceback; the scan; the fill) alone, launched once more in order on what the pass left,
    between two events;
  - the three passes of round 2 on what the pass left, each alone between two synchronisations;
  - the piece records, the codes, the stitched sequence and its words to pinned host memory, between two synchronisations.
The JSON line has median, min and max of each over the rounds, the sizes, the statuses, the DP kernel's cells per second (64 cells a row of every
piece that reached the DP), and whether the first windows equal the Python statement of the definition
(tests/window_realign_cases.window_realign_ref).

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 900 python tools/bench_window_realign.py 100000 10000 500 7 --out profiles/window_realign_bench_line.json && ...
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
STEPS = ("lift", "dp", "scan", "fill")


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
    ap.add_argument("--window2", type=int, default=640, help="round 2's window size: a window's stitched sequence is at most that long")
    ap.add_argument("--max-len", type=int, default=640)
    ap.add_argument("--min-margin", type=int, default=8)
    ap.add_argument("--check", type=int, default=16, help="windows compared with the Python reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import window_cns_cases as WC
    import window_realign_cases as R
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())                 # a stream of its own: the events below are recorded on the stream the library launches on
    stream = torch.cuda.current_stream().cuda_stream
    assert stream
    ctx.set_stream(stream)
    lib = B.lib()
    n, L, w, depth, min_cov, w2 = args.pairs, args.length, args.window, max(args.depth, 1), args.min_cov, args.window2
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

    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    ctx.window_pieces_run(d_seqs, d_qoff, d_qlen, d_win, d_woff, n, w, d_gbase, nwin, 0, d_piece, piece_cap, d_poff, d_bases, bases_cap, d_boff)
    ctx.piece_cigars_run(d_out, d_cig, d_off, n, d_piece, d_poff[nwin:], piece_cap, d_pcig, pcig_cap, d_pcoff, d_pst)
    torch.cuda.synchronize()
    npieces = int(d_poff.cpu().numpy()[nwin])
    assert npieces <= piece_cap
    doff, dlen = B.window_drafts(toff[::depth], tlen[::depth], w)
    assert len(doff) == nwin
    d_doff = torch.from_numpy(doff.view(np.int64)).to(dev)
    d_dlen = torch.from_numpy(dlen.view(np.int32)).to(dev)
    model = ctx.cns_model(WC.PAR7)

    class Round:
        """the MSA, the consensus without its compaction and the stitch of one round, on buffers of their own"""

        def __init__(self, d_piece, d_pcig, pcig_cap, d_pcoff, d_draft, d_doff, d_dlen, window):
            self.a = (d_piece, d_pcig, pcig_cap, d_pcoff, d_draft, d_doff, d_dlen, window)
            self.d_coff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
            self.d_cwin = torch.zeros(max(nwin, 1) * 5, dtype=torch.int64, device=dev)
            self.d_cols, self.need = None, 0
            timed(self.msa)                                    # count only: what the columns take
            self.need = int(self.d_coff.cpu().numpy()[nwin])
            assert self.need > 0
            self.d_cols = torch.zeros(self.need, dtype=torch.uint8, device=dev)
            timed(self.msa)
            self.cwin = self.d_cwin.cpu().numpy().view(B.CNS_WINDOW_DTYPE)[:nwin].copy()
            self.out_cap, self.max_rows = int(self.cwin["mlen"].astype(np.int64).sum()), int(self.cwin["nseq"].max())
            self.d_cns, self.d_qlt, self.d_alt, self.d_seq, self.d_sq = (torch.zeros(max(self.out_cap, 1), dtype=torch.uint8, device=dev) for _ in range(5))
            self.d_clen, self.d_status = torch.zeros(nwin, dtype=torch.int32, device=dev), torch.zeros(nwin, dtype=torch.int32, device=dev)
            self.d_soff, self.d_goff = (torch.zeros(nwin + 1, dtype=torch.int64, device=dev) for _ in range(2))
            self.d_words = torch.zeros(max(self.out_cap, 1), dtype=torch.int32, device=dev)
            self.d_rec = torch.zeros(nwin * 8, dtype=torch.int32, device=dev)
            timed(self.cns)
            timed(self.stitch)

        def msa(self):
            d_pc, d_g, gcap, d_goff, d_draft, d_do, d_dl, window = self.a
            ctx.window_msa_run(d_pc, d_poff, nwin, piece_cap, d_bases, bases_cap, d_g, gcap, d_goff, d_draft, d_do, d_dl, window, 0, 0, self.d_cols, self.need, self.d_coff, self.d_cwin)

        def cns(self):
            ctx.window_cns_run(model, self.d_cols, self.need, self.d_cwin, nwin, self.max_rows, self.d_cns, self.d_qlt, self.d_alt, self.out_cap, self.d_clen, None, self.d_status)

        def stitch(self):
            ctx.window_stitch_run(self.d_cols, self.need, self.d_cwin, nwin, self.d_status, min_cov, self.d_seq, self.d_sq, None, self.out_cap, self.d_soff, self.d_words, self.out_cap,
                                  self.d_goff, self.d_rec)

    one = Round(d_piece, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w)
    assert not one.d_status.cpu().numpy().any(), "a window of the MSA pass's own output was dead"
    par = B.realign_params(w2, args.max_len, args.min_margin, 1, 1)
    d_p2 = torch.zeros(max(piece_cap, 1) * 4, dtype=torch.int64, device=dev)
    d_off2 = torch.zeros(piece_cap + 1, dtype=torch.int64, device=dev)
    d_st2, d_cost = torch.zeros(max(piece_cap, 1), dtype=torch.int32, device=dev), torch.zeros(max(piece_cap, 1), dtype=torch.int32, device=dev)
    d_doff2, d_dlen2 = torch.zeros(nwin, dtype=torch.int64, device=dev), torch.zeros(nwin, dtype=torch.int32, device=dev)
    state = {"words": None, "cap": 0}

    def realign_args():
        return (p(d_piece), p(d_poff), nwin, piece_cap, p(d_bases), bases_cap, w, p(one.d_seq), one.out_cap, p(one.d_soff), p(one.d_words), one.out_cap, p(one.d_goff), C.byref(par),
                p(d_p2), p(state["words"]), state["cap"], p(d_off2), p(d_st2), p(d_cost), p(d_doff2), p(d_dlen2))

    def realign():
        assert lib.bsa_window_realign_run(ctx.h, *realign_args()) == 0, lib.bsa_last_error(ctx.h)

    def step(i):
        def fn():
            assert lib.bsa_window_realign_step_internal(ctx.h, i, *realign_args()) == 0
        return fn

    timed(realign)                                             # count only: what the words take
    words2 = int(d_off2.cpu().numpy()[piece_cap])
    assert words2 > 0
    state["words"], state["cap"] = torch.zeros(words2, dtype=torch.int32, device=dev), words2
    timed(realign)
    two = Round(d_p2, state["words"], words2, d_off2, one.d_seq, d_doff2, d_dlen2, w2)
    h = [torch.empty(t.numel(), dtype=t.dtype).pin_memory() for t in (d_piece, d_bases, one.d_seq, one.d_words, one.d_soff, one.d_goff)]

    def to_host():
        for dst, src in zip(h, (d_piece, d_bases, one.d_seq, one.d_words, one.d_soff, one.d_goff)):
            dst.copy_(src, non_blocking=True)

    rounds = (("window_msa", timed, one.msa), ("window_cns", timed, one.cns), ("window_stitch", timed, one.stitch), ("pass", timed, realign)) \
        + tuple((s + "_step", by_events, step(i)) for i, s in enumerate(STEPS)) \
        + (("window_msa_round2", timed, two.msa), ("window_cns_round2", timed, two.cns), ("window_stitch_round2", timed, two.stitch), ("inputs_d2h", timed, to_host))
    for _ in range(args.warmup):
        for _, how, fn in rounds:
            how(fn)
    t = {k: [] for k, _, _ in rounds}
    for _ in range(args.reps):
        for k, how, fn in rounds:
            t[k].append(how(fn))
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the first windows against the definition, on the arrays as they lie on the device
    timed(realign)
    st2 = d_st2.cpu().numpy().view(np.uint32)[:piece_cap]
    piece = d_piece.cpu().numpy().view(B.PIECE_DTYPE)[:piece_cap]
    poff = d_poff.cpu().numpy().view(np.uint64)
    soff, goff = one.d_soff.cpu().numpy().view(np.uint64), one.d_goff.cpu().numpy().view(np.uint64)
    off2 = d_off2.cpu().numpy().view(np.uint64)
    reached = (st2[:npieces] & 0xFF == 0) | (st2[:npieces] == R.ST_NO_DIAG)
    cells = 64 * int(piece["len"][:npieces][reached].astype(np.int64).sum())
    nchk = min(args.check, nwin)
    pend = int(poff[nchk])
    bend = int((piece["base_off"][:pend] + piece["len"][:pend]).max()) if pend else 0
    rb = R.RBatch(piece[:pend], poff[:nchk + 1], d_bases[:bend].cpu().numpy(), w, one.d_seq[:int(soff[nchk])].cpu().numpy(), soff[:nchk + 1],
                  one.d_words[:int(goff[nchk])].cpu().numpy().view(np.uint32), goff[:nchk + 1])
    wend = int(off2[pend])
    ref = R.window_realign_ref(rb, dict(window2=w2, max_len=args.max_len, min_margin=args.min_margin, x=1, g=1), wend)
    p2 = d_p2.cpu().numpy().view(B.PIECE_DTYPE)[:pend]
    same = bool(all(np.array_equal(p2[k], ref.piece2[k]) for k in B.PIECE_DTYPE.names) and np.array_equal(st2[:pend], ref.pstatus)
                and np.array_equal(d_cost[:pend].cpu().numpy().view(np.uint32), ref.cost) and np.array_equal(off2[:pend + 1], ref.pcig2_off)
                and np.array_equal(state["words"][:wend].cpu().numpy().view(np.uint32), ref.pcig2)
                and np.array_equal(d_doff2[:nchk].cpu().numpy().view(np.uint64), ref.doff2) and np.array_equal(d_dlen2[:nchk].cpu().numpy().view(np.uint32), ref.dlen2))
    names = ("ok", "no_window", "bad_piece", "too_long", "empty_span", "off_band", "no_diag")
    statuses = {names[k]: int((st2[:npieces] & 0xFF == k).sum()) for k in range(7)}
    statuses["edge"] = int((st2[:npieces] == R.ST_EDGE).sum())
    rec1, rec2 = one.d_rec.cpu().numpy().view(B.STITCH_DTYPE)[:nwin], two.d_rec.cpu().numpy().view(B.STITCH_DTYPE)[:nwin]
    tot = lambda rec: {k: int(rec[k].astype(np.int64).sum()) for k in ("slen", "eq", "x", "ins", "del", "kept")}
    slot = (2 * args.max_len + 63 + 15) // 16 * 4
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "min_cov": min_cov, "vote": 0, "window2": w2, "max_len": args.max_len, "min_margin": args.min_margin, "x": 1, "g": 1,
                      "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "statuses": statuses, "words_round2": words2, "cols_bytes": one.need, "cols_bytes_round2": two.need,
           "columns": one.out_cap, "columns_round2": two.out_cap, "scratch_bytes": piece_cap * (20 + slot), "dp_cells": cells,
           "dp_Gcells_per_s": round(cells / med["dp_step"] / 1e6, 2) if med["dp_step"] else None,
           "host_route_bytes": int(sum(x.numel() * x.element_size() for x in h)),
           "pass_over_window_msa": round(med["pass"] / med["window_msa"], 3) if med["window_msa"] else None,
           "pass_over_window_cns": round(med["pass"] / med["window_cns"], 3) if med["window_cns"] else None,
           "stitch_totals_round1": tot(rec1), "stitch_totals_round2": tot(rec2), "checked_windows": nchk, "identical": same}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
