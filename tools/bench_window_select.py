#!/usr/bin/env python3
"""What bsa_window_select_run costs at C2's shape, device-resident (one process, one GPU), what it is to be judged by, and what it buys the passes
behind it.

C2 as in tools/bench_window_stitch.py: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default
scoring, windows of 500 target bases, `--depth` pairs in a row on one draft, vote 0.  One align step, bsa_cigar_windows_run and
bsa_window_pieces_run leave every window's pieces on the device; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so
that all of them see the same device state):
  - the pass (bsa_window_select_run, sel_cap = piece_cap, with d_sel_src and d_ncand) at max_depth 0 (the output is the input), at max_depth =
    depth (no cap binds) and at depth / 2 and depth / 4 (the cap binds in every full window), each alone between two synchronisations, and each of
    its two steps (the count with its scan; the fill) alone, launched once more on what the pass left, between two events;
  - bsa_window_pieces_run, between two synchronisations, and a device-to-device copy of the piece records, between two events: the yardsticks;
  - the four passes behind it -- bsa_piece_cigars_run, bsa_window_msa_run, bsa_window_cns_run (without its compaction), bsa_window_stitch_run -- on
    the unselected pieces and on the selection at depth / 2, each chain between two synchronisations;
  - the pass at max_depth = depth on the same records with the first 5000 of them put into one window, against the same call on the batch as it is.
The JSON line has median, min and max of each over the rounds, the sizes, and whether the first windows equal the Python statement of the definition
(tests/window_select_cases.window_select_ref) at every max_depth; the tool fails if they do not.  Not measured: other seeds, the identity test's
cost, other window sizes, the _batch call.

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 900 python tools/bench_window_select.py 100000 10000 500 7 --out profiles/window_select_bench_line.json && ...
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
STEPS = ("count", "fill")
DEEP = 5000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=100000)
    ap.add_argument("length", type=int, nargs="?", default=10000)
    ap.add_argument("window", type=int, nargs="?", default=500)
    ap.add_argument("reps", type=int, nargs="?", default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--depth", type=int, default=40, help="pairs in a row that share a draft: the pieces a window holds")
    ap.add_argument("--check", type=int, default=16, help="windows compared with the Python reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import window_cns_cases as WC
    import window_select_cases as W
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())                 # a stream of its own: the events below are recorded on the stream the library launches on
    stream = torch.cuda.current_stream().cuda_stream
    assert stream
    ctx.set_stream(stream)
    lib = B.lib()
    n, L, w, depth = args.pairs, args.length, args.window, max(args.depth, 1)
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

    def pieces():
        ctx.window_pieces_run(d_seqs, d_qoff, d_qlen, d_win, d_woff, n, w, d_gbase, nwin, 0, d_piece, piece_cap, d_poff, d_bases, bases_cap, d_boff)

    timed(pieces)
    poff = d_poff.cpu().numpy().view(np.uint64).copy()
    npieces = int(poff[nwin])
    assert 0 < npieces <= piece_cap
    # the same records with the first DEEP of them in one window: the windows they came from are empty
    deep = poff.copy()
    last = int(np.searchsorted(poff, DEEP, side="left"))       # window 0 ends where window `last` ended
    assert 0 < last <= nwin and int(poff[last]) >= min(DEEP, npieces)
    deep[1:last] = poff[last]
    d_poff_deep = torch.from_numpy(deep.view(np.int64)).to(dev)

    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    caps = {"depth0": 0, "uncapped": depth, "half": max(depth // 2, 1), "quarter": max(depth // 4, 1)}
    d_sel = {k: torch.zeros(max(piece_cap, 1) * 4, dtype=torch.int64, device=dev) for k in caps}
    d_soff = {k: torch.zeros(nwin + 1, dtype=torch.int64, device=dev) for k in caps}
    d_src = torch.zeros(max(piece_cap, 1), dtype=torch.int32, device=dev)
    d_nc = torch.zeros(nwin, dtype=torch.int32, device=dev)
    d_soff_deep = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    par = {k: B.SELECT_PARAMS(md, 0, 0, 0, 0) for k, md in caps.items()}

    def select(k, offs=None, soff=None):
        def fn():
            ctx.window_select_run(d_piece, d_poff if offs is None else offs, nwin, piece_cap, None, 0, par[k], d_sel[k], piece_cap, d_soff[k] if soff is None else soff, d_src, d_nc)
        return fn

    def step(k, i):
        def fn():
            assert lib.bsa_window_select_step_internal(ctx.h, i, p(d_piece), p(d_poff), nwin, piece_cap, None, 0, C.byref(par[k]), p(d_sel[k]), piece_cap, p(d_soff[k]), p(d_src),
                                                       p(d_nc)) == 0
        return fn

    def pass_and_steps(k):
        """the pass between two synchronisations, then each of its steps once more on the scratch it left -> three times"""
        def fn():
            return [timed(select(k))] + [by_events(step(k, i)) for i in range(len(STEPS))]
        return fn

    # the chains behind the pass: guides, MSA, consensus, stitch, on the unselected pieces and on the selection at depth / 2
    for k in caps:
        timed(select(k))
    doff, dlen = B.window_drafts(toff[::depth], tlen[::depth], w)
    assert len(doff) == nwin
    d_doff = torch.from_numpy(doff.view(np.int64)).to(dev)
    d_dlen = torch.from_numpy(dlen.view(np.int32)).to(dev)
    model = ctx.cns_model(WC.PAR7)
    d_pcig = torch.zeros(max(pcig_cap, 1), dtype=torch.int32, device=dev)
    d_pcoff = torch.zeros(piece_cap + 1, dtype=torch.int64, device=dev)

    def chain_of(pc, po):
        """-> (the four passes as one function, its sizes); the buffers are the chain's own"""
        s = {"cols": None, "cap": 0}
        d_coff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
        d_cwin = torch.zeros(max(nwin, 1) * 5, dtype=torch.int64, device=dev)

        def guides():
            ctx.piece_cigars_run(d_out, d_cig, d_off, n, pc, po[nwin:], piece_cap, d_pcig, pcig_cap, d_pcoff, None)

        def msa():
            ctx.window_msa_run(pc, po, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w, 0, 0, s["cols"], s["cap"], d_coff, d_cwin)
        timed(guides)
        timed(msa)                                             # count only: what the columns take
        need = int(d_coff.cpu().numpy()[nwin])
        assert need > 0
        s["cols"], s["cap"] = torch.zeros(need, dtype=torch.uint8, device=dev), need
        timed(msa)
        cwin = d_cwin.cpu().numpy().view(B.CNS_WINDOW_DTYPE)[:nwin].copy()
        out_cap, max_rows = int(cwin["mlen"].astype(np.int64).sum()), int(cwin["nseq"].max())
        d_cns, d_qlt, d_alt, d_seq, d_sq, d_sa = (torch.zeros(max(out_cap, 1), dtype=torch.uint8, device=dev) for _ in range(6))
        d_clen, d_status = torch.zeros(nwin, dtype=torch.int32, device=dev), torch.zeros(nwin, dtype=torch.int32, device=dev)
        d_sqoff, d_goff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev), torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
        d_words = torch.zeros(max(out_cap, 1), dtype=torch.int32, device=dev)
        d_rec = torch.zeros(nwin * 8, dtype=torch.int32, device=dev)

        def cns():
            ctx.window_cns_run(model, s["cols"], need, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, None, d_status)

        def stitch():
            ctx.window_stitch_run(s["cols"], need, d_cwin, nwin, d_status, 1, d_seq, d_sq, d_sa, out_cap, d_sqoff, d_words, out_cap, d_goff, d_rec)

        def parts():
            return [timed(f) for f in (guides, msa, cns, stitch)]
        parts()
        assert not d_status.cpu().numpy().any(), "a window of the MSA pass's own output was dead"
        return parts, {"cols_bytes": need, "max_rows": max_rows, "stitched_bases": int(d_sqoff.cpu().numpy()[nwin])}

    chain_all, size_all = chain_of(d_piece, d_poff)
    chain_half, size_half = chain_of(d_sel["half"], d_soff["half"])
    d_copy = torch.empty(max(piece_cap, 1) * 4, dtype=torch.int64, device=dev)

    def recs_copy():
        d_copy[:4 * npieces].copy_(d_piece[:4 * npieces], non_blocking=True)

    direct = lambda fn: fn()
    rounds = tuple(("select_" + k, direct, pass_and_steps(k)) for k in caps) \
        + (("window_pieces", timed, pieces), ("records_copy_d2d", by_events, recs_copy), ("chain_unselected", direct, chain_all), ("chain_half", direct, chain_half),
           ("select_uncapped_again", timed, select("uncapped")), ("select_uncapped_deep_window", timed, select("uncapped", d_poff_deep, d_soff_deep)))
    for _ in range(args.warmup):
        for _, how, fn in rounds:
            how(fn)
    raw = {k: [] for k, _, _ in rounds}
    for _ in range(args.reps):
        for k, how, fn in rounds:
            raw[k].append(how(fn))
    t = {}
    for k, v in raw.items():
        if k.startswith("select_") and isinstance(v[0], list):
            for i, name in enumerate(("pass",) + tuple(s + "_step" for s in STEPS)):
                t["%s_%s" % (k, name)] = [x[i] for x in v]
        elif k.startswith("chain_"):
            for i, name in enumerate(("piece_cigars", "window_msa", "window_cns", "window_stitch")):
                t["%s_%s" % (k, name)] = [x[i] for x in v]
            t[k] = [sum(x) for x in v]
        else:
            t[k] = v
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the first windows against the definition, at every max_depth, and the deep window
    nchk = min(args.check, nwin)
    piece = d_piece.cpu().numpy().view(W.PIECE_DTYPE)[:max(int(poff[nchk]), int(deep[1]))]          # the records the checked windows speak of
    same, selected = True, {}
    for k, md in caps.items():
        timed(select(k))
        soff = d_soff[k].cpu().numpy().view(np.uint64)
        selected[k] = int(soff[nwin])
        ref = W.window_select_ref(piece, poff[:nchk + 1], piece_cap, None, W.Par(max_depth=md))
        m = int(ref.sel_off[nchk])
        same = same and bool(np.array_equal(ref.sel_off, soff[:nchk + 1]) and np.array_equal(ref.sel, d_sel[k].cpu().numpy().view(W.PIECE_DTYPE)[:m])
                             and np.array_equal(ref.src, d_src.cpu().numpy().view(np.uint32)[:m]) and np.array_equal(ref.ncand, d_nc.cpu().numpy().view(np.uint32)[:nchk]))
    timed(select("uncapped", d_poff_deep, d_soff_deep))
    soff = d_soff_deep.cpu().numpy().view(np.uint64)
    ref = W.window_select_ref(piece, deep[:2], piece_cap, None, W.Par(max_depth=depth))
    m = int(ref.sel_off[1])
    same = same and bool(m == int(soff[1]) and np.array_equal(ref.sel, d_sel["uncapped"].cpu().numpy().view(W.PIECE_DTYPE)[:m])
                         and int(d_nc.cpu().numpy().view(np.uint32)[0]) == int(ref.ncand[0]))
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "max_depth": caps, "deep_window": int(deep[1]), "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "record_bytes": 32 * npieces, "selected": selected, "scratch_bytes": 16 * nwin,
           "chain_unselected_sizes": size_all, "chain_half_sizes": size_half,
           "pass_over_window_pieces": {k: round(med["select_%s_pass" % k] / med["window_pieces"], 3) for k in caps},
           "pass_over_records_copy": {k: round(med["select_%s_pass" % k] / med["records_copy_d2d"], 3) for k in caps},
           "chain_half_over_unselected": round(med["chain_half"] / med["chain_unselected"], 3),
           "saved_ms_by_half": round(med["chain_unselected"] - med["chain_half"] - med["select_half_pass"], 3),
           "deep_window_over_plain": round(med["select_uncapped_deep_window"] / med["select_uncapped_again"], 3),
           "not_measured": ["other seeds", "the identity test's cost", "other window sizes", "the _batch call"],
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
