#!/usr/bin/env python3
"""What bsa_window_msa_run costs at C2's shape, device-resident (one process, one GPU), against what it is to be judged by: a plain device-to-device
copy of the bytes its fill writes, the three passes in front of it, and the copy of the MSA to the host.

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring, windows of 500 target
bases, `--depth` pairs in a row on one draft (as tools/bench_piece_cigars.py; the draft is the first of those pairs' targets).  One align step
makes records, words and offsets, the three passes make windows, pieces and guides, a count-only run of the pass says how many bytes the columns
take; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see the same device state):
  - bsa_cigar_windows_run, bsa_window_pieces_run, bsa_piece_cigars_run and the pass (bsa_window_msa_run), each alone between two synchronisations;
  - each of the pass's four steps (cols, scan, records, fill) alone, launched once more on what the pass left, between two events;
  - a device-to-device hipMemcpyAsync of as many bytes as the fill writes, between two events;
  - the copy of the MSA (columns, offsets, records) to pinned host memory, between two synchronisations.
The JSON line has median, min and max of each over the rounds, the sizes, the fill's ratio to the plain copy, and whether the first windows equal
the Python statement of the definition (tests/window_msa_cases.window_msa_ref).

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 600 python tools/bench_window_msa.py --out profiles/window_msa_bench_line.json && ...
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
STEPS = ("cols", "scan", "records", "fill")


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
    import window_msa_cases as W
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())                 # a stream of its own: the events below are recorded on the stream the library launches on
    stream = torch.cuda.current_stream().cuda_stream           # (the default stream's handle is 0, which bsa_ctx_set_stream takes for "the context's own")
    assert stream
    ctx.set_stream(stream)
    lib = B.lib()
    lib.bsa_window_msa_step_internal.argtypes = [C.c_void_p, C.c_int] + list(lib.bsa_window_msa_run.argtypes[1:])
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
    words = int(coff[n])
    assert words <= cig_cap, "the align run was not complete"
    records = int(d_woff.cpu().numpy()[n])
    assert records <= win_cap
    piece_cap, bases_cap = records, int(qlen.astype(np.int64).sum())          # the caps the header calls sufficient
    pcig_cap = B.piece_cigars_bound(coff, piece_cap)
    d_piece = torch.zeros(max(piece_cap, 1) * 4, dtype=torch.int64, device=dev)
    d_bases = torch.zeros(max(bases_cap, 1), dtype=torch.uint8, device=dev)
    d_poff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    d_boff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)
    d_pcig = torch.zeros(max(pcig_cap, 1), dtype=torch.int32, device=dev)
    d_pcoff = torch.zeros(piece_cap + 1, dtype=torch.int64, device=dev)
    d_pst = torch.zeros(max(piece_cap, 1), dtype=torch.int32, device=dev)
    d_np = d_poff[nwin:]                                       # the pieces there are: where bsa_window_pieces_run leaves the count

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

    p = lambda t: C.c_void_p(t.data_ptr())

    # the draft of window g: the target of the first pair on it, from the window's first base on
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
    pwords = int(d_pcoff.cpu().numpy()[piece_cap])
    assert npieces <= piece_cap and pwords <= pcig_cap, (npieces, piece_cap, pwords, pcig_cap)
    state = {"cols": None, "cap": 0}

    def msa():
        ctx.window_msa_run(d_piece, d_poff, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w, 0, 0,
                           state["cols"], state["cap"], d_coff, d_cwin)

    timed(msa)                                                 # count only: what the columns take
    need = int(d_coff.cpu().numpy()[nwin])
    ins_units = int(d_out.view(n, 10)[:, 7].sum().item())
    bound = B.window_msa_bound(d_poff.cpu().numpy().view(np.uint64), w, ins_units)
    assert 0 < need <= bound, (need, bound)
    state["cols"], state["cap"] = torch.zeros(need, dtype=torch.uint8, device=dev), need
    d_copy = torch.empty(need, dtype=torch.uint8, device=dev)
    d_cols = state["cols"]

    def step(i):
        def fn():
            assert lib.bsa_window_msa_step_internal(ctx.h, i, p(d_piece), p(d_poff), nwin, piece_cap, p(d_bases), bases_cap, p(d_pcig), pcig_cap, p(d_pcoff), p(d_seqs),
                                                    p(d_doff), p(d_dlen), w, 0, 0, p(d_cols), need, p(d_coff), p(d_cwin)) == 0
        return fn

    def plain_copy():
        d_copy.copy_(d_cols, non_blocking=True)

    h_cols = torch.empty(need, dtype=torch.uint8).pin_memory()
    h_coff = torch.empty(nwin + 1, dtype=torch.int64).pin_memory()
    h_cwin = torch.empty(max(nwin, 1) * 5, dtype=torch.int64).pin_memory()

    def to_host():
        h_cols.copy_(d_cols, non_blocking=True)
        h_coff.copy_(d_coff, non_blocking=True)
        h_cwin.copy_(d_cwin, non_blocking=True)

    for _ in range(args.warmup):
        timed(windows)
        timed(pieces)
        timed(cigars)
        timed(msa)
        for i in range(4):
            by_events(step(i))
        by_events(plain_copy)
        timed(to_host)
    names = ("cigar_windows", "window_pieces", "piece_cigars", "pass") + tuple(s + "_kernel" for s in STEPS) + ("plain_copy_d2d", "msa_d2h")
    t = {k: [] for k in names}
    for _ in range(args.reps):
        t["cigar_windows"].append(timed(windows))
        t["window_pieces"].append(timed(pieces))
        t["piece_cigars"].append(timed(cigars))
        t["pass"].append(timed(msa))
        for i, s in enumerate(STEPS):
            t[s + "_kernel"].append(by_events(step(i)))
        t["plain_copy_d2d"].append(by_events(plain_copy))
        t["msa_d2h"].append(timed(to_host))
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the first windows against the definition: they lie on the first draft
    timed(msa)
    nchk = min(args.check, nwin, wpt)
    poff = d_poff[:nchk + 1].cpu().numpy().view(np.uint64)
    pchk = int(poff[nchk])
    pcs = d_piece[:pchk * 4].cpu().numpy().view(B.PIECE_DTYPE)
    pcoff = d_pcoff[:pchk + 1].cpu().numpy().view(np.uint64)
    nb = int((pcs["base_off"] + pcs["len"]).max()) if pchk else 0
    b = W.Batch(pcs, poff, d_bases[:nb].cpu().numpy(), d_pcig[:int(pcoff[pchk])].cpu().numpy().view(np.uint32), pcoff, d_seqs[:L + 8].cpu().numpy(), doff[:nchk], dlen[:nchk], w)
    roff, rcwin, rcols = W.window_msa_ref(b, 0)
    g_off = d_coff[:nchk + 1].cpu().numpy().view(np.uint64)
    g_cwin = d_cwin[:nchk * 5].cpu().numpy().view(B.CNS_WINDOW_DTYPE)
    g_cols = d_cols[:int(roff[nchk])].cpu().numpy()
    same = bool(np.array_equal(roff, g_off) and g_cwin.tolist() == rcwin.tolist() and np.array_equal(rcols, g_cols))
    mlen = d_cwin.view(-1, 5)[:, 4].cpu().numpy().view(np.uint32).reshape(-1, 2)[:, 1]
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "piece_cigar_words": pwords, "cols_bytes": need, "cols_bound_bytes": bound, "ins_units": ins_units,
           "mlen_mean": round(float(mlen.mean()), 1), "mlen_max": int(mlen.max()), "line_scratch_bytes": 4 * nwin * w,
           "fill_over_plain_copy": round(med["fill_kernel"] / med["plain_copy_d2d"], 3) if med["plain_copy_d2d"] else None,
           "fill_GBps_written": round(1e-6 * need / med["fill_kernel"], 1) if med["fill_kernel"] else None,
           "pass_over_msa_d2h": round(med["pass"] / med["msa_d2h"], 3) if med["msa_d2h"] else None,
           "checked_windows": nchk, "checked_pieces": pchk, "identical": same}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
