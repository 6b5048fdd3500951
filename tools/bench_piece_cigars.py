#!/usr/bin/env python3
"""What bsa_piece_cigars_run costs at C2's shape, device-resident (one process, one GPU), against what it is to be judged by: the device-to-host
copy of the CIGAR arena that the host route needs before it can slice a single piece's words.

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring, windows of 500 target
bases, `--depth` pairs in a row on one draft (as tools/bench_window_pieces.py).  One align step makes records, words and offsets; then, after the
warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see the same device state):
  - bsa_cigar_windows_run, bsa_window_pieces_run and the pass (bsa_piece_cigars_run), each alone between two synchronisations;
  - each of the pass's four steps (index, count, scan, fill) alone, launched once more on what the pass left, between two events;
  - the host route's transfer: the words of the CIGAR arena, device to host into pinned memory, between two synchronisations.  The host
    route's walk over the words is NOT timed: its figure is a lower bound;
  - the transfer of what this pass leaves: its words and offsets, likewise.
The JSON line has median, min and max of each over the rounds, the sizes, and whether the first windows equal the Python statement of the
definition (tests/piece_cigars_cases.piece_cigars_ref).

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 600 python tools/bench_piece_cigars.py --out profiles/piece_cigars_bench_line.json && ...
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
STEPS = ("index", "count", "scan", "fill")


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
    import piece_cigars_cases as P
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())                 # a stream of its own: the events below are recorded on the stream the library launches on
    stream = torch.cuda.current_stream().cuda_stream           # (the default stream's handle is 0, which bsa_ctx_set_stream takes for "the context's own")
    assert stream
    ctx.set_stream(stream)
    lib = B.lib()
    lib.bsa_piece_cigars_step_internal.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
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

    def step(i):
        def fn():
            assert lib.bsa_piece_cigars_step_internal(ctx.h, i, p(d_out), p(d_cig), p(d_off), n, p(d_piece), p(d_np), piece_cap, p(d_pcig), pcig_cap, p(d_pcoff), p(d_pst)) == 0
        return fn

    timed(pieces)
    for _ in range(args.warmup):
        timed(windows)
        timed(pieces)
        timed(cigars)
        for i in range(4):
            by_events(step(i))
    npieces = int(d_poff.cpu().numpy()[nwin])
    assert npieces <= piece_cap
    pwords = int(d_pcoff.cpu().numpy()[piece_cap])
    assert pwords <= pcig_cap, (pwords, pcig_cap)
    h_cig = torch.empty(max(words, 1), dtype=torch.int32).pin_memory()
    h_pcig = torch.empty(max(pwords, 1), dtype=torch.int32).pin_memory()
    h_pcoff = torch.empty(npieces + 1, dtype=torch.int64).pin_memory()

    def host_route():
        h_cig[:words].copy_(d_cig[:words], non_blocking=True)

    def this_route():
        h_pcig[:pwords].copy_(d_pcig[:pwords], non_blocking=True)
        h_pcoff.copy_(d_pcoff[:npieces + 1], non_blocking=True)

    names = ("cigar_windows", "window_pieces", "pass") + tuple(s + "_kernel" for s in STEPS) + ("cigar_arena_d2h", "piece_cigars_d2h")
    t = {k: [] for k in names}
    for _ in range(args.reps):
        t["cigar_windows"].append(timed(windows))
        t["window_pieces"].append(timed(pieces))
        t["pass"].append(timed(cigars))
        for i, s in enumerate(STEPS):
            t[s + "_kernel"].append(by_events(step(i)))
        t["cigar_arena_d2h"].append(timed(host_route))
        t["piece_cigars_d2h"].append(timed(this_route))
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the first windows against the definition: the pairs of the first draft hold them all
    timed(cigars)
    nchk = min(args.check, nwin, wpt)
    kk = min(depth, n)
    poff = d_poff[:nchk + 1].cpu().numpy().view(np.uint64)
    pchk = int(poff[nchk])
    pcs = d_piece[:pchk * 4].cpu().numpy().view(B.PIECE_DTYPE)
    assert pchk == 0 or int(pcs["pair"].max()) < kk
    out = d_out[:kk * 10].cpu().numpy().view(B.RESULT_DTYPE)
    roff, rwords, rst = P.piece_cigars_ref(out, d_cig[:int(coff[kk])].cpu().numpy().view(np.uint32), coff[:kk + 1], pcs)
    g_off = d_pcoff[:pchk + 1].cpu().numpy().view(np.uint64)
    g_words = d_pcig[:int(roff[pchk])].cpu().numpy().view(np.uint32)
    g_st = d_pst[:pchk].cpu().numpy().view(np.uint32)
    same = bool(np.array_equal(roff, g_off) and np.array_equal(rwords, g_words) and np.array_equal(rst, g_st))
    not_cut = int((d_pst[:npieces] != 0).sum().item())
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "pieces_not_cut": not_cut, "cigar_words": words, "cigar_arena_bytes": 4 * words, "piece_cigar_words": pwords,
           "piece_cigars_bytes": 4 * pwords + 8 * (npieces + 1), "pcig_cap_words": pcig_cap, "index_scratch_bytes": 512 * n, "piece_scratch_bytes": 36 * piece_cap,
           "host_route_untimed": "the walk over every pair's words that slices them at the pieces' columns",
           "pass_over_arena_copy": round(med["pass"] / med["cigar_arena_d2h"], 3) if med["cigar_arena_d2h"] else None,
           "pass_GBps_arena_read_once_plus_words_written": round(4e-6 * (words + pwords) / med["pass"], 1) if med["pass"] else None,
           "checked_windows": nchk, "checked_pieces": pchk, "identical": same}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same and not_cut == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
