#!/usr/bin/env python3
"""What bsa_window_pieces_run costs at C2's shape, device-resident (one process, one GPU), against the two things it is to be judged by: a plain
device-to-device copy of the bytes it gathers, and the transfer of the host route it replaces.

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring, windows of 500 target
bases.  The generator gives every pair a target of its own; `--depth` pairs in a row are taken to lie on one draft (gbase[k] = (k // depth) *
ceil(length / window)), so that a window holds `depth` pieces as a polisher's does.  One align step and one bsa_cigar_windows_run make the window
records; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see the same device state):
  - the pass alone (bsa_window_pieces_run), between two synchronisations;
  - its gather kernel alone, launched once more over the records the pass left, between two events;
  - a device-to-device hipMemcpyAsync of as many bytes as the gather writes, between two events;
  - the host route's transfer: the window records and the query half of the blob, device to host into pinned memory, between two
    synchronisations.  The host route's bucketing, slicing, reverse-complementing and unpacking are NOT timed: its figure is a lower bound.
The JSON line has median, min and max of each over the rounds, the sizes, and whether the first windows equal the Python statement of the
definition (tests/window_pieces_cases.pieces_ref).

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 600 python tools/bench_window_pieces.py --out profiles/window_pieces_bench_line.json && ...
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
    ap.add_argument("reps", type=int, nargs="?", default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--depth", type=int, default=40, help="pairs in a row that share a draft: the pieces a window holds")
    ap.add_argument("--check", type=int, default=16, help="windows compared with the Python reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import window_pieces_cases as P
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    torch.cuda.set_stream(torch.cuda.Stream())                 # a stream of its own: the events below are recorded on the stream the library launches on
    stream = torch.cuda.current_stream().cuda_stream           # (the default stream's handle is 0, which bsa_ctx_set_stream takes for "the context's own")
    assert stream
    ctx.set_stream(stream)
    lib = B.lib()
    lib.bsa_window_pieces_gather_internal.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    hip = C.CDLL("libamdhip64.so")                             # (the copy the process already has: torch's)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
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
    del d_cig
    records = int(d_woff.cpu().numpy()[n])
    assert records <= win_cap
    piece_cap, bases_cap = records, int(qlen.astype(np.int64).sum())          # the caps the header calls sufficient
    d_piece = torch.zeros(max(piece_cap, 1) * 4, dtype=torch.int64, device=dev)
    d_bases = torch.zeros(max(bases_cap, 1), dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(max(bases_cap, 1), dtype=torch.uint8, device=dev)
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

    p = lambda t: C.c_void_p(t.data_ptr())

    def gather():
        assert lib.bsa_window_pieces_gather_internal(ctx.h, p(d_seqs), p(d_qoff), p(d_qlen), nwin, 0, p(d_piece), piece_cap, p(d_bases), bases_cap) == 0

    for _ in range(args.warmup):
        timed(pieces)
        by_events(gather)
    npieces, nbytes = int(d_poff.cpu().numpy()[nwin]), int(d_boff.cpu().numpy()[nwin])
    assert npieces <= piece_cap and nbytes <= bases_cap
    h_win = torch.empty(max(records, 1) * 4, dtype=torch.int32).pin_memory()
    h_seq = torch.empty(n * stride, dtype=torch.uint8).pin_memory()
    h_piece = torch.empty(max(npieces, 1) * 4, dtype=torch.int64).pin_memory()
    h_bases = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()

    def copy_d2d():
        assert hip.hipMemcpyAsync(p(d_copy), p(d_bases), nbytes, 3, C.c_void_p(stream)) == 0

    def host_route():
        h_win[:records * 4].copy_(d_win[:records * 4], non_blocking=True)
        h_seq.copy_(d_seqs[n * stride:], non_blocking=True)

    def this_route():
        h_piece[:npieces * 4].copy_(d_piece[:npieces * 4], non_blocking=True)
        h_bases[:nbytes].copy_(d_bases[:nbytes], non_blocking=True)

    t = {k: [] for k in ("pass", "gather_kernel", "copy_d2d", "host_route_d2h", "pieces_d2h")}
    for _ in range(args.reps):
        t["pass"].append(timed(pieces))
        t["gather_kernel"].append(by_events(gather))
        t["copy_d2d"].append(by_events(copy_d2d))
        t["host_route_d2h"].append(timed(host_route))
        t["pieces_d2h"].append(timed(this_route))
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the first windows against the definition: the pairs of the first draft hold them all
    timed(pieces)
    nchk = min(args.check, nwin, wpt)
    kk = min(depth, n)
    woff = d_woff.cpu().numpy().view(np.uint64)[:kk + 1].copy()
    win = d_win[:int(woff[kk]) * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)
    seqs = d_seqs[n * stride:(n + kk) * stride].cpu().numpy()
    poff, boff, recs, codes = P.pieces_ref(seqs, qoff[:kk] - qoff[0], qlen[:kk], win, woff, w, gbase[:kk], nchk, 0)
    g_poff, g_boff = d_poff[:nchk + 1].cpu().numpy().view(np.uint64), d_boff[:nchk + 1].cpu().numpy().view(np.uint64)
    g_recs = d_piece[:int(poff[nchk]) * 4].cpu().numpy().view(P.PIECE_DTYPE)
    g_codes = d_bases[:int(boff[nchk])].cpu().numpy()
    same = bool(np.array_equal(poff, g_poff) and np.array_equal(boff, g_boff) and np.array_equal(recs, g_recs) and np.array_equal(codes, g_codes))
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "flags": 0, "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "window_records": records, "pieces": npieces, "piece_bytes": 32 * npieces, "gathered_bytes": nbytes,
           "host_route_bytes": 16 * records + n * stride, "host_route_untimed": "bucketing by window, slicing, reverse complement, unpacking",
           "gather_GBps_read_plus_write": round(2e-6 * nbytes / med["gather_kernel"], 1) if med["gather_kernel"] else None,
           "copy_GBps_read_plus_write": round(2e-6 * nbytes / med["copy_d2d"], 1) if med["copy_d2d"] else None,
           "gather_over_copy": round(med["gather_kernel"] / med["copy_d2d"], 2) if med["copy_d2d"] else None,
           "checked_windows": nchk, "checked_pieces": int(len(recs)), "identical": same}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
