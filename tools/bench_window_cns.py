#!/usr/bin/env python3
"""What bsa_window_cns_run costs at C2's shape, device-resident (one process, one GPU), against what it is to be judged by: the route it replaces
(the MSA's copy to pinned host memory and bsa_msa_call_consensus_batch on it), the four passes in front of it, and what comes down afterwards.

C2 as in tools/bench_window_msa.py: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default
scoring, windows of 500 target bases, `--depth` pairs in a row on one draft.  One align step and the four passes leave every window's MSA and its
record on the device; then, after the warm-up, `reps` rounds time, one after the other (interleaved, so that all of them see the same device state):
  - bsa_cigar_windows_run, bsa_window_pieces_run, bsa_piece_cigars_run, bsa_window_msa_run and the pass (bsa_window_cns_run with compaction), each
    alone between two synchronisations;
  - each of the pass's four steps (prepare with its scan and the records; k_cns_dp; k_cns_finish; the pack with its scan) alone, launched once more
    on what the pass left, between two events;
  - a device-to-device copy of the three compact arrays, between two events: what the pack is measured against;
  - the route the pass replaces: the columns and records to pinned host memory, then bsa_msa_call_consensus_batch on them in slices of `--slice`
    windows (it uploads the columns and brings them back), between two synchronisations each;
  - the copy of the compact result (bases, both qualities, offsets, lengths, scores, statuses) to pinned host memory.
The JSON line has median, min and max of each over the rounds, the sizes, and whether the first windows equal the Python statement of the definition
(tests/window_cns_cases.window_cns_ref) and the host-pointer call's results.

Every step that touches the GPU belongs under a time limit of its own; run it as
    timeout -k 10 900 python tools/bench_window_cns.py --out profiles/window_cns_bench_line.json && ...
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
STEPS = ("prepare", "dp", "finish", "pack")


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
    ap.add_argument("--slice", type=int, default=5000, help="windows a call of the host-pointer route")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bsalign_amd as B
    import window_cns_cases as WC
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
    d_score = torch.zeros(nwin, dtype=torch.float64, device=dev)
    d_status = torch.zeros(nwin, dtype=torch.int32, device=dev)
    d_soff = torch.zeros(nwin + 1, dtype=torch.int64, device=dev)

    def cns():
        ctx.window_cns_run(model, d_cols, need, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, d_score, d_status, d_seq, d_sq, d_sa, out_cap, d_soff)

    def step(i):
        def fn():
            assert lib.bsa_window_cns_step_internal(ctx.h, i, model.h, p(d_cols), need, p(d_cwin), nwin, max_rows, p(d_cns), p(d_qlt), p(d_alt), out_cap, p(d_clen), p(d_score),
                                                    p(d_status), p(d_seq), p(d_sq), p(d_sa), out_cap, p(d_soff)) == 0
        return fn

    timed(cns)
    seq_bytes = int(d_soff.cpu().numpy()[nwin])
    status = d_status.cpu().numpy()
    assert 0 < seq_bytes <= out_cap and not status.any(), "a window of the MSA pass's own output was dead"
    d_copy = torch.empty(3 * seq_bytes, dtype=torch.uint8, device=dev)

    def plain_copy():
        for k, t in enumerate((d_seq, d_sq, d_sa)):
            d_copy[k * seq_bytes:(k + 1) * seq_bytes].copy_(t[:seq_bytes], non_blocking=True)

    h_cols = torch.empty(need, dtype=torch.uint8).pin_memory()
    h_cwin = torch.empty(max(nwin, 1) * 5, dtype=torch.int64).pin_memory()
    h_seq = torch.empty(3 * seq_bytes, dtype=torch.uint8).pin_memory()
    h_soff = torch.empty(nwin + 1, dtype=torch.int64).pin_memory()
    h_clen = torch.empty(nwin, dtype=torch.int32).pin_memory()
    h_score = torch.empty(nwin, dtype=torch.float64).pin_memory()
    h_status = torch.empty(nwin, dtype=torch.int32).pin_memory()

    def msa_to_host():
        h_cols.copy_(d_cols, non_blocking=True)
        h_cwin.copy_(d_cwin, non_blocking=True)

    def result_to_host():
        for k, t in enumerate((d_seq, d_sq, d_sa)):
            h_seq[k * seq_bytes:(k + 1) * seq_bytes].copy_(t[:seq_bytes], non_blocking=True)
        h_soff.copy_(d_soff, non_blocking=True)
        h_clen.copy_(d_clen, non_blocking=True)
        h_score.copy_(d_score, non_blocking=True)
        h_status.copy_(d_status, non_blocking=True)

    # the host-pointer route on the columns that came down, in slices of windows; each slice's records count from its own first byte and column
    lib.bsa_msa_call_consensus_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    hc = h_cols.numpy()
    slices = []
    for a in range(0, nwin, max(args.slice, 1)):
        b = min(a + max(args.slice, 1), nwin)
        r = cwin[a:b].copy()
        c0, o0 = int(r["cols_off"][0]), int(r["out_off"][0])
        c1, o1 = int(r["cols_off"][-1]) + int(r["mlen"][-1]) * (int(r["nall"][-1]) + 3), int(r["out_off"][-1]) + int(r["mlen"][-1])
        r["cols_off"] -= np.uint64(c0)
        r["out_off"] -= np.uint64(o0)
        slices.append((a, b, r, c0, c1, o0, o1))
    r_cns, r_qlt, r_alt = (np.zeros(max(out_cap, 1), np.uint8) for _ in range(3))
    r_clen, r_score = np.zeros(nwin, np.uint32), np.zeros(nwin, np.float64)
    par = np.ascontiguousarray(WC.PAR7, np.float32)

    def host_route():
        for a, b, r, c0, c1, o0, o1 in slices:
            rc = lib.bsa_msa_call_consensus_batch(ctx.h, B._p(hc[c0:c1]), c1 - c0, None, 0, B._p(r), b - a, B._p(par), B._p(r_cns[o0:]), B._p(r_qlt[o0:]), B._p(r_alt[o0:]), o1 - o0,
                                                  B._p(r_clen[a:]), B._p(r_score[a:]))
            assert rc == 0, rc

    rounds = (("cigar_windows", timed, windows), ("window_pieces", timed, pieces), ("piece_cigars", timed, cigars), ("window_msa", timed, msa), ("pass", timed, cns)) \
        + tuple((s + "_step", by_events, step(i)) for i, s in enumerate(STEPS)) \
        + (("plain_copy_d2d", by_events, plain_copy), ("msa_d2h", timed, msa_to_host), ("host_pointer_call", timed, host_route), ("result_d2h", timed, result_to_host))
    for _ in range(args.warmup):
        for _, how, fn in rounds:
            how(fn)
    t = {k: [] for k, _, _ in rounds}
    for _ in range(args.reps):
        for k, how, fn in rounds:
            t[k].append(how(fn))
    stat = lambda f: {k: round(float(f(v)), 3) for k, v in t.items()}
    med = stat(np.median)
    # the resident result against the host-pointer route's (the same kernels on the same tables: the same bits), and the first windows against the definition
    timed(msa)
    timed(cns)
    timed(result_to_host)
    clen = h_clen.numpy().view(np.uint32)
    same_route = bool(np.array_equal(clen, r_clen) and np.array_equal(h_score.numpy(), r_score))
    g_cns = d_cns.cpu().numpy()
    for g in range(0, nwin, max(nwin // 64, 1)):
        o, k = int(cwin[g]["out_off"]), int(clen[g])
        same_route = same_route and bool(np.array_equal(g_cns[o:o + k], r_cns[o:o + k]))
    nchk = min(args.check, nwin)
    cend = int(cwin[nchk - 1]["cols_off"]) + int(cwin[nchk - 1]["mlen"]) * (int(cwin[nchk - 1]["nall"]) + 3)
    oend = int(cwin[nchk - 1]["out_off"]) + int(cwin[nchk - 1]["mlen"])
    g_cols = d_cols[:cend].cpu().numpy()
    ref = WC.window_cns_ref(g_cols, cwin[:nchk], cend, oend, oend, max_rows, WC.PAR7)
    soff = h_soff.numpy().view(np.uint64)
    send = int(soff[nchk])
    hs = h_seq.numpy()
    same = bool(np.array_equal(ref.clen, clen[:nchk]) and np.array_equal(ref.seq_off, soff[:nchk + 1]) and np.array_equal(ref.cols, g_cols)
                and np.array_equal(ref.seq[:send], hs[:send]) and np.array_equal(ref.seq_qlt[:send], hs[seq_bytes:seq_bytes + send])
                and np.array_equal(ref.seq_alt[:send], hs[2 * seq_bytes:2 * seq_bytes + send])
                and bool(np.all(np.abs(ref.score - h_score.numpy()[:nchk]) <= 1e-12 * np.maximum(1.0, np.abs(ref.score)))))
    wcols = min(out_cap, need // 4)
    res = {"config": {"pairs": n, "length": L, "window": w, "depth": depth, "bandwidth": args.bw, "scoring": ",".join(str(x) for x in sc), "reps": args.reps,
                      "warmup": args.warmup, "slice_windows": args.slice, "library": os.path.relpath(B.LIB_PATH, ROOT)},
           "median_ms": med, "min_ms": stat(np.min), "max_ms": stat(np.max), "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "windows": nwin, "pieces": npieces, "cols_bytes": need, "out_cap": out_cap, "max_rows": max_rows, "seq_bytes": seq_bytes,
           "result_bytes": 3 * seq_bytes + 8 * (nwin + 1) + 16 * nwin, "scratch_bytes": 80 * nwin + 42 * (wcols + nwin),
           "mlen_mean": round(float(cwin["mlen"].mean()), 1), "clen_mean": round(float(clen.mean()), 1),
           "replaced_route_ms": round(med["msa_d2h"] + med["host_pointer_call"], 3),
           "pass_plus_result_ms": round(med["pass"] + med["result_d2h"], 3),
           "pack_over_plain_copy": round(med["pack_step"] / med["plain_copy_d2d"], 3) if med["plain_copy_d2d"] else None,
           "checked_windows": nchk, "identical": same, "identical_to_host_pointer_call": same_route}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same and same_route else 1


if __name__ == "__main__":
    sys.exit(main())
