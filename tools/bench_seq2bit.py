#!/usr/bin/env python3
"""2-bit packed sequence blobs (BSA_MODE_SEQ2BIT) against one byte a base, at C2 (one process, one GPU).

C2: 100 000 synthetic pairs of 10 kbp (bsa_synth_pairs_dev, bench.py's seed), global, bandwidth 128, default scoring.  The blob is made on the
device and packed there with bsa_seq_pack2bit; both forms are then measured on the same pairs at the same offsets:

1. host-pointer calls (bsa_align_batch: plan + upload from pageable memory + kernels + download of records and CIGAR words) on reused caller
   buffers, each form called once to warm its buffers, then the two forms alternately `--rounds` times; with BSA_API_TIMING the library's
   timeline of every call (stderr) is captured into the JSON line;
2. device-resident steps (plan.run between two synchronisations, as bench.py times its step), `--warmup` then `--steps` each;
3. `identical`: results, CIGAR words, offsets and status agree on every pair, between the two forms and between host and device calls.

--device-only runs part 2 alone (for a kernel trace: rocprofv3 --kernel-trace --stats in a run of its own); --stats CSV folds the staging
kernels' rows of such a trace (k_stage / k_stage2b) into the JSON line.  Prints ONE JSON line."""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20240611


def staging_stats(path):
    """the staging kernels' rows of a rocprofv3 --stats kernel table"""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "k_stage" in name and "k_edit" not in name:
                key = "k_stage2b" if "k_stage2b" in name else "k_stage"
                rows[key] = {"calls": int(r["Calls"]), "avg_ms": round(float(r["AverageNs"]) / 1e6, 4), "kernel": name.split("(")[0]}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--bw", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3, help="host-pointer calls of each form after the warm-up call, alternating")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel_stats.csv of a --device-only run")
    args = ap.parse_args()
    os.environ.setdefault("BSA_API_TIMING", "1")
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    ctx = B.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = B.lib()
    n, L, bw = args.pairs, args.length, args.bw
    stride = lib.bsa_synth_stride(L)
    nb = 2 * n * stride
    d_seqs = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    d_bits = torch.zeros((nb + 31) // 32, dtype=torch.int64, device=dev)
    d_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx.seq_pack2bit(d_seqs, d_bits, d_bad)
    torch.cuda.synchronize()
    assert int(d_bad.item()) == 0
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)          # (one byte a base: byte offsets are base offsets)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
    cells = float(L) * bw * n
    cig_cap = n * max(L // 4, 64)
    forms = {"bytes": (0, d_seqs), "seq2bit": (B.MODE_SEQ2BIT, d_bits)}
    res = {"config": {"pairs": n, "length": L, "bandwidth": bw, "scoring": "2,-6,-3,-2,0,0", "steps": args.steps, "warmup": args.warmup,
                      "blob_bytes": {"bytes": int(nb), "seq2bit": int(d_bits.numel() * 8)}}}

    # ---- 2. device-resident steps
    dev_out = {}
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(cig_cap, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    resident = {}
    for name, (flag, d) in forms.items():
        plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL | flag, bw, 2, -6, -3, -2, 0, 0))

        def step():
            torch.cuda.synchronize()
            plan.run(d, d_out, d_cig, d_off, d_st)
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            step()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        kms, _, _ = ctx.last_kernel_ms()
        off = d_off.cpu().numpy()
        dev_out[name] = (d_out.cpu().numpy().reshape(n, 10), off, d_cig[:int(off[n])].cpu().numpy().view(np.uint32), d_st.cpu().numpy().view(np.uint32))
        resident[name] = {"ms_per_step": round(ms, 3), "gcups": round(cells / ms / 1e6, 1), "forward_ms": round(kms, 3), "forward_kernel": ctx.last_kernel_names()[0]}
        plan.close()
    del d_cig
    res["device_resident"] = resident
    same = all(np.array_equal(a, b) for a, b in zip(dev_out["bytes"], dev_out["seq2bit"]))
    if args.stats:
        res["staging_kernels"] = staging_stats(args.stats)
    if args.device_only:
        res["identical"] = same
        print(json.dumps(res))
        return 0

    # ---- 1. host-pointer calls
    host = {"bytes": d_seqs.cpu().numpy(), "seq2bit": d_bits.cpu().numpy().view(np.uint64)}
    bufs = {name: (np.zeros((n, 10), np.int32), np.zeros(cig_cap, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)) for name in forms}
    times = {name: [] for name in forms}
    timelines = {name: [] for name in forms}

    def call(name):
        flag = forms[name][0]
        par = B.make_params(B.MODE_GLOBAL | flag, bw, 2, -6, -3, -2, 0, 0)
        blob = host[name]
        h_out, h_cig, h_off, h_st = bufs[name]
        # the library's timeline (BSA_API_TIMING, stderr) of this call
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile(mode="w+b") as tf:
            os.dup2(tf.fileno(), 2)
            try:
                t0 = time.perf_counter()
                rc = lib.bsa_align_batch(ctx.h, blob.ctypes.data, blob.nbytes, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data, n,
                                         C.byref(par), h_out.ctypes.data, h_cig.ctypes.data, cig_cap, h_off.ctypes.data, h_st.ctypes.data)
                ms = (time.perf_counter() - t0) * 1e3
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tf.seek(0)
            log = tf.read().decode(errors="replace").strip().splitlines()
        ctx._chk(rc)
        return ms, log
    for name in forms:
        call(name)                                    # (first call: page faults of the output buffers, first pinning of the input)
    for _ in range(args.rounds):
        for name in forms:
            ms, log = call(name)
            times[name].append(round(ms, 2))
            timelines[name].append(log)
    hp = {}
    for name in forms:
        hp[name] = {"ms": times[name], "median_ms": round(float(np.median(times[name])), 2), "upload_bytes": int(host[name].nbytes),
                    "timeline_last_call": timelines[name][-1]}
    hp["saving"] = round(1.0 - hp["seq2bit"]["median_ms"] / hp["bytes"]["median_ms"], 4)
    res["host_pointer"] = hp
    for name in forms:
        h_out, h_cig, h_off, h_st = bufs[name]
        d = dev_out[name]
        same = same and np.array_equal(h_out, d[0]) and np.array_equal(h_off.astype(np.int64), d[1]) and np.array_equal(h_cig[:int(h_off[n])], d[2]) \
            and np.array_equal(h_st, d[3])
    res["identical"] = bool(same)
    res["flagged"] = int((dev_out["seq2bit"][3] != 0).sum())
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
