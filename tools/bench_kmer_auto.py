"""What BSA_KMER_STRAND_AUTO costs beside the route it replaces: bsa_kmer_chain_batch2 on a blob in which every second query is stored
reverse-complemented and nobody says which.  Three variants in one process, one warm-up call each, median of the repetitions, calls interleaved:
    auto      the flagged call (one sort a pair, both strands chained from it)
    two_call  what a caller does today: the plain call, the call with BSA_MODE_QSTRAND and every pair marked, anchor counts compared on the host
    plain     one plain call (the floor: no strand search at all)
Reported per variant: the chain kernels' time (bsa_ctx_last_kmer_chain_ms; for two_call the sum of its two calls) and the whole call.  Every pair's
strand and anchors from `auto` are compared with the two-call route's (reverse exactly when the marked call has more anchors); a difference fails
the run.  Synthetic pairs, 10 % error.
    python tools/bench_kmer_auto.py [pairs] [length] [ksz] [reps] [--out profiles/kmer_auto_bench_line.json]
Prints one JSON line; --out also writes it to a file."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bsalign_amd as B

argv = [a for a in sys.argv[1:]]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n = int(argv[0]) if len(argv) > 0 else 4096
L = int(argv[1]) if len(argv) > 1 else 10000
ksz = int(argv[2]) if len(argv) > 2 else 13
reps = int(argv[3]) if len(argv) > 3 else 5

logical = B.synth_pairs_host(n, L)
flipped = np.array([k % 2 == 1 for k in range(n)])
stored = [(B.revcomp(q) if f else q, t) for (q, t), f in zip(logical, flipped)]          # what a caller with unoriented reads holds
seqs, qoff, qlen, toff, tlen = B.pack_pairs(stored)
qoff_marked = qoff | np.uint64(B.QOFF_REVCOMP)
lib = B.lib()
ctx = B.Context(0)
cap = int(np.minimum(qlen, tlen).sum()) + 1
bufs = {k: (np.zeros(cap, np.uint64), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)) for k in ("auto", "plain", "marked")}


def call(name, qo, flags):
    maps, off, st = bufs[name]
    t0 = time.perf_counter()
    rc = lib.bsa_kmer_chain_batch2(ctx.h, B._p(seqs), seqs.nbytes, B._p(qo), B._p(qlen), B._p(toff), B._p(tlen), n, ksz, B._p(maps), cap, B._p(off), B._p(st), flags)
    dt = time.perf_counter() - t0
    assert rc == 0, (name, rc)
    ms, on_dev, on_host = ctx.last_kmer_chain_ms()
    return dt, ms, on_dev


def run(variant):
    if variant == "auto":
        return call("auto", qoff, B.KMER_STRAND_AUTO)
    if variant == "plain":
        return call("plain", qoff, 0)
    d0, m0, on_dev = call("plain", qoff, 0)
    d1, m1, _ = call("marked", qoff_marked, B.MODE_QSTRAND)
    t0 = time.perf_counter()
    cf, cr = np.diff(bufs["plain"][1]), np.diff(bufs["marked"][1])
    marks = cr > cf                                                  # the host's part of the two-call route
    d2 = time.perf_counter() - t0
    return d0 + d1 + d2, m0 + m1, on_dev


def same_as_two_call():
    (ma, oa, sa), (mp, op, _), (mm, om, _) = bufs["auto"], bufs["plain"], bufs["marked"]
    rev = np.diff(om) > np.diff(op)
    if not np.array_equal((sa & np.uint32(B.ST_REVCOMP)) != 0, rev):
        return False, rev
    cnt = np.where(rev, np.diff(om), np.diff(op))
    if not np.array_equal(np.diff(oa), cnt):
        return False, rev
    for k in range(n):
        src, so = (mm, om) if rev[k] else (mp, op)
        if not np.array_equal(ma[int(oa[k]):int(oa[k + 1])], src[int(so[k]):int(so[k + 1])]):
            return False, rev
    return True, rev


names = ("auto", "two_call", "plain")
for v in names:
    run(v)
wall = {k: [] for k in names}
kern = {k: [] for k in names}
on_dev, same, rev = 0, True, None
for r in range(reps):
    for v in names:
        dt, ms, on_dev = run(v)
        wall[v].append(dt)
        kern[v].append(ms)
    ok, rev = same_as_two_call()
    same &= ok
med = lambda v: float(np.median(v))
line = {"bench": "kmer_auto", "pairs": n, "length": L, "ksz": ksz, "reps": reps, "stored_reverse": int(flipped.sum()), "found_reverse": int(rev.sum()),
        "found_equals_stored": bool(np.array_equal(rev, flipped)), "pairs_on_device": on_dev, "identical_to_two_call": bool(same)}
for v in names:
    line[v] = {"chain_kernels_ms": round(med(kern[v]), 3), "chain_kernels_min_max_ms": [round(min(kern[v]), 3), round(max(kern[v]), 3)],
               "whole_call_s": round(med(wall[v]), 4), "pairs_per_s": round(n / med(wall[v]), 1)}
line["auto_over_two_call_kernels"] = round(med(kern["auto"]) / med(kern["two_call"]), 3)
line["auto_over_plain_kernels"] = round(med(kern["auto"]) / med(kern["plain"]), 3)
s = json.dumps(line)
print(s)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(s + "\n")
ctx.close()
sys.exit(0 if same else 1)
