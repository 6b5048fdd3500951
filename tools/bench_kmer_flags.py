"""What BSA_MODE_QSTRAND / BSA_MODE_SEQ2BIT cost (or save) in the k-mer anchored edit alignment: bsa_kmer_edit_batch2 with BSA_KMER_CHAIN_DEVICE on a
blob in which every second query is stored reverse-complemented and marked -- 1 B/base + strand, packed, packed + strand -- each against the same call
without those flags on the host-made 1 B/base blob of the pairs as they are aligned.  One process, one warm-up call each, median of the repetitions,
calls interleaved.  Reported per variant: the chain kernels' time (bsa_ctx_last_kmer_chain_ms) and whole-call pairs/s; every pair's record, status and
CIGAR words are compared with the baseline's.  Synthetic pairs, 10 % error.
    python tools/bench_kmer_flags.py [pairs] [length] [ksz] [reps] [--out profiles/kmer_flags_bench_line.json]
Prints one JSON line; --out also writes it to a file."""
import ctypes as C
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
THREADS = 16

logical = B.synth_pairs_host(n, L)                                   # what every variant aligns
strands = [k % 2 == 1 for k in range(n)]
stored = [(B.revcomp(q) if s else q, t) for (q, t), s in zip(logical, strands)]          # what a caller with stranded reads holds
blobs = {
    "plain": (B.pack_pairs(logical), 0),
    "strand": (B.pack_pairs(stored, False, strands), B.MODE_QSTRAND),
    "packed": (B.pack_pairs(logical, True), B.MODE_SEQ2BIT),
    "packed_strand": (B.pack_pairs(stored, True, strands), B.MODE_SEQ2BIT | B.MODE_QSTRAND),
}
lib = B.lib()
ctx = B.Context(0)
par = B.KmerParams()
par.ksz, par.threads = ksz, THREADS
qlen, tlen = blobs["plain"][0][2], blobs["plain"][0][4]
ccap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
res = np.zeros(n, dtype=B.RESULT_DTYPE)
cig = np.zeros(ccap, dtype=np.uint32)
coff = np.zeros(n + 1, dtype=np.uint64)
st = np.zeros(n, dtype=np.uint32)


def whole(name):
    (seqs, qoff, ql, toff, tl), flags = blobs[name]
    t0 = time.perf_counter()
    rc = lib.bsa_kmer_edit_batch2(ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(ql), B._p(toff), B._p(tl), n, C.byref(par), B._p(res), B._p(cig), ccap,
                                  B._p(coff), B._p(st), flags | B.KMER_CHAIN_DEVICE)
    dt = time.perf_counter() - t0
    assert rc == 0, (name, rc)
    ms, on_dev, on_host = ctx.last_kmer_chain_ms()
    return dt, ms, on_dev, (res.tobytes(), st.tobytes(), coff.tobytes(), cig[:int(coff[n])].tobytes())


names = list(blobs)
for name in names:                                                   # warm-up: allocations, code objects, page faults of the host arrays
    whole(name)
wall = {k: [] for k in names}
kern = {k: [] for k in names}
same = {k: True for k in names}
on_dev = 0
for r in range(reps):
    base = None
    for name in names:
        dt, ms, on_dev, out = whole(name)
        wall[name].append(dt)
        kern[name].append(ms)
        if name == "plain":
            base = out
        else:
            same[name] &= out == base                                # every pair: records, status, cigar_off and CIGAR words
med = lambda v: float(np.median(v))
line = {"bench": "kmer_flags", "pairs": n, "length": L, "ksz": ksz, "reps": reps, "host_threads": THREADS, "marked_pairs": int(sum(strands)),
        "pairs_on_device": on_dev, "blob_bytes": {k: int(blobs[k][0][0].nbytes) for k in names}}
for name in names:
    line[name] = {"chain_kernels_ms": round(med(kern[name]), 3), "chain_kernels_min_max_ms": [round(min(kern[name]), 3), round(max(kern[name]), 3)],
                  "whole_call_s": round(med(wall[name]), 4), "pairs_per_s": round(n / med(wall[name]), 1)}
    if name != "plain":
        line[name]["identical_to_plain"] = bool(same[name])
s = json.dumps(line)
print(s)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(s + "\n")
ctx.close()
sys.exit(0 if all(same[k] for k in names if k != "plain") else 1)
