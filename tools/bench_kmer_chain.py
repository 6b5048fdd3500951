"""Where the k-mer anchored edit alignment spends its time: the chaining stage on the host route (bsa_kmer_chain, 16 threads over pairs) against the
device route (bsa_kmer_chain_batch: upload, kernels, anchor download), the device kernels alone, and the whole call -- bsa_kmer_edit_batch against
bsa_kmer_edit_batch2 with BSA_KMER_CHAIN_DEVICE -- in one process, interleaved, median of the repetitions.  Synthetic pairs, 10 % error.
    python tools/bench_kmer_chain.py [pairs] [length] [ksz] [reps] [--out profiles/kmer_chain_bench_line.json]
Prints one JSON line; --out also writes it to a file."""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

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

pairs = B.synth_pairs_host(n, L)
seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
lib = B.lib()
lib.bsa_kmer_chain.restype = C.c_uint32
ctx = B.Context(0)
u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
base = seqs.ctypes.data


def host_stage():
    """the chaining of every pair by the host code, THREADS threads over pairs (ctypes releases the GIL)"""
    def work(lo, hi):
        maps = np.zeros(L + 64, dtype=np.uint64)
        tot = 0
        for k in range(lo, hi):
            tot += lib.bsa_kmer_chain(C.c_uint32(ksz), C.cast(base + int(qoff[k]), u8p), C.c_uint32(int(qlen[k])), C.cast(base + int(toff[k]), u8p),
                                      C.c_uint32(int(tlen[k])), C.cast(maps.ctypes.data, u64p), C.c_uint32(len(maps)))
        return tot
    step = 64
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        tot = sum(ex.map(lambda lo: work(lo, min(n, lo + step)), range(0, n, step)))
    return time.perf_counter() - t0, tot


cap = int(np.minimum(qlen, tlen).sum()) + 1
maps = np.zeros(cap, dtype=np.uint64)
moff = np.zeros(n + 1, dtype=np.uint64)


def device_stage():
    t0 = time.perf_counter()
    rc = lib.bsa_kmer_chain_batch(ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, ksz, B._p(maps), cap, B._p(moff), None)
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt, int(moff[n])


par = B.KmerParams()
par.ksz, par.threads = ksz, THREADS
res = np.zeros(n, dtype=B.RESULT_DTYPE)
ccap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
cig = np.zeros(ccap, dtype=np.uint32)
coff = np.zeros(n + 1, dtype=np.uint64)
st = np.zeros(n, dtype=np.uint32)


def whole(flags):
    t0 = time.perf_counter()
    rc = lib.bsa_kmer_edit_batch2(ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(par), B._p(res), B._p(cig), ccap,
                                  B._p(coff), B._p(st), flags)
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt, res.tobytes(), cig[:int(coff[n])].tobytes()


# warm-up: allocations, code objects, page faults of the host arrays
device_stage()
whole(0)
whole(B.KMER_CHAIN_DEVICE)
th, td, tk, w0, w1 = [], [], [], [], []
same = True
for r in range(reps):
    a, words_h = host_stage()
    b, words_d = device_stage()
    ms, on_dev, on_host = ctx.last_kmer_chain_ms()
    same &= words_h == words_d
    c, r0, c0 = whole(0)
    d, r1, c1 = whole(B.KMER_CHAIN_DEVICE)
    same &= r0 == r1 and c0 == c1
    th.append(a); td.append(b); tk.append(ms / 1e3); w0.append(c); w1.append(d)
med = lambda v: float(np.median(v))
line = {
    "bench": "kmer_chain", "pairs": n, "length": L, "ksz": ksz, "reps": reps, "host_threads": THREADS,
    "chain_host_s": round(med(th), 4), "chain_device_s": round(med(td), 4), "chain_device_kernels_s": round(med(tk), 4),
    "chain_host_min_max_s": [round(min(th), 4), round(max(th), 4)], "chain_device_min_max_s": [round(min(td), 4), round(max(td), 4)],
    "pairs_on_device": on_dev, "pairs_on_host": on_host,
    "edit_batch_pairs_per_s": round(n / med(w0), 1), "edit_batch2_device_chain_pairs_per_s": round(n / med(w1), 1),
    "edit_batch_s": round(med(w0), 4), "edit_batch2_device_chain_s": round(med(w1), 4),
    "same_anchor_count_and_bytes": bool(same),
}
s = json.dumps(line)
print(s)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(s + "\n")
ctx.close()
