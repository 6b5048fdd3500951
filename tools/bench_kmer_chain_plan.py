"""The k-mer chain call on a resident blob (bsa_kmer_chain_plan_create / bsa_kmer_chain_run) beside the host-pointer call on the same pairs
(bsa_kmer_chain_batch: pack, upload, kernels, a synchronise per chunk, anchor download), in one process, interleaved, median of the repetitions:
  (a) host_pointer_s   bsa_kmer_chain_batch, wall time of the call (it synchronises itself), and its kernels by bsa_ctx_last_kmer_chain_ms;
  (b) resident_s       bsa_kmer_chain_run, wall time from the call to the end of bsa_ctx_sync -- the blob, the arena, the offsets and the status words
                       stay on the device;
  (c) resident_kernels_s   (b)'s kernels by bsa_ctx_last_kmer_chain_ms.
The plan is made once, outside the timed window (plan_create_s says what that costs).  Synthetic pairs, 10 % error.  The anchors of the two routes
are compared word for word after the timed loop.
    python tools/bench_kmer_chain_plan.py [pairs] [length] [ksz] [reps] [--out profiles/kmer_chain_plan_bench_line.json]
Prints one JSON line; --out also writes it to a file."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
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

pairs = B.synth_pairs_host(n, L)
seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
lib = B.lib()
ctx = B.Context(0)

cap = B.kmer_chain_words_bound(qlen, tlen) + 1
maps = np.zeros(cap, dtype=np.uint64)
moff = np.zeros(n + 1, dtype=np.uint64)
mst = np.zeros(n, dtype=np.uint32)


def host_pointer():
    t0 = time.perf_counter()
    rc = lib.bsa_kmer_chain_batch(ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, ksz, B._p(maps), cap, B._p(moff), B._p(mst))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt, ctx.last_kmer_chain_ms()


d_seqs = torch.from_numpy(seqs).cuda()
d_maps = torch.zeros(cap, dtype=torch.int64, device="cuda")
d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
t0 = time.perf_counter()
plan = B.KmerChainPlan(ctx, qoff, qlen, toff, tlen, ksz=ksz)
t_create = time.perf_counter() - t0


def resident():
    t0 = time.perf_counter()
    plan.run(d_seqs, d_maps, d_off, d_st)
    t1 = time.perf_counter()
    ctx.sync()
    dt = time.perf_counter() - t0
    return dt, t1 - t0, ctx.last_kmer_chain_ms()


# warm-up: allocations (the context's scratch grows to the larger of the two routes' needs), code objects, page faults of the host arrays
host_pointer()
resident()
host_pointer()
resident()
ta, tak, tb, tbe, tbk = [], [], [], [], []
for r in range(reps):
    a, (ams, adev, ahost) = host_pointer()
    b, enq, (bms, bdev, bhost) = resident()
    ta.append(a); tak.append(ams / 1e3); tb.append(b); tbe.append(enq); tbk.append(bms / 1e3)
torch.cuda.synchronize()
off = d_off.cpu().numpy().view(np.uint64)
same = bool(np.array_equal(off, moff) and np.array_equal(d_st.cpu().numpy().view(np.uint32), mst)
            and np.array_equal(d_maps.cpu().numpy().view(np.uint64)[:int(moff[n])], maps[:int(moff[n])]))
med = lambda v: float(np.median(v))
line = {
    "bench": "kmer_chain_plan", "pairs": n, "length": L, "ksz": ksz, "reps": reps, "plan_chunks": plan.chunks(), "anchor_words": int(moff[n]),
    "host_pointer_s": round(med(ta), 4), "host_pointer_min_max_s": [round(min(ta), 4), round(max(ta), 4)], "host_pointer_kernels_s": round(med(tak), 4),
    "resident_s": round(med(tb), 4), "resident_min_max_s": [round(min(tb), 4), round(max(tb), 4)], "resident_kernels_s": round(med(tbk), 4),
    "resident_enqueue_s": round(med(tbe), 5), "plan_create_s": round(t_create, 4),
    "host_pointer_pairs_per_s": round(n / med(ta), 1), "resident_pairs_per_s": round(n / med(tb), 1),
    "pairs_on_device_host_pointer": [adev, ahost], "pairs_on_device_resident": [bdev, bhost],
    "same_words_offsets_status": same,
}
s = json.dumps(line)
print(s)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(s + "\n")
plan.close()
ctx.close()
assert same, "the resident run and the host-pointer call disagree"
