"""Inputs and reference statements for the device k-mer chainer (bsa_kmer_chain_batch, bsa_kmer_edit_batch2); test code only.

host_arena()  -- the packed-arena contract of bsa_kmer_chain_batch in NumPy on top of per-pair bsa_kmer_chain calls (no GPU):
                 maps, maps_off, status, and the return code / maps_off[n] for a given maps_cap.
chain_py()    -- a restatement of bsa_kmer.cpp's chain() that also COUNTS what the product cannot tell: the diagonal filter's
                 iterations and how often the LIS bisection runs / stops on equality.  Only for clean bases (codes 0..3).
cases(ksz)    -- the named pairs test_kmer_chain_gpu.py sends at one k-mer size.
"""
import numpy as np

import kmer_support as K
import support as S

ST_BAD_BASE, ST_EMPTY = 1, 2
E_CIGAR_CAP = -5
DEV_MAX = 1 << 18          # qlen + tlen the device route takes (include/bsalign_hip.h)


def host_status(q, t):
    q = np.asarray(q, dtype=np.uint8)
    t = np.asarray(t, dtype=np.uint8)
    bad = (q.size and int(q.max()) > 3) or (t.size and int(t.max()) > 3)
    return (ST_BAD_BASE if bad else 0) | (ST_EMPTY if (q.size == 0 or t.size == 0) else 0)


def host_arena(pairs, ksz, maps_cap=None):
    """-> (rc, maps, maps_off, status): what bsa_kmer_chain_batch has to return for these pairs; with maps_cap too small rc is
    E_CIGAR_CAP, maps is empty and maps_off[n] the number of words needed"""
    per, st = [], []
    for q, t in pairs:
        s = host_status(q, t)
        st.append(s)
        per.append(np.zeros(0, np.uint64) if s else K.kmer_chain(ksz, q, t) if ksz else np.zeros(0, np.uint64))
    off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    if per:
        off[1:] = np.cumsum([len(m) for m in per])
    status = np.array(st, dtype=np.uint32)
    if maps_cap is not None and int(off[-1]) > maps_cap:
        return E_CIGAR_CAP, np.zeros(0, np.uint64), off, status
    maps = np.concatenate(per) if per else np.zeros(0, np.uint64)
    return 0, maps.astype(np.uint64), off, status


def _kmers(seq, ksz):
    n = len(seq) - ksz + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    s = seq.astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    rev = np.zeros(n, np.uint64)
    for m in range(ksz):
        b = s[m:m + n]
        fwd |= b << np.uint64(2 * (ksz - 1 - m))
        rev |= (np.uint64(3) - b) << np.uint64(2 * m)
    d = rev < fwd
    return np.where(d, rev, fwd) & np.uint64(0x3FFFFFFF), d


def chain_py(ksz, q, t):
    """-> (maps, info); info: hits, filter_iters (passes of the diagonal filter, the last one drops nothing), lis_search (hits that took the
    bisection), lis_equal (bisections that stopped on equality), dup_toff (hits sharing a target offset)"""
    q = np.asarray(q, dtype=np.uint8)
    t = np.asarray(t, dtype=np.uint8)
    assert (q.size == 0 or q.max() <= 3) and (t.size == 0 or t.max() <= 3)
    info = dict(hits=0, filter_iters=0, lis_search=0, lis_equal=0, dup_toff=0)
    none = np.zeros(0, np.uint64)
    ksz = min(ksz, 15)
    if ksz == 0:
        return none, info
    cmin = min(int(min(len(q), len(t)) * 0.05 + 1), 2 * ksz)
    kq, dq = _kmers(q, ksz)
    kt, dt = _kmers(t, ksz)
    if kq.size == 0 or kt.size == 0:
        return none, info
    top = max(int(kq.max()), int(kt.max()))
    uq, iq, cq = np.unique(kq, return_index=True, return_counts=True)
    ut, it, ct = np.unique(kt, return_index=True, return_counts=True)
    _, a, b = np.intersect1d(uq[cq == 1], ut[ct == 1], return_indices=True)
    km = uq[cq == 1][a]
    qo = iq[cq == 1][a]
    to = it[ct == 1][b]
    ok = dq[qo] == dt[to]
    if top == 0:
        ok &= km != 0            # the zeroed sentinel: a run of k-mer 0 that reaches the end is never closed
    qo, to = qo[ok], to[ok]
    order = np.argsort(qo, kind="stable")
    qo = [int(x) for x in qo[order]]
    to = [int(x) for x in to[order]]
    n = len(qo)
    info["hits"] = n
    info["dup_toff"] = n - len(set(to))
    if n * ksz < cmin:
        return none, info
    NONE = -1
    tail, prev = [0], [NONE] * n
    for i in range(1, n):
        tv = to[i]
        if tv > to[tail[-1]]:
            prev[i] = tail[-1]
            tail.append(i)
        elif tv <= to[tail[0]]:
            prev[i] = NONE
            tail[0] = i
        else:
            info["lis_search"] += 1
            lo, hi = 0, len(tail)
            while lo < hi:
                m = lo + ((hi - lo) >> 1)
                if tv > to[tail[m]]:
                    lo = m + 1
                elif tv < to[tail[m]]:
                    hi = m
                else:
                    lo = m
                    info["lis_equal"] += 1
                    break
            prev[i] = prev[tail[lo - 1]]
            tail[lo] = i
    keep = [False] * n
    cov, e, m = 0, 0xFFFFFFFF, tail[-1]
    while m != NONE:
        keep[m] = True
        cov += ksz if to[m] + ksz <= e else e - to[m]
        e = to[m]
        m = prev[m]
    if cov < cmin:
        return none, info
    while True:
        d = [qo[i] - to[i] for i in range(n) if keep[i]]
        if len(d) * ksz < cmin:
            break
        info["filter_iters"] += 1
        tot = sum(d)
        mean = abs(tot) // len(d) * (1 if tot >= 0 else -1)          # C's truncating division
        median = sorted(d)[len(d) // 2]
        var = max(abs(median - mean) * 3, 50)
        dropped = 0
        for i in range(n):
            if keep[i] and abs(qo[i] - to[i] - mean) > var:
                keep[i] = False
                dropped += 1
        if dropped == 0:
            break
    ks = [i for i in range(n) if keep[i]]
    cov, e = 0, 0
    for i in ks:
        cov += ksz if to[i] >= e + ksz else to[i] + ksz - e
        e = to[i] + ksz
    if cov < cmin:
        return none, info
    return np.array([(qo[i] << 32) | to[i] for i in ks], dtype=np.uint64), info


def staircase_pair(seed=7, L=6000):
    """80 % of the target on diagonal 0, 15 % behind a 200-base insertion, 5 % behind another 1800 bases: the filter drops the far
    group first and, with the mean pulled back, the near one in a second pass"""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 4, L).astype(np.uint8)
    a, b = int(L * 0.80), int(L * 0.95)
    Q = np.concatenate([T[:a], rng.integers(0, 4, 200).astype(np.uint8), T[a:b], rng.integers(0, 4, 1800).astype(np.uint8), T[b:]])
    return Q, T


def crossing_pair(seed=11, L=3000):
    """two blocks of the target swapped in the query: hits whose target offsets fall back, so the LIS bisection runs"""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 4, L).astype(np.uint8)
    Q = np.concatenate([T[:1000], T[1400:1700], T[1000:1400], T[1700:]])
    return S.mutate(rng, Q, 0.03), T


def cases(ksz, with_long=True):
    """[(name, q, t)]: the lengths 0, ksz - 1, ksz, 50, 1 k, 10 k (and one 30 k pair) at divergence 0 / 5 / 15 / 40 %, identical sequences,
    a reverse-complement query, poly-A and a period-2 repeat, the staircase and the crossing pair"""
    k = min(ksz, 15)
    rng = np.random.default_rng(1000 + ksz)
    out = []
    for L in (0, k - 1, k, 50, 1000, 10000):
        for div in (0.0, 0.05, 0.15, 0.40):
            T = rng.integers(0, 4, L).astype(np.uint8)
            Q = S.mutate(rng, T, div) if div else T.copy()
            out.append(("L%d_d%02d" % (L, int(div * 100)), Q, T))
    # one side empty / shorter than the k-mer, the other not
    T = rng.integers(0, 4, 300).astype(np.uint8)
    out.append(("empty_q", np.zeros(0, np.uint8), T))
    out.append(("short_t", T, T[:k - 1].copy()))
    if with_long:
        T = rng.integers(0, 4, 30000).astype(np.uint8)
        out.append(("L30000_d05", S.mutate(rng, T, 0.05), T))
    T = rng.integers(0, 4, 2000).astype(np.uint8)
    out.append(("identical", T.copy(), T))
    out.append(("revcomp", (3 - T[::-1]).astype(np.uint8), T))
    out.append(("polyA", np.zeros(500, np.uint8), np.zeros(400, np.uint8)))
    out.append(("polyA_k", np.zeros(k, np.uint8), np.zeros(k, np.uint8)))          # one k-mer 0 each: the run the sentinel never closes
    out.append(("polyA_in_random", np.concatenate([T[:700], np.zeros(k, np.uint8), T[700:]]), np.concatenate([T[:900], np.zeros(k, np.uint8), T[900:]])))
    p2 = np.tile(np.array([0, 1], np.uint8), 300)
    out.append(("period2", p2, p2[:500].copy()))
    out.append(("period2_shift", p2, p2[1:401].copy()))
    out.append(("staircase",) + staircase_pair())
    out.append(("crossing",) + crossing_pair())
    return out
