"""Inputs for the k-mer calls with BSA_MODE_SEQ2BIT / BSA_MODE_QSTRAND (bsa_kmer_chain_batch2, bsa_kmer_edit_batch2); test code only.

A test states its pairs LOGICALLY: (q, t) is what the call has to chain or align.  build() turns them into what a caller holds: every read stored once
-- a marked pair's query stored as revcomp(q), so that the mark gives q back -- as 1 B/base bytes or as 2-bit words.  The expectation never comes from
the code under test: it is the host chainer (bsa_kmer_chain through kmer_support / kmer_chain_cases.host_arena) or bsa_kmer_edit_batch without flags on the
logical pairs, packed by the caller into a plain 1 B/base blob (Batch.plain).
"""
import numpy as np

import bsalign_amd as B
import kmer_chain_cases as KC
import support as S

MODE_SEQ2BIT, MODE_QSTRAND, QOFF_REVCOMP = 0x800, 0x2000, 1 << 63
COMBOS = (("strand", False, True), ("packed", True, False), ("both", True, True))      # name, packed, strand
FRONT_GUARD, BACK_GUARD = 0x5A5AA5A5C3C33C3C, 0xFFFFFFFFFFFFFFFF


def revcomp(x):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    return (3 - x[::-1]).astype(np.uint8)


class Batch:
    """seqs (uint8 bytes, or uint64 words when packed), qoff (bit 63 = the mark), qlen, toff, tlen, flags; stored[k] = the bytes stored for pair k's query;
    shared = stored reads that serve a forward pair AND a marked pair; plain = B.pack_pairs(logical pairs): the host-made 1 B/base blob"""


def build(pairs, strands=None, packed=False, lead=5, guards=False, seed=99):
    """pairs: logical (q, t); strands: a bool per pair or None (no BSA_MODE_QSTRAND).  A read whose stored bytes equal those of an earlier read is not
    stored again.  packed: reads start at base offsets that are no multiples of 4 (so none of 32), random bases between them; guards: a non-zero
    word in front of the first read's word and a word of ones behind the last word, both inside the blob and part of no read."""
    rng = np.random.default_rng(seed)
    n = len(pairs)
    marks = [bool(s) for s in strands] if strands is not None else [False] * n
    b = Batch()
    b.packed, b.strand = packed, strands is not None
    b.flags = (MODE_SEQ2BIT if packed else 0) | (MODE_QSTRAND if strands is not None else 0)
    b.qlen = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
    b.tlen = np.array([len(t) for _, t in pairs], dtype=np.uint32)
    b.qoff = np.zeros(n, dtype=np.uint64)
    b.toff = np.zeros(n, dtype=np.uint64)
    b.stored = []
    parts, acc, seen, use = [], 0, {}, {}
    if packed:
        parts.append(rng.integers(0, 4, lead).astype(np.uint8))
        acc = lead

    def put(x):
        nonlocal acc
        x = np.ascontiguousarray(x, dtype=np.uint8)
        key = x.tobytes()
        if len(x) and key in seen:
            return seen[key]
        if packed:
            pad = 3 + (1 if (acc + 3) % 4 == 0 else 0)
            parts.append(rng.integers(0, 4, pad).astype(np.uint8))
            acc += pad
        at = acc
        parts.append(x)
        acc += len(x)
        if len(x):
            seen[key] = at
        return at

    for k, (q, t) in enumerate(pairs):
        sq = revcomp(q) if marks[k] else np.ascontiguousarray(q, dtype=np.uint8)
        b.stored.append(sq)
        at = put(sq)
        if len(sq):
            use.setdefault(at, set()).add(marks[k])
        b.qoff[k] = at | (QOFF_REVCOMP if marks[k] else 0)
        b.toff[k] = put(t)
    b.shared = sum(1 for v in use.values() if len(v) == 2)
    codes = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if packed:
        words = B.pack2bit(codes)
        if guards:
            words = np.concatenate([np.array([FRONT_GUARD], np.uint64), words, np.array([BACK_GUARD], np.uint64)])
            b.qoff += np.uint64(32)
            b.toff += np.uint64(32)
        b.seqs = words if words.size else np.zeros(1, np.uint64)
    else:
        b.seqs = codes if codes.size else np.zeros(1, np.uint8)
    b.plain = B.pack_pairs([(np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)) for q, t in pairs])
    return b


def decode(b, k):
    """pair k as the call has to see it, read back from the stored blob: (q, t)"""
    qo = int(b.qoff[k]) & ~QOFF_REVCOMP
    mk = bool(int(b.qoff[k]) >> 63)
    if b.packed:
        q = B.unpack2bit(b.seqs, qo, int(b.qlen[k]))
        t = B.unpack2bit(b.seqs, int(b.toff[k]), int(b.tlen[k]))
    else:
        q = b.seqs[qo:qo + int(b.qlen[k])]
        t = b.seqs[int(b.toff[k]):int(b.toff[k]) + int(b.tlen[k])]
    return (revcomp(q) if mk else np.array(q, dtype=np.uint8)), np.array(t, dtype=np.uint8)


def named_pairs(ksz):
    """every case of KC.cases(ksz) once unmarked and once marked -> (names, logical pairs, strands)"""
    names, pairs, strands = [], [], []
    for name, q, t in KC.cases(ksz):
        for mk in (False, True):
            names.append(name + ("/marked" if mk else ""))
            pairs.append((q, t))
            strands.append(mk)
    return names, pairs, strands


def random_pairs(n=300, seed=77):
    """the batch of test_kmer_chain_gpu.test_random_batch_equals_the_host_chainer (lengths 20 .. 4000, divergence 0 / 5 / 15 / 40 %, every seventh
    pair with an insertion), every second pair marked.  The divergence mix is the existing one: at 0, 5 and 15 % a pair of more than a few hundred
    bases keeps unique 8- and 13-mers, so about three quarters of the marked pairs have anchors (test_kmer_flags_cpu asserts a third)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for it in range(n):
        L = int(rng.integers(20, 4000))
        T = rng.integers(0, 4, L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice([0.0, 0.05, 0.15, 0.40])))
        if it % 7 == 3 and len(Q) > 400:
            a = int(rng.integers(50, len(Q) - 100))
            Q = np.concatenate([Q[:a], rng.integers(0, 4, int(rng.integers(30, 600))).astype(np.uint8), Q[a:]])
        pairs.append((Q, T))
    return pairs, [k % 2 == 1 for k in range(n)]


def random_edit_pairs(seed, n=3000):
    """the batch of test_kmer_chain_gpu.test_edit_batch2_is_byte_identical_on_a_random_batch (clean bases), half marked, and its tail of special
    pairs without a base code above 3: empty sides, a sequence shorter than k, identical sequences"""
    rng = np.random.default_rng(seed)
    pairs = []
    for it in range(n):
        L = int(rng.integers(30, 700))
        T = rng.integers(0, 4, L).astype(np.uint8)
        Q = T.copy()
        m = rng.random(L) < float(rng.choice([0.0, 0.03, 0.10, 0.40]))
        Q[m] = (Q[m] + rng.integers(1, 4, int(m.sum()))) & 3
        if it % 5 == 1:
            a = int(rng.integers(0, L))
            Q = np.concatenate([Q[:a], rng.integers(0, 4, int(rng.integers(1, 80))).astype(np.uint8), Q[a:]])
        if it % 11 == 4:
            Q = np.delete(Q, slice(L // 3, L // 3 + int(rng.integers(1, 40))))
        pairs.append((Q, T))
    T = rng.integers(0, 4, 600).astype(np.uint8)
    tail = [(np.zeros(0, np.uint8), T), (T, np.zeros(0, np.uint8)), (T[:9].copy(), T), (T.copy(), T)]
    pairs += tail + tail
    strands = [k % 2 == 1 for k in range(n)] + [False] * len(tail) + [True] * len(tail)
    return pairs, strands


def bad_base_tail(seed=5):
    """pairs with a base code above 3 (1 B/base only).  -> (pairs, strands): unmarked as the existing test has them, and marked where q' is defined
    (a clean query against a target with such a code)"""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 4, 600).astype(np.uint8)
    b1, b2 = T.copy(), T.copy()
    b1[300] = 4
    b2[0] = 200
    pairs = [(b1, T), (T, b2), (b2, b1), (T, b1), (T, b2)]
    return pairs, [False, False, False, True, True]
