"""Inputs for the k-mer calls with BSA_KMER_STRAND_AUTO (bsa_kmer_chain_batch2, bsa_kmer_edit_batch2); test code only.

A test states its pairs as they are STORED: (q, t), the call has to find out whether it chains q or revcomp(q).  The expectation never comes from the
code under test: expected() runs the host chainer (bsa_kmer_chain) on (q, t) and on a host-made (revcomp(q), t), reverse exactly when the second list
is longer; the edit expectation is bsa_kmer_edit_batch without flags on a host-made 1 B/base blob that holds each pair on its expected strand.
"""
import numpy as np

import kmer_chain_cases as KC
import kmer_flags_cases as F
import kmer_support as K
import support as S

KMER_STRAND_AUTO, ST_REVCOMP = 2, 16
EXTRA = ("palindrome", "both_fwd_wins", "both_rev_wins", "empty_both", "tie_with_anchors")


def extra_cases(seed=4242):
    """the pairs that only this flag can get wrong -> [(name, q, t)]"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    out = []
    x = rnd(1000)
    t = np.concatenate([x, F.revcomp(x)])
    # revcomp(q) == q: both strands give the same list, the tie is forward.  That list is EMPTY, and has to be: in a sequence that equals its own reverse
    # complement every canonical k-mer occurs at least twice (at p and at len - ksz - p), so none is unique.  The tie with anchors is the last case.
    out.append(("palindrome", t.copy(), t))
    for name, la, lb in (("both_fwd_wins", 1500, 600), ("both_rev_wins", 600, 1500)):
        a, b = rnd(la), rnd(lb)
        out.append((name, np.concatenate([a, b]), np.concatenate([S.mutate(rng, a, 0.03), F.revcomp(b)])))
    out.append(("empty_both", rnd(900), rnd(1100)))
    # q = a + b against t = a + revcomp(b), 1000 bases each: a chains forward, b chains reverse.  At this seed both strands keep exactly as many anchors
    # at ksz 8, 13 and 15 (test_kmer_auto_cpu asserts it with the host chainer): a tie of more than 500 a side, which has to come out forward.
    r2 = np.random.default_rng(14)
    a, b = r2.integers(0, 4, 1000).astype(np.uint8), r2.integers(0, 4, 1000).astype(np.uint8)
    out.append(("tie_with_anchors", np.concatenate([a, b]), np.concatenate([a, F.revcomp(b)])))
    return out


def named_pairs(ksz):
    """every case of KC.cases(ksz) stored as it is and stored with the query reverse-complemented, plus the extra cases -> (names, stored pairs)"""
    names, pairs = [], []
    for name, q, t in KC.cases(ksz):
        names += [name, name + "/rc"]
        pairs += [(q, t), (F.revcomp(q), t)]
    for name, q, t in extra_cases():
        names.append(name)
        pairs.append((q, t))
    return names, pairs


def random_pairs(n=300, seed=77, pick=123):
    """the 300 pairs of F.random_pairs, a seeded random half stored reverse-complemented -> (stored pairs, which were flipped)"""
    pairs, _ = F.random_pairs(n, seed)
    flip = np.zeros(n, dtype=bool)
    flip[np.random.default_rng(pick).permutation(n)[:n // 2]] = True
    return [(F.revcomp(q) if f else q, t) for (q, t), f in zip(pairs, flip)], flip


def random_edit_pairs(seed, n=3000, pick=321):
    """the pairs of F.random_edit_pairs (clean bases, with its tail of special pairs), a seeded random half stored reverse-complemented"""
    pairs, _ = F.random_edit_pairs(seed, n)
    flip = np.zeros(len(pairs), dtype=bool)
    flip[np.random.default_rng(pick).permutation(len(pairs))[:len(pairs) // 2]] = True
    return [(F.revcomp(q) if f else q, t) for (q, t), f in zip(pairs, flip)], flip


def both_strands(pairs, ksz):
    """-> (F, R): per pair the host chainer's anchors of (q, t) and of (revcomp(q), t); none for an empty pair or one with a base code above 3"""
    fw, rv = [], []
    none = np.zeros(0, np.uint64)
    for q, t in pairs:
        if KC.host_status(q, t) or not ksz:
            fw.append(none)
            rv.append(none)
        else:
            fw.append(K.kmer_chain(ksz, q, t))
            rv.append(K.kmer_chain(ksz, F.revcomp(q), t))
    return fw, rv


def expected(pairs, ksz, strands=None):
    """-> (maps_off, [anchors of pair k], status without ST_REVCOMP, strands): what the flagged chain call has to return for the stored pairs"""
    fw, rv = both_strands(pairs, ksz)
    if strands is None:
        strands = np.array([len(r) > len(f) for f, r in zip(fw, rv)], dtype=bool)
    per = [r if s else f for f, r, s in zip(fw, rv, strands)]
    off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    if per:
        off[1:] = np.cumsum([len(m) for m in per])
    status = np.array([KC.host_status(q, t) for q, t in pairs], dtype=np.uint32)
    return off, per, status, strands


def on_strand(pairs, strands):
    """the pairs as the call aligns them: revcomp(q) where the strand is reverse"""
    return [(F.revcomp(q) if s else np.ascontiguousarray(q, dtype=np.uint8), t) for (q, t), s in zip(pairs, strands)]
