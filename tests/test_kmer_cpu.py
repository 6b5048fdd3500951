"""CPU: the host side of the k-mer anchored edit alignment (bsa_kmer_chain / bsa_kmer_segments / bsa_kmer_assemble in
bsalign_amd/csrc/bsa_kmer.cpp; reference kmer_striped_seqedit_pairwise, bsalign.h:1209-1536) against the committed
results of the real reference (tests/golden/kmer_edit.npz).  No GPU here: the alignments between the anchors are done
by the oracle's edit DP, which is what the device path is checked against elsewhere; tests/test_kmer_gpu.py runs the
same fixture through bsa_kmer_edit_batch."""
import os

import numpy as np
import pytest

import support as S
import kmer_support as K

GOLD = np.load(os.path.join(S.ROOT, "tests", "golden", "kmer_edit.npz"))


def golden_cases():
    seqs, meta = GOLD["seqs"], GOLD["meta"]
    for k, (ksz, qo, ql, to, tl) in enumerate(meta):
        yield k, int(ksz), seqs[qo:qo + ql], seqs[to:to + tl], GOLD["res"][k], GOLD["cigar"][GOLD["cigar_off"][k]:GOLD["cigar_off"][k + 1]]


def oracle_segment(qs, ts, mode):
    r, c, n = S.oracle_edit(qs, ts, mode, 0)
    assert n >= 0
    return r, c


def test_host_chain_and_stitch_equal_reference_fixture():
    nochain = 0
    for k, ksz, q, t, res, cig in golden_cases():
        r, c, maps = K.kmer_host(ksz, q, t, oracle_segment)
        assert np.array_equal(r, res), (k, ksz, r, res)
        assert np.array_equal(c, cig), (k, ksz)
        nochain += len(maps) == 0
        # anchors are strictly increasing in both sequences and really are shared k-mers
        kk = min(ksz, 15)
        qo, to = (maps >> np.uint64(32)).astype(np.int64), (maps & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.all(np.diff(qo) > 0) and np.all(np.diff(to) > 0)
        for a, b in zip(qo[:5], to[:5]):
            assert np.array_equal(q[a:a + kk], t[b:b + kk])
    assert 0 < nochain < len(GOLD["meta"])          # the fixture covers both outcomes


def test_stitched_cigar_spans_the_result():
    for k, ksz, q, t, res, cig in golden_cases():
        r, c, _ = K.kmer_host(ksz, q, t, oracle_segment)
        qn, tn = S.cigar_spans(c)
        # the reference drops target bases next to an empty query stretch from the CIGAR (an empty side returns the
        # zero result, bsalign.h:1051-1054), so only the query side is exact
        assert qn == r[2] - r[1] or r[9] == 0, (k, qn, r)
        assert r[9] == r[5] + r[6] + r[7] + r[8]


def test_segments_of_a_hand_made_chain():
    # anchors at (10,12) and (11,13) are adjacent: the second one adds a match but no segment
    maps = np.array([(10 << 32) | 12, (11 << 32) | 13, (40 << 32) | 45], dtype=np.uint64)
    segs = K.kmer_segments(5, maps, 60, 70)
    got = [(int(s["qb"]), int(s["qe"]), int(s["tb"]), int(s["te"]), int(s["mode"]), int(s["ml"])) for s in segs]
    assert got == [
        (0, 12, 0, 14, S.MODE_EXTEND | K.SEG_REVERSED, 1),     # head, aligned reversed
        (14, 42, 16, 47, S.MODE_GLOBAL, 2),                    # gap; the two anchor columns 12 and 13 go in front of it
        (43, 60, 48, 70, S.MODE_EXTEND, 0),                    # tail
    ]
    # no anchors: one global alignment of the whole pair
    segs = K.kmer_segments(5, np.zeros(0, dtype=np.uint64), 60, 70)
    assert [(int(s["qb"]), int(s["qe"]), int(s["tb"]), int(s["te"]), int(s["mode"]), int(s["ml"])) for s in segs] == [(0, 60, 0, 70, S.MODE_GLOBAL, 0)]


def test_short_and_degenerate_inputs_have_no_chain():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 4, 7).astype(np.uint8)
    assert len(K.kmer_chain(13, q, q)) == 0                     # shorter than k
    z = np.zeros(300, dtype=np.uint8)
    assert len(K.kmer_chain(11, z, z)) == 0                     # one repeated k-mer
    t = rng.integers(0, 4, 400).astype(np.uint8)
    rc = (3 - t)[::-1].copy()
    assert len(K.kmer_chain(13, rc, t)) == 0                    # only reverse-strand matches
    assert len(K.kmer_chain(13, t, t)) == 400 - 13 + 1          # identical: every k-mer is an anchor


def test_host_pieces_against_the_live_reference():
    """(without the reference build: its answers to these very calls, tests/golden/ref_calls_kmer.npz)"""
    ref_kmer_edit = S.RefCalls("ref_calls_kmer", K.ref_kmer_edit)
    rng = np.random.default_rng(77)
    for it in range(120):
        L = int(rng.integers(20, 2500))
        T = rng.integers(0, 4, L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice([0.0, 0.03, 0.1, 0.2])))
        if it % 4 == 1 and len(Q) > 200:
            a = int(rng.integers(20, len(Q) - 100))
            Q = np.concatenate([Q[:a], rng.integers(0, 4, int(rng.integers(30, 200))).astype(np.uint8), Q[a:]])
        if len(Q) == 0:
            continue
        ksz = int(rng.choice([4, 7, 10, 13, 15]))
        r0, c0 = ref_kmer_edit(ksz, Q, T)[:2]
        r1, c1, _ = K.kmer_host(ksz, Q, T, oracle_segment)
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (it, ksz, L)
