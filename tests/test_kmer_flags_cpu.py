"""CPU: what the GPU tests of the flagged k-mer calls (test_kmer_flags_gpu.py) rest on -- the new symbol exists, the case builder stores what it says it
stores, and the marked cases are not vacuous.  Every anchor count here comes from the host chainer (bsa_kmer_chain) alone."""
import os

import numpy as np

import bsalign_amd as B
import kmer_chain_cases as KC
import kmer_flags_cases as F
import kmer_support as K
import support as S


def test_library_exports_and_header_declares_chain_batch2():
    lib = K.hostlib()
    assert hasattr(lib, "bsa_kmer_chain_batch2")
    hdr = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    assert "int bsa_kmer_chain_batch2(" in hdr
    assert (F.MODE_SEQ2BIT, F.MODE_QSTRAND, F.QOFF_REVCOMP) == (B.MODE_SEQ2BIT, B.MODE_QSTRAND, B.QOFF_REVCOMP)
    assert (B.MODE_SEQ2BIT | B.MODE_QSTRAND) & B.KMER_CHAIN_DEVICE == 0


def test_revcomp_and_packing_round_trip():
    rng = np.random.default_rng(1)
    for L in (0, 1, 31, 32, 33, 777):
        q = rng.integers(0, 4, L).astype(np.uint8)
        assert np.array_equal(F.revcomp(F.revcomp(q)), q)
        assert np.array_equal(F.revcomp(q), B.revcomp(q))
        if L:
            assert F.revcomp(q)[0] == 3 - q[-1]
        for off in (1, 3, 17, 31, 33, 63):
            x = np.concatenate([rng.integers(0, 4, off).astype(np.uint8), q, rng.integers(0, 4, 5).astype(np.uint8)])
            assert np.array_equal(B.unpack2bit(B.pack2bit(x), off, L), q)


def test_case_builder_is_sound():
    rng = np.random.default_rng(2)
    r = rng.integers(0, 4, 2000).astype(np.uint8)
    ta = S.mutate(rng, r, 0.05)
    tb = S.mutate(rng, F.revcomp(r), 0.05)
    pairs = [(r, ta), (F.revcomp(r), tb), (rng.integers(0, 4, 40).astype(np.uint8), rng.integers(0, 4, 33).astype(np.uint8)),
             (np.zeros(0, np.uint8), ta), (tb, np.zeros(0, np.uint8))]
    strands = [False, True, True, True, False]
    for packed in (False, True):
        for st in (strands, None):
            for guards in (False, True):
                b = F.build(pairs, st, packed, guards=guards)
                assert b.flags == (F.MODE_SEQ2BIT if packed else 0) | (F.MODE_QSTRAND if st is not None else 0)
                assert b.seqs.dtype == (np.uint64 if packed else np.uint8)
                for k, (q, t) in enumerate(pairs):
                    dq, dt = F.decode(b, k)
                    assert np.array_equal(dq, q) and np.array_equal(dt, t), (packed, k)
                    marked = bool(int(b.qoff[k]) >> 63)
                    assert marked == bool(st and st[k])
                    if marked:                                        # the stored bytes are the reverse complement, not the query
                        assert np.array_equal(b.stored[k], F.revcomp(q))
                    qo = int(b.qoff[k]) & ~F.QOFF_REVCOMP
                    lim = b.seqs.size * (32 if packed else 1)
                    assert qo + len(q) <= lim and int(b.toff[k]) + len(t) <= lim
                    if packed:
                        assert qo % 4 != 0 and int(b.toff[k]) % 4 != 0 and qo % 32 != 0
                if st is not None:
                    assert b.shared >= 1                              # r serves pair 0 forward and pair 1 marked
                    assert (int(b.qoff[0]) ^ int(b.qoff[1])) == F.QOFF_REVCOMP
                if packed and guards:
                    assert int(b.seqs[0]) == F.FRONT_GUARD and int(b.seqs[-1]) == F.BACK_GUARD
                    assert min(int(b.qoff[k]) & ~F.QOFF_REVCOMP for k in range(3)) >= 32
                    last = max(max((int(b.qoff[k]) & ~F.QOFF_REVCOMP) + int(b.qlen[k]), int(b.toff[k]) + int(b.tlen[k])) for k in range(len(pairs)))
                    assert (last + 31) // 32 <= b.seqs.size - 1       # no read reaches the guard word
                # the host-made blob the expectation runs on holds the logical pairs
                seqs, qoff, qlen, toff, tlen = b.plain
                for k, (q, t) in enumerate(pairs):
                    assert np.array_equal(seqs[int(qoff[k]):int(qoff[k]) + int(qlen[k])], q) and np.array_equal(seqs[int(toff[k]):int(toff[k]) + int(tlen[k])], t)


def test_marked_cases_are_not_vacuous():
    cs = {name: (q, t) for name, q, t in KC.cases(13)}
    q, t = cs["identical"]
    assert len(K.kmer_chain(13, q, t)) > 1800                         # sent marked, the pair is stored as revcomp(q) and chains as (q, t)
    b = F.build([(q, t)], [True])
    assert np.array_equal(b.stored[0], F.revcomp(q)) and len(K.kmer_chain(13, b.stored[0], t)) == 0
    # the stored bytes of `revcomp` are the reverse complement of their target: nothing unmarked, everything marked
    sq, t = cs["revcomp"]
    assert len(K.kmer_chain(13, sq, t)) == 0
    assert len(K.kmer_chain(13, F.revcomp(sq), t)) > 1800
    names, pairs, strands = F.named_pairs(13)
    assert len(pairs) == 2 * len(cs) and sum(strands) == len(cs)


def test_random_batch_has_anchors_on_marked_pairs():
    pairs, strands = F.random_pairs()
    assert len(pairs) == 300 and sum(strands) == 150
    for ksz in (8, 13):
        marked = [len(K.kmer_chain(ksz, q, t)) for (q, t), s in zip(pairs, strands) if s]
        assert 3 * sum(1 for c in marked if c) >= len(marked), (ksz, sum(1 for c in marked if c))
        # ... and the stored strand of those pairs chains to something else: the mark matters
        differ = sum(1 for (q, t), s in zip(pairs, strands) if s and len(K.kmer_chain(ksz, q, t)) != len(K.kmer_chain(ksz, F.revcomp(q), t)))
        assert 3 * differ >= len(marked)
    epairs, estrands = F.random_edit_pairs(31)
    assert len(epairs) == 3008 and sum(estrands) == 1504
    with_anchors = sum(1 for (q, t), s in zip(epairs, estrands) if s and len(K.kmer_chain(11, q, t)))
    assert 3 * with_anchors >= sum(estrands)
