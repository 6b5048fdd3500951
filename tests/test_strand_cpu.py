"""BSA_MODE_QSTRAND without a GPU: the flag and the offset bit are the same numbers in the header and in Python and collide with no
other mode bit; revcomp is the reference's reverse complement; pack_pairs(strands=...) stores every query once, forward, and marks only
the offsets it was asked to; and the coordinate rule of the header -- qb / qe are positions in the reverse complement, the interval on
the stored strand is [qlen - qe, qlen - qb) -- checked with the oracle."""
import os
import re

import numpy as np

import support as S


def _header():
    return open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()


def test_constants_match_the_header_and_collide_with_nothing():
    import bsalign_amd as B
    hdr = _header()
    modes = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(BSA_MODE_[A-Z0-9_]+)\s+(0x[0-9A-Fa-f]+|\d+)", hdr)}
    assert modes["BSA_MODE_QSTRAND"] == B.MODE_QSTRAND == 0x2000
    assert B.MODE_QSTRAND & 3 == 0
    assert all(v & B.MODE_QSTRAND == 0 for k, v in modes.items() if k != "BSA_MODE_QSTRAND"), modes
    # ... nor with the Python mirror's own flags
    for name in ("MODE_ROWRECORDS", "MODE_SCORE_ONLY", "MODE_SEQ2BIT", "MODE_CIGAR_EQX"):
        assert getattr(B, name) & B.MODE_QSTRAND == 0, name
    m = re.search(r"#define\s+BSA_QOFF_REVCOMP\s+\(1ull\s*<<\s*(\d+)\)", hdr)
    assert m and int(m.group(1)) == 63
    assert B.QOFF_REVCOMP == 1 << 63


def test_revcomp_is_an_involution_and_the_reference_complement():
    import bsalign_amd as B
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 15, 16, 17, 33, 1000):
        q = rng.integers(0, 4, size=n).astype(np.uint8)
        r = B.revcomp(q)
        assert r.dtype == np.uint8 and r.flags["C_CONTIGUOUS"]
        assert np.array_equal(r, (3 - q[::-1].astype(np.int64)).astype(np.uint8))
        assert np.array_equal(r, (~q[::-1]) & 3)                 # (~c) & 3, the reference's dna.h
        assert np.array_equal(B.revcomp(r), q)
    assert [int(x) for x in B.revcomp(np.array([0, 0, 1, 3], np.uint8))] == [0, 2, 3, 3]       # AACT -> AGTT


def test_pack_pairs_stores_queries_forward_and_marks_only_what_was_asked():
    import bsalign_amd as B
    rng = np.random.default_rng(12)
    pairs = [(rng.integers(0, 4, size=int(rng.integers(1, 200))).astype(np.uint8),
              rng.integers(0, 4, size=int(rng.integers(1, 200))).astype(np.uint8)) for _ in range(50)]
    strands = rng.random(len(pairs)) < 0.5
    strands[0], strands[1] = True, False
    bit = np.uint64(B.QOFF_REVCOMP)
    for seq2bit in (False, True):
        plain = B.pack_pairs(pairs, seq2bit)
        seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs, seq2bit, strands)
        # the same blob: nothing was reverse-complemented or stored twice
        assert np.array_equal(seqs, plain[0]) and np.array_equal(toff, plain[3])
        assert np.array_equal(qlen, plain[2]) and np.array_equal(tlen, plain[4])
        assert np.array_equal((qoff & bit) != 0, strands)
        assert np.array_equal(qoff & ~bit, plain[1])
        assert qoff.dtype == np.uint64
        for k, (q, _) in enumerate(pairs):
            o = int(qoff[k] & ~bit)
            got = B.unpack2bit(seqs, o, len(q)) if seq2bit else seqs[o:o + len(q)]
            assert np.array_equal(got, q), k
        # no strands: no bit anywhere
        none = B.pack_pairs(pairs, seq2bit, np.zeros(len(pairs), bool))
        assert np.array_equal(none[1], plain[1])
    # a packed blob may start at base 0 of word 0
    w, qo, _, _, _ = B.pack_pairs(pairs, True, strands, lead=0)
    assert int(qo[0] & ~bit) == 0 and np.array_equal(B.unpack2bit(w, 0, len(pairs[0][0])), pairs[0][0])


def _walk_on_stored(q, t, res, cig):
    """the CIGAR of an alignment of revcomp(q) walked by hand on the STORED query: column at position qp of the reverse complement
    is stored base qlen - 1 - qp, complemented.  -> (stored positions touched, mat, mis, ins, del, query bases, target bases)"""
    ql = len(q)
    qp, tp = int(res[1]), int(res[3])
    touched, mat, mis, ins, dele = [], 0, 0, 0, 0
    for w in cig.tolist():
        op, ln = w & 15, w >> 4
        for _ in range(ln):
            if op == 0:
                sp = ql - 1 - qp
                touched.append(sp)
                if 3 - int(q[sp]) == int(t[tp]):
                    mat += 1
                else:
                    mis += 1
                qp += 1
                tp += 1
            elif op == 1:
                touched.append(ql - 1 - qp)
                ins += 1
                qp += 1
            else:
                assert op == 2
                dele += 1
                tp += 1
    return touched, mat, mis, ins, dele, qp, tp


def test_coordinate_rule_with_the_oracle():
    import bsalign_amd as B
    rng = np.random.default_rng(77)
    done = 0
    for k in range(36):
        L = int(rng.integers(40, 400))
        t = rng.integers(0, 4, size=L).astype(np.uint8)
        qp_ = S.mutate(rng, t, 0.08)          # what the aligner sees: similar to the target ...
        if k % 3 == 1:
            qp_ = qp_[int(rng.integers(0, 10)):len(qp_) - int(rng.integers(0, 10))]
        q = B.revcomp(qp_)                    # ... so the caller's stored query is its reverse complement
        mode = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)[k % 3]
        if k % 2:
            res, cig, n = S.oracle_align(B.revcomp(q), t, mode, 128, 2, -6, -3, -2, 0, 0)
        else:
            res, cig, n = S.oracle_edit(B.revcomp(q), t, mode, 0)
        assert n >= 0, k
        qb, qe, tb, te = (int(res[i]) for i in (1, 2, 3, 4))
        touched, mat, mis, ins, dele, qend, tend = _walk_on_stored(q, t, res, cig)
        assert (qend, tend) == (qe, te), k
        # the alignment covers exactly the stored interval [qlen - qe, qlen - qb), from its top end downwards
        assert touched == list(range(len(q) - qb - 1, len(q) - qe - 1, -1)), k
        assert sorted(touched) == list(range(len(q) - qe, len(q) - qb)), k
        assert (mat, mis, ins, dele) == tuple(int(res[i]) for i in (5, 6, 7, 8)), (k, res)
        done += 1
    assert done == 36
