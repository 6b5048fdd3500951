"""BSA_MODE_CIGAR_EQX without a GPU: the numpy statement of the = / X split (bsalign_amd.expand_eqx / collapse_eqx) on hand-written
cases, the definition pinned against the oracle's own mat / mis counts on every corpus and parameter set the GPU file sends, the
share of pairs that can only be compared by status, and the ABI constants."""
import os
import re

import numpy as np
import pytest

import cigar_eqx_cases as K
import support as S

M, I, D, EQ, X = 0, 1, 2, 7, 8


def W(*pairs):
    return np.array([(n << 4) | op for n, op in pairs], dtype=np.uint32)


def seq(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def test_expand_hand_written_cases():
    import bsalign_amd as B
    assert (B.CIGAR_M, B.CIGAR_I, B.CIGAR_D, B.CIGAR_EQ, B.CIGAR_X) == (M, I, D, EQ, X)
    ex = B.expand_eqx
    # all match, all mismatch, alternating columns, an M word of length 1
    assert np.array_equal(ex(W((5, M)), seq("ACGTA"), seq("ACGTA")), W((5, EQ)))
    assert np.array_equal(ex(W((5, M)), seq("ACGTA"), seq("CGTAC")), W((5, X)))
    assert np.array_equal(ex(W((6, M)), seq("AAAAAA"), seq("ACACAC")), W((1, EQ), (1, X), (1, EQ), (1, X), (1, EQ), (1, X)))
    assert np.array_equal(ex(W((1, M)), seq("A"), seq("A")), W((1, EQ)))
    assert np.array_equal(ex(W((1, M)), seq("A"), seq("C")), W((1, X)))
    # runs inside a word, I and D between words: positions advance by the words in front
    q, t = seq("ACGTTTGA"), seq("ACCTGAC")
    #  q: A C G T T T G A     t: A C C T . . G A C      2= 1X 1= 2I 2= 1D
    assert np.array_equal(ex(W((4, M), (2, I), (2, M), (1, D)), q, t), W((2, EQ), (1, X), (1, EQ), (2, I), (2, EQ), (1, D)))
    # leading I / D in global mode
    assert np.array_equal(ex(W((2, I), (3, M)), seq("TTACG"), seq("ACC")), W((2, I), (2, EQ), (1, X)))
    assert np.array_equal(ex(W((2, D), (3, M)), seq("ACC"), seq("TTACG")), W((2, D), (2, EQ), (1, X)))
    # a CIGAR with no M at all, an empty one
    assert np.array_equal(ex(W((3, I), (2, D)), seq("ACG"), seq("TT")), W((3, I), (2, D)))
    assert ex(W(), seq("A"), seq("A")).size == 0
    # positions start at qb / tb
    assert np.array_equal(ex(W((3, M)), seq("TTACG"), seq("GACC"), qb=2, tb=1), W((2, EQ), (1, X)))
    # two M words around a gap do not merge their runs
    assert np.array_equal(ex(W((2, M), (1, I), (2, M)), seq("ACTGT"), seq("ACGT")), W((2, EQ), (1, I), (2, EQ)))
    with pytest.raises(ValueError):
        ex(W((4, M)), seq("ACG"), seq("ACGT"))


def test_collapse_is_the_inverse():
    import bsalign_amd as B
    rng = np.random.default_rng(5)
    for _ in range(200):
        words, qn, tn, last = [], 0, 0, -1
        for _ in range(int(rng.integers(0, 12))):
            op = int(rng.choice([o for o in (M, I, D) if o != last]))
            n = int(rng.integers(1, 9))
            words.append((n, op))
            qn += n if op != D else 0
            tn += n if op != I else 0
            last = op
        q = rng.integers(0, 2, size=qn + 3).astype(np.uint8)
        t = rng.integers(0, 2, size=tn + 2).astype(np.uint8)
        w = W(*words)
        e = B.expand_eqx(w, q, t)
        assert np.array_equal(B.collapse_eqx(e), w)
        assert e.size == 0 or K.well_formed(e)
    assert np.array_equal(B.collapse_eqx(W((2, EQ), (1, X), (3, I), (1, X))), W((3, M), (3, I), (1, M)))


def _pin(pairs, results, what):
    """sum of = lengths == mat and sum of X lengths == mis of the oracle's record; returns the share of untraceable pairs"""
    import bsalign_amd as B
    bad = 0
    for k, ((q, t), (res, cig, n)) in enumerate(zip(pairs, results)):
        if n == S.ORC_ERR_TRACE:
            bad += 1
            continue
        assert n >= 0, (what, k, n)
        e = B.expand_eqx(cig, q, t, res[1], res[3])
        ops, lens = e & 15, e >> 4
        assert int(lens[ops == EQ].sum()) == res[5] and int(lens[ops == X].sum()) == res[6], (what, k, res)
        assert np.array_equal(B.collapse_eqx(e), cig), (what, k)
        assert e.size == 0 or K.well_formed(e), (what, k)
        assert e.size <= cig.size + 2 * res[6], (what, k)                  # the bound the header gives a caller
    return bad / max(len(pairs), 1)


@pytest.mark.parametrize("case", K.ALIGN_CASES + K.HANDOVER_CASES, ids=lambda c: c[0])
def test_definition_agrees_with_the_oracles_counts_align(case):
    cid, cname, mode, bw, sc, flags, env, fwd, trace = case
    share = _pin(K.corpus(cname), K.align_oracle(cname, mode, bw, sc), cid)
    assert share <= K.MAX_UNTRACEABLE, (cid, share)


@pytest.mark.parametrize("case", K.EDIT_CASES, ids=lambda c: c[0])
def test_definition_agrees_with_the_oracles_counts_edit(case):
    cid, cname, mode, bw, env, fwd, trace, nottrace = case
    share = _pin(K.corpus(cname), K.edit_oracle(cname, mode, bw), cid)
    assert share <= K.MAX_UNTRACEABLE, (cid, share)


def test_corpora_reach_what_they_are_meant_for():
    """properties of the corpora the GPU cases rely on"""
    assert min(len(q) for q, _ in K.corpus("gt48")) > 48 and len(K.corpus("gt48")) >= 16         # bandwidth 48 / 1024: no whole-query bands
    assert min(len(q) for q, _ in K.corpus("gt1024")) > 1024 and len(K.corpus("gt1024")) >= 8
    assert min(len(q) for q, _ in K.corpus("longq")) > 256 and len(K.corpus("longq")) >= 16
    assert min(len(q) for q, _ in K.corpus("clamp")) > 256
    assert len(K.corpus("edit")) >= 24
    assert min(len(q) for q, _ in K.corpus("editwide")) > 1024
    assert min(len(q) for q, _ in K.corpus("editgen")) > 1088 and len(K.corpus("editgen")) >= 4
    # long words: the substitution-only pairs are one M word of 10 000 columns in both aligners
    res = K.align_oracle("long", K.G, 128, "affine")
    assert sum(1 for r, cig, n in res if n == 1 and int(cig[0]) == (K.LONG_L << 4)) >= 60
    res = K.edit_oracle("long", K.G, 256)
    assert sum(1 for r, cig, n in res if n == 1 and int(cig[0]) == (K.LONG_L << 4)) >= 60
    # long CIGARs: more than 64 and more than 4096 plain words
    n = [x[2] for x in K.align_oracle("words", K.G, 128, "affine")]
    assert n[0] > 64 and n[1] > 4096, n
    n = [x[2] for x in K.edit_oracle("words", K.G, 256)]
    assert n[0] > 64 and n[1] > 4096, n


def test_abi_constants():
    import bsalign_amd as B
    hdr = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()

    def val(name):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, hdr)
        assert m, name
        return int(m.group(1), 0)
    assert val("BSA_MODE_CIGAR_EQX") == B.MODE_CIGAR_EQX == 0x1000
    assert val("BSA_CIGAR_EQ") == B.CIGAR_EQ == 7
    assert val("BSA_CIGAR_X") == B.CIGAR_X == 8
    # the flag collides with no other mode bit
    others = [val(n) for n in ("BSA_MODE_ROWRECORDS", "BSA_MODE_SCORE_ONLY", "BSA_MODE_SEQ2BIT")]
    assert all(o & B.MODE_CIGAR_EQX == 0 for o in others + [3, 0x200])
