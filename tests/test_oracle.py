"""CPU: the oracle (own C restatement) against the committed golden vectors (generated from the real
reference) and, when the reference build is present in this container, against the reference itself."""
import os

import numpy as np
import pytest

import support as S

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    return np.load(os.path.join(HERE, "golden", name))


def test_align8_golden():
    g = _load("align8.npz")
    n = int(g["n"][0])
    assert n > 400
    for k in range(n):
        mode, bw, M, X, O, E, Q, P = [int(x) for x in g["meta_%d" % k]]
        res, cig, cnt = S.oracle_align(g["q_%d" % k], g["t_%d" % k], mode, bw, M, X, O, E, Q, P)
        assert cnt >= 0, "case %d: oracle refused" % k
        assert np.array_equal(res, g["res_%d" % k]), "case %d result %s != %s" % (k, res, g["res_%d" % k])
        assert np.array_equal(cig, g["cig_%d" % k]), "case %d cigar" % k


def test_edit_golden():
    g = _load("edit.npz")
    n = int(g["n"][0])
    assert n > 60
    for k in range(n):
        mode, bw = [int(x) for x in g["meta_%d" % k]]
        res, cig, cnt = S.oracle_edit(g["q_%d" % k], g["t_%d" % k], mode, bw)
        assert np.array_equal(res, g["res_%d" % k]), "case %d result %s != %s" % (k, res, g["res_%d" % k])
        assert np.array_equal(cig, g["cig_%d" % k]), "case %d cigar" % k


def test_edit_wide_golden():
    """the oracle against the reference's results on bands above 1024 columns (tests/golden/make_golden_edit_wide.py)"""
    g = _load("edit_wide.npz")
    n = int(g["n"][0])
    assert n >= 29
    for k in range(n):
        mode, bw = [int(x) for x in g["meta_%d" % k]]
        res, cig, cnt = S.oracle_edit(g["q_%d" % k], g["t_%d" % k], mode, bw)
        assert np.array_equal(res, g["res_%d" % k]), "case %d result %s != %s" % (k, res, g["res_%d" % k])
        assert np.array_equal(cig, g["cig_%d" % k]), "case %d cigar" % k


def test_golden_conventions():
    """result conventions of the reference: half-open spans, aln = mat+mis+ins+del, CIGAR covers the spans"""
    g = _load("align8.npz")
    for k in range(0, int(g["n"][0]), 7):
        res, cig = g["res_%d" % k], g["cig_%d" % k]
        score, qb, qe, tb, te, mat, mis, ins, dele, aln = [int(x) for x in res]
        assert aln == mat + mis + ins + dele
        qn, tn = S.cigar_spans(cig)
        assert qn == qe - qb and tn == te - tb
        if int(g["meta_%d" % k][0]) == S.MODE_GLOBAL:
            assert (qb, tb) == (0, 0) and qe == len(g["q_%d" % k]) and te == len(g["t_%d" % k])


def test_edit_score_is_levenshtein_when_band_is_full():
    """independent secondary oracle: unbanded global edit score == Levenshtein distance"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        L = int(rng.integers(5, 200))
        T = rng.integers(0, 4, size=L).astype(np.uint8)
        Q = S.mutate(rng, T, 0.15)
        if len(Q) == 0:
            continue
        res, cig, _ = S.oracle_edit(Q, T, S.MODE_GLOBAL, 0)
        prev = np.arange(len(Q) + 1)
        for y in range(L):
            cur = np.empty_like(prev)
            cur[0] = y + 1
            for x in range(len(Q)):
                cur[x + 1] = min(prev[x] + (Q[x] != T[y]), prev[x + 1] + 1, cur[x] + 1)
            prev = cur
        assert int(res[0]) == int(prev[-1])
        assert int(res[6] + res[7] + res[8]) == int(res[0])


def test_oracle_flags_nonterminating_input():
    """an input on which the reference's traceback never terminates (large scores, narrow band): the oracle
    reports ORC_ERR_TRACE instead of hanging (found by the randomized sweep against the reference)"""
    rng = np.random.default_rng(1)
    hits = 0
    for _ in range(300):
        T = rng.integers(0, 4, size=1000).astype(np.uint8)
        Q = S.mutate(rng, T, 0.5)
        _, _, n = S.oracle_align(Q, T, S.MODE_EXTEND, 32, 10, -30, -20, -10, 0, 0)
        hits += n == S.ORC_ERR_TRACE
        if hits:
            break
    assert hits >= 1


def test_oracle_rejects_bad_input():
    q = np.array([0, 1, 2, 3], dtype=np.uint8)
    bad = np.array([0, 4, 2, 3], dtype=np.uint8)
    assert S.oracle_align(bad, q, 0, 16, 2, -6, -3, -2, 0, 0)[2] == S.ERR_INPUT
    assert S.oracle_align(q[:0], q, 0, 16, 2, -6, -3, -2, 0, 0)[2] == S.ERR_INPUT
    res, cig, n = S.oracle_edit(q[:0], q, 0, 0)      # the reference returns a zeroed result (bsalign.h:1051-1054)
    assert n == 0 and not res.any()


def test_align8_oracle_vs_reference_random():
    """(without the reference build: its answers to these very calls, tests/golden/ref_calls_align8.npz)"""
    ref_align = S.RefCalls("ref_calls_align8", S.ref_align)
    rng = np.random.default_rng(11)
    scorings = [(2, -6, -3, -2, 0, 0), (2, -2, -4, -2, 0, 0), (2, -6, 0, -3, 0, 0), (2, -6, -3, -2, -8, -1), (1, -1, -1, -1, 0, 0)]
    n = 0
    for it in range(700):
        L = int(rng.choice([1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 100, 200, 500, 1000]))
        T = rng.integers(0, 4, size=L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice([0.01, 0.1, 0.2, 0.5])))
        r = float(rng.choice([1.0, 1.0, 0.9, 1.1, 2.0, 0.5]))
        if r != 1.0:
            Lq = max(1, int(len(Q) * r))
            Q = Q[:Lq] if Lq <= len(Q) else np.concatenate([Q, rng.integers(0, 4, size=Lq - len(Q)).astype(np.uint8)])
        if len(Q) == 0:
            continue
        bw = int(rng.choice([0, 16, 32, 64, 128, 256]))
        mode = int(rng.choice([0, 1, 2]))
        sc = scorings[int(rng.integers(len(scorings)))]
        o = S.oracle_align(Q, T, mode, bw, *sc)
        if o[2] == S.ORC_ERR_TRACE:
            continue        # the reference does not terminate on these
        rr = ref_align(Q, T, mode, bw, *sc)
        assert np.array_equal(rr[0], o[0]) and np.array_equal(rr[1], o[1]), (it, L, len(Q), bw, mode, sc)
        n += 1
    assert n > 600


def test_edit_oracle_vs_reference_random():
    """(without the reference build: its answers to these very calls, tests/golden/ref_calls_edit.npz)"""
    ref_edit = S.RefCalls("ref_calls_edit", S.ref_edit)
    rng = np.random.default_rng(12)
    for it in range(600):
        L = int(rng.choice([1, 2, 15, 63, 64, 65, 100, 129, 500, 1000, 3000]))
        T = rng.integers(0, 4, size=L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice([0.01, 0.1, 0.2, 0.5])))
        r = float(rng.choice([1.0, 1.0, 0.9, 1.1, 1.5, 0.6]))
        if r != 1.0:
            Lq = max(1, int(len(Q) * r))
            Q = Q[:Lq] if Lq <= len(Q) else np.concatenate([Q, rng.integers(0, 4, size=Lq - len(Q)).astype(np.uint8)])
        if len(Q) == 0:
            continue
        bw = int(rng.choice([0, 64, 128, 256]))
        mode = int(rng.choice([0, 1, 2]))
        rr = ref_edit(Q, T, mode, bw)
        o = S.oracle_edit(Q, T, mode, bw)
        assert np.array_equal(rr[0], o[0]) and np.array_equal(rr[1], o[1]), (it, L, len(Q), bw, mode)


def test_golden_filter_is_auditable():
    """tests/golden/make_golden.py skips candidate inputs on which the oracle says the reference's traceback does not
    terminate (the reference cannot be asked).  The fixture keeps every skipped input: none was skipped for the committed
    case list, and any that a future list skips must still be flagged by the oracle."""
    g = np.load(os.path.join(S.ROOT, "tests", "golden", "align8.npz"))
    nd = int(g["ndropped"][0])
    assert nd == 0 or nd < int(g["n"][0]) // 20
    for k in range(nd):
        mode, bw, M, X, O, E, Q, P = (int(x) for x in g["dropped_meta_%d" % k])
        assert S.oracle_align(g["dropped_q_%d" % k], g["dropped_t_%d" % k], mode, bw, M, X, O, E, Q, P)[2] == S.ORC_ERR_TRACE


def test_align8_oracle_vs_reference_custom_matrices():
    """general 4 x 4 substitution matrices (tests/matrix_support.py: asymmetric, transition / transversion, positive mismatches,
    non-positive diagonal entries, all-positive, all-negative, both sides of every exact-arithmetic guard bound), all three modes,
    bandwidths 0 / 16 / 48 / 64 / 128 / 256, linear, affine and two-piece gaps
    (without the reference build: its answers to these very calls, tests/golden/ref_calls_align8_mtx.npz)"""
    import matrix_support as MS
    ref_align = S.RefCalls("ref_calls_align8_mtx", S.ref_align)
    rng = np.random.default_rng(23)
    n = flagged = 0
    for name, (mtx, gaps) in MS.CATALOGUE.items():
        models = (gaps, MS.LINEAR, MS.TWOPIECE) if name in MS.GENERAL else (gaps,)
        for bw in (0, 16, 48, 64, 128, 256):
            for mode in (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND):
                for gp in models:
                    lens = [1, 15, 16, 17, 63, 64, 65, 300] + ([bw - 1, bw, bw + 1] if bw else []) + ([1500] if rng.random() < 0.2 else [])
                    for q, t in MS.mk_pairs(rng, 2 if len(models) == 1 else 1, bw, lens=lens):
                        o = S.oracle_align(q, t, mode, bw, 0, 0, *gp, mtx=mtx)
                        if o[2] == S.ORC_ERR_TRACE:
                            flagged += 1
                            continue        # the reference does not terminate on these
                        rr = ref_align(q, t, mode, bw, 0, 0, *gp, mtx)
                        assert np.array_equal(rr[0], o[0]) and np.array_equal(rr[1], o[1]), (name, len(q), len(t), bw, mode, gp)
                        n += 1
    assert n > 700 and flagged < n // 8, (n, flagged)
