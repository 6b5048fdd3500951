"""CPU: the matrix corpus of tests/matrix_support.py can tell the kernel bugs it is meant for from the right answer -- proved on the
oracle alone.  Without this a GPU parity test under these matrices could pass for the wrong reason (a corpus on which a transposed
lookup, or the matrix projected onto two values, happens to give the same alignments)."""
import numpy as np
import pytest

import matrix_support as MS
import support as S


def _pairs(seed, bw=128):
    return MS.mk_pairs(np.random.default_rng(seed), 60, bw)


def _answer(q, t, mode, bw, m, gaps):
    res, cig, n = S.oracle_align(q, t, mode, bw, 0, 0, *gaps, mtx=m)
    return n, res.tobytes(), cig.tobytes()


def _share_differing(pairs, mode, bw, m1, m2, gaps):
    return sum(_answer(q, t, mode, bw, m1, gaps) != _answer(q, t, mode, bw, m2, gaps) for q, t in pairs) / len(pairs)


@pytest.mark.parametrize("name", [k for k, (m, _) in MS.CATALOGUE.items() if not MS.symmetric(m)])
def test_transposed_matrix_changes_the_answers(name):
    """a kernel that reads matrix[t * 4 + q] instead of matrix[q * 4 + t] gives other answers on at least 30 % of the corpus"""
    m, gaps = MS.CATALOGUE[name]
    pairs = _pairs(700 + len(name))
    for mode in (S.MODE_GLOBAL, S.MODE_EXTEND):
        share = _share_differing(pairs, mode, 128, m, MS.transposed(m), gaps)
        assert share >= 0.30, (name, mode, share)


def _extremes_off_the_first_cells(m):
    hi, lo = MS.smax_smin(m)
    return hi != int(m[0]) or lo != int(m[1])


@pytest.mark.parametrize("name", [k for k, (m, _) in MS.CATALOGUE.items() if _extremes_off_the_first_cells(m)])
def test_matrix_projected_onto_two_values_changes_the_answers(name):
    """where smax / smin are not matrix[0] / matrix[1], a kernel that runs score_matrix(matrix[0], matrix[1]) (the diagonal as 'the
    match', matrix[1] as 'the mismatch') gives other answers on most pairs"""
    m, gaps = MS.CATALOGUE[name]
    pairs = _pairs(800 + len(name))
    proj = S.score_matrix(int(m[0]), int(m[1]))
    share = _share_differing(pairs, S.MODE_GLOBAL, 128, m, proj, gaps)
    assert share > 0.5, (name, share)


def test_projection_covers_the_asymmetric_diagonal_and_boundary_matrices():
    """their smax or smin lies off matrix[0] / matrix[1], so the projection test above takes them"""
    off = [k for k, (m, _) in MS.CATALOGUE.items() if _extremes_off_the_first_cells(m)]
    for k in ("asym", "zero_diag", "neg_diag") + tuple(MS.BOUNDARY):
        assert k in off, k


def test_catalogue_covers_both_sides_of_every_guard():
    assert {"asym", "transition", "posmis", "zero_diag", "neg_diag", "m3g_64", "m2n_128"} <= set(MS.IN_GUARD)
    assert {"allpos", "allneg", "m3g_65", "m2n_129", "n_63", "n_64", "m_63", "m_64"} <= set(MS.BEYOND_GUARD)
    for inside, beyond in (("n_63", "n_64"), ("m_63", "m_64"), ("gnm_128", "gnm_129")):
        assert MS.checked_sys_guard(*MS.CATALOGUE[inside]) and not MS.checked_sys_guard(*MS.CATALOGUE[beyond])
    assert MS.smax_smin(MS.GENERAL["allpos"])[1] > 0 and MS.smax_smin(MS.GENERAL["allneg"])[0] < 0
    # the extreme value of a boundary matrix sits in one cell only
    for k, (m, _) in MS.BOUNDARY.items():
        hi, lo = MS.smax_smin(m)
        assert (m == hi).sum() == 1 and (m == lo).sum() == 1, k


def test_corpus_reaches_nonnegative_mismatches_counted_as_mismatches():
    """mat / mis are counted by base identity (bsalign.h:3781): the corpus must contain alignments that take a mismatch scoring >= 0,
    and there the oracle's mis counts it -- a kernel that counts by the sign of the score would not"""
    m = MS.GENERAL["posmis"]
    pairs = _pairs(900)
    hits = 0
    for mode in (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND):
        for q, t in pairs:
            res, cig, n = S.oracle_align(q, t, mode, 128, 0, 0, *MS.AFFINE, mtx=m)
            if n < 0:
                continue
            mis, nonneg = MS.nonneg_mismatches(q, t, int(res[1]), int(res[3]), cig, m)
            assert mis == int(res[6]), (mode, len(q), len(t))
            hits += nonneg > 0 and int(res[6]) > 0
    assert hits >= 1
