"""Shared corpus of the tests that run the 8-bit pairwise alignment under general 4 x 4 substitution matrices.

The reference scores a cell as matrix[qbase * 4 + tbase] (row = query base, column = target base) and derives smax / smin from
all sixteen entries; they seed row 0, the band rebasing and every exact-arithmetic guard.  A symmetric two-value matrix
(score_matrix(M, X)) cannot tell a transposed lookup, a kernel that takes the diagonal / matrix[0] / "the mismatch" for smax / smin,
or a mat / mis count by score sign from the right thing: the catalogue below can (tests/test_matrix_corpus_cpu.py proves it on the
oracle).  Only test code imports this."""
import numpy as np

import support as S

A, C, G, T = 0, 1, 2, 3

# gap models (gapo1, gape1, gapo2, gape2)
AFFINE = (-3, -2, 0, 0)
LINEAR = (0, -3, 0, 0)
TWOPIECE = (-3, -2, -8, -1)


def mtx(rows):
    """4 x 4 nested list, rows = query base, columns = target base -> the 16 int8 entries in the API's order"""
    m = np.array(rows, dtype=np.int16).reshape(16)
    assert m.min() >= -128 and m.max() <= 127
    return m.astype(np.int8)


def transposed(m):
    return np.ascontiguousarray(np.asarray(m, np.int8).reshape(4, 4).T.reshape(16))


def symmetric(m):
    return np.array_equal(np.asarray(m, np.int8), transposed(m))


# General matrices (default gaps AFFINE; the tests also run them under LINEAR and TWOPIECE).  Each comment says which kernel bug
# the matrix exposes.
GENERAL = {
    # every entry set, M[q][t] != M[t][q] for every q != t; smax (4) only at G->G, smin (-6) only at T->C: a transposed lookup
    # (t * 4 + q) and a kernel that takes matrix[0] / the diagonal for smax or matrix[1] for smin both change answers
    "asym": mtx([[2, -3, -1, -4],
                 [-2, 3, -5, -1],
                 [-4, -3, 4, -2],
                 [-1, -6, -3, 1]]),
    # symmetric with two mismatch values (transitions A<->G, C<->T cost less than transversions): a kernel that keeps one
    # "mismatch" score scores every transition as a transversion
    "transition": mtx([[2, -5, -1, -5],
                       [-5, 2, -5, -1],
                       [-1, -5, 2, -5],
                       [-5, -1, -5, 2]]),
    # mismatches that score > 0 (A->G +1) and = 0 (C<->T): traceback ties h == s resolve differently than with negative
    # mismatches, and mat / mis must be counted by base identity, not by the sign of the score (bsalign.h:3781)
    "posmis": mtx([[3, -4, 1, -4],
                   [-4, 3, -4, 0],
                   [-2, -4, 3, -4],
                   [-4, 0, -4, 3]]),
    # A->A scores 0: smax (3, C->C) comes from another base, matrix[0] is not the largest entry; smin (-4) only at G->T; asymmetric
    "zero_diag": mtx([[0, -3, -1, -3],
                      [-2, 3, -3, -1],
                      [-3, -2, 2, -4],
                      [-1, -3, -2, 2]]),
    # C->C scores -1 (a negative diagonal entry): smax (3) only at G->G, smin (-5) only at T->G; asymmetric
    "neg_diag": mtx([[2, -3, -1, -3],
                     [-2, -1, -3, -1],
                     [-3, -2, 3, -3],
                     [-1, -3, -5, 2]]),
    # smin > 0: every exact-arithmetic guard refuses it (they need smin <= 0 <= smax) -- row-record / run-time-width kernels
    "allpos": mtx([[6, 1, 2, 1],
                   [1, 5, 1, 3],
                   [2, 1, 6, 1],
                   [1, 3, 1, 5]]),
    # smax < 0: refused by every guard as well
    "allneg": mtx([[-1, -4, -3, -5],
                   [-4, -1, -5, -3],
                   [-3, -5, -2, -4],
                   [-5, -3, -4, -1]]),
}

# Guard boundaries: a small asymmetric base (smax 3 at C->C, smin -4 at T->A), with the extreme value of each pair in ONE off-diagonal cell (the largest at C->G,
# index 6; the smallest at T->A, index 12) so that only a kernel deriving smax / smin from all sixteen entries gets the bound right.
# With m = smax, n = -smin, g = -(gapo + gape):
#   static guard of the compact / exact-arithmetic / systolic kernels: m + 3 g <= 64, n + m + g <= 100, m + 2 n <= 128
#   checked systolic kernel (outside the static guard): m <= 63, n <= 63, g + n + m <= 128
_BASE = [[2, -3, -1, -2],
         [-2, 3, -3, -1],
         [-3, -2, 2, -2],
         [-4, -2, -3, 1]]


def _edge(m=None, n=None):
    b = mtx(_BASE).astype(np.int16)
    if m is not None:
        b[6] = m
    if n is not None:
        b[12] = -n
    return b.astype(np.int8)


BOUNDARY = {
    "m3g_64": (_edge(m=19), (-10, -5, 0, 0)),           # m + 3 g = 19 + 45: inside
    "m3g_65": (_edge(m=20), (-10, -5, 0, 0)),           # one beyond
    # n + m + g = 100 cannot be reached while m + 3 g <= 64 and m + 2 n <= 128 hold: both of these are outside the static guard
    # (m + 2 n > 128) and inside the checked systolic kernel's
    "nmg_100": (_edge(m=30, n=60), (-6, -4, 0, 0)),
    "nmg_101": (_edge(m=30, n=61), (-6, -4, 0, 0)),
    "m2n_128": (_edge(m=6, n=61), AFFINE),               # m + 2 n = 6 + 122: inside
    "m2n_129": (_edge(m=7, n=61), AFFINE),               # one beyond (row 0's seed at a mismatch wraps as a byte)
    "n_63": (_edge(n=63), AFFINE),                       # checked systolic kernel: n <= 63 (m + 2 n = 129: outside the static guard)
    "n_64": (_edge(n=64), AFFINE),
    "m_63": (_edge(m=63), AFFINE),                       # checked systolic kernel: m <= 63
    "m_64": (_edge(m=64), AFFINE),
    "gnm_128": (_edge(m=60, n=60), (-5, -3, 0, 0)),      # checked systolic kernel: g + n + m <= 128
    "gnm_129": (_edge(m=60, n=60), (-6, -3, 0, 0)),
}

# every matrix with the gap model it is meant for
CATALOGUE = dict({k: (v, AFFINE) for k, v in GENERAL.items()}, **BOUNDARY)


def smax_smin(m):
    m = np.asarray(m, np.int8)
    return int(m.max()), int(m.min())


def _g(gaps):
    g = -(gaps[0] + gaps[1])
    if gaps[2] or gaps[3]:
        g = max(g, -(gaps[2] + gaps[3]))
    return g


def static_guard(m, gaps):
    """the exact-arithmetic guard every compact-path kernel starts from (bsa_align8_codes_supported, bsa_align8_sys_supported level 1)"""
    hi, lo = smax_smin(m)
    mm, n, g = hi, -lo, _g(gaps)
    return mm >= 0 and n >= 0 and mm + 3 * g <= 64 and n + mm + g <= 100 and mm + 2 * n <= 128


def checked_sys_guard(m, gaps):
    """outside the static guard, what the checked systolic kernel still takes (one-piece gaps)"""
    hi, lo = smax_smin(m)
    mm, n, g = hi, -lo, _g(gaps)
    return mm >= 0 and n >= 0 and mm <= 63 and n <= 63 and g <= 63 and g + n + mm <= 128


IN_GUARD = [k for k, (m, gp) in CATALOGUE.items() if static_guard(m, gp)]
BEYOND_GUARD = [k for k, (m, gp) in CATALOGUE.items() if not static_guard(m, gp)]
IN_GUARD_GENERAL = [k for k in GENERAL if static_guard(GENERAL[k], AFFINE)]


def _repeat_target(rng, L, unit):
    """a target made of `unit` repeated, with 10 % of its bases replaced at random"""
    t = np.resize(np.asarray(unit, np.uint8), L)
    hit = rng.random(L) < 0.10
    t[hit] = rng.integers(0, 4, size=int(hit.sum())).astype(np.uint8)
    return t


def default_lens(bw):
    lens = [1, 15, 16, 17, 63, 64, 65, 300, 1500]
    if bw > 1:
        lens += [bw - 1, bw, bw + 1]
    return lens


def mk_pairs(rng, n, bw=128, lens=None, eps_list=(0.01, 0.05, 0.1, 0.2), ratios=(0.5, 0.9, 1.0, 1.0, 1.1, 2.0), repeats=0.25):
    """n (query, target) pairs: target lengths from `lens` (default: 1, 15/16/17, 63/64/65, bw - 1 / bw / bw + 1, 300, 1500),
    the query a mutated copy (error rate from eps_list) scaled by a length ratio; a share `repeats` of the targets are homopolymer
    or dinucleotide repeats, where one or two diagonal entries dominate the scores"""
    lens = default_lens(bw) if lens is None else lens
    pairs = []
    for _ in range(n):
        L = int(rng.choice(lens))
        u = rng.random()
        if u < repeats / 2:
            T = _repeat_target(rng, L, [int(rng.integers(4))])
        elif u < repeats:
            a = int(rng.integers(4))
            T = _repeat_target(rng, L, [a, (a + 1 + int(rng.integers(3))) & 3])
        else:
            T = rng.integers(0, 4, size=L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice(eps_list)))
        r = float(rng.choice(ratios))
        if r != 1.0:
            Lq = max(1, int(len(Q) * r))
            Q = Q[:Lq] if Lq <= len(Q) else np.concatenate([Q, rng.integers(0, 4, size=Lq - len(Q)).astype(np.uint8)])
        if len(Q) == 0:
            Q = np.array([int(rng.integers(4))], dtype=np.uint8)
        pairs.append((Q, T))
    return pairs


def nonneg_mismatches(q, t, qb, tb, cig, m):
    """(mismatched M columns, how many of them scored >= 0) along an alignment that starts at query base qb, target base tb"""
    m = np.asarray(m, np.int8)
    x, y = qb, tb
    mis = nonneg = 0
    for c in cig:
        op, ln = int(c) & 0xF, int(c) >> 4
        if op == 0:
            for _ in range(ln):
                if q[x] != t[y]:
                    mis += 1
                    nonneg += int(m[int(q[x]) * 4 + int(t[y])]) >= 0
                x += 1
                y += 1
        elif op == 1:
            x += ln
        elif op == 2:
            y += ln
    return mis, nonneg
