"""BSA_MODE_BAND_MARGIN without a GPU: the reference statement of the margin (band_margin_cases.margin_ref) on hand-made paths whose value is
obvious, the constants of the header and the Python package, and -- on the oracle alone -- that every corpus test_band_margin_gpu.py sends is
fit for its purpose: enough pairs on an edge, enough inside the band's half, at least one without a margin, hardly any the reference cannot trace."""
import os
import re

import numpy as np
import pytest

import band_margin_cases as K
import support as S

NONE = K.NONE


def _w(*words):
    return np.array([(n << 4) | {"M": 0, "I": 1, "D": 2, "=": 7, "X": 8}[op] for n, op in words], dtype=np.uint32)


def _res(qb, tb):
    return np.array([0, qb, 0, tb, 0, 0, 0, 0, 0, 0], dtype=np.int32)


def test_straight_diagonal_in_a_centred_band():
    # bandwidth 16, 64 x 64 bases, the band 8 columns to either side of the diagonal wherever the query's ends allow
    begs = np.clip(np.arange(64) - 8, 0, 64 - 16)
    assert K.margin_ref(64, 64, 16, _res(0, 0), _w((64, "M")), begs) == 7          # high edge: b + 15 - c = 7; low edge: c - b = 8
    assert K.margin_ref(64, 64, 16, _res(0, 0), _w((30, "="), (4, "X"), (30, "=")), begs) == 7


def test_path_forced_onto_each_edge():
    begs = np.clip(np.arange(64) - 8, 0, 64 - 16)
    lo = begs.copy()
    lo[20:30] = np.arange(20, 30)                 # the band's low edge ON the diagonal for ten rows
    assert K.margin_ref(64, 64, 16, _res(0, 0), _w((64, "M")), lo) == 0
    hi = begs.copy()
    hi[20:30] = np.arange(20, 30) - 15            # ... its high edge
    assert K.margin_ref(64, 64, 16, _res(0, 0), _w((64, "M")), hi) == 0
    one = begs.copy()
    one[25] = 25 - 14                             # one cell beside the high edge
    assert K.margin_ref(64, 64, 16, _res(0, 0), _w((64, "M")), one) == 1


def test_edges_at_the_querys_ends_do_not_count():
    # the band lies at the query's start (b = 0) on the first rows and at its end (b + B = qlen) on the last: the path runs ON both
    begs = np.array([0] * 16 + list(range(1, 17)) + [16] * 16)
    cig = _w((48, "M"))
    m = K.margin_ref(32 + 16, 48, 32, _res(0, 0), cig, np.clip(np.arange(48) - 16, 0, 16))
    assert m == 15                                # rows 17..31: c - b = 16, b + 31 - c = 15; rows 0..15 on column b = 0 and rows 32.. at b + B = qlen count nothing on that side
    assert K.margin_ref(48, 48, 32, _res(0, 0), cig, begs) == 15
    # a path down column 0 of a band at offset 0 (a 4-base query inside a wider batch's bandwidth is whole-query: use D words): no low edge
    assert K.margin_ref(20, 4, 16, _res(1, 0), _w((4, "D")), np.zeros(4, np.int32)) == 15         # only the high edge, b + B = 16 < 20: 15 - 0
    # ... and ON the last column of a band that ends with the query: c = 14..17, b = 2, b + B = 18 = qlen: only the low edge, 12
    assert K.margin_ref(18, 4, 16, _res(14, 0), _w((4, "M")), np.full(4, 2)) == 12
    # both at once -- b = 0 and b + B = qlen is a whole-query band: nothing counts
    assert K.margin_ref(16, 4, 16, _res(12, 0), _w((4, "M")), np.zeros(4, np.int32)) == NONE


def test_start_vertex():
    begs = np.full(8, 4)
    # j = 0: the start vertex is no cell; the first counted one is (1, 1) -- column 0 with b = 4: outside, counts as 0
    assert K.margin_ref(40, 8, 16, _res(0, 0), _w((8, "M")), begs) == 0
    # the start vertex (3, 9) is the cell (2, 8): low 4, and the M word goes on from there
    assert K.margin_ref(40, 8, 16, _res(9, 3), _w((5, "M")), begs) == 4
    # ... it counts even where no word visits its row again: (3, 5) -> cell (2, 4), low 0; the D word stays in column 4
    assert K.margin_ref(40, 8, 16, _res(5, 3), _w((2, "D")), begs) == 0
    assert K.margin_ref(40, 8, 16, _res(6, 3), _w((2, "D")), begs) == 1
    # tb = 0: not a cell
    assert K.margin_ref(40, 8, 16, _res(6, 0), _w((2, "I")), begs) == NONE


def test_insertions_and_deletions_at_an_edge():
    begs = np.array([0, 0, 0, 0, 2, 4, 6, 8])
    # 4M to (4, 4), then 13I along row 3 (b = 0: only the high edge, 15 - c): c reaches 16 -> -1 counts as 0; 12I stops ON the edge; 11I one short
    for n, want in ((13, 0), (12, 0), (11, 1)):
        assert K.margin_ref(40, 8, 16, _res(0, 0), _w((4, "M"), (n, "I")), begs) == want, n
    # 6M to (6, 6), then D down column 5: rows 6, 7 have b = 6, 8 -> c - b = -1, -3: 0; with begs ending 2 3 4 5 the column stays inside
    assert K.margin_ref(40, 8, 16, _res(0, 0), _w((6, "M"), (2, "D")), begs) == 0
    assert K.margin_ref(40, 8, 16, _res(0, 0), _w((6, "M"), (2, "D")), np.array([0, 0, 0, 0, 2, 3, 4, 5])) == 0    # row 7: c = 5, b = 5
    assert K.margin_ref(40, 8, 16, _res(0, 0), _w((6, "M"), (1, "D")), np.array([0, 0, 0, 0, 2, 3, 4, 5])) == 1    # row 6: c = 5, b = 4
    # a leading D then I: the path enters row 2 at j = 0 and its first cell there is column 0
    assert K.margin_ref(40, 8, 16, _res(0, 0), _w((2, "D"), (3, "I")), np.array([0, 3, 3, 3, 3, 3, 3, 3])) == 0
    assert K.margin_ref(40, 8, 16, _res(0, 0), _w((2, "D"), (3, "I")), np.zeros(8, np.int32)) == 13               # high edge: 15 - 2


def test_whole_query_bands_and_pairs_without_a_cigar():
    begs = np.zeros(30, np.int32)
    assert K.margin_ref(30, 30, 0, _res(0, 0), _w((30, "M")), begs) == NONE
    assert K.margin_ref(30, 30, 32, _res(0, 0), _w((30, "M")), begs) == NONE
    assert K.margin_ref(30, 30, 17, _res(0, 0), _w((30, "M")), begs) == NONE          # 17 rounds up to 32
    assert K.margin_ref(64, 64, 16, _res(0, 0), _w(), begs) == NONE
    # clamped: a band of 70 000 columns that ends with the query, the path 69 983 columns above its low edge
    assert K.margin_ref(70016, 4, 70000, _res(70000, 0), _w((4, "M")), np.full(4, 16)) == 0xFFFE


def test_header_example():
    begs = np.array([0] * 8 + list(range(1, 9)) + [8] * 8)
    assert K.margin_ref(24, 24, 16, _res(0, 0), _w((24, "M")), begs) == 7
    assert K.margin_ref(24, 24, 16, _res(0, 0), _w((12, "M"), (4, "D"), (4, "I"), (8, "M")), begs) == 3


def test_constants_agree_with_the_header():
    import bsalign_amd as B
    with open(os.path.join(S.ROOT, "include", "bsalign_hip.h")) as f:
        h = f.read()

    def define(name):
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, h)
        assert m, name
        return int(m.group(1), 0)
    assert define("BSA_MODE_BAND_MARGIN") == B.MODE_BAND_MARGIN == 0x4000
    assert define("BSA_ST_MARGIN_SHIFT") == B.ST_MARGIN_SHIFT == 16
    assert define("BSA_ST_MARGIN_NONE") == B.ST_MARGIN_NONE == NONE == 0xFFFF
    flags = [B.MODE_ROWRECORDS, B.MODE_SCORE_ONLY, B.MODE_SEQ2BIT, B.MODE_CIGAR_EQX, B.MODE_QSTRAND, B.MODE_BAND_MARGIN]
    assert len(set(flags)) == len(flags) and all(f & 3 == 0 and f & (f - 1) == 0 for f in flags)
    assert "bsa_ctx_last_margin_ms" in h


@pytest.mark.parametrize("mode", K.MODES, ids=["global", "overlap", "extend"])
@pytest.mark.parametrize("bw", K.BANDWIDTHS)
def test_corpora_are_fit_for_purpose(bw, mode):
    """per (mode, bandwidth) corpus, under every scoring the GPU test uses: at least 10 % of the pairs on an edge, at least 10 % strictly inside
    the band's half, at least one without a margin, at most 2 % the oracle cannot trace (the GPU test compares those by status alone)"""
    B = K.roundup16(bw)
    for sc in K.SC:
        ex = K.expected(bw, mode, sc)
        n = len(ex)
        zero = sum(1 for m in ex if m == 0)
        mid = sum(1 for m in ex if m is not None and m != NONE and 1 <= m <= B // 2 - 1)
        none = sum(1 for m in ex if m == NONE)
        bad = sum(1 for m in ex if m is None)
        assert zero >= 0.10 * n, (bw, mode, sc, zero, n)
        assert mid >= 0.10 * n, (bw, mode, sc, mid, n)
        assert none >= 1, (bw, mode, sc)
        assert bad <= K.MAX_UNTRACEABLE * n, (bw, mode, sc, bad, n)


@pytest.mark.parametrize("which", ["short", "long", "mixed"])
def test_whole_query_corpora_have_no_margin(which):
    pairs = K.whole_corpus(which)
    if which == "short":
        assert all(len(q) <= 256 for q, _ in pairs)
    if which == "long":
        assert all(len(q) > 256 for q, _ in pairs)
    for mode in K.MODES:
        ex = K.expected(0, mode, "affine", which)
        assert all(m is None or m == NONE for m in ex)
        assert sum(1 for m in ex if m is None) <= K.MAX_UNTRACEABLE * len(ex)
