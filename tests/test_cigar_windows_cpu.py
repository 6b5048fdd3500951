"""CPU: bsa_cigar_windows_* (include/bsalign_hip.h) without a GPU -- the header's two worked examples against the Python statement of the
definition (cigar_windows_cases.windows_ref), bsa_cigar_windows_bound against numpy, and the properties every window record has, on CIGARs
of the oracle."""
import numpy as np
import pytest

import cigar_windows_cases as W
import support as S


def test_header_examples():
    import bsalign_amd as B
    assert B.WINDOW_NONE == W.NONE == 0xFFFFFFFF
    for w, rec, cig, want in W.header_examples():
        got = W.windows_ref(rec, cig, w)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (S.cigar_str(cig), got)
    # the examples are in the header as they are here
    text = open(S.ROOT + "/include/bsalign_hip.h").read()
    for s in ("5M 2I 4D 6M", "{10, 6, 19, 13}", "3M 25D 3M", "{28, 3, 29, 4}", "BSA_WINDOW_NONE 0xFFFFFFFFu"):
        assert s in text, s


def test_bound_equals_numpy():
    import bsalign_amd as B
    rng = np.random.default_rng(1)
    tlen = np.concatenate([rng.integers(0, 30000, 500), [0, 1, 499, 500, 501, 0xFFFFFFFF, 0xFFFFFFFE]]).astype(np.uint32)
    for w in (1, 2, 7, 500, 501, 29999, 30000, 1 << 20, 1 << 31, 0xFFFFFFFF):
        want = int(((tlen.astype(np.uint64) + np.uint64(w - 1)) // np.uint64(w)).sum())
        assert B.cigar_windows_bound(tlen, w) == want, w
    assert B.cigar_windows_bound(tlen, 1) == int(tlen.astype(np.uint64).sum())                  # w = 1: a window a base
    assert B.cigar_windows_bound(tlen[:500], 40000) == int((tlen[:500] > 0).sum())            # w > tlen: one window a pair that has bases
    assert B.cigar_windows_bound(tlen, 0) == 0                                                # w = 0
    assert B.cigar_windows_bound(np.zeros(0, np.uint32), 500) == 0                            # n = 0
    assert B.lib().bsa_cigar_windows_bound(None, 0, 500) == 0


def test_bound_suffices_for_the_hand_made_cases():
    """te <= tlen for a real record, so ceil(tlen / w) with tlen = te bounds its windows"""
    import bsalign_amd as B
    for name, (w, recs, cigs) in W.hand_cases().items():
        per, off = W.expected(w, recs, cigs)
        te = np.array([max(int(r[4]), 0) for r in recs], dtype=np.uint32)
        assert int(off[-1]) <= B.cigar_windows_bound(te, w), name


def _check_records(rec, res, w, what):
    tb, te = int(res[3]), int(res[4])
    m0 = tb // w
    assert len(rec) == (te - 1) // w - m0 + 1, (what, "windows tb / w .. (te - 1) / w")
    prev = None
    for r, (tf, qf, tl, ql) in enumerate(rec.tolist()):
        if tf == W.NONE:
            assert (qf, tl, ql) == (W.NONE,) * 3, what
            continue
        lo, hi = (m0 + r) * w, (m0 + r + 1) * w
        assert lo <= tf <= tl < hi and qf <= ql, (what, r)
        assert tb <= tf and tl < te and int(res[1]) <= qf and ql < int(res[2]), (what, r)
        if prev is not None:
            assert prev[0] < tf and prev[1] < qf, (what, r, "first and last columns increase strictly")
        assert (tf, qf) == (tl, ql) or (tf < tl and qf < ql), (what, r)
        prev = (tl, ql)
    return sum(1 for x in rec if x[0] != W.NONE)


@pytest.fixture(scope="module")
def oracle_pairs():
    """a few dozen pairs of about 300 bases with their oracle records and CIGARs: (what, record, words)"""
    rng = np.random.default_rng(2024)
    out = []
    sc = (2, -6, -3, -2, 0, 0)
    for k in range(36):
        T = rng.integers(0, 4, int(rng.integers(250, 350))).astype(np.uint8)
        Q = S.mutate(rng, T, float((0.03, 0.10, 0.20)[k % 3]))
        if k % 4 == 1:                                         # an indel burst: a window that a deletion can cover whole
            a = int(rng.integers(50, 200))
            Q = np.concatenate([Q[:a], Q[a + int(rng.integers(10, 40)):]])
        if k % 12 < 9:
            mode = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)[k % 3]
            res, cig, n = S.oracle_align(Q, T, mode, 64, *sc)
            what = "align mode %d pair %d" % (mode, k)
        else:
            res, cig, n = S.oracle_edit(Q, T, S.MODE_GLOBAL, 128)
            what = "edit pair %d" % k
        assert n > 0, what
        out.append((what, res, cig))
    return out


@pytest.mark.parametrize("w", [1, 7, 50, 64, 500])
def test_window_records_of_oracle_cigars(oracle_pairs, w):
    holes = 0
    for what, res, cig in oracle_pairs:
        qn, tn = S.cigar_spans(cig)
        assert int(res[4]) - int(res[3]) == tn and int(res[2]) - int(res[1]) == qn, what
        rec = W.windows_ref(res, cig, w)
        full = _check_records(rec, res, w, "%s, w %d" % (what, w))
        holes += len(rec) - full
        # the pieces of the read: disjoint, in order, and with the inserted and deleted bases they add up to the alignment
        filled = rec[rec[:, 0] != W.NONE].astype(np.int64)
        assert int((filled[:, 3] - filled[:, 1] + 1).sum()) <= qn
        if w >= 500:
            assert len(rec) == 1 and tuple(filled[0][[0, 2]]) == _first_last_diag(res, cig), what
    assert w != 1 or holes > 0                                 # w = 1: every deleted base is a window of its own without a column


def _first_last_diag(res, cig):
    t, first, last = int(res[3]), None, None
    for c in cig:
        op, ln = int(c) & 15, int(c) >> 4
        if op == 0 and ln:
            first = t if first is None else first
            last = t + ln - 1
        t += ln if op in (0, 2) else 0
    return first, last


def test_reference_rules_for_inconsistent_words():
    c = W.hand_cases()
    w, (r,), (x,) = c["more_target_than_te"]
    assert W.windows_ref(r, x, w).tolist() == [[0, 0, 9, 9], [10, 10, 19, 19], [20, 20, 29, 29]]
    w, (r,), (x,) = c["less_target_than_te"]
    assert W.windows_ref(r, x, w).tolist() == [[0, 0, 9, 9], [10, 10, 11, 11]] + [[W.NONE] * 4] * 8
    w, (r,), (x,) = c["far_more_target"]
    assert W.windows_ref(r, x, w).tolist() == [[0, 0, 4, 4]] + [[W.NONE] * 4] * 3
    w, (r,), (x,) = c["I_words_only"]
    assert len(W.windows_ref(r, x, w)) == 0
    w, (r,), (x,) = c["D_covers_three_windows"]
    assert W.windows_ref(r, x, w).tolist() == [[5, 2, 9, 6], [10, 7, 12, 9]] + [[W.NONE] * 4] * 3 + [[53, 10, 59, 16], [60, 17, 61, 18]]
