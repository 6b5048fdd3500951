"""The row target of global steering in integers (bsa_align8_x.hip: x_rt_at, x_rt_step, x_rt_set; host entry bsa_align8_row_target_internal) against numpy's float64
evaluation of the very expression the kernels had: (int)((1.0 * (double)a / (double)tlen) * (double)qlen), row a < tlen.  No GPU.

With a qlen = k tlen + r the absolute-score forward DP uses k where r != 0 (x_rt_double has the proof that the double expression truncates to k there while
qlen tlen < 2^52) and asks the double expression where r = 0, and on every row of a pair outside that bound.  Checked here: the value everywhere, the fallback exactly where a qlen mod tlen = 0, and that random
lengths take the fallback on well below one row in a hundred.  Every set is also taken with the state stepped to the row (4 and 8 rows a step, as the kernels do, the
state handed through the double expression at every row on the way that divides evenly) instead of by one division."""
import numpy as np
import pytest

import bsalign_amd as B

LMAX = (1 << 26) - 1


def _expr(a, t, q):
    """numpy's float64 evaluation of the kernels' expression, truncated to int32"""
    a, t, q = (np.asarray(x, dtype=np.float64) for x in (a, t, q))
    return ((1.0 * a / t) * q).astype(np.int32)


def _check(a, t, q, all_the_way=False):
    a, t, q = (np.asarray(x, dtype=np.uint32) for x in (a, t, q))
    want = _expr(a, t, q)
    divides = (a.astype(np.uint64) * q.astype(np.uint64)) % t.astype(np.uint64) == 0
    for stride, steps in ((4, 0), (4, 5), (8, 3)) + (((4, 1 << 20), (8, 1 << 20)) if all_the_way else ()):          # (all the way: from row a mod stride)
        value, fb = B.align8_row_target(a, t, q, stride=stride, steps=steps)
        bad = np.flatnonzero(value != want)
        assert len(bad) == 0, "stride %d steps %d: %d values differ, first (a, tlen, qlen) = %s: %d, expression %d" % (
            stride, steps, len(bad), (a[bad[0]], t[bad[0]], q[bad[0]]), value[bad[0]], want[bad[0]])
        assert np.array_equal(fb, divides), "stride %d steps %d: fallback differs from a qlen mod tlen = 0 on %d rows" % (stride, steps, int((fb != divides).sum()))
    return divides


def test_every_small_triple():
    """every 1 <= tlen, qlen <= 300 and every a < tlen"""
    rows = 0
    for t in range(1, 301):
        a, q = np.meshgrid(np.arange(t, dtype=np.uint32), np.arange(1, 301, dtype=np.uint32), indexing="ij")
        a, q = a.ravel(), q.ravel()
        _check(a, np.full(len(a), t, np.uint32), q, all_the_way=True)
        rows += len(a)
    assert rows == 300 * 300 * 301 // 2


def test_random_triples_and_the_fallback_share():
    """10^6 seeded triples with lengths up to 2^26 - 1; the fallback is taken on fewer than 1 % of them"""
    rng = np.random.default_rng(20240611)
    n = 1000000
    t = rng.integers(1, LMAX + 1, n, dtype=np.uint32)
    q = rng.integers(1, LMAX + 1, n, dtype=np.uint32)
    a = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % t.astype(np.uint64)).astype(np.uint32)
    divides = _check(a, t, q)
    share = divides.mean()
    print("fallback on %d of %d random triples" % (divides.sum(), n))
    assert share < 0.01, share
    # lengths of every magnitude (the above are nearly all above 2^20): the exponent uniform
    e = rng.integers(1, 27, n)
    t = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % ((np.uint64(1) << e.astype(np.uint64)) - np.uint64(1)) + np.uint64(1)).astype(np.uint32)
    e = rng.integers(1, 27, n)
    q = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % ((np.uint64(1) << e.astype(np.uint64)) - np.uint64(1)) + np.uint64(1)).astype(np.uint32)
    a = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % t.astype(np.uint64)).astype(np.uint32)
    _check(a, t, q)


@pytest.mark.parametrize("family", ["qlen = tlen", "qlen = 2 tlen", "tlen = 2^k", "qlen = 3 tlen / 4"])
def test_families(family):
    rng = np.random.default_rng(7)
    n = 200000
    if family == "tlen = 2^k":
        t = (np.uint32(1) << rng.integers(0, 26, n).astype(np.uint32)).astype(np.uint32)
        q = rng.integers(1, LMAX + 1, n, dtype=np.uint32)
    else:
        top = {"qlen = tlen": LMAX, "qlen = 2 tlen": LMAX // 2, "qlen = 3 tlen / 4": LMAX}[family]
        t = rng.integers(1, top + 1, n, dtype=np.uint32)
        if family == "qlen = 3 tlen / 4":
            t = np.maximum(t & ~np.uint32(3), 4)
            q = t // 4 * 3
        else:
            q = t * (2 if family == "qlen = 2 tlen" else 1)
    a = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % t.astype(np.uint64)).astype(np.uint32)
    divides = _check(a, t, q)
    if family in ("qlen = tlen", "qlen = 2 tlen"):
        assert divides.all()          # every row asks the double expression
    # the same lengths at their first and last rows
    assert _check(np.zeros(n, np.uint32), t, q).all()
    _check(t - 1, t, q)


def test_first_and_last_rows():
    """a = 0 and a = tlen - 1 of random lengths, and of the largest"""
    rng = np.random.default_rng(11)
    n = 200000
    t = rng.integers(1, LMAX + 1, n, dtype=np.uint32)
    q = rng.integers(1, LMAX + 1, n, dtype=np.uint32)
    t[:4], q[:4] = (LMAX, LMAX, LMAX - 1, 1), (LMAX, LMAX - 1, LMAX, LMAX)
    assert _check(np.zeros(n, np.uint32), t, q).all()
    _check(t - 1, t, q)


def test_pairs_outside_the_bound_take_the_double_expression():
    """qlen tlen >= 2^52, or a length of 2^31 and more: the proof does not cover the pair (the compact path bounds qlen, not tlen), so every row reports the fallback
    and has the expression's value; just inside the bound the integer form holds as everywhere else"""
    rng = np.random.default_rng(13)
    n = 200000
    q = rng.integers(1 << 20, 1 << 26, n, dtype=np.uint32)
    t = np.minimum((np.uint64(1 << 52) + q.astype(np.uint64) - np.uint64(1)) // q.astype(np.uint64) + rng.integers(0, 1 << 20, n, dtype=np.uint64), np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert (t.astype(np.uint64) * q.astype(np.uint64) >= np.uint64(1 << 52)).all()
    q[:3], t[:3] = (5, 1 << 31, 0xFFFFFFFF), (1 << 31, 5, 0xFFFFFFFF)
    a = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % t.astype(np.uint64)).astype(np.uint32)
    for stride, steps in ((4, 0), (4, 5), (8, 3)):
        value, fb = B.align8_row_target(a, t, q, stride=stride, steps=steps)
        assert fb.all() and np.array_equal(value, _expr(a, t, q))
    # the largest targets inside the bound
    t = ((np.uint64(1 << 52) - np.uint64(1)) // q.astype(np.uint64)).astype(np.uint64)
    t = np.minimum(t, np.uint64((1 << 31) - 1)).astype(np.uint32)
    q[:3] = (5, 1, (1 << 26) - 1)
    t[:3] = ((1 << 31) - 1, (1 << 31) - 1, ((1 << 52) - 1) // ((1 << 26) - 1))
    a = (rng.integers(0, 1 << 62, n, dtype=np.uint64) % t.astype(np.uint64)).astype(np.uint32)
    _check(a, t, q)
    _check(t - 1, t, q)


def test_arguments():
    one = np.ones(1, np.uint32)
    for a, t, q in ((1, 1, 5), (0, 0, 5), (7, 5, 1 << 26)):
        with pytest.raises(ValueError):
            B.align8_row_target(one * a, one * t, one * q)
