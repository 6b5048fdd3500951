"""Corpora, expected results and the arena checker of the plan / run surface tests (test_plan_surface_cpu.py, test_plan_surface_gpu.py).
No GPU here.

The contract the checker states (include/bsalign_hip.h, at bsa_align_run): with any cigar_cap_words, no word at or above the capacity is
touched, every pair's range inside the arena holds either exactly that pair's words or none of them, and d_cigar_off is the large-arena run's.
The tests fill the arena with a sentinel whose low four bits (5) are no CIGAR operation, so an untouched word cannot be mistaken for a written one.
"""
import functools

import numpy as np

import support as S

ST_BAD_BASE, ST_EMPTY = 1, 2
SENTINEL = 0xA5A5A5A5                     # a word of 0xA5 bytes: operation 5, which no aligner here writes (M 0, I 1, D 2, = 7, X 8)

SCORINGS = {
    "affine": (2, -6, -3, -2, 0, 0),
    "twopiece": (2, -6, -3, -2, -8, -1),
}
# every (kind, mode, bandwidth, scoring) the tests run a corpus of the shape of `small` with: the corpora hold no pair on which the
# reference's traceback does not terminate under any of them
CONFIGS = [
    ("align", S.MODE_GLOBAL, 128, SCORINGS["affine"]),
    ("align", S.MODE_GLOBAL, 0, SCORINGS["affine"]),
    ("align", S.MODE_GLOBAL, 128, SCORINGS["twopiece"]),
    ("align", S.MODE_GLOBAL, 64, SCORINGS["twopiece"]),
    ("edit", S.MODE_GLOBAL, 256, None),
    ("edit", S.MODE_EXTEND, 0, None),
]
# ... of which these run the compact (code) traceback on the device, which may hand a pair over to the literal kernels
# (oracle/bsalign_oracle.c, orc_align_pairwise_codes_mode says which): the corpora hold no such pair either
CODE_CONFIGS = [c for c in CONFIGS if c[0] == "align" and c[2] != 0]

N_SMALL = 96
EMPTY_QUERY, EMPTY_TARGET, BAD_BASE, SHARES_FROM, SHARES_TO = 10, 20, 30, 40, 41          # pair SHARES_TO aligns against pair SHARES_FROM's target bytes


class Corpus:
    """pairs plus the blob layout the tests upload: all sequences back to back in pair order, query then target; a pair in `shared`
    (j -> i) has no target bytes of its own, toff[j] = toff[i]"""

    def __init__(self, pairs, shared=None):
        self.pairs = pairs
        self.shared = dict(shared or {})
        n = len(pairs)
        self.qlen = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
        self.tlen = np.array([len(t) for _, t in pairs], dtype=np.uint32)
        self.qoff = np.zeros(n, dtype=np.uint64)
        self.toff = np.zeros(n, dtype=np.uint64)
        parts, acc = [], 0
        for k, (q, t) in enumerate(pairs):
            self.qoff[k] = acc
            parts.append(np.ascontiguousarray(q, dtype=np.uint8))
            acc += len(q)
            if k in self.shared:
                assert np.array_equal(t, pairs[self.shared[k]][1])
                self.toff[k] = self.toff[self.shared[k]]
                continue
            self.toff[k] = acc
            parts.append(np.ascontiguousarray(t, dtype=np.uint8))
            acc += len(t)
        self.seqs = np.concatenate(parts) if acc else np.zeros(1, dtype=np.uint8)

    def __len__(self):
        return len(self.pairs)

    def good(self):
        """indices of the pairs that are neither empty nor carry a base code above 3"""
        return [k for k, (q, t) in enumerate(self.pairs) if len(q) and len(t) and int(max(q.max(), t.max())) <= 3]


def _codes_align(q, t, mode, bw, sc):
    import ctypes as C
    o = S.oracle()
    o.orc_align_pairwise_codes_mode.restype = C.c_long
    o.orc_align_pairwise_codes_mode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_long]
    mtx = S.score_matrix(sc[0], sc[1])
    res = np.zeros(10, np.int32)
    cap = 4 * (len(q) + len(t)) + 16
    cig = np.zeros(cap, np.uint32)
    q, t = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
    return o.orc_align_pairwise_codes_mode(q.ctypes.data, len(q), t.ctypes.data, len(t), mode, bw, mtx.ctypes.data, *sc[2:], res.ctypes.data, cig.ctypes.data, cap)


_ORACLE = {}


def _oracle(q, t, kind, mode, bw, scoring):
    """the C oracle's (record, words, count), kept per input: the corpus builders and expected() ask for the same pairs"""
    ck = (np.asarray(q).tobytes(), np.asarray(t).tobytes(), kind, mode, bw, scoring)
    if ck not in _ORACLE:
        _ORACLE[ck] = S.oracle_align(q, t, mode, bw, *scoring) if kind == "align" else S.oracle_edit(q, t, mode, bw)
    return _ORACLE[ck]


def needs_handover(q, t):
    """does the device's compact traceback decline this pair under one of CODE_CONFIGS (the host entry would re-run it, bsa_align_run flags it)?"""
    return any(_codes_align(q, t, mode, bw, sc) == S.ORC_ERR_TRACE for _, mode, bw, sc in CODE_CONFIGS)


def usable(q, t):
    """a pair the corpora may hold: the reference's traceback terminates on it under every configuration of the tests, and the compact
    traceback decides it"""
    if any(_oracle(q, t, *cfg)[2] == S.ORC_ERR_TRACE for cfg in CONFIGS):
        return False
    return not needs_handover(q, t)


def _substituted(rng, T, div):
    Q = T.copy()
    hit = rng.random(len(T)) < div
    Q[hit] = (Q[hit] + 1 + rng.integers(0, 3, int(hit.sum())).astype(np.uint8)) & 3
    return Q


def _draw_small_pair(rng, k):
    L = 40 if k == 0 else 1500 if k == 1 else int(rng.integers(40, 1501))
    div = (0.0, 0.02, 0.10, 0.25)[k % 4]
    ratio = (0.9, 1.0, 1.1)[(k // 4) % 3]
    T = rng.integers(0, 4, size=L).astype(np.uint8)
    Q = S.mutate(rng, T, div)
    Lq = max(1, int(round(len(Q) * ratio))) if ratio != 1.0 else len(Q)
    Q = Q[:Lq] if Lq <= len(Q) else np.concatenate([Q, rng.integers(0, 4, size=Lq - len(Q)).astype(np.uint8)])
    if len(Q) == 0:
        Q = T[:1].copy()
    return Q, T


@functools.lru_cache(maxsize=None)
def small():
    """96 pairs of 40 to 1500 bases at 0 / 2 / 10 / 25 % divergence and length ratios 0.9 / 1.0 / 1.1, with one empty query, one empty
    target, one base code 9 and two pairs on one target.  A candidate that is not usable() is left out and the next one drawn."""
    rng = np.random.default_rng(20250917)
    pairs = []
    while len(pairs) < N_SMALL:
        k = len(pairs)
        q, t = _draw_small_pair(rng, k)
        if k == SHARES_TO:
            t = pairs[SHARES_FROM][1]
            q = _substituted(rng, t, 0.10)
        if not usable(q, t):
            continue
        pairs.append((q, t))
    pairs[EMPTY_QUERY] = (np.zeros(0, np.uint8), pairs[EMPTY_QUERY][1])
    pairs[EMPTY_TARGET] = (pairs[EMPTY_TARGET][0], np.zeros(0, np.uint8))
    bad = pairs[BAD_BASE][0].copy()
    bad[len(bad) // 2] = 9
    pairs[BAD_BASE] = (bad, pairs[BAD_BASE][1])
    return Corpus(pairs, {SHARES_TO: SHARES_FROM})


@functools.lru_cache(maxsize=None)
def same_lengths(seed):
    """the lengths and offsets of small() with fresh bases: the query lengths are fixed first, then the bases drawn -- targets iid, queries the
    target's prefix (or the target and fresh bases behind it) with substitutions only, so that one plan serves small() and every seed"""
    base = small()
    rng = np.random.default_rng(7000 + seed)
    pairs = []
    for k in range(len(base)):
        ql, tl = int(base.qlen[k]), int(base.tlen[k])
        div = (0.0, 0.02, 0.10, 0.25)[k % 4]
        while True:
            T = pairs[SHARES_FROM][1] if k == SHARES_TO else rng.integers(0, 4, size=tl).astype(np.uint8)
            Q = _substituted(rng, T, div)[:ql]
            if len(Q) < ql:
                Q = np.concatenate([Q, rng.integers(0, 4, size=ql - len(Q)).astype(np.uint8)])
            if ql == 0 or tl == 0 or usable(Q, T):
                break
        if k == BAD_BASE:
            Q[len(Q) // 3] = 9
        pairs.append((Q, T))
    c = Corpus(pairs, {SHARES_TO: SHARES_FROM})
    assert np.array_equal(c.qlen, base.qlen) and np.array_equal(c.tlen, base.tlen) and np.array_equal(c.qoff, base.qoff) and np.array_equal(c.toff, base.toff)
    return c


N_SHORT = 16400          # just above the 16384 counts at which the exclusive scans of the CIGAR compaction go over many blocks


@functools.lru_cache(maxsize=None)
def short_many():
    """16 400 pairs of 20 to 40 bases: identical, one substitution, or a substitution and a deletion"""
    rng = np.random.default_rng(16400)
    lens = rng.integers(20, 41, size=N_SHORT)
    pairs = []
    for k in range(N_SHORT):
        T = rng.integers(0, 4, size=int(lens[k])).astype(np.uint8)
        Q = T.copy()
        if k % 3:
            Q[int(rng.integers(len(Q)))] ^= 1
        if k % 5 == 0 and len(Q) > 25:
            Q = np.delete(Q, int(rng.integers(5, 20)))
        pairs.append((Q, T))
    return Corpus(pairs)


MIXED_LENS = [1, 5, 30, 60, 64, 65, 100, 128, 129, 200, 256, 257, 300, 700, 1200]


@functools.lru_cache(maxsize=None)
def mixed_whole_query():
    """60 pairs whose query lengths fall into every width class of the whole-query dispatch (64 / 128 / 256 columns and above), for
    bsa_align_batch at bandwidth 0, which sends each class down as a sub-batch of its own"""
    rng = np.random.default_rng(515)
    cfg = ("align", S.MODE_GLOBAL, 0, SCORINGS["affine"])
    pairs = []
    while len(pairs) < 60:
        k = len(pairs)
        T = rng.integers(0, 4, size=MIXED_LENS[(7 * k) % len(MIXED_LENS)]).astype(np.uint8)
        Q = S.mutate(rng, T, (0.0, 0.05, 0.2)[k % 3])
        Q = Q[:max(1, int(len(Q) * (1.0, 1.0, 0.7)[(k // 3) % 3]))]
        if len(Q) == 0:
            Q = T[:1].copy()
        if _oracle(Q, T, *cfg)[2] != S.ORC_ERR_TRACE:
            pairs.append((Q, T))
    return Corpus(pairs)


_EXPECTED = {}


def expected(pairs, kind, mode, bw, scoring, key=None):
    """what bsa_align_run / bsa_edit_run must leave for `pairs` (a list of (q, t)): records (n, 10) int32, the list of CIGAR word arrays,
    cigar_off (n + 1, uint64) and status (n, uint32).  Results are the C oracle's; status follows include/bsalign_hip.h: a base code above 3
    is BSA_ST_BAD_BASE, an empty sequence BSA_ST_EMPTY, both with a zero record and no words.  A pair the oracle reports as ORC_ERR_TRACE
    has no expected result: it must not be in a corpus (AssertionError).  key: a name for `pairs` under which the result is kept and shared
    between tests (read-only arrays)."""
    ck = (key, kind, mode, bw, scoring)
    if key is not None and ck in _EXPECTED:
        return _EXPECTED[ck]
    n = len(pairs)
    rec = np.zeros((n, 10), dtype=np.int32)
    st = np.zeros(n, dtype=np.uint32)
    cigs = []
    for k, (q, t) in enumerate(pairs):
        if len(q) == 0 or len(t) == 0:
            st[k] = ST_EMPTY
            cigs.append(np.zeros(0, dtype=np.uint32))
            continue
        if int(max(np.max(q), np.max(t))) > 3:
            st[k] = ST_BAD_BASE
            cigs.append(np.zeros(0, dtype=np.uint32))
            continue
        res, cig, m = _oracle(q, t, kind, mode, bw, scoring)
        assert m != S.ORC_ERR_TRACE, "pair %d: the reference's traceback does not terminate on it (%s mode %d bandwidth %d)" % (k, kind, mode, bw)
        assert m >= 0, (k, m)
        rec[k] = res
        cigs.append(cig.astype(np.uint32))
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cigs], dtype=np.uint64)
    for a in [rec, st, off] + cigs:
        a.setflags(write=False)
    r = (rec, cigs, off, st)
    if key is not None:
        _EXPECTED[ck] = r
    return r


def check_arena(words, cap, sentinel, exp_off, exp_cigs, all_fitting_present):
    """words: the caller's whole allocation (uint32, the arena's `cap` words and the guard words behind them), filled with `sentinel` before the
    run.  Asserts that nothing at or above `cap` was touched, that exp_off is n + 1 monotone offsets that agree with exp_cigs, and that every
    pair's range inside the arena holds either exactly its words or only the sentinel; with all_fitting_present every pair whose words end
    inside the arena must be there.  Returns the number of pairs whose words are there (pairs without words do not count)."""
    words = np.asarray(words, dtype=np.uint32)
    n = len(exp_cigs)
    off = np.asarray(exp_off)
    assert off.ndim == 1 and len(off) == n + 1, "cigar_off: %d entries for %d pairs" % (len(off), n)
    off = off.astype(np.int64)
    lens = np.array([len(c) for c in exp_cigs], dtype=np.int64)
    assert off[0] == 0 and np.array_equal(np.diff(off), lens), "cigar_off is not the running sum of the pairs' word counts"
    total = int(off[n])
    assert 0 <= cap <= len(words)
    full = np.concatenate([np.asarray(c, dtype=np.uint32) for c in exp_cigs] + [np.zeros(0, dtype=np.uint32)])
    assert not (full == np.uint32(sentinel)).any(), "the sentinel is a word of the expected CIGARs: choose another"
    touched = np.flatnonzero(words[cap:] != np.uint32(sentinel))
    assert touched.size == 0, "word %d, at or above the capacity %d, was written" % (cap + int(touched[0]), cap)
    m = min(cap, total)
    behind = np.flatnonzero(words[m:cap] != np.uint32(sentinel))
    assert behind.size == 0, "word %d, behind the last pair's words, was written" % (m + int(behind[0]))
    # per pair: how many words of its range [off[k], min(off[k + 1], cap)) equal its own words / the sentinel
    ceq = np.concatenate([[0], np.cumsum(words[:m] == full[:m])])
    cse = np.concatenate([[0], np.cumsum(words[:m] == np.uint32(sentinel))])
    lo, hi = np.minimum(off[:-1], m), np.minimum(off[1:], m)
    fits = off[1:] <= cap
    present = fits & (lens > 0) & (ceq[hi] - ceq[lo] == lens)
    absent = (cse[hi] - cse[lo]) == (hi - lo)
    torn = np.flatnonzero((lens > 0) & ~present & ~absent)
    assert torn.size == 0, "pair %d: its range [%d, %d) holds neither its words nor nothing (capacity %d)" % (int(torn[0]), off[torn[0]], off[torn[0] + 1], cap)
    if all_fitting_present:
        missing = np.flatnonzero(fits & (lens > 0) & ~present)
        assert missing.size == 0, "pair %d fits the arena ([%d, %d) of %d words) and is not there" % (int(missing[0]), off[missing[0]], off[missing[0] + 1], cap)
    return int(present.sum())
