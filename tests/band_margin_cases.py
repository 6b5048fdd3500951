"""BSA_MODE_BAND_MARGIN: the reference statement of the margin and the seeded corpora of test_band_margin_cpu.py and test_band_margin_gpu.py, so
that what the CPU file vets against the oracle (shares of margins 0, of margins inside the band's half and of pairs the reference cannot trace) is
exactly what the GPU file sends."""
import functools

import numpy as np

import support as S

G, O, E = S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND
MODES = (G, O, E)
NONE = 0xFFFF

SC = {
    "linear": (2, -6, 0, -3, 0, 0),
    "affine": (2, -6, -3, -2, 0, 0),
    "paper": (2, -2, -4, -2, 0, 0),
    "twopiece": (2, -6, -3, -2, -8, -1),
}
BANDWIDTHS = (16, 48, 64, 128, 256, 512, 1024)       # moving bands; bandwidth 0 has corpora of its own (whole-query bands: every margin NONE)


def roundup16(x):
    return (int(x) + 15) // 16 * 16


def margin_ref(qlen, tlen, bandwidth, res, cigar, begs):
    """the definition of include/bsalign_hip.h, vertex by vertex.  res: the record (score, qb, qe, tb, te, ...); cigar: plain or = / X words
    (len << 4 | op); begs[r]: band offset of target row r."""
    B = roundup16(bandwidth if bandwidth else qlen)
    if len(cigar) == 0:
        return NONE
    best = [None]

    def visit(i, j):
        if i < 1 or j < 1:
            return
        r, c = i - 1, j - 1
        b = int(begs[r])
        if b > 0:
            best[0] = c - b if best[0] is None else min(best[0], c - b)
        if b + B < qlen:
            v = b + B - 1 - c
            best[0] = v if best[0] is None else min(best[0], v)

    i, j = int(res[3]), int(res[1])
    visit(i, j)
    for w in np.asarray(cigar, dtype=np.uint32).tolist():
        op, ln = w & 15, w >> 4
        for _ in range(ln):
            if op in (0, 7, 8):
                i, j = i + 1, j + 1
            elif op == 1:
                j += 1
            elif op == 2:
                i += 1
            else:
                raise ValueError("margin_ref: CIGAR op %d" % op)
            visit(i, j)
    if best[0] is None:
        return NONE
    return min(max(best[0], 0), 0xFFFE)          # (a value below 0 -- a cell outside its row's band -- counts as 0)


def _burst(rng, T, at, n, insert):
    """a burst of n inserted (random) or deleted bases in a copy of T at position `at`"""
    if insert:
        return np.concatenate([T[:at], rng.integers(0, 4, size=n).astype(np.uint8), T[at:]])
    return np.concatenate([T[:at], T[at + n:]])


@functools.lru_cache(maxsize=None)
def corpus(bw):
    """pairs for one bandwidth, in five kinds: clean diagonals and scattered small indels, drifts of a good part of the band spread over many
    rows (margins inside the band's half), inserted and deleted bursts longer than the band (margin 0 where the alignment crosses them), and
    queries no longer than the band (whole-query: NONE)."""
    if bw == 0:
        raise KeyError(bw)
    rng = np.random.default_rng(7000 + bw)
    n = 50 if bw <= 256 else 20
    lo, hi = (max(6 * bw, 200), max(10 * bw, 400)) if bw <= 256 else (3 * bw, 4 * bw)
    pairs = []
    for k in range(n):
        kind = k % 5
        L = int(rng.integers(lo, hi))
        if kind in (2, 3):       # (flanks of at least four bands on both sides of a burst: in overlap and extend mode the alignment must gain more by crossing it than by ending in front of it)
            L = int(rng.integers(10 * bw, 12 * bw)) if bw <= 256 else 8 * bw + int(rng.integers(0, 64))
        T = rng.integers(0, 4, size=L).astype(np.uint8)
        if kind == 0 and k % 10 == 0:
            Q = S.mutate(rng, T, 0.01, ratio=(100, 0, 0))
        elif kind == 0:
            Q = S.mutate(rng, T, 0.08)
        elif kind == 1:          # a run of small gaps, all on one side, adding up to a quarter .. three quarters of the band
            Q = T.copy()
            total, ins = int(rng.integers(bw // 4, 3 * bw // 4 + 1)), bool(rng.integers(2))
            at = int(rng.integers(L // 8, L // 4))
            while total > 0:
                g = min(total, int(rng.integers(1, 4)))
                Q = _burst(rng, Q, at, g, ins)
                at += int(rng.integers(8, 24))
                total -= g
        elif kind in (2, 3):     # one burst longer than the band, inserted (2) or deleted (3), in the middle
            Q = _burst(rng, T, int(rng.integers(9 * L // 20, 11 * L // 20)), int(rng.integers(bw + 4, bw + 20)), kind == 2)
        else:
            Q = S.mutate(rng, T[:int(rng.integers(max(bw // 2, 4), bw + 1))], 0.05)[:bw]
        if len(Q) == 0:
            Q = np.array([0], dtype=np.uint8)
        pairs.append((Q, T))
    return pairs


@functools.lru_cache(maxsize=None)
def whole_corpus(name):
    """bandwidth 0: `short` (queries up to 256 bases: the static register kernels), `long` (above 256: the systolic kernel), `mixed`"""
    rng = np.random.default_rng({"short": 7101, "long": 7102, "mixed": 7103}[name])
    lens = {"short": [20, 60, 100, 200, 240], "long": [300, 500, 900, 1500], "mixed": [20, 100, 240, 300, 900]}[name]
    pairs = []
    for _ in range(24):
        T = rng.integers(0, 4, size=int(rng.choice(lens))).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice([0.02, 0.1])))
        if name == "short":
            Q = Q[:256]
        if name == "long" and len(Q) <= 256:
            Q = np.concatenate([Q, rng.integers(0, 4, size=300).astype(np.uint8)])
        if len(Q) == 0:
            Q = np.array([0], dtype=np.uint8)
        pairs.append((Q, T))
    return pairs


def pairs_of(bw, which="short"):
    return corpus(bw) if bw else whole_corpus(which)


@functools.lru_cache(maxsize=None)
def oracle(bw, mode, scname, which="short"):
    """[(record, CIGAR words, word count or ORC_ERR_TRACE, begs)] of a corpus under one parameter set"""
    return [S.oracle_align(q, t, mode, bw, *SC[scname], want_begs=True) for q, t in pairs_of(bw, which)]


def expected(bw, mode, scname, which="short"):
    """the margin of every pair from the oracle's record, CIGAR and band trajectory; None where the reference's traceback does not terminate"""
    out = []
    for (q, t), (res, cig, n, begs) in zip(pairs_of(bw, which), oracle(bw, mode, scname, which)):
        out.append(None if n == S.ORC_ERR_TRACE else margin_ref(len(q), len(t), bw, res, cig, begs))
    return out


MAX_UNTRACEABLE = 0.02       # share of a corpus the oracle may report as ORC_ERR_TRACE (the GPU test compares those by status only)
