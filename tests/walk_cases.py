"""A named corpus for the traceback walkers: long gaps, gaps at every tile and window phase, CIGAR token counts around the walkers' token buffers,
paths on a band edge and long overhangs.  test_walk_corpus_cpu.py shows on the oracle alone that every group holds what it claims;
test_walk_corpus_gpu.py sends the same pairs through every walker.  Test code only; every pair is built once (lru_cache) and never changed, and the
oracle's answers are kept per (pair, mode, scoring, bandwidth) for both files.

Nothing here restates a kernel's window arithmetic: the positions are swept (phase_sweep), and what a group holds is read from the oracle's CIGAR
words and band offsets.

Alphabets.  "random": four letters, random inserted bases -- affine and two-piece gaps keep a planted run as one word.  "disjoint": sequences over
{0, 1, 2}, planted stretches all base 3 -- linear gaps and the edit distance, which would spread a random insert over several words, keep it whole.

Largest planted run g that stays ONE word per bandwidth (GMAX; properties of the reference's band steering, asserted against the oracle in
test_walk_corpus_cpu.py, beyond them the band loses the path and the run fragments):
    affine, -gapo 4, two-piece   64: 40    128: 70    256: 150    whole-query band: 300
    linear (disjoint)            64: 40    128: 70    256: 130    whole-query band: 300
    edit (disjoint)              64: 20    128: 40    256: 100    whole-query band: 300
    a scoring outside the static guard (whole-query bands only, "chk"): 65 -- its gap extension of -12 makes 400 shifted columns cheaper than two longer runs
"""
import functools

import numpy as np

import band_margin_cases as K
import support as S

G, O, E = S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND
MODES = (G, O, E)

SC = {
    "affine": (2, -6, -3, -2, 0, 0),             # the benchmark's: code format 1 at bandwidth 128
    "go4": (2, -6, -4, -2, 0, 0),                # -gapo = 4: four planes
    "linear": (2, -6, 0, -3, 0, 0),
    "twopiece": (2, -6, -3, -2, -8, -1),
    "twopiece19": (2, -6, -6, -2, -19, -1),       # a long second piece that the compact path still takes: m + 3 (19 + 1) = 62 <= 64
    "twopiece23": (2, -6, -6, -2, -23, -1),       # ... and one it does not (m + 3 x 24 = 74): banded batches run the row-record kernels
    "chk": (2, -6, -10, -12, 0, 0),              # m + 3 g = 68 > 64: outside the static guard of the whole-query kernel, which then checks every pair
}
KIND = {"affine": "random", "go4": "random", "twopiece": "random", "twopiece19": "random", "twopiece23": "random", "chk": "random", "linear": "disjoint", "edit": "disjoint"}
_GKEY = {"affine": "random", "go4": "random", "twopiece": "random", "twopiece19": "random", "twopiece23": "random", "chk": "chk", "linear": "linear", "edit": "edit"}
GMAX = {
    "random": {64: 40, 128: 70, 256: 150, 0: 300},
    "linear": {64: 40, 128: 70, 256: 130, 0: 300},
    "edit": {64: 20, 128: 40, 256: 100, 0: 300},
    "chk": {0: 65},
}
LADDER = (8, 17, 24, 33, 40, 56, 65, 70, 100, 130, 150, 200, 300)
SWEEP_G, SWEEP_STEP, SWEEP_N, SWEEP_P0 = 24, 7, 74, 250          # 7 is coprime to 64; 7 x 73 = 511 columns
TOKEN_COUNTS = (62, 63, 64, 65, 127, 128, 129)
TOKEN_STEP, TOKEN_LONG, TOKEN_FROM_END = 12, 20, (63, 64, 65)
ADJ_G = 20
ADJ_DI = {64: (20, 36), 128: (40, 84), 256: (70, 176)}          # (rows in front of the stretch, leading insertion): see adjacent()


class Case:
    """one pair and what was planted in it"""
    __slots__ = ("name", "group", "q", "t", "info")

    def __init__(self, name, group, q, t, **info):
        self.name, self.group, self.info = name, group, info
        self.q, self.t = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
        self.q.setflags(write=False)
        self.t.setflags(write=False)

    def __repr__(self):
        return "%s (%d x %d)" % (self.name, len(self.q), len(self.t))


def gmax(scname, bw):
    return GMAX[_GKEY[scname]][bw]


def ladder(scname, bw):
    """8, 17, 24, 33, 40 and on to the largest run that stays one word under this scoring at this bandwidth"""
    top = gmax(scname, bw)
    return sorted({g for g in LADDER if g <= top} | {top})


def _alpha(kind):
    return 4 if kind == "random" else 3


def _stretch(rng, kind, g):
    return rng.integers(0, 4, size=g).astype(np.uint8) if kind == "random" else np.full(g, 3, np.uint8)


def _noisy(rng, seq, kind, keep_out, sub=0.02, indel=0.01):
    """a copy of seq with substitutions and single-base indels, none within 10 bases of a position in keep_out"""
    a = _alpha(kind)
    out = []
    for x, b in enumerate(seq.tolist()):
        if b >= a or any(lo - 10 <= x <= hi + 10 for lo, hi in keep_out):
            out.append(b)
            continue
        r = rng.random()
        if r < sub:
            out.append((b + 1 + int(rng.integers(a - 1))) % a)
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out.extend([int(rng.integers(a)), b])
        else:
            out.append(b)
    return np.array(out, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def long_gap_case(kind, g):
    """1500 target bases; the query carries an inserted stretch of g bases behind target column 700 and lacks the g target bases from 1100 on:
    one I run and one D run of g, 400 columns apart, between stretches with 2 % substitutions (no other indels: the longest runs leave the band no room for drift)"""
    rng = np.random.default_rng(81000 + g + (0 if kind == "random" else 500))
    T = rng.integers(0, _alpha(kind), size=1500).astype(np.uint8)
    if kind == "disjoint":
        T[1100:1100 + g] = 3
    parts = [_noisy(rng, T[:700], kind, [(0, 0), (700, 700)], indel=0.0), _stretch(rng, kind, g),
             _noisy(rng, T[700:1100], kind, [(0, 0), (400, 400)], indel=0.0), _noisy(rng, T[1100 + g:], kind, [(0, 0)], indel=0.0)]
    return Case("long_gap/%s/g%d" % (kind, g), "long_gap", np.concatenate(parts), T, ins=g, dele=g)


def long_gap(bw, scname):
    return [long_gap_case(KIND[scname], g) for g in ladder(scname, bw)]


@functools.lru_cache(maxsize=None)
def _sweep_base(kind):
    rng = np.random.default_rng(82000 + (0 if kind == "random" else 500))
    T = rng.integers(0, _alpha(kind), size=1300).astype(np.uint8)
    lo, hi = SWEEP_P0 - 16, SWEEP_P0 + SWEEP_STEP * SWEEP_N + 64
    head, tail = _noisy(rng, T[:lo], kind, [(0, 0)]), _noisy(rng, T[hi:], kind, [(0, 0)])        # (the swept stretch itself stays clean: the planted run is the only event in it)
    return T, head, tail, lo, hi, rng.integers(0, 4, size=64).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def phase_sweep(kind, which, g=SWEEP_G, step=SWEEP_STEP):
    """the same pair with one run of g -- which = "I": inserted, "D": deleted -- at target column p0 + step j, j = 0 .. 73: every phase of a 64-row tile
    once, and a span above 512 columns"""
    T, head, tail, lo, hi, junk = _sweep_base(kind)
    out = []
    for j in range(SWEEP_N):
        p = SWEEP_P0 + step * j
        if which == "I":
            ins = junk[:g] if kind == "random" else np.full(g, 3, np.uint8)
            q, t = np.concatenate([head, T[lo:p], ins, T[p:hi], tail]), T
            info = dict(ins=g)
        else:
            t = T.copy()
            if kind == "disjoint":
                t = np.concatenate([T[:p], np.full(g, 3, np.uint8), T[p:]])
                q = np.concatenate([head, T[lo:hi], tail])
            else:
                q = np.concatenate([head, T[lo:p], T[p + g:hi], tail])
            info = dict(dele=g)
        out.append(Case("phase_sweep/%s/%s%d@%d" % (kind, which, g, p), "phase_sweep", q, t, **info))
    return out


def _token_pair(n, long_from_end=None):
    """n gap events TOKEN_STEP columns apart, deletions and insertions of one base in turn, sequences over {0, 1, 2}; event number long_from_end,
    counted from the END of the alignment, is a deletion of TOKEN_LONG bases of 3 instead"""
    rng = np.random.default_rng(83000 + n)
    L = 120 + TOKEN_STEP * n
    T = rng.integers(0, 3, size=L).astype(np.uint8)
    tp, qp, at = [], [], 0
    for e in range(n):
        c = 60 + TOKEN_STEP * e
        tp.append(T[at:c])
        qp.append(T[at:c])
        at = c
        if long_from_end is not None and e == n - long_from_end:
            tp.append(np.full(TOKEN_LONG, 3, np.uint8))               # in the target only: a deletion of 20 rows
        elif e % 2 == 0:
            tp.append(T[c:c + 1])                                       # in the target only: a deletion of one
            at = c + 1
        else:
            b = (int(T[c - 1]) + 1 + int(rng.integers(2))) % 3          # differs from the base in front of it
            if b == int(T[c]):
                b = (b + 1) % 3 if (b + 1) % 3 != int(T[c - 1]) else b
            qp.append(np.array([b], np.uint8))                         # in the query only: an insertion of one
    tp.append(T[at:])
    qp.append(T[at:])
    return np.concatenate(qp), np.concatenate(tp)


@functools.lru_cache(maxsize=None)
def tokens():
    out = []
    for n in TOKEN_COUNTS:
        q, t = _token_pair(n)
        out.append(Case("tokens/n%d" % n, "tokens", q, t, gaps=n))
        for k in TOKEN_FROM_END:
            if k <= n:
                q, t = _token_pair(n, k)
                out.append(Case("tokens/n%d/long-D-%d-from-end" % (n, k), "tokens", q, t, gaps=n, long_from_end=k))
    return out


@functools.lru_cache(maxsize=None)
def adjacent(bw):
    """an I run and a D run with no match column between them: 20 bases of 3 in the query against 20 bases of 2 in the target, inside sequences over
    {0, 1}; affine and two-piece gaps only (two runs beat 20 mismatches at -6; under linear gaps and the edit distance they do not).
    "ID": in the middle of the pair -- the two orders score the same and the reference's traceback takes the deletion first, walking backwards: I then D.
    "DI": only where the band decides -- behind a leading insertion the cell above and to the right of the stretch lies outside the band, so the walk
    has to take the insertion first: D then I.  (rows in front, leading insertion) per bandwidth were found by search on the oracle (ADJ_DI); a
    whole-query band never cuts that cell off, so bandwidth 0 has the first order only."""
    rng = np.random.default_rng(84000)
    T0 = rng.integers(0, 2, size=1200).astype(np.uint8)
    q3, t2 = np.full(ADJ_G, 3, np.uint8), np.full(ADJ_G, 2, np.uint8)
    out = [Case("adjacent/ID", "adjacent", np.concatenate([T0[:600], q3, T0[600:]]), np.concatenate([T0[:600], t2, T0[600:]]), order=(1, 2))]
    if bw in ADJ_DI:
        a, lead = ADJ_DI[bw]
        out.append(Case("adjacent/DI/bw%d" % bw, "adjacent", np.concatenate([np.full(lead, 3, np.uint8), T0[:a], q3, T0[a:]]),
                        np.concatenate([T0[:a], t2, T0[a:]]), order=(2, 1)))
    return out


EDGE_SHAPES = (("rand", 100, 500, 1300), ("3", 100, 500, 900), ("3", 20, 480, 1200), ("3", 10, 490, 1300))


@functools.lru_cache(maxsize=None)
def edges(bw):
    """paths on a band edge.  "forced": the target carries a stretch of 900 .. 1300 bases the query lacks; in global mode the reference's steering keeps
    the band within a bandwidth of the proportional diagonal, so the band is dragged across the deletion run and the path rides on its first column
    for hundreds of rows -- which is also where the walk keeps meeting the first column of the PREVIOUS row's band (cpm_rows).  "drift-D3": one
    deletion every 3 rows for 900 rows; the band follows such a drift, the path stays inside (no row on an edge: a drift alone does not reach that
    column).  "margin": the first pair of each drift kind (spread drift, inserted burst, deleted burst) of band_margin_cases.corpus(bw), by reference.
    Searched and not found: a path that stays on an edge under a long second gap piece at bandwidth 256 (a run of hundreds of rows costs little
    there, the path leaves the edge at once), and any single path on an edge for 200 rows that is not forced there by the steering."""
    rng = np.random.default_rng(85000)
    X = rng.integers(0, 3, size=700).astype(np.uint8)
    out = []
    for jk, a, b, junk in EDGE_SHAPES:
        A, B_ = X[:a], X[a:a + b]
        J = np.full(junk, 3, np.uint8) if jk == "3" else rng.integers(0, 4, size=junk).astype(np.uint8)
        out.append(Case("edges/forced/%s-%d-%d-%d" % (jk, a, b, junk), "edges", np.concatenate([A, B_]), np.concatenate([A, J, B_]), forced=True))
    T = rng.integers(0, 4, size=1400).astype(np.uint8)
    keep = np.ones(len(T), bool)
    keep[300:1200:3] = False
    out.append(Case("edges/drift-D3", "edges", T[keep], T, drift=300))
    if bw:
        pairs = K.corpus(bw)
        for k in (1, 2, 3):
            out.append(Case("edges/margin/bw%d-kind%d" % (bw, k), "edges", pairs[k][0], pairs[k][1]))
    return out


@functools.lru_cache(maxsize=None)
def overhang():
    """a core of 800 bases (3 % errors) with 60 or 300 random bases in front of or behind either sequence"""
    rng = np.random.default_rng(86000)
    T0 = rng.integers(0, 4, size=800).astype(np.uint8)
    Q0 = S.mutate(rng, T0, 0.03)
    junk = rng.integers(0, 4, size=300).astype(np.uint8)
    out = []
    for n in (60, 300):
        out.append(Case("overhang/q-lead-%d" % n, "overhang", np.concatenate([junk[:n], Q0]), T0))
        out.append(Case("overhang/q-trail-%d" % n, "overhang", np.concatenate([Q0, junk[:n]]), T0))
        out.append(Case("overhang/t-lead-%d" % n, "overhang", Q0, np.concatenate([junk[:n], T0])))
        out.append(Case("overhang/t-trail-%d" % n, "overhang", Q0, np.concatenate([T0, junk[:n]])))
    return out


def sweep_g(scname, bw):
    return min(SWEEP_G, gmax(scname, bw))          # (edit distance at bandwidth 64: 20)


def cases(bw, scname, mode=G, step=SWEEP_STEP):
    """every group that fits (scoring, bandwidth, mode) in one list: overlap and extend mode get the overhangs alone"""
    if mode != G:
        return list(overhang())
    kind = KIND[scname]
    g = sweep_g(scname, bw)
    out = long_gap(bw, scname) + phase_sweep(kind, "I", g, step) + phase_sweep(kind, "D", g, step)
    if scname != "chk":
        out += tokens()
    if kind == "random" and scname != "chk":
        out += adjacent(bw)
    return out + edges(bw) + overhang()


# ---- the pairs a code walker declines in global mode: the literal kernels answer for them (bsa_ctx_last_handover counts them)
# The oracle's restatement of the code walk (backcal_codes) names two situations: a deletion run that climbs to row -1 under affine gaps, and, with
# two-piece gaps, a deletion decided at query column 0.  A search over 3000 short pairs with overhangs of 0 .. 80 bases on either sequence found the first
# under none of the one-piece scorings above (row -1 holds the -63 sentinel, which scores this small never meet) and the second under "twopiece" on
# the seeds below; the same search is why every other group is expected to be walked to the end.  test_walk_corpus_cpu.py holds both statements
# against the restatement.
DECLINE_SEEDS = (49, 254, 373, 2343)
DECLINE = {(64, "twopiece"): (49, 254, 373, 2343), (128, "twopiece"): (49, 373, 2343), (256, "twopiece"): (49, 373, 2343)}


@functools.lru_cache(maxsize=None)
def _decline_case(seed):
    rng = np.random.default_rng(70000 + seed)
    T = rng.integers(0, 4, size=int(rng.choice([30, 60, 100, 200]))).astype(np.uint8)
    Q = S.mutate(rng, T, float(rng.choice([0.05, 0.2, 0.4])))
    lt, lq = int(rng.choice([0, 1, 3, 10, 40, 80])), int(rng.choice([0, 1, 3, 10, 40, 80]))
    t = np.concatenate([rng.integers(0, 4, size=lt).astype(np.uint8), T])
    q = np.concatenate([rng.integers(0, 4, size=lq).astype(np.uint8), Q])
    return Case("overhang/decline/%d" % seed, "decline", q, t)


def decline_candidates():
    return [_decline_case(s) for s in DECLINE_SEEDS]


def decline(bw, scname):
    """the named list for one configuration (global mode); empty where the walker is expected to decline nothing"""
    return [_decline_case(s) for s in DECLINE.get((bw, scname), ())]


def codes_walk_declines(case, mode, scname, bw):
    """does the oracle's restatement of the code walk hand this pair to the literal traceback?"""
    import ctypes as C
    o = S.oracle()
    o.orc_align_pairwise_codes_mode.restype = C.c_long
    o.orc_align_pairwise_codes_mode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_long]
    sc = SC[scname]
    mtx = S.score_matrix(sc[0], sc[1])
    res = np.zeros(10, np.int32)
    cap = 4 * (len(case.q) + len(case.t)) + 16
    cig = np.zeros(cap, np.uint32)
    n = o.orc_align_pairwise_codes_mode(case.q.ctypes.data, len(case.q), case.t.ctypes.data, len(case.t), mode, bw, mtx.ctypes.data, *sc[2:],
                                        res.ctypes.data, cig.ctypes.data, cap)
    return n == S.ORC_ERR_TRACE


# ---- the oracle, once per (pair, mode, scoring, bandwidth)
_ORACLE = {}


def oracle(case, mode, scname, bw):
    """(record, words, count, begs) -- begs is None for the edit distance"""
    key = (case.name, mode, scname, bw)
    if key not in _ORACLE:
        if scname == "edit":
            _ORACLE[key] = S.oracle_edit(case.q, case.t, mode, bw) + (None,)
        else:
            _ORACLE[key] = S.oracle_align(case.q, case.t, mode, bw, *SC[scname], want_begs=True)
    return _ORACLE[key]


def words(cig):
    return [(int(w) & 15, int(w) >> 4) for w in np.asarray(cig).tolist()]


def edge_rows(case, bw, res, cig, begs):
    """target rows on which the path's distance to a band edge is 0, vertex by vertex with the visit rule of band_margin_cases.margin_ref (an edge at
    the query's start or end does not count, a cell outside its row's band counts as 0); the minimum over all rows is margin_ref's value"""
    qlen = len(case.q)
    B = K.roundup16(bw if bw else qlen)
    per = {}

    def visit(i, j):
        if i < 1 or j < 1:
            return
        r, c = i - 1, j - 1
        b = int(begs[r])
        if b > 0:
            per[r] = min(per.get(r, 1 << 30), max(c - b, 0))
        if b + B < qlen:
            per[r] = min(per.get(r, 1 << 30), max(b + B - 1 - c, 0))

    i, j = int(res[3]), int(res[1])
    visit(i, j)
    for op, ln in words(cig):
        for _ in range(ln):
            i, j = i + (op != 1), j + (op != 2)
            visit(i, j)
    return per


def cpm_rows(res, cig, begs):
    """rows y >= 1 in which the path visits column begs[y - 1], the first column of the previous row's band"""
    hit = set()
    i, j = int(res[3]), int(res[1])
    for op, ln in words(cig):
        for _ in range(ln):
            i, j = i + (op != 1), j + (op != 2)
            if i >= 2 and j >= 1 and j - 1 == int(begs[i - 2]):
                hit.add(i - 1)
    return hit
