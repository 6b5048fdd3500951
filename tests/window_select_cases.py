"""bsa_window_select_* (include/bsalign_hip.h): the definition in Python (window_select_ref: the candidate test clause by clause, then a sort by the
stated order and nothing cleverer), mix32 with its inverse -- the finaliser is a bijection, so a case can ask for a piece with any key it likes --
and hand-made windows: the smallest shapes at which the pass can go wrong."""
from collections import namedtuple

import numpy as np

PIECE_DTYPE = np.dtype([("pair", np.uint32), ("q_first", np.uint32), ("len", np.uint32), ("t_first", np.uint32), ("t_last", np.uint32), ("reserved", np.uint32),
                        ("base_off", np.uint64)])
RESULT_DTYPE = np.dtype([(n, np.int32) for n in ("score", "qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln")])
SYMBOLS = ("bsa_window_select_run", "bsa_window_select_batch")
FILL, FILL32, FILL64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
M32 = 0xFFFFFFFF
HELD = 512                                                     # a window of up to this many records keeps its keys in LDS (WSEL_HELD, bsa_window_select.hip)
DIGIT_BITS = 8                                                 # the radix selection's digit

Par = namedtuple("Par", "max_depth min_span ident_num ident_den seed", defaults=(0, 0, 0, 0, 0))


def need_symbols():
    """every test of bsa_window_select_* begins here: without the symbols none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in SYMBOLS:
        assert hasattr(B.lib(), name), "the library does not export " + name


def mix32(x):
    """the header's finaliser, in Python integers"""
    x &= M32
    x ^= x >> 16
    x = x * 0x85EBCA6B & M32
    x ^= x >> 13
    x = x * 0xC2B2AE35 & M32
    x ^= x >> 16
    return x


def unmix32(h):
    """its inverse: every step of mix32 is a bijection of 32-bit words"""
    h &= M32
    h ^= h >> 16
    h = h * pow(0xC2B2AE35, -1, 1 << 32) & M32
    h ^= h >> 13
    h ^= h >> 26
    h = h * pow(0x85EBCA6B, -1, 1 << 32) & M32
    h ^= h >> 16
    return h


def key_of(sp, h):
    """the order as one number, the larger the better: span first, then the smaller hash"""
    return sp << 32 | (~h & M32)


def piece_with_key(key, seed=0, t_first=0, **fields):
    """a record whose key under `seed` is `key`: (pair, q_first, len, t_first, t_last, reserved, base_off)"""
    sp, h = key >> 32, ~key & M32
    assert t_first + sp <= M32
    return (unmix32(h) ^ seed, fields.get("q_first", 0), fields.get("len", 1), t_first, t_first + sp, fields.get("reserved", 0), fields.get("base_off", 0))


def is_candidate(rec, out, n, par):
    """the candidate test of the header, clause by clause, in Python integers: nothing wraps.  rec: the record's fields in their order; out: None or
    a list of (mat, aln)"""
    pair, _, ln, tf, tl = rec[:5]
    if not (tf <= tl and ln >= 1):
        return False
    sp = tl - tf
    if not (par.min_span <= 1 or sp >= par.min_span - 1):
        return False
    if par.ident_den != 0:
        assert out is not None
        if not pair < n:
            return False
        mat, aln = out[pair]
        if not (aln > 0 and mat >= 0 and mat * par.ident_den >= par.ident_num * aln):
            return False
    return True


class Ref:
    pass


def window_select_ref(piece, piece_off, piece_cap, out, par, n=None):
    """the definition -> Ref: sel_off (nwin + 1), ncand (nwin), sel (the records of a complete run), src (their indices in piece), win (a list over
    the windows of the selected indices, counted from the window's first piece)"""
    nwin = len(piece_off) - 1
    n = (len(out) if out is not None else 0) if n is None else n
    P = piece.tolist()                                         # Python integers from here on
    O = None if out is None else list(zip(out["mat"].tolist(), out["aln"].tolist()))
    r = Ref()
    r.sel_off, r.ncand, r.win = np.zeros(nwin + 1, dtype=np.uint64), np.zeros(nwin, dtype=np.uint32), []
    src = []
    for g in range(nwin):
        a, b = int(piece_off[g]), int(piece_off[g + 1])
        if b > piece_cap or b < a:
            a = b = 0                                          # no pieces
        cand = [j for j in range(a, b) if is_candidate(P[j], O, n, par)]
        if par.max_depth != 0 and len(cand) > par.max_depth:
            order = sorted(cand, key=lambda j: (-(P[j][4] - P[j][3]), mix32(P[j][0] ^ par.seed), j))          # larger sp, smaller h, smaller index
            kept = sorted(order[:par.max_depth])
        else:
            kept = cand
        r.ncand[g] = len(cand)
        r.win.append(np.array(kept, dtype=np.int64) - a)
        src += kept
        r.sel_off[g + 1] = len(src)
    r.src = np.array(src, dtype=np.uint32)
    r.sel = piece[r.src.astype(np.int64)].copy() if len(src) else np.zeros(0, PIECE_DTYPE)
    return r


def expected_arena(ref, sel_cap, alloc):
    """what a run with this sel_cap leaves in arrays of `alloc` records prefilled with 0xA5 -> (sel as bytes, sel_src)"""
    sel = np.full(alloc * 32, FILL, dtype=np.uint8)
    src = np.full(alloc, FILL32, dtype=np.uint32)
    for g in range(len(ref.sel_off) - 1):
        a, b = int(ref.sel_off[g]), int(ref.sel_off[g + 1])
        if b <= sel_cap:
            sel[32 * a:32 * b] = ref.sel[a:b].view(np.uint8).reshape(-1)
            src[a:b] = ref.src[a:b]
    return sel, src


def records(rows):
    return np.array([tuple(int(x) for x in r) for r in rows], dtype=PIECE_DTYPE) if len(rows) else np.zeros(0, PIECE_DTYPE)


def batch(windows):
    """a list of windows, each a list of records -> (piece, piece_off)"""
    off = np.zeros(len(windows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w in windows], dtype=np.uint64)
    return records([r for w in windows for r in w]), off


def results(mat_aln):
    """(mat, aln) pairs -> the aligner's records, the other fields noise"""
    out = np.zeros(len(mat_aln), dtype=RESULT_DTYPE)
    for name in RESULT_DTYPE.names:
        out[name] = 0x5A5A5A5A
    for k, (m, a) in enumerate(mat_aln):
        out[k]["mat"], out[k]["aln"] = m, a
    return out


# ---- the header's example, typed in ----------------------------------------------------------------------------------------------------------------------
def header_example():
    """-> (piece, piece_off, {(seed, max_depth): selected indices})"""
    piece, off = batch([[(0, 0, 10, 0, 9, 0, 0), (1, 0, 8, 2, 9, 0, 10), (2, 0, 10, 0, 9, 0, 18), (3, 0, 5, 0, 4, 0, 28), (4, 0, 10, 0, 9, 0, 33), (5, 0, 9, 1, 9, 0, 43)]])
    want = {(0, 0): [0, 1, 2, 4, 5], (0, 1): [0], (0, 2): [0, 4], (0, 3): [0, 2, 4], (0, 4): [0, 2, 4, 5], (1, 2): [0, 2]}
    return piece, off, want


HEADER_MIX32 = {0: 0x00000000, 2: 0x30F4C306, 4: 0x249CB285}
HEADER_IDENTITY = [((80, 100), True), ((8, 10), True), ((79, 100), False), ((0, 0), False)]          # with 4 / 5


# ---- random windows ---------------------------------------------------------------------------------------------------------------------------------------
def random_window(rng, depth, n, spans=8, bad=0.1):
    """`depth` records of pairs below n: few distinct spans, so that ties are the rule; some records are no pieces; every other byte is noise"""
    rows = []
    for _ in range(depth):
        tf = int(rng.integers(0, 1000))
        sp = int(rng.integers(0, spans))
        ln = int(rng.integers(1, 2000))
        tl = tf + sp
        u = rng.random()
        if u < bad / 2:
            ln = 0
        elif u < bad and tf > 0:
            tl = tf - 1
        rows.append((int(rng.integers(0, n)), int(rng.integers(0, 1 << 32)), ln, tf, tl, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 62))))
    return rows


def random_results(rng, n):
    """records around an identity of 4 / 5, with a few that no alignment gives"""
    out = results([(int(a * rng.uniform(0.6, 1.0)), a) for a in (int(rng.integers(1, 5000)) for _ in range(n))])
    for k in rng.choice(n, size=max(n // 10, 1), replace=False):
        out[k]["aln"] = int(rng.choice([0, -5]))
    for k in rng.choice(n, size=max(n // 20, 1), replace=False):
        out[k]["mat"] = -1
    return out


def depth_cases(rng, n):
    """one window of every depth the kernels treat differently: the trips of 64, the depth up to which keys stay in LDS, and one deep window"""
    depths = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200, HELD - 1, HELD, HELD + 1, 5000]
    return depths, [random_window(rng, d, n, spans=6) for d in depths]


def max_depths(ncand):
    """the caps for a batch whose windows have these candidate counts"""
    s = {0, 1, 2, 63, 64, 65, M32}
    for c in ncand:
        s |= {int(c) - 1, int(c), int(c) + 1}
    return sorted(x for x in s if 0 <= x <= M32)


# ---- keys -------------------------------------------------------------------------------------------------------------------------------------------------
def key_windows(seed):
    """-> a list of (name, records): windows whose keys are chosen"""
    ws = []
    ws.append(("spans distinct", [piece_with_key(key_of(sp, 0x1234), seed, t_first=7) for sp in (5, 3, 9, 0, 7, 1, 8, 2, 6, 4)]))
    ws.append(("spans equal", [piece_with_key(key_of(11, h), seed) for h in (0x80000000, 7, 0xFFFFFFFF, 0, 0x7FFFFFFF, 1, 0x12345678, 0xFFFFFFFE)]))
    ws.append(("one pair", [(77, j, 1 + j, 100, 140, j, 1000 * j) for j in range(80)]))
    # a run of equal keys from j = 60 to 70 between better and worse ones: the quota ends inside it
    run = [piece_with_key(key_of(9, 5), seed, q_first=j) for j in range(60)] + [piece_with_key(key_of(8, 99), seed, q_first=j) for j in range(60, 71)] \
        + [piece_with_key(key_of(7, j), seed, q_first=j) for j in range(71, 75)]
    ws.append(("quota in a run", run))
    ws.append(("extreme spans", [piece_with_key(key_of(sp, h), seed) for sp, h in ((0, 1), (M32, 1), (1, 1), (1 << 31, 1), (0, 0), (M32, 0), (1 << 31, 0), (1, 0))]))
    ws.append(("hash lowest bit", [piece_with_key(key_of(4, h), seed) for h in (0x40, 0x41, 0x40, 0x41, 0x41, 0x40)]))
    ws.append(("hash highest bit", [piece_with_key(key_of(4, h), seed) for h in (0x80000040, 0x40, 0x80000040, 0x40, 0x40, 0x80000040)]))
    # for every digit: a threshold with a neighbour one below and one above in that digit, without and with a borrow from the digit above; every key twice
    for shift in range(0, 64, DIGIT_BITS):
        keys = []
        for t in (0x8080808080808080, 0x8080808080808080 & ~(0xFF << shift), 0x8080808080808080 | 0xFF << shift):
            keys += [k for k in (t + (1 << shift), t, t - (1 << shift)) if 0 <= k < 1 << 64]
        keys += [0, (1 << 64) - 1]
        order = [keys[(5 * i) % len(keys)] for i in range(len(keys))] if len(keys) % 5 else keys
        ws.append(("digit at bit %d" % shift, [piece_with_key(k, seed) for k in order + order[::-1]]))
    return ws


# ---- filters --------------------------------------------------------------------------------------------------------------------------------------------------
def filter_cases():
    """-> a list of (name, piece, piece_off, out, n, Par, the candidates' indices): every clause of the candidate test on its border"""
    cs = []
    rec = lambda pair, tf, tl, ln=1: (pair, 0, ln, tf, tl, 0, 0)
    p, off = batch([[rec(0, 10, 13), rec(1, 10, 14), rec(2, 10, 15), rec(3, 0, 0)]])
    cs.append(("min_span 5", p, off, None, 0, Par(min_span=5), [1, 2]))
    cs.append(("min_span 0", p, off, None, 0, Par(min_span=0), [0, 1, 2, 3]))
    cs.append(("min_span 1", p, off, None, 0, Par(min_span=1), [0, 1, 2, 3]))
    cs.append(("min_span 2", p, off, None, 0, Par(min_span=2), [0, 1, 2]))
    p, off = batch([[rec(0, 0, M32), rec(1, 0, M32 - 1), rec(2, 1, M32), rec(3, 5, 5)]])
    cs.append(("min_span 2^32 - 1", p, off, None, 0, Par(min_span=M32), [0, 1, 2]))          # spans 2^32, 2^32 - 1, 2^32 - 1 columns
    p, off = batch([[rec(0, 0, M32), rec(1, 0, M32 - 1), rec(2, 0, M32 - 2)]])
    cs.append(("min_span 2^32 - 1, one short", p, off, None, 0, Par(min_span=M32), [0, 1]))
    # the identity: mat * den == num * aln exactly, and with mat one less; the header's four pairs; the largest values; records no alignment gives
    out = results([(80, 100), (79, 100), (8, 10), (0, 0), (7, 10), (0x7FFFFFFF, 0x7FFFFFFF), (0x7FFFFFFE, 0x7FFFFFFF), (5, 0), (5, -3), (-1, 10), (-1, -1), (0, 1)])
    p, off = batch([[rec(k, 0, 9) for k in range(len(out))]])
    cs.append(("identity 4 / 5", p, off, out, len(out), Par(ident_num=4, ident_den=5), [0, 2, 5, 6]))
    cs.append(("identity 1 / 1 in the largest numbers", p, off, out, len(out), Par(ident_num=M32, ident_den=M32), [5]))
    cs.append(("identity 0 / 1", p, off, out, len(out), Par(ident_num=0, ident_den=1), [0, 1, 2, 4, 5, 6, 11]))
    cs.append(("no identity test, records given", p, off, out, len(out), Par(ident_num=4, ident_den=0), list(range(len(out)))))
    # pair == n and pair = 2^32 - 1: outside with the identity test, a hash input without it
    out = results([(9, 10), (9, 10), (9, 10)])
    p, off = batch([[rec(2, 0, 9), rec(3, 0, 9), rec(M32, 0, 9), rec(0, 0, 9)]])
    cs.append(("pair == n, identity", p, off, out, 3, Par(ident_num=1, ident_den=2), [0, 3]))
    cs.append(("pair == n, a smaller n", p, off, out, 2, Par(ident_num=1, ident_den=2), [3]))
    cs.append(("pair == n, no identity", p, off, None, 3, Par(), [0, 1, 2, 3]))
    cs.append(("pair == n, no identity, capped", p, off, None, 3, Par(max_depth=2), None))
    # records that are no pieces
    p, off = batch([[rec(0, 5, 4), rec(1, 5, 5), rec(2, 5, 6, ln=0), rec(3, M32, 0), rec(4, 0, M32, ln=M32), rec(5, 1, 0, ln=0)]])
    cs.append(("no pieces", p, off, None, 0, Par(), [1, 4]))
    return cs


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------------------
def window_cases(rng):
    """-> a list of (name, piece, piece_off, piece_cap): offsets that make no sense, empty windows, one window, many"""
    cs = []
    ws = [random_window(rng, d, 50) for d in (5, 9, 0, 7, 70, 3)]
    piece, off = batch(ws)
    cs.append(("an empty window between full ones", piece, off, len(piece)))
    cs.append(("a piece_cap inside the fifth window", piece, off, int(off[5]) - 1))
    cs.append(("a piece_cap of 0", piece, off, 0))
    bad = off.copy()
    bad[2] = bad[1] - 2                                        # decreases: window 1 has no pieces, window 2 runs from there to its own end
    cs.append(("a piece_off that decreases", piece, bad, len(piece)))
    bad = off.copy()
    bad[3] = (1 << 64) - 1                                     # windows 2 and 3
    cs.append(("a piece_off of 2^64 - 1", piece, bad, len(piece)))
    cs.append(("one window", *batch([random_window(rng, 33, 50)]), 33))
    many = [random_window(rng, int(d), 200) for d in rng.choice([0, 1, 3, 17, 40, 64, 65, 90], size=1000)]
    piece, off = batch(many)
    cs.append(("1000 windows", piece, off, len(piece)))
    return cs
