"""bsa_window_realign_* (include/bsalign_hip.h): the definition in Python (window_realign_ref) -- the liftable window, the lift of a piece's span
through the window's = / X / I / D words, the re-alignable piece clause by clause, the banded DP with its traceback order, the trimming, the records,
the offsets and the arena rule --, an unbanded DP to hold the cost against, and the builders of the batches the tests upload: both worked examples of
the header typed in byte by byte, hand-made spans and paths, one window and one piece for every way each can fail, simulated windows, the closed loop
of window_msa_cases continued into a second round, and a homopolymer window.  No GPU is used here."""
import numpy as np

import window_msa_cases as W
from window_pieces_cases import PIECE_DTYPE

ST_OK, ST_NO_WINDOW, ST_BAD_PIECE, ST_TOO_LONG, ST_EMPTY_SPAN, ST_OFF_BAND, ST_NO_DIAG = 0, 1, 2, 3, 4, 5, 6
ST_EDGE = 0x100
OP_M, OP_I, OP_D, OP_EQ, OP_X = 0, 1, 2, 7, 8
FILL, FILL32, FILL64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
MAX_WINDOW2, MAX_MAX_LEN, BAND = 4096, 2048, 64
SYMBOLS = ("bsa_window_realign_run", "bsa_window_realign_batch")
REALIGN_PARAMS_FIELDS = ("window2", "max_len", "min_margin", "x", "g")
INF = 1 << 40


def need_symbols():
    """every test of bsa_window_realign_* begins here: without the symbols none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in SYMBOLS:
        assert hasattr(B.lib(), name), "the library does not export " + name


def par(window2, max_len=1024, min_margin=8, x=1, g=1):
    return dict(window2=window2, max_len=max_len, min_margin=min_margin, x=x, g=g)


def W_(*p):
    """(length, op) pairs -> words"""
    return np.array([n << 4 | op for n, op in p], dtype=np.uint32)


class RBatch:
    """the arguments of the calls: the piece records with their offsets by window and their codes (what bsa_window_pieces_* left), that round's
    window size, and the windows' sequences and words with their offsets (what bsa_window_stitch_* left)"""

    def __init__(self, piece, piece_off, bases, window, seq, seq_off, cig, cig_off, piece_cap=None, bases_cap=None, seq_cap=None, cig_cap=None):
        self.piece = np.ascontiguousarray(piece, dtype=PIECE_DTYPE)
        self.piece_off = np.ascontiguousarray(piece_off, dtype=np.uint64)
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.window = int(window)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        self.cig = np.ascontiguousarray(cig, dtype=np.uint32)
        self.cig_off = np.ascontiguousarray(cig_off, dtype=np.uint64)
        self.nwin = len(self.piece_off) - 1
        self.piece_cap = len(self.piece) if piece_cap is None else piece_cap
        self.bases_cap = len(self.bases) if bases_cap is None else bases_cap
        self.seq_cap = len(self.seq) if seq_cap is None else seq_cap
        self.cig_cap = len(self.cig) if cig_cap is None else cig_cap
        assert len(self.seq_off) == self.nwin + 1 and len(self.cig_off) == self.nwin + 1
        assert self.piece_cap <= len(self.piece) and self.bases_cap <= len(self.bases) and self.seq_cap <= len(self.seq) and self.cig_cap <= len(self.cig)


# ---- the definition ------------------------------------------------------------------------------------------------------------------------------
def liftable(b, g, window2):
    """-> None, or (slen, Ld, the words as (op, length) pairs), in Python integers: nothing wraps"""
    s0, s1, c0, c1 = int(b.seq_off[g]), int(b.seq_off[g + 1]), int(b.cig_off[g]), int(b.cig_off[g + 1])
    if not (s0 <= s1 <= b.seq_cap) or s1 - s0 > window2 or not (c0 <= c1 <= b.cig_cap):
        return None
    ws = [(int(w) & 15, int(w) >> 4) for w in b.cig[c0:c1]]
    if any(op not in (OP_I, OP_D, OP_EQ, OP_X) or n < 1 for op, n in ws):
        return None
    if sum(n for op, n in ws if op != OP_D) != s1 - s0:
        return None
    Ld = sum(n for op, n in ws if op != OP_I)
    if Ld > b.window:
        return None
    return s1 - s0, Ld, ws


def lift_tables(ws):
    """-> (s, k): for every draft column j the sequence-consuming units in front of its unit, and 1 if the unit is = or X, 0 if it is D"""
    s, k, sacc = [], [], 0
    for op, n in ws:
        if op == OP_I:
            sacc += n
        elif op == OP_D:
            s += [sacc] * n
            k += [0] * n
        else:
            s += list(range(sacc, sacc + n))
            k += [1] * n
            sacc += n
    return s, k


def banded_dp(q, t, margin, x, g, banded=True):
    """the DP of the header on the codes q (n) against the bases t (m): rows over all jt with the cells outside the 64 diagonals unreachable ->
    (the cost at (n, m), the steps from (0, 0) to (n, m) as a list of M / I / D, does the path touch an edge diagonal)"""
    n, m = len(q), len(t)
    q, t = np.asarray(q, dtype=np.int64) & 3, np.asarray(t, dtype=np.int64) & 3
    dlo = min(0, m - n) - margin
    jt = np.arange(m + 1, dtype=np.int64)
    H = np.full((n + 1, m + 1), INF, dtype=np.int64)
    for i in range(n + 1):
        inside = ((jt - i >= dlo) & (jt - i <= dlo + BAND - 1)) if banded else np.ones(m + 1, dtype=bool)
        if i == 0:
            c = np.full(m + 1, INF, dtype=np.int64)
            c[0] = 0
        else:
            c = H[i - 1] + g                                    # the query step
            c[1:] = np.minimum(c[1:], H[i - 1][:-1] + np.where(t == q[i - 1], 0, x))
        c = np.where(inside, c, INF)
        row = np.minimum.accumulate(c - jt * g) + jt * g        # the target steps inside the row
        H[i] = np.where(inside, np.minimum(row, INF), INF)
    assert H[n][m] < INF
    steps, edge, i, j = [], False, n, m
    while True:
        edge |= banded and (j - i == dlo or j - i == dlo + BAND - 1)
        if i == 0 and j == 0:
            break
        v = int(H[i][j])
        if i and j and int(H[i - 1][j - 1]) + (0 if q[i - 1] == t[j - 1] else x) == v:
            steps.append(OP_M)
            i, j = i - 1, j - 1
        elif j and int(H[i][j - 1]) + g == v:
            steps.append(OP_D)
            j -= 1
        else:
            assert i and int(H[i - 1][j]) + g == v
            steps.append(OP_I)
            i -= 1
    return int(H[n][m]), steps[::-1], bool(edge)


def runs(steps):
    out = []
    for op in steps:
        if out and out[-1][1] == op:
            out[-1][0] += 1
        else:
            out.append([1, op])
    return W_(*[(n, op) for n, op in out])


class Ref:
    """what a run must leave: piece2, pstatus, cost, pcig2_off, doff2, dlen2; pcig2 (pcig2_cap words, FILL32 where no piece wrote); and per piece its
    words, with (u, v, m, margin) of every piece that reached the DP"""


def window_realign_ref(b, p, pcig2_cap):
    P, nwin = b.piece_cap, b.nwin
    r = Ref()
    r.piece2 = b.piece[:P].copy()
    r.piece2["len"] = 0
    r.pstatus = np.full(P, ST_NO_WINDOW, dtype=np.uint32)
    r.cost = np.zeros(P, dtype=np.uint32)
    r.doff2, r.dlen2 = np.zeros(nwin, dtype=np.uint64), np.zeros(nwin, dtype=np.uint32)
    r.words = [np.zeros(0, np.uint32) for _ in range(P)]
    r.span = {}
    for g in range(nwin):
        x0, x1 = int(b.piece_off[g]), int(b.piece_off[g + 1])
        mine = range(x0, x1) if x0 <= x1 <= P else range(0)
        lw = liftable(b, g, p["window2"])
        if lw is None:
            continue                                           # its pieces keep NO_WINDOW
        slen, Ld, ws = lw
        r.doff2[g], r.dlen2[g] = int(b.seq_off[g]), slen
        s, k = lift_tables(ws)
        for j in mine:
            pc = b.piece[j]
            n, tf, tl, bo = int(pc["len"]), int(pc["t_first"]), int(pc["t_last"]), int(pc["base_off"])
            a = tf % b.window
            bb = a + (tl - tf)
            if n < 1:
                st = ST_BAD_PIECE
            elif n > p["max_len"]:
                st = ST_TOO_LONG
            elif bo + n > b.bases_cap or tl < tf or bb >= Ld:
                st = ST_BAD_PIECE
            else:
                u, v = s[a], s[bb] + k[bb] - 1
                m = v - u + 1
                margin = (63 - abs(m - n)) // 2
                st = ST_EMPTY_SPAN if m < 1 else ST_OFF_BAND if (abs(m - n) > 63 or margin < p["min_margin"]) else ST_OK
            r.pstatus[j] = st
            if st != ST_OK:
                continue
            r.span[j] = (u, v, m, margin)
            o = int(b.seq_off[g])
            cost, steps, edge = banded_dp(b.bases[bo:bo + n], b.seq[o + u:o + v + 1], margin, p["x"], p["g"])
            r.cost[j] = cost
            dg = [i for i, op in enumerate(steps) if op == OP_M]
            if not dg:
                r.pstatus[j] = ST_NO_DIAG
                continue
            lead, trail = steps[:dg[0]], steps[dg[-1] + 1:]
            li, ld, ti, td = lead.count(OP_I), lead.count(OP_D), trail.count(OP_I), trail.count(OP_D)
            r.words[j] = runs(steps[dg[0]:dg[-1] + 1])
            r.pstatus[j] = ST_EDGE if edge else ST_OK
            r.piece2[j] = (int(pc["pair"]), (int(pc["q_first"]) + li) & 0xFFFFFFFF, n - li - ti, u + ld, v - td, 0, bo + li)
    r.pcig2_off = np.zeros(P + 1, dtype=np.uint64)
    r.pcig2_off[1:] = np.cumsum([len(w) for w in r.words], dtype=np.uint64)
    r.pcig2 = np.full(pcig2_cap, FILL32, dtype=np.uint32)
    for j in range(P):
        if len(r.words[j]) and int(r.pcig2_off[j + 1]) <= pcig2_cap:
            r.pcig2[int(r.pcig2_off[j]):int(r.pcig2_off[j + 1])] = r.words[j]
    return r


def round2_batch(b, r, window2):
    """what bsa_window_msa_* takes for round 2: the records and guides of the reference, the round-1 sequence as the draft"""
    need = int(r.pcig2_off[-1])
    pcig = np.concatenate([np.zeros(0, np.uint32)] + r.words)
    assert len(pcig) == need
    return W.Batch(r.piece2, b.piece_off, b.bases, pcig, r.pcig2_off, np.concatenate([b.seq, np.zeros(8, np.uint8)]), r.doff2, r.dlen2, window2,
                   piece_cap=b.piece_cap, bases_cap=b.bases_cap)


def check_piece(b, r, j, mb, g):
    """the invariants of a re-aligned piece j of window g; mb: round2_batch"""
    ws, pc = r.words[j], r.piece2[j]
    assert int(r.pstatus[j]) & 0xFF == ST_OK and len(ws) >= 1
    assert int(ws[0]) & 15 == OP_M and int(ws[-1]) & 15 == OP_M and all(int(w) & 15 in (OP_M, OP_I, OP_D) and int(w) >> 4 >= 1 for w in ws)
    assert all(int(ws[i]) & 15 != int(ws[i + 1]) & 15 for i in range(len(ws) - 1))
    assert sum(int(w) >> 4 for w in ws if int(w) & 15 != OP_D) == int(pc["len"])
    assert sum(int(w) >> 4 for w in ws if int(w) & 15 != OP_I) == int(pc["t_last"]) - int(pc["t_first"]) + 1
    assert int(pc["reserved"]) == 0 and int(pc["pair"]) == int(b.piece[j]["pair"])
    assert W.live_guide(mb, j, min(int(mb.dlen[g]), mb.window)) is not None, "a re-aligned piece that the MSA pass would not take"


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------
def make(windows, window, t_base=0):
    """windows: a list of (seq codes, words, [(a, b, codes)]) -- a piece on the draft columns a .. b of its window -> RBatch.  t_first is
    (t_base + g) * window + a, as a chain numbers them"""
    piece, poff, bases, seq, soff, cig, coff = [], [0], [], [], [], [], []
    for g, (sq, ws, ps) in enumerate(windows):
        soff.append(len(seq))
        coff.append(len(cig))
        seq += [int(x) for x in sq]
        cig += [int(x) for x in ws]
        for a, bb, code in ps:
            tf = ((t_base + g) * window + a) & 0xFFFFFFFF
            piece.append((len(piece), 50 + 7 * len(piece), len(code), tf, tf + (bb - a), 0, len(bases)))
            bases += [int(x) for x in code]
        poff.append(len(piece))
    soff.append(len(seq))
    coff.append(len(cig))
    return RBatch(np.array(piece, dtype=PIECE_DTYPE) if piece else np.zeros(0, PIECE_DTYPE), poff, bases, window, seq, soff, cig, coff)


def seq_words(rng, Ld, rate=0.08):
    """a window of Ld draft columns: its draft, the sequence called on it and the = / X / I / D words between them (maximal runs, never I beside I)"""
    draft = rng.integers(0, 4, Ld).astype(np.uint8)
    seq, units = [], []
    for j in range(Ld):
        r = rng.random()
        if r < rate / 2 and j:
            k = int(rng.integers(1, 3))
            seq += [int(v) for v in rng.integers(0, 4, k)]
            units += [OP_I] * k
        r = rng.random()
        if r < rate / 2:
            units.append(OP_D)
        elif r < rate:
            seq.append((int(draft[j]) + 1 + int(rng.integers(3))) & 3)
            units.append(OP_X)
        else:
            seq.append(int(draft[j]))
            units.append(OP_EQ)
    return draft, np.array(seq, dtype=np.uint8), runs(units)


def mutate(rng, s, sub, ins, dele):
    out = []
    for c in s:
        if rng.random() < ins:
            out.append(int(rng.integers(4)))
        r = rng.random()
        if r < dele:
            continue
        out.append((int(c) + 1 + int(rng.integers(3))) & 3 if r < dele + sub else int(c))
    if not out:
        out = [int(rng.integers(4))]
    return np.array(out, dtype=np.uint8)


def span_of(ws, a, bb):
    s, k = lift_tables([(int(w) & 15, int(w) >> 4) for w in ws])
    return s[a], s[bb] + k[bb] - 1


def simulated_window(rng, Ld, depth, sub=0.04, ins=0.03, dele=0.03, whole=False, codes_above_3=False):
    """a window whose pieces are reads of the called sequence over random column ranges (whole: all of them over the whole window)"""
    draft, seq, ws = seq_words(rng, Ld)
    ps = []
    for _ in range(depth):
        a, bb = (0, Ld - 1) if whole or rng.integers(3) == 0 else sorted(int(v) for v in rng.integers(0, Ld, 2))
        u, v = span_of(ws, a, bb)
        code = mutate(rng, seq[u:v + 1], sub, ins, dele) if v >= u else rng.integers(0, 4, 3).astype(np.uint8)
        if codes_above_3:
            code = code | (rng.integers(0, 64, len(code)).astype(np.uint8) << 2)
        ps.append((a, bb, code))
    return seq, ws, ps


# ---- the header's examples, typed in byte by byte ------------------------------------------------------------------------------------------------
def header_example_1():
    """the stitch block's example 2: seq 0 1 2 3 2 0 1 2 3 0 1, words 4= 1I 6=, window 10; a piece on the columns 2 .. 7 with the codes 2 3 2 0 2 3
    (the sequence's 2 3 2 0 1 2 3 without its 1), x = g = 1, min_margin 8 -> (RBatch, par, what the call leaves)"""
    seq = [0, 1, 2, 3, 2, 0, 1, 2, 3, 0, 1]
    b = RBatch(np.array([(9, 100, 6, 32, 37, 0, 0)], dtype=PIECE_DTYPE), [0, 1], [2, 3, 2, 0, 2, 3], 10, seq, [0, 11], W_((4, OP_EQ), (1, OP_I), (6, OP_EQ)), [0, 3])
    want = dict(u=2, v=8, m=7, margin=31, cost=1, words=W_((4, OP_M), (1, OP_D), (2, OP_M)).tolist(), piece2=(9, 100, 6, 2, 8, 0, 0), status=ST_OK, doff2=0, dlen2=11)
    return b, par(16, 64, 8, 1, 1), want


def header_example_2():
    """a and b on D units: draft of 8 columns, words 2= 2D 3= 1D, seq 0 1 2 3 0 (slen 5); a piece on the columns 2 .. 7 (a = 2 and b = 7 are
    deleted columns): u = s(2) = 2, v = s(7) + 0 - 1 = 4, T = 2 3 0; codes 1 2 3 0 2: the leading 1 and the trailing 2 are I steps that are cut"""
    b = RBatch(np.array([(3, 10, 5, 2, 7, 0, 0)], dtype=PIECE_DTYPE), [0, 1], [1, 2, 3, 0, 2], 8, [0, 1, 2, 3, 0], [0, 5],
               W_((2, OP_EQ), (2, OP_D), (3, OP_EQ), (1, OP_D)), [0, 4])
    want = dict(u=2, v=4, m=3, margin=30, cost=2, words=W_((3, OP_M)).tolist(), piece2=(3, 11, 3, 2, 4, 0, 1), status=ST_OK, doff2=0, dlen2=5)
    return b, par(8, 64, 8, 1, 1), want


# ---- hand-made spans and paths ---------------------------------------------------------------------------------------------------------------------
def _plain(L):
    """a window whose sequence is its draft: L columns, one = word"""
    return W_((L, OP_EQ))


def shapes_batch():
    """(RBatch, par): n and m in {1, 2, 63, 64, 65}, |m - n| in {0, 1, 62, 63, 64} both ways, paths that begin and end with I and with D runs, an
    all-gap middle, codes above 3, paths along each edge diagonal; window 256, max_len 200, min_margin 0"""
    rng = np.random.default_rng(4711)
    L = 200
    seq = rng.integers(0, 4, L).astype(np.uint8)
    ps = []
    for n in (1, 2, 63, 64, 65):
        for m in (1, 2, 63, 64, 65):
            a = int(rng.integers(0, L - m))
            code = mutate(rng, seq[a:a + m], 0.05, 0.0, 0.0)
            code = np.resize(code, n) if n <= m else np.concatenate([code, rng.integers(0, 4, n - m).astype(np.uint8)])
            ps.append((a, a + m - 1, code))
    for d in (0, 1, 62, 63, 64):
        for n, m in ((70, 70 + d), (70 + d, 70)):
            a = int(rng.integers(0, L - m))
            # the shorter one is a subsequence of the longer: the path runs along an edge diagonal where d is 62 or 63
            if m >= n:
                code = np.concatenate([seq[a:a + 20], seq[a + 20 + d:a + m]])
            else:
                code = np.concatenate([seq[a:a + 20], rng.integers(0, 4, d).astype(np.uint8), seq[a + 20:a + m]])
            ps.append((a, a + m - 1, code))
    t = seq[40:100]
    other = lambda c: (np.asarray(c, dtype=np.uint8) + 2) & 3
    ps.append((40, 99, np.concatenate([other(t[:5]), t[8:]])))            # begins with gaps: the first bases fit nowhere
    ps.append((40, 99, np.concatenate([t[:50], other(t[50:52])])))       # ends with gaps
    ps.append((40, 99, np.concatenate([rng.integers(0, 4, 7).astype(np.uint8), t, rng.integers(0, 4, 4).astype(np.uint8)])))      # I runs at both ends
    ps.append((40, 99, t[9:52]))                                          # D runs at both ends
    ps.append((40, 99, np.concatenate([t[:20], t[50:]])))                 # an all-gap middle: 30 D
    ps.append((40, 99, np.concatenate([t[:20], other(t[20:30]), t[30:]])))
    ps.append((40, 99, t | np.uint8(0xFC)))                               # codes above 3
    ps.append((40, 99, (t & 3) | (rng.integers(0, 64, 60).astype(np.uint8) << 2)))
    return make([(seq, _plain(L), ps)], 256), par(256, 200, 0, 1, 1)


def scoring_batches():
    """name -> (RBatch, par): x = 3, g = 1 on a one-base mismatch (two gaps are cheaper than the mismatch: no diagonal step), x = 1, g = 255, and
    every min_margin on the same pieces"""
    rng = np.random.default_rng(12)
    seq = rng.integers(0, 4, 120).astype(np.uint8)
    out = {}
    one = [(5, 5, [(int(seq[5]) + 1) & 3]), (5, 5, [int(seq[5])]), (7, 9, [int(seq[7]), (int(seq[8]) + 2) & 3, int(seq[9])])]
    out["x3_g1"] = (make([(seq, _plain(120), one)], 128), par(128, 64, 8, 3, 1))
    ps = [(10, 99, mutate(rng, seq[10:100], 0.05, 0.03, 0.03)) for _ in range(6)] + one
    out["x1_g255"] = (make([(seq, _plain(120), ps)], 128), par(128, 128, 8, 1, 255))
    out["x255_g1"] = (make([(seq, _plain(120), ps)], 128), par(128, 128, 8, 255, 1))
    wide = ps + [(10, 10 + 59 + d, mutate(rng, seq[10:70], 0.03, 0.0, 0.0)) for d in (0, 1, 15, 16, 17, 45, 46, 47, 48, 60)]      # |m - n| around 63 - 2 * 8 and 63 - 2 * 31 ..
    for mm in (0, 8, 31):
        out["min_margin_%d" % mm] = (make([(seq, _plain(120), wide)], 128), par(128, 128, mm, 1, 1))
    return out


def max_len_batch(max_len):
    """pieces of max_len - 1, max_len and max_len + 1 codes on one window"""
    rng = np.random.default_rng(max_len)
    L = max_len + 40
    seq = rng.integers(0, 4, L).astype(np.uint8)
    ps = [(3, 3 + n - 1, mutate(rng, seq[3:3 + n], 0.04, 0.0, 0.0)) for n in (max_len - 1, max_len, max_len + 1)]
    if max_len >= 1000:
        t = seq[3:3 + max_len + 20]
        keep = np.ones(len(t), dtype=bool)
        keep[rng.choice(len(t), 20, replace=False)] = False
        ps.append((3, 3 + len(t) - 1, t[keep]))                 # max_len codes with 20 deletions spread over the span
    return make([(seq, _plain(L), ps)], L), par(min(L, MAX_WINDOW2), max_len, 8, 1, 1)


WORD_COUNTS = (1, 63, 64, 65, 200)


def window_with_words(rng, nwords):
    """a window of exactly nwords words, kinds cycling = I = D = X .., with three pieces: the whole window, I units directly in front of a, and a
    and b on D units where the window has any"""
    kinds = [OP_EQ, OP_I, OP_EQ, OP_D, OP_EQ, OP_X]
    ops = [kinds[i % 6] for i in range(nwords)]
    lens = [int(rng.integers(1, 4)) for _ in range(nwords)]
    units = [op for op, n in zip(ops, lens) for _ in range(n)]
    seq = rng.integers(0, 4, sum(1 for u in units if u != OP_D)).astype(np.uint8)
    ws = W_(*[(n, op) for n, op in zip(lens, ops)])
    Ld = sum(1 for u in units if u != OP_I)
    s, k = lift_tables([(int(w) & 15, int(w) >> 4) for w in ws])
    cols = []                                                   # for every draft column: its unit's kind, and is an I unit directly in front of it
    prev = None
    for u in units:
        if u != OP_I:
            cols.append((u, prev == OP_I))
        prev = u
    ps = []

    def add(a, bb):
        u, v = s[a], s[bb] + k[bb] - 1
        ps.append((a, bb, mutate(rng, seq[u:v + 1], 0.05, 0.02, 0.02) if v >= u else np.array([1, 2], dtype=np.uint8)))
    add(0, Ld - 1)
    after_i = [j for j, (_, ins) in enumerate(cols) if ins]
    on_d = [j for j, (u, _) in enumerate(cols) if u == OP_D]
    if after_i:
        add(after_i[0], Ld - 1)
        add(after_i[len(after_i) // 2], after_i[-1])
    if on_d:
        add(on_d[0], on_d[-1])
        add(on_d[0], on_d[0])                                   # a span of one deleted column: m = 0
    return seq, ws, ps


def words_batch():
    rng = np.random.default_rng(909)
    wins = [window_with_words(rng, nw) for nw in WORD_COUNTS]
    wins.insert(2, (rng.integers(0, 4, 90).astype(np.uint8), _plain(90), [(0, 89, rng.integers(0, 4, 90).astype(np.uint8)), (4, 60, rng.integers(0, 4, 50).astype(np.uint8))]))
    return make(wins, 1024), par(1024, 1024, 8, 1, 1)


DEPTHS = (0, 1, 64, 65, 300)


def depths_batch():
    """windows of 0, 1, 64, 65 and 300 pieces, short ones: window 40"""
    rng = np.random.default_rng(300)
    return make([simulated_window(rng, 40, d, codes_above_3=(d == 65)) for d in DEPTHS], 40, t_base=5), par(64, 64, 8, 1, 1)


def bad_windows_batch():
    """liftable windows alternating with one window for every way the test fails -> (RBatch, par, names, name -> window).  Every window has two
    pieces; seq and cig end exactly at their caps."""
    rng = np.random.default_rng(77)
    names = ["slen_above_window2", "op_M", "op_15", "length_0", "seq_units_short", "seq_units_long", "Ld_above_window", "huge_D_word", "huge_I_word", "no_words"]
    wins = []
    for name in names:
        wins.append(simulated_window(rng, 30, 2))
        if name == "slen_above_window2":                        # 30 columns, 41 bases
            sq = rng.integers(0, 4, 41).astype(np.uint8)
            wins.append((sq, W_((10, OP_EQ), (11, OP_I), (20, OP_EQ)), [(0, 29, sq[:30]), (3, 8, sq[3:9])]))
        elif name == "Ld_above_window":
            wins.append(simulated_window(rng, 33, 2, whole=True))
        else:
            wins.append(simulated_window(rng, 30, 2))
    wins.append(simulated_window(rng, 30, 2))
    b = make(wins, 32)
    at = {name: 2 * i + 1 for i, name in enumerate(names)}
    first = lambda g: int(b.cig_off[g])
    g = at["op_M"]; b.cig[first(g)] = (int(b.cig[first(g)]) & ~15) | OP_M
    g = at["op_15"]; b.cig[first(g) + 1] |= 15
    g = at["length_0"]; b.cig[int(b.cig_off[g + 1]) - 1] &= 15
    g = at["seq_units_short"]
    i = next(i for i in range(first(g), int(b.cig_off[g + 1])) if int(b.cig[i]) & 15 == OP_EQ)
    b.cig[i] = (int(b.cig[i]) & ~15) | OP_D                    # an = word becomes a D word: the same columns, fewer bases
    g = at["seq_units_long"]; b.cig[first(g)] += 16
    g = at["huge_D_word"]; b.cig[first(g) + 1] = (0xFFFFFFF << 4) | OP_D
    g = at["huge_I_word"]; b.cig[first(g) + 1] = (0xFFFFFFF << 4) | OP_I
    g = at["no_words"]; b.cig_off[g + 1] = b.cig_off[g]        # (the next window's range then begins with this one's words: it is not liftable either)
    return b, par(40, 64, 8, 1, 1), names, at


def bad_offsets_batches():
    """name -> RBatch: offsets that decrease and ranges behind a cap, four windows each (the neighbour that shares the broken offset fails with it)"""
    out = {}
    for name in ("seq_off_decreases", "seq_behind_seq_cap", "cig_off_decreases", "cig_behind_cig_cap"):
        rng = np.random.default_rng(33)
        b = make([simulated_window(rng, 30, 2) for _ in range(4)], 32)
        if name == "seq_off_decreases":
            b.seq_off[2] = b.seq_off[1] - np.uint64(1)
        elif name == "seq_behind_seq_cap":
            b.seq_cap = len(b.seq) - 1
        elif name == "cig_off_decreases":
            b.cig_off[2] = b.cig_off[1] - np.uint64(1)
        else:
            b.cig_cap = len(b.cig) - 1
        out[name] = b
    return out, par(40, 64, 8, 1, 1)


def bad_pieces_batch():
    """one liftable window (32 columns, words with I and D) whose pieces violate the clauses one at a time, each between two good pieces ->
    (RBatch, par, name -> (piece, the status it must get))"""
    rng = np.random.default_rng(5)
    Ld, w, tb = 100, 100, 3
    seq, ws, _ = simulated_window(rng, Ld, 0)
    s, k = lift_tables([(int(x) & 15, int(x) >> 4) for x in ws])
    dcols = [j for j in range(2, Ld) if k[j] == 0 and k[j - 1] == 1]
    assert dcols, "the window needs a deleted column"
    good = lambda: (2, 89, mutate(rng, seq[s[2]:s[89] + k[89]], 0.03, 0.02, 0.02))
    names = ["len_0", "len_above_max_len", "codes_behind_bases_cap", "t_last_below_t_first", "b_at_Ld", "empty_span", "off_band_long", "off_band_short", "margin_below_min"]
    ps = []
    for name in names:
        ps += [good(), good()]
    ps.append(good())
    b = make([(seq, ws, ps)], w, t_base=tb)
    at = {name: 2 * i + 1 for i, name in enumerate(names)}
    pc = b.piece

    def codes(j, n):
        """piece j gets n fresh codes at the end of the bases"""
        pc[j]["base_off"], pc[j]["len"] = len(b.bases), n
        b.bases = np.concatenate([b.bases, rng.integers(0, 4, n).astype(np.uint8)])
        b.bases_cap = len(b.bases)

    def span(j, a, bb):
        pc[j]["t_first"], pc[j]["t_last"] = tb * w + a, tb * w + bb
    j = at["len_0"]; pc[j]["len"] = 0
    codes(at["len_above_max_len"], 101)
    j = at["t_last_below_t_first"]; pc[j]["t_last"] = int(pc[j]["t_first"]) - 1
    span(at["b_at_Ld"], 2, Ld)
    span(at["empty_span"], dcols[0], dcols[0])
    j = at["off_band_long"]; span(j, 2, 3); codes(j, 70)
    j = at["off_band_short"]; span(j, 0, Ld - 1); codes(j, 1)
    j = at["margin_below_min"]; span(j, 2, 3); codes(j, 44)    # |m - n| about 42: a margin of 10, below min_margin 12
    j = at["codes_behind_bases_cap"]; pc[j]["base_off"] = len(b.bases) - int(pc[j]["len"]) + 1
    want = dict(len_0=ST_BAD_PIECE, len_above_max_len=ST_TOO_LONG, codes_behind_bases_cap=ST_BAD_PIECE, t_last_below_t_first=ST_BAD_PIECE, b_at_Ld=ST_BAD_PIECE,
                empty_span=ST_EMPTY_SPAN, off_band_long=ST_OFF_BAND, off_band_short=ST_OFF_BAND, margin_below_min=ST_OFF_BAND)
    return b, par(128, 100, 12, 1, 1), at, want


def piece_off_batches():
    """piece_off entries above piece_cap, and indices below piece_cap that no window claims"""
    rng = np.random.default_rng(41)
    out = {}
    b = make([simulated_window(rng, 30, 2), simulated_window(rng, 30, 3), simulated_window(rng, 30, 2)], 32)
    b.piece_off[:] = [0, 2, 9, 9]                               # window 1 ends above piece_cap = 7: it has no pieces; window 2 starts above it
    out["above_piece_cap"] = b
    b = make([simulated_window(rng, 30, 2), simulated_window(rng, 30, 3), simulated_window(rng, 30, 2)], 32)
    b.piece_off[:] = [1, 2, 4, 6]                               # pieces 0 and 6 are in no window; window 1 holds pieces 2, 3 (one of them another window's)
    out["unclaimed"] = b
    return out, par(40, 64, 8, 1, 1)


def arena_batch():
    """the capacities test's batch: four windows, 12 pieces, dead ones among them"""
    rng = np.random.default_rng(2121)
    b = make([simulated_window(rng, 40, 4, 0.06, 0.05, 0.05), simulated_window(rng, 40, 0), simulated_window(rng, 25, 5, 0.06, 0.05, 0.05),
              simulated_window(rng, 40, 3, 0.06, 0.05, 0.05)], 40)
    b.piece[5]["len"] = 0
    return b, par(64, 64, 8, 1, 1)


def draft_window_batch():
    """a BSA_STITCH_ST_DRAFT window -- its draft row, one = word -- between two called ones"""
    rng = np.random.default_rng(8)
    d = rng.integers(0, 4, 50).astype(np.uint8)
    mid = (d, _plain(50), [(0, 49, mutate(rng, d, 0.04, 0.03, 0.03)), (10, 30, mutate(rng, d[10:31], 0.04, 0.03, 0.03))])
    return make([simulated_window(rng, 50, 3), mid, simulated_window(rng, 50, 3)], 50), par(64, 128, 8, 1, 1)


# ---- the closed loop of window_msa_cases, continued --------------------------------------------------------------------------------------------------
def stitched(b, vote=0, min_cov=1, max_rows=None):
    """a window_msa_cases.Batch through window_msa_ref, the HOST consensus caller and window_stitch_ref -> (the stitch's Ref, the cwin records)"""
    import window_cns_cases as WC
    import window_stitch_cases as WS
    off, cwin, cols = W.window_msa_ref(b, vote)
    out_cap = int(cwin["mlen"].sum())
    cns = WC.window_cns_ref(cols, cwin, len(cols), out_cap, out_cap, int(cwin["nseq"].max()) if max_rows is None else max_rows, W.PAR7)
    assert np.all(cns.status == 0)
    return WS.window_stitch_ref(cns.cols, cwin, len(cols), cns.status, min_cov, out_cap, out_cap), cwin


def from_round1(b, st):
    """the RBatch of a round-1 Batch and its stitch"""
    ns, nc = int(st.seq_off[-1]), int(st.cig_off[-1])
    return RBatch(b.piece, b.piece_off, b.bases, b.window, st.seq[:ns], st.seq_off, st.cig[:nc], st.cig_off, piece_cap=b.piece_cap, bases_cap=b.bases_cap)


def homopolymer_window():
    """the draft lacks one A of a run of six; five reads carry it, and their round-1 alignments place the inserted base at five different places of
    the run (in front of the draft's run columns 1 .. 5) -> the round-1 Batch (window 32, one window).  The reads are error-free copies of the truth."""
    left, right = [1, 2, 3, 1, 2, 1, 3, 2], [2, 1, 3, 2, 3, 1, 2, 1, 3, 2]
    draft = left + [0] * 5 + right
    truth = left + [0] * 6 + right
    ps = []
    for r in range(5):
        at = len(left) + 1 + r if r < 4 else len(left) + 5       # the column the inserted base stands in front of
        ps.append((0, W_((at, OP_M), (1, OP_I), (len(draft) - at, OP_M)), truth))
    return W.make([(draft, None, ps)], 32), np.array(truth, dtype=np.uint8), np.array(draft, dtype=np.uint8)
