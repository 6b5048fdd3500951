"""bsa_window_pieces_* (include/bsalign_hip.h): the definition, record by record in Python and numpy (pieces_ref), and hand-made reads and window
records -- the smallest shapes at which the pass can go wrong.  A hand-made case is written once as reads, marks and records (Case) and built for
each of the four flag combinations (build): the same reads as a 1 B/base blob or as 2-bit packed words, with or without the strand bit."""
import numpy as np

NONE = 0xFFFFFFFF
SEQ2BIT, QSTRAND = 0x800, 0x2000
REVCOMP = 1 << 63
ALL_FLAGS = (0, QSTRAND, SEQ2BIT, SEQ2BIT | QSTRAND)
PIECE_DTYPE = np.dtype([("pair", np.uint32), ("q_first", np.uint32), ("len", np.uint32), ("t_first", np.uint32), ("t_last", np.uint32), ("reserved", np.uint32),
                        ("base_off", np.uint64)])


def _stored(seqs, off, j, packed):
    """base j of the stored query at `off`: a byte of the blob, or two bits of the words (base i at bits 62 - 2 (i % 32) of word i / 32)"""
    i = off + j
    if packed:
        return (int(seqs[i >> 5]) >> (62 - 2 * (i & 31))) & 3
    return int(seqs[i])


def pieces_ref(seqs, qoff, qlen, win, win_off, window, gbase, nwin, flags):
    """the definition -> (piece_off, base_off, records as a PIECE_DTYPE array, bytes as uint8)"""
    packed, strands = bool(flags & SEQ2BIT), bool(flags & QSTRAND)
    per = [[] for _ in range(nwin)]
    for k in range(len(qlen)):
        for i in range(int(win_off[k]), int(win_off[k + 1])):
            tf, qf, tl, ql = (int(x) for x in win[i])
            if tf == NONE or tf > tl or qf > ql or ql >= int(qlen[k]):
                continue
            g = int(gbase[k]) + tf // window
            if g < nwin:
                per[g].append((i, k, qf, ql - qf + 1, tf, tl))
    piece_off, base_off = np.zeros(nwin + 1, dtype=np.uint64), np.zeros(nwin + 1, dtype=np.uint64)
    recs, codes = [], []
    for g in range(nwin):
        for i, k, qf, ln, tf, tl in sorted(per[g]):
            recs.append((k, qf, ln, tf, tl, 0, len(codes)))
            qo, n = int(qoff[k]), int(qlen[k])
            rev = strands and bool(qo & REVCOMP)
            if strands:
                qo &= ~REVCOMP
            for j in range(qf, qf + ln):
                codes.append(((_stored(seqs, qo, n - 1 - j, packed) & 3) ^ 3) if rev else (_stored(seqs, qo, j, packed) & 3))
        piece_off[g + 1], base_off[g + 1] = len(recs), len(codes)
    return piece_off, base_off, np.array(recs, dtype=PIECE_DTYPE), np.array(codes, dtype=np.uint8)


def header_example():
    """the worked example of include/bsalign_hip.h, typed in by hand: (arguments of pieces_ref, piece_off, base_off, records, bytes)"""
    seqs = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 0, 0, 1, 1, 2, 2, 3], dtype=np.uint8)          # ACGTACGTAC AACCGGT
    qoff = np.array([0, 10 | REVCOMP], dtype=np.uint64)
    qlen = np.array([10, 7], dtype=np.uint32)
    win = np.array([[1, 0, 3, 2], [4, 3, 7, 6], [8, 7, 10, 9], [5, 0, 7, 2], [8, 3, 11, 6]], dtype=np.uint32)
    win_off = np.array([0, 3, 5], dtype=np.uint64)
    args = (seqs, qoff, qlen, win, win_off, 4, np.array([0, 0], dtype=np.uint64), 3, QSTRAND)
    recs = np.array([(0, 0, 3, 1, 3, 0, 0), (0, 3, 4, 4, 7, 0, 3), (1, 0, 3, 5, 7, 0, 7), (0, 7, 3, 8, 10, 0, 10), (1, 3, 4, 8, 11, 0, 13)], dtype=PIECE_DTYPE)
    codes = np.array([0, 1, 2, 3, 0, 1, 2, 0, 1, 1, 3, 0, 1, 2, 2, 3, 3], dtype=np.uint8)
    return args, np.array([0, 1, 3, 5], dtype=np.uint64), np.array([0, 3, 10, 17], dtype=np.uint64), recs, codes


class Case:
    """reads: the stored queries (uint8 codes); marks: a bool a pair (the pair aligns the reverse complement); gaps: bases of filler in front of
    each read in the blob; recs: per pair a list of (t_first, q_first, t_last, q_last); raw: the reads hold codes above 3 (1 B/base only)"""

    def __init__(self, reads, marks, recs, window, gbase, nwin, gaps=None, raw=False):
        self.reads = [np.asarray(r, dtype=np.uint8) for r in reads]
        self.marks, self.recs, self.window, self.nwin, self.raw = list(marks), recs, window, nwin, raw
        self.gbase = np.array(gbase, dtype=np.uint64)
        self.gaps = list(gaps) if gaps is not None else [(3 * k + 1) % 7 for k in range(len(reads))]
        assert len(self.marks) == len(self.reads) == len(self.recs) == len(self.gbase) == len(self.gaps)

    def flag_sets(self):
        return (0, QSTRAND) if self.raw else ALL_FLAGS


def _pack2bit(codes):
    nw = (len(codes) + 31) // 32
    buf = np.zeros(nw * 32, dtype=np.uint64)
    buf[:len(codes)] = codes
    return np.bitwise_or.reduce(buf.reshape(nw, 32) << (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)), axis=1).astype(np.uint64) if nw else np.zeros(0, np.uint64)


def build(case, flags):
    """-> (seqs, qoff, qlen, win, win_off, window, gbase, nwin, flags): the arguments of pieces_ref and of the two calls.  The filler between the
    reads is not zero, so that a base read from outside a read shows; the last read ends the blob."""
    parts, qoff, acc = [], [], 0
    for k, r in enumerate(case.reads):
        fill = (np.arange(case.gaps[k]) + k) % 4 if not case.raw else np.full(case.gaps[k], 0xEE)
        parts += [fill.astype(np.uint8), r]
        acc += case.gaps[k]
        qoff.append(acc | (REVCOMP if (flags & QSTRAND) and case.marks[k] else 0))
        acc += len(r)
    blob = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    seqs = _pack2bit(blob) if flags & SEQ2BIT else blob
    win = np.array([x for rs in case.recs for x in rs], dtype=np.uint32).reshape(-1, 4)
    win_off = np.zeros(len(case.reads) + 1, dtype=np.uint64)
    win_off[1:] = np.cumsum([len(rs) for rs in case.recs], dtype=np.uint64)
    return (seqs, np.array(qoff, dtype=np.uint64), np.array([len(r) for r in case.reads], dtype=np.uint32), win, win_off, case.window, case.gbase, case.nwin, flags)


def _reads(rng, lens, raw=False):
    return [rng.integers(0, 256 if raw else 4, int(n)).astype(np.uint8) for n in lens]


LENGTHS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000)
DEPTHS = (0, 1, 2, 63, 64, 65, 129, 200)
MANY_NWIN = 16400
MANY_WINDOWS = (0, 4095, 4096, 4097, 8191, 8192, 12288, 16383, 16384, 16399)


def hand_cases():
    rng = np.random.default_rng(7)
    c = {}
    # windows holding 0, 1, 2, 63, 64, 65, 129 and 200 pieces: a pair a piece, pieces of 1 .. 24 bases
    reads, marks, recs = [], [], []
    for g, d in enumerate(DEPTHS):
        for j in range(d):
            n = int(rng.integers(1, 40))
            a = int(rng.integers(0, n))
            b = int(rng.integers(a, min(n, a + 24)))
            reads.append(rng.integers(0, 4, n)); marks.append(bool(j % 3 == 1)); recs.append([(10 * g + j % 10, a, 10 * g + 9, b)])
    order = rng.permutation(len(reads))                                             # the pairs of a window are spread over the batch
    c["depths"] = Case([reads[i] for i in order], [marks[i] for i in order], [recs[i] for i in order], 10, [0] * len(reads), len(DEPTHS))
    # one window of 5000 pieces of 1 .. 3 bases: 500 pairs with ten records each, in the middle of three windows
    reads = _reads(rng, rng.integers(3, 30, 500))
    recs = []
    for r in reads:
        rs = []
        for j in range(10):
            a = int(rng.integers(0, len(r)))
            rs.append((100 + j, a, 150, min(len(r) - 1, a + int(rng.integers(0, 3)))))
        recs.append(rs)
    c["deep_5000"] = Case(reads, [k % 2 == 1 for k in range(500)], recs, 100, [0] * 500, 3)
    # every length at every residue of base_off modulo 16: a piece of L, then a filler that moves the next start on by one byte
    reads = _reads(rng, [1100] * len(LENGTHS))
    recs = []
    for k, L in enumerate(LENGTHS):
        rs = []
        for rep in range(16):
            a = 3 * rep + k
            f = (1 - L) % 16 or 16
            rs += [(5, a, 9, a + L - 1), (5, 7 * rep, 9, 7 * rep + f - 1)]
        recs.append(rs)
    c["lengths_at_every_residue"] = Case(reads, [k % 2 == 1 for k in range(len(LENGTHS))], recs, 1000, [0] * len(LENGTHS), 1)
    # stored reads at every offset modulo 32 (so every residue modulo 16 of the byte blob and every place in a packed word); pieces that are the
    # whole read, its first and its last base, and that start and end on, before and behind a word border
    reads, gaps, recs, acc = [], [], [], 0
    for k in range(32):
        gap = (k - acc) % 32 + 32 * (k % 2)
        acc += gap
        assert acc % 32 == k
        a = (32 - k) % 32 or 32                                                    # q'[a] is the first base of a word (of a forward read)
        rs = [(0, 0, 0, 69), (10, 0, 10, 0), (20, 69, 20, 69), (30, a - 1, 30, a + 16), (0, a, 0, a + 31), (10, a + 1, 10, a + 33), (20, 2, 20, a - 1), (30, 2, 30, a),
              (0, 2, 0, a + 1), (10, 69 - a, 10, 69), (20, 69 - a - 1, 20, 68), (30, 69 - a + 1, 30, 69)]
        reads.append(rng.integers(0, 4, 70)); gaps.append(gap); recs.append(rs)
        acc += 70
    c["stored_at_every_offset"] = Case(reads, [k % 2 == 1 for k in range(32)], recs, 10, [0] * 32, 4, gaps=gaps)
    c["marked_read_of_length_1"] = Case([[2], [1], [0, 3]], [True, False, True], [[(0, 0, 0, 0)], [(1, 0, 1, 0)], [(2, 0, 3, 1)]], 5, [0, 0, 0], 1)
    # 1 B/base codes above 3, forward and marked: & 3, ^ 3
    reads = _reads(rng, [40, 40, 17, 1], raw=True)
    c["codes_above_3"] = Case(reads, [False, True, True, False], [[(0, 0, 9, 39), (10, 3, 19, 22)], [(0, 0, 9, 39), (10, 1, 19, 35)], [(3, 0, 4, 16)], [(12, 0, 12, 0)]],
                              10, [0, 0, 1, 0], 3, raw=True)
    # NONE records and pairs without records among good ones
    reads = _reads(rng, [50] * 6)
    good = lambda m, a, b: (10 * m + 1, a, 10 * m + 8, b)
    c["none_records"] = Case(reads, [False, True] * 3, [[good(0, 0, 9), (NONE,) * 4, good(2, 20, 29)], [(NONE,) * 4], [good(1, 5, 5)], [(NONE,) * 4, (NONE,) * 4, good(2, 0, 49)],
                                                        [good(0, 10, 40)], [(NONE,) * 4]], 10, [0] * 6, 3)
    c["pairs_without_records"] = Case(reads, [False, True] * 3, [[], [good(1, 0, 9)], [], [], [good(0, 3, 30), good(1, 31, 49)], []], 10, [0] * 6, 2)
    # inconsistent records, each alone in a call together with good ones
    base = [[good(0, 0, 9), good(1, 10, 19)], [good(0, 5, 44)], [good(1, 0, 49), good(2, 7, 7)]]

    def with_bad(bad, gbase=(0, 0, 0), nwin=3):
        return Case(reads[:3], [False, True, False], [base[0], [bad] + base[1], base[2] + [bad]], 10, list(gbase), nwin)
    c["q_last_at_qlen"] = with_bad((11, 40, 18, 50))
    c["q_last_far_above_qlen"] = with_bad((11, 40, 18, 0xFFFFFFFE))
    c["q_first_above_q_last"] = with_bad((11, 30, 18, 29))
    c["t_first_above_t_last"] = with_bad((19, 3, 18, 9))
    c["window_at_nwin"] = with_bad((30, 3, 31, 9))
    c["window_far_above_nwin"] = with_bad((0xFFFFFFF0, 3, 0xFFFFFFF1, 9))
    c["gbase_pushes_a_pair_out"] = with_bad((11, 3, 18, 9), gbase=(0, 2, 1))             # pair 1's window 1 is 3, pair 2's window 2 is 3: outside
    c["gbase_2_pow_40"] = with_bad((11, 3, 18, 9), gbase=(0, 1 << 40, 0))
    c["gbase_near_2_pow_64"] = with_bad((11, 3, 18, 9), gbase=(0, (1 << 64) - 1, 0))    # (would wrap to window 0)
    # two records of one pair in the same window, and a later record in an earlier window: the order is by record index
    c["two_records_in_one_window"] = Case(reads[:3], [True, False, False], [[good(1, 30, 39), good(1, 0, 9), good(0, 10, 12), good(1, 0, 9)], [good(1, 0, 49), good(0, 1, 1)],
                                                                           [good(0, 2, 3), good(1, 4, 8), good(1, 4, 8)]], 10, [0, 0, 0], 2)
    c["no_pairs"] = Case([], [], [], 10, [], 4)
    c["no_windows"] = Case(reads[:2], [False, True], [[good(0, 0, 9)], [good(1, 0, 9)]], 10, [0, 0], 0)
    c["one_window"] = Case(reads[:3], [False, True, True], [[good(0, 0, 9), good(1, 0, 9)], [good(0, 3, 49)], [good(0, 0, 0), (9, 49, 9, 49)]], 10, [0, 0, 0], 1)
    c["window_1"] = Case(reads[:3], [False, True, False], [[(m, 2 * m, m, 2 * m + 1) for m in range(20)], [(m, m, m, m) for m in range(5, 15)], [(19, 0, 19, 49), (20, 0, 20, 49)]],
                         1, [0, 0, 0], 20)
    big = 0xFFFFFFFF
    c["window_max"] = Case(reads[:3], [False, True, False], [[(0, 0, 5, 9), (big - 1, 10, big - 1, 19)], [(0x80000000, 0, 0x80000001, 49)], [(7, 3, 7, 3)]], big, [0, 1, 2], 3)
    # 1000 random pairs over 50 windows: 0 .. 6 records a pair, one in ten of them NONE, one in ten broken
    reads = _reads(rng, rng.integers(1, 300, 1000))
    recs, gb = [], []
    for r in reads:
        rs, n = [], len(r)
        for _ in range(int(rng.integers(0, 7))):
            a = int(rng.integers(0, n))
            b = int(rng.integers(a, n))
            tf = int(rng.integers(0, 1300))
            x = int(rng.integers(0, 10))
            rs.append((NONE,) * 4 if x == 0 else (tf, b, tf + 3, a + n) if x == 1 else (tf, a, tf + int(rng.integers(0, 25)), b))
        recs.append(rs)
        gb.append(int(rng.integers(0, 30)))
    c["thousand_pairs"] = Case(reads, [bool(x) for x in rng.integers(0, 2, 1000)], recs, 50, gb, 50)
    # the arena test's batch: 30 windows, 300 pieces
    reads = _reads(rng, rng.integers(20, 200, 100))
    recs = [[(int(t), 0, int(t) + 5, int(rng.integers(0, len(r)))) for t in sorted(rng.choice(30, 3, replace=False) * 10)] for r in reads]
    c["arena_batch"] = Case(reads, [k % 2 == 0 for k in range(100)], recs, 10, [0] * 100, 30)
    # 16 400 windows, nearly all empty: pieces on both sides of the borders of the scans' tiles of 4096 counts and of the 16 384 counts up to which
    # 32-bit counts are scanned by one block, and in the last window; one to three pieces a window, a pair and a record each, placed by gbase
    depth = dict(zip(MANY_WINDOWS, (3, 1, 2, 3, 2, 3, 1, 2, 3, 2)))
    gb = [g for g in MANY_WINDOWS for _ in range(depth[g])]
    gb = [gb[i] for i in rng.permutation(len(gb))] + [int(g) for g in rng.integers(0, MANY_NWIN, 40 - len(gb))]
    reads = _reads(rng, rng.integers(20, 61, len(gb)))
    recs = []
    for r in reads:
        a = int(rng.integers(0, len(r)))
        recs.append([(int(rng.integers(0, 10)), a, 9, int(rng.integers(a, len(r))))])
    c["many_windows"] = Case(reads, [k % 3 == 1 for k in range(len(gb))], recs, 10, gb, MANY_NWIN)
    return c
