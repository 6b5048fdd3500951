"""bsa_cigar_windows_* (include/bsalign_hip.h): the definition, unit by unit in Python, and hand-made records and words -- the smallest shapes
at which the kernel can go wrong.  No aligner runs here; the GPU tests upload these records and words directly."""
import numpy as np

NONE = 0xFFFFFFFF
M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8
T_LIMIT = 1 << 31                 # a record's target positions are int32: a column at or above 2^31 belongs to no window
RESULT_FIELDS = ("score", "qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln")


def _qb_tb_te(res):
    """a record as align_batch returns it (structured) or as the oracle does (int32[10] in the order of RESULT_FIELDS)"""
    if getattr(res, "dtype", None) is not None and res.dtype.names:
        return int(res["qb"]), int(res["tb"]), int(res["te"])
    return int(res[1]), int(res[3]), int(res[4])


def windows_ref(res, cigar, w):
    """the (nw, 4) uint32 records of one pair: t_first, q_first, t_last, q_last of every window tb // w .. (te - 1) // w"""
    qb, tb, te = _qb_tb_te(res)
    w = int(w)
    assert w > 0
    if tb < 0 or te <= tb or len(cigar) == 0:
        return np.zeros((0, 4), dtype=np.uint32)
    m0, m1 = tb // w, (te - 1) // w
    rec = [[NONE] * 4 for _ in range(m1 - m0 + 1)]
    lim = min((m1 + 1) * w, T_LIMIT)                           # columns in a window above m1 are ignored
    t, q = tb, qb
    for word in cigar:
        op, ln = int(word) & 15, int(word) >> 4
        if op in (M, EQ, X):
            for _ in range(ln):
                if t >= lim:
                    break
                r = rec[t // w - m0]
                if r[0] == NONE:
                    r[0], r[1] = t, q & 0xFFFFFFFF
                r[2], r[3] = t, q & 0xFFFFFFFF
                t += 1
                q += 1
        elif op == I:
            q += ln
        elif op == D:
            t += ln
        if t >= lim:                                           # t never decreases: nothing behind this word counts
            break
    return np.array(rec, dtype=np.uint32).reshape(-1, 4)


def words(*pairs):
    """words((5, M), (2, I)) -> uint32 CIGAR words"""
    return np.array([(ln << 4) | op for ln, op in pairs], dtype=np.uint32)


def spans(cig):
    qn = tn = 0
    for c in cig:
        op, ln = int(c) & 15, int(c) >> 4
        qn += ln if op in (M, EQ, X, I) else 0
        tn += ln if op in (M, EQ, X, D) else 0
    return qn, tn


def record(tb, qb, cig=None, te=None):
    """int32[10] in the order of RESULT_FIELDS; te from the words unless given (an inconsistent pair)"""
    qn, tn = spans(cig) if cig is not None else (0, 0)
    r = np.zeros(10, dtype=np.int32)
    r[1], r[2], r[3], r[4] = qb, (qb + qn) & 0x7FFFFFFF, tb, (tb + tn if te is None else te) & 0x7FFFFFFF      # (qe is not read)
    return r


def to_struct(recs):
    """a list of int32[10] -> the structured array the C calls take (10 x int32 a record)"""
    dt = np.dtype([(f, np.int32) for f in RESULT_FIELDS])
    a = np.zeros((len(recs), 10), dtype=np.int32)
    for k, r in enumerate(recs):
        a[k] = r
    return np.ascontiguousarray(a).view(dt).reshape(len(recs))


def random_words(rng, nwords, maxlen=12, eqx=False):
    """nwords words of 1 .. maxlen units: mostly diagonal, runs of I and D words next to each other as well, an N and a zero-length word now and then"""
    out = []
    for _ in range(nwords):
        r = int(rng.integers(100))
        ln = int(rng.integers(1, maxlen + 1))
        if r < 50:
            op = (EQ if rng.integers(2) else X) if eqx else M
        elif r < 70:
            op = I
        elif r < 92:
            op = D
        elif r < 96:
            op = N
        else:
            op, ln = (M, 0)
        out.append((ln, op))
    return words(*out)


def random_pair(rng, nwords, maxlen=12, eqx=False):
    cig = random_words(rng, nwords, maxlen, eqx)
    return record(int(rng.integers(0, 100)), int(rng.integers(0, 100)), cig), cig


def header_examples():
    """the two worked examples of the header: (w, record, words, expected records)"""
    a = words((5, M), (2, I), (4, D), (6, M))
    b = words((3, M), (25, D), (3, M))
    return [(10, record(7, 3, a), a, np.array([[7, 3, 9, 5], [10, 6, 19, 13], [20, 14, 21, 15]], dtype=np.uint32)),
            (10, record(0, 0, b), b, np.array([[0, 0, 2, 2], [NONE] * 4, [28, 3, 29, 4], [30, 5, 30, 5]], dtype=np.uint32))]


def hand_cases():
    """name -> (w, [records], [words]): one call each"""
    rng = np.random.default_rng(77)
    c = {}

    def one(name, w, tb, qb, cig, te=None):
        c[name] = (w, [record(tb, qb, cig, te)], [cig])

    ex = header_examples()
    c["header_examples"] = (10, [e[1] for e in ex], [e[2] for e in ex])
    one("one_word_10000M", 64, 0, 0, words((10000, M)))
    one("one_word_10000M_off_border", 64, 37, 11, words((10000, M)))
    one("alternating_1M_1D", 7, 3, 5, words(*([(1, M), (1, D)] * 100)))
    one("alternating_1D_1M", 7, 0, 0, words(*([(1, D), (1, M)] * 100)))
    one("D_covers_three_windows", 10, 5, 2, words((8, M), (40, D), (9, M)))          # D over t 13..52: windows 2, 3 and 4 whole
    one("leading_D_and_I", 10, 8, 4, words((5, D), (3, I), (4, M), (2, I), (20, M)))  # window 0 is t 8, 9: deleted
    one("leading_I_then_long_D", 10, 0, 0, words((3, I), (31, D), (2, M), (7, D)))    # windows 0..2 NONE in front, trailing D to te = 40
    one("I_words_only", 10, 12, 3, words((5, I), (3, I)))                             # te == tb: no windows
    one("D_words_only", 10, 12, 3, words((25, D)))                                    # windows and no column: all NONE
    one("tb_on_border", 10, 20, 0, words((30, M)))                                    # te on a border as well: m1 = 4
    one("tb_off_border", 10, 21, 0, words((30, M)))
    one("te_on_border", 10, 3, 1, words((4, M), (3, I), (13, M)))                     # te = 20
    one("one_column", 10, 19, 6, words((1, M)))
    one("w_1", 1, 3, 9, words((5, M), (2, D), (1, I), (4, M)))
    one("w_equals_te", 1000, 0, 0, words((400, M), (7, I), (600, M)))
    one("w_above_tlen", 5000, 123, 45, words((400, M), (9, D), (600, M)))
    one("w_2_pow_31", 1 << 31, 100, 7, words((50, M), (5, D), (50, M)))
    one("w_max", 0xFFFFFFFF, 100, 7, words((50, M), (5, I), (50, M)))
    one("w_large_odd", 0x7FFFFFF1, 5, 0, words((300, X), (2, I), (3, EQ)))
    one("eqx_words", 10, 4, 4, words((7, EQ), (1, X), (12, EQ), (2, D), (3, X), (1, I), (30, EQ)))
    one("other_ops_take_no_step", 10, 4, 4, words((2, S), (7, M), (9, N), (12, M), (3, 5), (5, M)))
    one("zero_length_words", 10, 9, 0, words((0, M), (1, M), (0, D), (0, I), (15, M), (0, M)))
    # the words consume more target than te - tb: columns up to the end of window m1 count, none behind it
    one("more_target_than_te", 10, 0, 0, words((60, M)), te=25)
    one("more_target_D_first", 10, 2, 0, words((5, M), (30, D), (40, M)), te=14)
    big = (1 << 28) - 1                                                                # the longest word: 40 of them pass 2^32 target bases
    one("far_more_target", 10, 0, 0, np.concatenate([words((5, M)), words((big, D), (big, M)).repeat(40)]), te=35)
    one("query_position_wraps", 10, 0, 0, np.concatenate([words((5, M)), words((big, I)).repeat(20), words((9, M))]))
    # ... and less: the windows the words never reach are NONE
    one("less_target_than_te", 10, 0, 0, words((12, M)), te=95)
    one("less_target_no_column", 10, 0, 0, words((5, I)), te=95)
    for nwords in (1, 2, 63, 64, 65, 127, 128, 129, 200):                              # tile edges
        r, cig = random_pair(rng, nwords)
        c["words_%d" % nwords] = (16, [r], [cig])
    r, cig = random_pair(rng, 129, maxlen=1)
    c["words_129_unit_lengths_w_3"] = (3, [r], [cig])
    # pairs with no words and score-only records (tb = -1, with and without words) mixed into a batch
    recs, cigs = [], []
    for k in range(40):
        r, cig = random_pair(rng, int(rng.integers(1, 150)), eqx=bool(k & 1))
        if k % 7 == 3:
            cig = cig[:0]
        if k % 9 == 4:
            r[3] = r[1] = -1
        if k % 11 == 5:
            r[4] = r[3]                                                                # te == tb
        if k == 20:
            r[3], r[1], cig = -1, -1, cig[:0]
        recs.append(r)
        cigs.append(cig)
    c["mixed_batch"] = (25, recs, cigs)
    c["no_pairs"] = (10, [], [])
    recs, cigs = zip(*[random_pair(rng, int(rng.integers(0, 90)), maxlen=int(rng.integers(1, 40))) for _ in range(1000)])
    c["thousand_pairs"] = (50, list(recs), list(cigs))
    return c


def flatten(cigs):
    """the CIGAR arena and its n + 1 offsets"""
    off = np.zeros(len(cigs) + 1, dtype=np.uint64)
    if len(cigs):
        off[1:] = np.cumsum([len(x) for x in cigs], dtype=np.uint64)
    arena = np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(x, dtype=np.uint32) for x in cigs]).astype(np.uint32)
    return arena, off


def expected(w, recs, cigs):
    """-> (per-pair records, the n + 1 offsets)"""
    per = [windows_ref(r, x, w) for r, x in zip(recs, cigs)]
    off = np.zeros(len(per) + 1, dtype=np.uint64)
    if len(per):
        off[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    return per, off
