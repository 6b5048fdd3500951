"""bsa_piece_cigars_* (include/bsalign_hip.h): the definition, word by word in Python (piece_cigars_ref), and hand-made alignments and pieces -- the
smallest shapes at which a tile walk, a clip or the arena can go wrong.  No aligner runs here; the GPU tests upload these arrays directly.  A batch
is (records, words per pair, pieces): records and words as in cigar_windows_cases, pieces a PIECE_DTYPE array in the order the call takes them."""
import numpy as np

import cigar_windows_cases as CW
from cigar_windows_cases import M, I, D, N, S, EQ, X, words, record
from window_pieces_cases import PIECE_DTYPE

H, OP15 = 5, 15
NOT_ON_PATH = 1
M32 = 0xFFFFFFFF
MAX_WORDS = 0xFFFFFFFF             # a pair of more words is cut nowhere
DIAG, STEPS = (M, EQ, X), (M, EQ, X, I, D)


def _cut(tb, qb, ws, tf, qf, tl, ql):
    """the words of the piece from column (tf, qf) to column (tl, ql) of the alignment that starts at (tb, qb) and follows ws; None when either
    is not a diagonal column of it"""
    t, q, out = tb, qb & M32, None
    for word in ws:
        op, ln = int(word) & 15, int(word) >> 4
        if op not in STEPS or ln == 0:
            continue                                           # no step, or no unit: dropped
        lo, hi = 0, ln                                         # the units of the word that are kept
        if out is None and op in DIAG and t <= tf < t + ln:
            if (q + tf - t) & M32 != qf:
                return None
            out, lo = [], tf - t
        if out is not None:
            if op in DIAG and t <= tl < t + ln:
                if (q + tl - t) & M32 != ql:
                    return None
                hi = tl - t + 1
                out.append(((hi - lo) << 4) | op)
                return out
            out.append(((hi - lo) << 4) | op)
        if op != I:
            t += ln
        if op != D:
            q = (q + ln) & M32
    return None


def piece_cigars_ref(res, cigar, cigar_off, pieces):
    """the definition -> (pcig_off [len(pieces) + 1], the words, the status of every piece).  res: the n records (structured, or int32[10] rows),
    cigar, cigar_off: the arena and its n + 1 offsets, pieces: a PIECE_DTYPE array"""
    n = len(res)
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    out, status = [], np.zeros(len(pieces), dtype=np.uint32)
    for j, pc in enumerate(pieces):
        k, qf, ln, tf, tl = (int(pc[f]) for f in ("pair", "q_first", "len", "t_first", "t_last"))
        ws = None
        if k < n and tf <= tl and ln >= 1:
            qb, tb, _ = CW._qb_tb_te(res[k])
            c0, c1 = int(cigar_off[k]), int(cigar_off[k + 1])
            if tb >= 0 and c0 < c1 <= c0 + MAX_WORDS:
                ws = _cut(tb, qb, cigar[c0:c1], tf, qf, tl, (qf + ln - 1) & M32)
        if ws is None:
            status[j] = NOT_ON_PATH
        else:
            out += ws
        off[j + 1] = len(out)
    return off, np.array(out, dtype=np.uint32), status


def sums(ws):
    """(units that advance q, units that advance t) of some words"""
    return CW.spans(ws)


def columns(rec, cig):
    """every diagonal column of a pair, unit by unit: (t, q, index of its word, unit inside the word)"""
    qb, tb, _ = CW._qb_tb_te(rec)
    t, q, out = tb, qb, []
    for wi, word in enumerate(cig):
        op, ln = int(word) & 15, int(word) >> 4
        if op in DIAG:
            out += [(t + u, (q + u) & M32, wi, u) for u in range(ln)]
        if op in DIAG or op == D:
            t += ln
        if op in DIAG or op == I:
            q += ln
    return out


def piece(k, a, b):
    """the piece of pair k from column a to column b (entries of columns())"""
    return (k, a[1], (b[1] - a[1] + 1) & M32, a[0], b[0])


def to_pieces(ps):
    """(pair, q_first, len, t_first, t_last) tuples -> PIECE_DTYPE; reserved and base_off are not read by the pass: they hold something"""
    a = np.zeros(len(ps), dtype=PIECE_DTYPE)
    for j, p in enumerate(ps):
        a[j] = (p[0] & M32, p[1] & M32, p[2] & M32, p[3] & M32, p[4] & M32, 0, 1000 + 7 * j)
    return a


def build(batch):
    """-> (records as the structured array, the arena, its offsets, pieces): the arguments of piece_cigars_ref and of the calls"""
    recs, cigs, ps = batch
    arena, off = CW.flatten(cigs)
    return CW.to_struct(recs), arena, off, to_pieces(ps)


def header_example():
    """the worked example of include/bsalign_hip.h, typed in by hand: (batch, pcig_off, words, status)"""
    cig = words((5, M), (2, I), (4, D), (6, M))
    ps = [(0, 3, 3, 7, 9), (0, 6, 8, 10, 19), (0, 14, 2, 20, 21), (0, 6, 3, 10, 12), (0, 7, 7, 10, 19)]
    return (([record(7, 3, cig)], [cig], ps), np.array([0, 1, 5, 6, 6, 6], dtype=np.uint64),
            words((3, M), (2, M), (2, I), (4, D), (4, M), (2, M)), np.array([0, 0, 0, 1, 1], dtype=np.uint32))


def refmode_guide(ws, t_first, t_last, w, wend):
    """what a refmode caller hands bsa_pog_place for a piece: its words between a leading D of t_first % w and a trailing D up to the window's end
    (wend: one behind the window's last target position), zero lengths left out"""
    lead, trail = t_first % w, wend - 1 - t_last
    return np.concatenate([words((lead, D))[:1 if lead else 0], np.asarray(ws, dtype=np.uint32), words((trail, D))[:1 if trail else 0]]).astype(np.uint32)


TILE_WORDS = (0, 1, 63, 64, 65, 128, 129, 200, 2048, 2049, 5000)      # words a pair: tile borders, and 2049 and 5000 for an index stride of 2 and 3


def _pieces_of_pair(rng, k, cols, nwords):
    """pieces of one pair that begin and end at every kind of place"""
    ps = [piece(k, cols[0], cols[-1])]                         # the first column of the first word to the last of the last: the whole pair
    byword = {}
    for c in cols:
        byword.setdefault(c[2], []).append(c)
    wis = sorted(byword)
    edge = [wi for wi in wis if wi % 64 in (0, 63)]
    pick = sorted(set([wis[0], wis[-1]] + edge[:6] + edge[-6:]))
    for wi in pick:
        u = byword[wi]
        ps += [piece(k, u[0], u[-1]), piece(k, u[0], u[0]), piece(k, u[-1], u[-1])]      # one word whole, its first unit, its last unit
        if len(u) >= 3:
            ps.append(piece(k, u[1], u[-2]))                   # strictly inside one word
        later = [c for c in cols if c[2] > wi]
        earlier = [c for c in cols if c[2] < wi]
        if later:
            ps += [piece(k, u[0], later[int(rng.integers(len(later)))]), piece(k, u[-1], later[0]), piece(k, u[len(u) // 2], later[-1])]
        if earlier:
            ps += [piece(k, earlier[int(rng.integers(len(earlier)))], u[-1]), piece(k, earlier[-1], u[0]), piece(k, earlier[0], u[len(u) // 2])]
    if nwords >= 129:                                          # from the first tile into the third and beyond
        a = [c for c in cols if c[2] < 64]
        b = [c for c in cols if c[2] >= 128]
        if b:
            ps += [piece(k, a[len(a) // 2], b[len(b) // 2]), piece(k, a[-1], b[0])]
    for _ in range(10):
        i, j = sorted(int(x) for x in rng.integers(0, len(cols), 2))
        ps.append(piece(k, cols[i], cols[j]))
    return ps


def hand_batches():
    """name -> (records, words per pair, pieces): one call each"""
    rng = np.random.default_rng(4242)
    c = {}
    c["header_example"] = header_example()[0]
    # pairs of every tile size, plain and = / X, with pieces at every kind of place; the pieces are shuffled, so not pair-major
    recs, cigs, ps = [], [], []
    for nw in TILE_WORDS:
        k = len(recs)
        cig = words() if nw == 0 else words((9, M)) if nw == 1 else CW.random_words(rng, nw, eqx=bool(nw & 1))
        rec = record(int(rng.integers(0, 100)), int(rng.integers(0, 100)), cig)
        recs.append(rec); cigs.append(cig)
        cols = columns(rec, cig)
        ps += _pieces_of_pair(rng, k, cols, nw) if cols else [(k, int(rec[1]), 1, int(rec[3]), int(rec[3]))]
    c["tile_sizes"] = (recs, cigs, [ps[i] for i in rng.permutation(len(ps))])
    # I and D words directly inside the borders; a piece inside a gap's neighbours only
    cig = words((3, M), (2, I), (4, M), (2, D), (3, M), (1, I), (1, D), (2, M))
    rec = record(10, 20, cig)
    cols = columns(rec, cig)
    c["gaps_inside_the_borders"] = ([rec], [cig], [piece(0, cols[2], cols[3]), piece(0, cols[6], cols[7]), piece(0, cols[9], cols[10]), piece(0, cols[2], cols[10]),
                                                   piece(0, cols[0], cols[3]), piece(0, cols[6], cols[11])])
    # a deletion that covers a whole window (the second example of bsa_cigar_windows_*, w = 10): the pieces of windows 0, 2 and 3
    cig = words((3, M), (25, D), (3, M))
    c["deletion_over_a_window"] = ([record(0, 0, cig)], [cig], [(0, 0, 3, 0, 2), (0, 3, 2, 28, 29), (0, 5, 1, 30, 30), (0, 0, 6, 0, 30), (0, 2, 2, 2, 28)])
    cig = words((7, EQ), (1, X), (12, EQ), (2, D), (3, X), (1, I), (30, EQ))
    rec = record(4, 4, cig)
    cols = columns(rec, cig)
    c["eqx_words"] = ([rec], [cig], [piece(0, cols[0], cols[-1]), piece(0, cols[7], cols[7]), piece(0, cols[3], cols[8]), piece(0, cols[19], cols[21]), piece(0, cols[22], cols[30])])
    # words of length 0 and ops that take no step, in front of, inside and behind a piece
    cig = words((2, S), (0, M), (4, M), (0, I), (3, H), (0, D), (5, M), (9, N), (2, I), (7, OP15), (0, X), (6, M), (0, M), (4, S), (3, M), (0, D), (2, H))
    rec = record(3, 8, cig)
    cols = columns(rec, cig)
    c["no_step_and_empty_words"] = ([rec], [cig], [piece(0, cols[0], cols[-1]), piece(0, cols[2], cols[10]), piece(0, cols[4], cols[14]), piece(0, cols[9], cols[15]),
                                                   piece(0, cols[3], cols[4]), piece(0, cols[14], cols[17]), piece(0, cols[0], cols[3])])
    # the words run on behind te: the record's te does not matter
    cig = words((20, M), (3, D), (40, M))
    rec = record(0, 0, cig, te=25)
    cols = columns(rec, cig)
    c["words_behind_te"] = ([rec], [cig], [piece(0, cols[5], cols[19]), piece(0, cols[18], cols[40]), piece(0, cols[30], cols[59])])
    # a score-only record with words, a pair without words, a good pair: pieces of all three; two pieces of the good pair that overlap
    cig = words((10, M), (2, I), (10, M))
    good = record(5, 5, cig)
    lost = record(5, 5, cig)
    lost[3] = lost[1] = -1
    cols = columns(good, cig)
    c["pairs_without_an_alignment"] = ([lost, record(5, 5, words()), good], [cig, words(), cig],
                                       [(0, 5, 4, 5, 8), piece(2, cols[0], cols[12]), (1, 5, 1, 5, 5), piece(2, cols[8], cols[19]), (0, 0, 1, 0, 0), piece(2, cols[8], cols[19])])
    c["no_pairs"] = ([], [], [(0, 0, 1, 0, 0), (3, 5, 2, 5, 6)])
    c["no_pieces"] = ([good], [cig], [])
    # the longest words: q wraps behind 20 insertions of 2^28 - 1, t comes close to 2^32 behind 15 such deletions and passes it behind 5 more (the
    # columns there have no t_first that could name them: the last piece names t modulo 2^32 and is not on the path)
    big = (1 << 28) - 1
    cig = np.concatenate([words((5, M)), words((big, I)).repeat(20), words((9, M)), words((big, D)).repeat(15), words((4, M)), words((big, D)).repeat(5), words((3, M))])
    rec = record(0, 0, cig)
    q1, t1, t2 = (5 + 20 * big) & M32, 14 + 15 * big, 18 + 20 * big
    assert t1 + 3 < (1 << 32) < t2
    c["long_words"] = ([rec], [cig], [(0, 2, (q1 + 3 - 2 + 1) & M32, 2, 8), (0, q1, 9, 5, 13), (0, (q1 + 9) & M32, 4, t1, t1 + 3), (0, 0, 5, 0, 4),
                                      (0, 0, (q1 + 13) & M32, 0, t1 + 3), (0, (q1 + 13) & M32, 3, t2 & M32, (t2 + 2) & M32)])
    return c


def not_on_path_batch():
    """pieces that must not be cut, each next to a good one: (batch, names)"""
    cig = words((10, M), (4, D), (3, I), (10, M))             # t 5..14, deletion t 15..18, t 19..28; q 7..16, insertion 17..19, q 20..29
    rec = record(5, 7, cig)
    good = (0, 9, 6, 7, 12)
    bad = [("pair_at_n", (2, 9, 6, 7, 12)), ("pair_far_above_n", (0xFFFFFFFF, 9, 6, 7, 12)), ("t_first_above_t_last", (0, 9, 6, 12, 7)), ("len_0", (0, 9, 0, 7, 12)),
           ("t_first_in_a_deletion", (0, 19, 3, 16, 21)), ("t_last_in_a_deletion", (0, 9, 8, 7, 17)), ("right_t_wrong_q_first", (0, 10, 5, 7, 12)),
           ("right_t_wrong_q_last", (0, 9, 7, 7, 12)), ("last_column_beyond_the_alignment", (0, 22, 9, 21, 29)), ("first_column_in_front_of_it", (0, 6, 3, 4, 6)),
           ("both_beyond", (0, 40, 3, 40, 42)), ("one_column_with_len_2", (0, 9, 2, 7, 7)), ("score_only_pair", (1, 9, 6, 7, 12))]
    lost = record(5, 7, cig)
    lost[3] = lost[1] = -1
    ps = []
    for _, b in bad:
        ps += [b, good]
    return ([rec, lost], [cig, cig], ps), [name for name, _ in bad]


def arena_batch():
    """the capacities test's batch: 40 pieces over six pairs, one in eight not on a path"""
    rng = np.random.default_rng(99)
    recs, cigs, ps = [], [], []
    for k in range(6):
        cig = CW.random_words(rng, int(rng.integers(20, 150)), eqx=bool(k & 1))
        rec = record(int(rng.integers(0, 50)), int(rng.integers(0, 50)), cig)
        recs.append(rec); cigs.append(cig)
    for j in range(40):
        k = j % 6
        cols = columns(recs[k], cigs[k])
        a, b = sorted(int(x) for x in rng.integers(0, len(cols), 2))
        p = piece(k, cols[a], cols[min(b, a + 60)])
        ps.append((k, p[1] + 1, p[2], p[3], p[4]) if j % 8 == 5 else p)
    return (recs, cigs, ps)
