"""bsa_window_msa_* (include/bsalign_hip.h): the definition, piece by piece in Python (window_msa_ref), and hand-made windows -- the smallest shapes at
which the pass can go wrong.  No aligner runs here; the GPU tests upload these arrays directly.  A Batch holds the arguments of the calls: the piece
records, their offsets by window, the codes, the guides and their offsets, the draft (one base a byte), and doff / dlen."""
import numpy as np

import cigar_windows_cases as CWC
import piece_cigars_cases as PCC
import window_pieces_cases as WPC
from cigar_windows_cases import M, I, D, N, EQ, X, words
from window_pieces_cases import PIECE_DTYPE

DIAG, STEPS = (M, EQ, X), (M, EQ, X, I, D)
MLEN_END = 1 << 31
CNS_WINDOW_DTYPE = np.dtype([("cols_off", np.uint64), ("idxs_off", np.uint64), ("out_off", np.uint64),
                             ("nall", np.uint32), ("nseq", np.uint32), ("nmax", np.uint32), ("mlen", np.uint32)])
NO_IDXS = 0xFFFFFFFFFFFFFFFF
PAR7 = np.array([0.10, 0.10, 0.15, 0.15, 0.20, 0.20, 0.40], dtype=np.float32)      # the reference's default rates (bsa_cns_params_t)


def pack2bit(codes):
    """base i at bits 62 - 2 (i % 32) of word i / 32"""
    nw = (len(codes) + 31) // 32
    buf = np.zeros(nw * 32, dtype=np.uint64)
    buf[:len(codes)] = np.asarray(codes, dtype=np.uint64) & np.uint64(3)
    sh = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
    return np.bitwise_or.reduce(buf.reshape(nw, 32) << sh, axis=1).astype(np.uint64) if nw else np.zeros(0, np.uint64)


class Batch:
    def __init__(self, piece, piece_off, bases, pcig, pcig_off, draft, doff, dlen, window, piece_cap=None, bases_cap=None, pcig_cap=None):
        self.piece = np.ascontiguousarray(piece, dtype=PIECE_DTYPE)
        self.piece_off = np.ascontiguousarray(piece_off, dtype=np.uint64)
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.pcig = np.ascontiguousarray(pcig, dtype=np.uint32)
        self.pcig_off = np.ascontiguousarray(pcig_off, dtype=np.uint64)
        self.draft = np.ascontiguousarray(draft, dtype=np.uint8)
        self.doff = np.ascontiguousarray(doff, dtype=np.uint64)
        self.dlen = np.ascontiguousarray(dlen, dtype=np.uint32)
        self.window = int(window)
        self.nwin = len(self.dlen)
        self.piece_cap = len(self.piece) if piece_cap is None else piece_cap
        self.bases_cap = len(self.bases) if bases_cap is None else bases_cap
        self.pcig_cap = len(self.pcig) if pcig_cap is None else pcig_cap
        assert len(self.piece_off) == self.nwin + 1 and len(self.doff) == self.nwin and len(self.pcig_off) == self.piece_cap + 1
        assert self.piece_cap <= len(self.piece) and self.bases_cap <= len(self.bases) and self.pcig_cap <= len(self.pcig)


def live_guide(b, j, L):
    """the live predicate for piece j in a window of L draft bases: (the guide as (op, length) pairs, a, b) or None"""
    pc = b.piece[j]
    o0, o1 = int(b.pcig_off[j]), int(b.pcig_off[j + 1])
    if not (o0 < o1 <= b.pcig_cap):
        return None
    ws = [(int(w) & 15, int(w) >> 4) for w in b.pcig[o0:o1]]
    if any(op not in STEPS or ln < 1 for op, ln in ws):
        return None
    if ws[0][0] not in DIAG or ws[-1][0] not in DIAG:
        return None
    ln, tf, tl = int(pc["len"]), int(pc["t_first"]), int(pc["t_last"])
    if sum(n for op, n in ws if op != D) != ln or sum(n for op, n in ws if op != I) != tl - tf + 1:
        return None
    if ln < 1 or int(pc["base_off"]) + ln > b.bases_cap:
        return None
    a = tf % b.window
    if not a + (tl - tf) < L:
        return None
    return ws, a, a + (tl - tf)


def window_ref(b, g):
    """window g -> (depth, mlen, ins as a list, the columns as an (mlen, depth + 4) uint8 array, the rows that are live)"""
    L = min(int(b.dlen[g]), b.window)
    x, y = int(b.piece_off[g]), int(b.piece_off[g + 1])
    depth = 0 if (y > b.piece_cap or y < x) else y - x
    guides = [live_guide(b, x + r, L) for r in range(depth)]
    ins = [0] * L
    for gd in guides:
        if gd is None:
            continue
        col, run = gd[1], 0
        for op, n in gd[0]:
            if op == I:
                run += n
                continue
            if run:
                ins[col], run = max(ins[col], run), 0
            col += n
    mlen = L + sum(ins)
    if mlen >= MLEN_END:
        return depth, 0, ins, np.zeros((0, depth + 4), np.uint8), [gd is not None for gd in guides]
    c = (np.arange(L, dtype=np.int64) + np.cumsum(np.array(ins, dtype=np.int64))) if L else np.zeros(0, np.int64)
    cols = np.full((mlen, depth + 4), 5, dtype=np.uint8)
    cols[:, depth] = 4
    cols[:, depth + 1] = 4
    cols[:, depth + 2:] = 0
    o = int(b.doff[g])
    cols[c, depth] = b.draft[o:o + L] & 3
    for r, gd in enumerate(guides):
        if gd is None:
            continue
        ws, a, _ = gd
        bo = int(b.piece[x + r]["base_off"])
        code = b.bases[bo:bo + int(b.piece[x + r]["len"])] & 3
        col, qi, run, qrun = a, 0, 0, 0
        for op, n in ws:
            if op == I:
                if run == 0:
                    qrun = qi
                run += n
                qi += n
                continue
            for u in range(n):
                j = col + u
                if j > a:
                    cols[c[j - 1] + 1:c[j], r] = 4
                    if u == 0 and run:
                        cols[c[j - 1] + 1:c[j - 1] + 1 + run, r] = code[qrun:qrun + run]
                cols[c[j], r] = code[qi + u] if op != D else 4
            col += n
            if op != D:
                qi += n
            run = 0
    return depth, mlen, ins, cols, [gd is not None for gd in guides]


def window_msa_ref(b, vote=0):
    """the definition -> (cols_off [nwin + 1], the records as a CNS_WINDOW_DTYPE array, all the bytes)"""
    off = np.zeros(b.nwin + 1, dtype=np.uint64)
    cwin = np.zeros(b.nwin, dtype=CNS_WINDOW_DTYPE)
    parts, out = [np.zeros(0, np.uint8)], 0
    for g in range(b.nwin):
        depth, mlen, _, cols, _ = window_ref(b, g)
        cwin[g] = (int(off[g]), NO_IDXS, out, depth + 1, depth + vote, depth + vote, mlen)
        parts.append(cols.reshape(-1))
        off[g + 1] = int(off[g]) + cols.size
        out += mlen
    return off, cwin, np.concatenate(parts)


# ---- building batches ------------------------------------------------------------------------------------------------------------------------
def guide_sums(ws):
    q = sum(int(w) >> 4 for w in ws if int(w) & 15 in (M, EQ, X, I))
    t = sum(int(w) >> 4 for w in ws if int(w) & 15 in (M, EQ, X, D))
    return q, t


def make(windows, window, seed=1, gap=0, codes_above_3=False):
    """windows: a list of (draft codes or a length, dlen or None, [(t_first, words[, codes])]) -> Batch.  t_first is a position in the window
    (any multiple of `window` may be added to it by the caller); codes are drawn where not given; `gap` bases lie between the windows' drafts."""
    rng = np.random.default_rng(seed)
    piece, poff, bases, pcig, pcoff, draft, doff, dlen = [], [0], [], [], [0], [], [], []
    for g, (dr, dl, ps) in enumerate(windows):
        dr = rng.integers(0, 4, dr).astype(np.uint8) if np.isscalar(dr) else np.asarray(dr, dtype=np.uint8)
        draft += [0] * gap
        doff.append(len(draft))
        draft += dr.tolist()
        dlen.append(len(dr) if dl is None else dl)
        for p in ps:
            tf, ws = p[0], np.asarray(p[1], dtype=np.uint32)
            qn, tn = guide_sums(ws)
            code = np.asarray(p[2], dtype=np.uint8) if len(p) > 2 else rng.integers(0, 256 if codes_above_3 else 4, qn).astype(np.uint8)
            piece.append((len(piece), 100 + 3 * len(piece), len(code), tf, tf + tn - 1, 0, len(bases)))
            bases += code.tolist()
            pcig += ws.tolist()
            pcoff.append(len(pcig))
        poff.append(len(piece))
    return Batch(np.array(piece, dtype=PIECE_DTYPE), poff, bases, pcig, pcoff, draft + [0] * 8, doff, dlen, window)


def random_guide(rng, tspan, nwords=None, eqx=False):
    """words over exactly tspan target bases, diagonal at both ends; nwords: exactly that many words (tspan permitting), 1M 1I 1M 1D .. style"""
    dg = lambda: int(rng.choice([EQ, X])) if eqx else M
    if tspan == 1:
        return words((1, dg()))
    if nwords is not None:
        assert nwords >= 1
        if nwords == 1:
            return words((tspan, dg()))
        # nwords odd: M g M g .. M with (nwords - 1) / 2 gaps; even: one more M word in front
        k, lead = (nwords - 1) // 2, (nwords - 1) % 2
        gaps = [I if rng.integers(2) else D for _ in range(k)]
        nd = sum(1 for x in gaps if x == D)
        assert tspan >= (k + 1 + lead) + nd, "too many words for the span"
        out = [(1, dg())] * lead
        spare = tspan - (k + 1 + lead) - nd
        for i in range(k):
            out += [(1, dg()), (int(rng.integers(1, 4)) if gaps[i] == I else 1, gaps[i])]
        out.append((1 + spare, dg()))
        return words(*out)
    out, t = [], 0
    while t < tspan:
        left = tspan - t
        if out and out[-1][1] in DIAG and left >= 2 and rng.integers(3) == 0:
            op = I if rng.integers(2) else D
            n = int(rng.integers(1, 4))
            if op == D:
                n = min(n, left - 1)
                t += n
            out.append((n, op))
            if rng.integers(6) == 0 and op == I:
                out.append((int(rng.integers(1, 3)), I))               # two I words in a row: one column
        else:
            n = int(rng.integers(1, min(left, 9) + 1))
            out.append((n, dg()))
            t += n
    if out[-1][1] not in DIAG:
        out.append((1, dg()))
    return words(*out)


def random_window(rng, L, depth, eqx=False, nwords=None):
    ps = []
    for _ in range(depth):
        a = int(rng.integers(0, L))
        b = int(rng.integers(a, L))
        if rng.integers(3) == 0:
            a, b = 0, L - 1
        ps.append((a, random_guide(rng, b - a + 1, nwords, eqx)))
    return (L, None, ps)


def header_example():
    """the worked example of include/bsalign_hip.h, typed in by hand: (Batch, the 72 bytes)"""
    b = make([([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], None, [(0, words((4, M), (2, I), (6, M)), [0, 1, 2, 3, 2, 2, 0, 1, 2, 3, 0, 1]),
                                                      (2, words((2, M), (1, I), (1, D), (3, M)), [2, 3, 1, 1, 2, 3])])], 10)
    row0 = [0, 1, 2, 3, 2, 2, 0, 1, 2, 3, 0, 1]
    row1 = [5, 5, 2, 3, 1, 4, 4, 1, 2, 3, 5, 5]
    drow = [0, 1, 2, 3, 4, 4, 0, 1, 2, 3, 0, 1]
    return b, np.array([[row0[i], row1[i], drow[i], 4, 0, 0] for i in range(12)], dtype=np.uint8).reshape(-1)


DEPTHS = (0, 1, 15, 16, 17, 63, 64, 65, 200)
GUIDE_WORDS = (1, 16, 17, 64, 65, 200)


def dead_batch():
    """every clause of the live predicate violated in one piece each, every such piece between two live ones that insert: (Batch, names, name ->
    piece).  Window 16, dlen 12.  (The two clauses about offsets that a piece cannot violate without its neighbours: dead_offsets_batches.)"""
    good = (2, words((3, M), (2, I), (4, M)))
    ins5 = words((3, M), (5, I), (3, M))
    bad = [("no_words", (1, words(), [0, 1, 2, 3, 0, 1])), ("op_N", (1, words((2, M), (3, N), (4, M)))), ("op_15", (1, words((2, M), (1, 15), (4, M)))),
           ("length_0", (1, words((2, M), (0, I), (4, M)))), ("first_word_I", (1, words((4, I), (6, M)))), ("last_word_D", (1, words((6, M), (2, D)))),
           ("first_word_D", (1, words((1, D), (5, M)))), ("q_sum_short", (1, ins5)), ("t_sum_long", (1, ins5)), ("len_0", (1, ins5)),
           ("codes_behind_bases_cap", (1, ins5)), ("b_at_L", (7, ins5)), ("t_last_below_t_first", (1, ins5)), ("b_behind_the_window", (14, ins5))]
    ps = []
    for _, p in bad:
        ps += [good, p]
    ps.append(good)
    b = make([(16, 12, ps)], 16, seed=5)
    at = {name: 2 * i + 1 for i, (name, _) in enumerate(bad)}
    pc = b.piece
    j = at["no_words"]; pc[j]["t_last"] = int(pc[j]["t_first"]) + 5          # six codes, a span of six, and no word
    j = at["q_sum_short"]; pc[j]["len"] = int(pc[j]["len"]) + 1
    j = at["t_sum_long"]; pc[j]["t_last"] = int(pc[j]["t_last"]) - 1
    j = at["len_0"]; pc[j]["len"] = 0
    j = at["codes_behind_bases_cap"]; pc[j]["base_off"] = len(b.bases) - int(pc[j]["len"]) + 1
    j = at["t_last_below_t_first"]; pc[j]["t_first"], pc[j]["t_last"] = 7, 1
    return b, [name for name, _ in bad], at


def dead_offsets_batches():
    """pcig_off[j + 1] above pcig_cap, and pcig_off[j] >= pcig_off[j + 1]: two windows of one piece each, one dead, one live"""
    out = {}
    two = [(16, None, [(1, words((6, M)))]), (16, None, [(0, words((3, M), (1, I), (3, M)))])]
    b = make(two, 16, seed=6)
    b.pcig_cap = 3                                             # piece 1's words end at 4
    out["words_behind_the_cap"] = b
    b = make(two, 16, seed=6)
    b.pcig_off[:] = [4, 1, 4]                                  # piece 0: offsets decrease; piece 1: its three words
    out["offsets_decrease"] = b
    return out


def hand_batches():
    """name -> Batch: one call each"""
    rng = np.random.default_rng(2024)
    c = {}
    c["header_example"] = header_example()[0]
    # every depth, window 16, random guides (I words in a row among them), L = window
    c["depths"] = make([random_window(rng, 16, d) for d in DEPTHS], 16, seed=11, gap=3)
    c["depths_eqx"] = make([random_window(rng, 16, d, eqx=True) for d in (3, 17, 64)], 16, seed=12, codes_above_3=True)
    # L = 1, window - 1, window; dlen above the window; dlen 0 with and without pieces
    c["draft_lengths"] = make([random_window(rng, 1, 3), random_window(rng, 15, 5), random_window(rng, 16, 5), (40, 40, random_window(rng, 16, 4)[2]),
                               (0, 0, []), (5, 0, [(0, words((3, M)))]), random_window(rng, 7, 2)], 16, seed=13)
    c["window_1"] = make([(1, None, [(0, words((1, M)))] * 3), (1, None, []), (1, None, [(0, words((1, X)))]), (0, 0, [(0, words((1, M)))])], 1, seed=14)
    c["window_500"] = make([random_window(rng, 500, 5), random_window(rng, 499, 17), random_window(rng, 500, 3, eqx=True)]
                           + [(500, None, [(int(rng.integers(0, 40)), random_guide(rng, 460, nw)) for nw in GUIDE_WORDS])], 500, seed=15, gap=5)
    c["window_4096"] = make([random_window(rng, 4096, 3), random_window(rng, 4095, 2), (4096, None, [(0, random_guide(rng, 4096, 200)), (4095, words((1, M)))])], 4096, seed=16)
    # the shapes the definition speaks of, typed in by hand (window 16, L 16 unless said)
    c["shapes"] = make([
        (16, None, [(10, words((5, M), (3, I), (1, M)))]),                                      # an insertion in front of the last draft column
        (16, None, [(0, words((4, M), (1, I), (12, M))), (2, words((2, M), (3, I), (5, M))), (3, words((1, M), (2, I), (1, M))), (0, words((16, M))),
                    (4, words((6, M)))]),                                                        # 1, 3, 2, none and no neighbour at column 4
        (16, None, [(3, words((1, M), (1, D), (5, M), (1, D), (1, M))), (3, words((1, M), (2, I), (7, M), (1, I), (1, M)))]),      # deletions at the second and second-to-last column
        (16, None, [(j, words((1, M))) for j in (0, 7, 15, 15)]),                                # pieces of one draft column
        (16, None, [(1, words((2, EQ), (1, X), (2, I), (3, EQ), (2, D), (1, X))), (0, words((3, X), (1, I), (13, EQ)))]),
        (16, None, [(2, words((3, M), (2, I), (1, I), (2, D), (1, I), (4, M))), (2, words((3, M), (1, I), (9, M)))]),      # I words in a row; I D I: two columns
        (12, None, [(0, words((6, M), (4, I), (6, M)))]),                                        # a draft of 12 bases: b = 11 = L - 1
        (16, None, []),
    ], 16, seed=17, codes_above_3=True)
    c["no_windows"] = Batch(np.zeros(0, PIECE_DTYPE), [0], [], [], [0], [0] * 8, [], [], 16)
    # packed drafts: 32 windows whose slices start at every offset modulo 32
    c["draft_offsets"] = make([random_window(rng, 16, 2) for g in range(32)], 16, seed=18, gap=1)      # (steps of 17: every residue, asserted in the CPU tests)
    # around the depth at which the fill gives up a thread a piece (256) and writes a window in place
    c["deep_windows"] = make([random_window(rng, 16, d) for d in (256, 257, 300)] + [random_window(rng, 40, 260)], 40, seed=22)
    return c


def piece_off_batches():
    """piece_off[g + 1] above piece_cap, and offsets that decrease: those windows have no rows, the others are what they are"""
    rng = np.random.default_rng(31)
    out = {}
    b = make([random_window(rng, 16, 2), random_window(rng, 16, 3), random_window(rng, 16, 2)], 16, seed=19)
    b.piece_off[:] = [0, 2, 9, 7]                              # window 1 ends above piece_cap = 7: no rows; window 2: 9 > 7 decreases: no rows
    out["above_piece_cap"] = b
    b = make([random_window(rng, 16, 2), random_window(rng, 16, 3), random_window(rng, 16, 2)], 16, seed=20)
    b.piece_off[:] = [0, 5, 3, 7]                              # window 1 decreases; window 2 holds pieces 3..6, two of which window 0 holds too
    out["decreasing"] = b
    return out


def arena_batch():
    """the capacities test's batch: seven windows of different depth and length, one of them without bytes"""
    rng = np.random.default_rng(77)
    return make([random_window(rng, 16, 3), random_window(rng, 9, 1), (0, 0, []), random_window(rng, 16, 17), random_window(rng, 16, 0), random_window(rng, 13, 6),
                 random_window(rng, 16, 2)], 16, seed=21, gap=2)


# ---- the closed loop: a truth, a draft with edits, error-free reads --------------------------------------------------------------------------
def edited_draft(rng, n=2000, w=100, border=20, apart=30):
    """-> (truth, draft, the CIGAR words of truth (query) against draft (target)): substitutions, insertions and deletions of 1 .. 3 bases, each at
    least `border` draft bases from every multiple of w and at least `apart` from the next"""
    truth = rng.integers(0, 4, n).astype(np.uint8)
    draft, ws = [], []
    i = 0                                                      # position in the truth
    run = 0                                                    # equal bases since the last edit

    def flush():
        nonlocal run
        if run:
            ws.append((run, M))
            run = 0
    next_edit = 40
    while i < n:
        d = len(draft)
        if d >= next_edit and border + 3 <= d % w <= w - border - 4 and i + 4 < n:
            kind, k = int(rng.integers(3)), int(rng.integers(1, 4))
            if kind == 0:                                      # substitution: the draft holds other bases
                draft += [(int(x) + 1 + int(rng.integers(3))) & 3 for x in truth[i:i + k]]
                run += k
                i += k
            elif kind == 1:                                    # the draft lacks k bases of the truth: an insertion of the read
                flush()
                ws.append((k, I))
                i += k
            else:                                              # the draft has k bases too many: a deletion of the read
                flush()
                ws.append((k, D))
                draft += [int(x) for x in rng.integers(0, 4, k)]
            next_edit = len(draft) + apart
            continue
        draft.append(int(truth[i]))
        run += 1
        i += 1
    flush()
    return truth, np.array(draft, dtype=np.uint8), words(*ws)


def from_python_calls(windows_out, guides, drafts, window):
    """what Context.window_pieces and Context.piece_cigars return, and one draft slice a window, as a Batch (the packing of Context.window_msa)"""
    piece = np.concatenate([np.zeros(0, PIECE_DTYPE)] + [np.asarray(ps, dtype=PIECE_DTYPE) for ps, _ in windows_out]).copy()
    poff = np.concatenate([[0], np.cumsum([len(ps) for ps, _ in windows_out])]).astype(np.uint64)
    codes = [np.asarray(c, dtype=np.uint8) for _, cs in windows_out for c in cs]
    ws = [np.asarray(w, dtype=np.uint32) for gs in guides for w, _ in gs]
    boff = np.concatenate([[0], np.cumsum([len(c) for c in codes])]).astype(np.uint64)
    piece["base_off"] = boff[:-1]
    pcoff = np.concatenate([[0], np.cumsum([len(w) for w in ws])]).astype(np.uint64)
    dlen = [len(d) for d in drafts]
    doff = np.concatenate([[0], np.cumsum(dlen)])[:-1]
    return Batch(piece, poff, np.concatenate([np.zeros(0, np.uint8)] + codes), np.concatenate([np.zeros(0, np.uint32)] + ws), pcoff,
                 np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(d, dtype=np.uint8) for d in drafts] + [np.zeros(8, np.uint8)]), doff, dlen, window)


# ---- through the references of the three passes before this one -------------------------------------------------------------------------------
def through_the_references(rng, npairs, w, eqx, reads=None, recs=None, cigs=None, draft=None):
    """pairs on one draft through windows_ref, pieces_ref and piece_cigars_ref -> (Batch, status of every piece)"""
    import bsalign_amd as B
    if recs is None:
        recs, cigs = zip(*[CWC.random_pair(rng, int(rng.integers(1, 120)), maxlen=int(rng.integers(1, 12)), eqx=eqx) for _ in range(npairs)])
    wins = [CWC.windows_ref(r, c, w) for r, c in zip(recs, cigs)]
    woff = np.zeros(len(recs) + 1, dtype=np.uint64)
    woff[1:] = np.cumsum([len(x) for x in wins], dtype=np.uint64)
    if reads is None:
        reads = [rng.integers(0, 4, int(r[1]) + CWC.spans(c)[0]).astype(np.uint8) for r, c in zip(recs, cigs)]
    qlen = np.array([len(x) for x in reads], dtype=np.uint32)
    qoff = np.zeros(len(recs), dtype=np.uint64)
    qoff[1:] = np.cumsum(qlen[:-1], dtype=np.uint64)
    tlen = max(int(r[4]) for r in recs) if draft is None else len(draft)
    if draft is None:
        draft = rng.integers(0, 4, tlen).astype(np.uint8)
    gbase, nwin = B.window_gbase(np.zeros(len(recs), np.int64), [tlen], w)
    poff, boff, pieces, codes = WPC.pieces_ref(np.concatenate(reads), qoff, qlen, np.concatenate(wins), woff, w, gbase, nwin, 0)
    arena, coff = CWC.flatten(list(cigs))
    pcoff, pwords, status = PCC.piece_cigars_ref(CWC.to_struct(list(recs)), arena, coff, pieces)
    doff, dlen = B.window_drafts([0], [tlen], w)
    assert len(doff) == nwin
    return Batch(pieces, poff, codes, pwords, pcoff, np.concatenate([draft, np.zeros(8, np.uint8)]), doff, dlen, w), status


def closed_loop(seed=5, w=100, nreads=4):
    """-> (truth, draft, the words of a read against the draft, the Batch of nreads error-free reads through the three references)"""
    rng = np.random.default_rng(seed)
    truth, draft, ws = edited_draft(rng, 2000, w)
    assert guide_sums(ws) == (len(truth), len(draft)) and sum(1 for x in ws if int(x) & 15 == CWC.I) >= 5 and sum(1 for x in ws if int(x) & 15 == CWC.D) >= 5
    rec = CWC.record(0, 0, ws)
    b, status = through_the_references(rng, nreads, w, False, reads=[truth] * nreads, recs=[rec] * nreads, cigs=[ws] * nreads, draft=draft)
    assert np.all(status == 0)
    return truth, draft, ws, b
