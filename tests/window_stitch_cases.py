"""bsa_window_stitch_* (include/bsalign_hip.h): the definition in Python (window_stitch_ref) -- the readable record in Python integers, a column's
bytes, what it emits, the runs, the records, both offset arrays and the arena rule --, a checker that walks a window's words (cigar_apply), and the
builders of the batches the tests upload: random MSAs with hand-made consensus bytes (no consensus run is needed to reach a case), the two worked
examples of the header typed in byte by byte, the hand-made windows, one window for every way a record fails, a fixed batch for the arena contract,
and the closed loop with a coverage hole.  No GPU is used here."""
import numpy as np

from window_msa_cases import CNS_WINDOW_DTYPE, NO_IDXS

ST_CALLED, ST_DRAFT, ST_BAD_RECORD = 0, 1, 2
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
FILL = 0xA5
FILL32 = 0xA5A5A5A5
U64 = 1 << 64
SYMBOLS = ("bsa_window_stitch_run", "bsa_window_stitch_batch")
STITCH_DTYPE = np.dtype([(n, np.uint32) for n in ("status", "slen", "eq", "x", "ins", "del", "kept", "ncig")])
# the kernels' tile paths (bsa_window_stitch.hip: a wave's 8176 bytes of LDS): 64 columns a tile up to nall 124, fewer up to nall 8173, by rows above
TILE_64_NALL, TILE_1_NALL = 124, 8173


def need_symbols():
    """every test of bsa_window_stitch_* begins here: without the symbols none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in SYMBOLS:
        assert hasattr(B.lib(), name), "the library does not export " + name


def readable(w, cols_cap):
    """the readable record, in Python integers: nothing wraps"""
    cols_off, nall, mlen = int(w["cols_off"]), int(w["nall"]), int(w["mlen"])
    if int(w["idxs_off"]) != NO_IDXS or nall < 1 or mlen >= 1 << 28:
        return False
    end = cols_off + mlen * (nall + 3)
    return end < U64 and end <= cols_cap


def column_units(cols, called, min_cov):
    """cols: an (mlen, nall + 3) array -> for every column (kind: 0 or the unit's op, emit, symbol, quality, alternative, kept)"""
    nall = cols.shape[1] - 3
    d, c, q, a = (cols[:, nall - 1 + k].astype(np.int64) for k in range(4))
    cov = (cols[:, :nall - 1] <= 4).sum(axis=1)
    covered = (cov >= min_cov) if called else np.zeros(len(cols), dtype=bool)
    kind_cov = np.where((d > 3) & (c > 3), 0, np.where(d > 3, OP_I, np.where(c > 3, OP_D, np.where(c == d, OP_EQ, OP_X))))
    kind = np.where(covered, kind_cov, np.where(d <= 3, OP_EQ, 0))
    emit = np.where(covered, c <= 3, d <= 3)
    kept = ~covered & (d <= 3)
    return kind, emit, np.where(covered, c, d), np.where(covered, q, 0), np.where(covered, a, 0), kept


def runs(kinds):
    """the maximal runs of equal kind over the units (kinds without the zeros) -> words len << 4 | op"""
    u = np.asarray(kinds)[np.asarray(kinds) != 0]
    if len(u) == 0:
        return np.zeros(0, np.uint32)
    first = np.flatnonzero(np.concatenate([[True], u[1:] != u[:-1]]))
    length = np.diff(np.concatenate([first, [len(u)]]))
    return (length.astype(np.uint32) << np.uint32(4) | u[first].astype(np.uint32)).astype(np.uint32)


class Ref:
    """what a run must leave: the records; seq_off and cig_off; the three sequence arrays (seq_cap bytes) and the words (cig_cap), FILL where no window
    wrote; and per window its bases, qualities, words and draft bases for the checks"""


def window_stitch_ref(cols, records, cols_cap, cns_status, min_cov, seq_cap, cig_cap):
    cols = np.asarray(cols, dtype=np.uint8).reshape(-1)
    n = len(records)
    r = Ref()
    r.rec = np.zeros(n, dtype=STITCH_DTYPE)
    r.win = []
    for g, w in enumerate(records):
        if not readable(w, cols_cap):
            r.rec[g]["status"] = ST_BAD_RECORD
            r.win.append((np.zeros(0, np.uint8),) * 3 + (np.zeros(0, np.uint32), np.zeros(0, np.uint8)))
            continue
        called = cns_status is None or int(cns_status[g]) == 0
        c0, nall, mlen = int(w["cols_off"]), int(w["nall"]), int(w["mlen"])
        mine = cols[c0:c0 + mlen * (nall + 3)].reshape(mlen, nall + 3)
        kind, emit, sym, q, a, kept = column_units(mine, called, int(min_cov))
        words = runs(kind)
        r.rec[g] = (ST_CALLED if called else ST_DRAFT, int(emit.sum()), int((kind == OP_EQ).sum()), int((kind == OP_X).sum()), int((kind == OP_I).sum()),
                    int((kind == OP_D).sum()), int(kept.sum()), len(words))
        dr = mine[:, nall - 1]
        r.win.append((sym[emit].astype(np.uint8), q[emit].astype(np.uint8), a[emit].astype(np.uint8), words, dr[dr <= 3].copy()))
    r.seq_off, r.cig_off = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    r.seq_off[1:] = np.cumsum(r.rec["slen"].astype(np.uint64), dtype=np.uint64)
    r.cig_off[1:] = np.cumsum(r.rec["ncig"].astype(np.uint64), dtype=np.uint64)
    r.seq, r.seq_qlt, r.seq_alt = (np.full(seq_cap, FILL, np.uint8) for _ in range(3))
    r.cig = np.full(cig_cap, FILL32, np.uint32)
    for g in range(n):
        a, b, c, d = int(r.seq_off[g]), int(r.seq_off[g + 1]), int(r.cig_off[g]), int(r.cig_off[g + 1])
        if b <= seq_cap:
            r.seq[a:b], r.seq_qlt[a:b], r.seq_alt[a:b] = r.win[g][0], r.win[g][1], r.win[g][2]
        if d <= cig_cap:
            r.cig[c:d] = r.win[g][3]
    return r


def cigar_apply(draft_bases, seq, words):
    """walks a window's words: = units are equal bases, X units unequal, and the lengths consume exactly the draft bases and the sequence; the runs
    are maximal.  -> (eq, x, ins, del)"""
    i = j = 0
    count = {OP_EQ: 0, OP_X: 0, OP_I: 0, OP_D: 0}
    prev = None
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        assert op in count and n >= 1 and op != prev, ("word", hex(int(w)))
        prev = op
        count[op] += n
        if op in (OP_EQ, OP_X):
            assert i + n <= len(draft_bases) and j + n <= len(seq)
            same = np.asarray(draft_bases[i:i + n]) == np.asarray(seq[j:j + n])
            assert np.all(same) if op == OP_EQ else not np.any(same), ("unit", op, i, j)
        i += n if op != OP_I else 0
        j += n if op != OP_D else 0
    assert i == len(draft_bases) and j == len(seq), (i, len(draft_bases), j, len(seq))
    return count[OP_EQ], count[OP_X], count[OP_I], count[OP_D]


def check_invariants(r, g):
    rec, (seq, _, _, words, dr) = r.rec[g], r.win[g]
    assert int(rec["eq"]) + int(rec["x"]) + int(rec["ins"]) == int(rec["slen"]) == len(seq)
    assert int(rec["eq"]) + int(rec["x"]) + int(rec["del"]) == len(dr)
    assert int(rec["kept"]) <= int(rec["eq"]) and int(rec["ncig"]) == len(words)
    for op, name in ((OP_EQ, "eq"), (OP_X, "x"), (OP_I, "ins"), (OP_D, "del")):
        assert sum(int(w) >> 4 for w in words if int(w) & 15 == op) == int(rec[name])


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------
def random_msa(rng, nall, mlen, odd_codes=False):
    """an (mlen, nall + 3) MSA with every byte made by hand: piece rows that copy a template with substitutions and gaps, are absent (5) at their ends
    or throughout; a draft row with 4 in the insertion columns; called symbols over 0 .. 4 that follow the template or not; any quality bytes.
    odd_codes: codes of the caller's own making too (draft 7, called 9, rows 6 and 255), which the rules already decide."""
    cols = np.zeros((mlen, nall + 3), dtype=np.uint8)
    truth = rng.integers(0, 4, mlen).astype(np.uint8)
    ins = rng.random(mlen) < 0.12                              # an insertion column: the draft holds 4
    for r in range(nall - 1):
        row = truth.copy()
        err = rng.random(mlen) < 0.1
        row[err] = rng.integers(0, 5, size=int(err.sum()))
        row[ins & (rng.random(mlen) < 0.6)] = 4
        kind = rng.random()
        if kind < 0.2:
            row[:] = 5                                         # a dead row
        else:
            if mlen >= 2 and kind < 0.6:
                row[:int(rng.integers(1, mlen))] = 5
            if mlen >= 2 and rng.random() < 0.4:
                row[mlen - int(rng.integers(1, mlen)):] = 5
        if odd_codes:
            odd = rng.random(mlen) < 0.05
            row[odd] = rng.choice(np.array([6, 255], dtype=np.uint8), size=int(odd.sum()))
        cols[:, r] = row
    draft = truth.copy()
    sub = rng.random(mlen) < 0.08
    draft[sub] = rng.integers(0, 4, size=int(sub.sum()))
    draft[ins] = 4
    called = truth.copy()
    other = rng.random(mlen) < 0.15
    called[other] = rng.integers(0, 5, size=int(other.sum()))
    called[ins & (rng.random(mlen) < 0.5)] = 4
    if odd_codes:
        draft[rng.random(mlen) < 0.05] = 7
        called[rng.random(mlen) < 0.05] = 9
    cols[:, nall - 1], cols[:, nall] = draft, called
    cols[:, nall + 1], cols[:, nall + 2] = rng.integers(0, 256, mlen), rng.integers(0, 256, mlen)
    return cols


def make_batch(windows, gap=0):
    """windows: arrays of shape (mlen, nall + 3) -> (the blob, the records: cols_off the running bytes with `gap` unowned FILL bytes in front of every
    window, out_off the running mlen, nseq = nmax = nall - 1: this pass looks at neither)"""
    rec = np.zeros(len(windows), dtype=CNS_WINDOW_DTYPE)
    parts, cacc, oacc = [], 0, 0
    for g, cols in enumerate(windows):
        mlen, nall = cols.shape[0], cols.shape[1] - 3
        if gap:
            parts.append(np.full(gap, FILL, np.uint8))
            cacc += gap
        rec[g] = (cacc, NO_IDXS, oacc, nall, nall - 1, nall - 1, mlen)
        parts.append(cols.reshape(-1))
        cacc += cols.size
        oacc += mlen
    return np.concatenate([np.zeros(0, np.uint8)] + parts), rec


def window_of(units, nall=3, cov=1):
    """a window from a list of column kinds: '=', 'X', 'I', 'D' and '-' (a column that emits nothing); `cov` of the nall - 1 piece rows present"""
    code = {"=": (1, 1), "X": (2, 0), "I": (4, 3), "D": (0, 4), "-": (4, 4)}
    cols = np.full((len(units), nall + 3), 5, dtype=np.uint8)
    cols[:, :cov] = 0
    for i, u in enumerate(units):
        cols[i, nall - 1], cols[i, nall] = code[u]
        cols[i, nall + 1], cols[i, nall + 2] = 40 + i % 50, i % 7
    return cols


NALLS = (1, 2, 3, 5, 41, 63, 64, 65, TILE_64_NALL, 125, 126, 257)
MLENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
KINDS = "=XID"


def mixed_batches():
    """name -> (blob, records, the cns statuses or None): every nall with every mlen, with odd codes in every second batch; the by-rows path and the
    last nall with a tile at mlen 70; one window of 8193 columns; the hand-made windows"""
    out = {}
    rng = np.random.default_rng(5113)
    for i, mlen in enumerate(MLENS):
        out["mlen_%d" % mlen] = make_batch([random_msa(rng, nall, mlen, odd_codes=bool(i & 1)) for nall in NALLS], gap=i % 3) + (None,)
    out["by_rows"] = make_batch([random_msa(rng, nall, 70) for nall in (TILE_1_NALL, TILE_1_NALL + 1, 3, TILE_1_NALL + 1)], gap=1) + (None,)
    out["long_window"] = make_batch([random_msa(rng, 3, 8193), random_msa(rng, 5, 5)]) + (None,)
    hand = [window_of("=" * 200),                                # one run across three tiles (and more where a tile holds fewer columns)
            window_of("=" * 200, nall=TILE_64_NALL + 2),
            window_of(KINDS * 50),                               # the kind changes at every column
            window_of(KINDS * 50, nall=200),
            window_of(("=" * 63 + "--" + "X" * 62 + "-" + "-" + "X" * 10) * 2),       # columns that emit nothing on the tile borders 63 | 64 and 127 | 128
            window_of("-" * 64 + "=" * 64 + "-" * 64 + "=" + "-" * 70 + "="),        # whole tiles that emit nothing, inside a run
            window_of("-" * 130)]
    other = lambda a, b: next(k for k in KINDS if k not in (a, b))
    hand += [window_of(a + "-" + other(a, b) * 2 + "-" + b) for a in KINDS for b in KINDS]      # every kind as the first and as the last word
    hand += [window_of(a * 70 + b * 70) for a in KINDS for b in KINDS if a != b]
    out["hand_made"] = make_batch(hand) + (None,)
    ws = [random_msa(rng, nall, 90) for nall in (4, 2, 70, 4, 130, 9)]
    out["cns_status"] = make_batch(ws) + (np.array([0, 1, 2, 0, 3, 0xFFFFFFFF], dtype=np.uint32),)
    # records that overlap: the same columns six times -- more column words than the pass keeps (cols_cap / 4), so some windows are classified twice
    one = random_msa(rng, 2, 150)
    blob, rec = make_batch([one])
    out["overlapping"] = (blob, np.repeat(rec, 6), None)
    return out


def min_covs(rec):
    """0, 1, 2, 3, 2^32 - 1, and nall - 1 and nall of the batch's windows (the fewest values that cover them)"""
    nalls = sorted(set(int(x) for x in rec["nall"]))
    return sorted({0, 1, 2, 3, 0xFFFFFFFF} | {v for nall in nalls[:6] for v in (nall - 1, nall)})


def bad_batch():
    """called windows alternating with one window for each way a record fails -> (blob, records, cols_cap, the cns statuses, the expected statuses,
    the names).  The columns end exactly at cols_cap."""
    rng = np.random.default_rng(131)
    names = ["idxs_off", "nall_0", "mlen_2_28", "cols_off_wraps", "past_cols_cap", "cns_1", "cns_2", "cns_3"]
    ws = []
    for _ in names:
        ws += [random_msa(rng, 5, int(rng.integers(3, 40))), random_msa(rng, 5, 7)]
    ws.append(random_msa(rng, 5, 11))
    blob, rec = make_batch(ws)
    cols_cap = len(blob)
    cst = np.zeros(len(ws), dtype=np.uint32)
    want = [ST_CALLED] * len(ws)

    def bad(name, status, **fields):
        g = 2 * names.index(name) + 1
        for k, v in fields.items():
            rec[g][k] = v
        want[g] = status
        return g
    bad("idxs_off", ST_BAD_RECORD, idxs_off=0)
    bad("nall_0", ST_BAD_RECORD, nall=0)
    bad("mlen_2_28", ST_BAD_RECORD, mlen=1 << 28, cols_off=0)
    bad("cols_off_wraps", ST_BAD_RECORD, cols_off=U64 - 16)      # (cols_off + 7 * 8 wraps to 40)
    g = bad("past_cols_cap", ST_BAD_RECORD)
    rec[g]["cols_off"] = cols_cap + 1 - 7 * 8
    for k in (1, 2, 3):
        cst[bad("cns_%d" % k, ST_DRAFT)] = k
    return blob, rec, cols_cap, cst, want, names


def arena_batch():
    """eight windows, depths and lengths mixed, one of them without columns, one not called"""
    rng = np.random.default_rng(313)
    shapes = [(4, 30), (2, 1), (9, 64), (3, 0), (65, 17), (5, 100), (1, 33), (6, 48)]
    blob, rec = make_batch([random_msa(rng, nall, mlen) for nall, mlen in shapes])
    return blob, rec, np.array([0, 0, 0, 0, 0, 2, 0, 0], dtype=np.uint32)


# ---- the header's examples, typed in byte by byte ------------------------------------------------------------------------------------------------
def header_example_1():
    """-> (the 50 bytes, the record, {min_cov or 'draft': (seq, qlt, words, eq, x, ins, del, kept)})"""
    piece = [5, 5, 5, 3, 2, 1, 5, 5, 5, 5]
    draft = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    called = [4, 4, 4, 3, 2, 1, 4, 4, 4, 4]
    qlt = [0, 0, 0, 90, 90, 90, 0, 0, 0, 0]
    cols = np.array([[piece[i], draft[i], called[i], qlt[i], 0] for i in range(10)], dtype=np.uint8).reshape(-1)
    rec = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    rec[0] = (0, NO_IDXS, 0, 2, 1, 1, 10)
    W = lambda *p: [n << 4 | op for n, op in p]
    kept_all = ([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], [0] * 10, W((10, OP_EQ)), 10, 0, 0, 0, 10)
    want = {0: ([3, 2, 1], [90, 90, 90], W((3, OP_D), (1, OP_EQ), (1, OP_X), (1, OP_EQ), (4, OP_D)), 2, 1, 0, 7, 0),
            1: ([0, 1, 2, 3, 2, 1, 2, 3, 0, 1], [0, 0, 0, 90, 90, 90, 0, 0, 0, 0], W((4, OP_EQ), (1, OP_X), (5, OP_EQ)), 9, 1, 0, 0, 7),
            2: kept_all, "draft": kept_all}
    return cols, rec, want


def header_example_2():
    """the 12 columns of the bsa_window_cns_* example with vote 1, as that pass leaves them -> (the 72 bytes, the record, {min_cov: (seq, qlt, alt,
    words, ins, kept)})"""
    row0 = [0, 1, 2, 3, 2, 2, 0, 1, 2, 3, 0, 1]
    row1 = [5, 5, 2, 3, 1, 4, 4, 1, 2, 3, 5, 5]
    drow = [0, 1, 2, 3, 4, 4, 0, 1, 2, 3, 0, 1]
    called = [0, 1, 2, 3, 2, 4, 0, 1, 2, 3, 0, 1]
    cq = [90, 90, 90, 90, 2, 4, 10, 90, 90, 90, 90, 90]
    ca = [0, 0, 0, 0, 5, 5, 5, 0, 0, 0, 0, 0]
    cols = np.array([[row0[i], row1[i], drow[i], called[i], cq[i], ca[i]] for i in range(12)], dtype=np.uint8).reshape(-1)
    rec = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    rec[0] = (0, NO_IDXS, 0, 3, 3, 3, 12)
    W = lambda *p: [n << 4 | op for n, op in p]
    bases = [0, 1, 2, 3, 2, 0, 1, 2, 3, 0, 1]
    w3 = W((4, OP_EQ), (1, OP_I), (6, OP_EQ))
    low = (bases, [90, 90, 90, 90, 2, 10, 90, 90, 90, 90, 90], [0, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0], w3, 1, 0)
    want = {0: low, 1: low,
            2: (bases, [0, 0, 90, 90, 2, 10, 90, 90, 90, 0, 0], [0, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0], w3, 1, 4),
            3: ([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], [0] * 10, [0] * 10, W((10, OP_EQ)), 0, 10)}
    return cols, rec, want


# ---- the closed loop with a coverage hole ----------------------------------------------------------------------------------------------------------
HOLES, PART, PART_COLS = (3, 4, 11), 7, 15


def truth_position(ws, d):
    """the truth's position at draft position d (d lies in a diagonal word of ws, the words of the truth against the draft)"""
    i = j = 0                                                  # truth, draft
    for w in ws:
        op, n = int(w) & 15, int(w) >> 4
        if op == OP_I:
            i += n
        elif op == OP_D:
            assert not j <= d < j + n, "a draft position inside a deletion"
            j += n
        else:
            if j <= d < j + n:
                return i + d - j
            i, j = i + n, j + n
    assert d == j
    return i


def closed_loop_with_hole(w=100):
    """window_msa_cases.closed_loop -- a truth of 2000 bases, an edited draft, four error-free reads -- with the reads' pieces taken out of the windows
    HOLES (their guides emptied: dead pieces, rows that are 5 throughout) and cut down to their first PART_COLS columns in window PART (the first word
    of every piece is diagonal and longer: no edit lies within 23 bases of a window border).  -> (truth, draft, the Batch, the sequence a stitch at
    min_cov 1 must give: the truth where a read covers, the draft where none does)"""
    import window_msa_cases as W
    truth, draft, ws, b = W.closed_loop(w=w)
    words, piece = [], b.piece.copy()
    for g in range(b.nwin):
        for j in range(int(b.piece_off[g]), int(b.piece_off[g + 1])):
            mine = b.pcig[int(b.pcig_off[j]):int(b.pcig_off[j + 1])]
            if g in HOLES:
                mine = mine[:0]
            elif g == PART:
                assert int(mine[0]) & 15 == 0 and int(mine[0]) >> 4 > PART_COLS and int(piece[j]["t_first"]) == g * w
                mine = np.array([PART_COLS << 4], dtype=np.uint32)
                piece[j]["len"], piece[j]["t_last"] = PART_COLS, g * w + PART_COLS - 1
            words.append(mine)
    pcoff = np.zeros(len(piece) + 1, dtype=np.uint64)
    pcoff[1:] = np.cumsum([len(x) for x in words], dtype=np.uint64)
    hb = W.Batch(piece, b.piece_off, b.bases, np.concatenate(words), pcoff, b.draft, b.doff, b.dlen, w)
    want = []
    for g in range(b.nwin):
        d0, d1 = g * w, min((g + 1) * w, len(draft))
        if g in HOLES:
            want.append(draft[d0:d1])
        elif g == PART:
            t0 = truth_position(ws, d0)
            want += [truth[t0:t0 + PART_COLS], draft[d0 + PART_COLS:d1]]
        else:
            want.append(truth[truth_position(ws, d0):truth_position(ws, d1)])
    return truth, draft, hb, np.concatenate(want)
