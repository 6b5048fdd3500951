"""The corpus of test_align8_steer_sum_gpu.py reaches the rows on which the noise sum of band steering decides (no GPU: everything here is read from the oracle).

Steering (bsalign.h:3331-3349; x_forward_abs, "adaptive band") forms nzsum = sum |ubegs[b + 1] - ubegs[b]| over the sixteen running blocks of the row just
computed, noisy = max(16, nzsum / 16 / W * 16 / 2) with W = bandwidth / 16 (bandwidth 128: max(16, (nzsum >> 7) << 3)) and d16 = ubegs[16] - ubegs[0], and
moves the band by rbx = 2 where noisy < d16, 0 where d16 < -noisy, 1 otherwise (0 on the first bandwidth / 4 rows and once the band has reached the query's
end).  A wrong nzsum therefore shows only on a row where it changes that choice: 16 < |d16| <= noisy (the floor of 16 alone would have moved by 0 or 2), or
noisy < |d16| with noisy above the floor.  Clean reads with a tenth of errors hardly hold such rows; the corpus here does: targets of 256 .. 1000 rows, queries
with stretches of 25 .. 40 % errors, runs of 20 .. 60 inserted or deleted bases, and queries cut to 3 / 4 or drawn out to 5 / 4 of the target's length.

The oracle's row records (orc_align_pairwise_rows: the u bytes of every block and ubegs[0 .. 15] of every row; ubegs[16] is ubegs[15] plus the u bytes of block
15) give nzsum, noisy and d16 of every row in numpy.  steer() is checked against the oracle itself: in extend mode the next row's move is rbx.

D's branch (cell 0's M flag behind the first-cell rule's mask): the corpus also holds rows at rbeg = 0 followed by a row that moves, and rows that stay at
rbeg > 0 directly followed by a row that moves by one."""
import ctypes as C

import numpy as np

import support as S

# (M, X, O, E, Q, P)
SC_BENCH = (2, -6, -3, -2, 0, 0)
SC_LINEAR = (2, -6, 0, -3, 0, 0)
SC_TWO = (2, -6, -3, -2, -8, -1)
SEED = 20261
_CACHE = {}


def max_gape_scoring(opens=(0, -1)):
    """the scoring (1, -1, O, -g, 0, 0), O in `opens`, with the largest g that the launcher still runs in the absolute-score form with three-operand maxima in the
    biased frame at bandwidth 128, asked of the library's own choice (bsa_align8_x_choice_internal); opens = (-1,): the largest with one-piece gaps (the mixed
    launch has no linear form)"""
    key = ("maxg", opens)
    if key not in _CACHE:
        import bsalign_amd as B
        best = None
        for g in range(1, 64):
            for o in opens:
                # (an opening penalty of 1 .. 3 takes the two-bit D / Od fields, code format 1, as the plan would ask for)
                d = B.align8_x_choice(B.make_params(B.MODE_GLOBAL, 128, 1, -1, o, -g, 0, 0), 64, 1000, code_fmt=1 if o else 0)
                if d["launch"] and d["abs"] and d["m3"] and (best is None or g > -best[3]):
                    best = (1, -1, o, -g, 0, 0)
        assert best is not None
        _CACHE[key] = best
    return _CACHE[key]


def _rand(rng, n):
    return rng.integers(0, 4, size=int(n)).astype(np.uint8)


def _rough_pair(rng, lt, ratio):
    """a query that follows the target through clean pieces (a tenth of errors), stretches of 25 .. 40 % errors and runs of 20 .. 60 bases that only one of the two
    has; ratio 3 / 4: the query is cut there; 5 / 4: the target is cut to 4 / 5 of the query"""
    t = _rand(rng, lt)
    parts, x = [], 0
    while x < lt:
        kind = int(rng.integers(0, 4))
        n = int(rng.integers(40, 140))
        if kind == 0:
            parts.append(S.mutate(rng, t[x:x + n], 0.10))
        elif kind == 1:
            parts.append(S.mutate(rng, t[x:x + n], float(rng.uniform(0.25, 0.40))))
        elif kind == 2:
            n = int(rng.integers(20, 61))          # the query lacks these bases
        else:
            parts.append(_rand(rng, int(rng.integers(20, 61))))          # ... or has bases of its own
            n = 0
        x += n
    q = np.concatenate(parts) if parts else _rand(rng, 1)
    if ratio == "3/4":
        q = q[:max(3 * lt // 4, 1)]
    elif ratio == "5/4":
        t = t[:max(4 * len(q) // 5, 1)]
    return np.ascontiguousarray(q), np.ascontiguousarray(t)


def corpus():
    """the rough pairs: built once, shared with the GPU test and never changed"""
    if "corpus" not in _CACHE:
        rng = np.random.default_rng(SEED)
        pairs = []
        for k in range(28):
            lt = int(rng.integers(256, 1001))
            pairs.append(_rough_pair(rng, lt, ("1", "3/4", "5/4", "1")[k % 4]))
        _CACHE["corpus"] = pairs
    return _CACHE["corpus"]


def plain():
    """benchmark pairs of 600 bases, a tenth of errors"""
    if "plain" not in _CACHE:
        _CACHE["plain"] = [S.synth_pair(k, 600) for k in range(28)]
    return _CACHE["plain"]


def batch(tag):
    """groups of sixteen: "rough_ends" has rough pairs first and last in each group of plain ones, "plain_ends" plain pairs first and last among rough ones"""
    if tag not in _CACHE:
        c, p = corpus(), plain()
        if tag == "rough_ends":
            pairs = [c[0]] + p[0:14] + [c[1], c[2]] + p[14:28] + [c[3]]
        elif tag == "plain_ends":
            pairs = [p[0]] + c[0:14] + [p[1], p[2]] + c[14:28] + [p[3]]
        else:
            raise KeyError(tag)
        assert len(pairs) == 32
        _CACHE[tag] = pairs
    return _CACHE[tag]


def steer(q, t, bw, sc, mode=S.MODE_GLOBAL):
    """per row i of the pair, from the oracle's row records: band offset b, nzsum, noisy, d16, whether steering is open on the row (past the first bw / 4 rows and
    the band short of the query's end), and rbx"""
    lib = S.oracle()
    lib.orc_align_pairwise_rows.restype = C.c_long
    q = np.ascontiguousarray(q, dtype=np.uint8)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    tl, W = len(t), bw // 16
    pw = lib.orc_get_piecewise(sc[2], sc[3], sc[4], sc[5], bw)
    cells = ((pw + 1) * W + 3) & ~3
    blk = cells + 4
    tg = max(64 // blk, 1)
    tileb = (tg * blk + 15) & ~15
    begs_bytes = ((tl + 2) * 4 + 15) & ~15
    nbytes = begs_bytes + ((tl + 1 + tg - 1) // tg + 1) * 16 * tileb
    slot = np.zeros(nbytes, dtype=np.uint8)
    res = np.zeros(10, dtype=np.int32)
    m = S.score_matrix(sc[0], sc[1])
    lib.orc_align_pairwise_rows(S.ptr(q, S.u8p), len(q), S.ptr(t, S.u8p), tl, mode, bw, S.ptr(m, S.i8p), sc[2], sc[3], sc[4], sc[5],
                                S.ptr(res, S.i32p), slot.ctypes.data_as(C.c_void_p), 0)
    b = slot[:(tl + 1) * 4].view(np.int32)[1:].astype(np.int64)          # band offset of row i
    r = np.arange(1, tl + 1)[:, None]                                  # record of row i (record 0 is row -1)
    y = np.arange(16)[None, :]
    o0 = begs_bytes + ((r // tg) * 16 + y) * tileb + (r % tg) * blk
    ub = np.zeros((tl, 17), dtype=np.int64)
    w = slot[(o0 + cells)[:, :, None] + np.arange(4)[None, None, :]].astype(np.uint32)
    ub[:, :16] = (w[:, :, 0] | (w[:, :, 1] << 8) | (w[:, :, 2] << 16) | (w[:, :, 3] << 24)).astype(np.int32)
    u15 = slot[o0[:, 15][:, None] + np.arange(W)[None, :]].view(np.int8).astype(np.int64)
    ub[:, 16] = ub[:, 15] + u15.sum(axis=1)
    nzsum = np.abs(np.diff(ub, axis=1)).sum(axis=1)
    noisy = np.maximum(16, (nzsum // 16) // W * 16 // 2)
    d16 = ub[:, 16] - ub[:, 0]
    i = np.arange(tl)
    is_open = (i > bw // 4) & (b + bw < len(q))
    rbx = np.where(~is_open, 0, np.where(noisy < d16, 2, np.where(d16 < -noisy, 0, 1)))
    return dict(b=b, nzsum=nzsum, noisy=noisy, d16=d16, open=is_open, rbx=rbx)


def census(pairs, bw, sc):
    c = dict(noisy=0, held=0, moved=0, stay0_then_move=0, stall_then_one=0, mov0=0, mov1=0, mov2=0)
    for q, t in pairs:
        s = steer(q, t, bw, sc)
        a, op = np.abs(s["d16"]), s["open"]
        c["noisy"] += int((op & (s["noisy"] > 16)).sum())
        c["held"] += int((op & (a > 16) & (a <= s["noisy"])).sum())                      # the band moves by one BECAUSE of noisy
        c["moved"] += int((op & (s["noisy"] > 16) & (a > s["noisy"])).sum())            # rbx is 0 or 2 against a noisy above its floor
        mv = np.diff(np.concatenate([[0], s["b"]]))
        stay = (mv == 0) & (s["b"] > 0)
        c["stay0_then_move"] += int(((mv[:-1] == 0) & (s["b"][:-1] == 0) & (mv[1:] >= 1)).sum())
        c["stall_then_one"] += int((stay[:-1] & (mv[1:] == 1)).sum())
        for k in (0, 1, 2):
            c["mov%d" % k] += int((mv == k).sum())
    return c


def test_steer_is_the_oracles_rule():
    """extend mode moves the band by rbx itself: the numpy restatement predicts every next row's band offset (where the query's end does not cut the move)"""
    n = 0
    for sc in (SC_BENCH, SC_LINEAR, max_gape_scoring()):
        for q, t in corpus()[:8]:
            s = steer(q, t, 128, sc, S.MODE_EXTEND)
            b = s["b"]
            room = b[:-1] + 128 + 2 < len(q)
            assert np.array_equal((b[1:] - b[:-1])[room], s["rbx"][:-1][room]), sc
            n += int(room.sum())
    assert n > 1000


def test_corpus_reaches_the_rows_where_the_noise_sum_decides():
    cases = [("bench", 128, SC_BENCH), ("bench", 256, SC_BENCH), ("linear", 128, SC_LINEAR), ("linear", 256, SC_LINEAR), ("maxgape", 128, max_gape_scoring()),
             ("maxgape", 128, max_gape_scoring(opens=(-1,))), ("two-piece", 128, SC_TWO), ("bench", 64, SC_BENCH)]
    tot = dict(noisy=0, held=0, moved=0)
    for name, bw, sc in cases:
        c = census(corpus(), bw, sc)
        print(name, bw, sc, c)
        for k in tot:
            tot[k] += c[k]
        if name in ("linear", "maxgape") and bw == 128:
            # each of the scorings with |gape| >= 3 meets the conditions on its own at bandwidth 128
            assert c["noisy"] >= 50 and c["held"] >= 10 and c["moved"] >= 10, (name, c)
        assert min(c["mov0"], c["mov1"], c["mov2"]) >= 20, (name, bw, c)
    assert tot["noisy"] >= 50 and tot["held"] >= 10 and tot["moved"] >= 10, tot


def test_corpus_holds_both_sides_of_the_first_cell_mask():
    """rows at rbeg = 0 followed by a row that moves, and stalls at rbeg > 0 directly followed by a move of one: the row behind takes the two-instruction insert
    for cell 0's M flag right after a row that took the saturating form"""
    for bw in (128, 256):
        c = census(corpus(), bw, SC_BENCH)
        assert c["stay0_then_move"] >= len(corpus()) // 2 and c["stall_then_one"] >= 10, (bw, c)
        c = census(plain(), bw, SC_BENCH)
        assert c["stay0_then_move"] >= len(plain()) and c["stall_then_one"] >= 10, (bw, c)


def test_batches_put_both_kinds_first_and_last_in_a_group_of_sixteen():
    c, p = corpus(), plain()
    ids_c, ids_p = {id(q) for q, t in c}, {id(q) for q, t in p}
    for tag, ends, inner in (("rough_ends", ids_c, ids_p), ("plain_ends", ids_p, ids_c)):
        b = batch(tag)
        for k, (q, t) in enumerate(b):
            assert (id(q) in ends) == (k in (0, 15, 16, 31)) and (id(q) in inner) == (k not in (0, 15, 16, 31)), (tag, k)
    for q, t in c:
        assert 1 <= len(t) <= 1000 and len(q) >= 1
