"""The batches of test_align8_rare_rows_gpu.py hold the rows they are meant to hold (no GPU: the oracle with want_begs = True gives every row's band offset, and a
row's move is the difference to the row before it; row 0 has offset 0 and move 0).

x_forward_abs (bsa_align8_x.hip) treats a row whose band does not move by exactly one cell in blocks behind wave-level branches: a constant form of the flag
fix-up while every live pair of the wave moved by at most two, the general loop beside a move of three and more, a shortcut of the first-cell rule while every
such row of the wave stays at rbeg > 0, the rule itself beside a jump or a row at rbeg = 0, with the two values of the rbeg = 0 fix-up formed only in a wave that
has such a row.  A GPU test of those paths proves nothing unless its inputs reach them:
    only2   32 benchmark pairs of 1200 bases: moves of 0, 1 and 2 only, stalls at rbeg = 0 and at rbeg > 0: the constant form alone runs
    rush    long query, short target: moves of two and of three in the thousands: the general loop
    stay    short query, long target: most rows stay at rbeg > 0
    jump    ~1970 bases against 8: moves >= the bandwidth, the score is SCORE_MIN and the oracle reports no traceback (the pair is flagged on the device)
    mixed   only2 with every fourth pair replaced in turn by a rush, stay or jump pair: waves hold both kinds
Global mode, the benchmark's scoring, bandwidth 128 unless said otherwise.

A row that stays at rbeg > 0 BEHIND a jump in the same pair was searched for and does not exist in this family: see test_no_stall_follows_a_jump."""
import numpy as np

import support as S

SC = (2, -6, -3, -2, 0, 0)
_CACHE = {}


def batch(tag):
    """the batches by name; built once, shared with the GPU test and never changed"""
    if tag in _CACHE:
        return _CACHE[tag]
    if tag == "only2":
        pairs = [S.synth_pair(k, 1200) for k in range(32)]
    elif tag == "rush":
        pairs = [(q, t[:600]) for q, t in (S.synth_pair(k, 1500) for k in range(8))]
    elif tag == "stay":
        pairs = [(q[:600], t) for q, t in (S.synth_pair(k, 1500) for k in range(8))]
    elif tag == "jump":
        pairs = [(q, t[:8]) for q, t in (S.synth_pair(k, 2000) for k in range(4))]
    elif tag == "rsj":
        pairs = batch("rush") + batch("stay") + batch("jump")
    elif tag == "mixed":
        pairs = list(batch("only2"))
        others = [batch("rush"), batch("stay"), batch("jump")]
        for n, k in enumerate(range(0, len(pairs), 4)):
            src = others[n % 3]
            pairs[k] = src[(n // 3) % len(src)]
    elif tag == "all":
        pairs = batch("only2") + batch("rsj") + batch("mixed")
    else:
        raise KeyError(tag)
    _CACHE[tag] = pairs
    return pairs


def moves(q, t, bw=128, mode=S.MODE_GLOBAL):
    """(band offset, move) of every row, and the oracle's return value"""
    res, cig, n, begs = S.oracle_align(q, t, mode, bw, *SC, want_begs=True)
    b = begs[:len(t)].astype(np.int64)
    return b, np.diff(np.concatenate([[0], b])), n


def _count(pairs, bw=128):
    c = dict(stay0=0, stay=0, one=0, two=0, three=0, jump=0, top=0, untraced=0)
    for q, t in pairs:
        b, mv, n = moves(q, t, bw)
        c["stay0"] += int(((mv == 0) & (b == 0)).sum())
        c["stay"] += int(((mv == 0) & (b > 0)).sum())
        c["one"] += int((mv == 1).sum())
        c["two"] += int((mv == 2).sum())
        c["three"] += int(((mv >= 3) & (mv < bw)).sum())
        c["jump"] += int((mv >= bw).sum())
        c["top"] = max(c["top"], int(mv.max()))
        c["untraced"] += int(n == S.ORC_ERR_TRACE)
    return c


def test_only2_never_moves_by_three():
    c = _count(batch("only2"))
    print(c)
    assert len(batch("only2")) == 32
    assert c["top"] == 2 and c["three"] == 0 and c["jump"] == 0, c
    assert c["two"] >= 50 and c["stay"] >= 1000 and c["stay0"] >= 300, c
    # bandwidth 256: the same classes
    c = _count(batch("only2"), 256)
    print(c)
    assert c["top"] == 2 and c["two"] >= 50 and c["stay"] >= 1000 and c["stay0"] >= 300, c


def test_rush_moves_by_two_and_by_three():
    c = _count(batch("rush"))
    print(c)
    assert len(batch("rush")) == 8 and c["two"] >= 1000 and c["three"] >= 1000, c
    c = _count(batch("rush"), 256)
    print(c)
    assert c["two"] >= 1000 and c["three"] >= 100, c


def test_stay_mostly_stays_behind_the_first_column():
    for bw in (128, 256):
        c = _count(batch("stay"), bw)
        print(c)
        rows = sum(len(t) for q, t in batch("stay"))
        assert len(batch("stay")) == 8 and 2 * c["stay"] > rows, (c, rows)


def test_jump_jumps_and_is_not_traced():
    c = _count(batch("jump"))
    print(c)
    assert len(batch("jump")) == 4
    assert all(1900 <= len(q) <= 2040 and len(t) == 8 for q, t in batch("jump"))
    assert c["jump"] >= 4 and c["stay0"] >= 4, c
    for q, t in batch("jump"):
        res, cig, n = S.oracle_align(q, t, S.MODE_GLOBAL, 128, *SC)
        assert n == S.ORC_ERR_TRACE, (res, n)
        assert -(0x7FFFFFFF >> 2) <= res[0] <= -(0x7FFFFFFF >> 2) + 4, res          # SCORE_MIN, at most a match above it
    # bandwidth 256: moves far above two, the general loop
    c = _count(batch("jump"), 256)
    print(c)
    assert c["three"] + c["jump"] >= 4, c


def test_mixed_puts_both_kinds_into_most_groups_of_sixteen():
    """every fourth pair is a rush, stay or jump pair in turn, so any sixteen pairs that a wave may be given hold moves of three and more beside pairs that never
    move by more than two, whatever order the plan puts them in (length-sorted orders included: eight of the thirty-two are replaced, three kinds)"""
    mixed, only2 = batch("mixed"), batch("only2")
    assert len(mixed) == 32
    kinds = []
    for k, (q, t) in enumerate(mixed):
        if k % 4:
            assert q is only2[k][0] and t is only2[k][1]
            kinds.append("only2")
        else:
            b, mv, n = moves(q, t)
            kinds.append("big" if mv.max() >= 3 else "small")
    assert kinds.count("big") >= 5 and kinds.count("only2") == 24, kinds
    for w in (0, 16):
        assert "big" in kinds[w:w + 16] and "only2" in kinds[w:w + 16], kinds


def test_no_stall_follows_a_jump():
    """A row with mov = 0 at rbeg > 0 behind a row with mov >= BW in the same pair would be the input that a shortcut of the first-cell rule for stalled rows must not
    get wrong (after a jump the row is rebuilt from SCORE_MIN).  None exists among targets of 2 .. 64 and some longer rows against queries of 400 .. 1970 bases,
    and the steering says why: only the rush of global mode moves by more than three, it sets mov = 1 + (cells still to go) / (rows left), which keeps the band on
    pace to reach the query's end on the last row, and a stall at rbeg > 0 needs the band at the query's end with rows to spare, i.e. a pace below two cells a row;
    from one row to the next the pace falls by about 1 / (rows left).  The kernel does not rest on this: a lane takes the shortcut only under its own test that
    the row's score lies far above SCORE_MIN, and a wave with a lane that fails it takes the rule as it stands.  The search stays as the record of why no batch
    of the GPU test holds such a row."""
    q, t = S.synth_pair(0, 2000)
    found = []
    for tl in list(range(2, 65, 3)) + [100, 200, 300]:
        for ql in (400, 1000, 1970):
            b, mv, n = moves(q[:ql], t[:tl])
            j = np.flatnonzero(mv >= 128)
            if len(j) and ((mv[j[0]:] == 0) & (b[j[0]:] > 0)).any():
                found.append((tl, ql))
    assert not found, found
