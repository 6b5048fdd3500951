"""The batches of test_align8_pair_shift_gpu.py hold the rows they are meant to hold (no GPU: band offsets and moves from the oracle, test_align8_rare_rows_cpu.moves).

x_forward_abs (bsa_align8_x.hip) shifts the slots of a row that stays (Hp[k] <- Hp[k - 1], E likewise) and, once per cell beyond one, of a row that moves by two and
more (Hp[k] <- Hp[k + 1]) two slots an instruction, in the lanes of the pairs that need it.  What can go wrong is the hand-over of a slot between the two registers
of a pair, between lanes, at the band's two ends, and between the two shifts when they follow each other; so the batches are, on targets of 600 rows:
    stalls    benchmark pairs of 600 bases: rows that stay at rbeg = 0 (the first rows) and at rbeg > 0, the odd move of two
    twos      queries of 1500 bases: moves of two and of three on nearly every row (the shift towards lower slots runs once and twice)
    stall2    queries of 1000 bases: moves of two on half the rows, and rows that stay at rbeg > 0 with a move of two on the very next row
    both      stalls with its pairs 0, 15, 16 and 31 -- the first and last of a group of sixteen -- replaced by a twos and a stall2 pair
Row segments of 64 rows begin on a row that stays at rbeg > 0 (stalls), on a move of two (twos, stall2) and on a move of three (twos): the pending move crosses the
hand-over.  Global mode, the benchmark's scoring, bandwidth 128 and 256."""
import numpy as np

import support as S
import test_align8_rare_rows_cpu as R

ROWS = 600
_CACHE = {}


def batch(tag):
    """the batches by name; built once, shared with the GPU test and never changed"""
    if tag in _CACHE:
        return _CACHE[tag]
    if tag == "stalls":
        pairs = [S.synth_pair(k, ROWS) for k in range(32)]
    elif tag == "twos":
        pairs = [(q, t[:ROWS].copy()) for q, t in (S.synth_pair(k, 1500) for k in range(16))]
    elif tag == "stall2":
        pairs = [(q[:1000].copy(), t[:ROWS].copy()) for q, t in (S.synth_pair(k, 1500) for k in range(16))]
    elif tag == "both":
        pairs = list(batch("stalls"))
        pairs[0], pairs[15], pairs[16], pairs[31] = batch("twos")[0], batch("stall2")[1], batch("stall2")[3], batch("twos")[1]
    else:
        raise KeyError(tag)
    _CACHE[tag] = pairs
    return pairs


def census(pairs, bw):
    c = dict(stay0=0, stay=0, two=0, three=0, top=0, stall_then_two=0, seg_stall=0, seg_two=0, seg_three=0)
    for q, t in pairs:
        b, mv, n = R.moves(q, t, bw)
        assert len(mv) == ROWS
        stay = (mv == 0) & (b > 0)
        c["stay0"] += int(((mv == 0) & (b == 0)).sum())
        c["stay"] += int(stay.sum())
        c["two"] += int((mv == 2).sum())
        c["three"] += int(((mv >= 3) & (mv < bw)).sum())
        c["top"] = max(c["top"], int(mv.max()))
        c["stall_then_two"] += int((stay[:-1] & (mv[1:] == 2)).sum())
        first = np.arange(64, ROWS, 64)          # a segment's first row
        c["seg_stall"] += int(stay[first].sum())
        c["seg_two"] += int((mv[first] == 2).sum())
        c["seg_three"] += int((mv[first] == 3).sum())
    return c


def test_stalls():
    for bw in (128, 256):
        c = census(batch("stalls"), bw)
        print(bw, c)
        assert c["stay0"] >= 32 * 30 and c["stay"] >= 32 * 80 and c["two"] >= 20 and c["top"] == 2, c
        assert c["seg_stall"] >= 32, c          # a stall first in a segment, in every pair


def test_twos():
    for bw, three in ((128, 1000), (256, 100)):
        c = census(batch("twos"), bw)
        print(bw, c)
        assert c["two"] >= 16 * 400 and c["three"] >= three and c["top"] == 3, c
        assert c["seg_two"] >= 16 and c["seg_three"] >= (16 if bw == 128 else 0), c


def test_stall2():
    for bw in (128, 256):
        c = census(batch("stall2"), bw)
        print(bw, c)
        assert c["two"] >= 16 * 200 and c["stay"] >= 40 and c["stall_then_two"] >= 8 and c["top"] == 2, c
        assert c["seg_two"] >= 16, c


def test_both_kinds_in_each_group_of_sixteen():
    both, stalls = batch("both"), batch("stalls")
    assert len(both) == 32
    for k, (q, t) in enumerate(both):
        if k in (0, 15, 16, 31):
            b, mv, n = R.moves(q, t)
            assert (mv == 2).sum() >= 200, k
        else:
            assert q is stalls[k][0] and t is stalls[k][1]
    for bw in (128, 256):
        assert census([both[1]], bw)["stay"] >= 80 and census([both[15]], bw)["stall_then_two"] + census([both[16]], bw)["stall_then_two"] >= 1
