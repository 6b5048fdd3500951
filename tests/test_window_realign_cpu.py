"""No GPU: the Python statement of bsa_window_realign_* (window_realign_cases.window_realign_ref) against both worked examples of
include/bsalign_hip.h typed in byte by byte, the invariants of a re-aligned piece and the unbanded cost on random windows, simulated pieces of a
500-base window, every clause of "liftable" and "re-alignable" violated one at a time, the closed loop of test_window_msa_cpu continued through a
second round, a homopolymer window through both rounds, the arena rule, and the symbols and constants the library must export."""
import os
import re

import numpy as np

import support as S
import window_cns_cases as WC
import window_msa_cases as W
import window_realign_cases as R
import window_stitch_cases as WS
from window_msa_cases import PAR7


def test_the_library_exports_the_calls():
    R.need_symbols()
    import bsalign_amd as B
    assert hasattr(B.lib(), "bsa_window_realign_step_internal")
    names = ("OK", "NO_WINDOW", "BAD_PIECE", "TOO_LONG", "EMPTY_SPAN", "OFF_BAND", "NO_DIAG")
    assert tuple(getattr(B, "REALIGN_ST_" + n) for n in names) == tuple(getattr(R, "ST_" + n) for n in names) == tuple(range(7))
    assert B.REALIGN_ST_EDGE == R.ST_EDGE == 0x100
    import ctypes as C
    assert C.sizeof(B.REALIGN_PARAMS) == 32 and tuple(n for n, _ in B.REALIGN_PARAMS._fields_[:5]) == R.REALIGN_PARAMS_FIELDS
    p = B.realign_params(500)
    assert (p.window2, p.max_len, p.min_margin, p.x, p.g, list(p.reserved)) == (500, 1024, 8, 1, 1, [0, 0, 0])
    assert hasattr(B.Context, "window_realign_run") and hasattr(B.Context, "window_realign")
    text = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    for value, name in enumerate(names):
        assert re.search(r"#define\s+BSA_REALIGN_ST_%s\s+%du\b" % (name, value), text), name
    assert re.search(r"#define\s+BSA_REALIGN_ST_EDGE\s+0x100u\b", text)
    assert "typedef struct { uint32_t window2, max_len, min_margin, x, g, reserved[3]; } bsa_realign_params_t;" in text
    assert "bsa_window_realign_run(" in text and "bsa_window_realign_batch(" in text


def _example(make):
    b, p, want = make()
    r = R.window_realign_ref(b, p, 8)
    assert r.span[0] == (want["u"], want["v"], want["m"], want["margin"])
    assert int(r.cost[0]) == want["cost"] and r.words[0].tolist() == want["words"] and int(r.pstatus[0]) == want["status"]
    assert tuple(int(v) for v in r.piece2[0]) == want["piece2"]
    assert r.doff2.tolist() == [want["doff2"]] and r.dlen2.tolist() == [want["dlen2"]]
    nw = len(want["words"])
    assert r.pcig2_off.tolist() == [0, nw] and r.pcig2[:nw].tolist() == want["words"] and np.all(r.pcig2[nw:] == R.FILL32)
    R.check_piece(b, r, 0, R.round2_batch(b, r, p["window2"]), 0)
    return b, p, r


def test_reference_on_header_example_1():
    b, p, r = _example(R.header_example_1)
    seq, _, _, words = WS.header_example_2()[2][1][:4]          # the stitch block's example 2 at min_cov 1: the same bases and words
    assert b.seq.tolist() == seq and b.cig.tolist() == words


def test_reference_on_header_example_2():
    b, p, r = _example(R.header_example_2)
    s, k = R.lift_tables([(int(w) & 15, int(w) >> 4) for w in b.cig])
    assert k[2] == 0 and k[7] == 0 and s == [0, 1, 2, 2, 2, 3, 4, 5]      # a and b are deleted columns


def test_invariants_on_random_windows():
    """a few hundred windows: a re-aligned piece's words sum to len' and to t_last' - t_first' + 1, begin and end with M, the piece is live under the
    MSA pass's predicate, and the banded cost is the unbanded one wherever the EDGE flag is clear and the margin is at least 8"""
    rng = np.random.default_rng(2718)
    seen, ncmp = set(), 0
    for k in range(240):
        Ld = int(rng.integers(2, 70))
        b = R.make([R.simulated_window(rng, Ld, int(rng.integers(1, 4)), 0.06, 0.05, 0.05, codes_above_3=bool(k & 1))], Ld + int(rng.integers(0, 3)), t_base=k)
        p = R.par(Ld + 16, 128, int(rng.integers(0, 12)), int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        r = R.window_realign_ref(b, p, 10000)
        mb = R.round2_batch(b, r, p["window2"])
        assert int(r.dlen2[0]) == len(b.seq)
        for j in range(b.piece_cap):
            st = int(r.pstatus[j])
            seen.add(st)
            if st & 0xFF:
                assert int(r.piece2[j]["len"]) == 0 and len(r.words[j]) == 0 and W.live_guide(mb, j, int(mb.dlen[0])) is None
                continue
            R.check_piece(b, r, j, mb, 0)
            u, v, m, margin = r.span[j]
            if not st & R.ST_EDGE and margin >= 8:
                bo, n = int(b.piece[j]["base_off"]), int(b.piece[j]["len"])
                full, _, _ = R.banded_dp(b.bases[bo:bo + n], b.seq[u:v + 1], margin, p["x"], p["g"], banded=False)
                assert full == int(r.cost[j]), (k, j, full, int(r.cost[j]))
                ncmp += 1
    assert ncmp >= 200 and R.ST_OK in seen and R.ST_EMPTY_SPAN in seen


def test_simulated_pieces_of_a_500_base_window_are_all_re_aligned():
    """200 reads of a 500-base window at 4 % substitutions, 3 % insertions and 3 % deletions: no piece is left out, none touches the band's edge"""
    rng = np.random.default_rng(500)
    b = R.make([R.simulated_window(rng, 500, 200, whole=True)], 500)
    p = R.par(550, 640, 8, 1, 1)
    r = R.window_realign_ref(b, p, 0)
    assert np.all(r.pstatus == R.ST_OK), np.unique(r.pstatus, return_counts=True)
    d = [abs(r.span[j][2] - int(b.piece[j]["len"])) for j in range(200)]
    assert max(d) <= 40
    mb = R.round2_batch(b, r, 550)
    for j in range(0, 200, 5):
        R.check_piece(b, r, j, mb, 0)
        u, v, m, margin = r.span[j]
        bo, n = int(b.piece[j]["base_off"]), int(b.piece[j]["len"])
        assert R.banded_dp(b.bases[bo:bo + n], b.seq[u:v + 1], margin, 1, 1, banded=False)[0] == int(r.cost[j])
    assert int(r.pcig2_off[-1]) == sum(len(w) for w in r.words) > 200 and len(r.pcig2) == 0      # a count-only reference


def test_each_clause_of_the_liftable_window():
    b, p, names, at = R.bad_windows_batch()
    r = R.window_realign_ref(b, p, 4096)
    for name in names:
        g = at[name]
        assert R.liftable(b, g, p["window2"]) is None, name
        assert int(r.dlen2[g]) == 0 and int(r.doff2[g]) == 0 and np.all(r.pstatus[int(b.piece_off[g]):int(b.piece_off[g + 1])] == R.ST_NO_WINDOW), name
        assert R.liftable(b, g - 1, p["window2"]) is not None, name
        assert np.all(r.pstatus[int(b.piece_off[g - 1]):int(b.piece_off[g])] & 0xFF != R.ST_NO_WINDOW), name
    assert R.liftable(b, at["slen_above_window2"], 41) is not None             # one base more room, and it is liftable
    b.window = 33
    assert R.liftable(b, at["Ld_above_window"], 40) is not None
    batches, p = R.bad_offsets_batches()
    want = {"seq_off_decreases": [True, False, False, True], "seq_behind_seq_cap": [True, True, True, False], "cig_off_decreases": [True, False, False, True],
            "cig_behind_cig_cap": [True, True, True, False]}
    for name, bb in batches.items():
        assert [R.liftable(bb, g, p["window2"]) is not None for g in range(4)] == want[name], name
        r = R.window_realign_ref(bb, p, 4096)
        assert [int(x) > 0 for x in r.dlen2] == want[name]


def test_each_clause_of_the_re_alignable_piece():
    b, p, at, want = R.bad_pieces_batch()
    r = R.window_realign_ref(b, p, 8192)
    for name, st in want.items():
        j = at[name]
        assert int(r.pstatus[j]) == st, (name, int(r.pstatus[j]))
        assert int(r.piece2[j]["len"]) == 0 and len(r.words[j]) == 0 and int(r.cost[j]) == 0
        rest = [n for n in R.PIECE_DTYPE.names if n != "len"]
        assert all(int(r.piece2[j][n]) == int(b.piece[j][n]) for n in rest), name
        assert int(r.pstatus[j - 1]) & 0xFF == 0 and int(r.pstatus[j + 1]) & 0xFF == 0, name
    assert sorted(set(want.values())) == [R.ST_BAD_PIECE, R.ST_TOO_LONG, R.ST_EMPTY_SPAN, R.ST_OFF_BAND]
    # one more code of room, one more unit of margin, one base less: each bound is the last value that passes
    j = at["len_above_max_len"]
    assert int(R.window_realign_ref(b, dict(p, max_len=101), 0).pstatus[j]) != R.ST_TOO_LONG
    j = at["margin_below_min"]
    margin = (63 - abs(int(b.piece[j]["len"]) - 2)) // 2
    assert margin < 12 and int(R.window_realign_ref(b, dict(p, min_margin=margin), 0).pstatus[j]) & 0xFF in (R.ST_OK, R.ST_NO_DIAG)
    batches, p = R.piece_off_batches()
    r = R.window_realign_ref(batches["above_piece_cap"], p, 0)
    assert np.all(r.pstatus[2:] == R.ST_NO_WINDOW) and np.all(r.pstatus[:2] & 0xFF == 0) and np.all(r.dlen2 > 0)
    r = R.window_realign_ref(batches["unclaimed"], p, 0)
    assert int(r.pstatus[0]) == R.ST_NO_WINDOW and int(r.pstatus[6]) == R.ST_NO_WINDOW


def test_no_diag_and_the_scorings():
    sb = R.scoring_batches()
    b, p = sb["x3_g1"]
    r = R.window_realign_ref(b, p, 64)
    assert r.pstatus.tolist() == [R.ST_NO_DIAG, R.ST_OK, R.ST_OK] and r.cost.tolist() == [2, 0, 2] and int(r.piece2[0]["len"]) == 0
    b, p = sb["x1_g255"]
    r = R.window_realign_ref(b, p, 0)
    assert any(int(c) >= 255 for c in r.cost) and all(len(w) == 1 for w, s, pc in zip(r.words, r.pstatus, b.piece) if s == 0 and len(w) and abs(int(pc["t_last"]) - int(pc["t_first"]) + 1 - int(pc["len"])) == 0)
    got = {mm: R.window_realign_ref(*sb["min_margin_%d" % mm], 0).pstatus & 0xFF for mm in (0, 8, 31)}
    assert int((got[0] == R.ST_OFF_BAND).sum()) < int((got[8] == R.ST_OFF_BAND).sum()) < int((got[31] == R.ST_OFF_BAND).sum())


def test_edge_flag_and_the_hand_made_paths():
    b, p = R.shapes_batch()
    r = R.window_realign_ref(b, p, 1 << 16)
    mb = R.round2_batch(b, r, p["window2"])
    st = r.pstatus
    assert int((st == R.ST_EDGE).sum()) >= 4 and int((st == R.ST_OFF_BAND).sum()) >= 4 and int((st == R.ST_OK).sum()) >= 20
    for j in range(b.piece_cap):
        if int(st[j]) & 0xFF == 0:
            R.check_piece(b, r, j, mb, 0)
    P = b.piece_cap
    lead_gaps, trail_gaps, i_ends, d_ends, middle = P - 8, P - 7, P - 6, P - 5, P - 4
    assert int(r.piece2[i_ends]["q_first"]) == int(b.piece[i_ends]["q_first"]) + 7 and int(r.piece2[i_ends]["len"]) == 60 and r.words[i_ends].tolist() == [60 << 4]
    assert int(r.piece2[d_ends]["t_first"]) == 40 + 9 and int(r.piece2[d_ends]["t_last"]) == 40 + 51 and r.words[d_ends].tolist() == [43 << 4]
    assert int(r.cost[middle]) == 30 and sum(int(w) >> 4 for w in r.words[middle] if int(w) & 15 == R.OP_D) == 30      # (which 30 bases: the leftmost that cost no more)
    assert int(st[lead_gaps]) & 0xFF == 0 and int(st[trail_gaps]) & 0xFF == 0 and int(r.piece2[lead_gaps]["t_first"]) > 40
    assert np.array_equal(r.words[P - 2], [60 << 4]) and np.array_equal(r.words[P - 1], [60 << 4]) and int(r.cost[P - 2]) == 0      # codes above 3 are read & 3


def test_offsets_and_the_arena_rule():
    b, p = R.arena_batch()
    full = R.window_realign_ref(b, p, 4096)
    need = int(full.pcig2_off[-1])
    assert need > 12 and np.all(full.pcig2[need:] == R.FILL32) and int(full.pstatus[5]) == R.ST_BAD_PIECE
    cut = int(full.pcig2_off[7]) + 1                                           # pieces 0 .. 6 fit, piece 7 does not
    short = R.window_realign_ref(b, p, cut)
    assert np.array_equal(short.pcig2_off, full.pcig2_off) and np.array_equal(short.pstatus, full.pstatus) and np.array_equal(short.piece2, full.piece2)
    assert np.array_equal(short.pcig2[:cut - 1], full.pcig2[:cut - 1]) and short.pcig2[cut - 1] == R.FILL32
    none = R.window_realign_ref(b, p, 0)
    assert np.array_equal(none.pcig2_off, full.pcig2_off) and len(none.pcig2) == 0 and np.array_equal(none.cost, full.cost)


def test_closed_loop_through_a_second_round():
    """the closed loop of test_window_msa_cpu -- a truth of 2000 bases, a draft with errors, error-free reads -- through the stitch, the re-alignment,
    the MSA, the host consensus and the stitch again: round 2's guides are one M word a piece, mlen == slen, and the sequence is the truth again"""
    truth, draft, ws, b = W.closed_loop()
    st1, cwin1 = R.stitched(b)
    seq1 = st1.seq[:int(st1.seq_off[-1])]
    assert np.array_equal(seq1, truth)
    rb = R.from_round1(b, st1)
    p = R.par(128, 128, 8, 1, 1)
    r = R.window_realign_ref(rb, p, 1 << 16)
    assert np.all(r.pstatus == R.ST_OK) and np.all(r.cost == 0)
    assert all(len(w) == 1 and int(w[0]) & 15 == R.OP_M for w in r.words)
    assert np.array_equal(r.dlen2, st1.rec["slen"]) and np.array_equal(r.doff2, st1.seq_off[:-1])
    mb = R.round2_batch(rb, r, 128)
    for g in range(b.nwin):
        for j in range(int(b.piece_off[g]), int(b.piece_off[g + 1])):
            R.check_piece(rb, r, j, mb, g)
    st2, cwin2 = R.stitched(mb)
    assert np.array_equal(cwin2["mlen"], st1.rec["slen"])                     # no insertion column is left
    assert np.array_equal(st2.seq[:int(st2.seq_off[-1])], truth)
    assert int(st2.rec["x"].sum()) == 0 and int(st2.rec["ins"].sum()) == 0 and int(st2.rec["del"].sum()) == 0      # round 2's words are against round 1's sequence


def test_homopolymer_window_through_both_rounds():
    """the draft lacks one base of a run of six; five error-free reads carry it and their round-1 guides place it at five different columns.  What
    the definitions imply, and all that is asserted: round 1's MSA has five insertion columns with one base each, and after the re-alignment all
    re-aligned rows carry the base in ONE column of round 2's MSA.  What each round calls is printed, not asserted."""
    b, truth, draft = R.homopolymer_window()
    depth, mlen, ins, cols, live = W.window_ref(b, 0)
    assert all(live) and sum(ins) == 5 and mlen == len(draft) + 5
    assert all(int((cols[c, :5] <= 3).sum()) == 1 for c in range(mlen) if cols[c, 5] == 4)          # every insertion column: one read
    st1, _ = R.stitched(b)
    seq1 = st1.seq[:int(st1.seq_off[-1])]
    rb = R.from_round1(b, st1)
    r = R.window_realign_ref(rb, R.par(32, 64, 8, 1, 1), 64)
    assert np.all(r.pstatus == R.ST_OK)
    assert len(set(tuple(w.tolist()) for w in r.words)) == 1                     # every read: the same words
    mb = R.round2_batch(rb, r, 32)
    depth2, mlen2, ins2, cols2, live2 = W.window_ref(mb, 0)
    assert all(live2)
    st2, _ = R.stitched(mb)
    seq2 = st2.seq[:int(st2.seq_off[-1])]
    print("round 1 calls", len(seq1), "bases:", "the truth" if np.array_equal(seq1, truth) else "the draft" if np.array_equal(seq1, draft) else seq1.tolist())
    print("round 2 calls", len(seq2), "bases:", "the truth" if np.array_equal(seq2, truth) else "the draft" if np.array_equal(seq2, draft) else seq2.tolist())
    if len(seq1) == len(truth):
        assert mlen2 == len(seq1) and sum(ins2) == 0             # round 1 called the base: nothing is inserted any more
    else:
        assert sum(ins2) == 1 and mlen2 == len(seq1) + 1         # one insertion column, and every row has its base there
        c = next(c for c in range(mlen2) if cols2[c, 5] == 4)
        assert np.all(cols2[c, :5] == 0)
