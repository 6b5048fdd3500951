"""The random POA programs of tests/poa_random.py on the CPU: the generator keeps its promises, the score guard of bsa_poa_graph_supported /
bsa_poa_graph_gen_supported is sound (inside it the absolute-score statement the device kernels compute equals the reference's lane-exact int8
rows, on random graphs, re-scored recordings, drawn scorings and the guard's boundary), and the reference's own walk ends on all but a few of the
programs the GPU tests send."""
import numpy as np
import pytest

import poa_random as R
import poa_support as P


def test_generator_programs_are_valid_and_branchy():
    """validate() on every program the GPU tests use, and floors on what they contain (over the GPU tests' own seeds), so that the generator cannot
    silently degrade: per narrow set of 64 programs at least 40 nodes with three inputs, 15 with four and 8 with five; programs shorter than the band;
    moved rows, jumps above the band's width, inputs of one merge with different offsets, long branches further back than any ring"""
    alljumps = allbig = 0
    for bw in R.NARROW_BW:
        pgs = R.narrow_set(bw)
        deg = np.zeros(6, np.int64)
        jumps = big = mixed = 0
        for pg in pgs:
            nodes, edges, cands, blocks = R.graph_of(pg)             # (validate() runs inside)
            deg += R.in_degrees(pg)[:6]
            mv = np.concatenate([nodes[j + "_movx"][((nodes[j + "_tk"] & P.IN_PRESENT) != 0) & ((nodes[j + "_tk"] & P.IN_MERGE) == 0)] for j in ("in0", "in1")])
            jumps += int((mv > 2).sum()); big += int((mv > bw).sum())
            both = ((nodes["in0_tk"] & (P.IN_PRESENT | P.IN_MERGE)) == P.IN_PRESENT) & ((nodes["in1_tk"] & (P.IN_PRESENT | P.IN_MERGE)) == P.IN_PRESENT)
            mixed += int((nodes["in0_movx"][both] != nodes["in1_movx"][both]).sum())
            assert set(int(k) for k in cands["kind"]) <= {0, 1} and int(cands[-1]["kind"]) == 0
            assert int(edges["cov"].min()) >= 1 and int(edges["cov"].max()) <= 4
        assert deg[3] >= 40 and deg[4] >= 15 and deg[5] >= 8, (bw, deg)
        assert sum(pg["slen"] < bw for pg in pgs) >= 3 or bw == 16, bw
        assert mixed >= 20, (bw, mixed)
        alljumps += jumps; allbig += big
        assert any(int(c["kind"]) == 1 for pg in pgs for c in R.graph_of(pg)[2])
        longs = [pg for pg in pgs if pg["long_branch"]]
        assert len(longs) >= 8 and all(R.max_input_distance(pg) > 32 for pg in longs), bw
    assert alljumps >= 20 and allbig >= 1, (alljumps, allbig)          # (jumps are rare on purpose: a row that jumped ahead of the read loses the walk)
    for bw, nn, c in R.WIDE:
        for v in (0, 1):
            pg = R.wide_program(bw, nn, v)
            R.graph_of(pg)
            assert pg["slen"] >= bw and R.max_input_distance(pg) > 32 and R.in_degrees(pg)[3:].sum() >= 5
            assert (bw + 1023) // 1024 <= c and ((bw + 1023) // 1024 > c // 2 or c == 1)
            assert len(set(int(x) for x in R.graph_of(pg)[0]["rpos"])) > 10            # rows move


def test_boundary_list_is_classified_as_stated():
    """the library's verdict on every boundary scoring is the one the list states (so that the list keeps one scoring on each side of every term
    that can bind); the by-one scorings of the width term are k_poa_gen's"""
    for b in R.BOUNDARY:
        bw = b.get("bw", 128)
        got = R.wf_supported(b["sc"], bw) > 0
        assert got == b["inside"], (b["term"], b["side"], R.sc_str(b["sc"]), bw, got)
        if b["inside"] or b.get("gen"):
            assert R.gen_supported(b["sc"], bw) == 1
        if not b["inside"] and not b.get("gen"):
            assert R.gen_supported(b["sc"], bw) == 0 and R.gen_supported(b["sc"], 4096) == 0, (b["term"], R.sc_str(b["sc"]))
    for term in set(b["term"] for b in R.BOUNDARY):
        assert any(b["inside"] for b in R.BOUNDARY if b["term"] == term) and (term == "gape1<=gape2" or any(not b["inside"] for b in R.BOUNDARY if b["term"] == term))


def _inside_scorings():
    """every drawn scoring that k_poa_gen's guard takes (the score part of both guards) and every boundary scoring on the inside"""
    out = [("boundary %s %s" % (b["term"], b["side"]), b["sc"], b.get("bw")) for b in R.BOUNDARY if b["inside"] or b.get("gen")]
    out += [("drawn %d" % k, sc, None) for k, sc in enumerate(R.drawn()[:120]) if R.gen_supported(sc, 128) == 1]
    return out


def test_guard_soundness_absolute_scores_are_the_lane_exact_rows():
    """Inside the guard nothing in the reference's int8 arithmetic clamps: for every in-guard scoring drawn and every boundary scoring on the
    inside, orc_wf_forward -> wf_rows_to_blocks equals orc_sweep_run's blocks byte for byte over the used part of every real block, and orc_wf_best
    is the lane-exact best end cell -- on random programs of every bandwidth and on the recorded programs of poa_sweep.npz re-scored (same tasks,
    new parameters).  The classification is the library's (bsa_poa_graph_gen_supported: the score terms both guards share)."""
    golden = [(case["par"]["alnmode"], pg) for case in P.load_golden() for pg in case["programs"] if pg["bandwidth"] <= 256 and len(pg["tasks"]) > 8]
    scs = _inside_scorings()
    assert len(scs) >= 40 and len(golden) >= 30
    n = 0
    for k, (name, sc, only_bw) in enumerate(scs):
        for j in range(10):
            bw = only_bw if only_bw else R.NARROW_BW[(k + j) % len(R.NARROW_BW)]          # (a width-bound scoring runs at its own width)
            pg = R.narrow_set(bw)[(7 * k + 3 * j) % R.NARROW_N]
            mode = (k + j) % 3
            assert R.gen_supported(sc, bw, mode) == 1
            R.lane_exact_check(pg, R.full_par(sc, mode), "%s, random program seed %d index %d mode %d" % (name, pg["seed"], pg["index"], mode))
            n += 1
        for j in range(6):
            mode, pg = golden[(5 * k + j) % len(golden)]
            if R.gen_supported(sc, pg["bandwidth"], mode) != 1:
                continue
            R.lane_exact_check(pg, R.full_par(sc, mode), "%s, recorded program %d re-scored" % (name, (5 * k + j) % len(golden)), recorded=True)
            n += 1
    assert n >= 600, n


def test_guard_soundness_on_the_wide_programs():
    """the same on one branching program per cells-a-thread class of k_poa_gen (bands of 704 ... 18 000 columns), at a boundary scoring"""
    for i, (bw, nn, c) in enumerate(R.WIDE):
        pw = i % 3
        sc = R.scorings_for(pw, bw, wide=True)[0]
        R.lane_exact_check(R.wide_program(bw, nn, 0), R.full_par(sc, (i + 1) % 3), "wide %d" % bw)


def test_the_references_walk_ends_on_all_but_a_few_programs():
    """orc_wf_trace returns n < 0 where the reference's own walk does not end.  Over the exact programs, scorings and modes the GPU tests send, at
    most 5 % of the programs of one parameter set may do so (those are compared by their status alone); no other program is left out of anything."""
    worst = (0.0, None)
    for pw, bw, mode, sc in R.narrow_cases():
        p = R.full_par(sc, mode)
        pgs = R.narrow_set(bw)
        bad = [pg["index"] for pg in pgs if R.oracle_run(pg, p)["n"] < 0]
        frac = len(bad) / len(pgs)
        if frac > worst[0]:
            worst = (frac, (pw, bw, mode, R.sc_str(sc), bad))
        assert frac <= 0.05, (pw, bw, mode, R.sc_str(sc), bad)
    print("largest share of walks that do not end: %.3f %r" % worst)


@pytest.mark.parametrize("pw", [0, 1, 2])
def test_the_references_walk_ends_on_the_wide_programs(pw):
    """the wide programs are one per parameter set: every walk has to end"""
    for pw_, bw, nn, c, mode, sc, variant in R.wide_cases():
        if pw_ != pw:
            continue
        assert R.oracle_run(R.wide_program(bw, nn, variant), R.full_par(sc, mode))["n"] > 0, (pw, bw, mode, R.sc_str(sc))


def test_regression_head_seed_below_a_byte_is_refused():
    """R.REGRESSION: scorings with m + 2 n <= 128 that the guard used to take.  The two statements of the oracle differ there (the reference's seed of
    band cell 0 over the head's row wraps in its byte lane), so the kernels' absolute scores are not the reference's: both guards refuse them now"""
    pg = R.narrow_set(176)[27]
    for sc in R.REGRESSION:
        assert R.gen_supported(sc, 176) == 0 and R.wf_supported(sc, 176) == 0 and R.gen_supported(sc, 4096) == 0, R.sc_str(sc)
        with pytest.raises(AssertionError, match="differs from the lane-exact rows"):
            R.lane_exact_check(pg, R.full_par(sc, 0), "regression")


def test_regression_vertical_difference_over_the_head_is_refused():
    """R.REGRESSION_VERTICAL: large match scores without an open cost, inside the guard until these tests; the lane-exact rows saturate over the head"""
    pg = R.narrow_set(16)[45]
    for sc in R.REGRESSION_VERTICAL:
        assert R.gen_supported(sc, 16) == 0 and R.wf_supported(sc, 16) == 0 and R.gen_supported(sc, 4096) == 0, R.sc_str(sc)
        with pytest.raises(AssertionError, match="differs from the lane-exact rows"):
            R.lane_exact_check(pg, R.full_par(sc, 1), "regression")


def test_the_references_walk_on_the_named_programs():
    """the programs single GPU tests send besides the sets above (poa_random: group_programs, program_272, program_lds, the sets behind a declined
    k_poa_wf, program_dead): every single program's walk has to end, of a set of 64 all but 5 %; program_dead has no best end cell at all"""
    sc = R.scorings_for(2, 704, wide=True)[1]
    for pg in R.group_programs():
        assert R.oracle_run(pg, R.full_par(sc, 1))["n"] > 0, pg["index"]
    assert R.oracle_run(R.program_272(), R.full_par(R.BOUNDARY[0]["sc"], 2))["n"] > 0
    assert R.oracle_run(R.program_lds(), R.full_par(R.BOUNDARY[0]["sc"], 1))["n"] > 0
    for b in R.BOUNDARY:
        if b.get("gen"):
            bad = [pg["index"] for pg in R.narrow_set(b["bw"]) if R.oracle_run(pg, R.full_par(b["sc"], 1))["n"] < 0]
            assert len(bad) <= 0.05 * R.NARROW_N, (b["bw"], bad)
    pg = R.program_dead()
    o = R.oracle_run(pg, R.full_par(R.DEAD_SC, R.DEAD_MODE))
    assert o["best"][1] < 0 and o["best"][0] <= -(1 << 29) + 1 and o["n"] < 0, o["best"]
    assert R.wf_supported(R.DEAD_SC, 96, pg["slen"], R.DEAD_MODE) > 0


def test_terms_that_cannot_bind():
    """what the comment at poa_random.BOUNDARY works out, by brute force over the library's own answers: inside the guard n + m + g stays at or below 86
    (65 with an open cost), so n + m + g <= 100 and min(X, -g) - 1 - m - g >= -100 never decide"""
    top = {0: 0, 1: 0}
    for M in range(0, 70, 1):
        for X in range(0, -70, -1):
            for O, E in ((0, 0), (0, -1), (0, -3), (-1, 0), (-1, -1), (-4, -2), (-10, -4)):
                sc = R._sc(M, X, 0, O, E)
                if R.gen_supported(sc, 128) == 1:
                    m, n, g = M + 1, -X, -O - E
                    top[int(O != 0)] = max(top[int(O != 0)], n + m + g)
                    assert min(X, -g) - 1 - m - g >= -100
    assert top == {0: 86, 1: 65}, top
