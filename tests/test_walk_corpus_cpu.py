"""The batches of test_walk_corpus_gpu.py hold what they claim (no GPU).  Every fact is read from the oracle's CIGAR words and, for the band,
from oracle_align(..., want_begs=True); which pairs a code walker may decline is read from the oracle's restatement of the code walk.  These are
conditions on the inputs: where a construction misses one, the input changes, not the assertion.

    long_gap, phase_sweep   the planted I and D runs come back as single words of exactly g, nothing else is longer than 3; the largest g per
                            bandwidth is the one walk_cases.GMAX states, the longest spans two code blocks of W cells and the 32-cell window,
                            a deletion run of 65 rows and more exists wherever the band admits one
    tokens                  exactly n gap words; the long D is the stated word counted from the end; adjacent I / D words in both orders
    edges                   a path on a band edge for at least 200 rows; a walk that keeps meeting the first column of the previous row's band
    overhang                leading and trailing runs of 60 and 300; nothing but the named decline list is declined, nothing is untraceable"""
import numpy as np
import pytest

import band_margin_cases as K
import support as S
import walk_cases as W

ONE_PIECE = ("affine", "go4", "linear")
TWO_PIECE = ("twopiece", "twopiece19", "twopiece23")
WHOLE = ("affine", "chk")
ALIGN = [(bw, sc) for bw in (64, 128, 256) for sc in ONE_PIECE + TWO_PIECE] + [(0, sc) for sc in WHOLE]
EDIT = [(bw, "edit") for bw in (64, 128, 256, 0)]


def _gap_words(cig):
    return [(op, ln) for op, ln in W.words(cig) if op in (1, 2)]


def _planted_ok(case, cig):
    """the planted runs as single words of exactly g, every other gap word at most 3"""
    gaps = _gap_words(cig)
    want = [(1, case.info["ins"])] if "ins" in case.info else []
    want += [(2, case.info["dele"])] if "dele" in case.info else []
    rest = list(gaps)
    for w in want:
        if w not in rest:
            return False
        rest.remove(w)
    return all(ln <= 3 for _, ln in rest)


@pytest.mark.parametrize("bw,scname", ALIGN + EDIT)
def test_long_gaps_and_sweeps_come_back_as_single_words(bw, scname):
    kind, g = W.KIND[scname], W.sweep_g(scname, bw)
    group = W.long_gap(bw, scname) + W.phase_sweep(kind, "I", g) + W.phase_sweep(kind, "D", g)
    bad = []
    for c in group:
        res, cig, n, _ = W.oracle(c, W.G, scname, bw)
        if n < 0 or not _planted_ok(c, cig):
            bad.append("%s: %s" % (c.name, n if n < 0 else S.cigar_str(cig)[:120]))
    assert not bad, "%d/%d (%s, bandwidth %d)\n%s" % (len(bad), len(group), scname, bw, "\n".join(bad[:8]))


@pytest.mark.parametrize("bw,scname", ALIGN + EDIT)
def test_largest_run_per_bandwidth(bw, scname):
    gs = [c.info["ins"] for c in W.long_gap(bw, scname)]
    top = W.gmax(scname, bw)
    print("largest g (%s, bandwidth %d): %d; ladder %s" % (scname, bw, top, gs))
    assert max(gs) == top and gs[:3] == [8, 17, 20 if top == 20 else 24]
    if scname in ("affine", "go4") + TWO_PIECE:
        assert top == {64: 40, 128: 70, 256: 150, 0: 300}[bw]
        assert top >= 2 * (bw // 16) + 32              # two code blocks of W cells and the 32-cell window
    if scname == "linear":
        assert top == {64: 40, 128: 70, 256: 130}[bw]
    if scname == "edit":
        assert top == {64: 20, 128: 40, 256: 100, 0: 300}[bw]
    # a tile of 64 rows without a match column: a deletion run of 65 and more wherever the band admits it
    if bw == 0 or (bw >= 128 and scname != "edit") or (bw == 256 and scname == "edit"):
        assert any(g >= 65 for g in gs), gs


def test_sweep_meets_every_tile_phase_and_spans_the_refill_cycle():
    for kind in ("random", "disjoint"):
        for which in ("I", "D"):
            for step in (7, 9):
                pos = [int(c.name.rsplit("@", 1)[1]) for c in W.phase_sweep(kind, which, W.SWEEP_G, step)]
                assert len(pos) == 74 and sorted(p % 64 for p in pos[:64]) == list(range(64))
                assert pos[-1] - pos[0] >= 448 + 56


@pytest.mark.parametrize("bw,scname", [a for a in ALIGN if a[0]] + [(0, "affine")] + EDIT)
def test_token_counts(bw, scname):
    for c in W.tokens():
        res, cig, n, _ = W.oracle(c, W.G, scname, bw)
        gaps = _gap_words(cig)
        assert n >= 0 and len(gaps) == c.info["gaps"], (c.name, scname, bw, len(gaps))
        k = c.info.get("long_from_end")
        if k:
            assert gaps[-k] == (2, W.TOKEN_LONG) and sum(1 for _, ln in gaps if ln > 1) == 1, (c.name, scname, bw, gaps[-k])
        else:
            assert all(ln == 1 for _, ln in gaps), (c.name, scname, bw)
    assert sorted({c.info["gaps"] for c in W.tokens()}) == [62, 63, 64, 65, 127, 128, 129]
    assert {c.info.get("long_from_end") for c in W.tokens() if c.info["gaps"] >= 65} == {None, 63, 64, 65}


@pytest.mark.parametrize("bw,scname", [(bw, sc) for bw in (64, 128, 256, 0) for sc in ("affine", "go4") + TWO_PIECE if (bw, sc) in ALIGN])
def test_adjacent_runs_in_both_orders(bw, scname):
    seen = set()
    for c in W.adjacent(bw):
        res, cig, n, _ = W.oracle(c, W.G, scname, bw)
        ws = W.words(cig)
        pairs = {(a[0], b[0]) for a, b in zip(ws, ws[1:]) if a[0] in (1, 2) and b[0] in (1, 2)}
        assert n >= 0 and c.info["order"] in pairs, (c.name, scname, bw, S.cigar_str(cig)[:80])
        if c.info["order"] == (1, 2):
            assert (1, W.ADJ_G) in ws and (2, W.ADJ_G) in ws and ws[ws.index((1, W.ADJ_G)) + 1] == (2, W.ADJ_G)
        seen.add(c.info["order"])
    assert seen == ({(1, 2), (2, 1)} if bw else {(1, 2)})          # (a whole-query band cuts no cell off: walk_cases.adjacent)


# under a long second piece a deletion run of hundreds of rows costs little and the path leaves the edge at once: no pair with 200 rows was found at
# bandwidth 256 (9 rows at most); the group runs there all the same
EDGE_CLAIMS = [(bw, sc) for bw in (64, 128, 256) for sc in ONE_PIECE + TWO_PIECE if (bw, sc) not in ((256, "twopiece19"), (256, "twopiece23"))]


@pytest.mark.parametrize("bw,scname", EDGE_CLAIMS)
def test_edges_ride_a_band_edge_for_200_rows(bw, scname):
    """... and on those rows the walk keeps meeting the first column of the previous row's band"""
    best, cpm = {}, {}
    for c in W.edges(bw):
        res, cig, n, begs = W.oracle(c, W.G, scname, bw)
        assert n >= 0, (c.name, scname, bw)
        per = W.edge_rows(c, bw, res, cig, begs)
        if per:
            assert min(per.values()) == K.margin_ref(len(c.q), len(c.t), bw, res, cig, begs), c.name          # the same statement of the margin
        best[c.name] = sum(1 for v in per.values() if v == 0)
        cpm[c.name] = len(W.cpm_rows(res, cig, begs))
        if "drift" in c.info:
            gaps = _gap_words(cig)
            assert sum(ln for op, ln in gaps if op == 2) - sum(ln for op, ln in gaps if op == 1) == c.info["drift"]
    print(scname, bw, best, cpm)
    assert max(best.values()) >= 200, (scname, bw, best)
    assert max(cpm.values()) >= 32, (scname, bw, cpm)          # repeatedly: on more rows than a code ring of 32 rows holds


def test_overhangs_give_long_first_and_last_words():
    for c in W.overhang():
        n60 = 60 if c.name.endswith("-60") else 300
        res, cig, n, _ = W.oracle(c, W.G, "affine", 0)
        ws = W.words(cig)
        assert n >= 0 and max(ln for op, ln in ws if op in (1, 2)) >= n60 - 30, (c.name, S.cigar_str(cig)[:60])
    c = [c for c in W.overhang() if c.name == "overhang/q-lead-60"][0]
    assert W.words(W.oracle(c, W.G, "affine", 128)[1])[0] == (1, 60)            # the walk's final emit gets the whole run
    assert W.words(W.oracle(c, W.O, "affine", 128)[1])[0][0] == 0 and W.oracle(c, W.O, "affine", 128)[0][1] == 60       # overlap: clipped, qb = 60


@pytest.mark.parametrize("bw,scname", ALIGN)
def test_nothing_is_untraceable_and_only_the_named_list_is_declined(bw, scname):
    for mode in W.MODES:
        for c in W.cases(bw, scname, mode):
            assert W.oracle(c, mode, scname, bw)[2] != S.ORC_ERR_TRACE, (c.name, mode, scname, bw)
            assert not W.codes_walk_declines(c, mode, scname, bw), (c.name, mode, scname, bw)
    named = {c.name for c in W.decline(bw, scname)}
    for c in W.decline_candidates():
        if bw:
            assert W.codes_walk_declines(c, W.G, scname, bw) == (c.name in named), (c.name, scname, bw)
        if c.name in named:
            assert W.oracle(c, W.G, scname, bw)[2] >= 0, c.name          # the literal traceback answers for it


@pytest.mark.parametrize("bw", [64, 128, 256, 0])
def test_edit_oracle_traces_every_pair(bw):
    for mode in W.MODES:
        for c in W.cases(bw, "edit", mode):
            assert W.oracle(c, mode, "edit", bw)[2] >= 0, (c.name, mode, bw)
