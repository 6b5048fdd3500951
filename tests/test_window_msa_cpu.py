"""CPU: bsa_window_msa_* (include/bsalign_hip.h) without a GPU -- the Python statement of the definition (window_msa_cases.window_msa_ref) against
the header's worked example typed in by hand, against what the definition implies on random windows made by the references of the three passes
before it, with every clause of the live predicate violated one at a time, and with the loop closed by the host consensus caller: the windows'
consensus strings, concatenated, are the truth the draft was made from.  The host-only helpers (window_drafts, window_msa_bound) as well."""
import numpy as np

import cigar_windows_cases as CW
import window_msa_cases as W

PAR7 = W.PAR7


def _need():
    """every test here is about bsa_window_msa_*: without its symbols in the library none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in ("bsa_window_msa_run", "bsa_window_msa_batch", "bsa_window_msa_bound"):
        assert hasattr(B.lib(), name), "the library does not export " + name


def test_header_example():
    _need()
    b, want = W.header_example()
    assert len(want) == 72
    for vote in (0, 1):
        off, cwin, cols = W.window_msa_ref(b, vote)
        assert off.tolist() == [0, 72] and np.array_equal(cols, want)
        assert cwin[0].tolist() == (0, W.NO_IDXS, 0, 3, 2 + vote, 2 + vote, 12)
    depth, mlen, ins, cols, live = W.window_ref(b, 0)
    assert (depth, mlen, ins, live) == (2, 12, [0, 0, 0, 0, 2, 0, 0, 0, 0, 0], [True, True])
    assert cols[:, 0].tolist() == [0, 1, 2, 3, 2, 2, 0, 1, 2, 3, 0, 1] and cols[:, 1].tolist() == [5, 5, 2, 3, 1, 4, 4, 1, 2, 3, 5, 5]
    assert cols[:, 2].tolist() == [0, 1, 2, 3, 4, 4, 0, 1, 2, 3, 0, 1]


def check_consequences(b, g, what):
    depth, mlen, ins, cols, live = W.window_ref(b, g)
    L = min(int(b.dlen[g]), b.window)
    assert mlen == L + sum(ins) and cols.shape == (mlen, depth + 4), what
    c = np.arange(L) + np.cumsum(ins) if L else np.zeros(0, np.int64)
    drow = cols[:, depth]
    o = int(b.doff[g])
    assert np.array_equal(drow[drow != 4], b.draft[o:o + L] & 3) and np.array_equal(np.flatnonzero(drow != 4), c), what
    assert np.all(cols[:, depth + 1] == 4) and np.all(cols[:, depth + 2:] == 0), what
    x = int(b.piece_off[g])
    for r in range(depth):
        row, pc = cols[:, r], b.piece[x + r]
        assert not np.any(row == 6), what
        if not live[r]:
            assert np.all(row == 5), (what, r)
            continue
        bo = int(pc["base_off"])
        assert np.array_equal(row[row < 4], b.bases[bo:bo + int(pc["len"])] & 3), (what, r)
        at = np.flatnonzero(row < 4)
        assert not np.any(row[at[0]:at[-1] + 1] == 5), (what, r)
        a = int(pc["t_first"]) % b.window
        assert np.all(row[:c[a]] == 5) and np.all(row[c[a + int(pc["t_last"]) - int(pc["t_first"])] + 1:] == 5), (what, r)
    inscol = np.setdiff1d(np.arange(mlen), c)
    if depth:
        assert np.all((cols[inscol, :depth] < 4).sum(axis=1) >= 1), (what, "an insertion column without a base")
    else:
        assert len(inscol) == 0
    return sum(live)


def test_random_windows_through_the_three_references():
    _need()
    rng = np.random.default_rng(17)
    seen_ins = 0
    for w, eqx in ((1, False), (3, True), (10, False), (64, True), (500, False)):
        b, status = W.through_the_references(rng, 20, w, eqx)
        assert np.all(status == 0) and len(b.piece) >= 20
        nlive = 0
        for g in range(b.nwin):
            nlive += check_consequences(b, g, (w, g))
            seen_ins += sum(W.window_ref(b, g)[2])
        assert nlive == len(b.piece), w                      # every piece of a complete chain is live
        off, cwin, cols = W.window_msa_ref(b, 1)
        assert int(off[-1]) == len(cols) == int((cwin["mlen"].astype(np.int64) * (cwin["nall"] + 3)).sum())
        assert np.array_equal(cwin["out_off"], np.concatenate([[0], np.cumsum(cwin["mlen"].astype(np.uint64))[:-1]]).astype(np.uint64))
        assert np.all(cwin["nseq"] == cwin["nall"]) and np.all(cwin["nmax"] == cwin["nall"]) and np.all(cwin["idxs_off"] == W.NO_IDXS)
    assert seen_ins > 100


def test_every_clause_of_the_live_predicate():
    _need()
    b, names, at = W.dead_batch()
    depth, mlen, ins, cols, live = W.window_ref(b, 0)
    assert depth == 2 * len(names) + 1 and live == [r % 2 == 0 for r in range(depth)]
    assert ins == [0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0] and mlen == 14          # as if the dead pieces, which insert 5 in front of column 4, were absent
    for name in names:
        assert np.all(cols[:, at[name]] == 5), name
    # each of them is live without its violation: the same pieces with the clause restored
    fixed, _, _ = W.dead_batch()
    j = at["len_0"]
    fixed.piece[j]["len"] = 11
    assert W.live_guide(fixed, j, 12) is not None and W.live_guide(b, j, 12) is None
    j = at["b_at_L"]
    assert W.live_guide(b, j, 13) is not None and W.live_guide(b, j, 12) is None
    for name, bb in W.dead_offsets_batches().items():
        dead = 0 if name == "offsets_decrease" else 1
        for g in (0, 1):
            d, m, i_, cc, lv = W.window_ref(bb, g)
            assert lv == [g != dead] and (np.all(cc[:, 0] == 5) if g == dead else np.any(cc[:, 0] < 4)), (name, g)
            assert sum(i_) == (0 if g == dead or g == 0 else 1), (name, g)
    for name, bb in W.piece_off_batches().items():
        depths = [W.window_ref(bb, g)[0] for g in range(3)]
        assert depths == ([2, 0, 0] if name == "above_piece_cap" else [5, 0, 4]), name


def test_hand_made_batches_hold_what_they_are_for():
    _need()
    c = W.hand_batches()
    assert [W.window_ref(c["depths"], g)[0] for g in range(len(W.DEPTHS))] == list(W.DEPTHS)
    assert sorted(set(int(x) % 32 for x in c["draft_offsets"].doff)) == list(range(32))
    b = c["window_500"]
    x = int(b.piece_off[3])
    assert [int(b.pcig_off[x + r + 1] - b.pcig_off[x + r]) for r in range(len(W.GUIDE_WORDS))] == list(W.GUIDE_WORDS)
    assert all(W.window_ref(b, 3)[4])
    b = c["shapes"]
    assert W.window_ref(b, 0)[2][15] == 3 and W.window_ref(b, 1)[2][4] == 3 and W.window_ref(b, 5)[2][5:8] == [3, 0, 1]
    assert all(all(W.window_ref(b, g)[4]) for g in range(b.nwin))
    assert np.any(b.bases > 3)
    d = c["draft_lengths"]
    assert [min(int(x), 16) for x in d.dlen] == [1, 15, 16, 16, 0, 0, 7] and int(d.dlen[3]) == 40
    assert W.window_ref(d, 5)[:2] == (1, 0) and W.window_ref(d, 5)[4] == [False]
    assert c["no_windows"].nwin == 0 and W.window_msa_ref(c["no_windows"])[0].tolist() == [0]


def test_window_drafts_and_bound():
    _need()
    import bsalign_amd as B
    doff, dlen = B.window_drafts([0, 1000, 5000], [120, 50, 0], 50)
    assert doff.tolist() == [0, 50, 100, 1000] and dlen.tolist() == [120, 70, 20, 50] and doff.dtype == np.uint64 and dlen.dtype == np.uint32
    gbase, nwin = B.window_gbase([0, 1, 1], [120, 50, 0], 50)
    assert nwin == len(doff) and gbase.tolist() == [0, 3, 3]
    assert B.window_msa_bound(np.array([0, 2, 5], np.uint64), 10, 7) == 10 * 6 + 10 * 7 + 7 * 7
    assert B.window_msa_bound(np.zeros(1, np.uint64), 10, 7) == 0 and B.lib().bsa_window_msa_bound(None, 3, 10, 7) == 0
    assert B.window_msa_bound(np.array([0, 1 << 40], np.uint64), 4096, 1 << 63) == (1 << 64) - 1          # saturates
    # it suffices on the pieces of one chain
    rng = np.random.default_rng(23)
    for w in (3, 10, 64):
        b, status = W.through_the_references(rng, 20, w, False)
        units = int(sum(int(x) >> 4 for x in b.pcig if int(x) & 15 == CW.I))
        need = int(W.window_msa_ref(b)[0][-1])
        assert 0 < need <= B.window_msa_bound(b.piece_off, w, units), w
    assert B.CNS_WINDOW_DTYPE == W.CNS_WINDOW_DTYPE and B.CNS_WINDOW_DTYPE.itemsize == 40
    assert callable(B.Context.window_msa) and callable(B.Context.window_msa_run)


def test_consensus_of_error_free_reads_is_the_truth():
    """the loop closed on the host: truth -> draft with edits -> the reads' guides against the draft -> MSA -> bsa_msa_call_consensus"""
    _need()
    import bsalign_amd.msa as MSA
    truth, draft, ws, b = W.closed_loop()
    assert not np.array_equal(truth[:len(draft)], draft[:len(truth)])
    off, cwin, cols = W.window_msa_ref(b, 0)
    out = []
    for g in range(b.nwin):
        rec = cwin[g]
        assert int(rec["nall"]) == 5 and int(rec["nseq"]) == 4
        mine = cols[int(off[g]):int(off[g + 1])].copy()
        rows = mine.reshape(int(rec["mlen"]), 8)[:, :4]
        assert np.all(rows == rows[:, :1]), g                  # the piece rows are unanimous
        cns, qlt, alt, score = MSA.call_consensus(mine, None, int(rec["nall"]), int(rec["nseq"]), int(rec["nmax"]), int(rec["mlen"]), PAR7)
        out.append(cns)
    assert np.array_equal(np.concatenate(out), truth)
