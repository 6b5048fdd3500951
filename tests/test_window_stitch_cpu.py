"""No GPU: the Python statement of bsa_window_stitch_* (window_stitch_cases.window_stitch_ref) against both worked examples of include/bsalign_hip.h
typed in byte by byte, the invariants and the word walker on random windows, the consensus pass's own compaction at min_cov 0, the closed loop with a
coverage hole on the HOST consensus caller, the readable record clause by clause, the arena rule, and the symbols the library must export."""
import os
import re

import numpy as np

import support as S
import window_cns_cases as WC
import window_msa_cases as W
import window_stitch_cases as WS
from window_msa_cases import CNS_WINDOW_DTYPE, NO_IDXS, PAR7


def test_the_library_exports_the_calls():
    WS.need_symbols()
    import bsalign_amd as B
    assert hasattr(B.lib(), "bsa_window_stitch_step_internal")
    assert (B.STITCH_ST_CALLED, B.STITCH_ST_DRAFT, B.STITCH_ST_BAD_RECORD) == (WS.ST_CALLED, WS.ST_DRAFT, WS.ST_BAD_RECORD) == (0, 1, 2)
    assert B.STITCH_DTYPE == WS.STITCH_DTYPE and B.STITCH_DTYPE.itemsize == 32
    assert hasattr(B.Context, "window_stitch_run") and hasattr(B.Context, "window_stitch")
    text = open(os.path.join(S.ROOT, "include", "bsalign_hip.h")).read()
    for name, value in (("CALLED", 0), ("DRAFT", 1), ("BAD_RECORD", 2)):
        assert re.search(r"#define\s+BSA_STITCH_ST_%s\s+%du\b" % (name, value), text), name
    assert "typedef struct { uint32_t status, slen, eq, x, ins, del, kept, ncig; } bsa_stitch_t;" in text
    assert "bsa_window_stitch_run(" in text and "bsa_window_stitch_batch(" in text


def _one(cols, rec, cst, min_cov):
    r = WS.window_stitch_ref(cols, rec, len(cols), cst, min_cov, 64, 64)
    WS.check_invariants(r, 0)
    return r


def test_reference_on_header_example_1():
    cols, rec, want = WS.header_example_1()
    for key, (seq, qlt, words, eq, x, ins, dl, kept) in want.items():
        r = _one(cols, rec, np.array([2], np.uint32) if key == "draft" else None, 0 if key == "draft" else key)
        got = r.rec[0]
        assert got.tolist() == (WS.ST_DRAFT if key == "draft" else WS.ST_CALLED, len(seq), eq, x, ins, dl, kept, len(words)), (key, got)
        assert r.win[0][0].tolist() == seq and r.win[0][1].tolist() == qlt and r.win[0][2].tolist() == [0] * len(seq) and r.win[0][3].tolist() == words, key
        assert r.seq[:len(seq)].tolist() == seq and r.seq[len(seq)] == WS.FILL and r.cig[:len(words)].tolist() == words and r.cig[len(words)] == WS.FILL32
        assert r.seq_off.tolist() == [0, len(seq)] and r.cig_off.tolist() == [0, len(words)]
        assert WS.cigar_apply(r.win[0][4], r.win[0][0], r.win[0][3]) == (eq, x, ins, dl)


def test_header_example_1_is_what_the_host_caller_leaves():
    """the called and the quality bytes of example 1 are the host consensus caller's at the default rates, and so is the window without any piece"""
    from bsalign_amd import msa as MSA
    cols, rec, want = WS.header_example_1()
    mine = cols.reshape(10, 5).copy()
    mine[:, 2:] = [4, 0, 0]
    mine = mine.reshape(-1)
    cns, qlt, alt, _ = MSA.call_consensus(mine, None, 2, 1, 1, 10, PAR7)
    assert np.array_equal(mine, cols) and cns.tolist() == want[0][0] and qlt.tolist() == want[0][1]
    bare = np.array([[b, 4, 0, 0] for b in (0, 1, 2, 3, 0, 1, 2, 3, 0, 1)], dtype=np.uint8).reshape(-1)
    cns, _, _, _ = MSA.call_consensus(bare, None, 1, 0, 0, 10, PAR7)
    assert len(cns) == 0 and np.all(bare.reshape(10, 4)[:, 1] == 4)                  # every draft base gone ...
    rec1 = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    rec1[0] = (0, NO_IDXS, 0, 1, 0, 0, 10)
    r = _one(bare, rec1, None, 1)
    assert r.win[0][0].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1] and r.rec[0]["kept"] == 10 and r.win[0][3].tolist() == [10 << 4 | WS.OP_EQ]      # ... and kept here


def test_reference_on_header_example_2():
    cols, rec, want = WS.header_example_2()
    ccols, crec, cns, qlt, alt, called = WC.header_example_cns()
    assert np.array_equal(cols.reshape(12, 6)[:, :3], ccols.reshape(12, 6)[:, :3]) and np.array_equal(cols.reshape(12, 6)[:, 3:].T, called)
    for min_cov, (seq, q, a, words, ins, kept) in want.items():
        r = _one(cols, rec, None, min_cov)
        assert r.win[0][0].tolist() == seq and r.win[0][1].tolist() == q and r.win[0][2].tolist() == a and r.win[0][3].tolist() == words, min_cov
        assert int(r.rec[0]["ins"]) == ins and int(r.rec[0]["kept"]) == kept and int(r.rec[0]["slen"]) == len(seq), min_cov
    r = _one(cols, rec, None, 0)                               # what the consensus pass packs
    assert np.array_equal(r.win[0][0], cns) and np.array_equal(r.win[0][1], qlt) and np.array_equal(r.win[0][2], alt)


def test_invariants_and_the_word_walker_on_random_windows():
    rng = np.random.default_rng(88)
    seen = set()
    for k in range(300):
        nall, mlen = int(rng.integers(1, 9)), int(rng.integers(0, 90))
        blob, rec = WS.make_batch([WS.random_msa(rng, nall, mlen, odd_codes=bool(k & 1))])
        cst = None if k % 3 else np.array([k % 4], np.uint32)
        r = WS.window_stitch_ref(blob, rec, len(blob), cst, int(rng.integers(0, nall + 1)), mlen, mlen)      # the sum of mlen suffices for both caps
        WS.check_invariants(r, 0)
        seq, _, _, words, dr = r.win[0]
        assert WS.cigar_apply(dr, seq, words) == tuple(int(r.rec[0][n]) for n in ("eq", "x", "ins", "del"))
        assert np.all(seq <= 3) and np.array_equal(r.seq[:len(seq)], seq) and np.array_equal(r.cig[:len(words)], words)
        seen |= set(int(w) & 15 for w in words)
    assert seen == {WS.OP_I, WS.OP_D, WS.OP_EQ, WS.OP_X}


def test_min_cov_0_is_the_compaction_of_the_consensus_pass():
    """on columns the host caller filled: the stitch at min_cov 0 and window_cns_ref's compact arrays are the same bytes at the same offsets"""
    blob, rec = WC.arena_batch()
    out_cap = int(rec["mlen"].sum())
    full = WC.window_cns_ref(blob, rec, len(blob), out_cap, out_cap, 65, PAR7)
    assert np.all(full.status == 0)
    r = WS.window_stitch_ref(full.cols, rec, len(blob), None, 0, out_cap, out_cap)
    assert np.all(r.rec["status"] == 0) and np.array_equal(r.seq_off, full.seq_off)
    need = int(full.seq_off[-1])
    assert need > 0 and np.array_equal(r.seq[:need], full.seq[:need]) and np.array_equal(r.seq_qlt[:need], full.seq_qlt[:need])
    assert np.array_equal(r.seq_alt[:need], full.seq_alt[:need]) and np.all(r.rec["kept"] == 0)


def test_closed_loop_with_a_coverage_hole():
    """three windows without reads and one covered in its first 15 columns only; vote 0, the consensus bytes from the host caller: the stitch at
    min_cov 1 is the truth where a read covers and the draft where none does; the consensus pass's compaction of the same columns is shorter"""
    truth, draft, b, want = WS.closed_loop_with_hole()
    off, cwin, cols = W.window_msa_ref(b, 0)
    assert np.all(cwin["nall"] == 5) and np.all(cwin["nseq"] == 4)
    out_cap = int(cwin["mlen"].sum())
    cns = WC.window_cns_ref(cols, cwin, len(cols), out_cap, out_cap, 4, PAR7)
    assert np.all(cns.status == 0)
    for g in WS.HOLES:
        assert cns.clen[g] == 0                                  # the hole, as the consensus pass packs it
    assert cns.clen[WS.PART] == WS.PART_COLS
    r = WS.window_stitch_ref(cns.cols, cwin, len(cols), cns.status, 1, out_cap, out_cap)
    got = r.seq[:int(r.seq_off[-1])]
    lost = sum(int(cwin[g]["mlen"]) for g in WS.HOLES) + int(cwin[WS.PART]["mlen"]) - WS.PART_COLS
    assert np.array_equal(got, want) and not np.array_equal(got, truth) and not np.array_equal(got, draft)
    assert int(cns.seq_off[-1]) == len(got) - lost and lost == 385
    assert int(r.rec["kept"].sum()) == lost and np.all(r.rec["kept"][[g for g in range(b.nwin) if g not in WS.HOLES + (WS.PART,)]] == 0)
    for g in range(b.nwin):
        WS.check_invariants(r, g)
        WS.cigar_apply(r.win[g][4], r.win[g][0], r.win[g][3])
    assert int(r.rec["x"].sum()) > 0 and int(r.rec["ins"].sum()) > 0 and int(r.rec["del"].sum()) > 0          # what the polish changed
    # the draft's own words, window by window, lead from the draft to the stitched sequence
    d = np.concatenate([w[4] for w in r.win])
    assert np.array_equal(d, draft)


def _rec(**kw):
    w = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    w[0] = (64, NO_IDXS, 10, 5, 5, 4, 7)                     # 7 columns of 8 bytes at 64
    for k, v in kw.items():
        w[0][k] = v
    return w[0]


def test_each_clause_of_the_readable_record():
    cap = 64 + 56
    assert WS.readable(_rec(), cap) and not WS.readable(_rec(), cap - 1)
    assert not WS.readable(_rec(idxs_off=0), cap) and not WS.readable(_rec(nall=0), cap)
    assert WS.readable(_rec(nseq=99, nmax=77), cap)            # nseq and nmax are not looked at
    assert not WS.readable(_rec(mlen=1 << 28, cols_off=0), 1 << 62) and WS.readable(_rec(mlen=(1 << 28) - 1, cols_off=0), 1 << 62)
    assert not WS.readable(_rec(cols_off=(1 << 64) - 56), (1 << 64) - 1) and WS.readable(_rec(cols_off=(1 << 64) - 57), (1 << 64) - 1)
    assert WS.readable(_rec(mlen=0, cols_off=cap), cap) and not WS.readable(_rec(mlen=0, cols_off=cap + 1), cap)
    assert not WS.readable(_rec(nall=0xFFFFFFFF, mlen=1, cols_off=0), (1 << 32) + 1) and WS.readable(_rec(nall=0xFFFFFFFF, mlen=1, cols_off=0), (1 << 32) + 2)
    blob, rec, cols_cap, cst, want, names = WS.bad_batch()
    r = WS.window_stitch_ref(blob, rec, cols_cap, cst, 1, 0, 0)
    assert r.rec["status"].tolist() == want and want[0::2] == [0] * 9 and sorted(set(want)) == [0, 1, 2]
    bad = np.array(want) == WS.ST_BAD_RECORD
    for name in ("slen", "eq", "x", "ins", "del", "kept", "ncig"):
        assert np.all(r.rec[name][bad] == 0)
    draft = np.flatnonzero(np.array(want) == WS.ST_DRAFT)
    assert np.all(r.rec["ncig"][draft] <= 1) and np.array_equal(r.rec["kept"][draft], r.rec["slen"][draft])


def test_offsets_and_the_arena_rule():
    blob, rec, cst = WS.arena_batch()
    total = int(rec["mlen"].sum())
    full = WS.window_stitch_ref(blob, rec, len(blob), cst, 1, total, total)
    ns, nc = int(full.seq_off[-1]), int(full.cig_off[-1])
    assert 0 < ns <= total and 0 < nc <= total and full.rec["slen"][3] == 0 and full.rec["status"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert np.all(full.seq[ns:] == WS.FILL) and np.all(full.cig[nc:] == WS.FILL32) and np.all(full.seq[:ns] <= 3)
    cut_s, cut_c = int(full.seq_off[5]) + 1, int(full.cig_off[2])           # the arenas are independent: bases of windows 0 .. 4, words of windows 0 .. 1
    short = WS.window_stitch_ref(blob, rec, len(blob), cst, 1, cut_s, cut_c)
    assert np.array_equal(short.seq_off, full.seq_off) and np.array_equal(short.cig_off, full.cig_off) and np.array_equal(short.rec, full.rec)
    assert np.array_equal(short.seq[:cut_s - 1], full.seq[:cut_s - 1]) and short.seq[cut_s - 1] == WS.FILL and np.array_equal(short.cig, full.cig[:cut_c])
    none = WS.window_stitch_ref(blob, rec, len(blob), cst, 1, 0, 0)
    assert np.array_equal(none.seq_off, full.seq_off) and len(none.seq) == 0 and len(none.cig) == 0


def test_the_batches_are_what_they_say():
    mb = WS.mixed_batches()
    assert sorted(int(x) for x in set(mb["mlen_200"][1]["nall"])) == sorted(WS.NALLS) and len(mb) == len(WS.MLENS) + 5
    assert WS.TILE_64_NALL in WS.NALLS and WS.TILE_64_NALL + 1 in WS.NALLS                      # just below and just above the 64-column tile
    assert mb["by_rows"][1]["nall"].tolist() == [WS.TILE_1_NALL, WS.TILE_1_NALL + 1, 3, WS.TILE_1_NALL + 1] and np.all(mb["by_rows"][1]["mlen"] == 70)
    blob, rec, _ = mb["hand_made"]
    r = WS.window_stitch_ref(blob, rec, len(blob), None, 1, len(blob), len(blob))
    assert r.win[0][3].tolist() == [200 << 4 | WS.OP_EQ] and r.win[2][3].tolist() == [1 << 4 | op for op in (WS.OP_EQ, WS.OP_X, WS.OP_I, WS.OP_D)] * 50
    assert int(r.rec[6]["ncig"]) == 0 and int(r.rec[6]["slen"]) == 0 and r.win[5][3].tolist() == [66 << 4 | WS.OP_EQ]
    firsts = set((int(w[3][0]) & 15, int(w[3][-1]) & 15) for w in r.win[7:23])
    assert len(firsts) == 16
    blob, rec, _ = mb["overlapping"]
    assert int(rec["mlen"].sum()) > len(blob) // 4
