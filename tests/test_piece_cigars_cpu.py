"""CPU: bsa_piece_cigars_* (include/bsalign_hip.h) without a GPU -- the Python statement of the definition (piece_cigars_cases.piece_cigars_ref)
against the header's worked example typed in by hand and against what the definition implies on random alignments, bsa_piece_cigars_bound against
the reference's totals on the pieces the two earlier passes' references make, and the exported symbols."""
import numpy as np

import cigar_windows_cases as CW
import piece_cigars_cases as P
import support as S
import window_pieces_cases as WP


def _need():
    """every test here is about bsa_piece_cigars_*: without its symbols in the library none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in ("bsa_piece_cigars_run", "bsa_piece_cigars_batch", "bsa_piece_cigars_bound"):
        assert hasattr(B.lib(), name), "the library does not export " + name


def test_header_example():
    _need()
    batch, off, ws, status = P.header_example()
    got = P.piece_cigars_ref(*P.build(batch))
    assert np.array_equal(got[0], off), got[0]
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], ws), got[1]
    assert np.array_equal(got[2], status), got[2]
    # the refmode guides of the three windows of 10
    guides = [P.refmode_guide(got[1][int(off[j]):int(off[j + 1])], int(batch[2][j][3]), int(batch[2][j][4]), 10, 10 * (j + 1)) for j in range(3)]
    assert guides[0].tolist() == CW.words((7, CW.D), (3, CW.M)).tolist()
    assert guides[1].tolist() == CW.words((2, CW.M), (2, CW.I), (4, CW.D), (4, CW.M)).tolist()
    assert guides[2].tolist() == CW.words((2, CW.M), (8, CW.D)).tolist()
    for g in guides:
        assert P.sums(g)[1] == 10                              # a guide covers its window of the backbone
    # the example is in the header as it is here
    text = open(S.ROOT + "/include/bsalign_hip.h").read()
    for s in ("tb = 7, qb = 3, words 5M 2I 4D 6M, cut at w = 10 into the pieces", "{q_first 3, len 3, t 7..9}    -> 3M", "{q_first 6, len 8, t 10..19}  -> 2M 2I 4D 4M",
              "{q_first 14, len 2, t 20..21} -> 2M", "pcig_off = {0, 1, 5, 6}, status 0 0 0", "{q_first 6, len 3, t 10..12} is not on the path",
              "{q_first 7, len 7, t 10..19} (t 10 aligns with q 6)", "window [0, 10): 7D 3M", "window [20, 30): 2M 8D", "#define BSA_PIECE_ST_NOT_ON_PATH 1u"):
        assert s in text, s


def _check_consequences(ws, pc, what):
    """what the definition implies for the words of a cut piece"""
    assert len(ws) >= 1, what
    ops, lens = ws & np.uint32(15), ws >> np.uint32(4)
    assert int(ops[0]) in P.DIAG and int(ops[-1]) in P.DIAG, what                 # the first and the last word are diagonal
    assert np.all(lens > 0) and all(int(o) in P.STEPS for o in ops), what          # nothing empty, nothing that takes no step
    qn, tn = P.sums(ws)
    assert qn & P.M32 == int(pc["len"]), what
    assert tn == int(pc["t_last"]) - int(pc["t_first"]) + 1, what


def test_consequences_on_random_alignments():
    _need()
    rng = np.random.default_rng(31337)
    cut = lost = 0
    for trial in range(60):
        eqx = bool(trial & 1)
        cig = CW.random_words(rng, int(rng.integers(1, 180)), maxlen=int(rng.integers(1, 14)), eqx=eqx)
        rec = CW.record(int(rng.integers(0, 1000)), int(rng.integers(0, 1000)), cig)
        cols = P.columns(rec, cig)
        ps = []
        for _ in range(12):
            if cols and rng.integers(4):
                i, j = sorted(int(x) for x in rng.integers(0, len(cols), 2))
                ps.append(P.piece(0, cols[i], cols[j]))
            else:                                              # anything: mostly not on the path
                t = int(rec[3]) + int(rng.integers(0, 400))
                ps.append((0, int(rec[1]) + int(rng.integers(0, 400)), int(rng.integers(0, 50)), t, t + int(rng.integers(0, 50))))
        args = P.build(([rec], [cig], ps))
        off, ws, status = P.piece_cigars_ref(*args)
        assert int(off[-1]) == len(ws)
        on = set((c[0], c[1]) for c in cols)
        for j, pc in enumerate(args[3]):
            mine = ws[int(off[j]):int(off[j + 1])]
            first = (int(pc["t_first"]), int(pc["q_first"]))
            last = (int(pc["t_last"]), (int(pc["q_first"]) + int(pc["len"]) - 1) & P.M32)
            want = int(pc["len"]) >= 1 and first[0] <= last[0] and first in on and last in on
            assert (int(status[j]) == 0) == want, (trial, j, pc)
            if want:
                cut += 1
                _check_consequences(mine, pc, (trial, j))
                # the words replayed from the first column arrive at the last, and are the pair's words unit for unit
                units = "".join("MIDNSHP=X"[int(w) & 15] * (int(w) >> 4) for w in cig if (int(w) & 15) in P.STEPS)
                got = "".join("MIDNSHP=X"[int(w) & 15] * (int(w) >> 4) for w in mine)
                assert got in units, (trial, j)
            else:
                lost += 1
                assert len(mine) == 0 and int(status[j]) == P.NOT_ON_PATH, (trial, j)
    assert cut > 300 and lost > 100


def test_nothing_is_merged_and_nothing_empty_is_kept():
    _need()
    cig = CW.words((3, CW.M), (4, CW.M), (0, CW.I), (2, CW.S), (5, CW.M), (2, CW.D), (2, CW.D), (1, CW.M))
    args = P.build(([CW.record(0, 0, cig)], [cig], [(0, 1, 12, 1, 16), (0, 3, 4, 3, 6), (0, 4, 5, 4, 8)]))
    off, ws, status = P.piece_cigars_ref(*args)
    assert status.tolist() == [0, 0, 0] and off.tolist() == [0, 6, 7, 9]
    assert ws.tolist() == CW.words((2, CW.M), (4, CW.M), (5, CW.M), (2, CW.D), (2, CW.D), (1, CW.M), (4, CW.M), (3, CW.M), (2, CW.M)).tolist()


def _windowed(rng, npairs, w, eqx):
    """random pairs through the references of the two earlier passes -> (records, words, the pieces in window-major order)"""
    recs, cigs = zip(*[CW.random_pair(rng, int(rng.integers(0, 200)), maxlen=int(rng.integers(1, 30)), eqx=eqx) for _ in range(npairs)])
    wins = [CW.windows_ref(r, c, w) for r, c in zip(recs, cigs)]
    woff = np.zeros(npairs + 1, dtype=np.uint64)
    woff[1:] = np.cumsum([len(x) for x in wins], dtype=np.uint64)
    qlen = np.array([r[1] + CW.spans(c)[0] for r, c in zip(recs, cigs)], dtype=np.uint32)
    qoff = np.zeros(npairs, dtype=np.uint64)
    qoff[1:] = np.cumsum(qlen[:-1], dtype=np.uint64)
    seqs = np.zeros(int(qlen.sum()), dtype=np.uint8)
    nwin = max((int(r[4]) + w - 1) // w for r in recs) + 1
    poff, boff, pieces, codes = WP.pieces_ref(seqs, qoff, qlen, np.concatenate(wins), woff, w, np.zeros(npairs, np.uint64), nwin, 0)
    return list(recs), list(cigs), pieces, poff


def test_bound_and_the_pieces_of_the_two_earlier_passes():
    """on what the references of bsa_cigar_windows and bsa_window_pieces make, every piece is cut, the consequences hold, and the bound suffices"""
    _need()
    import bsalign_amd as B
    rng = np.random.default_rng(8)
    for w, eqx in ((1, False), (3, True), (10, False), (64, True), (500, False)):
        recs, cigs, pieces, poff = _windowed(rng, 25, w, eqx)
        arena, coff = CW.flatten(cigs)
        assert len(pieces) > 25 or w == 500
        off, ws, status = P.piece_cigars_ref(CW.to_struct(recs), arena, coff, pieces)
        assert np.all(status == 0), w
        for j, pc in enumerate(pieces):
            _check_consequences(ws[int(off[j]):int(off[j + 1])], pc, (w, j))
        bound = B.piece_cigars_bound(coff, len(pieces))
        assert bound == len(arena) + len(pieces) and int(off[-1]) <= bound, (w, int(off[-1]), bound)
    # the bound counts the words the offsets speak of, wherever they start
    assert B.piece_cigars_bound(np.array([40, 50, 50, 75], np.uint64), 9) == 35 + 9
    assert B.piece_cigars_bound(np.array([7], np.uint64), 3) == 3 and B.piece_cigars_bound(np.zeros(0, np.uint64), 0) == 0
    assert B.lib().bsa_piece_cigars_bound(None, 5, 2) == 2


def test_hand_made_batches_hold_what_they_are_for():
    _need()
    c = P.hand_batches()
    recs, cigs, ps = c["tile_sizes"]
    assert [len(x) for x in cigs] == list(P.TILE_WORDS)
    args = P.build(c["tile_sizes"])
    off, ws, status = P.piece_cigars_ref(*args)
    pairs = args[3]["pair"]
    assert np.any(np.diff(pairs.astype(np.int64)) < 0), "the pieces are not pair-major"
    assert status[pairs == 0].tolist() == [1] and np.all(status[pairs != 0] == 0)
    # where the pieces' first and last columns lie
    first, last, spans, cache = set(), set(), set(), {}
    for j, pc in enumerate(args[3]):
        k = int(pc["pair"])
        if k == 0:
            continue
        if k not in cache:
            cache[k] = {(c_[0], c_[1]): c_ for c_ in P.columns(recs[k], cigs[k])}
            cache[k, "words"] = sorted(set(c_[2] for c_ in cache[k].values()))
        cols, nd = cache[k], cache[k, "words"]
        a = cols[(int(pc["t_first"]), int(pc["q_first"]))]
        b = cols[(int(pc["t_last"]), (int(pc["q_first"]) + int(pc["len"]) - 1) & P.M32)]
        la, lb = int(cigs[k][a[2]]) >> 4, int(cigs[k][b[2]]) >> 4
        for (wi, u, ln), into in (((a[2], a[3], la), first), ((b[2], b[3], lb), last)):
            into.add("first unit" if u == 0 else "last unit" if u == ln - 1 else "inside")
            into.add("lane %d" % (wi % 64) if wi % 64 in (0, 63) else "mid tile")
            if wi == nd[0]:
                into.add("first word")
            if wi == nd[-1]:
                into.add("last word")
        if a[2] == b[2]:
            spans.add("one word")
        spans.add("%d tiles" % min(b[2] // 64 - a[2] // 64 + 1, 3))
    need = {"first unit", "last unit", "inside", "lane 0", "lane 63", "mid tile", "first word", "last word"}
    assert need <= first and need <= last, (need - first, need - last)
    assert {"one word", "1 tiles", "2 tiles", "3 tiles"} <= spans
    # the other batches: what is cut and what is not
    st = lambda name: P.piece_cigars_ref(*P.build(c[name]))[2].tolist()
    assert st("gaps_inside_the_borders") == [0] * 6 and st("deletion_over_a_window") == [0, 0, 0, 0, 0] and st("eqx_words") == [0] * 5
    assert st("no_step_and_empty_words") == [0] * 7 and st("words_behind_te") == [0, 0, 0]
    assert st("pairs_without_an_alignment") == [1, 0, 1, 0, 1, 0] and st("no_pairs") == [1, 1] and st("no_pieces") == []
    assert st("long_words") == [0, 0, 0, 0, 0, 1]
    off, ws, status = P.piece_cigars_ref(*P.build(c["gaps_inside_the_borders"]))
    assert ws[:int(off[3])].tolist() == CW.words((1, CW.M), (2, CW.I), (1, CW.M), (1, CW.M), (2, CW.D), (1, CW.M), (1, CW.M), (1, CW.I), (1, CW.D), (1, CW.M)).tolist()
    off, ws, status = P.piece_cigars_ref(*P.build(c["deletion_over_a_window"]))
    assert ws[int(off[3]):int(off[4])].tolist() == CW.words((3, CW.M), (25, CW.D), (3, CW.M)).tolist()
    batch, names = P.not_on_path_batch()
    off, ws, status = P.piece_cigars_ref(*P.build(batch))
    assert status.tolist() == [1, 0] * len(names) and len(names) == 13
    off, ws, status = P.piece_cigars_ref(*P.build(P.arena_batch()))
    assert len(status) == 40 and int((status == 1).sum()) == 5 and int(off[-1]) > 100


def test_symbols_are_exported():
    _need()
    import bsalign_amd as B
    lib = B.lib()
    for name in ("bsa_piece_cigars_run", "bsa_piece_cigars_batch", "bsa_piece_cigars_bound"):
        assert hasattr(lib, name), name
    assert B.PIECE_ST_NOT_ON_PATH == P.NOT_ON_PATH == 1
    assert callable(B.Context.piece_cigars) and callable(B.Context.piece_cigars_run) and callable(B.piece_cigars_bound)
