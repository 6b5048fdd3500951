"""CPU: bsa_window_pieces_* (include/bsalign_hip.h) without a GPU -- the Python statement of the definition (window_pieces_cases.pieces_ref)
against the header's worked example typed in by hand, window_gbase, the exported symbols and the record's layout."""
import ctypes as C

import numpy as np
import pytest

import support as S
import window_pieces_cases as P


def test_header_example():
    args, piece_off, base_off, recs, codes = P.header_example()
    got = P.pieces_ref(*args)
    assert np.array_equal(got[0], piece_off) and np.array_equal(got[1], base_off)
    assert got[2].dtype == P.PIECE_DTYPE and np.array_equal(got[2], recs), got[2]
    assert got[3].dtype == np.uint8 and np.array_equal(got[3], codes), got[3]
    # the example is in the header as it is here
    text = open(S.ROOT + "/include/bsalign_hip.h").read()
    for s in ("piece_off = {0, 1, 3, 5}, base_off = {0, 3, 10, 17}", "{pair 1, q_first 3, len 4, t 8..11, base_off 13}  codes 2 2 3 3", "{5, 0, 7, 2}  {8, 3, 11, 6}",
              "bases = 0 1 2 | 3 0 1 2 0 1 1 | 3 0 1 2 2 3 3", "stored AACCGGT (0 0 1 1 2 2 3), qlen 7, marked: q' = ACCGGTT (0 1 1 2 2 3 3)"):
        assert s in text, s


def test_header_example_without_the_strand_flag_and_packed():
    """the same reads: packed words give the same pieces; without BSA_MODE_QSTRAND pair 1 is read forward"""
    import bsalign_amd as B
    (seqs, qoff, qlen, win, win_off, w, gbase, nwin, flags), piece_off, base_off, recs, codes = P.header_example()
    got = P.pieces_ref(B.pack2bit(seqs), qoff, qlen, win, win_off, w, gbase, nwin, flags | P.SEQ2BIT)
    assert np.array_equal(got[2], recs) and np.array_equal(got[3], codes)
    got = P.pieces_ref(seqs, qoff & np.uint64(~P.REVCOMP & (2 ** 64 - 1)), qlen, win, win_off, w, gbase, nwin, 0)
    assert np.array_equal(got[2], recs) and got[3].tolist() == [0, 1, 2, 3, 0, 1, 2, 0, 0, 1, 3, 0, 1, 1, 2, 2, 3]


def test_reference_on_a_reverse_complement_made_on_the_host():
    """every piece of every hand-made case is q'[q_first : q_first + len) of a reverse complement made with numpy, in all the flag sets"""
    import bsalign_amd as B
    for name, case in P.hand_cases().items():
        if name in ("deep_5000", "thousand_pairs"):
            continue
        want = {}
        for flags in case.flag_sets():
            args = P.build(case, flags)
            poff, boff, recs, codes = P.pieces_ref(*args)
            assert int(poff[-1]) == len(recs) and int(boff[-1]) == len(codes) == int(recs["len"].sum()), name
            for r in recs:
                k = int(r["pair"])
                q = case.reads[k] & 3
                if flags & P.QSTRAND and case.marks[k]:
                    q = B.revcomp(q)
                a, b = int(r["q_first"]), int(r["base_off"])
                assert np.array_equal(codes[b:b + int(r["len"])], q[a:a + int(r["len"])]), (name, flags, k)
            key = flags & P.QSTRAND                              # packing changes nothing
            if key not in want:
                want[key] = (recs, codes)
            else:
                assert np.array_equal(want[key][0], recs) and np.array_equal(want[key][1], codes), (name, flags)


def test_window_gbase():
    import bsalign_amd as B
    gb, nwin = B.window_gbase([0, 0, 1, 2, 1], [12, 9, 1], 4)
    assert gb.dtype == np.uint64 and gb.tolist() == [0, 0, 3, 6, 3] and nwin == 7            # 3, 3 and 1 windows
    gb, nwin = B.window_gbase([2, 0], [1000, 0, 1001], 500)
    assert gb.tolist() == [2, 0] and nwin == 5                                               # a target without bases has no window
    gb, nwin = B.window_gbase([], [], 500)
    assert len(gb) == 0 and nwin == 0
    gb, nwin = B.window_gbase([1, 1], [0xFFFFFFFF, 7], 1)
    assert gb.tolist() == [0xFFFFFFFF] * 2 and nwin == 0xFFFFFFFF + 7
    rng = np.random.default_rng(5)
    tl = rng.integers(0, 30000, 200)
    tid = rng.integers(0, 200, 1000)
    for w in (1, 7, 500, 29999, 1 << 20):
        gb, nwin = B.window_gbase(tid, tl, w)
        per = [-(-int(x) // w) for x in tl]
        assert nwin == sum(per) and gb.tolist() == [sum(per[:int(t)]) for t in tid], w
    with pytest.raises(ValueError):
        B.window_gbase([0], [5], 0)


def test_symbols_and_layout():
    import bsalign_amd as B
    lib = C.CDLL(B.LIB_PATH)
    assert hasattr(lib, "bsa_window_pieces_run") and hasattr(lib, "bsa_window_pieces_batch")
    assert B.PIECE_DTYPE.itemsize == 32 and B.PIECE_DTYPE == P.PIECE_DTYPE
    assert B.PIECE_DTYPE.names == ("pair", "q_first", "len", "t_first", "t_last", "reserved", "base_off")
    assert [B.PIECE_DTYPE.fields[n][1] for n in B.PIECE_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24]
