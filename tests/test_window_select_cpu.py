"""CPU: the definition of bsa_window_select_* as window_select_cases states it -- the header's example typed in, mix32 and its inverse, the properties
of a selection on random windows, every clause of the candidate test on its border -- and what of the feature needs no GPU: the exported symbols, the
parameter structure's layout and the Python plumbing's size checks."""
import ctypes as C

import numpy as np
import pytest

import window_select_cases as W
from window_select_cases import M32, Par


def test_header_example_and_both_seeds():
    piece, off, want = W.header_example()
    assert sorted(want) == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 2)]
    for (seed, md), idx in want.items():
        ref = W.window_select_ref(piece, off, len(piece), None, Par(max_depth=md, min_span=6, seed=seed))
        assert ref.win[0].tolist() == idx and int(ref.ncand[0]) == 5 and ref.sel_off.tolist() == [0, len(idx)], (seed, md)
        assert ref.src.tolist() == idx and np.array_equal(ref.sel, piece[idx])
    # the order among the three pieces of 10 columns, as the header states it: j0, j4, j2
    h = {j: W.mix32(int(piece[j]["pair"])) for j in (0, 2, 4)}
    assert sorted(h, key=h.get) == [0, 4, 2]


def test_mix32_values_of_the_header():
    import bsalign_amd as B
    for x, h in W.HEADER_MIX32.items():
        assert W.mix32(x) == h and B.mix32(x) == h
    rng = np.random.default_rng(31)
    for x in [0, 1, M32, 1 << 31] + [int(v) for v in rng.integers(0, 1 << 32, 200)]:
        assert B.mix32(x) == W.mix32(x) and 0 <= W.mix32(x) <= M32


def test_unmix32_inverts_mix32():
    rng = np.random.default_rng(32)
    for x in list(range(70)) + [M32, M32 - 1, 1 << 31, (1 << 31) - 1] + [int(v) for v in rng.integers(0, 1 << 32, 2000)]:
        assert W.unmix32(W.mix32(x)) == x and W.mix32(W.unmix32(x)) == x
    # so a case can ask for any key
    for key in (0, (1 << 64) - 1, 0x8080808080808080, 0x00000001FFFFFFFF):
        for seed in (0, 1, 0x9E3779B9):
            pair, _, ln, tf, tl, _, _ = W.piece_with_key(key, seed)
            assert W.key_of(tl - tf, W.mix32(pair ^ seed)) == key and ln >= 1


def _better(piece, seed, i, j):
    a = (-(int(piece[i]["t_last"]) - int(piece[i]["t_first"])), W.mix32(int(piece[i]["pair"]) ^ seed), i)
    b = (-(int(piece[j]["t_last"]) - int(piece[j]["t_first"])), W.mix32(int(piece[j]["pair"]) ^ seed), j)
    return a < b


def test_properties_on_random_windows():
    rng = np.random.default_rng(33)
    n = 40
    out = W.random_results(rng, n)
    O = list(zip(out["mat"].tolist(), out["aln"].tolist()))
    binding = 0
    for t in range(300):
        depth = int(rng.integers(0, 90))
        piece, off = W.batch([W.random_window(rng, depth, n, spans=int(rng.integers(1, 9)))])
        par = Par(max_depth=int(rng.integers(0, 50)), min_span=int(rng.integers(0, 6)), ident_num=3, ident_den=int(rng.choice([0, 4])), seed=int(rng.integers(0, 1 << 32)))
        ref = W.window_select_ref(piece, off, len(piece), out, par)
        cand = [j for j in range(depth) if W.is_candidate(piece[j].tolist(), O, n, par)]
        kept = ref.win[0].tolist()
        assert int(ref.ncand[0]) == len(cand) and set(kept) <= set(cand)
        assert len(kept) == min(len(cand), par.max_depth or len(cand)) and kept == sorted(kept) and len(set(kept)) == len(kept)
        dropped = [j for j in cand if j not in set(kept)]
        binding += bool(dropped)
        assert not any(_better(piece, par.seed, d, k) for d in dropped for k in kept)
        assert ref.src.tolist() == kept and np.array_equal(ref.sel, piece[kept]) and ref.sel_off.tolist() == [0, len(kept)]
    assert binding > 50


def test_no_tests_and_no_cap_is_the_identity():
    rng = np.random.default_rng(34)
    ws = [[r for r in W.random_window(rng, d, 30, bad=0.0)] for d in (5, 0, 70, 1)]
    piece, off = W.batch(ws)
    shifted = off + np.uint64(0)                               # well-formed windows
    ref = W.window_select_ref(piece, shifted, len(piece), None, Par())
    assert np.array_equal(ref.sel, piece) and np.array_equal(ref.sel_off, off) and ref.src.tolist() == list(range(len(piece)))
    # offsets that start above 0: sel_off is piece_off rebased
    tail = W.window_select_ref(piece, off[1:], len(piece), None, Par())
    assert np.array_equal(tail.sel_off, off[1:] - off[1]) and np.array_equal(tail.sel, piece[int(off[1]):])


def test_every_clause_of_the_candidate_test_on_its_border():
    names = set()
    for name, piece, off, out, n, par, want in W.filter_cases():
        ref = W.window_select_ref(piece, off, len(piece), out, par, n)
        if want is not None:
            assert ref.win[0].tolist() == want, (name, ref.win[0].tolist(), want)
        names.add(name)
    assert len(names) == len(W.filter_cases()) == 15
    # the header's identity example
    for (mat, aln), ok in W.HEADER_IDENTITY:
        assert W.is_candidate((0, 0, 1, 0, 9), [(mat, aln)], 1, Par(ident_num=4, ident_den=5)) == ok, (mat, aln)


def test_windows_that_have_no_pieces():
    rng = np.random.default_rng(35)
    for name, piece, off, piece_cap in W.window_cases(rng)[:5]:
        ref = W.window_select_ref(piece, off, piece_cap, None, Par())
        for g in range(len(off) - 1):
            a, b = int(off[g]), int(off[g + 1])
            if b > piece_cap or b < a:
                assert int(ref.ncand[g]) == 0 and len(ref.win[g]) == 0, (name, g)
        assert np.all(ref.src.astype(np.int64) < max(piece_cap, 1)), name


def test_chosen_keys_reach_either_side_of_every_digit_border():
    """the cases the GPU test runs hold what they promise: for every digit, keys that differ from a threshold by one in that digit, both ways"""
    ws = dict(W.key_windows(0x9E3779B9))
    for shift in range(0, 64, W.DIGIT_BITS):
        rows = ws["digit at bit %d" % shift]
        keys = sorted(set(W.key_of(r[4] - r[3], W.mix32(r[0] ^ 0x9E3779B9)) for r in rows))
        steps = set(b - a for a, b in zip(keys, keys[1:]))
        assert 1 << shift in steps and 2 * len(keys) == len(rows), shift
    run = ws["quota in a run"]
    assert len(set(W.key_of(r[4] - r[3], W.mix32(r[0] ^ 0x9E3779B9)) for r in run[60:71])) == 1 and len(run) > 71


def test_symbols_and_the_parameter_structure():
    import bsalign_amd as B
    W.need_symbols()
    assert C.sizeof(B.SELECT_PARAMS) == 32
    assert [(f, getattr(B.SELECT_PARAMS, f).offset) for f, _ in B.SELECT_PARAMS._fields_] == \
        [("max_depth", 0), ("min_span", 4), ("ident_num", 8), ("ident_den", 12), ("seed", 16), ("reserved", 20)]
    assert B.PIECE_DTYPE == W.PIECE_DTYPE and B.RESULT_DTYPE == W.RESULT_DTYPE and W.PIECE_DTYPE.itemsize == 32
    # without a context every call is refused before anything is touched
    par = B.SELECT_PARAMS()
    off = np.zeros(1, np.uint64)
    assert B.lib().bsa_window_select_run(None, None, None, 0, 0, None, 0, C.byref(par), None, 0, B._p(off), None, None) == -2
    assert B.lib().bsa_window_select_batch(None, None, None, 0, 0, None, 0, C.byref(par), None, 0, B._p(off), None, None) == -2


def test_python_size_checks():
    import torch
    import bsalign_amd as B
    nwin, piece_cap, n, sel_cap = 3, 10, 4, 7
    t = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8)
    good = dict(d_piece=t(32 * piece_cap), d_piece_off=t(8 * (nwin + 1)), d_out=t(40 * n), d_sel=t(32 * sel_cap), d_sel_off=t(8 * (nwin + 1)), d_sel_src=t(4 * sel_cap),
                d_ncand=t(4 * nwin))
    call = lambda **kw: B.Context.window_select_run(None, kw["d_piece"], kw["d_piece_off"], nwin, piece_cap, kw["d_out"], n, B.SELECT_PARAMS(), kw["d_sel"], sel_cap,
                                                    kw["d_sel_off"], kw["d_sel_src"], kw["d_ncand"])
    for k in good:                                             # (the checks come before the context is looked at)
        with pytest.raises(ValueError, match="window_select_run"):
            call(**dict(good, **{k: good[k][:-1]}))
    with pytest.raises(ValueError, match="min_ident needs results"):
        B.Context.window_select(None, [], min_ident=(7, 10))
