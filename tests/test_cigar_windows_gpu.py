"""GPU: bsa_cigar_windows_batch and bsa_cigar_windows_run (include/bsalign_hip.h) bit for bit against the Python statement of the definition
(cigar_windows_cases.windows_ref): on hand-made records and words uploaded directly, on what the aligners return, and for any arena capacity.
Every device buffer a run writes is prefilled with 0xA5 bytes and the window arena has 64 guard records on either side, so that a record a run
leaves unwritten, or one it writes where it must not, shows.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import cigar_windows_cases as W
import support as S

pytestmark = pytest.mark.gpu

GUARD = 64                         # guard records on either side of the window arena
SENT = 0xA5A5A5A5
E_ARG, E_CIGAR_CAP = -2, -5
_CASES = {}
CASE_NAMES = ["header_examples", "one_word_10000M", "one_word_10000M_off_border", "alternating_1M_1D", "alternating_1D_1M", "D_covers_three_windows",
              "leading_D_and_I", "leading_I_then_long_D", "I_words_only", "D_words_only", "tb_on_border", "tb_off_border", "te_on_border", "one_column",
              "w_1", "w_equals_te", "w_above_tlen", "w_2_pow_31", "w_max", "w_large_odd", "eqx_words", "other_ops_take_no_step", "zero_length_words",
              "more_target_than_te", "more_target_D_first", "far_more_target", "query_position_wraps", "less_target_than_te", "less_target_no_column",
              "words_1", "words_2", "words_63", "words_64", "words_65", "words_127", "words_128", "words_129", "words_200",
              "words_129_unit_lengths_w_3", "mixed_batch", "no_pairs", "thousand_pairs"]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


def _case(name):
    """(w, records, words, per-pair expected records, expected offsets), the reference computed once"""
    if not _CASES:
        for k, (w, recs, cigs) in W.hand_cases().items():
            _CASES[k] = (w, recs, cigs) + W.expected(w, recs, cigs)
    return _CASES[name]


def test_every_hand_made_case_is_run():
    _case("no_pairs")
    assert sorted(CASE_NAMES) == sorted(_CASES)


def _batch(ctx, w, recs, cigs, cap=None, alloc=None):
    """bsa_cigar_windows_batch -> (rc, win_off, the whole host arena of `alloc` records prefilled with 0xA5 bytes)"""
    import bsalign_amd as B
    n = len(recs)
    out = W.to_struct(recs)
    arena, off = W.flatten(cigs)
    win = np.full((max(alloc if alloc is not None else cap, 1), 4), SENT, dtype=np.uint32)
    woff = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = B.lib().bsa_cigar_windows_batch(ctx.h, B._p(out), B._p(arena) if len(arena) else None, B._p(off), n, w, B._p(win), cap, B._p(woff))
    return rc, woff, win


def _filled(nbytes):
    import torch
    return torch.full((max((nbytes + 15) // 16 * 16, 16),), 0xA5, dtype=torch.uint8, device="cuda")


def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.nbytes == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


class _Dev:
    """one batch on the device: records, words, offsets; a window arena of `alloc` records between two guards, and the offsets"""

    def __init__(self, w, recs, cigs, alloc):
        import torch
        self.w, self.n, self.alloc = w, len(recs), alloc
        arena, off = W.flatten(cigs)
        self.d_out, self.d_cig, self.d_coff = _upload(W.to_struct(recs)), _upload(arena), _upload(off)
        self.d_win = _filled((alloc + 2 * GUARD) * 16)
        self.d_woff = _filled((self.n + 1) * 8)
        torch.cuda.synchronize()

    def run(self, ctx, cap, null_win=False, want_rc=0):
        """-> (win_off, the records of the arena proper as (alloc, 4) uint32); the guards are checked here"""
        import torch
        import bsalign_amd as B
        assert cap <= self.alloc and not (null_win and cap)
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        rc = B.lib().bsa_cigar_windows_run(ctx.h, p(self.d_out), p(self.d_cig), p(self.d_coff), self.n, self.w,
                                           None if null_win else p(self.d_win, GUARD * 16), cap, p(self.d_woff))
        assert rc == want_rc, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        whole = self.d_win.cpu().numpy()[:(self.alloc + 2 * GUARD) * 16].view(np.uint32).reshape(-1, 4)
        assert np.all(whole[:GUARD] == SENT) and np.all(whole[GUARD + self.alloc:] == SENT), "a guard record was written"
        return self.d_woff.cpu().numpy()[:(self.n + 1) * 8].view(np.uint64).copy(), whole[GUARD:GUARD + self.alloc].copy()


def _check(off, win, per, woff, cap, what=""):
    """the arena contract: offsets exact; pair k's records there iff woff[k + 1] <= cap; every other record of the allocation untouched"""
    assert np.array_equal(off, woff), (what, "win_off", off[:8], woff[:8])
    untouched = np.ones(len(win), dtype=bool)
    present = 0
    for k in range(len(per)):
        a, b = int(woff[k]), int(woff[k + 1])
        assert b - a == len(per[k])
        if b <= cap:
            if not np.array_equal(win[a:b], per[k]):
                r = int(np.flatnonzero((win[a:b] != per[k]).any(axis=1))[0])
                raise AssertionError((what, "pair %d window %d of %d" % (k, r, b - a), win[a + r].tolist(), per[k][r].tolist()))
            untouched[a:b] = False
            present += 1
    assert np.all(win[untouched] == SENT), (what, "a record outside the pairs that fit was written", int(np.flatnonzero(untouched & (win != SENT).any(axis=1))[0]), cap)
    return present


# ---- 1. hand-made records and words, uploaded directly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hand_made_case(ctx, name):
    w, recs, cigs, per, woff = _case(name)
    need = int(woff[-1])
    rc, off, win = _batch(ctx, w, recs, cigs, cap=need, alloc=need + GUARD)
    assert rc == 0, rc
    assert _check(off, win, per, woff, need, name + " (batch)") == len(recs)
    dev = _Dev(w, recs, cigs, need + GUARD)
    off, win = dev.run(ctx, need + GUARD)
    assert _check(off, win, per, woff, need + GUARD, name + " (run)") == len(recs)


def test_one_pair_after_another(ctx):
    """n = 1: every pair of the mixed batch alone"""
    w, recs, cigs, per, woff = _case("mixed_batch")
    for k in range(0, len(recs), 3):
        rc, off, win = _batch(ctx, w, recs[k:k + 1], cigs[k:k + 1], cap=len(per[k]), alloc=len(per[k]) + 2)
        assert rc == 0 and list(off) == [0, len(per[k])] and np.array_equal(win[:len(per[k])], per[k]) and np.all(win[len(per[k]):] == SENT), k


N_TILED = 16400                    # above 16 384 counts the scan goes from one block to tiles of 4096


def test_more_pairs_than_one_scan_block(ctx):
    """16 400 pairs of one 30M word at w = 10: three or four records a pair, offsets across the borders of the scan's tiles"""
    cig = W.words((30, W.M))
    recs, cigs = [W.record(k % 7, k % 5, cig) for k in range(N_TILED)], [cig] * N_TILED
    per, woff = W.expected(10, recs, cigs)
    need = int(woff[-1])
    assert need > 3 * N_TILED and {len(p) for p in per} == {3, 4}
    dev = _Dev(10, recs, cigs, need + GUARD)
    off, win = dev.run(ctx, need + GUARD)
    assert _check(off, win, per, woff, need + GUARD, "16 400 pairs") == N_TILED


def test_window_counts_that_sum_above_2_pow_32_inside_a_thread(ctx):
    """count-only run at w = 1: every pair has one window, but pairs 4146 .. 4148 -- three of the sixteen counts of one thread of the tiled scan --
    have 2^31 - 1 each, so the prefix inside that thread passes 2^32"""
    cig = W.words((1, W.M))
    big = (4146, 4147, 4148)
    recs, cigs = [W.record(0, 0, cig, te=0x7FFFFFFF if k in big else 1) for k in range(N_TILED)], [cig] * N_TILED
    cnt = np.ones(N_TILED, dtype=np.uint64)
    cnt[list(big)] = 0x7FFFFFFF
    woff = np.zeros(N_TILED + 1, dtype=np.uint64)
    woff[1:] = np.cumsum(cnt, dtype=np.uint64)
    assert int(woff[4149]) - int(woff[4144]) > 1 << 32
    off, win = _Dev(1, recs, cigs, 0).run(ctx, 0, null_win=True)
    bad = np.flatnonzero(off != woff)
    assert len(bad) == 0, ("win_off", len(bad), int(bad[0]), int(off[bad[0]]), int(woff[bad[0]]))


# ---- 2. what the aligners return -----------------------------------------------------------------------------------------------------------
def _real_pairs():
    """64 pairs of 300 .. 2000 bases; every other one with a burst: a deleted or an inserted block of 10 .. 50 bases"""
    rng = np.random.default_rng(99)
    pairs = []
    for k in range(64):
        T = rng.integers(0, 4, int(rng.integers(300, 2001))).astype(np.uint8)
        Q = S.mutate(rng, T, float((0.02, 0.06, 0.12)[k % 3]))
        if k % 2:
            a, b = int(rng.integers(20, len(Q) - 80)), int(rng.integers(10, 51))
            Q = np.concatenate([Q[:a], Q[a + b:]]) if k % 4 == 1 else np.concatenate([Q[:a], rng.integers(0, 4, b).astype(np.uint8), Q[a:]])
        pairs.append((Q, T))
    return pairs


_REAL = {}


def _real(ctx, kind):
    """(records, CIGARs) of one aligner call, made once"""
    import bsalign_amd as B
    if kind not in _REAL:
        pairs = _real_pairs()
        sc = (2, -6, -3, -2, 0, 0)
        if kind in ("global", "overlap", "extend"):
            mode = {"global": B.MODE_GLOBAL, "overlap": B.MODE_OVERLAP, "extend": B.MODE_EXTEND}[kind]
            out, cigs, st = ctx.align_batch(pairs, B.make_params(mode, 64, *sc))
        elif kind == "edit":
            out, cigs, st = ctx.edit_batch(pairs, B.MODE_GLOBAL, 128)
        elif kind == "eqx":
            out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, 64, *sc), eqx=True)
            assert any(((c & 15) == B.CIGAR_X).any() for c in cigs) and not any(((c & 15) == B.CIGAR_M).any() for c in cigs)
        else:
            strands = [k % 3 == 0 for k in range(len(pairs))]
            stored = [(B.revcomp(q) if s else q, t) for (q, t), s in zip(pairs, strands)]
            out, cigs, st = ctx.align_batch(stored, B.make_params(B.MODE_OVERLAP, 64, *sc), strands=strands)
        assert sum(1 for c in cigs if len(c)) >= 32, kind
        _REAL[kind] = (out, cigs)
    return _REAL[kind]


@pytest.mark.parametrize("w", [50, 500])
@pytest.mark.parametrize("kind", ["global", "overlap", "extend", "edit", "eqx", "strands"])
def test_real_outputs(ctx, kind, w):
    import bsalign_amd as B
    out, cigs = _real(ctx, kind)
    per = [W.windows_ref(out[k], cigs[k], w) for k in range(len(cigs))]
    assert sum(len(p) for p in per) >= (600 if w == 50 else 100)
    got = ctx.cigar_windows(out, cigs, w)
    assert len(got) == len(per)
    for k, (g, p) in enumerate(zip(got, per)):
        assert g.dtype == np.uint32 and g.shape == p.shape and np.array_equal(g, p), (kind, w, k)
    # the resident form on the same records and words, through the Python wrapper
    n = len(cigs)
    recs = [np.array([out[k][f] for f in W.RESULT_FIELDS], dtype=np.int32) for k in range(n)]
    woff = np.zeros(n + 1, dtype=np.uint64)
    woff[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    tlen = np.array([max(int(r[4]), 0) for r in recs], dtype=np.uint32)
    cap = B.cigar_windows_bound(tlen, w)
    assert cap >= int(woff[-1])
    dev = _Dev(w, recs, cigs, cap)
    import torch
    d_win = dev.d_win[GUARD * 16:(GUARD + cap) * 16]
    ctx.cigar_windows_run(dev.d_out, dev.d_cig, dev.d_coff, n, w, d_win, cap, dev.d_woff)
    ctx.sync()
    torch.cuda.synchronize()
    off = dev.d_woff.cpu().numpy()[:(n + 1) * 8].view(np.uint64)
    win = dev.d_win.cpu().numpy().view(np.uint32).reshape(-1, 4)[GUARD:GUARD + cap]
    assert _check(off, win, per, woff, cap, "%s w %d (run)" % (kind, w)) == n


# ---- 3. the arena contract -------------------------------------------------------------------------------------------------------------
def test_arena_contract_for_any_capacity(ctx):
    w, recs, cigs, per, woff = _case("mixed_batch")
    need, n = int(woff[-1]), len(recs)
    assert need > 100 and sum(1 for p in per if len(p) == 0) >= 5
    mid = next(k for k in range(n // 2, n) if len(per[k]) >= 2)
    half = int(woff[mid]) + 1                                  # ends inside a pair's range
    assert 0 < woff[mid] and woff[mid + 1] > half
    dev = _Dev(w, recs, cigs, need + GUARD)
    for cap, null_win in ((0, False), (0, True), (half, False), (need - 1, False), (need, False), (int(woff[1]), False)):
        dev.d_win.fill_(0xA5)
        dev.d_woff.fill_(0xA5)
        off, win = dev.run(ctx, cap, null_win=null_win)
        what = "cap %d%s" % (cap, " (NULL arena)" if null_win else "")
        present = _check(off, win, per, woff, cap, what)
        assert present == sum(1 for k in range(n) if int(woff[k + 1]) <= cap), what
        if cap == 0:
            assert np.all(win == SENT), what
    # a second run on the same buffers, as the first left them: the same records
    dev.d_win.fill_(0xA5)
    dev.d_woff.fill_(0xA5)
    off1, win1 = dev.run(ctx, need)
    off2, win2 = dev.run(ctx, need)
    assert np.array_equal(off1, off2) and np.array_equal(win1, win2) and _check(off2, win2, per, woff, need, "second run") == n
    # ... and after a short run
    off3, win3 = dev.run(ctx, half)
    assert np.array_equal(off3, woff) and np.array_equal(win3, win1)


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    w, recs, cigs, per, woff = _case("header_examples")
    need = int(woff[-1])
    dev = _Dev(w, recs, cigs, need)
    run = B.lib().bsa_cigar_windows_run
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    args = [ctx.h, p(dev.d_out), p(dev.d_cig), p(dev.d_coff), dev.n, w, p(dev.d_win, GUARD * 16), need, p(dev.d_woff)]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return a
    assert run(*with_(5, 0)) == E_ARG                          # window == 0
    for i in (0, 1, 2, 3, 6, 8):                               # no context, records, words, offsets, arena (with a capacity), window offsets
        assert run(*with_(i, None)) == E_ARG, i
    off, win = dev.run(ctx, need)                              # nothing was launched by the refused calls; the good call still runs
    assert _check(off, win, per, woff, need, "after the refused calls") == 2
    batch = B.lib().bsa_cigar_windows_batch
    out, (arena, coff) = W.to_struct(recs), W.flatten(cigs)
    hwin, hoff = np.full((need, 4), SENT, np.uint32), np.zeros(dev.n + 1, np.uint64)
    bargs = [ctx.h, B._p(out), B._p(arena), B._p(coff), dev.n, w, B._p(hwin), need, B._p(hoff)]
    for i, v in ((5, 0), (0, None), (1, None), (2, None), (3, None), (6, None), (8, None)):
        a = list(bargs)
        a[i] = v
        assert batch(*a) == E_ARG, i
    assert np.all(hwin == SENT)
    with pytest.raises(B.BsaError) as e:
        ctx.cigar_windows(out, cigs, 0)
    assert e.value.code == E_ARG
    bad = coff.copy()
    bad[1] = bad[2] + 1                                        # offsets that decrease
    a = list(bargs)
    a[3] = B._p(bad)
    assert batch(*a) == E_ARG


def test_batch_with_a_short_arena(ctx):
    w, recs, cigs, per, woff = _case("mixed_batch")
    need = int(woff[-1])
    for cap in (0, 1, need - 1):
        rc, off, win = _batch(ctx, w, recs, cigs, cap=cap, alloc=need)
        assert rc == E_CIGAR_CAP and int(off[-1]) == need and np.array_equal(off, woff) and np.all(win == SENT), cap
    rc, off, win = _batch(ctx, w, recs, cigs, cap=need, alloc=need)
    assert rc == 0 and np.array_equal(win, np.concatenate(per))
