"""GPU: bsa_window_realign_run and bsa_window_realign_batch (include/bsalign_hip.h) against the Python statement of the definition
(window_realign_cases.window_realign_ref): both header examples, hand-made spans and paths at the smallest shapes at which the kernels can go wrong,
every way a window and a piece fail, windows of every depth and word count, any capacity of the word arena, re-runs, the argument errors, and a real
chain on resident buffers through two rounds.

Tolerance: none.  Offsets, records, statuses, costs, words, d_doff2 and d_dlen2 are compared bit for bit.

Every buffer a run writes is prefilled with 0xA5 bytes, the word arena has 256 guard bytes on either side, and the inputs are uploaded into
allocations of exactly their size.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import support as S
import window_cns_cases as WC
import window_msa_cases as W
import window_realign_cases as R
import window_stitch_cases as WS
from window_msa_cases import CNS_WINDOW_DTYPE, PAR7
from window_pieces_cases import PIECE_DTYPE

pytestmark = pytest.mark.gpu

GUARD = 256
FILL, FILL32, FILL64 = R.FILL, R.FILL32, R.FILL64
E_ARG, E_CIGAR_CAP, E_UNSUPPORTED = -2, -5, -6
_CASES = {}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


def _filled(nbytes):
    import torch
    return torch.full((max((nbytes + 15) // 16 * 16, 16),), FILL, dtype=torch.uint8, device="cuda")


def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.nbytes == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _down(t, nbytes, dtype):
    return t.cpu().numpy()[:nbytes].view(dtype).copy()


def _params(p):
    import bsalign_amd as B
    return B.realign_params(p["window2"], p["max_len"], p["min_margin"], p["x"], p["g"])


class Got:
    pass


class _Dev:
    """one batch on the device: every input in an allocation of exactly its size, the word arena of `alloc` words between guards"""

    def __init__(self, b, alloc):
        import torch
        self.b, self.alloc = b, alloc
        self.d_piece, self.d_poff, self.d_bases = _upload(b.piece[:b.piece_cap]), _upload(b.piece_off), _upload(b.bases[:b.bases_cap])
        self.d_seq, self.d_soff, self.d_cig, self.d_coff = _upload(b.seq[:b.seq_cap]), _upload(b.seq_off), _upload(b.cig[:b.cig_cap]), _upload(b.cig_off)
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        P, n = self.b.piece_cap, self.b.nwin
        self.d_words = _filled(4 * self.alloc + 2 * GUARD)
        self.d_p2, self.d_off2, self.d_st, self.d_cost = _filled(32 * P), _filled(8 * (P + 1)), _filled(4 * P), _filled(4 * P)
        self.d_doff2, self.d_dlen2 = _filled(8 * n), _filled(4 * n)

    def pointers(self, p, cap, null_words=False, null_cost=False):
        b = self.b
        ptr = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        self.par = _params(p)
        return [ptr(self.d_piece), ptr(self.d_poff), b.nwin, b.piece_cap, ptr(self.d_bases), b.bases_cap, b.window, ptr(self.d_seq), b.seq_cap, ptr(self.d_soff),
                ptr(self.d_cig), b.cig_cap, ptr(self.d_coff), C.byref(self.par), ptr(self.d_p2), None if null_words else ptr(self.d_words, GUARD), cap, ptr(self.d_off2),
                ptr(self.d_st), None if null_cost else ptr(self.d_cost), ptr(self.d_doff2), ptr(self.d_dlen2)]

    def run(self, ctx, p, cap, null_words=False, null_cost=False):
        import torch
        import bsalign_amd as B
        assert cap <= self.alloc and not (null_words and cap)
        rc = B.lib().bsa_window_realign_run(ctx.h, *self.pointers(p, cap, null_words, null_cost))
        assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        g, P, n = Got(), self.b.piece_cap, self.b.nwin
        w = self.d_words.cpu().numpy()
        assert np.all(w[:GUARD] == FILL) and np.all(w[GUARD + 4 * self.alloc:] == FILL), "a guard byte of the words was written"
        g.pcig2 = w[GUARD:GUARD + 4 * self.alloc].copy().view(np.uint32)
        g.piece2, g.pcig2_off = _down(self.d_p2, 32 * P, PIECE_DTYPE), _down(self.d_off2, 8 * (P + 1), np.uint64)
        g.pstatus, g.cost = _down(self.d_st, 4 * P, np.uint32), _down(self.d_cost, 4 * P, np.uint32)
        g.doff2, g.dlen2 = _down(self.d_doff2, 8 * n, np.uint64), _down(self.d_dlen2, 4 * n, np.uint32)
        return g


def _host(ctx, b, p, cap, alloc=None, null_words=False, null_cost=False):
    """bsa_window_realign_batch on host arrays prefilled with 0xA5 -> (rc, Got)"""
    import bsalign_amd as B
    P, n = b.piece_cap, b.nwin
    alloc = cap if alloc is None else alloc
    g = Got()
    g.pcig2 = np.full(max(alloc, 1), FILL32, np.uint32)
    g.piece2 = np.full(8 * max(P, 1), FILL32, np.uint32).view(PIECE_DTYPE)
    g.pcig2_off = np.full(P + 1, FILL64, np.uint64)
    g.pstatus, g.cost = np.full(max(P, 1), FILL32, np.uint32), np.full(max(P, 1), FILL32, np.uint32)
    g.doff2, g.dlen2 = np.full(max(n, 1), FILL64, np.uint64), np.full(max(n, 1), FILL32, np.uint32)
    hold = [np.ascontiguousarray(x) for x in (b.piece[:P], b.piece_off, b.bases[:b.bases_cap], b.seq[:b.seq_cap], b.seq_off, b.cig[:b.cig_cap], b.cig_off)]
    q = lambda a: B._p(a) if a.size else None
    par = _params(p)
    rc = B.lib().bsa_window_realign_batch(ctx.h, q(hold[0]), q(hold[1]), n, P, q(hold[2]), b.bases_cap, b.window, q(hold[3]), b.seq_cap, q(hold[4]), q(hold[5]), b.cig_cap, q(hold[6]),
                                          C.byref(par), B._p(g.piece2), None if null_words else B._p(g.pcig2), cap, B._p(g.pcig2_off), B._p(g.pstatus),
                                          None if null_cost else B._p(g.cost), B._p(g.doff2), B._p(g.dlen2))
    g.pcig2, g.piece2, g.pstatus, g.cost, g.doff2, g.dlen2 = g.pcig2[:alloc], g.piece2[:P], g.pstatus[:P], g.cost[:P], g.doff2[:n], g.dlen2[:n]
    return rc, g


def _same(got, ref, cap, what, cost=True):
    for name in PIECE_DTYPE.names:
        bad = np.flatnonzero(got.piece2[name] != ref.piece2[name])
        assert len(bad) == 0, (what, "piece2." + name, bad[:8], got.piece2[name][bad[:8]], ref.piece2[name][bad[:8]])
    for name in ("pstatus", "pcig2_off", "doff2", "dlen2") + (("cost",) if cost else ()):
        a, b = getattr(got, name), getattr(ref, name)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (what, name, bad[:8], a[bad[:8]], b[bad[:8]])
    bad = np.flatnonzero(got.pcig2[:cap] != ref.pcig2)
    assert len(bad) == 0, (what, "words", bad[:8], got.pcig2[bad[:8]], ref.pcig2[bad[:8]])
    assert np.all(got.pcig2[cap:] == FILL32), (what, "something at or above the cap was written")


def _both(ctx, b, p, what, slack=3):
    """_run and _batch against the reference with an arena of exactly the words needed -> the reference"""
    need = int(R.window_realign_ref(b, p, 0).pcig2_off[-1])
    ref = R.window_realign_ref(b, p, need)
    dev = _Dev(b, need + slack)
    _same(dev.run(ctx, p, need), ref, need, what + " (run)")
    rc, hgot = _host(ctx, b, p, need)
    assert rc == 0, rc
    _same(hgot, ref, need, what + " (batch)")
    return ref


# ---- 1. the header's examples ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [R.header_example_1, R.header_example_2])
def test_header_examples(ctx, make):
    R.need_symbols()
    b, p, want = make()
    ref = _both(ctx, b, p, make.__name__)
    assert ref.words[0].tolist() == want["words"] and int(ref.cost[0]) == want["cost"] and tuple(int(v) for v in ref.piece2[0]) == want["piece2"]


# ---- 2. spans, paths and scorings ------------------------------------------------------------------------------------------------------------------
def test_lengths_band_offsets_and_hand_made_paths(ctx):
    """n and m in {1, 2, 63, 64, 65}, |m - n| in {0, 1, 62, 63, 64}, paths along each edge diagonal, gap runs at both ends, an all-gap middle, codes
    above 3"""
    R.need_symbols()
    b, p = R.shapes_batch()
    ref = _both(ctx, b, p, "shapes")
    assert int((ref.pstatus == R.ST_EDGE).sum()) >= 4 and int((ref.pstatus == R.ST_OFF_BAND).sum()) >= 4


@pytest.mark.parametrize("name", ["x3_g1", "x1_g255", "x255_g1", "min_margin_0", "min_margin_8", "min_margin_31"])
def test_scorings_and_margins(ctx, name):
    R.need_symbols()
    b, p = R.scoring_batches()[name]
    ref = _both(ctx, b, p, name)
    if name == "x3_g1":
        assert int(ref.pstatus[0]) == R.ST_NO_DIAG


@pytest.mark.parametrize("max_len", [64, 2048])
def test_pieces_at_and_above_max_len(ctx, max_len):
    R.need_symbols()
    b, p = R.max_len_batch(max_len)
    ref = _both(ctx, b, p, "max_len %d" % max_len)
    assert ref.pstatus[:3].tolist() == [0, 0, R.ST_TOO_LONG] and int(ref.piece2[1]["len"]) == max_len


# ---- 3. windows --------------------------------------------------------------------------------------------------------------------------------------
def test_windows_of_every_word_count(ctx):
    """windows whose words are 1, 63, 64, 65 and 200 long, a one-word (draft) window among them; I runs directly in front of a; a and b on D units"""
    R.need_symbols()
    b, p = R.words_batch()
    assert [int(b.cig_off[g + 1] - b.cig_off[g]) for g in range(b.nwin)] == [1, 63, 1, 64, 65, 200]
    ref = _both(ctx, b, p, "word counts")
    assert R.ST_EMPTY_SPAN in ref.pstatus.tolist() and int((ref.pstatus & 0xFF == 0).sum()) >= 12


def test_a_draft_window_between_called_ones(ctx):
    R.need_symbols()
    b, p = R.draft_window_batch()
    ref = _both(ctx, b, p, "a DRAFT window")
    assert np.all(ref.pstatus & 0xFF == 0)


def test_windows_of_every_depth(ctx):
    """0, 1, 64, 65 and 300 pieces; t_first far from 0"""
    R.need_symbols()
    b, p = R.depths_batch()
    assert [int(b.piece_off[g + 1] - b.piece_off[g]) for g in range(b.nwin)] == list(R.DEPTHS)
    _both(ctx, b, p, "depths")


def test_every_way_a_window_fails(ctx):
    R.need_symbols()
    b, p, names, at = R.bad_windows_batch()
    assert len(b.seq) == b.seq_cap and len(b.cig) == b.cig_cap          # the arrays end where their allocations end
    ref = _both(ctx, b, p, "failing windows")
    for name in names:
        assert int(ref.dlen2[at[name]]) == 0 and int(ref.dlen2[at[name] - 1]) > 0, name
    batches, p = R.bad_offsets_batches()
    for name, bb in batches.items():
        _both(ctx, bb, p, name)


def test_every_way_a_piece_fails(ctx):
    R.need_symbols()
    b, p, at, want = R.bad_pieces_batch()
    ref = _both(ctx, b, p, "failing pieces")
    for name, st in want.items():
        assert int(ref.pstatus[at[name]]) == st, name
    batches, p = R.piece_off_batches()
    for name, bb in batches.items():
        _both(ctx, bb, p, name)


# ---- 4. the arena contract ---------------------------------------------------------------------------------------------------------------------------
def _arena_case():
    R.need_symbols()
    if "arena" not in _CASES:
        b, p = R.arena_batch()
        _CASES["arena"] = (b, p, R.window_realign_ref(b, p, 4096))
    return _CASES["arena"]


def test_any_pcig2_cap(ctx):
    """every pcig2_cap at, just before and just after a piece border, 0 and count-only: the offsets, records, statuses and costs are those of a
    large run, a piece's words are written whole if and only if its range ends inside the cap"""
    b, p, full = _arena_case()
    need = int(full.pcig2_off[-1])
    ends = sorted(set(int(x) for x in full.pcig2_off[1:]))
    caps = sorted(set(c for e in ends for c in (e - 1, e, e + 1) if 0 <= c <= need + 1) | {0})
    dev = _Dev(b, need + 1)
    for cap, null in [(c, False) for c in caps] + [(0, True)]:
        dev.fresh()
        ref = R.window_realign_ref(b, p, cap)
        _same(dev.run(ctx, p, cap, null_words=null), ref, cap, "pcig2_cap %d%s" % (cap, " (NULL arena)" if null else ""))
    dev.fresh()
    got = dev.run(ctx, p, need, null_cost=True)                 # d_cost may be missing
    _same(got, R.window_realign_ref(b, p, need), need, "no d_cost", cost=False)
    assert np.all(got.cost == FILL32)


def test_batch_with_a_short_arena(ctx):
    import bsalign_amd as B
    b, p, full = _arena_case()
    need = int(full.pcig2_off[-1])
    for cap, null in ((0, False), (0, True), (need - 1, False), (1, False)):
        rc, got = _host(ctx, b, p, cap, alloc=need, null_words=null)
        assert rc == E_CIGAR_CAP and int(got.pcig2_off[-1]) == need and np.all(got.pcig2 == FILL32) and B.lib().bsa_last_error(ctx.h), cap
        _same(got, R.window_realign_ref(b, p, 0), 0, "short arena %d" % cap)
    rc, got = _host(ctx, b, p, need + 5)
    assert rc == 0
    _same(got, R.window_realign_ref(b, p, need + 5), need + 5, "batch, a larger arena")


# ---- 5. re-run -----------------------------------------------------------------------------------------------------------------------------------------
def test_second_run_other_parameters_and_the_first_again(ctx):
    R.need_symbols()
    b, p = R.scoring_batches()["min_margin_8"]
    need = int(R.window_realign_ref(b, p, 0).pcig2_off[-1]) + 40
    dev = _Dev(b, need)
    one = dev.run(ctx, p, need)
    _same(one, R.window_realign_ref(b, p, need), need, "first run")
    two = dev.run(ctx, p, need)                                 # into the same arrays
    names = ("piece2", "pcig2", "pcig2_off", "pstatus", "cost", "doff2", "dlen2")
    for name in names:
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    dev.fresh()
    q = dict(p, min_margin=0, x=2, g=3, max_len=100)
    _same(dev.run(ctx, q, need), R.window_realign_ref(b, q, need), need, "other parameters")
    dev.fresh()
    three = dev.run(ctx, p, need)
    for name in names:
        assert np.array_equal(getattr(one, name), getattr(three, name)), name


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    b, p, full = _arena_case()
    need = int(full.pcig2_off[-1])
    dev = _Dev(b, need)
    run, batch, err = B.lib().bsa_window_realign_run, B.lib().bsa_window_realign_batch, B.lib().bsa_last_error
    rargs = [ctx.h] + dev.pointers(p, need)
    h = Got()
    h.in_ = [np.ascontiguousarray(x) for x in (b.piece, b.piece_off, b.bases, b.seq, b.seq_off, b.cig, b.cig_off)]
    h.p2, h.words, h.off2 = np.zeros(b.piece_cap, PIECE_DTYPE), np.full(need, FILL32, np.uint32), np.zeros(b.piece_cap + 1, np.uint64)
    h.st, h.cost, h.doff2, h.dlen2 = np.zeros(b.piece_cap, np.uint32), np.zeros(b.piece_cap, np.uint32), np.zeros(b.nwin, np.uint64), np.zeros(b.nwin, np.uint32)
    par = _params(p)
    bargs = [ctx.h, B._p(h.in_[0]), B._p(h.in_[1]), b.nwin, b.piece_cap, B._p(h.in_[2]), b.bases_cap, b.window, B._p(h.in_[3]), b.seq_cap, B._p(h.in_[4]), B._p(h.in_[5]), b.cig_cap,
             B._p(h.in_[6]), C.byref(par), B._p(h.p2), B._p(h.words), need, B._p(h.off2), B._p(h.st), B._p(h.cost), B._p(h.doff2), B._p(h.dlen2)]

    def refused(fn, base, changes, code=E_ARG):
        a = list(base)
        for i, v in changes.items():
            a[i] = v
        assert fn(*a) == code, (fn.__name__, changes)
        if 0 not in changes:
            assert err(ctx.h), (fn.__name__, changes)
    for fn, base in ((run, rargs), (batch, bargs)):
        # no context, pieces, piece_off, bases (with a cap), seq (with a cap), seq_off, words of the stitch (with a cap), cig_off, par, piece2, the arena (with a
        # cap), pcig2_off, pstatus, doff2, dlen2
        for i in (0, 1, 2, 5, 8, 10, 11, 13, 14, 15, 16, 18, 19, 21, 22):
            refused(fn, base, {i: None})
        refused(fn, base, {7: 0})                              # window
        refused(fn, base, {3: 0xFFFFFFF1})                     # nwin
        refused(fn, base, {4: 0xFFFFFFF1})                     # piece_cap
        refused(fn, base, {17: 0xFFFFFFF1})                    # pcig2_cap
        for q, code in ((dict(p, window2=0), E_ARG), (dict(p, max_len=0), E_ARG), (dict(p, x=0), E_ARG), (dict(p, g=0), E_ARG), (dict(p, x=256), E_ARG), (dict(p, g=256), E_ARG),
                        (dict(p, min_margin=32), E_ARG), (dict(p, window2=4097), E_UNSUPPORTED), (dict(p, max_len=2049), E_UNSUPPORTED)):
            bad = _params(q)
            refused(fn, base, {14: C.byref(bad)}, code)
        bad = _params(p)
        bad.reserved[1] = 1
        refused(fn, base, {14: C.byref(bad)})
    # nothing was launched by the refused calls; the good calls still run
    assert np.all(h.words == FILL32)
    assert run(*rargs) == 0
    ctx.sync()
    _same(dev.read(), R.window_realign_ref(b, p, need), need, "after the refused calls")
    assert batch(*bargs) == 0 and np.array_equal(h.words, full.pcig2[:need]) and np.array_equal(h.off2, full.pcig2_off) and np.array_equal(h.st, full.pstatus)
    # the limits themselves are accepted
    ok = _params(dict(p, window2=4096, max_len=2048, min_margin=31, x=255, g=255))
    a = list(rargs)
    a[14] = C.byref(ok)
    assert run(*a) == 0
    ctx.sync()
    # no windows: every offset 0, every status NO_WINDOW, every record its input with len 0
    dev.fresh()
    a = [ctx.h] + dev.pointers(p, need)
    a[3] = 0
    assert run(*a) == 0
    ctx.sync()
    got = dev.read()
    assert np.all(got.pcig2_off == 0) and np.all(got.pstatus == R.ST_NO_WINDOW) and np.all(got.pcig2 == FILL32) and np.all(got.piece2["len"] == 0)
    assert np.array_equal(got.piece2["base_off"], b.piece["base_off"]) and np.all(got.doff2 == FILL64)
    off = np.full(1, FILL64, np.uint64)
    assert batch(ctx.h, None, None, 0, 0, None, 0, 5, None, 0, None, None, 0, None, C.byref(par), None, None, 0, B._p(off), None, None, None, None) == 0 and off.tolist() == [0]
    # the Python plumbing's size checks
    import torch
    t = lambda nbytes: torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    P, n = b.piece_cap, b.nwin
    good = dict(d_piece=t(32 * P), d_piece_off=t(8 * (n + 1)), d_bases=t(b.bases_cap), d_seq=t(b.seq_cap), d_seq_off=t(8 * (n + 1)), d_cig=t(4 * b.cig_cap), d_cig_off=t(8 * (n + 1)),
                d_piece2=t(32 * P), d_pcig2=t(4 * need), d_pcig2_off=t(8 * (P + 1)), d_pstatus=t(4 * P), d_cost=t(4 * P), d_doff2=t(8 * n), d_dlen2=t(4 * n))
    call = lambda **kw: ctx.window_realign_run(kw["d_piece"], kw["d_piece_off"], n, P, kw["d_bases"], b.bases_cap, b.window, kw["d_seq"], b.seq_cap, kw["d_seq_off"], kw["d_cig"],
                                               b.cig_cap, kw["d_cig_off"], par, kw["d_piece2"], kw["d_pcig2"], need, kw["d_pcig2_off"], kw["d_pstatus"], kw["d_cost"],
                                               kw["d_doff2"], kw["d_dlen2"])
    call(**good)
    ctx.sync()
    for k in good:
        with pytest.raises(ValueError):
            call(**dict(good, **{k: good[k][:-1]}))


# ---- 7. a real chain, two rounds, on resident buffers ------------------------------------------------------------------------------------------------
def _cns_stitch(ctx, d_cols, cols_cap, d_cwin, nwin, max_rows, out_cap, min_cov):
    """bsa_window_cns_run without its compaction and bsa_window_stitch_run behind it on the same buffers -> (Got, the device arrays of the stitch)"""
    import torch
    d = {k: _filled(out_cap) for k in ("cns", "qlt", "alt")}
    d_clen, d_status = _filled(4 * nwin), _filled(4 * nwin)
    model = _CASES.setdefault("model", ctx.cns_model(PAR7))
    ctx.window_cns_run(model, d_cols, cols_cap, d_cwin, nwin, max_rows, d["cns"], d["qlt"], d["alt"], out_cap, d_clen, None, d_status)
    d_seq, d_sq, d_cig = _filled(out_cap), _filled(out_cap), _filled(4 * out_cap)
    d_soff, d_coff, d_rec = _filled(8 * (nwin + 1)), _filled(8 * (nwin + 1)), _filled(32 * nwin)
    ctx.window_stitch_run(d_cols, cols_cap, d_cwin, nwin, d_status, min_cov, d_seq, d_sq, None, out_cap, d_soff, d_cig, out_cap, d_coff, d_rec)
    ctx.sync()
    torch.cuda.synchronize()
    g = Got()
    g.status = _down(d_status, 4 * nwin, np.uint32)
    g.seq, g.cig = d_seq.cpu().numpy()[:out_cap].copy(), _down(d_cig, 4 * out_cap, np.uint32)
    g.seq_off, g.cig_off, g.rec = _down(d_soff, 8 * (nwin + 1), np.uint64), _down(d_coff, 8 * (nwin + 1), np.uint64), _down(d_rec, 32 * nwin, WS.STITCH_DTYPE)
    g.cols = d_cols.cpu().numpy()[:cols_cap].copy()
    return g, (d_seq, d_soff, d_cig, d_coff)


def test_two_rounds_on_resident_buffers(ctx):
    """align_batch's records and words uploaded, then windows, pieces, guides, MSA, consensus and stitch on the device at w = 50 on three short drafts;
    then the re-alignment, MSA, consensus and stitch again, nothing coming down in between.  Every round-2 output equals the Python references of
    those passes fed from window_realign_ref, and every re-aligned piece is live in the round-2 MSA."""
    import bsalign_amd as B
    R.need_symbols()
    w, w2 = 50, 64
    rng = np.random.default_rng(2207)
    drafts = [rng.integers(0, 4, L).astype(np.uint8) for L in (230, 150, 95)]
    truths = [S.mutate(rng, d, 0.05) for d in drafts]
    pairs, tid = [], []
    for t, (dr, tr) in enumerate(zip(drafts, truths)):
        for _ in range(5):
            pairs.append((S.mutate(rng, tr, 0.08), dr))
            tid.append(t)
    n = len(pairs)
    out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, 64, 2, -6, -3, -2, 0, 0))
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(c) for c in cigs], dtype=np.uint64)
    arena = np.concatenate(cigs).astype(np.uint32)
    ins = int(sum(int(x) >> 4 for c in cigs for x in c if int(x) & 15 == 1))
    gbase, nwin = B.window_gbase(tid, [len(d) for d in drafts], w)
    win_cap = B.cigar_windows_bound(tlen, w)
    piece_cap, bases_cap, pcig_cap = win_cap, int(qlen.sum()), B.piece_cigars_bound(coff, win_cap)
    doff, dlen = B.window_drafts([int(toff[5 * t]) for t in range(3)], [len(d) for d in drafts], w)      # each draft: its first pair's target in the blob
    cols_cap, out_cap = (nwin * w2 + 2 * ins) * (5 + 4), nwin * w2 + 2 * ins
    d_seqs, d_qoff, d_qlen, d_out, d_cig, d_coff, d_gbase, d_doff, d_dlen = (_upload(x) for x in (np.concatenate([seqs, np.zeros(8, np.uint8)]), qoff, qlen, out, arena, coff, gbase,
                                                                                                  doff, dlen))
    d_win, d_woff = _filled(16 * win_cap), _filled(8 * (n + 1))
    d_piece, d_poff, d_bases, d_boff = _filled(32 * piece_cap), _filled(8 * (nwin + 1)), _filled(bases_cap), _filled(8 * (nwin + 1))
    d_pcig, d_pcoff = _filled(4 * pcig_cap), _filled(8 * (piece_cap + 1))
    d_cols, d_cwoff, d_cwin = _filled(cols_cap), _filled(8 * (nwin + 1)), _filled(40 * nwin)
    ctx.cigar_windows_run(d_out, d_cig, d_coff, n, w, d_win, win_cap, d_woff)
    ctx.window_pieces_run(d_seqs, d_qoff, d_qlen, d_win, d_woff, n, w, d_gbase, nwin, 0, d_piece, piece_cap, d_poff, d_bases, bases_cap, d_boff)
    ctx.piece_cigars_run(d_out, d_cig, d_coff, n, d_piece, d_poff[8 * nwin:], piece_cap, d_pcig, pcig_cap, d_pcoff, None)
    ctx.window_msa_run(d_piece, d_poff, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w, 0, 0, d_cols, cols_cap, d_cwoff, d_cwin)
    one, (d_seq, d_soff, d_scig, d_scoff) = _cns_stitch(ctx, d_cols, cols_cap, d_cwin, nwin, 5, out_cap, 1)
    assert np.all(one.status == 0) and np.all(one.rec["status"] == 0)
    # round 2
    p = R.par(w2, 128, 8, 1, 1)
    pcig2_cap = 2 * bases_cap + 63 * piece_cap
    d_p2, d_pcig2, d_off2 = _filled(32 * piece_cap), _filled(4 * pcig2_cap), _filled(8 * (piece_cap + 1))
    d_st, d_cost, d_doff2, d_dlen2 = _filled(4 * piece_cap), _filled(4 * piece_cap), _filled(8 * nwin), _filled(4 * nwin)
    ctx.window_realign_run(d_piece, d_poff, nwin, piece_cap, d_bases, bases_cap, w, d_seq, out_cap, d_soff, d_scig, out_cap, d_scoff, _params(p), d_p2, d_pcig2, pcig2_cap, d_off2,
                           d_st, d_cost, d_doff2, d_dlen2)
    d_cols2, d_cwoff2, d_cwin2 = _filled(cols_cap), _filled(8 * (nwin + 1)), _filled(40 * nwin)
    ctx.window_msa_run(d_p2, d_poff, nwin, piece_cap, d_bases, bases_cap, d_pcig2, pcig2_cap, d_off2, d_seq, d_doff2, d_dlen2, w2, 0, 0, d_cols2, cols_cap, d_cwoff2, d_cwin2)
    two, _ = _cns_stitch(ctx, d_cols2, cols_cap, d_cwin2, nwin, 5, out_cap, 1)
    # the references, fed from what round 1 left
    piece, poff, bases = _down(d_piece, 32 * piece_cap, PIECE_DTYPE), _down(d_poff, 8 * (nwin + 1), np.uint64), d_bases.cpu().numpy()[:bases_cap].copy()
    rb = R.RBatch(piece, poff, bases, w, one.seq, one.seq_off, one.cig, one.cig_off)
    ref = R.window_realign_ref(rb, p, pcig2_cap)
    got = Got()
    got.piece2, got.pcig2, got.pcig2_off = _down(d_p2, 32 * piece_cap, PIECE_DTYPE), _down(d_pcig2, 4 * pcig2_cap, np.uint32), _down(d_off2, 8 * (piece_cap + 1), np.uint64)
    got.pstatus, got.cost, got.doff2, got.dlen2 = _down(d_st, 4 * piece_cap, np.uint32), _down(d_cost, 4 * piece_cap, np.uint32), _down(d_doff2, 8 * nwin, np.uint64), _down(d_dlen2, 4 * nwin, np.uint32)
    _same(got, ref, pcig2_cap, "round 2, the re-alignment")
    npiece = int(poff[nwin])
    assert npiece > 40 and np.all(ref.pstatus[npiece:] == R.ST_NO_WINDOW) and int((ref.pstatus[:npiece] & 0xFF == 0).sum()) >= npiece - 2
    mb = W.Batch(ref.piece2, poff, bases, ref.pcig2, ref.pcig2_off, np.concatenate([one.seq, np.zeros(8, np.uint8)]), ref.doff2, ref.dlen2, w2, piece_cap=piece_cap, bases_cap=bases_cap)
    for g in range(nwin):
        live = W.window_ref(mb, g)[4]
        for r_, j in enumerate(range(int(poff[g]), int(poff[g + 1]))):
            assert live[r_] == (int(ref.pstatus[j]) & 0xFF == 0), (g, j)
    roff, rcwin, rcols = W.window_msa_ref(mb, 0)
    assert np.array_equal(_down(d_cwoff2, 8 * (nwin + 1), np.uint64), roff)
    cwin2 = _down(d_cwin2, 40 * nwin, CNS_WINDOW_DTYPE)
    for name in CNS_WINDOW_DTYPE.names:
        assert np.array_equal(cwin2[name], rcwin[name]), name
    need = int(roff[-1])
    rcns = WC.window_cns_ref(rcols, rcwin, need, out_cap, out_cap, 5, PAR7)
    assert np.array_equal(two.status, rcns.status) and np.array_equal(two.cols[:need], rcns.cols[:need])
    rst = WS.window_stitch_ref(rcns.cols, rcwin, need, rcns.status, 1, out_cap, out_cap)
    assert np.array_equal(two.seq_off, rst.seq_off) and np.array_equal(two.cig_off, rst.cig_off) and np.array_equal(two.rec, rst.rec)
    ns, nc = int(rst.seq_off[-1]), int(rst.cig_off[-1])
    assert np.array_equal(two.seq[:ns], rst.seq[:ns]) and np.array_equal(two.cig[:nc], rst.cig[:nc])
    # round 2's words are against round 1's sequence
    for g in range(nwin):
        WS.cigar_apply(one.seq[int(one.seq_off[g]):int(one.seq_off[g + 1])], rst.win[g][0], rst.win[g][3])
    # the host-pointer call gives the same pieces, guides and drafts
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(pairs, wins, w, gbase, nwin)
    per, flat = ctx.window_stitch([(one.cols[int(c["cols_off"]):int(c["cols_off"]) + int(c["mlen"]) * (int(c["nall"]) + 3)], c) for c in _down(d_cwin, 40 * nwin, CNS_WINDOW_DTYPE)],
                                  min_cov=1, status=[0] * nwin)
    pieces2, guides2, drafts2 = ctx.window_realign(wp, (per, flat), w, _params(p))
    for g in range(nwin):
        a, b_ = int(poff[g]), int(poff[g + 1])
        assert np.array_equal(drafts2[g], one.seq[int(one.seq_off[g]):int(one.seq_off[g + 1])])
        for r_, j in enumerate(range(a, b_)):
            ws_, st_ = guides2[g][r_]
            assert st_ == int(ref.pstatus[j]) and np.array_equal(ws_, ref.words[j]), (g, j)
            for name in ("pair", "q_first", "len", "t_first", "t_last"):
                assert int(pieces2[g][0][r_][name]) == int(ref.piece2[j][name]), (g, j, name)
            lead = int(ref.piece2[j]["base_off"]) - int(piece[j]["base_off"])
            bo = int(piece[j]["base_off"])
            assert np.array_equal(pieces2[g][1][r_], bases[bo + lead:bo + lead + int(ref.piece2[j]["len"])])
    msas2 = ctx.window_msa(pieces2, guides2, drafts2, w2, vote=False)
    for g in range(nwin):
        assert np.array_equal(msas2[g][0].reshape(-1), rcols[int(roff[g]):int(roff[g + 1])]), g
