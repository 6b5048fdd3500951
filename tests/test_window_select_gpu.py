"""GPU: bsa_window_select_run and bsa_window_select_batch (include/bsalign_hip.h) against the Python statement of the definition
(window_select_cases.window_select_ref): the header's example, every depth at which the kernels take another path with every cap around it, chosen
keys on either side of every digit border of the selection, every clause of the candidate test on its border, offsets that make no sense, any
capacity of the arena, re-runs, the aligner's output through all resident passes with the selection in place, and the argument errors.

Tolerance: none.  Offsets, candidate counts, records and source indices are compared bit for bit.

Every buffer a run writes is prefilled with 0xA5 bytes; d_sel lies between 64 guard records and d_sel_src between 64 guard words; the records, the
offsets and the aligner's records are uploaded into allocations of exactly their size.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import support as S
import window_select_cases as W
from window_select_cases import FILL, FILL32, FILL64, M32, Par

pytestmark = pytest.mark.gpu

GUARD = 64                                                     # records in front of and behind d_sel, words around d_sel_src
E_ARG, E_CIGAR_CAP = -2, -5


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


def _inside(t, guard, nbytes, what):
    w = t.cpu().numpy()
    assert np.all(w[:guard] == FILL) and np.all(w[guard + nbytes:] == FILL), "a guard byte of %s was written" % what
    return w[guard:guard + nbytes].copy()


def _params(par, reserved=(0, 0, 0)):
    import bsalign_amd as B
    return B.SELECT_PARAMS(par.max_depth, par.min_span, par.ident_num, par.ident_den, par.seed, (C.c_uint32 * 3)(*reserved))


class Got:
    pass


class _Dev:
    """one batch on the device: piece_cap records, nwin + 1 offsets and n aligner's records in allocations of exactly their size; d_sel of `alloc`
    records and d_sel_src of `alloc` words between guards"""

    def __init__(self, piece, piece_off, piece_cap, out, n, alloc, shift=0, in_shift=0):
        import torch
        self.nwin, self.piece_cap, self.n, self.alloc, self.shift = len(piece_off) - 1, piece_cap, n, alloc, shift          # shift: bytes d_sel lies behind its guard
        self.in_shift = in_shift                                 # bytes of padding in front of the records: they still end where their allocation ends
        self.d_piece = _upload(np.concatenate([np.zeros(in_shift, np.uint8), np.ascontiguousarray(piece[:piece_cap]).view(np.uint8).reshape(-1)]))
        self.d_poff = _upload(piece_off)
        self.d_out = None if out is None else _upload(out[:n])
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        self.d_sel, self.d_src = _filled(32 * (self.alloc + 2 * GUARD) + 16), _filled(4 * (self.alloc + 2 * GUARD))
        self.d_soff, self.d_nc = _filled(8 * (self.nwin + 1)), _filled(4 * self.nwin)

    def pointers(self, par, sel_cap, null_sel=False, null_src=False, null_nc=False):
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        return [p(self.d_piece, self.in_shift) if self.piece_cap else None, p(self.d_poff), self.nwin, self.piece_cap, None if self.d_out is None else p(self.d_out), self.n, C.byref(_params(par)),
                None if null_sel else p(self.d_sel, 32 * GUARD + self.shift), sel_cap, p(self.d_soff), None if (null_src or null_sel) else p(self.d_src, 4 * GUARD), None if null_nc else p(self.d_nc)]

    def run(self, ctx, par, sel_cap, **null):
        import torch
        import bsalign_amd as B
        assert sel_cap <= self.alloc and not (null.get("null_sel") and sel_cap)
        rc = B.lib().bsa_window_select_run(ctx.h, *self.pointers(par, sel_cap, **null))
        assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        g = Got()
        g.sel = _inside(self.d_sel, 32 * GUARD + self.shift, 32 * self.alloc, "d_sel")
        g.src = _inside(self.d_src, 4 * GUARD, 4 * self.alloc, "d_sel_src").view(np.uint32)
        g.sel_off, g.ncand = _down(self.d_soff, 8 * (self.nwin + 1), np.uint64), _down(self.d_nc, 4 * self.nwin, np.uint32)
        return g


def _host(ctx, piece, piece_off, piece_cap, out, n, par, sel_cap, alloc, null_sel=False, null_src=False, null_nc=False):
    """bsa_window_select_batch on host arrays prefilled with 0xA5 -> (rc, Got)"""
    import bsalign_amd as B
    nwin = len(piece_off) - 1
    g = Got()
    sel, src = np.full(32 * max(alloc, 1), FILL, np.uint8), np.full(max(alloc, 1), FILL32, np.uint32)
    g.sel_off, nc = np.full(nwin + 1, FILL64, np.uint64), np.full(max(nwin, 1), FILL32, np.uint32)
    hp, ho = np.ascontiguousarray(piece[:piece_cap]).copy(), None if out is None else np.ascontiguousarray(out[:n]).copy()
    rc = B.lib().bsa_window_select_batch(ctx.h, B._p(hp) if piece_cap else None, B._p(piece_off), nwin, piece_cap, None if ho is None else B._p(ho), n, C.byref(_params(par)),
                                         None if null_sel else B._p(sel), sel_cap, B._p(g.sel_off), None if (null_src or null_sel) else B._p(src), None if null_nc else B._p(nc))
    assert np.array_equal(hp, piece[:piece_cap]), "the records are read-only"
    g.sel, g.src, g.ncand = sel[:32 * alloc], src[:alloc], nc[:nwin]
    return rc, g


def _same(got, ref, sel_cap, what, src=True, ncand=True):
    assert np.array_equal(got.sel_off, ref.sel_off), (what, "sel_off", got.sel_off[:12], ref.sel_off[:12])
    if ncand:
        assert np.array_equal(got.ncand, ref.ncand), (what, "ncand", got.ncand[:12], ref.ncand[:12])
    else:
        assert np.all(got.ncand == FILL32), (what, "ncand was not given")
    alloc = len(got.src)
    sel, sr = W.expected_arena(ref, sel_cap, alloc)
    bad = np.flatnonzero(got.sel != sel)
    assert len(bad) == 0, (what, "sel: first wrong record", int(bad[0]) // 32, got.sel[bad[0] // 32 * 32:][:32], sel[bad[0] // 32 * 32:][:32])
    if src:
        bad = np.flatnonzero(got.src != sr)
        assert len(bad) == 0, (what, "sel_src", bad[:8], got.src[bad[:8]], sr[bad[:8]])
    else:
        assert np.all(got.src == FILL32), (what, "sel_src was not given")


def _both(ctx, piece, piece_off, piece_cap, out, n, par, what, dev=None, ref=None, slack=3):
    """the device-pointer call, with an arena `slack` records larger than needed, and the host-pointer call with the exact cap, against the reference"""
    ref = ref or W.window_select_ref(piece, piece_off, piece_cap, out, par, n)
    need = int(ref.sel_off[-1])
    if dev is None:
        dev = _Dev(piece, piece_off, piece_cap, out, n, need + slack)
    else:
        assert dev.alloc >= need
        dev.fresh()
    _same(dev.run(ctx, par, dev.alloc), ref, dev.alloc, what + ", run")
    rc, got = _host(ctx, piece, piece_off, piece_cap, out, n, par, need, need + slack)
    assert rc == 0, (what, rc)
    _same(got, ref, need, what + ", batch")
    return ref


# ---- 1. the header's example ---------------------------------------------------------------------------------------------------------------------------
def test_header_example(ctx):
    W.need_symbols()
    piece, off, want = W.header_example()
    for (seed, md), idx in want.items():
        ref = _both(ctx, piece, off, len(piece), None, 0, Par(max_depth=md, min_span=6, seed=seed), "header example, seed %d, max_depth %d" % (seed, md))
        assert ref.win[0].tolist() == idx and int(ref.ncand[0]) == 5


# ---- 2. depths -------------------------------------------------------------------------------------------------------------------------------------------
def test_every_depth_with_every_cap(ctx):
    """one window of each depth -- around the trips of 64, around the depth up to which the keys stay in LDS, one of 5000 -- under every max_depth
    around 64 and around every window's candidate count; some records are no pieces, a span test and an identity test drop others"""
    W.need_symbols()
    rng = np.random.default_rng(4101)
    n = 300
    depths, ws = W.depth_cases(rng, n)
    piece, off = W.batch(ws)
    out = W.random_results(rng, n)
    base = Par(min_span=2, ident_num=4, ident_den=5, seed=77)
    ncand = W.window_select_ref(piece, off, len(piece), out, base).ncand
    assert int(ncand[-1]) > 1000 and len(set(ncand.tolist())) >= 12
    dev = _Dev(piece, off, len(piece), out, n, int(ncand.sum()))
    for md in W.max_depths(ncand):
        par = base._replace(max_depth=md)
        ref = W.window_select_ref(piece, off, len(piece), out, par)
        dev.fresh()
        _same(dev.run(ctx, par, dev.alloc), ref, dev.alloc, "depths %s, max_depth %d" % (depths, md))
        assert np.array_equal(np.diff(ref.sel_off.astype(np.int64)), np.minimum(ncand, md or M32))
    for md in (0, 1, 64, int(ncand[-1]) - 1, M32):             # the host-pointer call
        par = base._replace(max_depth=md)
        ref = W.window_select_ref(piece, off, len(piece), out, par)
        rc, got = _host(ctx, piece, off, len(piece), out, n, par, int(ref.sel_off[-1]), int(ref.sel_off[-1]))
        assert rc == 0
        _same(got, ref, int(ref.sel_off[-1]), "depths, batch, max_depth %d" % md)


def test_either_side_of_the_lds_threshold_gives_the_same_selection(ctx):
    """the same 511 records as a window of 511, of 512 with one record that is no piece, and of 513 with two: the selected records are the same"""
    W.need_symbols()
    rng = np.random.default_rng(4102)
    rows = W.random_window(rng, W.HELD - 1, 100, spans=3, bad=0.0)
    dead = (1, 2, 0, 5, 9, 0, 0)                               # len 0
    piece, off = W.batch([rows, rows + [dead], rows + [dead, dead]])
    for md in (1, 100, 300, 510):
        ref = _both(ctx, piece, off, len(piece), None, 0, Par(max_depth=md, seed=5), "around the threshold, max_depth %d" % md)
        assert ref.win[0].tolist() == ref.win[1].tolist() == ref.win[2].tolist() and len(ref.win[0]) == md


# ---- 3. keys ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0x9E3779B9])
def test_chosen_keys_under_every_cap(ctx, seed):
    """windows whose keys are chosen through the inverse of mix32 -- all spans distinct, all equal, one pair throughout, a quota that ends inside a run
    of equal keys across a trip's border, the extreme spans, hashes that differ in one bit, and for every digit of the selection a threshold with a
    neighbour on either side -- in one batch, under every max_depth from 1 to the deepest window's depth"""
    W.need_symbols()
    ws = W.key_windows(seed)
    piece, off = W.batch([rows for _, rows in ws])
    deepest = max(len(rows) for _, rows in ws)
    dev = _Dev(piece, off, len(piece), None, 0, len(piece))
    for md in list(range(1, deepest + 2)) + [0]:
        par = Par(max_depth=md, seed=seed)
        ref = W.window_select_ref(piece, off, len(piece), None, par)
        dev.fresh()
        _same(dev.run(ctx, par, dev.alloc), ref, dev.alloc, "chosen keys, seed %#x, max_depth %d" % (seed, md))
    # the quota ends at j = 63, 64 and 65 inside the run of equal keys from j = 60 to 70
    g = [name for name, _ in ws].index("quota in a run")
    for md in (64, 65, 66):
        ref = W.window_select_ref(piece, off, len(piece), None, Par(max_depth=md, seed=seed))
        assert ref.win[g].tolist() == list(range(md))
    rc, got = _host(ctx, piece, off, len(piece), None, 0, Par(max_depth=7, seed=seed), len(piece), len(piece))
    assert rc == 0
    _same(got, W.window_select_ref(piece, off, len(piece), None, Par(max_depth=7, seed=seed)), len(piece), "chosen keys, batch")


# ---- 4. filters --------------------------------------------------------------------------------------------------------------------------------------------
def test_every_clause_of_the_candidate_test_on_its_border(ctx):
    W.need_symbols()
    for name, piece, off, out, n, par, want in W.filter_cases():
        ref = _both(ctx, piece, off, len(piece), out, n, par, name)
        if want is not None:
            assert ref.win[0].tolist() == want, (name, ref.win[0].tolist(), want)
        capped = par._replace(max_depth=max(int(ref.ncand[0]) - 1, 1))
        _both(ctx, piece, off, len(piece), out, n, capped, name + ", capped")


# ---- 5. windows --------------------------------------------------------------------------------------------------------------------------------------------
def test_offsets_that_make_no_sense_and_many_windows(ctx):
    W.need_symbols()
    rng = np.random.default_rng(4105)
    for name, piece, off, piece_cap in W.window_cases(rng):
        for par in (Par(), Par(max_depth=4, min_span=3, seed=1), Par(max_depth=40)):
            ref = _both(ctx, piece, off, piece_cap, None, 0, par, "%s, %s" % (name, par))
            if name == "a piece_off that decreases":
                assert int(ref.ncand[1]) == 0 and int(ref.ncand[2]) > 0
            if name == "a piece_cap of 0":
                assert int(ref.sel_off[-1]) == 0


# ---- 6. the arena --------------------------------------------------------------------------------------------------------------------------------------------
def _arena_case():
    rng = np.random.default_rng(4106)
    piece, off = W.batch([W.random_window(rng, d, 60) for d in (9, 0, 70, 3, 1, 130, 12)])
    par = Par(max_depth=50, min_span=2, seed=3)
    return piece, off, par, W.window_select_ref(piece, off, len(piece), None, par)


def test_any_sel_cap(ctx):
    """every sel_cap at, just before and just after a window border: the offsets and counts are those of a large run, a window's records and source
    indices are written whole if and only if its range ends inside sel_cap, and nothing else is touched"""
    W.need_symbols()
    piece, off, par, full = _arena_case()
    need = int(full.sel_off[-1])
    dev = _Dev(piece, off, len(piece), None, 0, need + 1)
    ends = sorted(set(int(x) for x in full.sel_off[1:]))
    caps = sorted(set(c for e in ends for c in (e - 1, e, e + 1) if 0 <= c <= need + 1) | {0})
    assert len(caps) >= 14
    for cap in caps:
        dev.fresh()
        _same(dev.run(ctx, par, cap), full, cap, "sel_cap %d" % cap)


def test_count_only_and_missing_arrays(ctx):
    W.need_symbols()
    piece, off, par, full = _arena_case()
    need = int(full.sel_off[-1])
    dev = _Dev(piece, off, len(piece), None, 0, need)
    for null in (False, True):                                 # cap 0 with arenas, and without
        dev.fresh()
        _same(dev.run(ctx, par, 0, null_sel=null), full, 0, "count only")
    dev.fresh()
    _same(dev.run(ctx, par, need, null_src=True), full, need, "no d_sel_src", src=False)
    dev.fresh()
    _same(dev.run(ctx, par, need, null_nc=True), full, need, "no d_ncand", ncand=False)
    rc, got = _host(ctx, piece, off, len(piece), None, 0, par, need, need, null_src=True, null_nc=True)
    assert rc == 0
    _same(got, full, need, "batch without both", src=False, ncand=False)


@pytest.mark.parametrize("shift,in_shift", [(8, 0), (0, 8), (8, 8)])
def test_arrays_aligned_to_8_bytes_only(ctx, shift, in_shift):
    """d_sel, d_piece or both 8 bytes behind a 16-byte border: the records move as 8-byte vectors, the result is the same"""
    W.need_symbols()
    piece, off, par, full = _arena_case()
    need = int(full.sel_off[-1])
    dev = _Dev(piece, off, len(piece), None, 0, need + 2, shift=shift, in_shift=in_shift)
    assert (dev.d_piece.data_ptr() + in_shift) % 16 == in_shift and (dev.d_sel.data_ptr() + 32 * GUARD + shift) % 16 == shift
    for cap in (need + 2, need, int(full.sel_off[3]), 0):
        dev.fresh()
        _same(dev.run(ctx, par, cap), full, cap, "d_sel at %d, d_piece at %d bytes, sel_cap %d" % (shift, in_shift, cap))


def test_batch_with_a_short_arena(ctx):
    import bsalign_amd as B
    W.need_symbols()
    piece, off, par, full = _arena_case()
    need = int(full.sel_off[-1])
    for cap, null in ((0, False), (0, True), (1, False), (need - 1, False)):
        rc, got = _host(ctx, piece, off, len(piece), None, 0, par, cap, need, null_sel=null)
        assert rc == E_CIGAR_CAP and B.lib().bsa_last_error(ctx.h), cap
        _same(got, full, -1, "batch, sel_cap %d" % cap)        # the offsets and counts with the total; no record, no source index


# ---- 7. re-run -------------------------------------------------------------------------------------------------------------------------------------------
def test_second_run_with_other_parameters_then_the_first_again(ctx):
    W.need_symbols()
    rng = np.random.default_rng(4107)
    piece, off = W.batch([W.random_window(rng, d, 80) for d in (40, 600, 7, 64)])
    out = W.random_results(rng, 80)
    one, two = Par(max_depth=20, seed=1), Par(max_depth=5, min_span=4, ident_num=3, ident_den=4, seed=2)
    dev = _Dev(piece, off, len(piece), out, 80, len(piece))
    a = dev.run(ctx, one, dev.alloc)
    _same(a, W.window_select_ref(piece, off, len(piece), out, one), dev.alloc, "first run")
    b = dev.run(ctx, one, dev.alloc)                           # into the same arrays
    for name in ("sel", "src", "sel_off", "ncand"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    dev.fresh()
    _same(dev.run(ctx, two, dev.alloc), W.window_select_ref(piece, off, len(piece), out, two), dev.alloc, "other parameters")
    dev.fresh()
    c = dev.run(ctx, one, dev.alloc)
    for name in ("sel", "src", "sel_off", "ncand"):
        assert np.array_equal(getattr(a, name), getattr(c, name)), name


# ---- 8. the chain ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_resident_chain_with_the_selection_in_place(ctx):
    """align_batch on twelve reads over one 300-base draft, two of them random queries; then windows, pieces, the selection (max_depth 5, identity
    7 / 10), guides, MSA, consensus and stitch on the resident buffers at w = 50, with d_sel and d_sel_off where the pieces went and the ORIGINAL
    d_bases.  The stitched sequence, words and records equal those of the host-pointer calls on Context.window_select's output, and those of the same
    calls on a piece list filtered by window_select_ref."""
    import torch
    import bsalign_amd as B
    import window_stitch_cases as WS
    from window_msa_cases import CNS_WINDOW_DTYPE, PAR7
    W.need_symbols()
    w, md, ident, min_cov = 50, 5, (7, 10), 1
    rng = np.random.default_rng(4108)
    draft = rng.integers(0, 4, 300).astype(np.uint8)
    pairs = [(S.mutate(rng, draft, 0.10), draft) if k not in (3, 8) else (rng.integers(0, 4, 290).astype(np.uint8), draft) for k in range(12)]
    n = len(pairs)
    out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, 64, 2, -6, -3, -2, 0, 0))
    low = [k for k in range(n) if int(out[k]["mat"]) * ident[1] < ident[0] * int(out[k]["aln"])]
    assert low == [3, 8], low
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(c) for c in cigs], dtype=np.uint64)
    arena = np.concatenate(cigs).astype(np.uint32)
    ins = int(sum(int(x) >> 4 for c in cigs for x in c if int(x) & 15 == 1))
    gbase, nwin = B.window_gbase([0] * n, [len(draft)], w)
    win_cap = B.cigar_windows_bound(tlen, w)
    piece_cap, bases_cap, pcig_cap = win_cap, int(qlen.sum()), B.piece_cigars_bound(coff, win_cap)
    doff, dlen = B.window_drafts([int(toff[0])], [len(draft)], w)
    cols_cap, out_cap = (nwin * w + ins) * (n + 4), nwin * w + ins
    d_seqs, d_qoff, d_qlen, d_out, d_cig, d_coff, d_gbase, d_doff, d_dlen = (_upload(x) for x in (np.concatenate([seqs, np.zeros(8, np.uint8)]), qoff, qlen, out, arena, coff, gbase,
                                                                                                  doff, dlen))
    d_win, d_woff = _filled(16 * win_cap), _filled(8 * (n + 1))
    d_piece, d_poff, d_bases, d_boff = _filled(32 * piece_cap), _filled(8 * (nwin + 1)), _filled(bases_cap), _filled(8 * (nwin + 1))
    d_sel, d_soff, d_src, d_nc = _filled(32 * piece_cap), _filled(8 * (nwin + 1)), _filled(4 * piece_cap), _filled(4 * nwin)
    d_pcig, d_pcoff = _filled(4 * pcig_cap), _filled(8 * (piece_cap + 1))
    d_cols, d_cwoff, d_cwin = _filled(cols_cap), _filled(8 * (nwin + 1)), _filled(40 * nwin)
    par = B.SELECT_PARAMS(md, 0, ident[0], ident[1], 0)
    ctx.cigar_windows_run(d_out, d_cig, d_coff, n, w, d_win, win_cap, d_woff)
    ctx.window_pieces_run(d_seqs, d_qoff, d_qlen, d_win, d_woff, n, w, d_gbase, nwin, 0, d_piece, piece_cap, d_poff, d_bases, bases_cap, d_boff)
    ctx.window_select_run(d_piece, d_poff, nwin, piece_cap, d_out, n, par, d_sel, piece_cap, d_soff, d_src, d_nc)
    ctx.piece_cigars_run(d_out, d_cig, d_coff, n, d_sel, d_soff[8 * nwin:], piece_cap, d_pcig, pcig_cap, d_pcoff, None)
    ctx.window_msa_run(d_sel, d_soff, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w, 0, 0, d_cols, cols_cap, d_cwoff, d_cwin)
    model = ctx.cns_model(PAR7)
    d_cns, d_qlt, d_alt, d_clen, d_status = _filled(out_cap), _filled(out_cap), _filled(out_cap), _filled(4 * nwin), _filled(4 * nwin)
    ctx.window_cns_run(model, d_cols, cols_cap, d_cwin, nwin, n, d_cns, d_qlt, d_alt, out_cap, d_clen, None, d_status)
    d_seq, d_sq, d_sa, d_scig = _filled(out_cap), _filled(out_cap), _filled(out_cap), _filled(4 * out_cap)
    d_sqoff, d_cgoff, d_rec = _filled(8 * (nwin + 1)), _filled(8 * (nwin + 1)), _filled(32 * nwin)
    ctx.window_stitch_run(d_cols, cols_cap, d_cwin, nwin, d_status, min_cov, d_seq, d_sq, d_sa, out_cap, d_sqoff, d_scig, out_cap, d_cgoff, d_rec)
    ctx.sync()
    torch.cuda.synchronize()
    model.close()
    seq_off, cig_off = _down(d_sqoff, 8 * (nwin + 1), np.uint64), _down(d_cgoff, 8 * (nwin + 1), np.uint64)
    ns, nc = int(seq_off[nwin]), int(cig_off[nwin])
    seq, words, rec = _down(d_seq, ns, np.uint8), _down(d_scig, 4 * nc, np.uint32), _down(d_rec, 32 * nwin, WS.STITCH_DTYPE)
    cwin = _down(d_cwin, 40 * nwin, CNS_WINDOW_DTYPE)
    sel_off, ncand = _down(d_soff, 8 * (nwin + 1), np.uint64), _down(d_nc, 4 * nwin, np.uint32)
    assert np.all(_down(d_status, 4 * nwin, np.uint32) == 0) and cwin["nall"].tolist() == [md + 1] * nwin and ncand.tolist() == [10] * nwin
    # the selection itself, against the reference on the resident pieces
    piece, poff = _down(d_piece, 32 * piece_cap, W.PIECE_DTYPE), _down(d_poff, 8 * (nwin + 1), np.uint64)
    refp = W.window_select_ref(piece, poff, piece_cap, out, Par(md, 0, ident[0], ident[1], 0))
    assert np.array_equal(sel_off, refp.sel_off) and np.array_equal(_down(d_sel, 32 * piece_cap, W.PIECE_DTYPE)[:int(sel_off[nwin])], refp.sel)
    assert np.array_equal(_down(d_src, 4 * piece_cap, np.uint32)[:int(sel_off[nwin])], refp.src) and not set(refp.sel["pair"].tolist()) & {3, 8}
    # the host-pointer calls on Context.window_select's output, and on a piece list filtered by the reference
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(pairs, wins, w, gbase, nwin)
    selected, src = ctx.window_select(wp, max_depth=md, min_ident=ident, results=out)
    hp, hoff = W.batch([ps.tolist() for ps, _ in wp])
    href = W.window_select_ref(hp, hoff, len(hp), out, Par(md, 0, ident[0], ident[1], 0))
    by_ref = [(wp[g][0][href.win[g]], [wp[g][1][int(j)] for j in href.win[g]]) for g in range(nwin)]
    drafts = [draft[g * w:(g + 1) * w] for g in range(nwin)]
    for what, pieces in (("Context.window_select", selected), ("window_select_ref", by_ref)):
        msas = ctx.window_msa(pieces, ctx.piece_cigars(out, cigs, pieces), drafts, w, vote=False)
        res, _ = ctx.window_cns(msas, PAR7)
        per, (hseq, hsq, hsa, hsoff, hcig, hcgoff) = ctx.window_stitch(res, min_cov=min_cov)
        assert np.array_equal(hsoff, seq_off) and np.array_equal(hcgoff, cig_off), what
        assert np.array_equal(hseq, seq) and np.array_equal(hcig, words), what
        assert [r.tolist() for _, _, _, _, r in per] == [r.tolist() for r in rec], what
    for g in range(nwin):
        assert np.array_equal(src[g], href.win[g]) and np.array_equal(selected[g][0], by_ref[g][0]), g
        assert all(np.array_equal(a, b) for a, b in zip(selected[g][1], by_ref[g][1])), g


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_windows(ctx):
    import torch
    import bsalign_amd as B
    W.need_symbols()
    piece, off, par, full = _arena_case()
    need, nwin = int(full.sel_off[-1]), len(off) - 1
    out = W.results([(9, 10)] * 60)
    dev = _Dev(piece, off, len(piece), out, 60, need)
    run, batch, err = B.lib().bsa_window_select_run, B.lib().bsa_window_select_batch, B.lib().bsa_last_error
    rargs = [ctx.h] + dev.pointers(par, need)
    h = Got()
    h.sel, h.src, h.soff, h.nc = np.full(32 * need, FILL, np.uint8), np.full(need, FILL32, np.uint32), np.zeros(nwin + 1, np.uint64), np.zeros(nwin, np.uint32)
    bargs = [ctx.h, B._p(piece), B._p(off), nwin, len(piece), B._p(out), 60, C.byref(_params(par)), B._p(h.sel), need, B._p(h.soff), B._p(h.src), B._p(h.nc)]

    def refused(fn, base, changes):
        a = list(base)
        for i, v in changes.items():
            a[i] = v
        assert fn(*a) == E_ARG, (fn.__name__, changes)
        if 0 not in changes:
            assert err(ctx.h), (fn.__name__, changes)
    for fn, base in ((run, rargs), (batch, bargs)):
        # no context, records (with a cap), offsets (with windows), parameters, arena (with a cap), sel_off
        for i in (0, 1, 2, 7, 8, 10):
            refused(fn, base, {i: None})
        refused(fn, base, {8: None, 9: 0})                     # d_sel_src without d_sel
        refused(fn, base, {5: None, 7: C.byref(_params(par._replace(ident_num=1, ident_den=2)))})          # an identity test without d_out
        for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            refused(fn, base, {7: C.byref(_params(par, reserved=r))})
        for i in (3, 4, 6, 9):                                 # nwin, piece_cap, n, sel_cap
            refused(fn, base, {i: 0xFFFFFFF1})
    # nothing was launched by the refused calls; the good calls still run
    assert np.all(h.sel == FILL) and np.all(h.src == FILL32)
    assert run(*rargs) == 0
    ctx.sync()
    _same(dev.read(), full, need, "after the refused calls")
    assert batch(*bargs) == 0
    h.sel_off, h.ncand = h.soff, h.nc
    _same(h, full, need, "batch after the refused calls")
    # no windows: sel_off[0] = 0 and nothing else; NULL is fine where there is no work
    dev.fresh()
    a = [ctx.h] + dev.pointers(par, need)
    a[3] = 0
    assert run(*a) == 0
    ctx.sync()
    got = dev.read()
    assert got.sel_off.tolist()[:2] == [0, FILL64] and np.all(got.sel == FILL) and np.all(got.src == FILL32) and np.all(got.ncand == FILL32)
    o = np.full(2, FILL64, np.uint64)
    assert batch(ctx.h, None, None, 0, 0, None, 0, C.byref(_params(Par())), None, 0, B._p(o), None, None) == 0 and o.tolist() == [0, FILL64]
    d_off = _filled(16)
    assert run(ctx.h, None, None, 0, 0, None, 0, C.byref(_params(Par())), None, 0, C.c_void_p(d_off.data_ptr()), None, None) == 0
    ctx.sync()
    assert _down(d_off, 16, np.uint64).tolist() == [0, FILL64]
    # the Python plumbing's size checks
    t = lambda nbytes: torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    good = dict(d_piece=t(32 * len(piece)), d_piece_off=t(8 * (nwin + 1)), d_out=t(40 * 60), d_sel=t(32 * need), d_sel_off=t(8 * (nwin + 1)), d_sel_src=t(4 * need), d_ncand=t(4 * nwin))
    call = lambda **kw: ctx.window_select_run(kw["d_piece"], kw["d_piece_off"], nwin, len(piece), kw["d_out"], 60, _params(Par()), kw["d_sel"], need, kw["d_sel_off"],
                                              kw["d_sel_src"], kw["d_ncand"])
    call(**good)
    for k in good:
        with pytest.raises(ValueError):
            call(**dict(good, **{k: good[k][:-1]}))
