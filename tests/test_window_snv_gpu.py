"""GPU: bsa_snv_model_create, bsa_window_snv_run and bsa_window_snv_batch (include/bsalign_hip.h) against bsa_msa_call_snvs window by window: the
fixture of the real reference, hand-made batches at the smallest shapes at which the kernels can go wrong, every way a record fails and every
status, any capacity of the arena, re-runs with other parameters, the whole chain from align_batch on a diploid sample, and the argument errors.

Tolerance: none.  Window records, offsets and SNV records are compared byte for byte.

Every buffer a run writes is prefilled with 0xA5 bytes and the arena has 256 guard bytes on either side; the columns are uploaded into an allocation
of exactly their size.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import snv_cases as SC
from window_msa_cases import CNS_WINDOW_DTYPE, PAR7

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5
E_ARG, E_CIGAR_CAP, E_UNSUPPORTED = -2, -5, -6
_MODELS = {}


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


def _model(ctx, max_rows):
    key = (id(ctx), max_rows)
    if key not in _MODELS:
        _MODELS[key] = ctx.snv_model(max_rows)
    return _MODELS[key]


def _host_call(cols, nall, nseq, par):
    import bsalign_amd.msa as MSA
    return MSA.call_snvs(cols, nall, nseq, par)


class Got:
    pass


def _run(ctx, blob, rec, cst, max_rows, par, cap, alloc=None, cols_cap=None, null=False):
    """bsa_window_snv_run on resident buffers -> Got (the arena between guards)"""
    import torch
    import bsalign_amd as B
    n = len(rec)
    alloc = cap if alloc is None else alloc
    cols_cap = len(blob) if cols_cap is None else cols_cap
    d_cols, d_cwin = _upload(blob), _upload(rec)
    d_cst = None if cst is None else _upload(np.asarray(cst, dtype=np.uint32))
    d_snv, d_off, d_rec = _filled(24 * alloc + 2 * GUARD), _filled(8 * (n + 1)), _filled(16 * n)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    par = np.ascontiguousarray(par, dtype=SC.SNV_PARAMS)
    rc = B.lib().bsa_window_snv_run(ctx.h, _model(ctx, max_rows).h, p(d_cols), cols_cap, p(d_cwin), n, None if d_cst is None else p(d_cst), B._p(par),
                                    None if null else p(d_snv, GUARD), cap, p(d_off), p(d_rec))
    assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
    ctx.sync()
    torch.cuda.synchronize()
    g = Got()
    w = d_snv.cpu().numpy()
    assert np.all(w[:GUARD] == FILL) and np.all(w[GUARD + 24 * alloc:] == FILL), "a guard byte of the arena was written"
    g.snv = w[GUARD:GUARD + 24 * alloc].copy()
    g.off = d_off.cpu().numpy()[:8 * (n + 1)].view(np.uint64).copy()
    g.rec = d_rec.cpu().numpy()[:16 * n].view(SC.SNV_WINDOW_DTYPE).copy()
    assert np.array_equal(d_cols.cpu().numpy()[:len(blob)], blob), "the columns are read-only"
    return g


def _batch(ctx, blob, rec, cst, max_rows, par, cap, alloc=None, cols_cap=None, null=False):
    """bsa_window_snv_batch on host arrays prefilled with 0xA5 -> (rc, Got)"""
    import bsalign_amd as B
    n = len(rec)
    alloc = cap if alloc is None else alloc
    cols_cap = len(blob) if cols_cap is None else cols_cap
    g = Got()
    cols = np.ascontiguousarray(blob).copy()
    g.snv = np.full(max(24 * alloc, 1), FILL, np.uint8)
    g.off = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    g.rec = np.full(16 * max(n, 1), FILL, np.uint8)
    cst = None if cst is None else np.ascontiguousarray(cst, dtype=np.uint32)
    par = np.ascontiguousarray(par, dtype=SC.SNV_PARAMS)
    rc = B.lib().bsa_window_snv_batch(ctx.h, max_rows, B._p(cols) if len(blob) else None, cols_cap, B._p(rec), n, None if cst is None else B._p(cst), B._p(par),
                                      None if null else B._p(g.snv), cap, B._p(g.off), B._p(g.rec))
    g.snv, g.rec = g.snv[:24 * alloc], g.rec[:16 * n].view(SC.SNV_WINDOW_DTYPE)
    assert np.array_equal(cols, blob), "the columns are read-only"
    return rc, g


def _same(got, want, cap, what):
    """the house arena contract: offsets and window records of a complete run; window g's records written, whole, iff off[g + 1] <= cap; nothing else"""
    snv, off, wrec = want
    assert np.array_equal(got.off, off), (what, "offsets", got.off, off)
    assert got.rec.tobytes() == wrec.tobytes(), (what, "window records", got.rec, wrec)
    exp = np.full(len(got.snv), FILL, np.uint8)
    for g in range(len(wrec)):
        a, b = int(off[g]), int(off[g + 1])
        if b <= cap and b > a:
            exp[24 * a:24 * b] = snv[a:b].view(np.uint8)
    bad = np.flatnonzero(got.snv != exp)
    assert len(bad) == 0, (what, "records", bad[:8] // 24, got.snv[bad[:8]], exp[bad[:8]])


def _both(ctx, windows, par, what, max_rows=None, cst=None, gap=0, slack=2):
    """_run and _batch against bsa_msa_call_snvs with an arena of the need (+ slack in the allocation) -> (want, blob, rec)"""
    blob, rec = SC.pack(windows, gap)
    if max_rows is None:
        max_rows = max([int(w["nseq"]) for w in rec] + [1])
    want = SC.window_snv_expect(blob, rec, len(blob), cst, max_rows, par, _host_call)
    need = int(want[1][-1])
    _same(_run(ctx, blob, rec, cst, max_rows, par, need, need + slack), want, need, what + " (run)")
    rc, h = _batch(ctx, blob, rec, cst, max_rows, par, need, need + slack)
    assert rc == 0, (what, rc)
    _same(h, want, need, what + " (batch)")
    return want, blob, rec


# ---- 1. the examples and the fixture ---------------------------------------------------------------------------------------------------------------------
def test_header_example(ctx):
    SC.need_symbols()
    rows = [[0, 0, 0, 0, 0], [1, 1, 3, 3, 1], [4, 4, 5, 2, 4], [2, 2, 2, 0, 2], [3, 6, 6, 6, 3]]
    cols = np.array([r + [0, 0] for r in rows], dtype=np.uint8)
    (snv, off, wrec), blob, rec = _both(ctx, [(cols, 4)], SC.params(1, 0.5, 1, 0), "header", max_rows=4)
    assert len(blob) == 35 and off.tolist() == [0, 2] and wrec.tolist() == [(0, 2, 3, np.float32(0.01))]
    assert snv.tolist() == [(1, 1, 1, 3, 4, 2, 2, 1, 3), (3, 2, 3, 1, 4, 3, 1, 2, 0)]


def test_fixture_of_the_reference_replayed(ctx):
    """all sets of tests/golden/snv.npz as one batch, skip_first_row 1: the records are the reference's SNP lines"""
    SC.need_symbols()
    gold = SC.golden()
    (snv, off, wrec), _, _ = _both(ctx, [(cols, nseq) for cols, nall, nseq, _, _, _ in gold], SC.params(skip_first_row=1), "fixture")
    for g, (cols, nall, nseq, snp, recs, prob) in enumerate(gold):
        mine = np.array([[int(r[f]) for f in SC.GOLDEN_FIELDS] for r in snv[int(off[g]):int(off[g + 1])]], dtype=np.int64).reshape(-1, 8)
        assert np.array_equal(mine, recs) and int(round(float(wrec[g]["pexp"]) * 10000)) == prob, g
    assert sum(1 for w in wrec if w["pexp"] != np.float32(0.01)) >= 3


# ---- 2. hand-made batches ----------------------------------------------------------------------------------------------------------------------------------
def test_depths(ctx):
    """nseq on both sides of 20 (the grid), of a dword, of the wave and of what fits a tile; nall equal to and above nseq; 1001 is too deep"""
    SC.need_symbols()
    rng = np.random.default_rng(31)
    windows = []
    for nseq in (1, 2, 3, 20, 21, 63, 64, 65, 255, 256, 257, 1000):
        for extra in (0, 1 + nseq % 3):
            mlen = 70 if nseq <= 257 else 21
            windows.append((SC.random_window(rng, mlen, nseq + extra, nseq, err=0.03, nhet=4), nseq))
    windows.append((SC.random_window(rng, 5, 1001, 1001), 1001))
    windows.append((SC.random_window(rng, 40, 9000, 30), 30))              # a column that does not fit the tile: the lanes go over the rows
    windows.append((SC.random_window(rng, 200, 41, 40, err=0.05, nhet=6), 40))
    for par in (SC.params(), SC.params(1, 0.2, 0, 1)):
        (snv, off, wrec), _, _ = _both(ctx, windows, par, "depths", max_rows=1000, gap=5)
        assert wrec["status"].tolist() == [0] * 24 + [SC.ST_TOO_DEEP, 0, 0] and int(off[-1]) > 20
        assert sum(1 for w in wrec if w["status"] == 0 and w["pexp"] != np.float32(0.01)) >= 4


def test_lengths(ctx):
    """mlen 0, 1, on both sides of a tile and of two, and the longest the histogram's counters take; 65536 is too long"""
    SC.need_symbols()
    rng = np.random.default_rng(32)
    windows = [(SC.random_window(rng, mlen, 30, 28, err=0.04, nhet=min(mlen, 5)), 28) for mlen in (0, 1, 63, 64, 65, 129)]
    long_ = np.zeros((65535, 4), dtype=np.uint8)
    long_[:, 0] = rng.integers(0, 6, 65535)
    long_[:, 1] = rng.integers(0, 5, 65535)
    windows += [(long_, 1), (np.zeros((65536, 4), dtype=np.uint8), 1)]
    (snv, off, wrec), _, _ = _both(ctx, windows, SC.params(0, 0.0, 0, 0), "lengths", max_rows=28, gap=3)
    assert wrec["status"].tolist() == [0] * 7 + [SC.ST_TOO_LONG] and wrec["nsnv"][0] == 0


def test_calls_at_tile_borders_and_three_coordinates(ctx):
    """calls in the first and the last column and on both sides of a tile border, between insertion columns (consensus a gap, last row a gap or a
    base) so that mpos, cpos and lpos all differ"""
    SC.need_symbols()
    nall, nseq, mlen = 13, 12, 200
    cols = np.zeros((mlen, nall + 3), dtype=np.uint8)
    cols[:, :nseq] = 2
    cols[:, nseq] = 1
    cols[:, nall] = 2
    for i in range(5, mlen, 7):                                 # consensus gap, draft base
        cols[i, :nseq] = 4
        cols[i, nall] = 4
    for i in range(3, mlen, 11):                                # consensus base, draft gap
        cols[i, nseq] = 4
    het = [0, 62, 63, 64, 65, 127, 128, 199]
    for i in het:
        cols[i, :nseq] = [2] * 6 + [3] * 6
        cols[i, nall] = 2
    (snv, off, wrec), _, _ = _both(ctx, [(cols, nseq), (cols[:64].copy(), nseq), (cols[:65].copy(), nseq)], SC.params(), "borders")
    mine = snv[:int(off[1])]
    assert mine["mpos"].tolist() == het and all(len({int(v["mpos"]), int(v["cpos"]), int(v["lpos"])}) == 3 for v in mine[2:])
    assert snv[int(off[1]):int(off[2])]["mpos"].tolist() == [0, 62, 63] and snv[int(off[2]):]["mpos"].tolist() == [0, 62, 63, 64]


def test_no_windows(ctx):
    SC.need_symbols()
    rec = np.zeros(0, dtype=CNS_WINDOW_DTYPE)
    got = _run(ctx, np.zeros(0, np.uint8), rec, None, 4, SC.params(), 0, 2)
    assert got.off.tolist() == [0] and np.all(got.snv == FILL)
    rc, h = _batch(ctx, np.zeros(0, np.uint8), rec, None, 4, SC.params(), 0, 2)
    assert rc == 0 and h.off.tolist() == [0] and np.all(h.snv == FILL)


# ---- 3. records and statuses -------------------------------------------------------------------------------------------------------------------------------
def test_every_way_a_record_fails_and_every_status(ctx):
    SC.need_symbols()
    rng = np.random.default_rng(33)
    good = SC.random_window(rng, 90, 25, 24, err=0.04, nhet=5)
    blob, rec = SC.pack([(good, 24)] * 12)
    n = len(blob)
    rec[1]["idxs_off"] = 0
    rec[2]["nall"] = 0
    rec[3]["mlen"] = 1 << 28
    rec[4]["cols_off"] = n - good.size + 1                    # one byte past the end
    rec[5]["cols_off"] = (1 << 64) - 8                        # the sum wraps
    rec[6]["nseq"] = 26                                       # above nall
    rec[7]["nseq"] = 25                                       # nall itself: fine, the last row votes
    rec[8]["nall"] = 0xFFFFFFFF
    cst = [0] * 12
    cst[9], cst[10], cst[11] = 1, 2, 3
    for cols_cap in (n, n - 1):
        want = SC.window_snv_expect(blob, rec, cols_cap, cst, 25, SC.params(), _host_call)
        bad = [SC.ST_BAD_RECORD] * 6
        assert want[2]["status"].tolist() == [0] + bad + [0, SC.ST_BAD_RECORD] + [SC.ST_NOT_CALLED] * 3 if cols_cap == n else want[2]["status"][0] == 0
        need = int(want[1][-1])
        _same(_run(ctx, blob, rec, cst, 25, SC.params(), need, need + 1, cols_cap=cols_cap), want, need, "records (run)")
        rc, h = _batch(ctx, blob, rec, cst, 25, SC.params(), need, need + 1, cols_cap=cols_cap)
        assert rc == 0
        _same(h, want, need, "records (batch)")
    # the model's depth decides what is too deep
    want = SC.window_snv_expect(blob, rec[:1], n, None, 23, SC.params(), _host_call)
    assert want[2]["status"].tolist() == [SC.ST_TOO_DEEP]
    _same(_run(ctx, blob, rec[:1], None, 23, SC.params(), 4), want, 4, "too deep for the model")


# ---- 4. the arena ----------------------------------------------------------------------------------------------------------------------------------------------
def _arena_case():
    rng = np.random.default_rng(34)
    windows = [(SC.random_window(rng, 80, 25, 24, err=0.03, nhet=k), 24) for k in (3, 0, 5, 2, 4)]
    blob, rec = SC.pack(windows)
    want = SC.window_snv_expect(blob, rec, len(blob), None, 24, SC.params(2, 0.3, 1, 0), _host_call)
    off = want[1]
    assert off[1] > 1 and off[2] == off[1] and off[5] > off[3] + 1
    return blob, rec, want


def test_any_capacity(ctx):
    """seven capacities around the window borders; a count-only run; NULL arenas"""
    SC.need_symbols()
    blob, rec, want = _arena_case()
    off, par = want[1], SC.params(2, 0.3, 1, 0)
    need = int(off[-1])
    for cap in (0, int(off[1]) - 1, int(off[1]), int(off[1]) + 1, int(off[3]), need - 1, need):
        _same(_run(ctx, blob, rec, None, 24, par, cap, need + 1), want, cap, "cap %d (run)" % cap)
        rc, h = _batch(ctx, blob, rec, None, 24, par, cap, need + 1)
        assert rc == (0 if cap >= need else E_CIGAR_CAP), (cap, rc)
        if rc == 0:
            _same(h, want, cap, "cap %d (batch)" % cap)
        else:
            assert np.array_equal(h.off, off) and h.rec.tobytes() == want[2].tobytes() and np.all(h.snv == FILL), cap
    _same(_run(ctx, blob, rec, None, 24, par, 0, need, null=True), want, 0, "count only (run)")
    rc, h = _batch(ctx, blob, rec, None, 24, par, 0, need, null=True)
    assert rc == E_CIGAR_CAP and np.array_equal(h.off, off) and np.all(h.snv == FILL)


def test_two_runs_with_other_parameters_on_one_context(ctx):
    SC.need_symbols()
    blob, rec, _ = _arena_case()
    for par in (SC.params(), SC.params(1, 0.1, 0, 1), SC.params(5, 0.9, 20, 0), SC.params()):
        want = SC.window_snv_expect(blob, rec, len(blob), None, 24, par, _host_call)
        need = int(want[1][-1])
        _same(_run(ctx, blob, rec, None, 24, par, need, need + 3), want, need, "run with %s" % (par.tolist(),))


# ---- 5. the chain ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [50, 500])
def test_whole_chain_from_align_batch_on_a_diploid_sample(ctx, w):
    """a draft with small edits, ten error-free reads of each of two haplotypes, aligned by align_batch, through windows, pieces, guides, MSA and
    consensus: the calls, as window * w + lpos, are the planted sites with ten reads on either side"""
    import bsalign_amd as B
    SC.need_symbols()
    truth, hap2, draft, ws, sites, reads, rec, rng = SC.diploid_loop(11, w)
    pairs = [(r, draft) for r in reads]
    n = len(pairs)
    out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, 64, 2, -6, -3, -2, 0, 0))
    assert np.all(st == 0)
    gbase, nwin = B.window_gbase([0] * n, [len(draft)], w)
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(pairs, wins, w, gbase, nwin)
    msas = ctx.window_msa(wp, ctx.piece_cigars(out, cigs, wp), [draft[g * w:(g + 1) * w] for g in range(nwin)], w, vote=False)
    res, _ = ctx.window_cns(msas, PAR7)
    per, (snv, off) = ctx.window_snv(res)
    called = []
    for g, (v, r) in enumerate(per):
        cols = res[g][5]
        hv, hp, hs = _host_call(cols, cols.shape[1] - 3, cols.shape[1] - 4, SC.params())
        assert v.tobytes() == hv.tobytes() and r.tolist() == (0, len(hv), hs, np.float32(hp)), g
        assert all(int(x["refn"]) == 10 and int(x["altn"]) == 10 for x in v)
        called += [g * w + int(x["lpos"]) for x in v]
    assert called == sites and int(off[nwin]) == len(sites)


# ---- 6. the argument errors ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    SC.need_symbols()
    L = B.lib()
    blob, rec, _ = _arena_case()
    par = SC.params()
    want = SC.window_snv_expect(blob, rec, len(blob), None, 24, par, _host_call)
    n, need = len(rec), int(want[1][-1])
    assert need >= 2
    d_cols, d_cwin, d_snv, d_off, d_rec = _upload(blob), _upload(rec), _filled(24 * need), _filled(8 * (n + 1)), _filled(16 * n)
    p = lambda t: C.c_void_p(t.data_ptr())
    m = _model(ctx, 24)
    good = [ctx.h, m.h, p(d_cols), len(blob), p(d_cwin), n, None, B._p(par), p(d_snv), need, p(d_off), p(d_rec)]
    assert L.bsa_window_snv_run(*good) == 0
    ctx.sync()
    other = B.Context(0)
    try:
        foreign = other.snv_model(4)
        bad = {"ctx": (0, None), "model": (1, None), "another context's model": (1, foreign.h), "cols": (2, None), "cwin": (4, None), "par": (7, None),
               "snv": (8, None), "snv_off": (10, None), "rec": (11, None), "nwin": (5, 0xFFFFFFF1), "skip_first_row": (7, B._p(SC.params(skip_first_row=2))),
               "min_covfrq": (7, B._p(SC.params(min_covfrq=-1.0)))}
        keep = [SC.params(skip_first_row=2), SC.params(min_covfrq=-1.0)]
        bad["skip_first_row"], bad["min_covfrq"] = (7, B._p(keep[0])), (7, B._p(keep[1]))
        for what, (i, v) in bad.items():
            args = list(good)
            args[i] = v
            assert L.bsa_window_snv_run(*args) == E_ARG, what
        h_snv, h_off, h_rec = np.zeros(need, SC.SNV_DTYPE), np.zeros(n + 1, np.uint64), np.zeros(n, SC.SNV_WINDOW_DTYPE)
        hgood = [ctx.h, 24, B._p(blob), len(blob), B._p(rec), n, None, B._p(par), B._p(h_snv), need, B._p(h_off), B._p(h_rec)]
        assert L.bsa_window_snv_batch(*hgood) == 0 and h_snv.tobytes() == want[0].tobytes()
        for what, (i, v) in {"ctx": (0, None), "cols": (2, None), "cwin": (4, None), "par": (7, None), "snv": (8, None), "snv_off": (10, None), "rec": (11, None),
                             "skip_first_row": (7, B._p(keep[0]))}.items():
            args = list(hgood)
            args[i] = v
            assert L.bsa_window_snv_batch(*args) == E_ARG, what
        args = list(hgood)
        args[1] = 1001
        assert L.bsa_window_snv_batch(*args) == E_UNSUPPORTED
        h = C.c_void_p()
        assert L.bsa_snv_model_create(ctx.h, 1001, C.byref(h)) == E_UNSUPPORTED and not h.value
        assert L.bsa_snv_model_create(None, 4, C.byref(h)) == E_ARG and L.bsa_snv_model_create(ctx.h, 4, None) == E_ARG
        L.bsa_snv_model_destroy(None)
    finally:
        other.close()
    # the run after the errors is the run before them
    _same(_run(ctx, blob, rec, None, 24, par, need), want, need, "after the errors")
