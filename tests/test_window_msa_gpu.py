"""GPU: bsa_window_msa_batch and bsa_window_msa_run (include/bsalign_hip.h) bit for bit against the Python statement of the definition
(window_msa_cases.window_msa_ref): the offsets, every field of every record and every byte, on hand-made windows uploaded directly, on dead pieces,
for any arena capacity, on what the aligners give through all four passes, and with the loop closed by the device consensus caller.  Every buffer a
run writes is prefilled with 0xA5 bytes and the column arena has 256 guard bytes on either side, so that a byte a run leaves unwritten, or one it
writes where it must not, shows.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import support as S
import window_msa_cases as W

pytestmark = pytest.mark.gpu

GUARD = 256                        # guard bytes around the column arena
FILL = 0xA5
FILL64 = 0xA5A5A5A5A5A5A5A5
E_ARG, E_CIGAR_CAP, E_UNSUPPORTED = -2, -5, -6
SEQ2BIT = 0x800
_BATCHES, _REFS = {}, {}
BATCH_NAMES = ["header_example", "depths", "depths_eqx", "draft_lengths", "window_1", "window_500", "window_4096", "shapes", "no_windows", "draft_offsets", "deep_windows"]
DEAD_NAMES = ["dead", "words_behind_the_cap", "offsets_decrease", "above_piece_cap", "decreasing"]


def _need():
    """every test here is about bsa_window_msa_*: without its symbols in the library none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in ("bsa_window_msa_run", "bsa_window_msa_batch", "bsa_window_msa_bound"):
        assert hasattr(B.lib(), name), "the library does not export " + name


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


def _named(name, vote=0):
    """(the batch, (cols_off, records, bytes)): the reference computed once"""
    _need()
    if not _BATCHES:
        _BATCHES.update(W.hand_batches())
        _BATCHES["dead"] = W.dead_batch()[0]
        _BATCHES.update(W.dead_offsets_batches())
        _BATCHES.update(W.piece_off_batches())
        _BATCHES["arena"] = W.arena_batch()
    if (name, vote) not in _REFS:
        _REFS[(name, vote)] = W.window_msa_ref(_BATCHES[name], vote)
    return _BATCHES[name], _REFS[(name, vote)]


def _ptr(a):
    import bsalign_amd as B
    return B._p(a) if a is not None and a.size else None


def _draft(b, packed):
    return W.pack2bit(b.draft) if packed else b.draft


def _batch(ctx, b, cap, vote=0, packed=False, alloc=None, null=False):
    """bsa_window_msa_batch -> (rc, cols_off, records, the whole host arena), all prefilled with 0xA5"""
    import bsalign_amd as B
    cols = np.full(max(alloc if alloc is not None else cap, 1), FILL, dtype=np.uint8)
    off = np.full(b.nwin + 1, FILL64, dtype=np.uint64)
    cwin = np.full(max(b.nwin, 1) * 40, FILL, dtype=np.uint8).view(W.CNS_WINDOW_DTYPE)
    rc = B.lib().bsa_window_msa_batch(ctx.h, _ptr(b.piece), B._p(b.piece_off), b.nwin, b.piece_cap, _ptr(b.bases), b.bases_cap, _ptr(b.pcig), b.pcig_cap, B._p(b.pcig_off),
                                      B._p(_draft(b, packed)), _ptr(b.doff), _ptr(b.dlen), b.window, SEQ2BIT if packed else 0, vote,
                                      None if null else B._p(cols), cap, B._p(off), B._p(cwin))
    return rc, off, cwin[:b.nwin], cols


def _filled(nbytes):
    import torch
    return torch.full((max((nbytes + 15) // 16 * 16, 16),), FILL, dtype=torch.uint8, device="cuda")


def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.nbytes == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


class _Dev:
    """one batch on the device; the column arena of `alloc` bytes lies between two guards"""

    def __init__(self, b, alloc, packed=False):
        import torch
        self.b, self.alloc, self.packed = b, alloc, packed
        self.d_piece, self.d_poff, self.d_bases, self.d_pcig, self.d_pcoff = _upload(b.piece), _upload(b.piece_off), _upload(b.bases), _upload(b.pcig), _upload(b.pcig_off)
        self.d_draft, self.d_doff, self.d_dlen = _upload(_draft(b, packed)), _upload(b.doff), _upload(b.dlen)
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        self.d_cols = _filled(self.alloc + 2 * GUARD)
        self.d_coff = _filled((self.b.nwin + 1) * 8)
        self.d_cwin = _filled(max(self.b.nwin, 1) * 40)

    def pointers(self, cap, vote=0, null=False):
        b = self.b
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        return [p(self.d_piece), p(self.d_poff), b.nwin, b.piece_cap, p(self.d_bases), b.bases_cap, p(self.d_pcig), b.pcig_cap, p(self.d_pcoff), p(self.d_draft), p(self.d_doff),
                p(self.d_dlen), b.window, SEQ2BIT if self.packed else 0, vote, None if null else p(self.d_cols, GUARD), cap, p(self.d_coff), p(self.d_cwin)]

    def run(self, ctx, cap, vote=0, null=False):
        """-> (cols_off, records, the bytes of the arena proper); the guards are checked here"""
        import torch
        import bsalign_amd as B
        assert cap <= self.alloc and not (null and cap)
        rc = B.lib().bsa_window_msa_run(ctx.h, *self.pointers(cap, vote, null))
        assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        w = self.d_cols.cpu().numpy()[:self.alloc + 2 * GUARD]
        assert np.all(w[:GUARD] == FILL) and np.all(w[GUARD + self.alloc:] == FILL), "a guard byte was written"
        n = self.b.nwin
        return (self.d_coff.cpu().numpy()[:(n + 1) * 8].view(np.uint64).copy(), self.d_cwin.cpu().numpy()[:n * 40].view(W.CNS_WINDOW_DTYPE).copy(), w[GUARD:GUARD + self.alloc].copy())


def _check(got, ref, cap, what=""):
    """the arena contract: every offset and every field of every record exact; window g's bytes there iff its range ends inside the cap; every
    other byte of the allocation untouched.  -> the windows present"""
    off, cwin, cols = got
    roff, rcwin, rcols = ref
    assert np.array_equal(off, roff), (what, "cols_off", off[:8], roff[:8])
    for f in W.CNS_WINDOW_DTYPE.names:
        assert np.array_equal(cwin[f], rcwin[f]), (what, "cwin", f, np.flatnonzero(cwin[f] != rcwin[f])[:8])
    untouched = np.ones(len(cols), dtype=bool)
    present = 0
    for g in range(len(rcwin)):
        a, b = int(roff[g]), int(roff[g + 1])
        if b <= cap:
            bad = np.flatnonzero(cols[a:b] != rcols[a:b])
            assert len(bad) == 0, (what, "window %d" % g, "byte %d of %d, column bytes %d" % (bad[0], b - a, int(rcwin[g]["nall"]) + 3), cols[a:b][bad[:8]], rcols[a:b][bad[:8]])
            untouched[a:b] = False
            present += 1
    assert np.all(cols[untouched] == FILL), (what, "a byte outside the windows that fit was written", cap, np.flatnonzero(untouched & (cols != FILL))[:8])
    return present


def _both(ctx, b, ref, what, vote=0, packed=False):
    """_batch with the exact cap and _run with room to spare, each against the reference"""
    total = int(ref[0][-1])
    rc, off, cwin, cols = _batch(ctx, b, total, vote, packed, total + 7)
    assert rc == 0, (what, rc)
    assert _check((off, cwin, cols), ref, total, what + " (batch)") == b.nwin
    dev = _Dev(b, total + 7, packed)
    assert _check(dev.run(ctx, total + 7, vote), ref, total + 7, what + " (run)") == b.nwin
    return dev


# ---- 1. hand-made windows, uploaded directly ---------------------------------------------------------------------------------------------------
def test_every_hand_made_batch_is_run():
    _named("header_example")
    assert sorted(BATCH_NAMES + DEAD_NAMES + ["arena"]) == sorted(_BATCHES)


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_hand_made_batch(ctx, name):
    """both calls, both values of vote; the draft one base a byte with vote 0 and 2-bit packed with vote 1"""
    for vote, packed in ((0, False), (1, True)):
        b, ref = _named(name, vote)
        dev = _both(ctx, b, ref, "%s vote %d" % (name, vote), vote, packed)
        if name == "header_example":
            assert np.array_equal(dev.read()[2][:72], W.header_example()[1])
    if name == "draft_offsets":
        b, ref = _named(name, 0)
        _both(ctx, b, ref, name + " packed, vote 0", 0, True)


@pytest.mark.parametrize("name", DEAD_NAMES)
def test_dead_pieces_and_windows_without_rows(ctx, name):
    b, ref = _named(name, 0)
    dev = _both(ctx, b, ref, name)
    if name == "dead":
        _, names, at = W.dead_batch()
        cols = dev.read()[2][:int(ref[0][-1])].reshape(14, len(b.piece) + 4)
        for nm in names:
            assert np.all(cols[:, at[nm]] == 5), nm
        assert np.any(cols[:, 0] < 4)


def test_through_the_python_calls(ctx):
    """Context.window_msa on host arrays, Context.window_msa_run on torch tensors"""
    import torch
    b, ref = _named("depths", 1)
    roff, rcwin, rcols = ref
    wp, guides, drafts = [], [], []
    for g in range(b.nwin):
        x, y = int(b.piece_off[g]), int(b.piece_off[g + 1])
        ps = b.piece[x:y].copy()
        wp.append((ps, [b.bases[int(p["base_off"]):int(p["base_off"]) + int(p["len"])] for p in ps]))
        guides.append([(b.pcig[int(b.pcig_off[j]):int(b.pcig_off[j + 1])], 0) for j in range(x, y)])
        drafts.append(b.draft[int(b.doff[g]):int(b.doff[g]) + int(b.dlen[g])])
    for seq2bit in (False, True):
        got = ctx.window_msa(wp, guides, drafts, b.window, vote=True, seq2bit=seq2bit)
        assert len(got) == b.nwin
        for g, (cols, rec) in enumerate(got):
            assert cols.dtype == np.uint8 and cols.shape == (int(rcwin[g]["mlen"]), W.DEPTHS[g] + 4)
            assert np.array_equal(cols.reshape(-1), rcols[int(roff[g]):int(roff[g + 1])]), g
            assert rec.tolist() == rcwin[g].tolist(), g
    total = int(roff[-1])
    dev = _Dev(b, total)
    d_cols = dev.d_cols[GUARD:GUARD + total]
    args = [dev.d_piece, dev.d_poff, b.nwin, b.piece_cap, dev.d_bases, b.bases_cap, dev.d_pcig, b.pcig_cap, dev.d_pcoff, dev.d_draft, dev.d_doff, dev.d_dlen, b.window, 0, 1]
    ctx.window_msa_run(*args, d_cols, total, dev.d_coff, dev.d_cwin)
    ctx.sync()
    torch.cuda.synchronize()
    assert _check(dev.read(), ref, total, "resident") == b.nwin
    with pytest.raises(ValueError):
        ctx.window_msa_run(*args, d_cols, total + 1, dev.d_coff, dev.d_cwin)


# ---- 2. the arena contract ---------------------------------------------------------------------------------------------------------------------
def test_arena_contract_for_any_capacity(ctx):
    b, ref = _named("arena", 0)
    roff = ref[0]
    total = int(roff[-1])
    assert b.nwin == 7 and int(roff[3]) == int(roff[2]) and int(roff[6]) < total
    inside = int(roff[3]) + (int(roff[4]) - int(roff[3])) // 2          # ends inside window 3
    fits = lambda cap: sum(1 for g in range(b.nwin) if int(roff[g + 1]) <= cap)
    dev = _Dev(b, total + 1)
    for cap, null in ((0, False), (0, True), (int(roff[6]), False), (total - 1, False), (total, False), (total + 1, False), (inside, False)):
        dev.fresh()
        what = "cap %d%s" % (cap, " (NULL arena)" if null else "")
        got = dev.run(ctx, cap, null=null)
        present = _check(got, ref, cap, what)
        assert present == fits(cap), what
        if cap >= total:
            assert present == b.nwin
        elif cap == 0:
            assert np.all(got[2] == FILL), what
        else:
            assert 0 < present < b.nwin, what
    # twice into fresh buffers: the same bytes; a run after a short run on the same context is complete
    dev.fresh()
    one = dev.run(ctx, total)
    dev.fresh()
    _check(dev.run(ctx, inside), ref, inside, "short run")
    dev.fresh()
    two = dev.run(ctx, total)
    assert all(np.array_equal(x, y) for x, y in zip(one, two)) and _check(two, ref, total, "second run") == b.nwin


def test_batch_with_a_short_arena(ctx):
    import bsalign_amd as B
    b, ref = _named("arena", 1)
    total = int(ref[0][-1])
    for cap, null in ((0, False), (0, True), (1, False), (total - 1, False)):
        rc, off, cwin, cols = _batch(ctx, b, cap, 1, alloc=total, null=null)
        assert rc == E_CIGAR_CAP and np.array_equal(off, ref[0]) and cwin.tolist() == ref[1].tolist(), cap
        assert np.all(cols == FILL), cap
        assert B.lib().bsa_last_error(ctx.h), cap
    rc, off, cwin, cols = _batch(ctx, b, total, 1)
    assert rc == 0 and np.array_equal(cols, ref[2])


# ---- 3. what the aligners return, through all four passes --------------------------------------------------------------------------------------
_REAL = {}


def _real():
    """three drafts of 700, 520 and 130 bases; five reads a draft with about 10 % errors, each against the draft from a multiple of 500 on; every
    second read stored reverse-complemented and marked.  -> (drafts, pairs as stored, strands, pairs as aligned, target of each pair, its start)"""
    import bsalign_amd as B
    if not _REAL:
        rng = np.random.default_rng(811)
        drafts = [rng.integers(0, 4, n).astype(np.uint8) for n in (700, 520, 130)]
        pairs, strands, fwd, tid, start = [], [], [], [], []
        for d, T in enumerate(drafts):
            for j in range(5):
                a = 500 if (d == 0 and j % 2) else 0
                Q = S.mutate(rng, T[a:], 0.10)
                rev = len(pairs) % 2 == 1
                pairs.append((B.revcomp(Q) if rev else Q, T[a:]))
                fwd.append((Q, T[a:]))
                strands.append(rev); tid.append(d); start.append(a)
        _REAL["x"] = (drafts, pairs, strands, fwd, np.array(tid), np.array(start))
    return _REAL["x"]


@pytest.mark.parametrize("w", [50, 500])
@pytest.mark.parametrize("kind", ["align", "align_overlap", "align_eqx", "align_strands", "align_seq2bit", "align_overlap_eqx_strands_seq2bit", "edit", "edit_eqx"])
def test_on_aligner_output(ctx, kind, w):
    import bsalign_amd as B
    drafts, pairs, strands, fwd, tid, start = _real()
    eqx, stranded, packed = "eqx" in kind, "strands" in kind, "seq2bit" in kind
    kw = dict(eqx=eqx, seq2bit=packed, strands=strands if stranded else None)
    use = pairs if stranded else fwd
    mode = B.MODE_OVERLAP if "overlap" in kind else B.MODE_GLOBAL
    if kind.startswith("edit"):
        out, cigs, st = ctx.edit_batch(use, mode, 128, **kw)
    else:
        out, cigs, st = ctx.align_batch(use, B.make_params(mode, 64, 2, -6, -3, -2, 0, 0), **kw)
    tlens = [len(d) for d in drafts]
    gbase, nwin = B.window_gbase(tid, tlens, w)
    gbase = gbase + (start // w).astype(np.uint64)
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(use, wins, w, gbase, nwin, seq2bit=packed, strands=strands if stranded else None)
    guides = ctx.piece_cigars(out, cigs, wp)
    toff = np.concatenate([[0], np.cumsum(tlens)])[:-1]
    doff, dlen = B.window_drafts(toff, tlens, w)
    blob = np.concatenate(drafts)
    slices = [blob[int(o):int(o) + min(int(n), w)] for o, n in zip(doff, dlen)]
    assert len(slices) == nwin and sum(len(ps) for ps, _ in wp) >= 15
    b = W.from_python_calls(wp, guides, slices, w)
    for vote in (False, True):
        got = ctx.window_msa(wp, guides, slices, w, vote=vote, seq2bit=packed)
        roff, rcwin, rcols = W.window_msa_ref(b, int(vote))
        for g, (cols, rec) in enumerate(got):
            assert rec.tolist() == rcwin[g].tolist(), (kind, w, g)
            assert np.array_equal(cols.reshape(-1), rcols[int(roff[g]):int(roff[g + 1])]), (kind, w, g)
    nins = 0
    for g in range(nwin):
        depth, mlen, ins, cols, live = W.window_ref(b, g)
        assert all(live) and depth == len(wp[g][0]), (kind, w, g)          # on this, every piece is live
        assert all(s == 0 for _, s in guides[g])
        nins += sum(ins)
    assert nins > 20, (kind, w)


def test_consensus_of_error_free_reads_is_the_truth(ctx):
    """the CPU loop test's construction through the real aligner, all four passes and the device consensus caller: consensus = truth"""
    import bsalign_amd as B
    from bsalign_amd import msa as MSA
    truth, draft, ws, _ = W.closed_loop()
    w = 100
    pairs = [(truth, draft)] * 4
    out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, 64, 2, -6, -3, -2, 0, 0))
    assert all(int(o["tb"]) == 0 and int(o["te"]) == len(draft) for o in out)
    gbase, nwin = B.window_gbase([0] * 4, [len(draft)], w)
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(pairs, wins, w, gbase, nwin)
    guides = ctx.piece_cigars(out, cigs, wp)
    doff, dlen = B.window_drafts([0], [len(draft)], w)
    slices = [draft[int(o):int(o) + min(int(n), w)] for o, n in zip(doff, dlen)]
    msa = ctx.window_msa(wp, guides, slices, w, vote=False)
    assert all(int(rec["nall"]) == 5 and int(rec["nseq"]) == 4 for _, rec in msa)
    res = MSA.call_consensus_batch(ctx, [(cols, None, int(r["nall"]), int(r["nseq"]), int(r["nmax"]), int(r["mlen"])) for cols, r in msa], W.PAR7)
    assert np.array_equal(np.concatenate([x[0] for x in res]), truth)


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    b, ref = _named("arena", 0)
    total = int(ref[0][-1])
    dev = _Dev(b, total)
    run, batch, err = B.lib().bsa_window_msa_run, B.lib().bsa_window_msa_batch, B.lib().bsa_last_error
    rargs = [ctx.h] + dev.pointers(total)
    hcols, hoff, hcwin = np.full(total, FILL, np.uint8), np.zeros(b.nwin + 1, np.uint64), np.zeros(b.nwin, W.CNS_WINDOW_DTYPE)
    bargs = [ctx.h, B._p(b.piece), B._p(b.piece_off), b.nwin, b.piece_cap, B._p(b.bases), b.bases_cap, B._p(b.pcig), b.pcig_cap, B._p(b.pcig_off), B._p(b.draft), B._p(b.doff),
             B._p(b.dlen), b.window, 0, 0, B._p(hcols), total, B._p(hoff), B._p(hcwin)]

    def refused(fn, base, i, v, code=E_ARG):
        a = list(base)
        a[i] = v
        assert fn(*a) == code, (fn.__name__, i, v)
        if i:
            assert err(ctx.h), (fn.__name__, i, v)
    for fn, base in ((run, rargs), (batch, bargs)):
        # no context, pieces, piece_off, codes, words, pcig_off, draft, doff, dlen, arena (with a cap), cols_off, cwin
        for i in (0, 1, 2, 5, 7, 9, 10, 11, 12, 16, 18, 19):
            refused(fn, base, i, None)
        refused(fn, base, 3, 0xFFFFFFF1)                       # nwin
        refused(fn, base, 4, 0xFFFFFFF1)                       # piece_cap
        refused(fn, base, 13, 0)                               # window
        refused(fn, base, 13, 4097, E_UNSUPPORTED)
        refused(fn, base, 14, 0x2000)                          # a flag that is not the draft's
        refused(fn, base, 14, SEQ2BIT | 1)
        refused(fn, base, 15, 2)                               # vote
    a = list(rargs)
    a[10] = C.c_void_p(dev.d_draft.data_ptr() + 1)             # a packed draft that is not 8-byte aligned
    a[14] = SEQ2BIT
    assert run(*a) == E_ARG and err(ctx.h)
    # nothing was launched by the refused calls; the good calls still run
    assert np.all(hcols == FILL)
    assert run(*rargs) == 0
    ctx.sync()
    assert _check(dev.read(), ref, total, "after the refused calls") == b.nwin
    assert batch(*bargs) == 0 and np.array_equal(hcols, ref[2]) and np.array_equal(hoff, ref[0]) and hcwin.tolist() == ref[1].tolist()
    # NULL is fine where there is no work: no windows, a count-only call
    off1 = np.full(1, FILL64, np.uint64)
    assert batch(ctx.h, None, B._p(b.piece_off), 0, 0, None, 0, None, 0, B._p(b.pcig_off), None, None, None, 16, 0, 0, None, 0, B._p(off1), None) == 0 and off1.tolist() == [0]
    a = list(bargs)
    a[16], a[17] = None, 0
    assert batch(*a) == E_CIGAR_CAP and int(hoff[-1]) == total
