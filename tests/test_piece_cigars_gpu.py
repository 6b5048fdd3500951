"""GPU: bsa_piece_cigars_batch and bsa_piece_cigars_run (include/bsalign_hip.h) bit for bit against the Python statement of the definition
(piece_cigars_cases.piece_cigars_ref): on hand-made alignments and pieces uploaded directly, on pieces that lie on no path, for any arena
capacity, and on what the aligners, bsa_cigar_windows and bsa_window_pieces return.  Every buffer a run writes is prefilled with 0xA5 bytes and the
word arena has 64 guard words on either side, so that a word a run leaves unwritten, or one it writes where it must not, shows.  Every test runs
under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import cigar_windows_cases as CW
import piece_cigars_cases as P
import support as S

pytestmark = pytest.mark.gpu

GUARD = 64                         # guard words around the word arena
FILL = 0xA5
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
E_ARG, E_CIGAR_CAP = -2, -5
_BATCHES, _REFS = {}, {}
BATCH_NAMES = ["header_example", "tile_sizes", "gaps_inside_the_borders", "deletion_over_a_window", "eqx_words", "no_step_and_empty_words", "words_behind_te",
               "pairs_without_an_alignment", "no_pairs", "no_pieces", "long_words"]


def _need():
    """every test here is about bsa_piece_cigars_*: without its symbols in the library none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in ("bsa_piece_cigars_run", "bsa_piece_cigars_batch", "bsa_piece_cigars_bound"):
        assert hasattr(B.lib(), name), "the library does not export " + name


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


def _named(name):
    """(arguments, (pcig_off, words, status)): the reference computed once"""
    _need()
    if not _BATCHES:
        _BATCHES.update(P.hand_batches())
        _BATCHES["not_on_path"] = P.not_on_path_batch()[0]
        _BATCHES["arena"] = P.arena_batch()
    if name not in _REFS:
        args = P.build(_BATCHES[name])
        _REFS[name] = (args, P.piece_cigars_ref(*args))
    return _REFS[name]


def _ptr(a):
    import bsalign_amd as B
    return B._p(a) if a is not None and a.size else None


def _batch(ctx, args, cap, alloc=None):
    """bsa_piece_cigars_batch -> (rc, pcig_off, the whole host arena, status), all prefilled with 0xA5"""
    import bsalign_amd as B
    out, arena, coff, pieces = args
    pcig = np.full(max(alloc if alloc is not None else cap, 1), FILL32, dtype=np.uint32)
    off = np.full(len(pieces) + 1, FILL64, dtype=np.uint64)
    status = np.full(max(len(pieces), 1), FILL32, dtype=np.uint32)
    rc = B.lib().bsa_piece_cigars_batch(ctx.h, _ptr(out), _ptr(arena), B._p(coff), len(out), _ptr(pieces), len(pieces), B._p(pcig), cap, B._p(off), B._p(status))
    return rc, off, pcig, status[:len(pieces)]


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
    """one batch on the device: the piece array has room for piece_cap records (those behind the batch's own hold 0xA5 bytes), *d_npiece is
    `npiece`, the word arena of `alloc` words lies between two guards"""

    def __init__(self, args, piece_cap, alloc, npiece=None):
        import torch
        out, arena, coff, pieces = args
        self.n, self.piece_cap, self.alloc = len(out), piece_cap, alloc
        self.npiece = len(pieces) if npiece is None else npiece
        room = np.full(max(piece_cap, len(pieces), 1) * 32, FILL, dtype=np.uint8)
        room[:len(pieces) * 32] = pieces.view(np.uint8).reshape(-1)
        self.d_out, self.d_cig, self.d_coff, self.d_piece = _upload(out), _upload(arena), _upload(coff), _upload(room)
        self.d_np = _upload(np.array([self.npiece], dtype=np.uint64))
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        self.d_pcig = _filled((self.alloc + 2 * GUARD) * 4)
        self.d_poff = _filled((self.piece_cap + 1) * 8)
        self.d_st = _filled(max(self.piece_cap, 1) * 4)

    def pointers(self, cap, null=False, status=True):
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        return [p(self.d_out), p(self.d_cig), p(self.d_coff), self.n, p(self.d_piece), p(self.d_np), self.piece_cap, None if null else p(self.d_pcig, GUARD * 4), cap,
                p(self.d_poff), p(self.d_st) if status else None]

    def run(self, ctx, cap, null=False, status=True):
        """-> (all piece_cap + 1 offsets, the words of the arena proper, all piece_cap status words); the guards are checked here"""
        import torch
        import bsalign_amd as B
        assert cap <= self.alloc and not (null and cap)
        rc = B.lib().bsa_piece_cigars_run(ctx.h, *self.pointers(cap, null, status))
        assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        w = self.d_pcig.cpu().numpy()[:(self.alloc + 2 * GUARD) * 4].view(np.uint32)
        assert np.all(w[:GUARD] == FILL32) and np.all(w[GUARD + self.alloc:] == FILL32), "a guard word was written"
        return (self.d_poff.cpu().numpy()[:(self.piece_cap + 1) * 8].view(np.uint64).copy(), w[GUARD:GUARD + self.alloc].copy(),
                self.d_st.cpu().numpy()[:self.piece_cap * 4].view(np.uint32).copy())


def _check(got, ref, cap, what="", status=True):
    """the arena contract: every offset exact, those above P equal to the total; piece j's words there iff its range ends inside the cap; every
    other word of the allocation untouched; the status of every piece below P exact, nothing written above.  got may speak of more places than
    the reference has pieces (a run with a piece_cap above P).  -> the pieces present"""
    off, words, st = got
    roff, rwords, rst = ref
    np_ = len(rst)
    assert np.array_equal(off[:np_ + 1], roff), (what, "pcig_off", off[:8], roff[:8])
    assert np.all(off[np_:] == roff[-1]), (what, "the offsets above P are the total", off[np_:][:8], int(roff[-1]))
    if status:
        assert np.array_equal(st[:np_], rst), (what, "status", np.flatnonzero(st[:np_] != rst)[:8])
        assert np.all(st[np_:] == FILL32), (what, "a status above P was written")
    else:
        assert np.all(st == FILL32), (what, "a status was written")
    untouched = np.ones(len(words), dtype=bool)
    present = 0
    for j in range(np_):
        a, b = int(roff[j]), int(roff[j + 1])
        if b <= cap:
            assert np.array_equal(words[a:b], rwords[a:b]), (what, "piece %d" % j, [hex(x) for x in words[a:b][:8]], [hex(x) for x in rwords[a:b][:8]])
            untouched[a:b] = False
            present += 1
    assert np.all(words[untouched] == FILL32), (what, "a word outside the pieces that fit was written", cap, np.flatnonzero(untouched & (words != FILL32))[:8])
    return present


def _both(ctx, args, ref, what, spare=3):
    """_batch with the exact cap and _run with room to spare (in the arena and in the piece array), each against the reference"""
    np_, total = len(ref[2]), int(ref[0][-1])
    rc, off, pcig, st = _batch(ctx, args, total, total + GUARD)
    assert rc == 0, (what, rc)
    assert _check((off, pcig, st), ref, total, what + " (batch)") == np_
    dev = _Dev(args, np_ + spare, total + GUARD)
    assert _check(dev.run(ctx, total + GUARD), ref, total + GUARD, what + " (run)") == np_
    return dev


# ---- 1. hand-made alignments and pieces, uploaded directly ---------------------------------------------------------------------------------
def test_every_hand_made_batch_is_run():
    _named("header_example")
    assert sorted(BATCH_NAMES + ["not_on_path", "arena"]) == sorted(_BATCHES)


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_hand_made_batch(ctx, name):
    args, ref = _named(name)
    dev = _both(ctx, args, ref, name)
    if name == "header_example":
        hdr = P.header_example()
        assert np.array_equal(dev.read()[0][:6], hdr[1]) and np.array_equal(dev.read()[1][:6], hdr[2])
    # a piece array with no room to spare, and no status
    dev = _Dev(args, len(ref[2]), int(ref[0][-1]))
    assert _check(dev.run(ctx, int(ref[0][-1]), status=False), ref, int(ref[0][-1]), name + " (run, exact room, no status)", status=False) == len(ref[2])


def test_more_pieces_announced_than_there_is_room_for(ctx):
    """*d_npiece > piece_cap: P = piece_cap"""
    args, ref = _named("tile_sizes")
    out, arena, coff, pieces = args
    for announced in (len(pieces), 1 << 40):
        cap_p = 50
        want = P.piece_cigars_ref(out, arena, coff, pieces[:cap_p])
        dev = _Dev((out, arena, coff, pieces), cap_p, int(want[0][-1]) + 7, npiece=announced)
        assert _check(dev.run(ctx, int(want[0][-1]) + 7), want, int(want[0][-1]) + 7, "announced %d" % announced) == cap_p


def test_more_room_than_one_scan_block_takes(ctx):
    """piece_cap = 16 400 with the batch's own piece count in *d_npiece: the scan of all piece_cap counts runs in tiles (above 16 384), and every
    offset above P is the total"""
    args, ref = _named("tile_sizes")
    np_, total = len(ref[2]), int(ref[0][-1])
    assert 0 < np_ < 4096 and total > 0
    dev = _Dev(args, 16400, total + GUARD)
    assert dev.npiece == np_
    assert _check(dev.run(ctx, total + GUARD), ref, total + GUARD, "piece_cap 16 400") == np_


def test_through_the_python_calls(ctx):
    """Context.piece_cigars on host arrays, Context.piece_cigars_run on torch tensors"""
    import torch
    import bsalign_amd as B
    args, ref = _named("tile_sizes")
    out, arena, coff, pieces = args
    recs, cigs, _ = _BATCHES["tile_sizes"]
    groups = [(pieces[:40], None), (pieces[40:40], None), (pieces[40:], None)]          # three "windows", the middle one empty
    got = ctx.piece_cigars(out, cigs, groups)
    assert [len(g) for g in got] == [40, 0, len(pieces) - 40]
    flat = [x for g in got for x in g]
    for j, (ws, st) in enumerate(flat):
        assert ws.dtype == np.uint32 and st == int(ref[2][j]) and np.array_equal(ws, ref[1][int(ref[0][j]):int(ref[0][j + 1])]), j
    # pieces that overlap need more than the bound: the call asks again with what the first answer said
    p10 = pieces[pieces["pair"] == 10]
    whole = np.repeat(p10[np.argmax(p10["t_last"].astype(np.int64) - p10["t_first"])].reshape(1), 3)          # the 5000-word pair, end to end, three times
    got = ctx.piece_cigars(out, cigs, [(whole, None)])
    want = P.piece_cigars_ref(out, arena, coff, whole)
    assert int(want[0][-1]) > B.piece_cigars_bound(coff, 3) and np.array_equal(np.concatenate([ws for ws, _ in got[0]]), want[1])
    total, np_ = int(ref[0][-1]), len(pieces)
    dev = _Dev(args, np_, total)
    d_pcig = dev.d_pcig[GUARD * 4:(GUARD + total) * 4]
    ctx.piece_cigars_run(dev.d_out, dev.d_cig, dev.d_coff, dev.n, dev.d_piece, dev.d_np, np_, d_pcig, total, dev.d_poff, dev.d_st)
    ctx.sync()
    torch.cuda.synchronize()
    assert _check(dev.read(), ref, total, "resident") == np_
    with pytest.raises(ValueError):
        ctx.piece_cigars_run(dev.d_out, dev.d_cig, dev.d_coff, dev.n, dev.d_piece, dev.d_np, np_, d_pcig, total + 1, dev.d_poff, dev.d_st)


# ---- 2. pieces that lie on no path -----------------------------------------------------------------------------------------------------------
def test_not_on_a_path(ctx):
    args, ref = _named("not_on_path")
    names = P.not_on_path_batch()[1]
    assert ref[2].tolist() == [1, 0] * len(names)
    dev = _both(ctx, args, ref, "not on a path")
    off, words, st = dev.read()
    for i, name in enumerate(names):
        assert off[2 * i] == off[2 * i + 1] and st[2 * i] == P.NOT_ON_PATH, name          # no words, status 1
        assert off[2 * i + 2] - off[2 * i + 1] == 1 and st[2 * i + 1] == 0, name          # the good piece next to it: 6 M
    assert np.all(words[:len(names)] == (6 << 4 | CW.M))


# ---- 3. the arena contract -------------------------------------------------------------------------------------------------------------------
def test_arena_contract_for_any_capacity(ctx):
    args, ref = _named("arena")
    roff = ref[0]
    np_, total = len(ref[2]), int(roff[-1])
    assert np_ == 40
    inside = [int(roff[j]) + (int(roff[j + 1]) - int(roff[j])) // 2 for j in (7, 30)]          # two caps that end inside a piece
    assert all(int(roff[j]) < c < int(roff[j + 1]) for j, c in zip((7, 30), inside))
    fits = lambda cap: sum(1 for j in range(np_) if int(roff[j + 1]) <= cap)
    dev = _Dev(args, np_ + 5, total + 7)
    for cap, null in ((0, False), (0, True), (total - 1, False), (total, False), (total + 7, False), (inside[0], False), (inside[1], False)):
        dev.fresh()
        what = "cap %d%s" % (cap, " (NULL arena)" if null else "")
        got = dev.run(ctx, cap, null=null)
        present = _check(got, ref, cap, what)
        assert present == fits(cap), what
        if cap >= total:
            assert present == np_
        elif cap == 0:
            assert present == 0 and np.all(got[1] == FILL32), what
        else:
            assert 0 < present < np_, what
    # twice into fresh buffers: the same bytes; a run after a short run on the same context is complete
    dev.fresh()
    one = dev.run(ctx, total)
    dev.fresh()
    _check(dev.run(ctx, inside[0]), ref, inside[0], "short run")
    dev.fresh()
    two = dev.run(ctx, total)
    assert all(np.array_equal(a, b) for a, b in zip(one, two)) and _check(two, ref, total, "second run") == np_


def test_batch_with_a_short_arena(ctx):
    args, ref = _named("arena")
    total = int(ref[0][-1])
    import bsalign_amd as B
    for cap in (0, 1, total - 1):
        rc, off, pcig, st = _batch(ctx, args, cap, total)
        assert rc == E_CIGAR_CAP and int(off[-1]) == total and np.array_equal(off, ref[0]), cap
        assert np.all(pcig == FILL32), cap
        assert B.lib().bsa_last_error(ctx.h), cap
    rc, off, pcig, st = _batch(ctx, args, total)
    assert rc == 0 and np.array_equal(pcig, ref[1]) and np.array_equal(st, ref[2])


# ---- 4. what the aligners return, through all three passes -----------------------------------------------------------------------------------
W_REAL = 100
_PAIRS = {}


def _real_pairs():
    """8 reads of about 600 bases on one draft of 600, about 10 % errors with indels; every second read is stored reverse-complemented and marked.
    -> (pairs as stored, strands, the same pairs stored as they are aligned)"""
    import bsalign_amd as B
    if not _PAIRS:
        rng = np.random.default_rng(606)
        T = rng.integers(0, 4, 600).astype(np.uint8)
        pairs, strands, fwd = [], [], []
        for j in range(8):
            a = (j % 3) * W_REAL
            Q = S.mutate(rng, T[a:], 0.10)
            rev = j % 2 == 1
            pairs.append((B.revcomp(Q) if rev else Q, T[a:]))
            fwd.append((Q, T[a:]))
            strands.append(rev)
        _PAIRS["x"] = (pairs, strands, fwd, np.array([(j % 3) for j in range(8)], dtype=np.uint64))
    return _PAIRS["x"]


@pytest.mark.parametrize("kind", ["align", "align_eqx", "edit", "edit_eqx", "align_eqx_stranded_seq2bit"])
def test_on_aligner_output(ctx, kind):
    import bsalign_amd as B
    pairs, strands, fwd, gbase = _real_pairs()
    eqx = "eqx" in kind
    stranded = "stranded" in kind
    kw = dict(eqx=eqx, seq2bit=stranded, strands=strands if stranded else None)
    use = pairs if stranded else fwd
    if kind.startswith("edit"):
        out, cigs, st = ctx.edit_batch(use, B.MODE_GLOBAL, 128, **kw)
    else:
        out, cigs, st = ctx.align_batch(use, B.make_params(B.MODE_GLOBAL, 64, 2, -6, -3, -2, 0, 0), **kw)
    assert all(len(c) > 20 for c in cigs) and sum(int(((c & 15) == CW.I).sum() + ((c & 15) == CW.D).sum()) for c in cigs) > 50, kind
    nwin = 6
    wins = ctx.cigar_windows(out, cigs, W_REAL)
    wp = ctx.window_pieces(use, wins, W_REAL, gbase, nwin, seq2bit=stranded, strands=strands if stranded else None)
    got = ctx.piece_cigars(out, cigs, wp)
    pieces = np.concatenate([ps for ps, _ in wp])
    arena, coff = CW.flatten(cigs)
    roff, rwords, rst = P.piece_cigars_ref(out, arena, coff, pieces)
    assert len(pieces) >= 36 and len(got) == nwin
    assert np.all(rst == 0)
    j = 0
    for g in range(nwin):
        ps, codes = wp[g]
        assert len(got[g]) == len(ps)
        for pc, code, (ws, status) in zip(ps, codes, got[g]):
            assert status == 0, (kind, g, pc)                  # every piece is cut: no exception
            assert np.array_equal(ws, rwords[int(roff[j]):int(roff[j + 1])]), (kind, g, j)
            j += 1
            ops = ws & np.uint32(15)
            assert int(ops[0]) in P.DIAG and int(ops[-1]) in P.DIAG
            qn, tn = P.sums(ws)
            assert qn == int(pc["len"]) and tn == int(pc["t_last"]) - int(pc["t_first"]) + 1
            assert np.all(np.isin(ops, (CW.EQ, CW.X, CW.I, CW.D) if eqx else (CW.M, CW.I, CW.D)))
            # the guide a refmode caller makes covers the window's slice of the target
            k = int(pc["pair"])
            t = fwd[k][1]
            m = int(pc["t_first"]) // W_REAL
            wend = min((m + 1) * W_REAL, len(t))
            assert P.sums(P.refmode_guide(ws, int(pc["t_first"]), int(pc["t_last"]), W_REAL, wend))[1] == wend - m * W_REAL
            if eqx:
                # replay: every = unit is an equal base, every X unit a different one -- the codes are window_pieces', the target the pair's own
                ti, qi = int(pc["t_first"]), 0
                for w_ in ws:
                    op, ln = int(w_) & 15, int(w_) >> 4
                    if op in (CW.EQ, CW.X):
                        same = code[qi:qi + ln] == t[ti:ti + ln]
                        assert np.all(same) if op == CW.EQ else not np.any(same), (kind, g, pc, op, ln)
                    ti += ln if op != CW.I else 0
                    qi += ln if op != CW.D else 0
                assert qi == len(code) and ti == int(pc["t_last"]) + 1
    assert j == len(pieces)


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    args, ref = _named("arena")
    out, arena, coff, pieces = args
    np_, total, n = len(pieces), int(ref[0][-1]), len(out)
    dev = _Dev(args, np_, total)
    run, batch, err = B.lib().bsa_piece_cigars_run, B.lib().bsa_piece_cigars_batch, B.lib().bsa_last_error
    rargs = [ctx.h] + dev.pointers(total)
    hw, hoff, hst = np.full(total, FILL32, np.uint32), np.zeros(np_ + 1, np.uint64), np.zeros(np_, np.uint32)
    bargs = [ctx.h, B._p(out), B._p(arena), B._p(coff), n, B._p(pieces), np_, B._p(hw), total, B._p(hoff), B._p(hst)]

    def refused(fn, base, i, v):
        a = list(base)
        a[i] = v
        assert fn(*a) == E_ARG, (fn.__name__, i, v)
        if i:
            assert err(ctx.h), (fn.__name__, i, v)
    # run: no context, records, words, offsets, pieces, piece count, arena (with a cap), offsets out; n 4, piece_cap 7
    for i in (0, 1, 2, 3, 5, 6, 8, 10):
        refused(run, rargs, i, None)
    refused(run, rargs, 4, 0xFFFFFFF1)
    refused(run, rargs, 7, 0xFFFFFFF1)
    # nothing was launched by the refused calls; the good call still runs
    assert run(*rargs) == 0
    ctx.sync()
    assert _check(dev.read(), ref, total, "after the refused calls") == np_
    # batch: no context, records, words, offsets, pieces, arena (with a cap), offsets out; n 4, npiece 6
    for i in (0, 1, 2, 3, 5, 7, 9):
        refused(batch, bargs, i, None)
    refused(batch, bargs, 4, 0xFFFFFFF1)
    refused(batch, bargs, 6, 0xFFFFFFF1)
    down = coff.copy()
    down[1] = down[2] + np.uint64(1)                           # offsets that decrease
    refused(batch, bargs, 3, B._p(down))
    assert np.all(hw == FILL32)
    a = list(bargs)
    a[8] = total - 1
    assert batch(*a) == E_CIGAR_CAP and err(ctx.h) and int(hoff[-1]) == total and np.all(hw == FILL32)
    a = list(bargs)
    a[10] = None                                               # no status array
    assert batch(*a) == 0 and np.array_equal(hoff, ref[0]) and np.array_equal(hw, ref[1])
    # NULL is fine where there is no work: no pairs, no pieces, a count-only call
    off2 = np.full(3, FILL64, np.uint64)
    st2 = np.full(2, FILL32, np.uint32)
    assert batch(ctx.h, None, None, None, 0, B._p(pieces), 2, None, 0, B._p(off2), B._p(st2)) == 0 and off2.tolist() == [0, 0, 0] and st2.tolist() == [1, 1]
    off1 = np.full(1, FILL64, np.uint64)
    assert batch(ctx.h, B._p(out), B._p(arena), B._p(coff), n, None, 0, None, 0, B._p(off1), None) == 0 and off1.tolist() == [0]
    with pytest.raises(B.BsaError) as e:
        ctx._chk(batch(ctx.h, None, B._p(arena), B._p(coff), n, B._p(pieces), np_, B._p(hw), total, B._p(hoff), None))
    assert e.value.code == E_ARG
