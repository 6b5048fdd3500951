"""GPU: bsa_window_pieces_batch and bsa_window_pieces_run (include/bsalign_hip.h) bit for bit against the Python statement of the definition
(window_pieces_cases.pieces_ref): on hand-made reads and records uploaded directly, on what the aligners and bsa_cigar_windows return, and for any
pair of arena capacities.  Every buffer a run writes is prefilled with 0xA5 bytes; the piece arena has 64 guard records on either side and the
base arena 256 guard bytes, so that a record or a byte a run leaves unwritten, or one it writes where it must not, shows.  Every test runs under
a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import support as S
import window_pieces_cases as P

pytestmark = pytest.mark.gpu

GUARD, BGUARD = 64, 256            # guard records around the piece arena, guard bytes around the base arena
FILL = 0xA5
FILL64 = 0xA5A5A5A5A5A5A5A5
E_ARG, E_CIGAR_CAP = -2, -5
_CASES, _REFS = {}, {}
CASE_NAMES = ["depths", "deep_5000", "lengths_at_every_residue", "stored_at_every_offset", "marked_read_of_length_1", "codes_above_3", "none_records",
              "pairs_without_records", "q_last_at_qlen", "q_last_far_above_qlen", "q_first_above_q_last", "t_first_above_t_last", "window_at_nwin",
              "window_far_above_nwin", "gbase_pushes_a_pair_out", "gbase_2_pow_40", "gbase_near_2_pow_64", "two_records_in_one_window", "no_pairs", "no_windows",
              "one_window", "window_1", "window_max", "thousand_pairs", "arena_batch", "many_windows"]
RAW_CASES = ("codes_above_3",)     # codes above 3 have no packed form: built for 1 B/base only


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


def _case(name, flags):
    """(arguments, (piece_off, base_off, records, bytes)): the reference computed once"""
    if not _CASES:
        _CASES.update(P.hand_cases())
    if (name, flags) not in _REFS:
        args = P.build(_CASES[name], flags)
        _REFS[name, flags] = (args, P.pieces_ref(*args))
    return _REFS[name, flags]


def _ptr(a):
    import bsalign_amd as B
    return B._p(a) if a is not None and a.size else None


def _batch(ctx, args, pcap, bcap, palloc=None, balloc=None):
    """bsa_window_pieces_batch -> (rc, piece_off, base_off, the whole host piece arena, the whole host base arena), all prefilled with 0xA5"""
    import bsalign_amd as B
    seqs, qoff, qlen, win, win_off, w, gbase, nwin, flags = args
    piece = np.full(max(palloc if palloc is not None else pcap, 1) * 32, FILL, dtype=np.uint8).view(P.PIECE_DTYPE)
    bases = np.full(max(balloc if balloc is not None else bcap, 1), FILL, dtype=np.uint8)
    poff, boff = np.full(nwin + 1, FILL64, dtype=np.uint64), np.full(nwin + 1, FILL64, dtype=np.uint64)
    rc = B.lib().bsa_window_pieces_batch(ctx.h, _ptr(seqs), seqs.nbytes, _ptr(qoff), _ptr(qlen), _ptr(win), B._p(win_off), len(qlen), w, _ptr(gbase), nwin, flags,
                                         B._p(piece), pcap, B._p(poff), B._p(bases), bcap, B._p(boff))
    return rc, poff, boff, piece, bases


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
    """one batch on the device; a piece arena of `palloc` records and a base arena of `balloc` bytes, each between two guards, and the offsets"""

    def __init__(self, args, palloc, balloc):
        import torch
        seqs, qoff, qlen, win, win_off, self.w, gbase, self.nwin, self.flags = args
        self.n, self.palloc, self.balloc = len(qlen), palloc, balloc
        self.d_seqs, self.d_qoff, self.d_qlen, self.d_win, self.d_woff, self.d_gbase = (_upload(x) for x in (seqs, qoff, qlen, win, win_off, gbase))
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        self.d_piece = _filled((self.palloc + 2 * GUARD) * 32)
        self.d_bases = _filled(self.balloc + 2 * BGUARD)
        self.d_poff, self.d_boff = _filled((self.nwin + 1) * 8), _filled((self.nwin + 1) * 8)

    def run(self, ctx, pcap, bcap, null=False, want_rc=0):
        """-> (piece_off, base_off, the records of the arena proper, its bytes); the guards are checked here"""
        import torch
        import bsalign_amd as B
        assert pcap <= self.palloc and bcap <= self.balloc and not (null and (pcap or bcap))
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        rc = B.lib().bsa_window_pieces_run(ctx.h, p(self.d_seqs), p(self.d_qoff), p(self.d_qlen), p(self.d_win), p(self.d_woff), self.n, self.w, p(self.d_gbase),
                                           self.nwin, self.flags, None if null else p(self.d_piece, GUARD * 32), pcap, p(self.d_poff),
                                           None if null else p(self.d_bases, BGUARD), bcap, p(self.d_boff))
        assert rc == want_rc, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        pw = self.d_piece.cpu().numpy()[:(self.palloc + 2 * GUARD) * 32]
        bw = self.d_bases.cpu().numpy()[:self.balloc + 2 * BGUARD]
        assert np.all(pw[:GUARD * 32] == FILL) and np.all(pw[(GUARD + self.palloc) * 32:] == FILL), "a guard record was written"
        assert np.all(bw[:BGUARD] == FILL) and np.all(bw[BGUARD + self.balloc:] == FILL), "a guard byte was written"
        off = lambda t: t.cpu().numpy()[:(self.nwin + 1) * 8].view(np.uint64).copy()
        return off(self.d_poff), off(self.d_boff), pw[GUARD * 32:(GUARD + self.palloc) * 32].copy().view(P.PIECE_DTYPE), bw[BGUARD:BGUARD + self.balloc].copy()


def _check(got, ref, pcap, bcap, what=""):
    """the arena contract: both offset arrays exact; window g's records and bytes there iff both of its ranges end inside the caps; every other
    record and byte of both allocations untouched.  -> the windows present"""
    poff, boff, piece, bases = got
    rpoff, rboff, recs, codes = ref
    assert np.array_equal(poff, rpoff), (what, "piece_off", poff[:8], rpoff[:8])
    assert np.array_equal(boff, rboff), (what, "base_off", boff[:8], rboff[:8])
    pu, bu = np.ones(len(piece), dtype=bool), np.ones(len(bases), dtype=bool)
    present = 0
    for g in range(len(rpoff) - 1):
        a, b, x, y = int(rpoff[g]), int(rpoff[g + 1]), int(rboff[g]), int(rboff[g + 1])
        if b <= pcap and y <= bcap:
            if not np.array_equal(piece[a:b], recs[a:b]):
                r = int(np.flatnonzero(piece[a:b] != recs[a:b])[0])
                raise AssertionError((what, "window %d piece %d of %d" % (g, r, b - a), piece[a + r].tolist(), recs[a + r].tolist()))
            if not np.array_equal(bases[x:y], codes[x:y]):
                r = int(np.flatnonzero(bases[x:y] != codes[x:y])[0])
                j = int(np.searchsorted(recs["base_off"][a:b], x + r, side="right")) - 1
                raise AssertionError((what, "window %d byte %d of %d" % (g, r, y - x), int(bases[x + r]), int(codes[x + r]), "piece", recs[a + j].tolist()))
            pu[a:b] = False
            bu[x:y] = False
            present += 1
    assert np.all(piece.view(np.uint8).reshape(-1, 32)[pu] == FILL), (what, "a record outside the windows that fit was written", pcap, bcap)
    assert np.all(bases[bu] == FILL), (what, "a byte outside the windows that fit was written", int(np.flatnonzero(bu & (bases != FILL))[0]), pcap, bcap)
    return present


def _both(ctx, args, ref, what):
    """_batch with exact caps and _run with room to spare, each against the reference"""
    nwin = args[7]
    np_, nb = int(ref[0][-1]), int(ref[1][-1])
    rc, poff, boff, piece, bases = _batch(ctx, args, np_, nb, np_ + GUARD, nb + BGUARD)
    assert rc == 0, (what, rc)
    assert _check((poff, boff, piece, bases), ref, np_, nb, what + " (batch)") == nwin
    dev = _Dev(args, np_ + GUARD, nb + BGUARD)
    assert _check(dev.run(ctx, np_ + GUARD, nb + BGUARD), ref, np_ + GUARD, nb + BGUARD, what + " (run)") == nwin


# ---- 1. hand-made reads and records, uploaded directly -----------------------------------------------------------------------------------
def test_every_hand_made_case_is_run():
    _case("no_pairs", 0)
    assert sorted(CASE_NAMES) == sorted(_CASES)
    assert sorted(n for n in CASE_NAMES if _CASES[n].raw) == sorted(RAW_CASES)


@pytest.mark.parametrize("name,flags", [(n, f) for n in CASE_NAMES for f in P.ALL_FLAGS if not (n in RAW_CASES and f & P.SEQ2BIT)])
def test_hand_made_case(ctx, name, flags):
    args, ref = _case(name, flags)
    _both(ctx, args, ref, "%s flags %#x" % (name, flags))


def test_hand_made_cases_hold_what_they_are_for():
    """the depths, lengths, residues and offsets the cases are there for are in the reference's output"""
    args, (poff, boff, recs, codes) = _case("depths", P.QSTRAND)
    assert np.diff(poff.astype(np.int64)).tolist() == list(P.DEPTHS)
    args, (poff, boff, recs, codes) = _case("deep_5000", 0)
    assert np.diff(poff.astype(np.int64)).tolist() == [0, 5000, 0] and set(recs["len"].tolist()) == {1, 2, 3}
    args, (poff, boff, recs, codes) = _case("lengths_at_every_residue", P.QSTRAND)
    for L in P.LENGTHS:
        assert sorted(set((recs["base_off"][recs["len"] == L] % 16).tolist())) == list(range(16)), L
    for flags in (0, P.SEQ2BIT):
        args, (poff, boff, recs, codes) = _case("stored_at_every_offset", flags)
        assert sorted(set((args[1] % np.uint64(32)).tolist())) == list(range(32))
        assert (recs["len"] == 70).sum() == 32 and len(recs) >= 32 * 10
    args, (poff, boff, recs, codes) = _case("thousand_pairs", 0)
    assert len(recs) > 1500 and (np.diff(poff.astype(np.int64)) > 0).sum() >= 45 and len(recs) < len(args[3]) * 0.85
    args, ref = _case("codes_above_3", P.QSTRAND)
    assert (args[0] > 3).sum() > 50 and ref[3].max() <= 3
    for name in ("q_last_at_qlen", "q_last_far_above_qlen", "q_first_above_q_last", "t_first_above_t_last", "window_at_nwin", "window_far_above_nwin", "gbase_2_pow_40",
                 "gbase_near_2_pow_64"):
        args, ref = _case(name, 0)
        assert len(args[3]) == 7 and len(ref[2]) in (4, 5), name          # the two broken records, or a whole pair of two, are ignored
    args, (poff, boff, recs, codes) = _case("many_windows", P.QSTRAND)
    d = np.diff(poff.astype(np.int64))
    assert args[7] == 16400 and len(args[2]) == 40 and int(poff[-1]) == 40 and all(1 <= d[g] <= 4 for g in P.MANY_WINDOWS) and max(d[g] for g in P.MANY_WINDOWS) >= 3


# ---- 2. what the aligners return -------------------------------------------------------------------------------------------------------
W_REAL = 100


def _real_pairs():
    """three targets of 600 bases; 40 reads a target, each cut from a slice that starts on a window border, about 10 % errors; every second read
    is stored reverse-complemented and marked.  -> (pairs as stored, strands, q' per pair, gbase, nwin)"""
    import bsalign_amd as B
    rng = np.random.default_rng(2025)
    pairs, strands, qs, tid, first = [], [], [], [], []
    for t in range(3):
        T = rng.integers(0, 4, 600).astype(np.uint8)
        for j in range(40):
            a = (j % 5) * W_REAL
            b = int(rng.integers(a + 80, 601))
            Q = S.mutate(rng, T[a:b], 0.10)
            rev = j % 2 == 1
            pairs.append((B.revcomp(Q) if rev else Q, T[a:b]))
            strands.append(rev); qs.append(Q); tid.append(t); first.append(a // W_REAL)
    gbase, nwin = B.window_gbase(tid, [600] * 3, W_REAL)
    return pairs, strands, qs, gbase + np.array(first, dtype=np.uint64), nwin


_REAL = {}


def _real(ctx, kind):
    """(pairs, strands, q', gbase, nwin, window records per pair) of one aligner call, made once"""
    import bsalign_amd as B
    if "pairs" not in _REAL:
        _REAL["pairs"] = _real_pairs()
    pairs, strands, qs, gbase, nwin = _REAL["pairs"]
    if kind not in _REAL:
        sc = (2, -6, -3, -2, 0, 0)
        if kind == "edit":
            out, cigs, st = ctx.edit_batch(pairs, B.MODE_GLOBAL, 128, strands=strands)
        else:
            out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL if kind == "global" else B.MODE_OVERLAP, 64, *sc), strands=strands)
        assert sum(1 for c in cigs if len(c)) >= 100, kind
        _REAL[kind] = ctx.cigar_windows(out, cigs, W_REAL)
    return pairs, strands, qs, gbase, nwin, _REAL[kind]


@pytest.mark.parametrize("kind", ["global", "overlap", "edit"])
def test_real_outputs(ctx, kind):
    import bsalign_amd as B
    pairs, strands, qs, gbase, nwin, wins = _real(ctx, kind)
    assert nwin == 18
    fwd = [(q, t) for q, (_, t) in zip(qs, pairs)]            # the same reads stored as they were aligned: no strand needed
    first = None
    for seq2bit in (False, True):
        for stranded in (False, True):
            got = ctx.window_pieces(pairs if stranded else fwd, wins, W_REAL, gbase, nwin, seq2bit=seq2bit, strands=strands if stranded else None)
            seqs, qoff, qlen, _, _ = B.pack_pairs(pairs if stranded else fwd, seq2bit, strands if stranded else None)
            woff = np.zeros(len(pairs) + 1, dtype=np.uint64)
            woff[1:] = np.cumsum([len(x) for x in wins], dtype=np.uint64)
            flags = (P.SEQ2BIT if seq2bit else 0) | (P.QSTRAND if stranded else 0)
            poff, boff, recs, codes = P.pieces_ref(seqs, qoff, qlen, np.concatenate(wins), woff, W_REAL, gbase, nwin, flags)
            assert len(got) == nwin and len(recs) >= 200 and np.all(np.diff(poff.astype(np.int64)) >= 3)
            for g in range(nwin):
                ps, cs = got[g]
                a, b = int(poff[g]), int(poff[g + 1])
                assert ps.dtype == B.PIECE_DTYPE and np.array_equal(ps, recs[a:b]), (kind, seq2bit, stranded, g)
                assert np.all(np.diff(ps["pair"].astype(np.int64)) > 0)          # a record a pair and window: ascending pair index
                for r, c in zip(ps, cs):
                    x, n = int(r["base_off"]), int(r["len"])
                    assert c.dtype == np.uint8 and np.array_equal(c, codes[x:x + n])
                    # directly: the piece is q'[q_first : q_first + len) of the read as it was aligned
                    assert np.array_equal(c, qs[int(r["pair"])][int(r["q_first"]):int(r["q_first"]) + n]), (kind, seq2bit, stranded, g)
            if first is None:
                first = (recs, codes)
            assert np.array_equal(first[0], recs) and np.array_equal(first[1], codes), "the four flag combinations give the same records and bytes"


def test_real_outputs_resident(ctx):
    """the same through Context.window_pieces_run on torch tensors"""
    import torch
    import bsalign_amd as B
    pairs, strands, qs, gbase, nwin, wins = _real(ctx, "global")
    seqs, qoff, qlen, _, _ = B.pack_pairs(pairs, True, strands)
    woff = np.zeros(len(pairs) + 1, dtype=np.uint64)
    woff[1:] = np.cumsum([len(x) for x in wins], dtype=np.uint64)
    args = (seqs, qoff, qlen, np.concatenate(wins), woff, W_REAL, gbase, nwin, P.SEQ2BIT | P.QSTRAND)
    ref = P.pieces_ref(*args)
    pcap, bcap = int(woff[-1]), int(qlen.astype(np.int64).sum())          # the caps the header calls sufficient
    assert pcap >= int(ref[0][-1]) and bcap >= int(ref[1][-1])
    dev = _Dev(args, pcap, bcap)
    d_piece, d_bases = dev.d_piece[GUARD * 32:(GUARD + pcap) * 32], dev.d_bases[BGUARD:BGUARD + bcap]
    ctx.window_pieces_run(dev.d_seqs, dev.d_qoff, dev.d_qlen, dev.d_win, dev.d_woff, dev.n, W_REAL, dev.d_gbase, nwin, args[8], d_piece, pcap, dev.d_poff, d_bases, bcap, dev.d_boff)
    ctx.sync()
    torch.cuda.synchronize()
    off = lambda t: t.cpu().numpy()[:(nwin + 1) * 8].view(np.uint64)
    got = (off(dev.d_poff), off(dev.d_boff), dev.d_piece.cpu().numpy()[GUARD * 32:(GUARD + pcap) * 32].view(P.PIECE_DTYPE), dev.d_bases.cpu().numpy()[BGUARD:BGUARD + bcap])
    assert _check(got, ref, pcap, bcap, "resident") == nwin
    with pytest.raises(ValueError):
        ctx.window_pieces_run(dev.d_seqs, dev.d_qoff, dev.d_qlen, dev.d_win, dev.d_woff, dev.n, W_REAL, dev.d_gbase, nwin, args[8], d_piece, pcap + 1, dev.d_poff, d_bases, bcap,
                              dev.d_boff)


def test_base_sums_above_2_pow_32(ctx):
    """count-only run (no arenas: the blob is never read): three pieces of 2^32 - 1 bases, two in window 0 and one in window 4096, the first window of the
    scan's second tile.  base_off is summed in 64 bits inside a thread, across a tile and across the tiles.  (_batch rightly refuses such reads.)"""
    n, nwin, big = 3, 4100, 0xFFFFFFFF
    args = (np.zeros(16, np.uint8), np.zeros(n, np.uint64), np.full(n, big, np.uint32), np.array([[0, 0, 5, big - 1]] * n, np.uint32),
            np.arange(n + 1, dtype=np.uint64), 10, np.array([0, 0, 4096], np.uint64), nwin, 0)
    cnt = np.zeros(nwin, np.uint64)
    cnt[0], cnt[4096] = 2, 1
    rpoff, rboff = np.zeros(nwin + 1, np.uint64), np.zeros(nwin + 1, np.uint64)
    rpoff[1:], rboff[1:] = np.cumsum(cnt, dtype=np.uint64), np.cumsum(cnt * np.uint64(big), dtype=np.uint64)
    assert int(rboff[1]) == 2 * big > 1 << 32 and int(rboff[-1]) == 3 * big
    poff, boff, piece, bases = _Dev(args, 0, 0).run(ctx, 0, 0, null=True)
    assert np.array_equal(poff, rpoff), ("piece_off", poff[[0, 1, 4096, 4097, nwin]])
    assert np.array_equal(boff, rboff), ("base_off", boff[[0, 1, 4096, 4097, nwin]])


# ---- 3. the arena contract -------------------------------------------------------------------------------------------------------------
def test_arena_contract_for_any_capacities(ctx):
    args, ref = _case("arena_batch", P.QSTRAND)
    rpoff, rboff = ref[0], ref[1]
    nwin, np_, nb = args[7], int(rpoff[-1]), int(rboff[-1])
    assert nwin == 30 and np_ == 300 and nb > 3000
    fits = lambda pcap, bcap: sum(1 for g in range(nwin) if int(rpoff[g + 1]) <= pcap and int(rboff[g + 1]) <= bcap)
    dev = _Dev(args, np_ + GUARD, nb + BGUARD)
    for pcap, bcap, null in ((0, 0, False), (0, 0, True), (np_ - 1, nb, False), (np_, nb - 1, False), (np_ // 2, nb, False), (np_, nb // 2, False), (np_, nb, False)):
        dev.fresh()
        what = "caps %d, %d%s" % (pcap, bcap, " (NULL arenas)" if null else "")
        got = dev.run(ctx, pcap, bcap, null=null)
        present = _check(got, ref, pcap, bcap, what)
        assert present == fits(pcap, bcap), what
        if (pcap, bcap) == (np_, nb):
            assert present == nwin
        elif pcap == 0:
            assert present == 0 and np.all(got[2].view(np.uint8) == FILL) and np.all(got[3] == FILL), what
        else:
            assert 0 < present < nwin, what
    # twice into fresh buffers: the same bytes
    dev.fresh()
    one = dev.run(ctx, np_, nb)
    dev.fresh()
    two = dev.run(ctx, np_, nb)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(one, two)) and _check(two, ref, np_, nb, "second run") == nwin
    # a run after a short run on the same context is complete
    dev.fresh()
    _check(dev.run(ctx, np_ // 2, nb // 2), ref, np_ // 2, nb // 2, "short run")
    dev.fresh()
    three = dev.run(ctx, np_, nb)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(one, three))


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    args, ref = _case("none_records", P.QSTRAND)
    seqs, qoff, qlen, win, win_off, w, gbase, nwin, flags = args
    np_, nb, n = int(ref[0][-1]), int(ref[1][-1]), len(qlen)
    dev = _Dev(args, np_, nb)
    run = B.lib().bsa_window_pieces_run
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    rargs = [ctx.h, p(dev.d_seqs), p(dev.d_qoff), p(dev.d_qlen), p(dev.d_win), p(dev.d_woff), n, w, p(dev.d_gbase), nwin, flags,
             p(dev.d_piece, GUARD * 32), np_, p(dev.d_poff), p(dev.d_bases, BGUARD), nb, p(dev.d_boff)]
    hp, hb = np.full(np_ * 32, FILL, np.uint8), np.full(nb, FILL, np.uint8)
    hpoff, hboff = np.zeros(nwin + 1, np.uint64), np.zeros(nwin + 1, np.uint64)
    bargs = [ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(win), B._p(win_off), n, w, B._p(gbase), nwin, flags, B._p(hp), np_, B._p(hpoff), B._p(hb), nb, B._p(hboff)]

    def refused(fn, base, i, v):
        a = list(base)
        a[i] = v
        assert fn(*a) == E_ARG, (fn.__name__, i, v)
    # run: index of window 7, flags 10, n 6, nwin 9; no context, blob, offsets, lengths, records, record offsets, gbase, arenas (with a cap), offsets
    refused(run, rargs, 7, 0)
    for bad in (1, 0x400, 0x1000, 0x4000, 0x80000000):
        refused(run, rargs, 10, flags | bad)
    for i in (0, 1, 2, 3, 4, 5, 8, 11, 13, 14, 16):
        refused(run, rargs, i, None)
    refused(run, rargs, 6, 0xFFFFFFF1)
    refused(run, rargs, 9, 0xFFFFFFF1)
    a = list(rargs)
    a[1], a[10] = p(dev.d_seqs, 4), P.SEQ2BIT                   # packed words need an 8-byte aligned blob
    assert run(*a) == E_ARG
    # nothing was launched by the refused calls; the good call still runs
    assert _check(dev.run(ctx, np_, nb), ref, np_, nb, "after the refused calls") == nwin
    # batch: the same arguments one place further on behind seqs_bytes
    batch = B.lib().bsa_window_pieces_batch
    refused(batch, bargs, 8, 0)
    for bad in (1, 0x400, 0x1000, 0x4000, 0x80000000):
        refused(batch, bargs, 11, flags | bad)
    for i in (0, 1, 3, 4, 5, 6, 9, 12, 14, 15, 17):
        refused(batch, bargs, i, None)
    refused(batch, bargs, 7, 0xFFFFFFF1)
    refused(batch, bargs, 10, 0xFFFFFFF1)
    down = win_off.copy()
    down[1] = down[2] + np.uint64(1)                           # offsets that decrease
    refused(batch, bargs, 6, B._p(down))
    assert np.all(hp == FILL) and np.all(hb == FILL)
    assert batch(*bargs) == 0 and np.array_equal(hpoff, ref[0]) and np.array_equal(hp.view(P.PIECE_DTYPE), ref[2]) and np.array_equal(hb, ref[3])
    with pytest.raises(B.BsaError) as e:
        ctx.window_pieces([(np.zeros(5, np.uint8), np.zeros(5, np.uint8))], [np.array([[0, 0, 4, 4]], np.uint32)], 0, [0], 1)
    assert e.value.code == E_ARG


def test_batch_with_short_arenas(ctx):
    args, ref = _case("arena_batch", P.SEQ2BIT | P.QSTRAND)
    np_, nb = int(ref[0][-1]), int(ref[1][-1])
    for pcap, bcap in ((0, 0), (np_ - 1, nb), (np_, nb - 1), (1, 1)):
        rc, poff, boff, piece, bases = _batch(ctx, args, pcap, bcap, np_, nb)
        assert rc == E_CIGAR_CAP and int(poff[-1]) == np_ and int(boff[-1]) == nb and np.array_equal(poff, ref[0]) and np.array_equal(boff, ref[1]), (pcap, bcap)
        assert np.all(piece.view(np.uint8) == FILL) and np.all(bases == FILL), (pcap, bcap)
    rc, poff, boff, piece, bases = _batch(ctx, args, np_, nb)
    assert rc == 0 and np.array_equal(piece, ref[2]) and np.array_equal(bases, ref[3])


def test_batch_with_a_read_outside_the_blob(ctx):
    import bsalign_amd as B
    for flags in P.ALL_FLAGS:
        seqs, qoff, qlen, win, win_off, w, gbase, nwin, _ = _case("none_records", flags)[0]
        have = seqs.nbytes * (4 if flags & P.SEQ2BIT else 1)
        np_ = 16

        def call(qo, ql, nbytes=seqs.nbytes):
            piece, bases = np.full(np_ * 32, FILL, np.uint8), np.full(1024, FILL, np.uint8)
            poff, boff = np.zeros(nwin + 1, np.uint64), np.zeros(nwin + 1, np.uint64)
            rc = B.lib().bsa_window_pieces_batch(ctx.h, B._p(seqs), nbytes, B._p(qo), B._p(ql), B._p(win), B._p(win_off), len(ql), w, B._p(gbase), nwin, flags,
                                                 B._p(piece), np_, B._p(poff), B._p(bases), 1024, B._p(boff))
            assert np.all(piece == FILL) or rc == 0
            return rc
        assert call(qoff, qlen) == 0, flags
        ql = qlen.copy()
        ql[-1] = have - int(qoff[-1] & np.uint64(P.REVCOMP - 1)) + 1                      # one base behind the blob
        assert call(qoff, ql) == E_ARG, flags
        qo = qoff.copy()
        qo[2] = np.uint64(have + 1)
        assert call(qo, qlen) == E_ARG, flags
        qo = qoff.copy()
        qo[0] = np.uint64((1 << 64) - 8) & np.uint64(~P.REVCOMP & (2 ** 64 - 1) if flags & P.QSTRAND else 2 ** 64 - 1)      # offset + length wraps
        assert call(qo, qlen) == E_ARG, flags
        if not flags & P.QSTRAND:
            qo = qoff.copy()
            qo[1] |= np.uint64(P.REVCOMP)                      # without BSA_MODE_QSTRAND bit 63 is part of the offset
            assert call(qo, qlen) == E_ARG, flags
        if flags & P.SEQ2BIT and seqs.nbytes > 8:
            assert call(qoff, qlen, seqs.nbytes - 4) == E_ARG  # a packed blob is whole words
