"""GPU: bsa_window_stitch_run and bsa_window_stitch_batch (include/bsalign_hip.h) against the Python statement of the definition
(window_stitch_cases.window_stitch_ref): both header examples, mixed batches at the smallest shapes at which the kernels can go wrong, behind a real
bsa_window_cns_run on the same resident buffers, one window for every way a record fails, any capacity of the two arenas, the closed loop with a
coverage hole and the aligner's output through all resident passes, re-runs, and the argument errors.

Tolerance: none.  Records, both offset arrays, bases, both quality strings and words are compared bit for bit.

Every buffer a run writes is prefilled with 0xA5 bytes and every arena has 256 guard bytes on either side; the columns are uploaded into an
allocation of exactly their size.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import support as S
import window_cns_cases as WC
import window_msa_cases as W
import window_stitch_cases as WS
from window_msa_cases import CNS_WINDOW_DTYPE, PAR7

pytestmark = pytest.mark.gpu

GUARD = 256
FILL, FILL32, FILL64 = WS.FILL, WS.FILL32, 0xA5A5A5A5A5A5A5A5
E_ARG, E_CIGAR_CAP = -2, -5
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


def _arena(nbytes):
    return _filled(nbytes + 2 * GUARD)


def _inside(t, nbytes, what):
    w = t.cpu().numpy()
    assert np.all(w[:GUARD] == FILL) and np.all(w[GUARD + nbytes:] == FILL), "a guard byte of %s was written" % what
    return w[GUARD:GUARD + nbytes].copy()


def _down(t, nbytes, dtype):
    return t.cpu().numpy()[:nbytes].view(dtype).copy()


class Got:
    pass


class _Dev:
    """one batch on the device: the columns in an allocation of exactly their size, the sequence arrays of seq_alloc bytes and the words of cig_alloc
    words each between guards"""

    def __init__(self, blob, rec, cst, seq_alloc, cig_alloc):
        import torch
        self.blob, self.rec, self.n, self.seq_alloc, self.cig_alloc = blob, rec, len(rec), seq_alloc, cig_alloc
        self.d_cols, self.d_cwin = _upload(blob), _upload(rec)
        self.d_cst = None if cst is None else _upload(np.asarray(cst, dtype=np.uint32))
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        n = self.n
        self.d_seq, self.d_sq, self.d_sa = (_arena(self.seq_alloc) for _ in range(3))
        self.d_cig = _arena(4 * self.cig_alloc)
        self.d_soff, self.d_coff, self.d_rec = _filled(8 * (n + 1)), _filled(8 * (n + 1)), _filled(32 * n)

    def pointers(self, cols_cap, min_cov, seq_cap, cig_cap, null_seq=False, null_cig=False):
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        seqs = [None] * 3 if null_seq else [p(self.d_seq, GUARD), p(self.d_sq, GUARD), p(self.d_sa, GUARD)]
        return [p(self.d_cols), cols_cap, p(self.d_cwin), self.n, None if self.d_cst is None else p(self.d_cst), min_cov] + seqs + \
               [seq_cap, p(self.d_soff), None if null_cig else p(self.d_cig, GUARD), cig_cap, p(self.d_coff), p(self.d_rec)]

    def run(self, ctx, cols_cap, min_cov, seq_cap, cig_cap, null_seq=False, null_cig=False):
        import torch
        import bsalign_amd as B
        assert cols_cap <= len(self.blob) and seq_cap <= self.seq_alloc and cig_cap <= self.cig_alloc and not (null_seq and seq_cap) and not (null_cig and cig_cap)
        rc = B.lib().bsa_window_stitch_run(ctx.h, *self.pointers(cols_cap, min_cov, seq_cap, cig_cap, null_seq, null_cig))
        assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        g, n = Got(), self.n
        g.seq, g.seq_qlt, g.seq_alt = (_inside(t, self.seq_alloc, "a sequence array") for t in (self.d_seq, self.d_sq, self.d_sa))
        g.cig = _inside(self.d_cig, 4 * self.cig_alloc, "the words").view(np.uint32)
        g.seq_off, g.cig_off = _down(self.d_soff, 8 * (n + 1), np.uint64), _down(self.d_coff, 8 * (n + 1), np.uint64)
        g.rec = _down(self.d_rec, 32 * n, WS.STITCH_DTYPE)
        g.cols = self.d_cols.cpu().numpy()[:len(self.blob)].copy()
        return g


def _host(ctx, blob, rec, cst, cols_cap, min_cov, seq_cap, cig_cap, seq_alloc=None, cig_alloc=None, null_seq=False, null_cig=False):
    """bsa_window_stitch_batch on host arrays prefilled with 0xA5 -> (rc, Got)"""
    import bsalign_amd as B
    n = len(rec)
    g = Got()
    seq_alloc, cig_alloc = seq_cap if seq_alloc is None else seq_alloc, cig_cap if cig_alloc is None else cig_alloc
    g.cols = np.ascontiguousarray(blob).copy()
    g.seq, g.seq_qlt, g.seq_alt = (np.full(max(seq_alloc, 1), FILL, np.uint8) for _ in range(3))
    g.cig = np.full(max(cig_alloc, 1), FILL32, np.uint32)
    g.seq_off, g.cig_off = np.full(n + 1, FILL64, np.uint64), np.full(n + 1, FILL64, np.uint64)
    g.rec = np.full(8 * max(n, 1), FILL32, np.uint32).view(WS.STITCH_DTYPE)
    cst = None if cst is None else np.ascontiguousarray(cst, dtype=np.uint32)
    seqs = [None] * 3 if null_seq else [B._p(g.seq), B._p(g.seq_qlt), B._p(g.seq_alt)]
    rc = B.lib().bsa_window_stitch_batch(ctx.h, B._p(g.cols) if len(blob) else None, cols_cap, B._p(rec), n, None if cst is None else B._p(cst), min_cov, *seqs, seq_cap,
                                         B._p(g.seq_off), None if null_cig else B._p(g.cig), cig_cap, B._p(g.cig_off), B._p(g.rec))
    g.seq, g.seq_qlt, g.seq_alt, g.cig, g.rec = g.seq[:seq_alloc], g.seq_qlt[:seq_alloc], g.seq_alt[:seq_alloc], g.cig[:cig_alloc], g.rec[:n]
    assert np.array_equal(g.cols, blob), "the columns are read-only"
    return rc, g


def _same(got, ref, seq_cap, cig_cap, what):
    for name in WS.STITCH_DTYPE.names:
        assert np.array_equal(got.rec[name], ref.rec[name]), (what, name, got.rec[name], ref.rec[name])
    assert np.array_equal(got.seq_off, ref.seq_off), (what, "seq_off", got.seq_off, ref.seq_off)
    assert np.array_equal(got.cig_off, ref.cig_off), (what, "cig_off", got.cig_off, ref.cig_off)
    for name, cap, fill in (("seq", seq_cap, FILL), ("seq_qlt", seq_cap, FILL), ("seq_alt", seq_cap, FILL), ("cig", cig_cap, FILL32)):
        a, b = getattr(got, name), getattr(ref, name)
        bad = np.flatnonzero(a[:cap] != b)
        assert len(bad) == 0, (what, name, bad[:8], a[bad[:8]], b[bad[:8]])
        assert np.all(a[cap:] == fill), (what, name, "something at or above the cap was written")


def _both(ctx, blob, rec, cst, min_cov, what, cols_cap=None, slack=3):
    """_run and _batch against the reference with arenas of the sum of mlen (it suffices for both) -> the reference"""
    cols_cap = len(blob) if cols_cap is None else cols_cap
    cap = sum(int(w["mlen"]) for w in rec if WS.readable(w, cols_cap))
    ref = WS.window_stitch_ref(blob, rec, cols_cap, cst, min_cov, cap, cap)
    dev = _Dev(blob, rec, cst, cap + slack, cap + slack)
    got = dev.run(ctx, cols_cap, min_cov, cap, cap)
    _same(got, ref, cap, cap, what + " (run)")
    assert np.array_equal(got.cols, blob), "the columns are read-only"
    rc, hgot = _host(ctx, blob, rec, cst, cols_cap, min_cov, cap, cap)
    assert rc == 0
    _same(hgot, ref, cap, cap, what + " (batch)")
    return ref


# ---- 1. the header's examples ----------------------------------------------------------------------------------------------------------------------
def test_header_example_1(ctx):
    WS.need_symbols()
    cols, rec, want = WS.header_example_1()
    for key, (seq, qlt, words, eq, x, ins, dl, kept) in want.items():
        cst, min_cov = (np.array([3], np.uint32), 0) if key == "draft" else (None, key)
        ref = _both(ctx, cols, rec, cst, min_cov, "example 1, %s" % key)
        assert ref.rec[0].tolist() == (1 if key == "draft" else 0, len(seq), eq, x, ins, dl, kept, len(words))
        assert ref.seq[:len(seq)].tolist() == seq and ref.seq_qlt[:len(seq)].tolist() == qlt and ref.cig[:len(words)].tolist() == words


def test_header_example_2(ctx):
    WS.need_symbols()
    cols, rec, want = WS.header_example_2()
    for min_cov, (seq, q, a, words, ins, kept) in want.items():
        ref = _both(ctx, cols, rec, None, min_cov, "example 2, min_cov %d" % min_cov)
        k = len(seq)
        assert ref.seq[:k].tolist() == seq and ref.seq_qlt[:k].tolist() == q and ref.seq_alt[:k].tolist() == a and ref.cig[:len(words)].tolist() == words
        assert int(ref.rec[0]["ins"]) == ins and int(ref.rec[0]["kept"]) == kept


# ---- 2. mixed batches against the reference ----------------------------------------------------------------------------------------------------------
def _mixed(name):
    WS.need_symbols()
    if "mixed" not in _CASES:
        _CASES["mixed"] = WS.mixed_batches()
    return _CASES["mixed"][name]


MIXED_NAMES = ["mlen_%d" % m for m in WS.MLENS] + ["by_rows", "long_window", "hand_made", "cns_status", "overlapping"]


def test_every_mixed_batch_is_run():
    _mixed("mlen_0")
    assert sorted(MIXED_NAMES) == sorted(_CASES["mixed"])


@pytest.mark.parametrize("name", MIXED_NAMES)
def test_mixed_batches_equal_the_reference(ctx, name):
    """every nall with every mlen in one batch, every min_cov of the issue's list; _run on uploaded tensors and _batch"""
    blob, rec, cst = _mixed(name)
    covs = WS.min_covs(rec) if name != "by_rows" else [0, 1, 40, WS.TILE_1_NALL, 0xFFFFFFFF]
    kept = set()
    for min_cov in covs:
        ref = _both(ctx, blob, rec, cst, min_cov, "%s, min_cov %d" % (name, min_cov))
        for g in range(0, len(rec), 3):
            WS.check_invariants(ref, g)
            WS.cigar_apply(ref.win[g][4], ref.win[g][0], ref.win[g][3])
        kept.add(int(ref.rec["kept"].sum()))
    if name != "mlen_0":
        assert len(kept) >= 2                                  # min_cov moves columns between the consensus and the draft


# ---- 3. behind a real bsa_window_cns_run ---------------------------------------------------------------------------------------------------------------
def _cns_resident(ctx, d_cols, cols_cap, d_cwin, nwin, max_rows, out_cap, pack):
    """Context.window_cns_run on resident columns -> Got: clen, status, seq_off and the compact arrays as they come down (pack), the columns stay"""
    import torch
    d = {k: _filled(out_cap) for k in ("cns", "qlt", "alt", "seq", "seq_qlt", "seq_alt")}
    d_clen, d_status, d_soff = _filled(4 * nwin), _filled(4 * nwin), _filled(8 * (nwin + 1))
    model = _CASES.setdefault("model", ctx.cns_model(PAR7))
    if pack:
        ctx.window_cns_run(model, d_cols, cols_cap, d_cwin, nwin, max_rows, d["cns"], d["qlt"], d["alt"], out_cap, d_clen, None, d_status,
                           d["seq"], d["seq_qlt"], d["seq_alt"], out_cap, d_soff)
    else:
        ctx.window_cns_run(model, d_cols, cols_cap, d_cwin, nwin, max_rows, d["cns"], d["qlt"], d["alt"], out_cap, d_clen, None, d_status)
    ctx.sync()
    torch.cuda.synchronize()
    g = Got()
    for k in ("seq", "seq_qlt", "seq_alt"):
        setattr(g, k, d[k].cpu().numpy()[:out_cap].copy())
    g.clen, g.status, g.seq_off = _down(d_clen, 4 * nwin, np.uint32), _down(d_status, 4 * nwin, np.uint32), _down(d_soff, 8 * (nwin + 1), np.uint64)
    g.d_status = d_status
    return g


def _stitch_resident(ctx, d_cols, cols_cap, d_cwin, nwin, d_status, min_cov, cap):
    """Context.window_stitch_run behind it on the same buffers, no copy in between -> Got"""
    import torch
    d_seq, d_sq, d_sa, d_cig = _arena(cap), _arena(cap), _arena(cap), _arena(4 * cap)
    d_soff, d_coff, d_rec = _filled(8 * (nwin + 1)), _filled(8 * (nwin + 1)), _filled(32 * nwin)
    view = lambda t, nbytes: t[GUARD:GUARD + max(nbytes, 16)]
    ctx.window_stitch_run(d_cols, cols_cap, d_cwin, nwin, d_status, min_cov, view(d_seq, cap), view(d_sq, cap), view(d_sa, cap), cap, d_soff, view(d_cig, 4 * cap), cap, d_coff, d_rec)
    ctx.sync()
    torch.cuda.synchronize()
    g = Got()
    g.seq, g.seq_qlt, g.seq_alt = (_inside(t, cap, "a sequence array") for t in (d_seq, d_sq, d_sa))
    g.cig = _inside(d_cig, 4 * cap, "the words").view(np.uint32)
    g.seq_off, g.cig_off, g.rec = _down(d_soff, 8 * (nwin + 1), np.uint64), _down(d_coff, 8 * (nwin + 1), np.uint64), _down(d_rec, 32 * nwin, WS.STITCH_DTYPE)
    g.cols = d_cols.cpu().numpy()[:cols_cap].copy()
    return g


def test_min_cov_0_behind_the_consensus_pass_is_its_compaction(ctx):
    """a batch whose windows are all live: the stitch's sequence, both qualities and offsets are the consensus pass's compact arrays, byte for byte"""
    WS.need_symbols()
    rng = np.random.default_rng(733)
    shapes = [(5, 40), (2, 1), (9, 64), (3, 0), (65, 17), (41, 130), (6, 200), (126, 70)]
    blob, rec = WC.make_batch([(WC.random_msa(rng, nall, mlen), nall - 1, nall - 1) for nall, mlen in shapes])
    n, cap = len(rec), int(rec["mlen"].sum())
    d_cols, d_cwin = _upload(blob), _upload(rec)
    cns = _cns_resident(ctx, d_cols, len(blob), d_cwin, n, 125, cap, True)
    assert np.all(cns.status == 0) and int(cns.seq_off[n]) > 0
    got = _stitch_resident(ctx, d_cols, len(blob), d_cwin, n, cns.d_status, 0, cap)
    need = int(cns.seq_off[n])
    assert np.array_equal(got.seq_off, cns.seq_off) and np.array_equal(got.rec["slen"], cns.clen) and np.all(got.rec["status"] == 0) and np.all(got.rec["kept"] == 0)
    for name in ("seq", "seq_qlt", "seq_alt"):
        assert np.array_equal(getattr(got, name)[:need], getattr(cns, name)[:need]), name
        assert np.all(getattr(got, name)[need:] == FILL), name
    _same(got, WS.window_stitch_ref(got.cols, rec, len(blob), cns.status, 0, cap, cap), cap, cap, "behind the consensus pass")


def test_windows_the_consensus_pass_refuses_come_out_as_their_draft_rows(ctx):
    """dead windows interleaved -- nseq = max_rows + 1, an output range past out_cap --: with the pass's d_status they are DRAFT"""
    WS.need_symbols()
    rng = np.random.default_rng(734)
    max_rows = 4
    ws = [(WC.random_msa(rng, 6, int(rng.integers(20, 90))), 5 if g in (1, 4) else 4, 5 if g in (1, 4) else 4) for g in range(7)]
    blob, rec = WC.make_batch(ws)
    n, cap = len(rec), int(rec["mlen"].sum())
    rec[5]["out_off"] = cap - int(rec[5]["mlen"]) + 1            # one byte past out_cap
    d_cols, d_cwin = _upload(blob), _upload(rec)
    cns = _cns_resident(ctx, d_cols, len(blob), d_cwin, n, max_rows, cap, False)
    assert cns.status.tolist() == [0, WC.ST_TOO_DEEP, 0, 0, WC.ST_TOO_DEEP, WC.ST_NO_ROOM, 0]
    got = _stitch_resident(ctx, d_cols, len(blob), d_cwin, n, cns.d_status, 1, cap)
    ref = WS.window_stitch_ref(got.cols, rec, len(blob), cns.status, 1, cap, cap)
    _same(got, ref, cap, cap, "refused windows")
    assert got.rec["status"].tolist() == [0, 1, 0, 0, 1, 1, 0]
    for g in (1, 4, 5):
        a, b, c = int(got.seq_off[g]), int(got.seq_off[g + 1]), int(got.cig_off[g])
        draft = blob[int(rec[g]["cols_off"]):].reshape(-1)[:int(rec[g]["mlen"]) * 9].reshape(-1, 9)[:, 5]
        assert np.array_equal(got.seq[a:b], draft[draft <= 3]) and np.all(got.seq_qlt[a:b] == 0) and np.all(got.seq_alt[a:b] == 0)
        assert int(got.cig_off[g + 1]) == c + 1 and int(got.cig[c]) == (b - a) << 4 | WS.OP_EQ and int(got.rec[g]["kept"]) == b - a
    # without the statuses every window counts as called: the refused windows' consensus bytes are still 4 0 0, so their covered columns are deletions
    blind = _stitch_resident(ctx, d_cols, len(blob), d_cwin, n, None, 1, cap)
    _same(blind, WS.window_stitch_ref(got.cols, rec, len(blob), None, 1, cap, cap), cap, cap, "no statuses")
    assert np.all(blind.rec["status"] == 0) and int(blind.rec[1]["del"]) > 0


# ---- 4. records that fail --------------------------------------------------------------------------------------------------------------------------
def test_every_way_a_record_fails(ctx):
    WS.need_symbols()
    blob, rec, cols_cap, cst, want, names = WS.bad_batch()
    assert cols_cap == len(blob)                               # the columns end where their allocation ends
    for min_cov in (0, 1, 4):
        ref = _both(ctx, blob, rec, cst, min_cov, "failing records, min_cov %d" % min_cov, cols_cap=cols_cap)
        assert ref.rec["status"].tolist() == want
    # one byte less: the last window is not readable any more, nothing else changes
    ref = _both(ctx, blob, rec, cst, 1, "failing records, cols_cap - 1", cols_cap=cols_cap - 1)
    assert ref.rec["status"].tolist() == want[:-1] + [WS.ST_BAD_RECORD]


# ---- 5. the arena contract ---------------------------------------------------------------------------------------------------------------------------
def _arena_case():
    WS.need_symbols()
    if "arena" not in _CASES:
        blob, rec, cst = WS.arena_batch()
        total = int(rec["mlen"].sum())
        _CASES["arena"] = (blob, rec, cst, total, WS.window_stitch_ref(blob, rec, len(blob), cst, 1, total, total))
    return _CASES["arena"]


def _border_caps(off, top):
    ends = sorted(set(int(x) for x in off[1:]))
    return sorted(set(c for e in ends for c in (e - 1, e, e + 1) if 0 <= c <= top) | {0})


def test_any_seq_cap(ctx):
    """every seq_cap at, just before and just after a window border, the words' arena large: the offsets and records are those of a large run, a
    window's bases are written whole if and only if its range ends inside seq_cap, every word is written"""
    blob, rec, cst, total, full = _arena_case()
    need_s, need_c = int(full.seq_off[-1]), int(full.cig_off[-1])
    dev = _Dev(blob, rec, cst, need_s + 1, need_c + 1)
    for cap, null in [(c, False) for c in _border_caps(full.seq_off, need_s + 1)] + [(0, True)]:
        dev.fresh()
        ref = WS.window_stitch_ref(blob, rec, len(blob), cst, 1, cap, need_c)
        assert np.array_equal(ref.cig, full.cig[:need_c])
        _same(dev.run(ctx, len(blob), 1, cap, need_c, null_seq=null), ref, cap, need_c, "seq_cap %d%s" % (cap, " (NULL arrays)" if null else ""))


def test_any_cig_cap(ctx):
    """the reverse: every cig_cap around every border, the sequence arena large"""
    blob, rec, cst, total, full = _arena_case()
    need_s, need_c = int(full.seq_off[-1]), int(full.cig_off[-1])
    dev = _Dev(blob, rec, cst, need_s + 1, need_c + 1)
    for cap, null in [(c, False) for c in _border_caps(full.cig_off, need_c + 1)] + [(0, True)]:
        dev.fresh()
        ref = WS.window_stitch_ref(blob, rec, len(blob), cst, 1, need_s, cap)
        assert np.array_equal(ref.seq, full.seq[:need_s])
        _same(dev.run(ctx, len(blob), 1, need_s, cap, null_cig=null), ref, need_s, cap, "cig_cap %d%s" % (cap, " (NULL arena)" if null else ""))


def test_count_only_and_missing_quality_arrays(ctx):
    import bsalign_amd as B
    blob, rec, cst, total, full = _arena_case()
    need_s, need_c = int(full.seq_off[-1]), int(full.cig_off[-1])
    dev = _Dev(blob, rec, cst, need_s, need_c)
    none = WS.window_stitch_ref(blob, rec, len(blob), cst, 1, 0, 0)
    for null in (False, True):                                 # caps 0 with arenas, and without
        dev.fresh()
        got = dev.run(ctx, len(blob), 1, 0, 0, null_seq=null, null_cig=null)
        _same(got, none, 0, 0, "count only")
        assert np.array_equal(got.rec, full.rec) and int(got.seq_off[-1]) == need_s and int(got.cig_off[-1]) == need_c
    for skip in (7, 8):                                        # either quality array may be missing
        dev.fresh()
        args = dev.pointers(len(blob), 1, need_s, need_c)
        args[skip] = None
        assert B.lib().bsa_window_stitch_run(ctx.h, *args) == 0
        ctx.sync()
        got = dev.read()
        assert np.array_equal(got.seq, full.seq[:need_s]) and np.array_equal(got.cig, full.cig[:need_c]) and np.array_equal(got.rec, full.rec)
        assert np.all((got.seq_qlt if skip == 7 else got.seq_alt) == FILL)
        assert np.array_equal(got.seq_alt if skip == 7 else got.seq_qlt, (full.seq_alt if skip == 7 else full.seq_qlt)[:need_s])


def test_batch_with_short_arenas(ctx):
    import bsalign_amd as B
    blob, rec, cst, total, full = _arena_case()
    need_s, need_c = int(full.seq_off[-1]), int(full.cig_off[-1])
    for scap, ccap, ns, nc in ((0, 0, False, False), (0, 0, True, True), (need_s - 1, need_c, False, False), (need_s, need_c - 1, False, False), (1, total, False, False),
                               (total, 1, False, False)):
        rc, got = _host(ctx, blob, rec, cst, len(blob), 1, scap, ccap, seq_alloc=need_s, cig_alloc=need_c, null_seq=ns, null_cig=nc)
        assert rc == E_CIGAR_CAP and np.array_equal(got.seq_off, full.seq_off) and np.array_equal(got.cig_off, full.cig_off), (scap, ccap)          # both totals
        assert np.all(got.seq == FILL) and np.all(got.seq_qlt == FILL) and np.all(got.seq_alt == FILL) and np.all(got.cig == FILL32), (scap, ccap)
        assert np.array_equal(got.rec, full.rec) and B.lib().bsa_last_error(ctx.h), (scap, ccap)
    rc, got = _host(ctx, blob, rec, cst, len(blob), 1, need_s, need_c)
    assert rc == 0
    _same(got, WS.window_stitch_ref(blob, rec, len(blob), cst, 1, need_s, need_c), need_s, need_c, "batch, exact caps")


# ---- 6. behind the real passes ---------------------------------------------------------------------------------------------------------------------
def _msa_resident(ctx, b, vote):
    """bsa_window_msa_run on a window_msa_cases.Batch -> (d_cols, cols_cap, d_cwin, the records the reference gives); nothing comes down"""
    roff, rcwin, _ = W.window_msa_ref(b, vote)
    cap = int(roff[-1])
    up = [_upload(x) for x in (b.piece, b.piece_off, b.bases, b.pcig, b.pcig_off, b.draft, b.doff, b.dlen)]
    d_cols, d_coff, d_cwin = _filled(cap), _filled(8 * (b.nwin + 1)), _filled(40 * b.nwin)
    ctx.window_msa_run(up[0], up[1], b.nwin, b.piece_cap, up[2], b.bases_cap, up[3], b.pcig_cap, up[4], up[5], up[6], up[7], b.window, 0, vote, d_cols, cap, d_coff, d_cwin)
    return d_cols, cap, d_cwin, rcwin


def test_closed_loop_with_a_coverage_hole(ctx):
    """the closed loop of the CPU test on the device: bsa_window_msa_run, bsa_window_cns_run without its compaction, bsa_window_stitch_run, no copy in
    between.  At min_cov 1 the draft's stitched sequence is the truth where a read covers and the draft where none does."""
    WS.need_symbols()
    truth, draft, b, want = WS.closed_loop_with_hole()
    d_cols, cap, d_cwin, rcwin = _msa_resident(ctx, b, 0)
    out_cap = int(rcwin["mlen"].sum())
    cns = _cns_resident(ctx, d_cols, cap, d_cwin, b.nwin, 4, out_cap, False)
    assert np.all(cns.status == 0) and int(cns.clen.sum()) == len(want) - 385
    got = _stitch_resident(ctx, d_cols, cap, d_cwin, b.nwin, cns.d_status, 1, out_cap)
    _same(got, WS.window_stitch_ref(got.cols, rcwin, cap, cns.status, 1, out_cap, out_cap), out_cap, out_cap, "closed loop")
    assert np.array_equal(got.seq[:int(got.seq_off[b.nwin])], want) and int(got.rec["kept"].sum()) == 385
    words = got.cig[:int(got.cig_off[b.nwin])]
    eq, x, ins, dl = (sum(int(w) >> 4 for w in words if int(w) & 15 == op) for op in (WS.OP_EQ, WS.OP_X, WS.OP_I, WS.OP_D))
    assert eq + x + dl == len(draft) and eq + x + ins == len(want) and x > 0 and ins > 0 and dl > 0


def test_all_six_resident_passes_on_aligner_output(ctx):
    """align_batch's records and words uploaded, then windows, pieces, guides, MSA, consensus and stitch on the device at w = 50.  Two of the six
    reads end at draft base 260: behind it four reads cover, and at min_cov 5 the draft is kept there"""
    import bsalign_amd as B
    WS.need_symbols()
    w, cut, min_cov = 50, 260, 5
    rng = np.random.default_rng(1812)
    draft = rng.integers(0, 4, 430).astype(np.uint8)
    pairs = [(S.mutate(rng, draft, 0.10), draft) for _ in range(4)] + [(S.mutate(rng, draft[:cut], 0.10), draft[:cut]) for _ in range(2)]
    n = len(pairs)
    out, cigs, st = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, 64, 2, -6, -3, -2, 0, 0))
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    coff = np.zeros(n + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(c) for c in cigs], dtype=np.uint64)
    arena = np.concatenate(cigs).astype(np.uint32)
    ins = int(sum(int(x) >> 4 for c in cigs for x in c if int(x) & 15 == 1))
    gbase, nwin = B.window_gbase([0] * n, [len(draft)], w)
    win_cap = B.cigar_windows_bound(tlen, w)
    piece_cap, bases_cap, pcig_cap = win_cap, int(qlen.sum()), B.piece_cigars_bound(coff, win_cap)
    doff, dlen = B.window_drafts([int(toff[0])], [len(draft)], w)          # the draft: the first pair's target in the blob
    cols_cap, out_cap = (nwin * w + ins) * (n + 4), nwin * w + ins
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
    cns = _cns_resident(ctx, d_cols, cols_cap, d_cwin, nwin, n, out_cap, False)
    got = _stitch_resident(ctx, d_cols, cols_cap, d_cwin, nwin, cns.d_status, min_cov, out_cap)
    rec = _down(d_cwin, 40 * nwin, CNS_WINDOW_DTYPE)
    assert np.all(cns.status == 0) and rec["nall"].tolist() == [7] * 6 + [5] * 3
    ref = WS.window_stitch_ref(got.cols, rec, cols_cap, cns.status, min_cov, out_cap, out_cap)
    _same(got, ref, out_cap, out_cap, "six passes")
    for g in range(nwin):
        WS.check_invariants(ref, g)
        WS.cigar_apply(ref.win[g][4], ref.win[g][0], ref.win[g][3])
        assert np.array_equal(ref.win[g][4], draft[g * w:(g + 1) * w])
    assert np.all(got.rec["status"] == 0) and np.all(got.rec["kept"][6:] == got.rec["slen"][6:]) and int(got.rec["kept"][:5].sum()) < int(got.rec["slen"][:5].sum()) // 2
    assert np.array_equal(got.seq[int(got.seq_off[6]):int(got.seq_off[nwin])], draft[300:])
    # the host-pointer calls give the same windows
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(pairs, wins, w, gbase, nwin)
    msas = ctx.window_msa(wp, ctx.piece_cigars(out, cigs, wp), [draft[int(o) - int(toff[0]):int(o) - int(toff[0]) + min(int(k), w)] for o, k in zip(doff, dlen)], w, vote=False)
    res, _ = ctx.window_cns(msas, PAR7)
    per, (seq, sq, sa, soff, cig, cgoff) = ctx.window_stitch(res, min_cov=min_cov)
    ns, nc = int(got.seq_off[nwin]), int(got.cig_off[nwin])
    assert np.array_equal(soff, got.seq_off) and np.array_equal(cgoff, got.cig_off) and np.array_equal(seq, got.seq[:ns]) and np.array_equal(cig, got.cig[:nc])
    assert np.array_equal(sq, got.seq_qlt[:ns]) and np.array_equal(sa, got.seq_alt[:ns])
    for g, (s, q, a, ws, r) in enumerate(per):
        assert np.array_equal(s, ref.win[g][0]) and np.array_equal(ws, ref.win[g][3]) and r.tolist() == ref.rec[g].tolist(), g
    per2, _ = ctx.window_stitch([(cols, None) for _, _, _, _, _, cols in res], min_cov=min_cov, status=[0] * nwin)          # (cols, cwin) pairs with a status list
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) for a, b in zip(per, per2))


# ---- 7. re-run -----------------------------------------------------------------------------------------------------------------------------------------
def test_second_run_and_another_min_cov(ctx):
    blob, rec, cst = _mixed("mlen_129")
    cap = int(rec["mlen"].sum())
    dev = _Dev(blob, rec, cst, cap, cap)
    one = dev.run(ctx, len(blob), 2, cap, cap)
    _same(one, WS.window_stitch_ref(blob, rec, len(blob), cst, 2, cap, cap), cap, cap, "first run")
    two = dev.run(ctx, len(blob), 2, cap, cap)                  # into the same arrays
    names = ("seq", "seq_qlt", "seq_alt", "cig", "seq_off", "cig_off", "rec", "cols")
    for name in names:
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    dev.fresh()
    _same(dev.run(ctx, len(blob), 0, cap, cap), WS.window_stitch_ref(blob, rec, len(blob), cst, 0, cap, cap), cap, cap, "another min_cov")
    dev.fresh()
    three = dev.run(ctx, len(blob), 2, cap, cap)
    for name in names:
        assert np.array_equal(getattr(one, name), getattr(three, name)), name


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    blob, rec, cst, total, full = _arena_case()
    need_s, need_c = int(full.seq_off[-1]), int(full.cig_off[-1])
    dev = _Dev(blob, rec, cst, need_s, need_c)
    run, batch, err = B.lib().bsa_window_stitch_run, B.lib().bsa_window_stitch_batch, B.lib().bsa_last_error
    rargs = [ctx.h] + dev.pointers(len(blob), 1, need_s, need_c)
    h = Got()
    h.cols, h.cst = blob.copy(), np.ascontiguousarray(cst)
    h.seq, h.sq, h.sa = (np.full(need_s, FILL, np.uint8) for _ in range(3))
    h.cig, h.soff, h.coff, h.rec = np.full(need_c, FILL32, np.uint32), np.zeros(9, np.uint64), np.zeros(9, np.uint64), np.zeros(8, WS.STITCH_DTYPE)
    bargs = [ctx.h, B._p(h.cols), len(blob), B._p(rec), 8, B._p(h.cst), 1, B._p(h.seq), B._p(h.sq), B._p(h.sa), need_s, B._p(h.soff), B._p(h.cig), need_c, B._p(h.coff), B._p(h.rec)]

    def refused(fn, base, changes):
        a = list(base)
        for i, v in changes.items():
            a[i] = v
        assert fn(*a) == E_ARG, (fn.__name__, changes)
        if 0 not in changes:
            assert err(ctx.h), (fn.__name__, changes)
    for fn, base in ((run, rargs), (batch, bargs)):
        # no context, columns (with a cap), records, sequence (with a cap), seq_off, words (with a cap), cig_off, d_rec
        for i in (0, 1, 3, 7, 11, 12, 14, 15):
            refused(fn, base, {i: None})
        refused(fn, base, {7: None, 10: 0})                    # quality arrays without the sequence
        refused(fn, base, {7: None, 8: None, 10: 0})           # one quality array without the sequence
        refused(fn, base, {4: 0xFFFFFFF1})                     # nwin
    # nothing was launched by the refused calls; the good calls still run
    assert np.all(h.seq == FILL) and np.all(h.cig == FILL32)
    assert run(*rargs) == 0
    ctx.sync()
    _same(dev.read(), WS.window_stitch_ref(blob, rec, len(blob), cst, 1, need_s, need_c), need_s, need_c, "after the refused calls")
    assert batch(*bargs) == 0 and np.array_equal(h.seq, full.seq[:need_s]) and np.array_equal(h.cig, full.cig[:need_c]) and np.array_equal(h.soff, full.seq_off)
    assert np.array_equal(h.coff, full.cig_off) and np.array_equal(h.rec, full.rec)
    # no windows: the two zero offsets and nothing else; NULL is fine where there is no work
    dev.fresh()
    a = [ctx.h] + dev.pointers(len(blob), 1, need_s, need_c)
    a[4] = 0
    assert run(*a) == 0
    ctx.sync()
    got = dev.read()
    assert got.seq_off.tolist()[:2] == [0, FILL64] and got.cig_off.tolist()[:2] == [0, FILL64] and np.all(got.seq == FILL) and np.all(got.cig == FILL32)
    assert np.all(got.rec["status"] == FILL32)
    off = np.full(2, FILL64, np.uint64)
    assert batch(ctx.h, None, 0, None, 0, None, 1, None, None, None, 0, B._p(off[:1]), None, 0, B._p(off[1:]), None) == 0 and off.tolist() == [0, 0]
    d_off = _filled(16)
    p = lambda o: C.c_void_p(d_off.data_ptr() + o)
    assert run(ctx.h, None, 0, None, 0, None, 1, None, None, None, 0, p(0), None, 0, p(8), None) == 0
    ctx.sync()
    assert _down(d_off, 16, np.uint64).tolist() == [0, 0]
    # the Python plumbing's size checks
    import torch
    t = lambda nbytes: torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    good = dict(d_cols=t(len(blob)), d_cwin=t(320), d_cns_status=t(32), d_seq=t(need_s), d_seq_qlt=t(need_s), d_seq_alt=t(need_s), d_seq_off=t(72), d_cig=t(4 * need_c),
                d_cig_off=t(72), d_rec=t(256))
    call = lambda **kw: ctx.window_stitch_run(kw["d_cols"], len(blob), kw["d_cwin"], 8, kw["d_cns_status"], 1, kw["d_seq"], kw["d_seq_qlt"], kw["d_seq_alt"], need_s, kw["d_seq_off"],
                                              kw["d_cig"], need_c, kw["d_cig_off"], kw["d_rec"])
    call(**good)
    for k in good:
        with pytest.raises(ValueError):
            call(**dict(good, **{k: good[k][:-1]}))
