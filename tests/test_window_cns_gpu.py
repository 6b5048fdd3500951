"""GPU: bsa_window_cns_run and bsa_window_cns_batch (include/bsalign_hip.h) against the Python statement of the definition
(window_cns_cases.window_cns_ref: the predicate in Python integers, the HOST consensus caller for every live window, the compaction): against the host
form on random MSAs, bit for bit against bsa_msa_call_consensus_batch on the same bytes, on the reference fixture, on dead windows, for any capacity of
the output and the compact arenas, behind the real passes, run twice and with two models, and the argument errors.

Tolerance: consensus, both quality strings, clen, status, every byte of every column and the compact arrays and offsets are compared byte for byte; the
log probability of the best path to a relative 1e-12 against the host form -- the tolerance tests/test_cns_gpu.py states for the device form, whose cause
(the device's exp / log in the merges) is unchanged -- and bit for bit against bsa_msa_call_consensus_batch, which runs the same kernels on the same tables.

Every buffer a run writes is prefilled with 0xA5 bytes and every arena has 256 guard bytes on either side.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

import support as S
import window_cns_cases as WC
import window_msa_cases as W
from window_msa_cases import CNS_WINDOW_DTYPE, NO_IDXS, PAR7

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = WC.FILL
REL = 1e-12
E_ARG, E_CIGAR_CAP, E_UNSUPPORTED = -2, -5, -6
_MODELS, _HOST_FORM, _REFS = {}, {}, {}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


def _model(ctx, par):
    key = np.asarray(par, np.float32).tobytes()
    if key not in _MODELS:
        _MODELS[key] = ctx.cns_model(par)
    return _MODELS[key]


def _filled(nbytes):
    import torch
    return torch.full((max((nbytes + 15) // 16 * 16, 16),), FILL, dtype=torch.uint8, device="cuda")


def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.nbytes == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _arena(nbytes, init=None):
    """nbytes between two guards, 0xA5 throughout, `init` at its start"""
    t = _filled(nbytes + 2 * GUARD)
    if init is not None and len(init):
        t[GUARD:GUARD + len(init)] = _upload(init)[:len(init)]
    return t


def _inside(t, nbytes, what):
    w = t.cpu().numpy()
    assert np.all(w[:GUARD] == FILL) and np.all(w[GUARD + nbytes:] == FILL), "a guard byte of %s was written" % what
    return w[GUARD:GUARD + nbytes].copy()


class Got:
    pass


class _Dev:
    """one batch on the device: the column arena holds the blob, the output arrays out_alloc and the compact arrays seq_alloc bytes, each between guards"""

    def __init__(self, blob, rec, out_alloc, seq_alloc):
        import torch
        self.blob, self.rec, self.n, self.out_alloc, self.seq_alloc = blob, rec, len(rec), out_alloc, seq_alloc
        self.d_cwin = _upload(rec)
        self.fresh()
        torch.cuda.synchronize()

    def fresh(self):
        n = self.n
        self.d_cols = _arena(len(self.blob), self.blob)
        self.d_cns, self.d_qlt, self.d_alt = (_arena(self.out_alloc) for _ in range(3))
        self.d_seq, self.d_sq, self.d_sa = (_arena(self.seq_alloc) for _ in range(3))
        self.d_clen, self.d_score, self.d_status, self.d_soff = _filled(4 * n), _filled(8 * n), _filled(4 * n), _filled(8 * (n + 1))

    def pointers(self, model, cols_cap, out_cap, seq_cap, max_rows, pack=True, null_seq=False):
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        seqs = [None] * 3 if (null_seq or not pack) else [p(self.d_seq, GUARD), p(self.d_sq, GUARD), p(self.d_sa, GUARD)]
        return [model.h, p(self.d_cols, GUARD), cols_cap, p(self.d_cwin), self.n, max_rows, p(self.d_cns, GUARD), p(self.d_qlt, GUARD), p(self.d_alt, GUARD), out_cap,
                p(self.d_clen), p(self.d_score), p(self.d_status)] + seqs + [seq_cap if pack else 0, p(self.d_soff) if pack else None]

    def run(self, ctx, model, cols_cap, out_cap, seq_cap, max_rows, pack=True, null_seq=False):
        import torch
        import bsalign_amd as B
        assert cols_cap <= len(self.blob) and out_cap <= self.out_alloc and seq_cap <= self.seq_alloc and not (null_seq and seq_cap)
        rc = B.lib().bsa_window_cns_run(ctx.h, *self.pointers(model, cols_cap, out_cap, seq_cap, max_rows, pack, null_seq))
        assert rc == 0, (rc, (B.lib().bsa_last_error(ctx.h) or b"").decode())
        ctx.sync()
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        g, n = Got(), self.n
        g.cols = _inside(self.d_cols, len(self.blob), "the columns")
        g.cns, g.qlt, g.alt = (_inside(t, self.out_alloc, "an output array") for t in (self.d_cns, self.d_qlt, self.d_alt))
        g.seq, g.seq_qlt, g.seq_alt = (_inside(t, self.seq_alloc, "a compact array") for t in (self.d_seq, self.d_sq, self.d_sa))
        g.clen = self.d_clen.cpu().numpy()[:4 * n].view(np.uint32).copy()
        g.score = self.d_score.cpu().numpy()[:8 * n].view(np.float64).copy()
        g.status = self.d_status.cpu().numpy()[:4 * n].view(np.uint32).copy()
        g.seq_off = self.d_soff.cpu().numpy()[:8 * (n + 1)].view(np.uint64).copy()
        return g


def _host(ctx, par, blob, rec, cols_cap, out_cap, seq_cap, max_rows, out_alloc=None, seq_alloc=None, null_seq=False):
    """bsa_window_cns_batch on host arrays prefilled with 0xA5 -> (rc, Got)"""
    import bsalign_amd as B
    n = len(rec)
    g = Got()
    out_alloc, seq_alloc = out_cap if out_alloc is None else out_alloc, seq_cap if seq_alloc is None else seq_alloc
    g.cols = blob.copy()
    g.cns, g.qlt, g.alt = (np.full(max(out_alloc, 1), FILL, np.uint8) for _ in range(3))
    g.seq, g.seq_qlt, g.seq_alt = (np.full(max(seq_alloc, 1), FILL, np.uint8) for _ in range(3))
    g.clen, g.score, g.status = np.full(max(n, 1), 0xA5A5A5A5, np.uint32), np.full(max(n, 1), -1.5, np.float64), np.full(max(n, 1), 0xA5A5A5A5, np.uint32)
    g.seq_off = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    par = np.ascontiguousarray(par, np.float32)
    seqs = [None] * 3 if null_seq else [B._p(g.seq), B._p(g.seq_qlt), B._p(g.seq_alt)]
    rc = B.lib().bsa_window_cns_batch(ctx.h, B._p(par), B._p(g.cols) if len(blob) else None, cols_cap, B._p(rec), n, max_rows, B._p(g.cns), B._p(g.qlt), B._p(g.alt), out_cap,
                                      B._p(g.clen), B._p(g.score), B._p(g.status), *seqs, seq_cap, B._p(g.seq_off))
    for name in ("cns", "qlt", "alt"):
        setattr(g, name, getattr(g, name)[:out_alloc])
    for name in ("seq", "seq_qlt", "seq_alt"):
        setattr(g, name, getattr(g, name)[:seq_alloc])
    g.clen, g.score, g.status = g.clen[:n], g.score[:n], g.status[:n]
    return rc, g


def _same(got, ref, out_cap, seq_cap, what, exact_score=False, pack=True):
    assert np.array_equal(got.status, ref.status), (what, "status", got.status, ref.status)
    assert np.array_equal(got.clen, ref.clen), (what, "clen", got.clen, ref.clen)
    if exact_score:
        assert np.array_equal(got.score, ref.score), (what, "score", got.score, ref.score)
    else:
        assert np.all(np.abs(got.score - ref.score) <= REL * np.maximum(1.0, np.abs(ref.score))), (what, "score", got.score, ref.score)
    bad = np.flatnonzero(got.cols != ref.cols)
    assert len(bad) == 0, (what, "columns", bad[:8], got.cols[bad[:8]], ref.cols[bad[:8]])
    for name in ("cns", "qlt", "alt"):
        a, b = getattr(got, name), getattr(ref, name)
        bad = np.flatnonzero(a[:out_cap] != b)
        assert len(bad) == 0, (what, name, bad[:8], a[bad[:8]], b[bad[:8]])
        assert np.all(a[out_cap:] == FILL), (what, name, "a byte at or above out_cap was written")
    if not pack:
        return
    assert np.array_equal(got.seq_off, ref.seq_off), (what, "seq_off", got.seq_off, ref.seq_off)
    for name in ("seq", "seq_qlt", "seq_alt"):
        a, b = getattr(got, name), getattr(ref, name)
        bad = np.flatnonzero(a[:seq_cap] != b)
        assert len(bad) == 0, (what, name, bad[:8], a[bad[:8]], b[bad[:8]])
        assert np.all(a[seq_cap:] == FILL), (what, name, "a byte at or above seq_cap was written")


def _host_form(name):
    """(blob, records, out_cap, max_rows, the reference with a large compact arena): computed once"""
    WC.need_symbols()
    if not _HOST_FORM:
        _HOST_FORM.update(WC.host_form_batches())
    if name not in _REFS:
        blob, rec = _HOST_FORM[name]
        out_cap, max_rows = int(rec["mlen"].sum()), int(rec["nseq"].max())
        _REFS[name] = (blob, rec, out_cap, max_rows, WC.window_cns_ref(blob, rec, len(blob), out_cap, out_cap, max_rows, PAR7))
    return _REFS[name]


HOST_FORM_NAMES = ["mlen_%d" % m for m in WC.MLENS] + ["long_window"]


# ---- 1. against the host form --------------------------------------------------------------------------------------------------------------------
def test_every_host_form_batch_is_run():
    _host_form("mlen_1")
    assert sorted(HOST_FORM_NAMES) == sorted(_HOST_FORM)


@pytest.mark.parametrize("name", HOST_FORM_NAMES)
def test_random_msas_equal_the_host_form(ctx, name):
    """depths 1 .. 257 in one batch, max_rows the largest; _run on uploaded tensors and _batch"""
    blob, rec, out_cap, max_rows, ref = _host_form(name)
    assert np.all(ref.status == 0) and int(ref.seq_off[-1]) > 0
    dev = _Dev(blob, rec, out_cap + 3, out_cap + 5)
    _same(dev.run(ctx, _model(ctx, PAR7), len(blob), out_cap, out_cap, max_rows), ref, out_cap, out_cap, name + " (run)")
    rc, got = _host(ctx, PAR7, blob, rec, len(blob), out_cap, out_cap, max_rows)
    assert rc == 0
    _same(got, ref, out_cap, out_cap, name + " (batch)")


# ---- 2. against bsa_msa_call_consensus_batch on the same bytes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mlen_65", "mlen_200", "long_window"])
def test_equal_to_the_host_pointer_call_bit_for_bit(ctx, name):
    from bsalign_amd import msa as MSA
    blob, rec, out_cap, max_rows, _ = _host_form(name)
    wins = [(blob[int(w["cols_off"]):int(w["cols_off"]) + int(w["mlen"]) * (int(w["nall"]) + 3)].copy(), None, int(w["nall"]), int(w["nseq"]), int(w["nmax"]), int(w["mlen"]))
            for w in rec]
    out = MSA.call_consensus_batch(ctx, wins, PAR7)
    got = _Dev(blob, rec, out_cap, out_cap).run(ctx, _model(ctx, PAR7), len(blob), out_cap, out_cap, max_rows)
    for g, w in enumerate(rec):
        cns, qlt, alt, score, cols = out[g]
        o, k, c0 = int(w["out_off"]), len(cns), int(w["cols_off"])
        assert int(got.clen[g]) == k and got.score[g] == score, (name, g, got.score[g], score)          # the same bits
        assert np.array_equal(got.cns[o:o + k], cns) and np.array_equal(got.qlt[o:o + k], qlt) and np.array_equal(got.alt[o:o + k], alt), (name, g)
        assert np.array_equal(got.cols[c0:c0 + len(cols)], cols), (name, g)


# ---- 3. the reference fixture ----------------------------------------------------------------------------------------------------------------------
def test_fixture_of_the_real_cns_bspoa_as_one_resident_batch(ctx):
    WC.need_symbols()
    g = np.load(os.path.join(S.ROOT, "tests", "golden", "cns.npz"))
    n = int(g["n"][0])
    rec = np.zeros(n, dtype=CNS_WINDOW_DTYPE)
    parts, cacc, oacc = [], 0, 0
    for k in range(n):
        nmsa, nrds, nall, mlen = (int(x) for x in g["dims_%d" % k])
        mine = g["cols_%d" % k].copy().reshape(-1, nall + 3)
        mine[:, nall:] = 255                                   # nothing of the reference's answer left in the input
        rec[k] = (cacc, NO_IDXS, oacc, nall, min(nmsa, nrds), nrds, mlen)
        parts.append(mine.reshape(-1))
        cacc += mine.size
        oacc += mlen
    blob = np.concatenate(parts)
    max_rows = int(rec["nseq"].max())
    got = _Dev(blob, rec, oacc, oacc).run(ctx, _model(ctx, g["par_0"]), len(blob), oacc, oacc, max_rows)
    assert np.all(got.status == 0)
    for k in range(n):
        o, c0, a = int(rec[k]["out_off"]), int(rec[k]["cols_off"]), int(got.seq_off[k])
        cns, qlt, alt, score, cols = g["cns_%d" % k], g["qlt_%d" % k], g["alt_%d" % k], float(g["score_%d" % k][0]), g["cols_%d" % k].reshape(-1)
        m = len(cns)
        assert int(got.clen[k]) == m and np.array_equal(got.cns[o:o + m], cns) and np.array_equal(got.qlt[o:o + m], qlt) and np.array_equal(got.alt[o:o + m], alt), k
        nb = int(rec[k]["mlen"]) * (int(rec[k]["nall"]) + 3)
        assert np.array_equal(got.cols[c0:c0 + nb], cols[:nb]), k
        assert abs(got.score[k] - score) <= REL * max(1.0, abs(score)), (k, got.score[k], score)
        assert np.array_equal(got.seq[a:a + m], cns) and np.array_equal(got.seq_qlt[a:a + m], qlt) and np.array_equal(got.seq_alt[a:a + m], alt), k


# ---- 4. dead windows -------------------------------------------------------------------------------------------------------------------------------
def test_dead_windows(ctx):
    WC.need_symbols()
    blob, rec, cols_cap, out_cap, max_rows, want, names = WC.dead_batch()
    ref = WC.window_cns_ref(blob, rec, cols_cap, out_cap, out_cap, max_rows, PAR7)
    assert ref.status.tolist() == want
    dev = _Dev(blob, rec, out_cap + 9, out_cap)
    got = dev.run(ctx, _model(ctx, PAR7), cols_cap, out_cap, out_cap, max_rows)
    assert got.status.tolist() == want, dict(zip(names, got.status[1::2]))
    dead = np.flatnonzero(np.array(want) != 0)
    assert np.all(got.clen[dead] == 0) and np.all(got.score[dead] == 0.0)
    assert np.all(got.clen[np.array(want) == 0] > 0)
    _same(got, ref, out_cap, out_cap, "dead windows (run)")      # (the dead windows' columns as uploaded, their output ranges 0xA5: the reference leaves them so)
    # the dead windows' slots in the arena, 7 columns of 8 bytes each: rows as generated, 4 0 0 behind
    slots = got.cols.reshape(-1, 8)
    assert np.array_equal(slots[:, :5], blob.reshape(-1, 8)[:, :5])          # no run writes a row byte
    untouched = np.ones(len(slots), dtype=bool)
    for g in np.flatnonzero(np.array(want) == 0):
        untouched[int(rec[g]["cols_off"]) // 8:int(rec[g]["cols_off"]) // 8 + int(rec[g]["mlen"])] = False
    assert untouched.sum() == 7 * 9 and np.all(slots[untouched, 5:] == [4, 0, 0])
    rc, hgot = _host(ctx, PAR7, blob, rec, cols_cap, out_cap, out_cap, max_rows)
    assert rc == 0
    _same(hgot, ref, out_cap, out_cap, "dead windows (batch)")
    # without the optional arrays
    dev.fresh()
    args = dev.pointers(_model(ctx, PAR7), cols_cap, out_cap, out_cap, max_rows)
    args[11] = args[12] = None
    import bsalign_amd as B
    assert B.lib().bsa_window_cns_run(ctx.h, *args) == 0
    ctx.sync()
    g2 = dev.read()
    assert np.array_equal(g2.clen, ref.clen) and np.array_equal(g2.cns[:out_cap], ref.cns) and np.array_equal(g2.seq, ref.seq) and np.array_equal(g2.cols, ref.cols)
    assert np.all(g2.status == 0xA5A5A5A5)


# ---- 5. the arena contract -------------------------------------------------------------------------------------------------------------------------
def _arena_case():
    WC.need_symbols()
    if "arena" not in _REFS:
        blob, rec = WC.arena_batch()
        _REFS["arena"] = (blob, rec, int(rec["mlen"].sum()), int(rec["nseq"].max()))
    return _REFS["arena"]


def test_any_out_cap(ctx):
    """every out_cap at, just before and just after a window's end: the windows whose range ends above it are dead (no room), the others equal the reference"""
    blob, rec, total, max_rows = _arena_case()
    assert len(rec) == 8
    ends = sorted(set(int(w["out_off"]) + int(w["mlen"]) for w in rec))
    caps = sorted(set(c for e in ends for c in (e - 1, e, e + 1) if 0 <= c <= total + 1) | {0})
    dev = _Dev(blob, rec, total + 1, total + 1)
    model = _model(ctx, PAR7)
    seen = set()
    for cap in caps:
        dev.fresh()
        ref = WC.window_cns_ref(blob, rec, len(blob), cap, total + 1, max_rows, PAR7)
        _same(dev.run(ctx, model, len(blob), cap, total + 1, max_rows), ref, cap, total + 1, "out_cap %d" % cap)
        seen.add(int((ref.status == 0).sum()))
    assert {0, 8} <= seen and len(seen) >= 6                   # (nothing is live at out_cap 0: the window without columns lies at out_off 95)


def test_any_seq_cap(ctx):
    """the compact arena: all offsets are those of a large run, a window is copied whole if and only if its range ends inside seq_cap, nothing else is touched"""
    blob, rec, total, max_rows = _arena_case()
    full = WC.window_cns_ref(blob, rec, len(blob), total, total, max_rows, PAR7)
    need = int(full.seq_off[-1])
    ends = sorted(set(int(x) for x in full.seq_off[1:]))
    caps = sorted(set(c for e in ends for c in (e - 1, e, e + 1) if 0 <= c <= need + 1) | {0})
    dev = _Dev(blob, rec, total, need + 1)
    model = _model(ctx, PAR7)
    for cap, null in [(c, False) for c in caps] + [(0, True)]:
        dev.fresh()
        ref = WC.window_cns_ref(blob, rec, len(blob), total, cap, max_rows, PAR7)
        assert np.array_equal(ref.seq_off, full.seq_off)
        got = dev.run(ctx, model, len(blob), total, cap, max_rows, null_seq=null)
        _same(got, ref, total, cap, "seq_cap %d%s" % (cap, " (NULL arenas)" if null else ""))
        copied = sum(1 for g in range(len(rec)) if int(full.seq_off[g + 1]) <= cap and full.clen[g])
        assert (cap >= need) == (copied == int((full.clen > 0).sum()))
    # either quality array may be missing; without d_seq_off nothing is packed
    for skip in (14, 15):
        dev.fresh()
        args = dev.pointers(model, len(blob), total, need, max_rows)
        args[skip] = None
        import bsalign_amd as B
        assert B.lib().bsa_window_cns_run(ctx.h, *args) == 0
        ctx.sync()
        got = dev.read()
        assert np.array_equal(got.seq[:need], full.seq[:need]) and np.array_equal(got.seq_off, full.seq_off)
        assert np.all((got.seq_qlt if skip == 14 else got.seq_alt) == FILL)
        assert np.array_equal((got.seq_alt if skip == 14 else got.seq_qlt)[:need], (full.seq_alt if skip == 14 else full.seq_qlt)[:need])
    dev.fresh()
    got = dev.run(ctx, model, len(blob), total, 0, max_rows, pack=False)
    _same(got, full, total, 0, "no compaction", pack=False)
    assert np.all(got.seq == FILL) and np.all(got.seq_off == 0xA5A5A5A5A5A5A5A5)


def test_batch_with_a_short_compact_arena(ctx):
    import bsalign_amd as B
    blob, rec, total, max_rows = _arena_case()
    full = WC.window_cns_ref(blob, rec, len(blob), total, total, max_rows, PAR7)
    need = int(full.seq_off[-1])
    for cap, null in ((0, False), (0, True), (1, False), (need - 1, False)):
        rc, got = _host(ctx, PAR7, blob, rec, len(blob), total, cap, max_rows, seq_alloc=need, null_seq=null)
        assert rc == E_CIGAR_CAP and int(got.seq_off[-1]) == need and np.array_equal(got.seq_off, full.seq_off), cap
        assert np.all(got.seq == FILL) and np.all(got.seq_qlt == FILL) and np.array_equal(got.clen, full.clen), cap
        assert B.lib().bsa_last_error(ctx.h), cap
    rc, got = _host(ctx, PAR7, blob, rec, len(blob), total, need, max_rows)
    assert rc == 0
    _same(got, WC.window_cns_ref(blob, rec, len(blob), total, need, max_rows, PAR7), total, need, "batch, exact seq_cap")


# ---- 6. behind the real passes ---------------------------------------------------------------------------------------------------------------------
def _msa_resident(ctx, b, vote):
    """bsa_window_msa_run on a window_msa_cases.Batch -> (d_cols, cols_cap, d_cwin, the records the reference gives); nothing comes down"""
    import bsalign_amd as B
    roff, rcwin, _ = W.window_msa_ref(b, vote)
    cap = int(roff[-1])
    up = [_upload(x) for x in (b.piece, b.piece_off, b.bases, b.pcig, b.pcig_off, b.draft, b.doff, b.dlen)]
    d_cols, d_coff, d_cwin = _filled(cap), _filled(8 * (b.nwin + 1)), _filled(40 * b.nwin)
    ctx.window_msa_run(up[0], up[1], b.nwin, b.piece_cap, up[2], b.bases_cap, up[3], b.pcig_cap, up[4], up[5], up[6], up[7], b.window, 0, vote, d_cols, cap, d_coff, d_cwin)
    return d_cols, cap, d_cwin, rcwin


def _cns_resident(ctx, par, d_cols, cols_cap, d_cwin, nwin, max_rows, out_cap):
    """Context.window_cns_run behind it, no copy in between -> Got (the arrays as they come down)"""
    import torch
    d = {k: _filled(out_cap) for k in ("cns", "qlt", "alt", "seq", "seq_qlt", "seq_alt")}
    d_clen, d_score, d_status, d_soff = _filled(4 * nwin), _filled(8 * nwin), _filled(4 * nwin), _filled(8 * (nwin + 1))
    ctx.window_cns_run(_model(ctx, par), d_cols, cols_cap, d_cwin, nwin, max_rows, d["cns"], d["qlt"], d["alt"], out_cap, d_clen, d_score, d_status,
                       d["seq"], d["seq_qlt"], d["seq_alt"], out_cap, d_soff)
    ctx.sync()
    torch.cuda.synchronize()
    g = Got()
    for k, t in d.items():
        setattr(g, k, t.cpu().numpy()[:out_cap].copy())
    g.cols = d_cols.cpu().numpy()[:cols_cap].copy()
    g.clen, g.score = d_clen.cpu().numpy()[:4 * nwin].view(np.uint32).copy(), d_score.cpu().numpy()[:8 * nwin].view(np.float64).copy()
    g.status, g.seq_off = d_status.cpu().numpy()[:4 * nwin].view(np.uint32).copy(), d_soff.cpu().numpy()[:8 * (nwin + 1)].view(np.uint64).copy()
    g.rec = d_cwin.cpu().numpy()[:40 * nwin].view(CNS_WINDOW_DTYPE).copy()
    return g


def test_header_example_behind_the_msa_pass(ctx):
    WC.need_symbols()
    b, _ = W.header_example()
    d_cols, cap, d_cwin, rcwin = _msa_resident(ctx, b, 1)
    got = _cns_resident(ctx, PAR7, d_cols, cap, d_cwin, 1, 3, 12)
    cols, rec, cns, qlt, alt, called = WC.header_example_cns()
    assert cap == 72 and got.rec.tolist() == rec.tolist() and got.status.tolist() == [0] and got.clen.tolist() == [11] and got.seq_off.tolist() == [0, 11]
    assert np.array_equal(got.cns[:11], cns) and np.array_equal(got.qlt[:11], qlt) and np.array_equal(got.alt[:11], alt) and got.cns[11] == FILL
    assert np.array_equal(got.seq[:11], cns) and np.array_equal(got.seq_qlt[:11], qlt) and np.array_equal(got.seq_alt[:11], alt) and got.seq[11] == FILL
    assert np.array_equal(got.cols.reshape(12, 6)[:, 3:].T, called) and np.array_equal(got.cols.reshape(12, 6)[:, :3], cols.reshape(12, 6)[:, :3])


@pytest.mark.parametrize("vote", [0, 1])
def test_polished_draft_of_error_free_reads_is_the_truth(ctx, vote):
    """the closed loop: a truth of 2000 bases, an edited draft, four error-free reads, w = 100; bsa_window_msa_run, then bsa_window_cns_run on what it left:
    the compact sequence of the draft's windows, read from d_seq_off, is the truth (four reads outvote the draft where it votes too)"""
    WC.need_symbols()
    truth, draft, ws, b = W.closed_loop()
    d_cols, cap, d_cwin, rcwin = _msa_resident(ctx, b, vote)
    out_cap = int(rcwin["mlen"].sum())
    got = _cns_resident(ctx, PAR7, d_cols, cap, d_cwin, b.nwin, 4 + vote, out_cap)
    assert got.rec.tolist() == rcwin.tolist() and np.all(got.status == 0)
    ref = WC.window_cns_ref(got.cols, got.rec, cap, out_cap, out_cap, 4 + vote, PAR7)
    _same(got, ref, out_cap, out_cap, "closed loop, vote %d" % vote)
    first, last = int(got.seq_off[0]), int(got.seq_off[b.nwin])
    assert np.array_equal(got.seq[first:last], truth)


@pytest.mark.parametrize("vote", [0, 1])
def test_all_five_resident_passes_on_aligner_output(ctx, vote):
    """align_batch's records and words uploaded, then windows, pieces, guides, MSA and consensus on the device at w = 50, against the reference on the MSA
    that came down"""
    import torch
    import bsalign_amd as B
    WC.need_symbols()
    w = 50
    rng = np.random.default_rng(1811)
    draft = rng.integers(0, 4, 430).astype(np.uint8)
    pairs = [(S.mutate(rng, draft, 0.10), draft) for _ in range(6)]
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
    d_np = d_poff[8 * nwin:]
    ctx.piece_cigars_run(d_out, d_cig, d_coff, n, d_piece, d_np, piece_cap, d_pcig, pcig_cap, d_pcoff, None)
    ctx.window_msa_run(d_piece, d_poff, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcoff, d_seqs, d_doff, d_dlen, w, 0, vote, d_cols, cols_cap, d_cwoff, d_cwin)
    got = _cns_resident(ctx, PAR7, d_cols, cols_cap, d_cwin, nwin, n + vote, out_cap)
    need = int(d_cwoff.cpu().numpy()[:8 * (nwin + 1)].view(np.uint64)[nwin])
    assert 0 < need <= cols_cap and np.all(got.status == 0) and np.all(got.rec["nseq"] == n + vote) and int(got.rec["mlen"].sum()) > nwin * w - w
    ref = WC.window_cns_ref(got.cols, got.rec, cols_cap, out_cap, out_cap, n + vote, PAR7)
    _same(got, ref, out_cap, out_cap, "five passes, vote %d" % vote)
    polished = got.seq[:int(got.seq_off[nwin])]
    assert int((got.clen > 0).sum()) == nwin
    # the host-pointer calls give the same windows
    wins = ctx.cigar_windows(out, cigs, w)
    wp = ctx.window_pieces(pairs, wins, w, gbase, nwin)
    msas = ctx.window_msa(wp, ctx.piece_cigars(out, cigs, wp), [draft[int(o) - int(toff[0]):int(o) - int(toff[0]) + min(int(k), w)] for o, k in zip(doff, dlen)], w, vote=bool(vote))
    res, (seq, sq, sa, soff) = ctx.window_cns(msas, PAR7)
    assert np.array_equal(seq, polished) and np.array_equal(soff, got.seq_off) and np.array_equal(sq, got.seq_qlt[:len(seq)]) and np.array_equal(sa, got.seq_alt[:len(seq)])
    for g, (cns, qlt, alt, score, status, cols) in enumerate(res):
        a, k = int(got.rec[g]["out_off"]), int(got.clen[g])
        assert status == 0 and np.array_equal(cns, got.cns[a:a + k]) and np.array_equal(qlt, got.qlt[a:a + k]) and score == got.score[g], g
        c0 = int(got.rec[g]["cols_off"])
        assert np.array_equal(cols.reshape(-1), got.cols[c0:c0 + cols.size]), g


# ---- 7. re-run ---------------------------------------------------------------------------------------------------------------------------------------
def test_second_run_and_another_model(ctx):
    blob, rec, out_cap, max_rows, ref = _host_form("mlen_65")
    dev = _Dev(blob, rec, out_cap, out_cap)
    one = dev.run(ctx, _model(ctx, PAR7), len(blob), out_cap, out_cap, max_rows)
    _same(one, ref, out_cap, out_cap, "first run")
    two = dev.run(ctx, _model(ctx, PAR7), len(blob), out_cap, out_cap, max_rows)          # on columns that carry consensus bytes, into the same arrays
    for name in ("cols", "cns", "qlt", "alt", "seq", "seq_qlt", "seq_alt", "clen", "score", "status", "seq_off"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    other = WC.window_cns_ref(blob, rec, len(blob), out_cap, out_cap, max_rows, WC.PAR_OTHER)
    assert not np.array_equal(other.qlt, ref.qlt)
    dev.d_cns, dev.d_qlt, dev.d_alt = (_arena(out_cap) for _ in range(3))
    dev.d_seq, dev.d_sq, dev.d_sa = (_arena(out_cap) for _ in range(3))
    _same(dev.run(ctx, _model(ctx, WC.PAR_OTHER), len(blob), out_cap, out_cap, max_rows), other, out_cap, out_cap, "another model, on the columns of the first")
    dev.fresh()
    _same(dev.run(ctx, _model(ctx, PAR7), len(blob), out_cap, out_cap, max_rows), ref, out_cap, out_cap, "the first model again")


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import bsalign_amd as B
    blob, rec, total, max_rows = _arena_case()
    full = WC.window_cns_ref(blob, rec, len(blob), total, total, max_rows, PAR7)
    dev = _Dev(blob, rec, total, total)
    model = _model(ctx, PAR7)
    run, batch, err = B.lib().bsa_window_cns_run, B.lib().bsa_window_cns_batch, B.lib().bsa_last_error
    rargs = [ctx.h] + dev.pointers(model, len(blob), total, total, max_rows)
    h = Got()
    h.cols, par = blob.copy(), np.ascontiguousarray(PAR7)
    h.cns, h.qlt, h.alt, h.seq, h.sq, h.sa = (np.full(total, FILL, np.uint8) for _ in range(6))
    h.clen, h.score, h.status, h.soff = np.zeros(8, np.uint32), np.zeros(8, np.float64), np.zeros(8, np.uint32), np.zeros(9, np.uint64)
    bargs = [ctx.h, B._p(par), B._p(h.cols), len(blob), B._p(rec), 8, max_rows, B._p(h.cns), B._p(h.qlt), B._p(h.alt), total, B._p(h.clen), B._p(h.score), B._p(h.status),
             B._p(h.seq), B._p(h.sq), B._p(h.sa), total, B._p(h.soff)]

    def refused(fn, base, changes, code=E_ARG):
        a = list(base)
        for i, v in changes.items():
            a[i] = v
        assert fn(*a) == code, (fn.__name__, changes)
        if 0 not in changes:
            assert err(ctx.h), (fn.__name__, changes)
    for fn, base in ((run, rargs), (batch, bargs)):
        # no context, model / parameters, columns (with a cap), records, cns, qlt, alt, clen, compact sequence (with a cap)
        for i in (0, 1, 2, 4, 7, 8, 9, 11, 14):
            refused(fn, base, {i: None})
        refused(fn, base, {18: None})                          # compact arrays and a cap without seq_off
        refused(fn, base, {18: None, 14: None, 15: None, 16: None})                # seq_cap alone
        refused(fn, base, {18: None, 14: None, 16: None, 17: 0})                   # a quality array alone
        refused(fn, base, {5: 0xFFFFFFF1})                     # nwin
        refused(fn, base, {6: 20000}, E_UNSUPPORTED)           # max_rows: 16 bytes of LDS a row
    other = B.Context(0)
    try:
        refused(run, rargs, {1: other.cns_model(PAR7).h})      # a model of another context
    finally:
        other.close()
    # nothing was launched by the refused calls; the good calls still run
    assert np.all(h.cns == FILL) and np.all(h.seq == FILL)
    assert run(*rargs) == 0
    ctx.sync()
    _same(dev.read(), full, total, total, "after the refused calls")
    assert batch(*bargs) == 0 and np.array_equal(h.cns, full.cns) and np.array_equal(h.seq, full.seq) and np.array_equal(h.soff, full.seq_off) and np.array_equal(h.cols, full.cols)
    # no windows: seq_off[0] = 0 and nothing else; NULL is fine where there is no work
    dev.fresh()
    a = [ctx.h] + dev.pointers(model, len(blob), total, total, max_rows)
    a[5] = 0
    assert run(*a) == 0
    ctx.sync()
    got = dev.read()
    assert int(got.seq_off[0]) == 0 and int(got.seq_off[1]) == 0xA5A5A5A5A5A5A5A5 and np.all(got.cns == FILL) and np.all(got.seq == FILL) and np.all(got.clen == 0xA5A5A5A5)
    assert np.array_equal(got.cols, blob)
    off1 = np.full(1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert batch(ctx.h, B._p(par), None, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None, 0, B._p(off1)) == 0 and off1.tolist() == [0]
    assert run(ctx.h, model.h, None, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    # the Python plumbing's size checks
    import torch
    t = lambda nbytes: torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    good = dict(d_cols=t(len(blob)), d_cwin=t(320), d_cns=t(total), d_qlt=t(total), d_alt=t(total), d_clen=t(32), d_score=t(64), d_status=t(32), d_seq=t(total), d_seq_off=t(72))
    call = lambda **kw: ctx.window_cns_run(model, kw["d_cols"], len(blob), kw["d_cwin"], 8, max_rows, kw["d_cns"], kw["d_qlt"], kw["d_alt"], total, kw["d_clen"], kw["d_score"],
                                           kw["d_status"], kw["d_seq"], None, None, total, kw["d_seq_off"])
    for k in good:
        with pytest.raises(ValueError):
            call(**dict(good, **{k: good[k][:-1]}))
    with pytest.raises(ValueError):
        ctx.cns_model(PAR7[:6])
