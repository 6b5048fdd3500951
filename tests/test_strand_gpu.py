"""BSA_MODE_QSTRAND on the MI355X.  The yardstick is the UNFLAGGED call on a blob in which the host stored the reverse complement of
every marked query: the flagged call on the blob that holds every query forward must return the same status, records, CIGAR offsets and
CIGAR words, bit for bit, through the same forward kernel -- on every forward kernel of the 8-bit aligner, the edit aligner in all
modes, both forms (a wave per pair, a block per pair) of all four staging kernels, 1 B/base and 2-bit packed blobs, host pointers and
device-pointer plans.  A sample of every case is also checked against the oracle on revcomp(q); no sampled pair is skipped (the seeds
were chosen so that the oracle finishes every one of them) and no pair is left out of the flagged-against-unflagged comparison.

Packed blobs: pair k's query starts at position k % 32 of a word -- the first one at base 0 of word 0, nothing in front of it -- and the
last pair's query is the last thing in the blob, so its last base lies in the last word."""
import ctypes as C

import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.gpu

MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)
SC = (2, -6, -3, -2, 0, 0)
LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 1000, 2000]


def _pairs(seed, n, lens=LENS, qmax=None):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(n):
        L = int(lens[k % len(lens)])
        t = rng.integers(0, 4, size=L).astype(np.uint8)
        q = S.mutate(rng, t, 0.1)
        if not len(q):
            q = t[:1].copy()
        if qmax is not None:
            q = q[:qmax]
        pairs.append((q, t))
    return pairs


def _strands(seed, n, kind="mixed"):
    """mixed: at random, the first and the last pair marked (the packed blob's first query has nothing in front of it, its last one
    nothing behind it)"""
    if kind == "forward":
        return np.zeros(n, bool)
    if kind == "reverse":
        return np.ones(n, bool)
    s = np.random.default_rng(seed + 99991).random(n) < 0.5
    s[0] = s[-1] = True
    return s


def _stored(pairs, strands):
    """what the aligner sees for every pair: the host-made reverse complement of the marked queries"""
    import bsalign_amd as B
    return [(B.revcomp(q) if s else q, t) for (q, t), s in zip(pairs, strands)]


def _blob(pairs, seq2bit):
    """1 B/base: pack_pairs' blob (the first query at byte 0).  Packed: see the module docstring; base offsets"""
    import bsalign_amd as B
    if not seq2bit:
        return B.pack_pairs(pairs)
    parts, acc, qoff, toff = [], 0, [0] * len(pairs), [0] * len(pairs)

    def place(seq, r):
        nonlocal acc
        pad = (r - acc) % 32
        parts.append(np.zeros(pad, np.uint8))
        acc += pad
        off = acc
        parts.append(np.ascontiguousarray(seq, dtype=np.uint8))
        acc += len(seq)
        return off
    for k, (q, t) in enumerate(pairs):
        if k + 1 < len(pairs):
            qoff[k] = place(q, k % 32)
            toff[k] = place(t, (7 * k + 5) % 32)
        else:
            toff[k] = place(t, (7 * k + 5) % 32)
            qoff[k] = place(q, k % 32)
    words = B.pack2bit(np.concatenate(parts))
    assert qoff[0] == 0 and (acc - 1) // 32 == words.size - 1
    return (words, np.array(qoff, np.uint64), np.array([len(q) for q, _ in pairs], np.uint32),
            np.array(toff, np.uint64), np.array([len(t) for _, t in pairs], np.uint32))


def _raw(ctx, fn, blob, par, extra_mode, score_only=False):
    """one host-pointer call -> (rc, results, CIGAR list, offsets, status)"""
    seqs, qoff, qlen, toff, tlen = blob
    p = type(par).from_buffer_copy(par)
    p.mode = par.mode | extra_mode
    n = len(qlen)
    out = np.zeros(n, dtype=_B().RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    cig = np.zeros(cap, dtype=np.uint32)
    off = np.full(n + 1, 7, dtype=np.uint64)
    rc = fn(ctx.h, seqs.ctypes.data, seqs.nbytes, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data, n, C.byref(p),
            out.ctypes.data, None if score_only else cig.ctypes.data, 0 if score_only else cap, off.ctypes.data, st.ctypes.data)
    return rc, out, [cig[int(off[k]):int(off[k + 1])].copy() for k in range(n)], off, st


def _B():
    import bsalign_amd as B
    return B


def _mark(blob, strands):
    seqs, qoff, qlen, toff, tlen = blob
    return seqs, qoff | np.where(strands, np.uint64(_B().QOFF_REVCOMP), np.uint64(0)).astype(np.uint64), qlen, toff, tlen


def _sc(par):
    return (int(par.matrix[0]), int(par.matrix[1]), int(par.gapo1), int(par.gape1), int(par.gapo2), int(par.gape2))


def oracle_sample(pairs, strands, par, edit=False, count=4):
    """`count` pairs spread over the batch through the oracle, on the reverse complement where marked: [(k, q', t, record, words)].
    Every one of them must come through (n >= 0): nothing is skipped."""
    B = _B()
    mode, bw = par.mode & 3, par.bandwidth
    res = []
    for k in (np.linspace(0, len(pairs) - 1, min(count, len(pairs))).astype(int) if count else []):
        q, t = pairs[k]
        qq = B.revcomp(q) if strands[k] else q
        r, cig, n = S.oracle_edit(qq, t, mode, bw) if edit else S.oracle_align(qq, t, mode, bw, *_sc(par))
        assert n >= 0, ("the oracle does not finish sampled pair %d: choose another seed" % k)
        res.append((int(k), qq, t, r, cig))
    return res


def _same(ctx, pairs, strands, par, edit=False, score_only=False, seq2bit=False, eqx=False, oracle=4):
    """(1) the unflagged call on a blob that holds revcomp(q) for the marked pairs, (2) the flagged call on a blob that holds every
    query forward: equal status, records, offsets and words pair by pair, the same forward kernel; a sample against the oracle.
    Returns the forward kernel's name and the flagged call's CIGAR lists."""
    B = _B()
    fn = B.lib().bsa_edit_batch if edit else B.lib().bsa_align_batch
    strands = np.asarray(strands, bool)
    extra = (B.MODE_SEQ2BIT if seq2bit else 0) | (B.MODE_SCORE_ONLY if score_only else 0) | (B.MODE_CIGAR_EQX if eqx else 0)
    rc, uo, uc, uoff, ust = _raw(ctx, fn, _blob(_stored(pairs, strands), seq2bit), par, extra, score_only)
    ctx._chk(rc)
    ufwd = ctx.last_kernel_names()[0]
    rc, fo, fc, foff, fst = _raw(ctx, fn, _mark(_blob(pairs, seq2bit), strands), par, extra | B.MODE_QSTRAND, score_only)
    ctx._chk(rc)
    ffwd = ctx.last_kernel_names()[0]
    assert ffwd == ufwd, (ffwd, ufwd)
    assert np.array_equal(fst, ust), [(int(k), int(fst[k]), int(ust[k])) for k in np.nonzero(fst != ust)[0][:10]]
    assert np.array_equal(fo.view(np.int32), uo.view(np.int32)), [(int(k), bool(strands[k]), fo[k], uo[k]) for k in np.nonzero(fo != uo)[0][:5]]
    assert np.array_equal(foff, uoff)
    for k in range(len(pairs)):
        assert np.array_equal(fc[k], uc[k]), (k, bool(strands[k]))
    for k, qq, t, res, cig in oracle_sample(pairs, strands, par, edit, oracle):
        got = np.array([fo[k][f] for f in fo.dtype.names], dtype=np.int32)
        if score_only:
            assert (got[0], got[2], got[4]) == (res[0], res[2], res[4]), (k, got, res)
        elif eqx:
            assert fst[k] == 0 and np.array_equal(got, res) and np.array_equal(fc[k], B.expand_eqx(cig, qq, t, res[1], res[3])), (k, got, res)
        else:
            assert fst[k] == 0 and np.array_equal(got, res) and np.array_equal(fc[k], cig), (k, got, res)
    return ffwd, fc


def _par(mode, bw, sc=SC):
    return _B().make_params(mode, bw, *sc)


def _epar(mode, bw):
    p = _B().EditParams()
    p.mode, p.bandwidth = mode, bw
    return p


FORMATS = [False, True]           # 1 B/base, BSA_MODE_SEQ2BIT


# the cases as data (pairs, strands, parameters, keywords of _same, a piece of the forward kernel's name), so that the oracle sample of
# every one of them can be checked on a CPU
def cases_register(bw):
    pairs = _pairs(100 + bw, 40)
    return [(pairs, _strands(bw + m, 40), _par(m, bw), {}, "k_align8_fwd_x") for m in MODES]


def cases_two_piece_rowrecords_wide():
    B = _B()
    pairs = _pairs(200, 40)
    st = _strands(200, 40)
    return [(pairs, st, _par(S.MODE_GLOBAL, 128, (2, -6, -3, -2, -8, -1)), {}, "k_align8_fwd_x2"),
            (pairs, st, _par(S.MODE_GLOBAL | B.MODE_ROWRECORDS, 128), {}, "row records"),
            (pairs, st, _par(S.MODE_OVERLAP, 512), {}, "row records")]


def cases_whole_query():
    short = _pairs(300, 40, qmax=256)
    longq = [(q, t) for q, t in _pairs(301, 26, lens=[257, 300, 700, 1000, 2000]) if len(q) > 256]
    out = [(short, _strands(300 + m, len(short)), _par(m, 0), {}, "k_align8_fwd_x") for m in MODES]
    out += [(longq, _strands(310 + m, len(longq)), _par(m, 0), {}, "k_align8_fwd_sys (") for m in MODES]
    mixed = short[:20] + longq[:10]           # a mixed batch at bandwidth 0: one sub-batch per width class
    out.append((mixed, _strands(320, len(mixed)), _par(S.MODE_OVERLAP, 0), {}, ""))
    return out


def cases_run_time_width():
    pairs = [(q, t) for q, t in _pairs(448, 30, lens=[100, 300, 1000]) if len(q) > 48]
    return [(pairs, _strands(448 + m, len(pairs)), _par(m, 48), {}, "k_align8_fwd_gen") for m in MODES]


def cases_score_only():
    pairs = _pairs(500, 40)
    return [(pairs, _strands(500 + m, 40), _par(m, 128), {"score_only": True}, "score-only") for m in MODES]


def cases_edit(bw):
    pairs = _pairs(700 + bw, 36)
    out = []
    for m in MODES:
        out.append((pairs, _strands(700 + bw + m, 36), _epar(m, bw), {"edit": True}, ""))
        out.append((pairs, _strands(710 + bw + m, 36), _epar(m, bw), {"edit": True, "score_only": True}, ""))
    return out


def cases_strand_patterns():
    pairs = _pairs(1100, 39)
    out = []
    for kind in ("mixed", "forward", "reverse"):
        out.append((pairs, _strands(1100, 39, kind), _par(S.MODE_GLOBAL, 128), {}, "k_align8_fwd_x"))
        out.append((pairs, _strands(1100, 39, kind), _epar(S.MODE_OVERLAP, 64), {"edit": True}, ""))
    return out


def cases_block_per_pair():
    # >= 8192 staged bytes a pair: a block per pair in k_stage / k_stage2b; everything else in this file: a wave per pair
    long = _pairs(600, 6, lens=[5000, 6001, 7003])
    assert min(len(t) for _, t in long) >= 5000
    return [(long, np.array([True, False, True, True, False, True]), _par(S.MODE_GLOBAL, 128), {"oracle": 2}, "k_align8_fwd_x"),
            (long, np.array([True, True, False, True, False, True]), _epar(S.MODE_GLOBAL, 256), {"edit": True, "oracle": 2}, "")]


def cases_eqx():
    pairs = _pairs(1200, 40)
    st = _strands(1200, 40)
    return [(pairs, st, _par(S.MODE_GLOBAL, 128), {"eqx": True}, "k_align8_fwd_x"),
            (pairs, st, _epar(S.MODE_GLOBAL, 256), {"edit": True, "eqx": True}, "")]


CASES = {
    "register64": lambda: cases_register(64), "register128": lambda: cases_register(128), "register256": lambda: cases_register(256),
    "two_piece_rowrecords_wide": cases_two_piece_rowrecords_wide, "whole_query": cases_whole_query, "run_time_width": cases_run_time_width,
    "score_only": cases_score_only, "edit0": lambda: cases_edit(0), "edit64": lambda: cases_edit(64), "edit256": lambda: cases_edit(256),
    "strand_patterns": cases_strand_patterns, "block_per_pair": cases_block_per_pair, "eqx": cases_eqx,
}


@pytest.mark.parametrize("seq2bit", FORMATS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_flagged_equals_unflagged_on_the_reverse_complement(ctx, name, seq2bit):
    B = _B()
    for pairs, strands, par, kw, fwd in CASES[name]():
        got, cigs = _same(ctx, pairs, strands, par, seq2bit=seq2bit, **kw)
        assert fwd in got, (fwd, got)
        if kw.get("eqx"):
            # ... and merging the = / X runs gives the plain words of the flagged call
            edit = kw.get("edit", False)
            fn = B.lib().bsa_edit_batch if edit else B.lib().bsa_align_batch
            rc, _, plain, _, _ = _raw(ctx, fn, _mark(_blob(pairs, seq2bit), strands), par, B.MODE_QSTRAND | (B.MODE_SEQ2BIT if seq2bit else 0))
            ctx._chk(rc)
            assert any(len(c) for c in cigs)
            for k in range(len(pairs)):
                assert np.array_equal(B.collapse_eqx(cigs[k]), plain[k]), k


@pytest.mark.parametrize("seq2bit", FORMATS)
def test_checked_whole_query_kernel_handover_and_slices_keep_the_strand(ctx, monkeypatch, seq2bit):
    longq = [(q, t) for q, t in _pairs(301, 26, lens=[257, 300, 700, 1000, 2000]) if len(q) > 256]
    monkeypatch.setenv("BSA_ALIGN8_SYS_CHK", "1")
    fwd, _ = _same(ctx, longq, _strands(330, len(longq)), _par(S.MODE_GLOBAL, 0, (10, -30, -20, -10, 0, 0)), seq2bit=seq2bit)
    assert "k_align8_fwd_sys<CHK>" in fwd
    monkeypatch.delenv("BSA_ALIGN8_SYS_CHK")
    pairs = _pairs(500, 40)
    monkeypatch.setenv("BSA_DEBUG_HANDOVER", "7")
    _same(ctx, pairs, _strands(540, 40), _par(S.MODE_GLOBAL, 128), seq2bit=seq2bit)
    assert ctx.last_handover() > 0
    monkeypatch.delenv("BSA_DEBUG_HANDOVER")
    monkeypatch.setenv("BSA_BATCH_SLICES", "2")
    _same(ctx, pairs, _strands(541, 40), _par(S.MODE_GLOBAL, 128), seq2bit=seq2bit)
    _same(ctx, pairs, _strands(542, 40), _par(S.MODE_EXTEND, 64), score_only=True, seq2bit=seq2bit)


def many_short_pairs():
    rng = np.random.default_rng(800)
    n = 65536 + 37
    lens = rng.integers(1, 70, size=n)
    pairs = []
    for L in lens:
        t = rng.integers(0, 4, size=int(L)).astype(np.uint8)
        q = t.copy()
        hit = rng.random(int(L)) < 0.1
        q[hit] = (q[hit] + 1 + rng.integers(0, 3, size=int(hit.sum()))) & 3
        if L > 4 and rng.random() < 0.5:
            q = np.delete(q, int(rng.integers(0, L)))
        pairs.append((q, t))
    return pairs, _strands(800, n), _epar(S.MODE_GLOBAL, 64)


@pytest.mark.parametrize("seq2bit", FORMATS)
def test_edit_many_short_pairs(ctx, seq2bit):
    """65 536 pairs or more: the wave-per-pair form of the edit staging kernels"""
    pairs, strands, par = many_short_pairs()
    _same(ctx, pairs, strands, par, edit=True, seq2bit=seq2bit, oracle=16)


def test_python_entry_points(ctx):
    B = _B()
    pairs = _pairs(601, 33)
    st = _strands(601, 33)
    rcp = _stored(pairs, st)
    for seq2bit in FORMATS:
        a, ac, ast = ctx.align_batch(rcp, _par(S.MODE_GLOBAL, 128))
        b, bc, bst = ctx.align_batch(pairs, _par(S.MODE_GLOBAL, 128), seq2bit=seq2bit, strands=st)
        assert np.array_equal(a, b) and np.array_equal(ast, bst) and all(np.array_equal(x, y) for x, y in zip(ac, bc))
        a, ast = ctx.align_scores(rcp, _par(S.MODE_OVERLAP, 64))
        b, bst = ctx.align_scores(pairs, _par(S.MODE_OVERLAP, 64), seq2bit=seq2bit, strands=st)
        assert np.array_equal(a, b) and np.array_equal(ast, bst)
        a, ac, ast = ctx.edit_batch(rcp, S.MODE_EXTEND, 64)
        b, bc, bst = ctx.edit_batch(pairs, S.MODE_EXTEND, 64, seq2bit=seq2bit, strands=st)
        assert np.array_equal(a, b) and np.array_equal(ast, bst) and all(np.array_equal(x, y) for x, y in zip(ac, bc))
        a, ast = ctx.edit_scores(rcp, S.MODE_GLOBAL, 0)
        b, bst = ctx.edit_scores(pairs, S.MODE_GLOBAL, 0, seq2bit=seq2bit, strands=st)
        assert np.array_equal(a, b) and np.array_equal(ast, bst)
    assert st.any() and not st.all()


@pytest.mark.parametrize("seq2bit", FORMATS)
def test_plans_on_device_pointers(ctx, seq2bit):
    import torch
    B = _B()
    pairs = _pairs(900, 40)
    st = _strands(900, 40)
    n = len(pairs)
    seqs, qoff, qlen, toff, tlen = _mark(_blob(pairs, seq2bit), st)
    d_seqs = torch.from_numpy(seqs.view(np.int64) if seq2bit else seqs).cuda()
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    fl = B.MODE_QSTRAND | (B.MODE_SEQ2BIT if seq2bit else 0)
    for edit in (False, True):
        if edit:
            plan = B.EditPlan(ctx, qoff, qlen, toff, tlen, S.MODE_GLOBAL | fl, 128)
            ref, rc, rst = ctx.edit_batch(_stored(pairs, st), S.MODE_GLOBAL, 128)
        else:
            plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, _par(S.MODE_GLOBAL | fl, 128))
            ref, rc, rst = ctx.align_batch(_stored(pairs, st), _par(S.MODE_GLOBAL, 128))
        d_out = torch.zeros(n * 10, dtype=torch.int32, device="cuda")
        d_cig = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run(d_seqs, d_out, d_cig, d_off, d_st)
        ctx.sync()
        out = d_out.cpu().numpy().reshape(n, 10)
        off = d_off.cpu().numpy()
        cig = d_cig.cpu().numpy().view(np.uint32)
        assert np.array_equal(d_st.cpu().numpy().view(np.uint32), rst)
        assert np.array_equal(out, ref.view(np.int32).reshape(n, 10)), np.nonzero((out != ref.view(np.int32).reshape(n, 10)).any(axis=1))[0][:10]
        for k in range(n):
            assert np.array_equal(cig[int(off[k]):int(off[k + 1])], rc[k]), k
        plan.close()


def test_bad_base_in_a_marked_query(ctx):
    """a code of 4 in a stored 1 B/base query: BSA_ST_BAD_BASE exactly where the unflagged call on the stored query sets it -- in the
    pieces loaded eight bytes at a time and in the ragged piece, which for a marked query holds the START of the stored query"""
    B = _B()
    pairs = _pairs(1300, 26)
    rng = np.random.default_rng(1300)
    dirty = []
    for k, (q, t) in enumerate(pairs):
        if k % 3 == 0:
            continue
        q = q.copy()
        q[[0, len(q) - 1, int(rng.integers(0, len(q)))][(k // 3) % 3]] = 4
        pairs[k] = (q, t)
        dirty.append(k)
    st = np.ones(len(pairs), bool)
    st[1::4] = False
    for fn, par in ((B.lib().bsa_align_batch, _par(S.MODE_GLOBAL, 128)), (B.lib().bsa_edit_batch, _epar(S.MODE_GLOBAL, 64))):
        rc, _, _, _, ust = _raw(ctx, fn, _blob(pairs, False), par, 0)
        ctx._chk(rc)
        rc, _, _, _, fst = _raw(ctx, fn, _mark(_blob(pairs, False), st), par, B.MODE_QSTRAND)
        ctx._chk(rc)
        assert np.array_equal(fst & B.ST_BAD_BASE, ust & B.ST_BAD_BASE)
        assert sorted(np.nonzero(fst & B.ST_BAD_BASE)[0].tolist()) == dirty


def test_argument_errors_and_empty_queries(ctx):
    B = _B()
    pairs = _pairs(1000, 5)
    n = len(pairs)
    bit = np.uint64(B.QOFF_REVCOMP)
    for seq2bit in FORMATS:
        blob = _blob(pairs, seq2bit)
        seqs, qoff, qlen, toff, tlen = blob
        lim = 4 * seqs.nbytes if seq2bit else seqs.nbytes
        fl = B.MODE_SEQ2BIT if seq2bit else 0
        for fn, par in ((B.lib().bsa_align_batch, _par(S.MODE_GLOBAL, 128)), (B.lib().bsa_edit_batch, _epar(S.MODE_GLOBAL, 128))):
            marked = qoff.copy()
            marked[2] |= bit
            assert _raw(ctx, fn, (seqs, marked, qlen, toff, tlen), par, fl | B.MODE_QSTRAND)[0] == 0
            # bit 63 without the flag: part of the offset, outside every blob -- as before
            assert _raw(ctx, fn, (seqs, marked, qlen, toff, tlen), par, fl)[0] == -2
            # a marked offset whose masked value lies outside the blob
            past = qoff.copy()
            past[2] = np.uint64(lim - int(qlen[2]) + 1) | bit
            assert _raw(ctx, fn, (seqs, past, qlen, toff, tlen), par, fl | B.MODE_QSTRAND)[0] == -2
            past[2] = np.uint64(lim + 1) | bit
            assert _raw(ctx, fn, (seqs, past, qlen, toff, tlen), par, fl | B.MODE_QSTRAND)[0] == -2
            # a marked query of length 0: BSA_ST_EMPTY, the other pairs as without it
            zl = qlen.copy()
            zl[2] = 0
            rc, out, cig, off, st = _raw(ctx, fn, (seqs, marked, zl, toff, tlen), par, fl | B.MODE_QSTRAND)
            assert rc == 0 and st[2] == B.ST_EMPTY and len(cig[2]) == 0
            rc, uout, _, _, ust = _raw(ctx, fn, (seqs, qoff, zl, toff, tlen), par, fl)
            assert rc == 0 and np.array_equal(st, ust) and np.array_equal(out, uout)


def test_a_resident_batch_at_size(ctx):
    """4096 x 10 kbp from bsa_synth_pairs_dev: every second query reverse-complemented in place on the device and marked -- records,
    offsets, words and status are those of the unmarked run on the untouched buffer; 1 B/base and packed"""
    import torch
    B = _B()
    n, L = 4096, 10000
    lib = B.lib()
    stride = lib.bsa_synth_stride(L)
    nb = 2 * n * stride
    d_seqs = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    d_qlen = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, S.SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    ctx.sync()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)

    def run(mode, d, qo):
        plan = B.AlignPlan(ctx, qo, qlen, toff, tlen, _par(mode, 128))
        d_out = torch.zeros(n * 10, dtype=torch.int32, device="cuda")
        d_cig = torch.zeros(n * (L // 4), dtype=torch.int32, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run(d, d_out, d_cig, d_off, d_st)
        ctx.sync()
        off = d_off.cpu().numpy()
        res = (d_out.cpu().numpy(), off, d_cig.cpu().numpy()[:int(off[-1])], d_st.cpu().numpy())
        plan.close()
        return res
    ref = run(S.MODE_GLOBAL, d_seqs, qoff)
    assert not ref[3].any() and int(ref[1][-1]) > n
    marked = qoff.copy()
    for k in range(0, n, 2):
        a, b = int(qoff[k]), int(qoff[k]) + int(qlen[k])
        d_seqs[a:b] = 3 - d_seqs[a:b].flip(0)
        marked[k] |= np.uint64(B.QOFF_REVCOMP)
    torch.cuda.synchronize()
    got = run(S.MODE_GLOBAL | B.MODE_QSTRAND, d_seqs, marked)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    d_bits = torch.zeros((nb + 31) // 32, dtype=torch.int64, device="cuda")
    ctx.seq_pack2bit(d_seqs, d_bits)
    ctx.sync()
    got = run(S.MODE_GLOBAL | B.MODE_QSTRAND | B.MODE_SEQ2BIT, d_bits, marked)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
