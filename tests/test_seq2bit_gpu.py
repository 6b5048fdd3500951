"""BSA_MODE_SEQ2BIT on the MI355X: every call on a 2-bit packed blob returns what the same call on the unpacked bytes returns --
results, CIGAR words, offsets and status, bit for bit -- on every forward kernel of the 8-bit aligner (each case asserts which one ran),
the edit aligner in all modes, both forms of both staging kernels, the device-pointer plans and the device packer.  Pairs start at
every position in a word; the last pair ends in the blob's last word.  A sample of each case is checked against the oracle."""
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


def _blob(pairs):
    """2-bit words with pair k's query starting at position k % 32 of a word and its target at (7 k + 5) % 32, nothing behind the last
    target (so its last base lies in the last word); base offsets"""
    import bsalign_amd as B
    parts, acc, qoff, toff = [], 0, [], []

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
        qoff.append(place(q, k % 32))
        toff.append(place(t, (7 * k + 5) % 32))
    words = B.pack2bit(np.concatenate(parts))
    assert (acc - 1) // 32 == words.size - 1
    return (words, np.array(qoff, np.uint64), np.array([len(q) for q, _ in pairs], np.uint32),
            np.array(toff, np.uint64), np.array([len(t) for _, t in pairs], np.uint32))


def _packed(ctx, fn, pairs, par, score_only=False):
    """the host-pointer call on _blob's words with BSA_MODE_SEQ2BIT: (results, CIGAR list, offsets, status)"""
    import bsalign_amd as B
    words, qoff, qlen, toff, tlen = _blob(pairs)
    p = type(par).from_buffer_copy(par)
    p.mode = par.mode | B.MODE_SEQ2BIT | (B.MODE_SCORE_ONLY if score_only else 0)
    n = len(pairs)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    cig = np.zeros(cap, dtype=np.uint32)
    off = np.full(n + 1, 7, dtype=np.uint64)
    rc = fn(ctx.h, words.ctypes.data, words.nbytes, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data, n, C.byref(p),
            out.ctypes.data, None if score_only else cig.ctypes.data, 0 if score_only else cap, off.ctypes.data, st.ctypes.data)
    ctx._chk(rc)
    return out, [cig[int(off[k]):int(off[k + 1])].copy() for k in range(n)], off, st


def _unpacked(ctx, fn, pairs, par, score_only=False):
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    p = type(par).from_buffer_copy(par)
    p.mode = par.mode | (B.MODE_SCORE_ONLY if score_only else 0)
    n = len(pairs)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    cig = np.zeros(cap, dtype=np.uint32)
    off = np.full(n + 1, 7, dtype=np.uint64)
    ctx._chk(fn(ctx.h, seqs.ctypes.data, seqs.nbytes, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data, n, C.byref(p),
                out.ctypes.data, None if score_only else cig.ctypes.data, 0 if score_only else cap, off.ctypes.data, st.ctypes.data))
    return out, [cig[int(off[k]):int(off[k + 1])].copy() for k in range(n)], off, st


def _same(ctx, pairs, par, edit=False, score_only=False, oracle=4):
    """packed == unpacked, field by field; the same forward kernel ran; `oracle` pairs (spread over the batch) against the oracle.
    Returns the forward kernel's name."""
    import bsalign_amd as B
    fn = B.lib().bsa_edit_batch if edit else B.lib().bsa_align_batch
    uo, uc, uoff, ust = _unpacked(ctx, fn, pairs, par, score_only)
    ufwd = ctx.last_kernel_names()[0]
    po, pc, poff, pst = _packed(ctx, fn, pairs, par, score_only)
    pfwd = ctx.last_kernel_names()[0]
    assert pfwd == ufwd, (pfwd, ufwd)
    assert np.array_equal(pst, ust), np.nonzero(pst != ust)[0][:10]
    assert np.array_equal(po.view(np.int32), uo.view(np.int32)), [(k, po[k], uo[k]) for k in np.nonzero(po != uo)[0][:5]]
    assert np.array_equal(poff, uoff)
    for k in range(len(pairs)):
        assert np.array_equal(pc[k], uc[k]), k
    mode, bw = par.mode & 3, par.bandwidth
    for k in np.linspace(0, len(pairs) - 1, min(oracle, len(pairs))).astype(int):
        q, t = pairs[k]
        res, cig, n = S.oracle_edit(q, t, mode, bw) if edit else S.oracle_align(q, t, mode, bw, *(SC if not hasattr(par, "matrix") else _sc(par)))
        if n < 0:
            continue
        got = np.array([po[k][f] for f in po.dtype.names], dtype=np.int32)
        if score_only:
            assert (got[0], got[2], got[4]) == (res[0], res[2], res[4]), (k, got, res)
        else:
            assert pst[k] == 0 and np.array_equal(got, res) and np.array_equal(pc[k], cig), (k, got, res)
    return pfwd


def _sc(par):
    return (int(par.matrix[0]), int(par.matrix[1]), int(par.gapo1), int(par.gape1), int(par.gapo2), int(par.gape2))


def _par(mode, bw, sc=SC):
    import bsalign_amd as B
    return B.make_params(mode, bw, *sc)


@pytest.mark.parametrize("bw", [64, 128, 256])
def test_align8_register_kernels_all_modes(ctx, bw):
    pairs = _pairs(100 + bw, 40)
    for mode in MODES:
        fwd = _same(ctx, pairs, _par(mode, bw))
        assert fwd.startswith("k_align8_fwd_x"), fwd


def test_align8_row_segments_two_piece_and_row_records(ctx, monkeypatch):
    import bsalign_amd as B
    pairs = _pairs(200, 40)
    assert "k_align8_fwd_x2" in _same(ctx, pairs, _par(S.MODE_GLOBAL, 128, (2, -6, -3, -2, -8, -1)))
    assert "row records" in _same(ctx, pairs, _par(S.MODE_GLOBAL | B.MODE_ROWRECORDS, 128))
    assert "row records" in _same(ctx, pairs, _par(S.MODE_OVERLAP, 512))
    monkeypatch.setenv("BSA_ALIGN8_I32", "1")
    monkeypatch.setenv("BSA_ALIGN8_LITERAL", "1")
    assert "row records" in _same(ctx, pairs, _par(S.MODE_GLOBAL, 512))
    monkeypatch.delenv("BSA_ALIGN8_I32")
    monkeypatch.delenv("BSA_ALIGN8_LITERAL")
    monkeypatch.setenv("BSA_ALIGN8_XQ", "1")
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    assert "k_align8_fwd_xq" in _same(ctx, pairs, _par(S.MODE_GLOBAL, 128))


def test_align8_whole_query_bands(ctx, monkeypatch):
    short = _pairs(300, 40, qmax=256)
    for mode in MODES:
        assert _same(ctx, short, _par(mode, 0)).startswith("k_align8_fwd_x")
    longq = [(q, t) for q, t in _pairs(301, 26, lens=[257, 300, 700, 1000, 2000]) if len(q) > 256]
    for mode in MODES:
        assert "k_align8_fwd_sys (" in _same(ctx, longq, _par(mode, 0))
    monkeypatch.setenv("BSA_ALIGN8_SYS_CHK", "1")
    assert "k_align8_fwd_sys<CHK>" in _same(ctx, longq, _par(S.MODE_GLOBAL, 0, (10, -30, -20, -10, 0, 0)))
    monkeypatch.delenv("BSA_ALIGN8_SYS_CHK")
    # a mixed batch at bandwidth 0: one sub-batch per width class
    _same(ctx, short[:20] + longq[:10], _par(S.MODE_OVERLAP, 0))


@pytest.mark.parametrize("bw", [48, 80])
def test_align8_run_time_width_kernel(ctx, bw):
    pairs = [(q, t) for q, t in _pairs(400 + bw, 30, lens=[100, 300, 1000]) if len(q) > bw]
    for mode in MODES:
        assert "k_align8_fwd_gen" in _same(ctx, pairs, _par(mode, bw))


def test_align8_score_only_handover_and_slices(ctx, monkeypatch):
    pairs = _pairs(500, 40)
    for mode in MODES:
        assert "score-only" in _same(ctx, pairs, _par(mode, 128), score_only=True)
    monkeypatch.setenv("BSA_DEBUG_HANDOVER", "7")
    _same(ctx, pairs, _par(S.MODE_GLOBAL, 128))
    assert ctx.last_handover() > 0
    monkeypatch.delenv("BSA_DEBUG_HANDOVER")
    monkeypatch.setenv("BSA_BATCH_SLICES", "2")
    _same(ctx, pairs, _par(S.MODE_GLOBAL, 128))
    _same(ctx, pairs, _par(S.MODE_EXTEND, 64), score_only=True)


def test_align8_both_staging_forms(ctx):
    # >= 8192 staged bytes a pair: a block per pair; the rest of this file: a wave per pair
    long = _pairs(600, 6, lens=[5000, 6001, 7003])
    assert long and min(len(t) for _, t in long) >= 5000
    _same(ctx, long, _par(S.MODE_GLOBAL, 128), oracle=2)
    # through the Python entry points
    import bsalign_amd as B
    pairs = _pairs(601, 33)
    a, ac, ast = ctx.align_batch(pairs, _par(S.MODE_GLOBAL, 128))
    b, bc, bst = ctx.align_batch(pairs, _par(S.MODE_GLOBAL, 128), seq2bit=True)
    assert np.array_equal(a, b) and np.array_equal(ast, bst) and all(np.array_equal(x, y) for x, y in zip(ac, bc))
    a, ast = ctx.align_scores(pairs, _par(S.MODE_OVERLAP, 64))
    b, bst = ctx.align_scores(pairs, _par(S.MODE_OVERLAP, 64), seq2bit=True)
    assert np.array_equal(a, b) and np.array_equal(ast, bst)
    assert B.MODE_SEQ2BIT == 0x800


@pytest.mark.parametrize("bw", [0, 64, 256])
def test_edit_all_modes(ctx, bw):
    import bsalign_amd as B
    pairs = _pairs(700 + bw, 36)
    for mode in MODES:
        p = B.EditParams()
        p.mode, p.bandwidth = mode, bw
        _same(ctx, pairs, p, edit=True)
        _same(ctx, pairs, p, edit=True, score_only=True)
    a, ac, ast = ctx.edit_batch(pairs, S.MODE_EXTEND, bw)
    b, bc, bst = ctx.edit_batch(pairs, S.MODE_EXTEND, bw, seq2bit=True)
    assert np.array_equal(a, b) and np.array_equal(ast, bst) and all(np.array_equal(x, y) for x, y in zip(ac, bc))
    a, ast = ctx.edit_scores(pairs, S.MODE_GLOBAL, bw)
    b, bst = ctx.edit_scores(pairs, S.MODE_GLOBAL, bw, seq2bit=True)
    assert np.array_equal(a, b) and np.array_equal(ast, bst)


def test_edit_many_short_pairs(ctx):
    """65 536 pairs or more: the wave-per-pair form of the edit staging kernel"""
    import bsalign_amd as B
    rng = np.random.default_rng(800)
    n = 65536 + 37
    lens = rng.integers(1, 70, size=n)
    pairs = []
    for L in lens:
        t = rng.integers(0, 4, size=int(L)).astype(np.uint8)
        q = S.mutate(rng, t, 0.1)
        pairs.append((q if len(q) else t[:1].copy(), t))
    p = B.EditParams()
    p.mode, p.bandwidth = S.MODE_GLOBAL, 64
    _same(ctx, pairs, p, edit=True, oracle=16)


def _dev_blob(pairs):
    import torch
    words, qoff, qlen, toff, tlen = _blob(pairs)
    return torch.from_numpy(words.view(np.int64)).cuda(), qoff, qlen, toff, tlen


def test_plans_on_device_pointers(ctx):
    import torch
    import bsalign_amd as B
    pairs = _pairs(900, 40)
    n = len(pairs)
    d_words, qoff, qlen, toff, tlen = _dev_blob(pairs)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    for edit in (False, True):
        if edit:
            plan = B.EditPlan(ctx, qoff, qlen, toff, tlen, S.MODE_GLOBAL | B.MODE_SEQ2BIT, 128)
            ref, rc, rst = ctx.edit_batch(pairs, S.MODE_GLOBAL, 128)
        else:
            plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, _par(S.MODE_GLOBAL | B.MODE_SEQ2BIT, 128))
            ref, rc, rst = ctx.align_batch(pairs, _par(S.MODE_GLOBAL, 128))
        d_out = torch.zeros(n * 10, dtype=torch.int32, device="cuda")
        d_cig = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run(d_words, d_out, d_cig, d_off, d_st)
        ctx.sync()
        out = d_out.cpu().numpy().reshape(n, 10)
        off = d_off.cpu().numpy()
        cig = d_cig.cpu().numpy().view(np.uint32)
        assert np.array_equal(out, ref.view(np.int32).reshape(n, 10)) and np.array_equal(d_st.cpu().numpy().view(np.uint32), rst)
        for k in range(n):
            assert np.array_equal(cig[int(off[k]):int(off[k + 1])], rc[k]), k
        # a d_seqs that is not 8-byte aligned: refused before anything is launched
        rcode = (B.lib().bsa_edit_run if edit else B.lib().bsa_align_run)(plan.h, C.c_void_p(d_words.data_ptr() + 4), C.c_void_p(d_out.data_ptr()),
                                                                         None, 0, None, None)
        assert rcode == -2
        plan.close()


def test_device_packer_and_a_resident_batch(ctx):
    """4096 x 10 kbp from bsa_synth_pairs_dev, packed on the device: the words are pack2bit's, the packed run's results the unpacked run's"""
    import torch
    import bsalign_amd as B
    n, L = 4096, 10000
    lib = B.lib()
    stride = lib.bsa_synth_stride(L)
    nb = 2 * n * stride
    d_seqs = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    d_qlen = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, S.SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    ctx.sync()
    nw = (nb + 31) // 32
    d_bits = torch.full((nw,), -1, dtype=torch.int64, device="cuda")
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.seq_pack2bit(d_seqs, d_bits, d_bad)
    ctx.sync()
    host = d_seqs.cpu().numpy()
    assert np.array_equal(d_bits.cpu().numpy().view(np.uint64), B.pack2bit(host))
    assert int(d_bad.item()) == 0 and not (host > 3).any()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
    res = []
    for mode, d in ((S.MODE_GLOBAL, d_seqs), (S.MODE_GLOBAL | B.MODE_SEQ2BIT, d_bits)):
        plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, _par(mode, 128))
        d_out = torch.zeros(n * 10, dtype=torch.int32, device="cuda")
        d_cig = torch.zeros(n * (L // 4), dtype=torch.int32, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run(d, d_out, d_cig, d_off, d_st)
        ctx.sync()
        off = d_off.cpu().numpy()
        res.append((d_out.cpu().numpy(), off, d_cig.cpu().numpy()[:int(off[-1])], d_st.cpu().numpy()))
        plan.close()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert not res[1][3].any()
    q, t = S.synth_pair(n - 1, L)
    o, cig, _ = S.oracle_align(q, t, S.MODE_GLOBAL, 128, *SC)
    assert np.array_equal(res[1][0].reshape(n, 10)[n - 1], o)
    # a code of 4 sets d_bad; the packed word takes it as 0
    codes = torch.tensor([1, 2, 3, 0, 4, 1], dtype=torch.uint8, device="cuda")
    bits = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_bad.zero_()
    torch.cuda.synchronize()
    ctx.seq_pack2bit(codes, bits, d_bad)
    ctx.sync()
    assert int(d_bad.item()) == 1
    assert int(bits.cpu().numpy().view(np.uint64)[0]) == int(B.pack2bit(np.array([1, 2, 3, 0, 0, 1], np.uint8))[0])
    d_bad.zero_()
    torch.cuda.synchronize()
    ctx.seq_pack2bit(codes[:4], bits, d_bad)
    ctx.sync()
    assert int(d_bad.item()) == 0


def test_argument_errors(ctx):
    import bsalign_amd as B
    pairs = _pairs(1000, 5)
    words, qoff, qlen, toff, tlen = _blob(pairs)
    n = len(pairs)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    for fn, par in ((B.lib().bsa_align_batch, _par(S.MODE_GLOBAL | B.MODE_SEQ2BIT, 128)),
                    (B.lib().bsa_edit_batch, B.EditParams(S.MODE_GLOBAL | B.MODE_SEQ2BIT, 128))):
        def call(nbytes, to):
            return fn(ctx.h, words.ctypes.data, nbytes, qoff.ctypes.data, qlen.ctypes.data, to.ctypes.data, tlen.ctypes.data, n, C.byref(par),
                      out.ctypes.data, None, 0, None, st.ctypes.data)
        assert call(words.nbytes, toff) == 0
        past = toff.copy()
        past[-1] = 4 * words.nbytes - int(tlen[-1]) + 1
        assert call(words.nbytes, past) == -2
        assert call(words.nbytes - 4, toff) == -2
