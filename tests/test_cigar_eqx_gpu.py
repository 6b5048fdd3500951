"""BSA_MODE_CIGAR_EQX on the MI355X.  For every case of cigar_eqx_cases.py: the flagged call's words are expand_eqx of the ORACLE's
CIGAR, its records and status the oracle's and bit-identical to the plain call's on the same context, collapse_eqx of its words the
plain call's words, no equal neighbouring ops and no zero lengths -- on every traceback kernel (each case asserts which one ran), the
routes inside bsa_align_batch, several chunks and both ways out of one chunk, device-pointer plans with the arena one word short and
exactly large enough, packed sequences, score-only, empty and bad-base pairs, M words of 10 000 columns and CIGARs of thousands of words."""
import ctypes as C

import numpy as np
import pytest

import cigar_eqx_cases as K
import support as S

pytestmark = pytest.mark.gpu


def _rec(out, k):
    return np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)


def _compare(pairs, oracle, flagged, plain, what):
    """the checks every case makes; returns the number of pairs compared word by word"""
    import bsalign_amd as B
    fo, fc, fs = flagged
    po, pc, ps = plain
    assert np.array_equal(fo.view(np.int32), po.view(np.int32)), what            # (1) out and status bit-identical to the plain call
    assert np.array_equal(fs, ps), what
    full = 0
    for k, ((q, t), (res, cig, n)) in enumerate(zip(pairs, oracle)):
        if n == S.ORC_ERR_TRACE:
            assert fs[k] & B.ST_TRACE and len(fc[k]) == 0, (what, k, fs[k])
            continue
        assert fs[k] == 0 and np.array_equal(_rec(fo, k), res), (what, k, fs[k], fo[k], res)
        want = B.expand_eqx(cig, q, t, res[1], res[3])
        assert np.array_equal(fc[k], want), (what, k, S.cigar_str(fc[k])[:160], S.cigar_str(want)[:160])
        assert np.array_equal(B.collapse_eqx(fc[k]), pc[k]), (what, k)
        assert len(fc[k]) == 0 or K.well_formed(fc[k]), (what, k)
        full += 1
    assert full >= (1.0 - K.MAX_UNTRACEABLE) * len(pairs), (what, full)
    return full


def _setenv(monkeypatch, env):
    for name, val in env.items():
        monkeypatch.setenv(name, val)


@pytest.mark.parametrize("case", K.ALIGN_CASES, ids=lambda c: c[0])
def test_align8(ctx, monkeypatch, case):
    import bsalign_amd as B
    cid, cname, mode, bw, sc, flags, env, fwd, trace = case
    _setenv(monkeypatch, env)
    pairs = K.corpus(cname)
    par = B.make_params(mode | flags, bw, *K.SC[sc])
    flagged = ctx.align_batch(pairs, par, eqx=True)
    names, handed = ctx.last_kernel_names(), ctx.last_handover()
    plain = ctx.align_batch(pairs, par)
    _compare(pairs, K.align_oracle(cname, mode, bw, sc), flagged, plain, cid)
    if fwd is not None:
        assert fwd in names[0], names
    if trace is not None:
        assert trace in names[1], names
    if "BSA_DEBUG_HANDOVER" in env:
        assert handed > 0
    if cid == "long-words":
        assert max(len(c) for c in flagged[1]) >= 2 * 57
    if cid == "many-words":
        assert len(plain[1][0]) > 64 and len(plain[1][1]) > 4096 and len(flagged[1][1]) > len(plain[1][1])


def test_align8_pairs_handed_over_keep_the_flag(ctx):
    """scorings outside the guard on the checked whole-query kernel: the pairs it flags are re-run by the literal kernels inside bsa_align_batch"""
    import bsalign_amd as B
    handed = 0
    for cid, cname, mode, bw, sc, flags, env, fwd, trace in K.HANDOVER_CASES:
        pairs = K.corpus(cname)
        par = B.make_params(mode, bw, *K.SC[sc])
        flagged = ctx.align_batch(pairs, par, eqx=True)
        names, h = ctx.last_kernel_names(), ctx.last_handover()
        plain = ctx.align_batch(pairs, par)
        _compare(pairs, K.align_oracle(cname, mode, bw, sc), flagged, plain, cid)
        assert fwd in names[0], names
        handed += h
    assert handed > 0


@pytest.mark.parametrize("case", K.EDIT_CASES, ids=lambda c: c[0])
def test_edit(ctx, monkeypatch, case):
    cid, cname, mode, bw, env, fwd, trace, nottrace = case
    _setenv(monkeypatch, env)
    pairs = K.corpus(cname)
    flagged = ctx.edit_batch(pairs, mode, bw, eqx=True)
    names = ctx.last_kernel_names()
    plain = ctx.edit_batch(pairs, mode, bw)
    _compare(pairs, K.edit_oracle(cname, mode, bw), flagged, plain, cid)
    if fwd is not None:
        assert fwd in names[0], names
    assert trace in names[1], names
    if nottrace is not None:
        assert nottrace not in names[1], names
    if cid == "long-words":
        assert max(len(c) for c in flagged[1]) > 4096                   # the alternating pair: thousands of one-column runs out of a few words


def _same_lists(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_chunks_arena_route_and_slices(ctx, monkeypatch):
    """one chunk straight to the caller's arena (k_cigar_final_direct's EQX form) is the reference point; BSA_CIGAR_VIA_ARENA=1 and several chunks go
    through the staging arena (k_cigar_collect's EQX form, then k_cigar_final); BSA_BATCH_SLICES=2 runs two plans"""
    import bsalign_amd as B
    pairs = K.corpus("mixed")
    par = B.make_params(K.G, 128, *K.SC["affine"])
    oracle = K.align_oracle("mixed", K.G, 128, "affine")
    eoracle = K.edit_oracle("mid", K.G, 256)
    direct = ctx.align_batch(pairs, par, eqx=True)
    plain = ctx.align_batch(pairs, par)
    _compare(pairs, oracle, direct, plain, "direct")
    edirect = ctx.edit_batch(K.corpus("mid"), K.G, 256, eqx=True)
    eplain = ctx.edit_batch(K.corpus("mid"), K.G, 256)
    _compare(K.corpus("mid"), eoracle, edirect, eplain, "edit direct")
    for env in ({"BSA_CIGAR_VIA_ARENA": "1"}, {"BSA_CHUNK_PAIRS": "7"}, {"BSA_CHUNK_PAIRS": "5", "BSA_PIPELINE": "1"}, {"BSA_BATCH_SLICES": "2"}):
        _setenv(monkeypatch, env)
        got = ctx.align_batch(pairs, par, eqx=True)
        assert _same_lists(got, direct), env
        assert _same_lists(ctx.align_batch(pairs, par), plain), env
        egot = ctx.edit_batch(K.corpus("mid"), K.G, 256, eqx=True)
        assert _same_lists(egot, edirect), env
        for name in env:
            monkeypatch.delenv(name)


def _raw(ctx, fn, pairs, par, cap, seq2bit=False):
    """the C call with an arena of `cap` words: (return code, results, arena, offsets, status)"""
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs, seq2bit)
    n = len(pairs)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    off = np.full(n + 1, 7, dtype=np.uint64)
    rc = fn(ctx.h, seqs.ctypes.data, seqs.nbytes, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data, n, C.byref(par),
            out.ctypes.data, cig.ctypes.data, cap, off.ctypes.data, st.ctypes.data)
    return rc, out, cig, off, st


@pytest.mark.parametrize("edit", [False, True], ids=["align", "edit"])
def test_arena_capacity_counts_expanded_words(ctx, edit):
    """host pointers with a short arena: BSA_E_CIGAR_CAP and cigar_off[n] = the expanded total; device-pointer plans with the arena one word
    too small (offsets still complete, nothing written behind the arena) and exactly large enough"""
    import torch
    import bsalign_amd as B
    pairs = K.corpus("mid")
    n = len(pairs)
    if edit:
        par = B.EditParams(K.G | B.MODE_CIGAR_EQX, 256)
        fn = B.lib().bsa_edit_batch
        ref = ctx.edit_batch(pairs, K.G, 256, eqx=True)
        nplain = sum(len(c) for c in ctx.edit_batch(pairs, K.G, 256)[1])
    else:
        par = B.make_params(K.G | B.MODE_CIGAR_EQX, 128, *K.SC["affine"])
        fn = B.lib().bsa_align_batch
        ref = ctx.align_batch(pairs, par)
        nplain = sum(len(c) for c in ctx.align_batch(pairs, B.make_params(K.G, 128, *K.SC["affine"]))[1])
    total = sum(len(c) for c in ref[1])
    assert total > nplain                                       # an arena sized for the plain words is too small
    rc, out, cig, off, st = _raw(ctx, fn, pairs, par, nplain)
    assert rc == -5 and int(off[n]) == total
    rc, out, cig, off, st = _raw(ctx, fn, pairs, par, total - 1)
    assert rc == -5 and int(off[n]) == total
    rc, out, cig, off, st = _raw(ctx, fn, pairs, par, total)
    assert rc == 0 and int(off[n]) == total and np.array_equal(out, ref[0])
    assert all(np.array_equal(cig[int(off[k]):int(off[k + 1])], ref[1][k]) for k in range(n))
    # device pointers
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    plan = B.EditPlan(ctx, qoff, qlen, toff, tlen, K.G | B.MODE_CIGAR_EQX, 256) if edit else B.AlignPlan(ctx, qoff, qlen, toff, tlen, par)
    d_seqs = torch.from_numpy(seqs).cuda()
    want_off = np.concatenate([[0], np.cumsum([len(c) for c in ref[1]])]).astype(np.int64)
    for cap in (total - 1, total):
        d_out = torch.zeros(n * 10, dtype=torch.int32, device="cuda")
        d_cig = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run(d_seqs, d_out, d_cig[:cap], d_off, d_st)
        ctx.sync()
        assert np.array_equal(d_off.cpu().numpy(), want_off), cap
        assert np.array_equal(d_out.cpu().numpy().reshape(n, 10), ref[0].view(np.int32).reshape(n, 10))
        words = d_cig.cpu().numpy().view(np.uint32)
        assert (words[cap:] == 0xFFFFFFFF).all(), cap                      # nothing behind the arena
        if cap == total:
            assert np.array_equal(words[:total], np.concatenate(ref[1]))
        else:
            fit = int(np.searchsorted(want_off, cap, side="right")) - 1       # pairs whose words end inside the arena are all there
            assert fit >= n - 2 and np.array_equal(words[:want_off[fit]], np.concatenate(ref[1])[:want_off[fit]])
    plan.close()


def test_packed_sequences_score_only_and_pairs_without_a_cigar(ctx):
    import bsalign_amd as B
    pairs = K.corpus("mixed")
    par = B.make_params(K.G, 128, *K.SC["affine"])
    ref = ctx.align_batch(pairs, par, eqx=True)
    assert _same_lists(ctx.align_batch(pairs, par, eqx=True, seq2bit=True), ref)
    eref = ctx.edit_batch(pairs, K.E, 0, eqx=True)
    assert _same_lists(ctx.edit_batch(pairs, K.E, 0, eqx=True, seq2bit=True), eref)
    assert any((c & 15 == B.CIGAR_X).any() for c in eref[1])
    # BSA_MODE_SCORE_ONLY: no CIGAR, offsets all zero, not an error, the results of the call without BSA_MODE_CIGAR_EQX
    sp = B.make_params(K.G | B.MODE_SCORE_ONLY | B.MODE_CIGAR_EQX, 128, *K.SC["affine"])
    rc, out, cig, off, st = _raw(ctx, B.lib().bsa_align_batch, pairs, sp, 64)
    assert rc == 0 and not off.any() and not cig.any()
    so, sst = ctx.align_scores(pairs, par)
    assert np.array_equal(out, so) and np.array_equal(st, sst)
    rc, out, cig, off, st = _raw(ctx, B.lib().bsa_edit_batch, pairs, B.EditParams(K.G | B.MODE_SCORE_ONLY | B.MODE_CIGAR_EQX, 256), 64)
    assert rc == 0 and not off.any() and not cig.any()
    so, sst = ctx.edit_scores(pairs, K.G, 256)
    assert np.array_equal(out, so) and np.array_equal(st, sst)
    # an empty pair, a pair with a bad base and a good one: the first two return no CIGAR with the flag as without it
    rng = np.random.default_rng(3)
    t = rng.integers(0, 4, size=300).astype(np.uint8)
    bad = S.mutate(rng, t, 0.1)
    bad[17] = 7
    good = S.mutate(rng, t, 0.1)
    trio = [(np.zeros(0, np.uint8), t), (bad, t), (good, t)]
    for flagged, plain in ((ctx.align_batch(trio, par, eqx=True), ctx.align_batch(trio, par)),
                           (ctx.edit_batch(trio, K.G, 256, eqx=True), ctx.edit_batch(trio, K.G, 256))):
        assert np.array_equal(flagged[0], plain[0]) and np.array_equal(flagged[2], plain[2])
        assert flagged[2][0] & B.ST_EMPTY and flagged[2][1] & B.ST_BAD_BASE and flagged[2][2] == 0
        assert len(flagged[1][0]) == 0 and len(plain[1][0]) == 0
        assert len(flagged[1][1]) == len(plain[1][1]) == 0
        assert K.well_formed(flagged[1][2]) and np.array_equal(B.collapse_eqx(flagged[1][2]), plain[1][2])
    res, cig, n = S.oracle_align(good, t, K.G, 128, *K.SC["affine"])
    assert np.array_equal(ctx.align_batch(trio, par, eqx=True)[1][2], B.expand_eqx(cig, good, t))
