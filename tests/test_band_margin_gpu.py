"""BSA_MODE_BAND_MARGIN on the MI355X.  For every pair of every case the device margin equals band_margin_cases.margin_ref applied to the
ORACLE's record, CIGAR and band trajectory; records, words, offsets and the low status half equal the same call without the flag, whose upper
status half is 0.  Three modes x four scorings x bandwidths 16 .. 1024 and 0, the kernel routes asserted by name, every flag the margin combines
with, every route inside bsa_align_batch, several chunks, device-pointer plans, single words of thousands of rows, and the BSA_E_ARG cases."""
import ctypes as C

import numpy as np
import pytest

import band_margin_cases as K
import cigar_eqx_cases as KE
import support as S

pytestmark = pytest.mark.gpu

E_ARG = -2


def _both(ctx, pairs, par, **kw):
    flagged = ctx.align_batch(pairs, par, margins=True, **kw)
    names, handed = ctx.last_kernel_names(), ctx.last_handover()
    plain = ctx.align_batch(pairs, par, **kw)
    return flagged, plain, names, handed


def _same_as_plain(flagged, plain, what):
    fo, fc, fs, fm = flagged
    po, pc, ps = plain
    assert np.array_equal(fo.view(np.int32), po.view(np.int32)), what
    assert len(fc) == len(pc) and all(np.array_equal(x, y) for x, y in zip(fc, pc)), what
    assert np.array_equal(fs, ps), (what, fs, ps)            # low half; the plain call's upper half is 0
    assert not (ps >> 16).any(), what


def _check(expected, flagged, plain, what):
    """the checks every case makes: bit-identity with the plain call, then every margin against the oracle's"""
    import bsalign_amd as B
    _same_as_plain(flagged, plain, what)
    fo, fc, fs, fm = flagged
    assert fm.dtype == np.uint16
    full = 0
    for k, want in enumerate(expected):
        if want is None:          # the reference's traceback does not terminate: no CIGAR, no margin
            assert fs[k] & B.ST_TRACE and len(fc[k]) == 0 and fm[k] == K.NONE, (what, k, fs[k], fm[k])
            continue
        assert fs[k] == 0, (what, k, fs[k])
        print("%s pair %d: margin %d, oracle %d" % (what, k, fm[k], want))
        assert fm[k] == want, (what, k, int(fm[k]), want, S.cigar_str(fc[k])[:120])
        full += 1
    assert full >= (1.0 - K.MAX_UNTRACEABLE) * len(expected), (what, full)


def _route(bw, which, scname):
    """a substring the forward kernel's name must have for this case, or None where the dispatch depends on more than the bandwidth"""
    if bw == 1024:
        return "k_align8_fwd_gen"                   # run-time width (bandwidth 48 too, but its corpus also holds whole-query pairs: bsa_align_batch
    if bw in (16, 512):                             # runs those as sub-batches of their own and the last one's kernels are the ones reported)
        return "row records"
    if bw == 128:
        return "k_align8_fwd_x"                     # compact, one- and two-piece
    if bw == 0 and which == "long":
        return "k_align8_fwd_sys"                   # systolic
    return None


CASES = [(bw, "short") for bw in K.BANDWIDTHS] + [(0, "short"), (0, "long")]


@pytest.mark.parametrize("scname", list(K.SC))
@pytest.mark.parametrize("mode", K.MODES, ids=["global", "overlap", "extend"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "bw%d-%s" % c)
def test_margins_equal_the_oracles(ctx, case, mode, scname):
    import bsalign_amd as B
    bw, which = case
    pairs = K.pairs_of(bw, which)
    par = B.make_params(mode, bw, *K.SC[scname])
    flagged, plain, names, _ = _both(ctx, pairs, par)
    what = "bw%d-%s-mode%d-%s" % (bw, which, mode, scname)
    expected = K.expected(bw, mode, scname, which)
    _check(expected, flagged, plain, what)
    want = _route(bw, which, scname)
    if want is not None:
        assert want in names[0], (what, names)
    if bw == 0:
        assert (flagged[3] == K.NONE).all(), what


def test_every_route_really_taken(ctx):
    """compact, row-record, run-time-width and systolic slots, each by the name of the kernel that filled them"""
    import bsalign_amd as B
    for bw, which, fwd, trace in ((128, "short", "k_align8_fwd_x", "k_align8_trace_codes"), (64, "short", "k_align8_fwd_x", "k_align8_trace_codes"),
                                  (16, "short", "row records", "k_align8_backcal"), (512, "short", "row records", "k_align8_backcal"),
                                  (48, "short", "k_align8_fwd_gen", "k_align8_backcal"), (0, "long", "k_align8_fwd_sys", "k_align8_trace_sys")):
        par = B.make_params(K.G, bw, *K.SC["affine"])
        pairs, expected = K.pairs_of(bw, which), K.expected(bw, K.G, "affine", which)
        if bw:                    # the moving bands alone: one plan, one forward kernel
            keep = [k for k, (q, _) in enumerate(pairs) if len(q) > bw]
            pairs, expected = [pairs[k] for k in keep], [expected[k] for k in keep]
            assert any(e == 0 for e in expected) and any(e not in (None, 0, K.NONE) for e in expected)
        flagged, plain, names, _ = _both(ctx, pairs, par)
        _check(expected, flagged, plain, "route-bw%d" % bw)
        assert fwd in names[0] and trace in names[1], (bw, names)
    par = B.make_params(K.G, 128, *K.SC["twopiece"])
    flagged, plain, names, _ = _both(ctx, K.pairs_of(128), par)
    _check(K.expected(128, K.G, "twopiece"), flagged, plain, "route-twopiece")
    assert "k_align8_fwd_x2" in names[0] and "codes2" in names[1], names


@pytest.mark.parametrize("mode", K.MODES, ids=["global", "overlap", "extend"])
def test_combines_with_the_other_flags(ctx, mode):
    """ROWRECORDS, SEQ2BIT, QSTRAND (marked and unmarked pairs) and CIGAR_EQX: the margin is the plain one"""
    import bsalign_amd as B
    bw, sc = 64, "affine"
    pairs = K.corpus(bw)
    expected = K.expected(bw, mode, sc)
    par = B.make_params(mode, bw, *K.SC[sc])
    base = ctx.align_batch(pairs, par, margins=True)
    _check(expected, base, ctx.align_batch(pairs, par), "base")
    # row records: the literal kernels' slots
    rpar = B.make_params(mode | B.MODE_ROWRECORDS, bw, *K.SC[sc])
    flagged, plain, names, _ = _both(ctx, pairs, rpar)
    _check(expected, flagged, plain, "rowrecords")
    assert "row records" in names[0] and "k_align8_backcal" in names[1], names
    # packed sequences
    flagged, plain, _, _ = _both(ctx, pairs, par, seq2bit=True)
    _check(expected, flagged, plain, "seq2bit")
    # strands: every second query stored as its reverse complement and marked -- the aligner sees the corpus' own queries
    strands = [k % 2 == 0 for k in range(len(pairs))]
    stored = [(B.revcomp(q) if s else q, t) for (q, t), s in zip(pairs, strands)]
    flagged, plain, _, _ = _both(ctx, stored, par, strands=strands)
    _check(expected, flagged, plain, "qstrand")
    flagged, plain, _, _ = _both(ctx, stored, par, strands=strands, seq2bit=True)
    _check(expected, flagged, plain, "qstrand+seq2bit")
    # = / X words count as M
    flagged, plain, _, _ = _both(ctx, pairs, par, eqx=True)
    _same_as_plain(flagged, plain, "eqx")
    assert np.array_equal(flagged[3], base[3]) and any((c & 15 == B.CIGAR_X).any() for c in flagged[1])
    flagged, plain, _, _ = _both(ctx, pairs, rpar, eqx=True, seq2bit=True)
    _same_as_plain(flagged, plain, "eqx+rowrecords+seq2bit")
    assert np.array_equal(flagged[3], base[3])


def test_slices_chunks_and_workspace_limit(ctx, monkeypatch):
    import bsalign_amd as B
    bw, sc = 128, "affine"
    pairs = K.corpus(bw)
    par = B.make_params(K.G, bw, *K.SC[sc])
    expected = K.expected(bw, K.G, sc)
    for env in ({"BSA_BATCH_SLICES": "2"}, {"BSA_CHUNK_PAIRS": "7"}, {"BSA_CHUNK_PAIRS": "5", "BSA_PIPELINE": "1"}, {"BSA_CIGAR_VIA_ARENA": "1"}):
        for name, val in env.items():
            monkeypatch.setenv(name, val)
        flagged, plain, _, _ = _both(ctx, pairs, par)
        _check(expected, flagged, plain, str(env))
        flagged, plain, _, _ = _both(ctx, pairs, par, eqx=True)
        _same_as_plain(flagged, plain, str(env) + " eqx")
        assert [m for m, e in zip(flagged[3], expected) if e is not None] == [e for e in expected if e is not None], env
        for name in env:
            monkeypatch.delenv(name)
    # a workspace limit that holds the largest pair but not the batch: several chunks sharing one region
    need = max(len(t) for _, t in pairs) * 64 + (max(len(t) for _, t in pairs) + 2) * 4 + 4096
    small = B.Context(0, workspace_limit=4 * need)
    try:
        flagged = small.align_batch(pairs, par, margins=True)
        _check(expected, flagged, small.align_batch(pairs, par), "workspace limit")
    finally:
        small.close()


def test_mixed_width_whole_query_batch(ctx):
    """bandwidth 0 over queries of 20 .. 900 bases: bsa_align_batch runs one sub-batch per width class; every margin is NONE"""
    import bsalign_amd as B
    pairs = K.whole_corpus("mixed")
    for mode in K.MODES:
        par = B.make_params(mode, 0, *K.SC["affine"])
        flagged, plain, _, _ = _both(ctx, pairs, par)
        _check(K.expected(0, mode, "affine", "mixed"), flagged, plain, "mixed-%d" % mode)
        assert (flagged[3] == K.NONE).all()
    # a bandwidth the register kernels do not have over queries on both sides of it: the short ones are whole-query sub-batches, the long ones
    # keep a moving band on the run-time-width kernel and get real margins
    par = B.make_params(K.G, 48, *K.SC["affine"])
    flagged, plain, _, _ = _both(ctx, K.corpus(48), par)
    _check(K.expected(48, K.G, "affine"), flagged, plain, "classes-48")
    assert (flagged[3] == K.NONE).any() and (flagged[3] == 0).any()


def test_pairs_handed_over(ctx, monkeypatch):
    """scorings outside the guard on the checked whole-query kernel: the pairs it flags are re-run by the literal kernels inside bsa_align_batch;
    and the debug hook that hands every third pair of a moving band over: its margin comes from the re-run's own slot"""
    import bsalign_amd as B
    handed = 0
    for cid, cname, mode, bw, sc, flags, env, fwd, trace in KE.HANDOVER_CASES:
        pairs = KE.corpus(cname)
        par = B.make_params(mode, bw, *KE.SC[sc])
        flagged, plain, names, h = _both(ctx, pairs, par)
        _same_as_plain(flagged, plain, cid)
        assert (flagged[3] == K.NONE).all() and fwd in names[0], (cid, names)
        handed += h
    assert handed > 0
    monkeypatch.setenv("BSA_DEBUG_HANDOVER", "3")
    for bw in (64, 128):
        par = B.make_params(K.G, bw, *K.SC["affine"])
        flagged, plain, _, h = _both(ctx, K.corpus(bw), par)
        assert h > 0
        _check(K.expected(bw, K.G, "affine"), flagged, plain, "debug-handover-%d" % bw)


def test_device_pointer_plan(ctx):
    """bsa_align_plan_create / bsa_align_run with the flag: the margins of the host-pointer call; flagged empty and bad-base pairs get NONE"""
    import torch
    import bsalign_amd as B
    bw, sc = 128, "affine"
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=300).astype(np.uint8)
    bad = S.mutate(rng, t, 0.1)
    bad[17] = 7
    pairs = [(np.zeros(0, np.uint8), t), (bad, t)] + K.corpus(bw)
    expected = [K.NONE, K.NONE] + K.expected(bw, K.G, sc)
    n = len(pairs)
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    d_seqs = torch.from_numpy(seqs).cuda()
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    got = {}
    for flags in (0, B.MODE_BAND_MARGIN, B.MODE_BAND_MARGIN | B.MODE_CIGAR_EQX):
        plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(K.G | flags, bw, *K.SC[sc]))
        d_out = torch.zeros(n * 10, dtype=torch.int32, device="cuda")
        d_cig = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):           # a plan is run again and again: the second run must not see the first one's margins
            plan.run(d_seqs, d_out, d_cig, d_off, d_st)
        ctx.sync()
        got[flags] = (d_out.cpu().numpy().copy(), d_off.cpu().numpy().copy(), d_cig.cpu().numpy().copy(), d_st.cpu().numpy().view(np.uint32).copy())
        if flags:
            ms, launches = ctx.last_margin_ms()
            assert launches >= 1 and ms > 0
            with pytest.raises(B.BsaError) as e:
                plan.run(d_seqs, d_out, d_cig, d_off, None)           # no status array: nowhere for the margin to go
            assert e.value.code == E_ARG
        else:
            assert ctx.last_margin_ms()[1] == 0                       # without the flag the pass is not launched
        plan.close()
    po, poff, pcig, pst = got[0]
    fo, foff, fcig, fst = got[B.MODE_BAND_MARGIN]
    assert not (pst >> 16).any()
    assert np.array_equal(fo, po) and np.array_equal(foff, poff) and np.array_equal(fcig, pcig) and np.array_equal(fst & 0xFFFF, pst)
    assert pst[0] & B.ST_EMPTY and pst[1] & B.ST_BAD_BASE
    margins = (fst >> 16).astype(np.int64)
    for k, want in enumerate(expected):
        if want is not None:
            assert margins[k] == want, (k, margins[k], want)
    eo, eoff, ecig, est = got[B.MODE_BAND_MARGIN | B.MODE_CIGAR_EQX]
    assert np.array_equal(est, fst) and np.array_equal(eo, po)


def test_single_words_of_thousands_of_rows(ctx):
    """two identical 10 kbp reads are ONE M word of 10 000 rows; a 3 kbp read inside a longer target is one M word beside a band that moved"""
    import bsalign_amd as B
    rng = np.random.default_rng(77)
    t = rng.integers(0, 4, size=10000).astype(np.uint8)
    t2 = rng.integers(0, 4, size=3400).astype(np.uint8)
    cases = [(K.G, 128, (t.copy(), t)), (K.G, 64, (t.copy(), t)), (K.O, 256, (t2[100:3100].copy(), t2)), (K.O, 128, (t2[:3000].copy(), t2)),
             (K.E, 64, (t2[:3000].copy(), t2))]
    moved = 0
    for mode, bw, (q, tt) in cases:
        par = B.make_params(mode, bw, *K.SC["affine"])
        flagged, plain, _, _ = _both(ctx, [(q, tt)], par)
        res, cig, n, begs = S.oracle_align(q, tt, mode, bw, *K.SC["affine"], want_begs=True)
        assert n == 1 and cig[0] & 15 == 0 and cig[0] >> 4 == len(q)
        moved += int(begs[int(res[3]):int(res[4])].max() > 0)
        _check([K.margin_ref(len(q), len(tt), bw, res, cig, begs)], flagged, plain, "long-%d-%d" % (mode, bw))
        assert flagged[3][0] != K.NONE
    assert moved == len(cases)


def _raw(ctx, fn, pairs, par, status=True):
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    n = len(pairs)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    cig = np.zeros(cap, dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    return fn(ctx.h, seqs.ctypes.data, seqs.nbytes, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data, n, C.byref(par),
              out.ctypes.data, cig.ctypes.data, cap, off.ctypes.data, st.ctypes.data if status else None)


def test_argument_errors(ctx):
    import bsalign_amd as B
    pairs = K.corpus(64)[:6]
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    ok = B.make_params(K.G | B.MODE_BAND_MARGIN, 64, *K.SC["affine"])
    assert _raw(ctx, B.lib().bsa_align_batch, pairs, ok) == 0
    # no status array
    assert _raw(ctx, B.lib().bsa_align_batch, pairs, ok, status=False) == E_ARG
    # score only: there is no path
    so = B.make_params(K.G | B.MODE_BAND_MARGIN | B.MODE_SCORE_ONLY, 64, *K.SC["affine"])
    assert _raw(ctx, B.lib().bsa_align_batch, pairs, so) == E_ARG
    with pytest.raises(B.BsaError) as e:
        B.AlignPlan(ctx, qoff, qlen, toff, tlen, so)
    assert e.value.code == E_ARG
    # the edit aligner does not take the flag
    assert _raw(ctx, B.lib().bsa_edit_batch, pairs, B.EditParams(K.G | B.MODE_BAND_MARGIN, 256)) == E_ARG
    with pytest.raises(B.BsaError) as e:
        B.EditPlan(ctx, qoff, qlen, toff, tlen, K.G | B.MODE_BAND_MARGIN, 256)
    assert e.value.code == E_ARG
    assert _raw(ctx, B.lib().bsa_edit_batch, pairs, B.EditParams(K.G, 256)) == 0
