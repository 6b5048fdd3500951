"""GPU parity under general 4 x 4 substitution matrices: every forward kernel of the 8-bit pairwise path against the oracle, bit-exact.

Each kernel builds its own score lookup and takes smax / smin (which seed row 0 and the band rebasing, and decide every
exact-arithmetic guard) from the matrix; with score_matrix(M, X) a transposed lookup or an M / X assumption cannot be seen.  The
matrices and pairs are tests/matrix_support.py's (tests/test_matrix_corpus_cpu.py shows on the oracle that they tell such bugs apart).
Every case also asserts which forward kernel ran, so that a dispatch change cannot move it off the kernel it covers."""
import ctypes as C

import numpy as np
import pytest

import matrix_support as MS
import support as S

pytestmark = pytest.mark.gpu

MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)
ALL = list(MS.CATALOGUE)


def _check(ctx, pairs, mode, bw, m, gaps):
    """results and CIGAR words equal the oracle's; ORC_ERR_TRACE <=> BSA_ST_TRACE; every other status is 0"""
    import bsalign_amd as B
    out, cigs, status = ctx.align_batch(pairs, B.make_params(mode, bw, 0, 0, *gaps, matrix=m))
    nbad = 0
    msgs = []
    for k, (q, t) in enumerate(pairs):
        res, cig, n = S.oracle_align(q, t, mode, bw, 0, 0, *gaps, mtx=m)
        if n == S.ORC_ERR_TRACE:
            ok = bool(status[k] & B.ST_TRACE)
        else:
            got = np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)
            ok = status[k] == 0 and np.array_equal(got, res) and np.array_equal(cigs[k], cig)
        if not ok:
            nbad += 1
            if len(msgs) < 5:
                msgs.append("pair %d qlen %d tlen %d status %d\n  gpu %s %s\n  orc %s %s" % (
                    k, len(q), len(t), status[k], out[k], S.cigar_str(cigs[k])[:120], res, S.cigar_str(cig)[:120]))
    assert nbad == 0, "%d/%d pairs differ (mode %d bw %d gaps %s matrix %s, %s)\n%s" % (
        nbad, len(pairs), mode, bw, gaps, list(np.asarray(m, np.int8)), ctx.last_kernel_names()[0], "\n".join(msgs))


def _fwd(ctx):
    return ctx.last_kernel_names()[0]


def _pairs(seed, n, bw, **kw):
    return MS.mk_pairs(np.random.default_rng(seed), n, bw, **kw)


@pytest.mark.parametrize("bw", [64, 128, 256])
def test_exact_arithmetic_forward_kernel(ctx, monkeypatch, bw):
    """k_align8_fwd_x (whole pairs, one-piece gaps): every in-guard matrix, all three modes, linear and affine gaps (at bandwidth 128
    with gapo -4: gap openings of 1 .. 3 take the two-bit code rows, their own case below); at 64 also the eight-lane shape"""
    pairs = _pairs(6400 + bw, 40, bw)
    affine = (-4, -2, 0, 0) if bw == 128 else MS.AFFINE
    for name in MS.IN_GUARD_GENERAL:
        m = MS.GENERAL[name]
        for gaps in (affine, MS.LINEAR):
            for mode in MODES:
                _check(ctx, pairs, mode, bw, m, gaps)
                fwd = _fwd(ctx)
                assert fwd.startswith("k_align8_fwd_x") and "two-bit" not in fwd and "two-piece" not in fwd, (name, fwd)
    if bw == 64:
        monkeypatch.setenv("BSA_ALIGN8_X_LANES", "8")
        for name in MS.IN_GUARD_GENERAL:
            _check(ctx, pairs, S.MODE_GLOBAL, bw, MS.GENERAL[name], MS.AFFINE)
            assert _fwd(ctx).startswith("k_align8_fwd_x"), _fwd(ctx)


@pytest.mark.parametrize("gaps", [MS.AFFINE, (-4, -2, 0, 0)])
def test_row_segments_of_the_persistent_forward_kernel(ctx, monkeypatch, gaps):
    """k_align8_fwd_xq (the headline kernel): pairs of 1 500 bp and more in segments of 64 rows, bandwidth 128, global"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "1")
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    pairs = _pairs(6500 + gaps[0], 24, 128, lens=[1500, 1537, 2000, 2600], ratios=(0.9, 1.0, 1.0, 1.1))
    for name in ("asym", "transition", "posmis"):
        _check(ctx, pairs, S.MODE_GLOBAL, 128, MS.GENERAL[name], gaps)
        assert "k_align8_fwd_xq" in _fwd(ctx), (name, _fwd(ctx))


def test_code_rows_with_two_bit_fields(ctx):
    """code format 1 (D / Od as two-bit fields: one-piece gaps with -gapo in 1 .. 3 at bandwidth 128), default dispatch, all modes"""
    pairs = _pairs(6600, 60, 128, eps_list=(0.0, 0.05, 0.2, 0.4))
    m = MS.GENERAL["asym"]
    for gapo in (-1, -2, -3):
        for mode in MODES:
            _check(ctx, pairs, mode, 128, m, (gapo, -2, 0, 0))
            assert "two-bit" in _fwd(ctx), (gapo, _fwd(ctx))


@pytest.mark.parametrize("bw", [64, 128, 256])
def test_packed_forward_kernel_with_code_rows(ctx, monkeypatch, bw):
    """k_align8_fwd_pk<., ., true> (BSA_ALIGN8_FWD=pk): every matrix inside the compact path's guard, the two at its bounds included;
    those two run it under the default dispatch as well (the exact-arithmetic kernel's own bound refuses them)"""
    pairs = _pairs(6700 + bw, 40, bw)
    for name in ("m3g_64", "m2n_128"):
        m, gaps = MS.CATALOGUE[name]
        _check(ctx, pairs, S.MODE_GLOBAL, bw, m, gaps)
        assert "k_align8_fwd_pk<.,.,true>" in _fwd(ctx), (name, _fwd(ctx))
    monkeypatch.setenv("BSA_ALIGN8_FWD", "pk")
    for name in MS.IN_GUARD:
        m, gaps = MS.CATALOGUE[name]
        for mode in MODES:
            _check(ctx, pairs, mode, bw, m, gaps)
            assert "k_align8_fwd_pk<.,.,true>" in _fwd(ctx), (name, _fwd(ctx))


@pytest.mark.parametrize("bw", [64, 128, 256])
def test_two_piece_gaps(ctx, bw):
    """k_align8_fwd_x2 and its code-row walkers: two-piece gaps, all three modes"""
    pairs = _pairs(6800 + bw, 40, bw)
    for name in ("asym", "transition"):
        for mode in MODES:
            _check(ctx, pairs, mode, bw, MS.GENERAL[name], MS.TWOPIECE)
            fwd, trace = ctx.last_kernel_names()
            assert "k_align8_fwd_x2" in fwd and "k_align8_trace_codes2" in trace, (name, fwd, trace)


@pytest.mark.parametrize("bw", [64, 128])
def test_row_record_kernels(ctx, monkeypatch, bw):
    """the row-record kernels (BSA_ALIGN8_LITERAL=1: packed two-pairs-per-row where it applies; with BSA_ALIGN8_I32=1 the int32
    kernel): every matrix, all-positive, all-negative and beyond every guard included"""
    pairs = _pairs(6900 + bw, 28, bw)
    monkeypatch.setenv("BSA_ALIGN8_LITERAL", "1")
    for name in ALL:
        m, gaps = MS.CATALOGUE[name]
        for mode in MODES:
            _check(ctx, pairs, mode, bw, m, gaps)
            assert "row records" in _fwd(ctx) and "gen" not in _fwd(ctx), (name, _fwd(ctx))
    monkeypatch.setenv("BSA_ALIGN8_I32", "1")
    for name in ALL:
        m, gaps = MS.CATALOGUE[name]
        _check(ctx, pairs, S.MODE_GLOBAL, bw, m, gaps)
        assert "row records" in _fwd(ctx) and "gen" not in _fwd(ctx), (name, _fwd(ctx))


@pytest.mark.parametrize("bw", [16, 32, 512])
def test_other_register_widths(ctx, bw):
    """bandwidths 16, 32, 512 (row records): the asymmetric matrix and every matrix beyond the guard"""
    pairs = _pairs(7000 + bw, 28, bw)
    for name in ["asym"] + MS.BEYOND_GUARD:
        m, gaps = MS.CATALOGUE[name]
        for mode in (S.MODE_GLOBAL, S.MODE_OVERLAP):
            _check(ctx, pairs, mode, bw, m, gaps)
            assert "row records" in _fwd(ctx) and "gen" not in _fwd(ctx), (name, _fwd(ctx))


@pytest.mark.parametrize("bw", [48, 80, 1024])
def test_run_time_width_kernel(ctx, monkeypatch, bw):
    """k_align8_fwd_gen (bandwidths the register kernels do not have): every matrix.  The host entry sends the pairs whose query fits
    the band to the widened compact path as a sub-batch of their own, so the kernel is asserted on the pairs with longer queries, and
    on the whole corpus with BSA_ALIGN8_WIDEN=0"""
    pairs = _pairs(7100 + bw, 24, bw)
    rng = np.random.default_rng(7150 + bw)
    t = rng.integers(0, 4, size=bw + 200).astype(np.uint8)
    pairs.append((S.mutate(rng, t, 0.05), t))
    longer = [(q, t) for q, t in pairs if len(q) > bw]
    assert len(longer) >= 4
    modes = MODES if bw < 1024 else (S.MODE_GLOBAL, S.MODE_EXTEND)
    for name in ALL:
        m, gaps = MS.CATALOGUE[name]
        for mode in modes:
            _check(ctx, longer, mode, bw, m, gaps)
            assert "k_align8_fwd_gen" in _fwd(ctx), (name, _fwd(ctx))
            if bw < 1024:
                _check(ctx, pairs, mode, bw, m, gaps)           # (mixed: some pairs on the widened compact path)
    monkeypatch.setenv("BSA_ALIGN8_WIDEN", "0")
    for name in ALL:
        m, gaps = MS.CATALOGUE[name]
        _check(ctx, pairs, S.MODE_GLOBAL, bw, m, gaps)
        assert "k_align8_fwd_gen" in _fwd(ctx), (name, _fwd(ctx))


def test_whole_query_bands_widened_on_the_compact_path(ctx):
    """bandwidth 0 with every query <= 256 bases: the band runs widened at a register-kernel width on the exact-arithmetic kernel,
    in-guard matrices, all three modes; matrices beyond the guard keep the run-time-width kernel"""
    pairs = [(q[:256], t) for q, t in _pairs(7200, 60, 256, lens=[1, 15, 16, 17, 63, 64, 65, 100, 200, 255, 256, 300])]
    for name in MS.IN_GUARD_GENERAL:
        for mode in MODES:
            _check(ctx, pairs, mode, 0, MS.GENERAL[name], MS.AFFINE)
            assert _fwd(ctx).startswith("k_align8_fwd_x"), (name, _fwd(ctx))
    for name in ("allpos", "allneg", "m2n_129"):
        m, gaps = MS.CATALOGUE[name]
        _check(ctx, pairs, S.MODE_GLOBAL, 0, m, gaps)
        assert "k_align8_fwd_gen" in _fwd(ctx), (name, _fwd(ctx))


def _sys_pairs(bw):
    rng = np.random.default_rng(7300 + bw)
    top = bw if bw else 3000
    lens = [l for l in (257, 300, 320, 511, 700, 1008, 1500, 3000) if l <= top]
    pairs = [(q[:top] if len(q) > top else q, t) for q, t in MS.mk_pairs(rng, 14, 0, lens=lens, ratios=(1.0, 1.0, 0.9, 1.1))]
    pairs = [(q, t) for q, t in pairs if len(q) > 256 or bw]
    pairs.append((pairs[0][0], pairs[0][1][:1]))            # a one-row target
    pairs.append((pairs[1][0], pairs[1][1][:65]))
    return pairs


def _sys_expect(name):
    """the kernel a whole-query band above 256 columns runs: the systolic kernel inside the static guard, its checked form outside
    it where the checked form's bounds hold, the run-time-width kernel beyond"""
    m, gaps = MS.CATALOGUE[name]
    if MS.static_guard(m, gaps):
        return "k_align8_fwd_sys ("
    return "k_align8_fwd_sys<CHK>" if MS.checked_sys_guard(m, gaps) else "k_align8_fwd_gen"


@pytest.mark.parametrize("bw", [0, 1008])
def test_systolic_wavefront(ctx, monkeypatch, bw):
    """k_align8_fwd_sys / k_align8_fwd_sys<CHK> (whole-query bands above 256 columns): in-guard matrices in all three modes, every
    guard boundary on both sides (which kernel runs is part of the check), and the checked form forced inside the guard"""
    pairs = _sys_pairs(bw)
    for name in MS.IN_GUARD_GENERAL:
        for mode in MODES:
            _check(ctx, pairs, mode, bw, MS.GENERAL[name], MS.AFFINE)
            assert "k_align8_fwd_sys (" in _fwd(ctx), (name, _fwd(ctx))
    for name in list(MS.BOUNDARY) + ["allpos", "allneg"]:
        m, gaps = MS.CATALOGUE[name]
        _check(ctx, pairs, S.MODE_GLOBAL, bw, m, gaps)
        assert _sys_expect(name) in _fwd(ctx), (name, _fwd(ctx))
    monkeypatch.setenv("BSA_ALIGN8_SYS_CHK", "1")
    for name in ("asym", "posmis", "m3g_64", "m2n_128"):
        m, gaps = MS.CATALOGUE[name]
        _check(ctx, pairs, S.MODE_GLOBAL, bw, m, gaps)
        assert "k_align8_fwd_sys<CHK>" in _fwd(ctx), (name, _fwd(ctx))
    _check(ctx, pairs, S.MODE_EXTEND, bw, MS.GENERAL["asym"], MS.AFFINE)
    assert "k_align8_fwd_sys<CHK>" in _fwd(ctx)


@pytest.mark.parametrize("wave", ["1", "0"])
def test_traceback_walkers(ctx, monkeypatch, wave):
    """the code-row walkers at bandwidth 128, global: one walk per wave and one per lane"""
    monkeypatch.setenv("BSA_ALIGN8_TRACE_WAVE", wave)
    pairs = _pairs(7400, 60, 128, eps_list=(0.0, 0.05, 0.2, 0.4))
    for name in ("asym", "posmis"):
        for gaps in (MS.AFFINE, (-4, -2, 0, 0)):
            _check(ctx, pairs, S.MODE_GLOBAL, 128, MS.GENERAL[name], gaps)
            fwd, trace = ctx.last_kernel_names()
            assert fwd.startswith("k_align8_fwd_x"), fwd
            if wave == "1":
                assert trace == "k_align8_trace_codes_wave", trace
            else:
                assert trace.startswith("k_align8_trace_codes") and "wave" not in trace, trace


def test_handover_to_the_literal_kernels(ctx, monkeypatch):
    """bsa_align_batch re-runs undecided pairs through the row-record kernels (BSA_DEBUG_HANDOVER=7 declares every 7th pair undecided)
    and splices the answers back: the re-run gets the same matrix"""
    monkeypatch.setenv("BSA_DEBUG_HANDOVER", "7")
    pairs = _pairs(7500, 50, 128)
    _check(ctx, pairs, S.MODE_GLOBAL, 128, MS.GENERAL["asym"], MS.AFFINE)
    assert _fwd(ctx).startswith("k_align8_fwd_x") and ctx.last_handover() >= len(pairs) // 7, (_fwd(ctx), ctx.last_handover())


def test_plan_on_device_pointers_at_a_reduced_headline_shape(ctx, monkeypatch):
    """the two-phase API on device-resident synthetic pairs (bsa_synth_pairs_dev): 4 096 pairs x 10 kbp, bandwidth 128, global, the
    asymmetric matrix, the row-segment kernel (BSA_ALIGN8_XQ=1: at this size the dispatch would take whole pairs).  No pair is flagged;
    256 pairs spread over the batch, the first and the last equal the oracle word for word"""
    import torch
    import bsalign_amd as B
    monkeypatch.setenv("BSA_ALIGN8_XQ", "1")
    n, L = 4096, 10000
    m = MS.GENERAL["asym"]
    dev = torch.device("cuda", 0)
    lib = B.lib()
    stride = lib.bsa_synth_stride(L)
    d_seqs = torch.empty(2 * n * stride, dtype=torch.uint8, device=dev)
    d_qlen = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.bsa_synth_pairs_dev(ctx.h, S.SEED, 0, n, L, int(0.10 * 4294967296.0), C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_qlen.data_ptr())) == 0
    ctx.sync()
    qlen = d_qlen.cpu().numpy().astype(np.uint32)
    tlen = np.full(n, L, dtype=np.uint32)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    qoff = (np.arange(n, dtype=np.uint64) + np.uint64(n)) * np.uint64(stride)
    plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(S.MODE_GLOBAL, 128, 0, 0, *MS.AFFINE, matrix=m))
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.empty(n * (L // 4), dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    plan.run(d_seqs, d_out, d_cig, d_off, d_st)
    ctx.sync()
    assert "k_align8_fwd_xq" in _fwd(ctx), _fwd(ctx)
    out = d_out.cpu().numpy().reshape(n, 10)
    off = d_off.cpu().numpy()
    st = d_st.cpu().numpy()
    cig = d_cig.cpu().numpy().view(np.uint32)
    plan.close()
    assert not st.any(), "%d flagged pairs" % int((st != 0).sum())
    sample = sorted(set(np.linspace(0, n - 1, 256).astype(int).tolist()) | {0, n - 1})
    for k in sample:
        q, t = S.synth_pair(k, L)
        assert len(q) == qlen[k]
        res, ocig, _ = S.oracle_align(q, t, S.MODE_GLOBAL, 128, 0, 0, *MS.AFFINE, mtx=m)
        assert np.array_equal(out[k], res) and np.array_equal(cig[int(off[k]):int(off[k + 1])], ocig), (k, out[k], res)
