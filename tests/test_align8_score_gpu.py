"""BSA_MODE_SCORE_ONLY on the MI355X: score, qe, te and status as the full path returns them (and as the oracle computes them), the
fields only a traceback finds set to -1, no CIGAR -- on the SCORE forward kernels where they exist and on the full path everywhere else."""
import ctypes as C

import numpy as np
import pytest

import matrix_support as MS
import support as S

pytestmark = pytest.mark.gpu

SCORINGS = {
    "affine": (2, -6, -3, -2, 0, 0),
    "linear": (2, -6, 0, -3, 0, 0),
    "twopiece": (2, -6, -3, -2, -8, -1),
}
TRACE_FIELDS = ("qb", "tb", "mat", "mis", "ins", "del", "aln")
END_FIELDS = ("score", "qe", "te")
LENS = [1, 15, 16, 17, 63, 64, 65, 300, 1000, 2000]
MODES = [S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND]


def _pairs(rng, n, lens=LENS):
    """related pairs of the given lengths (queries a little shorter or longer) and unrelated pairs whose lengths differ by a factor
    that makes the band jump (tlen << qlen) or crawl (qlen << tlen)"""
    pairs = []
    for k in range(n):
        if k % 4 == 3:
            lt = int(rng.integers(20, 400))
            lq = max(1, int(lt * float(rng.choice([2.0, 3.0, 5.0, 0.5, 0.3]))))
            pairs.append((rng.integers(0, 4, size=lq).astype(np.uint8), rng.integers(0, 4, size=lt).astype(np.uint8)))
            continue
        L = int(rng.choice(lens))
        t = rng.integers(0, 4, size=L).astype(np.uint8)
        q = S.mutate(rng, t, float(rng.choice([0.01, 0.1, 0.2])))
        r = float(rng.choice([1.0, 0.9, 1.1]))
        lq = max(1, int(len(q) * r))
        q = q[:lq] if lq <= len(q) else np.concatenate([q, rng.integers(0, 4, size=lq - len(q)).astype(np.uint8)])
        pairs.append((q if len(q) else t[:1].copy(), t))
    return pairs


def _params(mode, bw, sc=None, m=None, gaps=MS.AFFINE):
    import bsalign_amd as B
    if m is not None:
        return B.make_params(mode, bw, 0, 0, *gaps, matrix=m)
    return B.make_params(mode, bw, *sc)


def _compare(ctx, pairs, par, fast, oracle=None):
    """score-only against the full call on the same pairs (and, with oracle = (sc, mtx), against the oracle): returns the forward kernel's name"""
    import bsalign_amd as B
    full, _, fst = ctx.align_batch(pairs, par)
    so, sst = ctx.align_scores(pairs, par)
    fwd, fin = ctx.last_kernel_names()
    if fast:
        assert "score-only" in fwd and fin == "k_align8_score_finish", (fwd, fin)
    else:
        assert "score-only" not in fwd and fin != "k_align8_score_finish", (fwd, fin)
    for f in TRACE_FIELDS:
        assert (so[f] == -1).all(), f
    # a pair on which the reference's own traceback does not terminate is flagged by the full path only (no traceback runs here)
    walk_flag = ((fst & B.ST_TRACE) != 0) & ((sst & B.ST_TRACE) == 0)
    keep = ~walk_flag
    for f in END_FIELDS:
        bad = np.nonzero((so[f] != full[f]) & keep)[0]
        assert bad.size == 0, "%s differs for %d pairs, first %d: %s vs %s" % (f, bad.size, bad[0], so[bad[0]], full[bad[0]])
    assert np.array_equal(sst[keep], fst[keep])
    if oracle is not None:
        sc, m = oracle
        mode, bw = par.mode & 3, par.bandwidth
        for k, (q, t) in enumerate(pairs):
            res, _, n = S.oracle_align(q, t, mode, bw, *sc, mtx=m)
            if n == S.ORC_ERR_TRACE:
                continue
            got = (int(so[k]["score"]), int(so[k]["qe"]), int(so[k]["te"]))
            assert sst[k] == 0 and got == (int(res[0]), int(res[2]), int(res[4])), (k, len(q), len(t), got, res)
    return fwd


@pytest.mark.parametrize("scname", ["affine", "linear"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bw", [64, 128, 256])
def test_score_only_on_the_fast_shapes(ctx, bw, mode, scname):
    rng = np.random.default_rng(9100 + bw + 10 * mode + len(scname))
    pairs = _pairs(rng, 48)
    _compare(ctx, pairs, _params(mode, bw, SCORINGS[scname]), True, (SCORINGS[scname], None))


@pytest.mark.parametrize("name", ["asym", "transition", "zero_diag"])
@pytest.mark.parametrize("mode", MODES)
def test_score_only_with_general_matrices(ctx, name, mode):
    assert name in MS.IN_GUARD_GENERAL
    m = MS.GENERAL[name]
    rng = np.random.default_rng(9200 + mode + len(name))
    pairs = _pairs(rng, 40)
    _compare(ctx, pairs, _params(mode, 128, m=m), True, ((0, 0) + MS.AFFINE, m))


@pytest.mark.parametrize("xq", ["0", "1"])
def test_row_segments_and_whole_pairs(ctx, monkeypatch, xq):
    """BSA_ALIGN8_XQ=1 forces the row-segment form (k_align8_fwd_xq) on any batch, 0 keeps whole pairs"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    rng = np.random.default_rng(9300 + int(xq))
    pairs = _pairs(rng, 40, [1, 63, 64, 65, 127, 128, 129, 700])
    for bw in (64, 128, 256):
        for mode in MODES:
            fwd = _compare(ctx, pairs, _params(mode, bw, SCORINGS["affine"]), True, (SCORINGS["affine"], None))
            assert ("k_align8_fwd_xq" in fwd) == (xq == "1"), fwd


@pytest.mark.parametrize("mode", MODES)
def test_whole_query_bands_in_place(ctx, mode):
    """bandwidth 0 and queries of at most 256 bases: the static kernel at the widened width (overlap / extend take row_max over the
    reference's own band)"""
    rng = np.random.default_rng(9400 + mode)
    for lo, hi in ((20, 64), (100, 128), (200, 256)):
        pairs = []
        for _ in range(24):
            lq = int(rng.integers(lo, hi + 1))
            t = rng.integers(0, 4, size=int(rng.integers(10, 600))).astype(np.uint8)
            q = S.mutate(rng, t, 0.1)[:lq] if rng.random() < 0.5 else rng.integers(0, 4, size=lq).astype(np.uint8)
            pairs.append((q if len(q) else t[:1].copy(), t))
        fwd = _compare(ctx, pairs, _params(mode, 0, SCORINGS["affine"]), True, (SCORINGS["affine"], None))
        assert "k_align8_fwd_x_static" in fwd, fwd


@pytest.mark.parametrize("case", ["twopiece_128", "bw512", "bw1024", "bw48", "beyond_guard", "systolic"])
def test_fallbacks_keep_the_contract(ctx, case):
    """configurations without SCORE kernels run the full path: same score / end cell / status, the -1 fields, no CIGAR"""
    rng = np.random.default_rng(9500 + len(case))
    mode = S.MODE_OVERLAP if case in ("bw48", "systolic") else S.MODE_GLOBAL
    if case == "twopiece_128":
        par = _params(mode, 128, SCORINGS["twopiece"])
    elif case.startswith("bw"):
        par = _params(mode, int(case[2:]), SCORINGS["affine"])
    elif case == "beyond_guard":
        m, gaps = MS.CATALOGUE["nmg_101"]
        assert "nmg_101" in MS.BEYOND_GUARD
        par = _params(mode, 128, m=m, gaps=gaps)
    else:
        par = _params(mode, 0, SCORINGS["affine"])
    lens = [1000, 1500, 2000] if case == "systolic" else [16, 300, 1000, 2000]
    # (queries longer than the band: a host-pointer batch at bandwidth 48 would send whole-query pairs down the widened fast path)
    pairs = [p for p in _pairs(rng, 40, lens) if len(p[0]) > (256 if case == "systolic" else 64)]
    fwd = _compare(ctx, pairs, par, False)
    if case == "systolic":
        assert "k_align8_fwd_sys" in fwd, fwd


def test_host_pointer_batch_in_two_slices(ctx, monkeypatch):
    """the flag travels to both slices of a sliced host-pointer batch"""
    monkeypatch.setenv("BSA_BATCH_SLICES", "2")
    rng = np.random.default_rng(9550)
    pairs = _pairs(rng, 200, [40, 300, 900, 1500])
    _compare(ctx, pairs, _params(S.MODE_GLOBAL, 128, SCORINGS["affine"]), True)


def test_device_pointer_plan(ctx):
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    q = np.array([0, 1, 2, 3] * 30, dtype=np.uint8)
    bad = q.copy()
    bad[7] = 4
    rng = np.random.default_rng(9600)
    pairs = [(q, q), (bad, q), (np.zeros(0, np.uint8), q), (q, np.zeros(0, np.uint8))] + _pairs(rng, 60, [100, 500, 1200])
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    n = len(pairs)
    d_seqs = torch.from_numpy(seqs).to(dev)
    for mode in MODES:
        par = _params(mode, 128, SCORINGS["affine"])
        full, _, fst = ctx.align_batch(pairs, par)
        sp = B.AlignParams.from_buffer_copy(par)
        sp.mode |= B.MODE_SCORE_ONLY
        plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, sp)
        d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
        d_off = torch.full((n + 1,), 7, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        plan.run(d_seqs, d_out, None, d_off, d_st)
        ctx.sync()
        plan.close()
        assert "score-only" in ctx.last_kernel_names()[0]
        out = d_out.cpu().numpy().view(B.RESULT_DTYPE).reshape(n)
        st = d_st.cpu().numpy().view(np.uint32)
        assert (d_off.cpu().numpy() == 0).all()
        assert np.array_equal(st, fst)
        assert st[1] & B.ST_BAD_BASE and st[2] & B.ST_EMPTY and st[3] & B.ST_EMPTY
        for f in END_FIELDS:
            assert np.array_equal(out[f], full[f]), f
        for f in TRACE_FIELDS:
            assert (out[f] == -1).all(), f
    # the two flags exclude each other, in both entry points
    both = B.AlignParams.from_buffer_copy(_params(S.MODE_GLOBAL, 128, SCORINGS["affine"]))
    both.mode |= B.MODE_SCORE_ONLY | B.MODE_ROWRECORDS
    with pytest.raises(B.BsaError) as e:
        B.AlignPlan(ctx, qoff, qlen, toff, tlen, both)
    assert e.value.code == -2
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    rc = B.lib().bsa_align_batch(ctx.h, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(both),
                                 B._p(out), None, 0, None, None)
    assert rc == -2


def test_workspace_of_a_single_launch():
    """a workspace limit that cuts the full plan of 4096 x 5 kbp into several forward launches: the score-only plan (a 256-byte record a
    pair) takes the batch in one"""
    import bsalign_amd as B
    pairs = B.synth_pairs_host(4096, 5000)
    par = _params(S.MODE_GLOBAL, 128, SCORINGS["affine"])
    small = B.Context(0, workspace_limit=256 << 20)
    try:
        full, _, fst = small.align_batch(pairs, par)
        _, full_launches, _ = small.last_kernel_ms()
        so, sst = small.align_scores(pairs, par)
        _, so_launches, _ = small.last_kernel_ms()
        assert "score-only" in small.last_kernel_names()[0]
    finally:
        small.close()
    assert full_launches >= 4 and so_launches == 1, (full_launches, so_launches)
    assert (fst == 0).all() and np.array_equal(sst, fst)
    for f in END_FIELDS:
        assert np.array_equal(so[f], full[f]), f
    for f in TRACE_FIELDS:
        assert (so[f] == -1).all(), f


@pytest.mark.parametrize("mode", [S.MODE_GLOBAL, S.MODE_OVERLAP])
def test_mid_size_batch(ctx, mode):
    import bsalign_amd as B
    pairs = B.synth_pairs_host(20000, 2000, seed=777 + mode)
    _compare(ctx, pairs, _params(mode, 128, SCORINGS["affine"]), True)
