"""BSA_MODE_SCORE_ONLY on the edit aligner, on the MI355X: score, qe, te and status as the full path returns them (and as the oracle computes
them), the fields only a traceback finds set to -1, no CIGAR.  Global and extend mode run the SCORE forward kernels and k_edit_score_finish;
overlap mode runs the full path and drops the walk's fields."""
import os

import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.gpu

TRACE_FIELDS = ("qb", "tb", "mat", "mis", "ins", "del", "aln")
END_FIELDS = ("score", "qe", "te")


def _mk(rng, L, eps, ratio):
    T = rng.integers(0, 4, size=L).astype(np.uint8)
    Q = S.mutate(rng, T, eps)
    if ratio != 1.0:
        Lq = max(1, int(len(Q) * ratio))
        Q = Q[:Lq] if Lq <= len(Q) else np.concatenate([Q, rng.integers(0, 4, size=Lq - len(Q)).astype(np.uint8)])
    if len(Q) == 0:
        Q = np.array([0], dtype=np.uint8)
    return Q, T


def _pairs(rng, n, lens):
    return [_mk(rng, int(rng.choice(lens)), float(rng.choice([0.01, 0.05, 0.1, 0.2])), float(rng.choice([1.0, 0.9, 1.1]))) for _ in range(n)]


def _compare(ctx, pairs, mode, bw, fast=True, sample=12, seed=0):
    """score-only against the full call on the same pairs, and a sample against the oracle: returns the forward kernel's name"""
    full, _, fst = ctx.edit_batch(pairs, mode, bw)
    so, sst = ctx.edit_scores(pairs, mode, bw)
    fwd, fin = ctx.last_kernel_names()
    if fast:
        assert "score-only" in fwd and fin == "k_edit_score_finish", (fwd, fin)
    else:
        assert "score-only" not in fwd and fin != "k_edit_score_finish", (fwd, fin)
    for f in TRACE_FIELDS:
        assert (so[f] == -1).all(), f
    assert np.array_equal(sst, fst)
    for f in END_FIELDS:
        bad = np.nonzero(so[f] != full[f])[0]
        assert bad.size == 0, "%s differs for %d pairs, first %d: %s vs %s" % (f, bad.size, bad[0], so[bad[0]], full[bad[0]])
    rng = np.random.default_rng(seed)
    for k in rng.choice(len(pairs), size=min(sample, len(pairs)), replace=False):
        q, t = pairs[k]
        if sst[k] != 0:
            continue
        res, _, n = S.oracle_edit(q, t, mode, bw)
        assert n >= 0
        assert (int(so[k]["score"]), int(so[k]["qe"]), int(so[k]["te"])) == (int(res[0]), int(res[2]), int(res[4])), (k, len(q), len(t), so[k], res)
    return fwd


@pytest.mark.parametrize("bw", [64, 128, 256, 512, 1024, 0])
def test_global(ctx, bw):
    """banded pairs and short queries (qlen < bandwidth: the band is the whole rounded query) in one batch"""
    rng = np.random.default_rng(5100 + bw)
    pairs = _pairs(rng, 72, [300, 700, 1500, 3000]) + _pairs(rng, 40, [1, 2, 30, 63, 64, 65, 100, 129, 200, 500])
    _compare(ctx, pairs, S.MODE_GLOBAL, bw, seed=bw)


def test_extend_on_whole_read_bands(ctx, monkeypatch):
    """bandwidth 0, extend mode: reads above 1024 bases are the wide class, the short reads of a small batch move to the same kernel"""
    rng = np.random.default_rng(5200)
    for lens in ([5, 64, 100, 300, 800], [1100, 1500, 2500, 4000]):
        pairs = _pairs(rng, 48, lens)
        fwd = _compare(ctx, pairs, S.MODE_EXTEND, 0, seed=lens[0])
        assert "k_edit_fwd_wide" in fwd, fwd
    # no moving: the short reads stay on the register kernels (TRACK forms)
    pairs = _pairs(rng, 48, [5, 64, 100, 300, 800])
    monkeypatch.setenv("BSA_EDIT_NO_MERGE", "1")
    fwd = _compare(ctx, pairs, S.MODE_EXTEND, 0, seed=1)
    assert "k_edit_fwd_wide" not in fwd, fwd


@pytest.mark.parametrize("env,kernel", [({"BSA_EDIT_GRP32": "1"}, "k_edit_fwd_grp32 "), ({"BSA_EDIT_GRP": "1"}, "k_edit_fwd_grp "),
                                        ({"BSA_EDIT_GRP": "0"}, "k_edit_fwd "), ({"BSA_EDIT_GRP": "0", "BSA_EDIT_FWD_LANES": "16"}, "k_edit_fwd ")],
                         ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) if isinstance(e, dict) else e.strip())
def test_forced_kernel_forms(ctx, monkeypatch, env, kernel):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BSA_EDIT_NO_MERGE", "1")          # (extend mode: the short static bands stay on the register kernels)
    rng = np.random.default_rng(5300 + len(env))
    for mode, bw, lens in ((S.MODE_GLOBAL, 128, [400, 1500]), (S.MODE_GLOBAL, 256, [700, 2000]), (S.MODE_GLOBAL, 512, [900, 3000]),
                           (S.MODE_EXTEND, 0, [150, 250])):
        pairs = [p for p in _pairs(rng, 40, lens) if len(p[0]) > bw]
        fwd = _compare(ctx, pairs, mode, bw, sample=6, seed=bw + mode)
        assert fwd.startswith(kernel), (env, mode, bw, fwd)


def test_mixed_classes_with_the_generic_kernel(ctx):
    """global, bandwidth 2048: queries longer than 2048 move the band (k_edit_fwd_gen, two rows in turn -- odd and even targets), the
    others have whole-query bands of every class; and one extend-mode band above 32768 columns, which only the generic kernel takes"""
    rng = np.random.default_rng(5400)
    pairs = []
    for L in (2201, 2600, 3001, 3500, 4000, 4001):
        pairs.append(_mk(rng, L, 0.1, float(rng.choice([1.0, 1.1]))))
    pairs += _pairs(rng, 30, [60, 300, 900, 1500])
    assert any(len(q) > 2048 and len(t) % 2 == 1 for q, t in pairs) and any(len(q) > 2048 and len(t) % 2 == 0 for q, t in pairs)
    fwd = _compare(ctx, pairs, S.MODE_GLOBAL, 2048, sample=40, seed=5)
    assert "k_edit_fwd_gen" in fwd, fwd
    T = rng.integers(0, 4, size=9837).astype(np.uint8)
    Q = rng.integers(0, 4, size=32790).astype(np.uint8)
    M = S.mutate(rng, T, 0.08)[:9837]                  # related over the common prefix
    Q[:len(M)] = M
    _compare(ctx, [(Q, T), _mk(rng, 500, 0.1, 1.0)], S.MODE_EXTEND, 0, sample=2, seed=6)


@pytest.mark.parametrize("bw", [0, 256])
def test_overlap_runs_the_full_path(ctx, bw):
    rng = np.random.default_rng(5500 + bw)
    pairs = _pairs(rng, 48, [5, 64, 300, 800, 1500])
    _compare(ctx, pairs, S.MODE_OVERLAP, bw, fast=False)


@pytest.mark.parametrize("name", ["edit.npz", "edit_wide.npz"])
def test_golden_cases(ctx, name):
    """the reference's recorded results, under the flag"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    groups = {}
    for k in range(int(g["n"][0])):
        mode, bw = [int(x) for x in g["meta_%d" % k]]
        groups.setdefault((mode, bw), []).append(k)
    for (mode, bw), ks in groups.items():
        so, sst = ctx.edit_scores([(g["q_%d" % k], g["t_%d" % k]) for k in ks], mode, bw)
        fwd, fin = ctx.last_kernel_names()
        assert ("score-only" in fwd) == (mode != S.MODE_OVERLAP), (mode, fwd)
        for i, k in enumerate(ks):
            res = g["res_%d" % k]
            assert sst[i] == 0 and (int(so[i]["score"]), int(so[i]["qe"]), int(so[i]["te"])) == (int(res[0]), int(res[2]), int(res[4])), (name, mode, bw, k)
            assert all(int(so[i][f]) == -1 for f in TRACE_FIELDS)


@pytest.mark.parametrize("mode,bw", [(S.MODE_GLOBAL, 256), (S.MODE_EXTEND, 0), (S.MODE_GLOBAL, 0), (S.MODE_OVERLAP, 0)])
def test_flagged_pairs_next_to_normal_ones(ctx, mode, bw):
    import bsalign_amd as B
    rng = np.random.default_rng(5600 + mode + bw)
    pairs = _pairs(rng, 24, [300, 900, 1500, 2600])
    bad = pairs[5][0].copy()
    bad[len(bad) // 2] = 9
    pairs[5] = (bad, pairs[5][1])
    pairs[6] = (np.zeros(0, np.uint8), pairs[6][1])
    pairs[7] = (pairs[7][0], np.zeros(0, np.uint8))
    _compare(ctx, pairs, mode, bw, fast=mode != S.MODE_OVERLAP, sample=24)
    so, sst = ctx.edit_scores(pairs, mode, bw)
    assert sst[5] & B.ST_BAD_BASE and sst[6] & B.ST_EMPTY and sst[7] & B.ST_EMPTY
    assert all(int(so[k]["score"]) == 0 and int(so[k]["qe"]) == 0 and int(so[k]["te"]) == 0 for k in (5, 6, 7))


def test_benchmark_shape_100k_bw256(ctx):
    """C3's per-pair shape"""
    pairs = [S.synth_pair(k, 100000) for k in range(4)]
    fwd = _compare(ctx, pairs, S.MODE_GLOBAL, 256, sample=4)
    assert "k_edit_fwd_grp32" in fwd, fwd


def test_device_pointer_plan(ctx):
    import torch
    import bsalign_amd as B
    dev = torch.device("cuda:0")
    q = np.array([0, 1, 2, 3] * 30, dtype=np.uint8)
    bad = q.copy()
    bad[7] = 4
    rng = np.random.default_rng(5700)
    pairs = [(q, q), (bad, q), (np.zeros(0, np.uint8), q), (q, np.zeros(0, np.uint8))] + _pairs(rng, 60, [100, 500, 1200, 2500])
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    n = len(pairs)
    d_seqs = torch.from_numpy(seqs).to(dev)
    for mode, bw in ((S.MODE_GLOBAL, 128), (S.MODE_GLOBAL, 0), (S.MODE_EXTEND, 0), (S.MODE_OVERLAP, 0)):
        full, _, fst = ctx.edit_batch(pairs, mode, bw)
        plan = B.EditPlan(ctx, qoff, qlen, toff, tlen, mode | B.MODE_SCORE_ONLY, bw)
        d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
        d_off = torch.full((n + 1,), 7, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        plan.run(d_seqs, d_out, None, d_off, d_st)
        ctx.sync()
        plan.close()
        assert ("score-only" in ctx.last_kernel_names()[0]) == (mode != S.MODE_OVERLAP)
        out = d_out.cpu().numpy().view(B.RESULT_DTYPE).reshape(n)
        st = d_st.cpu().numpy().view(np.uint32)
        assert (d_off.cpu().numpy() == 0).all()
        assert np.array_equal(st, fst)
        assert st[1] & B.ST_BAD_BASE and st[2] & B.ST_EMPTY and st[3] & B.ST_EMPTY
        for f in END_FIELDS:
            assert np.array_equal(out[f], full[f]), (mode, bw, f)
        for f in TRACE_FIELDS:
            assert (out[f] == -1).all(), f


def test_workspace_of_a_single_launch():
    """a workspace limit that cuts the full plan of 4096 x 20 kbp (bandwidth 256) into several forward launches: the score-only plan (a
    256-byte record a pair) takes the batch in one"""
    import bsalign_amd as B
    pairs = B.synth_pairs_host(4096, 20000)
    small = B.Context(0, workspace_limit=256 << 20)
    try:
        full, _, fst = small.edit_batch(pairs, S.MODE_GLOBAL, 256)
        _, full_launches, _ = small.last_kernel_ms()
        so, sst = small.edit_scores(pairs, S.MODE_GLOBAL, 256)
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
