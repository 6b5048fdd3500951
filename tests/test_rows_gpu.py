"""GPU parity: the POA row kernels (bsa_rows_run: row_init / row_movx + row_cal with the 4 POA profiles / row_merge)
against the oracle's row functions (which tests/test_oracle_rows.py pins against the real reference)."""
import ctypes as C

import numpy as np
import pytest
import torch

import poa_support as P
import rows_sat_cases as RS
import support as S

pytestmark = pytest.mark.gpu
i8p, i32p, u8p = S.i8p, S.i32p, S.u8p


class Query(C.Structure):
    _fields_ = [("seq", u8p), ("len", C.c_uint32), ("mtx", i8p), ("hpc", C.c_int), ("bonus", C.c_int)]


def _views(block, bw, pw):
    us = block[:bw].view(np.int8)
    es = block[bw:2 * bw].view(np.int8) if pw >= 1 else np.zeros(bw, np.int8)
    qs = block[2 * bw:3 * bw].view(np.int8) if pw == 2 else np.zeros(bw, np.int8)
    ub = block[(pw + 1) * bw:(pw + 1) * bw + 68].view(np.int32)
    return us, es, qs, ub


@pytest.mark.parametrize("gaps", [(-3, -2, 0, 0), (0, -3, 0, 0), (-3, -2, -8, -1)])
@pytest.mark.parametrize("bw", [16, 64, 128, 256])
def test_row_tasks_match_oracle(ctx, gaps, bw):
    import bsalign_amd as B
    lib, o = B.lib(), S.oracle()
    o.orc_row_cal.restype = C.c_int
    rng = np.random.default_rng(bw * 3 + abs(gaps[2]) + abs(gaps[0]))
    W = bw // 16
    pw = o.orc_get_piecewise(*gaps, bw)
    M, X, RB, mode = 2, -6, 1, S.MODE_OVERLAP
    blk = lib.bsa_rows_block_bytes(bw, *gaps)
    nq, qlen_max = 6, 700
    queries = [rng.integers(0, 4, size=int(rng.integers(bw + 40, qlen_max))).astype(np.uint8) for _ in range(nq)]
    qoff = np.zeros(nq, dtype=np.uint64)
    qlen = np.array([len(q) for q in queries], dtype=np.uint32)
    acc = 0
    for k, q in enumerate(queries):
        qoff[k] = acc
        acc += len(q) + 8
    qblob = np.zeros(acc, dtype=np.uint8)
    for k, q in enumerate(queries):
        qblob[int(qoff[k]):int(qoff[k]) + len(q)] = q
    nchain, depth = 24, 14           # independent chains of row updates, one level per launch
    nrows = nchain * (depth + 2)
    rows = np.zeros(nrows * blk, dtype=np.uint8)          # host mirror maintained with the oracle
    d_rows = torch.zeros(nrows * blk, dtype=torch.uint8, device="cuda:0")
    d_q = torch.from_numpy(qblob).cuda()
    d_qoff = torch.from_numpy(qoff.view(np.int64)).cuda()
    d_qlen = torch.from_numpy(qlen.view(np.int32)).cuda()
    par = B.RowsParams(mode, bw, M, X, RB, *gaps)
    mtxs = [S.score_matrix(M, X), S.score_matrix(M + RB, X)]

    def run(tasks):
        t = np.array(tasks, dtype=B.ROW_TASK_DTYPE)
        d_t = torch.from_numpy(t.view(np.uint8)).cuda()
        rc = lib.bsa_rows_run(ctx.h, C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_t.data_ptr()), len(t), C.c_void_p(d_q.data_ptr()),
                              C.c_void_p(d_qoff.data_ptr()), C.c_void_p(d_qlen.data_ptr()), C.byref(par))
        assert rc == 0
        ctx.sync()
        torch.cuda.synchronize()

    def blockv(idx):
        return rows[idx * blk:(idx + 1) * blk]

    # level 0: init every chain's first row (device) and with the oracle (host)
    tasks = []
    for c in range(nchain):
        dst = c * (depth + 2)
        tasks.append((B.lib() and 2, 0, dst, 0, 0, 0, c % nq, 0, 0, 0))
        us, es, qs, ub = _views(blockv(dst), bw, pw)
        ubt = np.zeros(17, dtype=np.int32)
        uu, ee, qq = np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(bw, np.int8)
        o.orc_row_init(S.ptr(uu, i8p), S.ptr(ee, i8p), S.ptr(qq, i8p), S.ptr(ubt, i32p), mode, bw, M + RB + 1, X, *gaps)
        us[:] = uu
        if pw >= 1:
            es[:] = ee
        if pw == 2:
            qs[:] = qq
        ub[:] = ubt
    run(tasks)
    state = [(0, c % nq) for c in range(nchain)]       # (band offset, query) per chain
    for lev in range(depth):
        tasks, expect = [], []
        for c in range(nchain):
            src = c * (depth + 2) + lev
            dst = src + 1
            qoff_src, qi = state[c]
            ql = int(qlen[qi])
            movx = int(rng.choice([0, 1, 1, 2, 3, W, W + 1, 2 * W + 1, bw - 1, bw, bw + 3]))
            if qoff_src + movx + bw > ql:
                movx = 0
            qoff_dst = qoff_src + movx
            base, prof = int(rng.integers(4)), int(rng.integers(4))
            tasks.append((0, src, dst, qoff_src, qoff_dst, lev + 1, qi, base, prof, 0))
            # oracle: movx then row_cal with the profile's matrix / hpc flag
            us, es, qs, ub = _views(blockv(src), bw, pw)
            mu, me, mq, mb = np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(17, np.int32)
            o.orc_row_movx(S.ptr(mu, i8p), S.ptr(me, i8p), S.ptr(mq, i8p), S.ptr(mb, i32p),
                           S.ptr(np.ascontiguousarray(us), i8p), S.ptr(np.ascontiguousarray(es), i8p), S.ptr(np.ascontiguousarray(qs), i8p), S.ptr(np.ascontiguousarray(ub), i32p),
                           W, movx, pw, M + RB + 1, X, *gaps)
            if movx == 0:
                rh = -(0x7FFFFFFF >> 2) if qoff_src else (0 if mode == S.MODE_OVERLAP else gaps[0] + gaps[1] * (lev + 1))
            elif movx <= bw:
                rh = int(mb[0])
            else:
                rh = -(0x7FFFFFFF >> 2)
            q = queries[qi]
            mtx = mtxs[prof & 1]
            qy = Query(S.ptr(q, u8p), len(q), S.ptr(mtx, i8p), 0 if (prof & 2) else 1, 1)
            nu, ne, nqv, nb = np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(17, np.int32)
            o.orc_row_cal(qoff_dst, base, S.ptr(mu, i8p), S.ptr(me, i8p), S.ptr(mq, i8p), S.ptr(mb, i32p),
                          S.ptr(nu, i8p), S.ptr(ne, i8p), S.ptr(nqv, i8p), S.ptr(nb, i32p), C.byref(qy), *gaps, W, rh, pw)
            dus, des, dqs, dub = _views(blockv(dst), bw, pw)
            dus[:] = nu
            if pw >= 1:
                des[:] = ne
            if pw == 2:
                dqs[:] = nqv
            dub[:] = nb
            state[c] = (qoff_dst, qi)
        run(tasks)
        got = d_rows.cpu().numpy()
        for c in range(nchain):
            dst = c * (depth + 2) + lev + 1
            used = (pw + 1) * bw + 68
            assert np.array_equal(got[dst * blk:dst * blk + used], rows[dst * blk:dst * blk + used]), ("update", gaps, bw, lev, c, tasks[c])
    # merges: rows[dst] = max(rows[src], rows[dst]) for pairs of chains
    tasks = []
    for c in range(0, nchain - 1, 2):
        src = c * (depth + 2) + depth
        dst = (c + 1) * (depth + 2) + depth
        tasks.append((1, src, dst, 0, 0, 0, 0, 0, 0, 0))
        a0 = [np.ascontiguousarray(x) for x in _views(blockv(src), bw, pw)]
        a1 = [np.ascontiguousarray(x) for x in _views(blockv(dst), bw, pw)]
        mu, me, mq, mb = np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(bw, np.int8), np.zeros(17, np.int32)
        o.orc_row_merge(S.ptr(a0[0], i8p), S.ptr(a0[1], i8p), S.ptr(a0[2], i8p), S.ptr(a0[3], i32p),
                        S.ptr(a1[0], i8p), S.ptr(a1[1], i8p), S.ptr(a1[2], i8p), S.ptr(a1[3], i32p),
                        S.ptr(mu, i8p), S.ptr(me, i8p), S.ptr(mq, i8p), S.ptr(mb, i32p), W, pw)
        dus, des, dqs, dub = _views(blockv(dst), bw, pw)
        dus[:] = mu
        if pw >= 1:
            des[:] = me
        if pw == 2:
            dqs[:] = mq
        dub[:] = mb
    run(tasks)
    got = d_rows.cpu().numpy()
    for c in range(0, nchain - 1, 2):
        dst = (c + 1) * (depth + 2) + depth
        used = (pw + 1) * bw + 68
        assert np.array_equal(got[dst * blk:dst * blk + used], rows[dst * blk:dst * blk + used]), ("merge", gaps, bw, c)


# ---- outside the exactness guard of the POA graph kernels (tests/rows_sat_cases.py) ---------------------------------------------------
def _run_rows(ctx, d_rows, tasks, d_q, d_qoff, d_qlen, par):
    import bsalign_amd as B
    t = np.array(tasks, dtype=B.ROW_TASK_DTYPE)
    d_t = torch.from_numpy(t.view(np.uint8)).cuda()
    rc = B.lib().bsa_rows_run(ctx.h, C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_t.data_ptr()), len(t), C.c_void_p(d_q.data_ptr()),
                              C.c_void_p(d_qoff.data_ptr()), C.c_void_p(d_qlen.data_ptr()), C.byref(par))
    assert rc == 0
    ctx.sync()
    torch.cuda.synchronize()


def _chains_on_the_device(ctx, name, bw, mode):
    """rows_sat_cases.chains (24 chains x 20 levels, then merges of chain pairs; left-boundary rh with both gap pieces for piecewise 2, as
    bspoa.h:2243-2255) level by level through bsa_rows_run: every used byte of every destination block after each level"""
    import bsalign_amd as B
    ch = RS.chains(name, bw, mode)
    sc, blk, used = ch["sc"], ch["blk"], RS.used_bytes(bw, ch["pw"])
    assert B.lib().bsa_rows_block_bytes(bw, *RS.gaps(sc)) == blk
    d_rows = torch.zeros(ch["nrows"] * blk, dtype=torch.uint8, device="cuda:0")
    d_q = torch.from_numpy(ch["qblob"]).cuda()
    d_qoff = torch.from_numpy(ch["qoff"].view(np.int64)).cuda()
    d_qlen = torch.from_numpy(ch["qlen"].view(np.int32)).cuda()
    par = B.RowsParams(mode, bw, sc["M"], sc["X"], sc["refbonus"], *RS.gaps(sc))
    for lev, (tasks, exp) in enumerate(ch["levels"]):
        _run_rows(ctx, d_rows, tasks, d_q, d_qoff, d_qlen, par)
        got = d_rows.cpu().numpy()
        for tk, (dst, want) in zip(tasks, exp):
            assert np.array_equal(got[dst * blk:dst * blk + used], want), (name, bw, mode, "level", lev, tk)
    return ch


@pytest.mark.parametrize("mode", RS.MODES)
@pytest.mark.parametrize("name,bw", [(n, bw) for n in RS.SETS for bw in RS.bandwidths(n)])
def test_row_tasks_match_oracle_outside_the_guard(ctx, name, bw, mode):
    """the saturating, lane-exact arithmetic of rows_update / rows_merge / rows_task_gen where it does clamp and wrap: the sets of
    rows_sat_cases.SETS, each refused by bsa_poa_graph_supported (and, but for the two wide_ext sets, by bsa_poa_graph_gen_supported)"""
    import bsalign_amd as B
    RS.assert_outside_guard(name, bw, B.lib(), bw + 700)
    ch = _chains_on_the_device(ctx, name, bw, mode)
    RS.check_share(name, bw, mode, ch["share"])


@pytest.mark.parametrize("mode", RS.MODES)
@pytest.mark.parametrize("bw", RS.BANDWIDTHS)
def test_row_tasks_match_oracle_default_scoring_every_mode(ctx, bw, mode):
    """test_row_tasks_match_oracle's scoring family (the POA's defaults) at bandwidth 32 as well, and in global and extend mode"""
    _chains_on_the_device(ctx, "default", bw, mode)


def test_recorded_reference_rows_replayed(ctx):
    """tests/golden/rows_sat.npz through bsa_rows_run: every recorded step as one UPDATE task on the reference's own previous row (its result
    against the reference's row after row_cal) and one MERGE task on the reference's moved and new row -- the device against the reference
    directly, without the oracle in between"""
    import bsalign_amd as B
    recs = RS.load_fixture()[0]
    groups = {}
    for c, rows in recs:
        groups.setdefault((c["name"], c["bw"], c["mode"]), []).append((c, rows))
    for (name, bw, mode), chains in groups.items():
        sc = chains[0][0]["sc"]
        pw = RS.piecewise(sc, bw)
        blk, used = P.block_bytes(bw, pw), RS.used_bytes(bw, pw)
        host, upd, mrg, want = [], [], [], {}
        qlen = np.array([len(c["query"]) for c, _ in chains], np.uint32)
        qoff = np.zeros(len(chains), np.uint64)
        qoff[1:] = np.cumsum(qlen + 8)[:-1]
        qblob = np.zeros(int(qoff[-1]) + int(qlen[-1]) + 8, np.uint8)

        def put(b):
            host.append(np.concatenate([b, np.zeros(blk - used, np.uint8)]))
            return len(host) - 1

        for qi, (c, rows) in enumerate(chains):
            qblob[int(qoff[qi]):int(qoff[qi]) + len(c["query"])] = c["query"]
            rbeg = 0
            for st, (movx, base, prof, _) in enumerate(c["steps"]):
                src = put(rows[0] if st == 0 else rows[2 + 4 * (st - 1)])
                dst = put(np.zeros(used, np.uint8))
                upd.append((0, src, dst, rbeg, rbeg + movx, st, qi, base, prof, 0))
                want[dst] = rows[2 + 4 * st]
                rbeg += movx
                a, b = put(rows[1 + 4 * st]), put(rows[2 + 4 * st])
                mrg.append((1, a, b, 0, 0, 0, 0, 0, 0, 0))
                want[b] = rows[3 + 4 * st]
        d_rows = torch.from_numpy(np.concatenate(host)).cuda()
        d_q = torch.from_numpy(qblob).cuda()
        d_qoff = torch.from_numpy(qoff.view(np.int64)).cuda()
        d_qlen = torch.from_numpy(qlen.view(np.int32)).cuda()
        par = B.RowsParams(mode, bw, sc["M"], sc["X"], sc["refbonus"], *RS.gaps(sc))
        _run_rows(ctx, d_rows, upd + mrg, d_q, d_qoff, d_qlen, par)
        got = d_rows.cpu().numpy()
        for dst, w in want.items():
            assert np.array_equal(got[dst * blk:dst * blk + used], w), (name, bw, mode, "block", dst, (upd + mrg)[[t[2] for t in upd + mrg].index(dst)])


def test_merge_where_int16_saturates(ctx):
    """rows_sat_cases.draw_merge_s16_cases as recorded in tests/golden/rows_sat.npz: one MERGE task per pair at 4096 columns (W = 256, the
    run-time-width form), where the int16 sums of row_merge reach -32768 -- the device against the reference's merged row directly"""
    import bsalign_amd as B
    cases = RS.load_s16_cases()
    bw, sc = RS.S16_BW, RS.MERGE_SC
    assert RS.piecewise(sc, bw) == 1
    blk, used = P.block_bytes(bw, 1), RS.used_bytes(bw, 1)
    assert B.lib().bsa_rows_block_bytes(bw, *RS.gaps(sc)) == blk and cases[0][0].shape == (used,)
    host = np.zeros((2 * len(cases), blk), np.uint8)
    for k, (a, b, _) in enumerate(cases):
        host[2 * k, :used], host[2 * k + 1, :used] = a, b
    d_rows = torch.from_numpy(host.reshape(-1)).cuda()
    d_q = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    d_qoff = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_qlen = torch.full((1,), 64, dtype=torch.int32, device="cuda:0")
    par = B.RowsParams(sc["alnmode"], bw, sc["M"], sc["X"], sc["refbonus"], *RS.gaps(sc))
    _run_rows(ctx, d_rows, [(1, 2 * k, 2 * k + 1, 0, 0, 0, 0, 0, 0, 0) for k in range(len(cases))], d_q, d_qoff, d_qlen, par)
    got = d_rows.cpu().numpy().reshape(-1, blk)
    for k, (a, _, want) in enumerate(cases):
        assert np.array_equal(got[2 * k, :used], a), ("source block", k)
        assert np.array_equal(got[2 * k + 1, :used], want), ("merged block", k, int(np.nonzero(got[2 * k + 1, :used] != want)[0][0]))
