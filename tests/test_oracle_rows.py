"""CPU: the oracle's row-level functions (row_init / row_movx incl. jumps >= W / row_cal with the POA's
homopolymer-bonus profiles / row_merge / row_max / band_mov) against the real reference, when it is built here, and
against its recorded rows (tests/golden/rows_sat.npz) where it is not.
These are the functions the POA seq->graph DP drives directly (bspoa.h:2232-2272)."""
import ctypes as C

import numpy as np
import pytest

import rows_sat_cases as RS
import support as S

needs_ref = pytest.mark.skipif(not S.have_ref(), reason="reference build (oracle/_ref) not present")

i8p, i32p, u8p = S.i8p, S.i32p, S.u8p


def _al(n, dt):
    """16-byte aligned numpy array (the reference uses aligned SSE loads)"""
    raw = np.zeros(n * np.dtype(dt).itemsize + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dt).itemsize].view(dt)


def _libs():
    o, r = S.oracle(), S.ref()
    o.orc_row_movx.restype = None
    o.orc_row_cal.restype = C.c_int
    o.orc_row_merge.restype = None
    o.orc_row_max.restype = C.c_uint32
    o.orc_getscore.restype = C.c_int
    o.orc_band_mov.restype = C.c_int
    r.ref_row_movx.restype = None
    r.ref_row_cal.restype = C.c_int
    r.ref_row_merge.restype = None
    r.ref_row_max.restype = C.c_uint32
    r.ref_band_mov.restype = C.c_int
    r.ref_qprof_size.restype = C.c_uint64
    return o, r


class Query(C.Structure):
    _fields_ = [("seq", u8p), ("len", C.c_uint32), ("mtx", i8p), ("hpc", C.c_int), ("bonus", C.c_int)]


def _row(rng, bw, pw, mode, gaps, lib_ref, W):
    """a plausible row: run the reference's row_init, then a few row_cal steps on a random query"""
    us, es, qs, ub = _al(bw, np.int8), _al(bw, np.int8), _al(bw, np.int8), _al(20, np.int32)
    lib_ref.ref_row_init(S.ptr(us, i8p), S.ptr(es, i8p), S.ptr(qs, i8p), S.ptr(ub, i32p), mode, bw, 3, -6, *gaps)
    return us, es, qs, ub


@needs_ref
@pytest.mark.parametrize("gaps", [(-3, -2, 0, 0), (0, -3, 0, 0), (-3, -2, -8, -1)])
@pytest.mark.parametrize("bw", [16, 64, 128])
def test_row_functions_match_reference(gaps, bw):
    o, r = _libs()
    rng = np.random.default_rng(bw + abs(gaps[0]) * 7 + abs(gaps[2]))
    W = bw // 16
    pw = o.orc_get_piecewise(*gaps, bw)
    qlen = 400
    q = rng.integers(0, 4, size=qlen).astype(np.uint8)
    mtxs = [S.score_matrix(2, -6), S.score_matrix(3, -6)]
    for trial in range(60):
        mode = int(rng.choice([0, 1]))
        use_hpc = int(rng.integers(2))
        mtx = mtxs[int(rng.integers(2))]
        # reference profile for this (matrix, hpc) choice (bspoa.h:2199-2215)
        qprof = _al(int(r.ref_qprof_size(qlen, bw)) + 64, np.int8)
        if use_hpc:
            r.ref_set_query_prof_hpc(S.ptr(q, u8p), qlen, S.ptr(qprof, i8p), bw, S.ptr(mtx, i8p), 1)
        else:
            r.ref_set_query_prof(S.ptr(q, u8p), qlen, S.ptr(qprof, i8p), bw, S.ptr(mtx, i8p))
        qy = Query(S.ptr(q, u8p), qlen, S.ptr(mtx, i8p), use_hpc, 1)
        us, es, qs, ub = _row(rng, bw, pw, mode, gaps, r, W)
        rbeg = 0
        for step in range(12):
            movx = int(rng.choice([0, 1, 1, 2, 3, W, W + 1, 2 * W + 3, bw - 1, bw, bw + 5])) if step else 0
            if rbeg + movx + bw > qlen:      # the reference only guarantees profile rows up to qlen (bsalign.h:2147)
                movx = 0
            base = int(rng.integers(4))
            # ---- movx: reference vs oracle
            ru, re, rq, rb = _al(bw, np.int8), _al(bw, np.int8), _al(bw, np.int8), _al(20, np.int32)
            ou, oe, oq, ob = _al(bw, np.int8), _al(bw, np.int8), _al(bw, np.int8), _al(20, np.int32)
            r.ref_row_movx(S.ptr(ru, i8p), S.ptr(re, i8p), S.ptr(rq, i8p), S.ptr(rb, i32p), S.ptr(us, i8p), S.ptr(es, i8p), S.ptr(qs, i8p), S.ptr(ub, i32p),
                           W, movx, pw, 3, -6, *gaps)
            o.orc_row_movx(S.ptr(ou, i8p), S.ptr(oe, i8p), S.ptr(oq, i8p), S.ptr(ob, i32p), S.ptr(us, i8p), S.ptr(es, i8p), S.ptr(qs, i8p), S.ptr(ub, i32p),
                           W, movx, pw, 3, -6, *gaps)
            assert np.array_equal(ru, ou) and np.array_equal(rb[:17], ob[:17]), ("movx u/ubegs", gaps, bw, movx, step)
            if pw >= 1:
                assert np.array_equal(re, oe), ("movx e", movx)
            if pw == 2:
                assert np.array_equal(rq, oq), ("movx q", movx)
            rbeg += movx
            # ---- row_cal on the moved row (rh as dpalign_row_update_bspoa computes it, bspoa.h:2243-2255)
            if movx == 0:
                rh = -(0x7FFFFFFF >> 2) if rbeg else (0 if (mode == 1 or step == 0) else gaps[0] + gaps[1] * step)
            elif movx <= bw:
                rh = int(rb[0])
            else:
                rh = -(0x7FFFFFFF >> 2)
            r2u, r2e, r2q, r2b = _al(bw, np.int8), _al(bw, np.int8), _al(bw, np.int8), _al(20, np.int32)
            o2u, o2e, o2q, o2b = _al(bw, np.int8), _al(bw, np.int8), _al(bw, np.int8), _al(20, np.int32)
            r.ref_row_cal(rbeg, base, S.ptr(ru, i8p), S.ptr(re, i8p), S.ptr(rq, i8p), S.ptr(rb, i32p),
                          S.ptr(r2u, i8p), S.ptr(r2e, i8p), S.ptr(r2q, i8p), S.ptr(r2b, i32p), S.ptr(qprof, i8p), *gaps, W, movx, rh, pw)
            o.orc_row_cal(rbeg, base, S.ptr(ou, i8p), S.ptr(oe, i8p), S.ptr(oq, i8p), S.ptr(ob, i32p),
                          S.ptr(o2u, i8p), S.ptr(o2e, i8p), S.ptr(o2q, i8p), S.ptr(o2b, i32p), C.byref(qy), *gaps, W, rh, pw)
            assert np.array_equal(r2u, o2u) and np.array_equal(r2b[:17], o2b[:17]), ("row_cal u/ubegs", gaps, bw, movx, step, use_hpc)
            if pw >= 1:
                assert np.array_equal(r2e, o2e)
            if pw == 2:
                assert np.array_equal(r2q, o2q)
            # ---- row_max / band_mov on the new row
            ms_r, ms_o = C.c_int32(), C.c_int32()
            xr = r.ref_row_max(S.ptr(r2u, i8p), S.ptr(r2b, i32p), W, C.byref(ms_r))
            xo = o.orc_row_max(S.ptr(o2u, i8p), S.ptr(o2b, i32p), W, C.byref(ms_o))
            assert (xr, ms_r.value) == (xo, ms_o.value)
            assert r.ref_band_mov(S.ptr(r2u, i8p), S.ptr(r2b, i32p), W, 50 + step, rbeg, qlen) == o.orc_band_mov(S.ptr(o2b, i32p), W, 50 + step, rbeg, qlen)
            # ---- row_merge of the moved row and the new row (two progenitors of one graph node, bspoa.h:2263-2272)
            m_r = [_al(bw, np.int8) for _ in range(3)] + [_al(20, np.int32)]
            m_o = [_al(bw, np.int8) for _ in range(3)] + [_al(20, np.int32)]
            r.ref_row_merge(S.ptr(ru, i8p), S.ptr(re, i8p), S.ptr(rq, i8p), S.ptr(rb, i32p), S.ptr(r2u, i8p), S.ptr(r2e, i8p), S.ptr(r2q, i8p), S.ptr(r2b, i32p),
                            S.ptr(m_r[0], i8p), S.ptr(m_r[1], i8p), S.ptr(m_r[2], i8p), S.ptr(m_r[3], i32p), W, pw)
            o.orc_row_merge(S.ptr(ou, i8p), S.ptr(oe, i8p), S.ptr(oq, i8p), S.ptr(ob, i32p), S.ptr(o2u, i8p), S.ptr(o2e, i8p), S.ptr(o2q, i8p), S.ptr(o2b, i32p),
                            S.ptr(m_o[0], i8p), S.ptr(m_o[1], i8p), S.ptr(m_o[2], i8p), S.ptr(m_o[3], i32p), W, pw)
            assert np.array_equal(m_r[0], m_o[0]) and np.array_equal(m_r[3][:17], m_o[3][:17]), ("merge", gaps, bw, step)
            if pw >= 1:
                assert np.array_equal(m_r[1], m_o[1])
            if pw == 2:
                assert np.array_equal(m_r[2], m_o[2])
            us, es, qs, ub = r2u, r2e, r2q, r2b


# ---- outside the exactness guard of the POA graph kernels: the scorings of tests/rows_sat_cases.py ------------------------------------
_STEP = ("row_movx", "row_cal", "row_merge", "row_max")


def _compare_chain(c, got, want, side):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        what = "row_init" if k == 0 else "%s of step %d" % (_STEP[(k - 1) % 4], (k - 1) // 4)
        assert np.array_equal(a, b), "%s: %s differs from the %s (%s, bandwidth %d, mode %d, chain %d, first byte %d)" % (
            RS.OracleRows.name, what, side, c["name"], c["bw"], c["mode"], c["chain"], int(np.nonzero(a != b)[0][0]))


def test_saturating_sets_are_outside_the_guard_and_clamp():
    """Every set of rows_sat_cases.SETS is refused by the guard's inequalities (restated there; the GPU tests ask the library itself), at every
    bandwidth it is used at, with the piecewise form it is named for.  And the inputs are not vacuous: of the rows the oracle makes by UPDATE
    tasks, at least 10 % hold a us byte of 127 or -128 -- in the chains test_rows_gpu.py sends, in the sweep programs test_poa_sweep_gpu.py
    sends (of which a third must end with rpos + bw == slen) and among the reference's recorded rows -- under wrapping, two_piece_big,
    linear_clamp and affine_clamp, at every bandwidth and mode: one set per piecewise form, and one whose head cell wraps.
    big_affine and linear_big do not reach that share with any reads and bases, and what they do reach is asserted instead
    (rows_sat_cases.check_share): linear_big never clamps, with every us in [-30, 47]; big_affine never clamps up to 128 columns and, from 176
    columns on, only in the lane-start cells that the f crossing a whole lane decides (0.2 ... 2 % of the rows; 1.0 % of the chains' and
    1.6 / 2.0 % of the sweep programs' at 256 / 512 columns in global mode).  linear_clamp and affine_clamp are their siblings (piecewise 0
    and 1) with scores large enough to clamp throughout."""
    for name in RS.SETS:
        for bw in RS.bandwidths(name):
            RS.assert_outside_guard(name, bw)
    assert sorted(RS.PIECEWISE[n] for n in RS.SHARE_SETS) == [0, 1, 1, 2]
    for name in RS.SAT_SETS:
        for bw in RS.BANDWIDTHS:
            for mode in RS.MODES:
                ch = RS.chains(name, bw, mode)
                assert ch["nupd"] == 24 * 20
                RS.check_share(name, bw, mode, ch["share"])
                if name == "linear_big":
                    us = np.concatenate([b[:bw].view(np.int8) for _, exp in ch["levels"][1:-1] for _, b in exp])
                    assert -30 <= us.min() and us.max() <= 47, (bw, mode, us.min(), us.max())
        for bw in RS.SWEEP_BANDWIDTHS:
            for mode in RS.MODES:
                sb = RS.sweep_batch(name, bw, mode)
                RS.check_share(name, bw, mode, sb["share"])
                assert sb["ends"] >= 8, (name, bw, mode, sb["ends"])
                if name == "big_affine":          # the clamped bytes are lane-start cells: vector 0
                    us = sb["orows"].reshape(sb["nblocks"], sb["blk"])[:, 16:bw].view(np.int8)
                    assert not ((us == 127) | (us == -128)).any(), (bw, mode)
    recs = RS.load_fixture()[0]
    for name in RS.SAT_SETS:
        new = [(c["bw"], RS.clamped(RS.unpack(rows[2 + 4 * st], c["bw"], RS.piecewise(c["sc"], c["bw"]))))
               for c, rows in recs if c["name"] == name for st in range(len(c["steps"]))]
        if name in RS.SHARE_SETS:
            assert np.mean([x for _, x in new]) >= RS.MIN_SHARE, name
        else:            # (the recorded chains are few: none of big_affine's at 256 columns meets a clamped lane start)
            assert not any(x for bw, x in new if name == "linear_big" or bw <= 128), name


def test_oracle_rows_match_the_recorded_reference():
    """tests/golden/rows_sat.npz (the reference's own rows: every set and the default scoring x bandwidth 16 ... 256 x global / overlap /
    extend, inputs included) replayed through the oracle, every call on the RECORDED input, byte for byte; runs without the reference build"""
    recs, mp, merge = RS.load_fixture()
    assert len(recs) >= 200
    R = RS.OracleRows()
    for c, want in recs:
        _compare_chain(c, RS.run_fixture_chain(R, c, feed=want), want, "recorded reference")
    pw = RS.piecewise(mp["sc"], RS.MERGE_BW)
    got = RS.run_program(R, mp, RS.MERGE_BW)
    assert sorted(merge) == [5, 8, 9]
    for k, want in merge.items():
        assert np.array_equal(RS.pack(got[k], RS.MERGE_BW, pw), want), "8192-column program: block %d differs from the recorded reference" % k
    # without the re-basing after 256 vectors a lane of either input leaves int16: that is what this program is there for
    W = RS.MERGE_BW // 16
    for k in (5, 8):
        lane = RS.unpack(merge[k], RS.MERGE_BW, pw)[0].reshape(W, 16).astype(np.int64).sum(axis=0)
        assert lane.min() < -32768, (k, lane.min())
    # row_merge where its int16 sums saturate: the merged es are the reference's, and they are not what exact sums give
    n = RS.S16_BW
    for k, (a, b, want) in enumerate(RS.load_s16_cases()):
        got = RS.pack(R.merge(RS.unpack(a, n, 1), RS.unpack(b, n, 1), n // 16, 1), n, 1)
        assert np.array_equal(got, want), "int16 merge case %d differs from the recorded reference (first byte %d)" % (k, int(np.nonzero(got != want)[0][0]))
        assert (RS.merge_without_int16(a, b) != want[n:2 * n].view(np.int8)).sum() >= 5, k


@needs_ref
def test_oracle_rows_match_the_live_reference_outside_the_guard():
    """the same chains, each side running on its own rows, and the 8192-column merge program (W = 512: the re-basing every 256 vectors of
    row_merge, bsalign.h:2496), oracle against the reference as it is built here; and the fixture is what the reference gives today"""
    R, O = RS.RefRows(), RS.OracleRows()
    recs, mp, merge = RS.load_fixture()
    for c, rec in recs:
        want = RS.run_fixture_chain(R, c)
        _compare_chain(c, RS.run_fixture_chain(O, c), want, "reference")
        assert all(np.array_equal(a, b) for a, b in zip(rec, want)), "tests/golden/rows_sat.npz is stale (%s)" % c["name"]
    pw = RS.piecewise(mp["sc"], RS.MERGE_BW)
    assert pw == 1
    a, b = RS.run_program(O, mp, RS.MERGE_BW), RS.run_program(R, mp, RS.MERGE_BW)
    for k in sorted(b):
        assert np.array_equal(RS.pack(a[k], RS.MERGE_BW, pw), RS.pack(b[k], RS.MERGE_BW, pw)), "8192-column program: block %d" % k
    n = RS.S16_BW
    for k, ((a, b), (fa, fb, want)) in enumerate(zip(RS.draw_merge_s16_cases(), RS.load_s16_cases())):
        assert np.array_equal(a, fa) and np.array_equal(b, fb), "tests/golden/rows_sat.npz is stale (int16 merge case %d)" % k
        ref = RS.pack(R.merge(RS.unpack(a, n, 1), RS.unpack(b, n, 1), n // 16, 1), n, 1)
        assert np.array_equal(ref, want), "tests/golden/rows_sat.npz is stale (int16 merge case %d)" % k
        assert np.array_equal(RS.pack(O.merge(RS.unpack(a, n, 1), RS.unpack(b, n, 1), n // 16, 1), n, 1), ref), "int16 merge case %d" % k
