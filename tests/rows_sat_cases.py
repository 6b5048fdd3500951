"""POA scorings OUTSIDE the exactness guard of bsa_poa_graph_supported / bsa_poa_graph_gen_supported, where the reference's int8 operations clamp
(_mm_adds_epi8 ...: sat8), wrap (an int stored into a byte: trunc8) or saturate to int16 (row_merge), and the seeded inputs that
test_oracle_rows.py (oracle against the real reference, live and from tests/golden/rows_sat.npz), test_rows_gpu.py and test_poa_sweep_gpu.py
(bsa_rows_run / bsa_sweep_host against the oracle and against the recorded reference) send through them.  What the CPU file vets here -- every
set is refused by the guard, and the oracle's rows really clamp -- is exactly what the GPU files send."""
import ctypes as C
import functools
import os
import zlib

import numpy as np

import poa_support as P
import support as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "rows_sat.npz")
i8p, i32p, u8p = S.i8p, S.i32p, S.u8p
SCORE_MIN = -(0x7FFFFFFF >> 2)

# (M, X, refbonus, O, E, Q, P, T); "clause": the inequality of the guard (bsa_poa_wf.hip, bsa_poa_graph_supported) the set is there to break
SETS = {
    # every derived constant (gapo + gape, the head cell, the synthetic cell behind a moved row) still fits int8
    "big_affine": dict(M=20, X=-40, refbonus=1, O=-30, E=-10, Q=0, P=0, T=20, clause="m+3g"),
    # the head cell gapo1 + gape1 + X - (M + refbonus + 1) = -172 leaves int8: the reference's byte store wraps (trunc8, not sat8)
    "wrapping": dict(M=30, X=-60, refbonus=1, O=-60, E=-20, Q=0, P=0, T=20, clause="head_cell"),
    "linear_big": dict(M=15, X=-45, refbonus=1, O=0, E=-30, Q=0, P=0, T=20, clause="m+3g"),            # piecewise 0
    "two_piece_big": dict(M=10, X=-30, refbonus=2, O=-20, E=-8, Q=-60, P=-2, T=20, clause="synthetic_cell"),
    # siblings of linear_big and big_affine (same piecewise forms 0 and 1) whose rows clamp throughout.  Under those two the difference between
    # neighbouring cells of a lane stays below 127; only big_affine's lane-start cells clamp, from 176 columns on (check_share)
    "linear_clamp": dict(M=60, X=-100, refbonus=1, O=0, E=-100, Q=0, P=0, T=20, clause="m+3g"),
    "affine_clamp": dict(M=100, X=-120, refbonus=1, O=-40, E=-10, Q=0, P=0, T=20, clause="m+3g"),
    # default scoring with a long extension at 256 columns: (bw / 16) * ge > 60, and W * gape1 = -144 below int8
    "wide_ext_e4": dict(M=2, X=-6, refbonus=1, O=-3, E=-4, Q=-8, P=-1, T=20, clause="width"),
    "wide_ext_e9": dict(M=2, X=-6, refbonus=1, O=-3, E=-9, Q=-8, P=-1, T=20, clause="width"),
}
DEFAULT = dict(M=2, X=-6, refbonus=1, O=-3, E=-2, Q=-8, P=-1, T=20)
BANDWIDTHS = (16, 32, 64, 128, 256)
MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)
SAT_SETS = ("big_affine", "wrapping", "linear_big", "two_piece_big", "linear_clamp", "affine_clamp")
SHARE_SETS = ("wrapping", "two_piece_big", "linear_clamp", "affine_clamp")          # at least MIN_SHARE of their rows clamp; check_share says what holds for the other two
WIDE_SETS = ("wide_ext_e4", "wide_ext_e9")                                   # 256 columns only: the width is what leaves the guard
PIECEWISE = {"big_affine": 1, "wrapping": 1, "linear_big": 0, "two_piece_big": 2, "linear_clamp": 0, "affine_clamp": 1, "wide_ext_e4": 2, "wide_ext_e9": 1}
MIN_SHARE = 0.10


def _seed(name):
    return zlib.crc32(name.encode())          # (not the set's place in SETS: a new set leaves the inputs of the others alone)


def bandwidths(name):
    return (256,) if name in WIDE_SETS else BANDWIDTHS


def gaps(sc):
    return (sc["O"], sc["E"], sc["Q"], sc["P"])


def piecewise(sc, bw):
    return int(S.oracle().orc_get_piecewise(*gaps(sc), bw))


def guard_clauses(sc, bw):
    """the inequalities of bsa_poa_graph_supported restated: -> names of the violated clauses.  "width" is the one clause that
    bsa_poa_graph_gen_supported (the generic-width kernel) does not have."""
    pw = piecewise(sc, bw)
    m, n, ge, go = sc["M"] + sc["refbonus"] + 1, -sc["X"], -sc["E"], -sc["O"]
    assert min(m, n, ge, go, sc["M"], sc["refbonus"]) >= 0
    g = go + ge
    if pw == 2:
        assert -sc["P"] >= 0 and -sc["Q"] >= 0 and sc["E"] <= sc["P"]
        g = max(g, -sc["Q"] - sc["P"])
    bad = []
    if m + 3 * g > 64:
        bad.append("m+3g")
    if n + m + g > 100:
        bad.append("n+m+g")
    if m + 2 * n > 128:
        bad.append("m+2n")
    if min(sc["X"], -g) - 1 - m - g < -100:
        bad.append("synthetic_cell")
    if go + ge + m + n + (ge if pw == 0 else 63) > 128:
        bad.append("seed_byte")
    if 2 * m + n + go + ge > 126:
        bad.append("seed_delta")
    if (bw // 16) * ge > 60:
        bad.append("width")
    if not -128 <= sc["O"] + sc["E"] + sc["X"] - m <= 127:
        bad.append("head_cell")          # no clause of its own in the library: every such set breaks m+3g long before
    return bad


def assert_outside_guard(name, bw, lib=None, slen=None):
    """CPU: through the restated inequalities.  With lib (B.lib(), the GPU tests): through the library's own two functions.  The two wide_ext
    sets leave only bsa_poa_graph_supported (k_poa_wf): the generic-width kernel has no width clause and takes them."""
    sc = SETS[name]
    bad = guard_clauses(sc, bw)
    assert sc["clause"] in bad, (name, bw, bad)
    assert all(-127 <= sc[k] <= 127 for k in "MXOEQP") and sc["M"] + sc["refbonus"] + 1 <= 127
    assert piecewise(sc, bw) == PIECEWISE[name], (name, bw)
    if name in WIDE_SETS:
        assert bad == ["width"], (name, bad)
    if lib is not None:
        import bsalign_amd as B
        sp = B.SweepParams()
        sp.rows = B.RowsParams(S.MODE_OVERLAP, bw, sc["M"], sc["X"], sc["refbonus"], *gaps(sc))
        sp.T = sc["T"]
        lib.bsa_poa_graph_supported.restype = C.c_int
        lib.bsa_poa_graph_gen_supported.restype = C.c_int
        assert lib.bsa_poa_graph_supported(C.byref(sp), int(slen or bw + 50)) == 0, (name, bw)
        if name not in WIDE_SETS:
            assert lib.bsa_poa_graph_gen_supported(C.byref(sp)) == 0, (name, bw)


# ---- the row functions of one side (the oracle, or the real reference when it is built) behind one face ------------------------------
def _al(n, dt):
    """16-byte aligned numpy array (the reference uses aligned SSE loads)"""
    raw = np.zeros(n * np.dtype(dt).itemsize + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dt).itemsize].view(dt)


def new_row(bw):
    return _al(bw, np.int8), _al(bw, np.int8), _al(bw, np.int8), _al(20, np.int32)


def row_ptrs(r):
    return S.ptr(r[0], i8p), S.ptr(r[1], i8p), S.ptr(r[2], i8p), S.ptr(r[3], i32p)


class Query(C.Structure):
    _fields_ = [("seq", u8p), ("len", C.c_uint32), ("mtx", i8p), ("hpc", C.c_int), ("bonus", C.c_int)]


def prof_matrix(sc, prof):
    """the four POA profiles (bspoa.h:2199-2215): bit 0 the refbonus matrix, bit 1 clear the homopolymer bonus 1"""
    return S.score_matrix(sc["M"] + (sc["refbonus"] if prof & 1 else 0), sc["X"]), 0 if prof & 2 else 1


class OracleRows:
    name = "oracle"

    def __init__(self):
        o = self.o = S.oracle()
        o.orc_row_movx.restype = None
        o.orc_row_cal.restype = C.c_int
        o.orc_row_merge.restype = None
        o.orc_row_max.restype = C.c_uint32

    def init(self, sc, bw, mode):
        r = new_row(bw)
        self.o.orc_row_init(*row_ptrs(r), mode, bw, sc["M"] + sc["refbonus"] + 1, sc["X"], *gaps(sc))
        return r

    def movx(self, src, W, movx, pw, sc):
        r = new_row(W * 16)
        self.o.orc_row_movx(*row_ptrs(r), *row_ptrs(src), W, movx, pw, sc["M"] + sc["refbonus"] + 1, sc["X"], *gaps(sc))
        return r

    def cal(self, moved, q, rbeg, base, prof, sc, W, movx, rh, pw):
        r = new_row(W * 16)
        mtx, hpc = prof_matrix(sc, prof)
        qy = Query(S.ptr(q, u8p), len(q), S.ptr(mtx, i8p), hpc, 1)
        self.o.orc_row_cal(rbeg, base, *row_ptrs(moved), *row_ptrs(r), C.byref(qy), *gaps(sc), W, rh, pw)
        return r

    def merge(self, a, b, W, pw):
        r = new_row(W * 16)
        self.o.orc_row_merge(*row_ptrs(a), *row_ptrs(b), *row_ptrs(r), W, pw)
        return r

    def rowmax(self, r, W):
        ms = C.c_int32()
        x = self.o.orc_row_max(S.ptr(r[0], i8p), S.ptr(r[3], i32p), W, C.byref(ms))
        return int(x), ms.value


class RefRows:
    """oracle/_ref/libbsref.so's ref_row_* (the reference's own functions, unchanged)"""
    name = "reference"

    def __init__(self):
        r = self.r = S.ref()
        r.ref_row_movx.restype = None
        r.ref_row_cal.restype = C.c_int
        r.ref_row_merge.restype = None
        r.ref_row_max.restype = C.c_uint32
        r.ref_qprof_size.restype = C.c_uint64
        self.profs = {}

    def init(self, sc, bw, mode):
        r = new_row(bw)
        self.r.ref_row_init(*row_ptrs(r), mode, bw, sc["M"] + sc["refbonus"] + 1, sc["X"], *gaps(sc))
        return r

    def movx(self, src, W, movx, pw, sc):
        r = new_row(W * 16)
        self.r.ref_row_movx(*row_ptrs(r), *row_ptrs(src), W, movx, pw, sc["M"] + sc["refbonus"] + 1, sc["X"], *gaps(sc))
        return r

    def _prof(self, q, bw, prof, sc):
        key = (q.tobytes(), bw, prof, sc["M"], sc["X"], sc["refbonus"])
        if key not in self.profs:
            if len(self.profs) > 64:
                self.profs.clear()
            mtx, hpc = prof_matrix(sc, prof)
            qp = _al(int(self.r.ref_qprof_size(len(q), bw)) + 64, np.int8)
            if hpc:
                self.r.ref_set_query_prof_hpc(S.ptr(q, u8p), len(q), S.ptr(qp, i8p), bw, S.ptr(mtx, i8p), 1)
            else:
                self.r.ref_set_query_prof(S.ptr(q, u8p), len(q), S.ptr(qp, i8p), bw, S.ptr(mtx, i8p))
            self.profs[key] = qp
        return self.profs[key]

    def cal(self, moved, q, rbeg, base, prof, sc, W, movx, rh, pw):
        r = new_row(W * 16)
        qp = self._prof(q, W * 16, prof, sc)
        self.r.ref_row_cal(rbeg, base, *row_ptrs(moved), *row_ptrs(r), S.ptr(qp, i8p), *gaps(sc), W, movx, rh, pw)
        return r

    def merge(self, a, b, W, pw):
        r = new_row(W * 16)
        self.r.ref_row_merge(*row_ptrs(a), *row_ptrs(b), *row_ptrs(r), W, pw)
        return r

    def rowmax(self, r, W):
        ms = C.c_int32()
        x = self.r.ref_row_max(S.ptr(r[0], i8p), S.ptr(r[3], i32p), W, C.byref(ms))
        return int(x), ms.value


def left_rh(sc, mode, pw, toff):
    """the left-boundary score of a movx == 0, qoff == 0 update (bspoa.h:2246-2248): both gap pieces for piecewise 2"""
    if mode == S.MODE_OVERLAP or toff == 0:
        return 0
    if pw < 2:
        return sc["O"] + sc["E"] * toff
    return max(sc["O"] + sc["E"] * toff, sc["Q"] + sc["P"] * toff)


def update_rh(sc, mode, pw, qoff_src, movx, bw, toff, moved_ub0):
    """rh as dpalign_row_update_bspoa computes it (bspoa.h:2242-2254)"""
    if movx == 0:
        return SCORE_MIN if qoff_src else left_rh(sc, mode, pw, toff)
    return int(moved_ub0) if movx <= bw else SCORE_MIN


def pack(r, bw, pw):
    """a row in the layout of the reference's row block (us | es | qs | ubegs[17]; only the planes the piecewise form has)"""
    return np.concatenate([r[k].view(np.uint8) for k in range(pw + 1)] + [r[3][:17].view(np.uint8)])


def unpack(b, bw, pw):
    r = new_row(bw)
    for k in range(pw + 1):
        r[k][:] = b[k * bw:(k + 1) * bw].view(np.int8)
    r[3][:17] = b[(pw + 1) * bw:(pw + 1) * bw + 68].view(np.int32)
    return r


def used_bytes(bw, pw):
    return (pw + 1) * bw + 68


def clamped(r):
    return bool(np.any((r[0] == 127) | (r[0] == -128)))


def check_share(name, bw, mode, share):
    """what is asserted of the share of UPDATE rows that hold a us byte of 127 or -128, on the CPU and again in the GPU tests.
    SHARE_SETS: at least MIN_SHARE, at every bandwidth and mode.
    linear_big: none anywhere.  With linear gaps a cell is at least its left neighbour + gape1 and at most that + (M + refbonus + 1) - gape1,
    so every us lies in [-30, 47], and the synthetic cell behind a moved row is -78.
    big_affine: none up to 128 columns.  Neighbouring cells differ by -40 ... 92 in exact arithmetic, the synthetic cell is -103, and the
    int8 arithmetic stays exact there.  From 176 columns on it does not: the f that crosses a whole lane (f_penetrate) carries
    gapo1 + W * gape1 <= -140, which no byte holds, and a lane-start cell (vector 0 of a lane) that such an f decides is stored clamped.  An f
    seldom outlives a whole lane, so this is 0.2 ... 2 % of the rows in global and extend mode and none in overlap mode, all of them in
    vector 0 -- but at 256 and 512 columns in global mode these inputs do meet it, and that is asserted: the W * gape1 = -160 term of
    f_penetrate decides stored bytes under this set too.  It stays far below MIN_SHARE, hence affine_clamp."""
    if name in SHARE_SETS:
        assert share >= MIN_SHARE, (name, bw, mode, share)
    elif name == "linear_big" or (name == "big_affine" and bw <= 128):
        assert share == 0, (name, bw, mode, share)
    elif name == "big_affine" and bw >= 256 and mode == S.MODE_GLOBAL:
        assert 0 < share < MIN_SHARE, (name, bw, mode, share)


# ---- inputs whose rows clamp ------------------------------------------------------------------------------------------------------------
def sat_read(rng, n):
    """a read of homopolymer stretches between short random pieces: under a base that has nothing to do with the read whole runs of cells
    mismatch together, then a run matches, and the steps between the two are what leaves int8"""
    out = []
    while sum(len(x) for x in out) < n:
        if rng.random() < 0.6:
            out.append(np.full(int(rng.integers(3, 40)), int(rng.integers(4)), np.uint8))
        else:
            out.append(rng.integers(0, 4, size=int(rng.integers(2, 12))).astype(np.uint8))
    return np.concatenate(out)[:n].copy()


def movx_menu(W, bw, tail=5):
    return [0, 1, 1, 2, 3, W, W + 1, 2 * W + tail - 2, bw - 1, bw, bw + tail]


@functools.lru_cache(maxsize=None)
def chains(name, bw, mode, nchain=24, depth=20, nq=6):
    """the chain scheme of test_rows_gpu.py under one set: nchain independent chains of `depth` UPDATE levels (one level = one launch of
    bsa_rows_run), then MERGE tasks over pairs of chains, all of it computed ONCE with the oracle.
    -> dict(queries, qblob, qoff, qlen, blk, nrows, levels=[(tasks, [(dst, used bytes)])], share)"""
    sc = SETS[name] if name != "default" else DEFAULT
    R = OracleRows()
    rng = np.random.default_rng([bw, mode, _seed(name)])
    W, pw = bw // 16, piecewise(sc, bw)
    blk = P.block_bytes(bw, pw)
    queries = [sat_read(rng, int(rng.integers(bw + 40, 700))) for _ in range(nq)]
    qlen = np.array([len(q) for q in queries], dtype=np.uint32)
    qoff = np.zeros(nq, dtype=np.uint64)
    qoff[1:] = np.cumsum(qlen + 8)[:-1]
    qblob = np.zeros(int(qoff[-1]) + int(qlen[-1]) + 8, dtype=np.uint8)
    for k, q in enumerate(queries):
        qblob[int(qoff[k]):int(qoff[k]) + len(q)] = q
    stride = depth + 2
    rows, levels = {}, []
    tasks, exp = [], []
    for c in range(nchain):
        rows[c * stride] = R.init(sc, bw, mode)
        tasks.append((2, 0, c * stride, 0, 0, 0, c % nq, 0, 0, 0))
        exp.append((c * stride, pack(rows[c * stride], bw, pw)))
    levels.append((tasks, exp))
    state = [(0, c % nq) for c in range(nchain)]
    nupd = nclamp = 0
    for lev in range(depth):
        tasks, exp = [], []
        for c in range(nchain):
            src = c * stride + lev
            qs, qi = state[c]
            movx = int(rng.choice(movx_menu(W, bw, 3) + [1, 2, 3, 2, 3, 2, 3]))      # every move brings in a synthetic cell
            if qs + movx + bw > int(qlen[qi]):
                movx = 0
            qd = qs + movx
            # the task's base has nothing to do with the read (mismatches stack), except that one chain in four follows the read now and then
            base = int(queries[qi][min(qd + bw // 2, len(queries[qi]) - 1)]) if (c % 4 == 1 and rng.random() < 0.5) else int(rng.integers(4))
            prof = int(rng.integers(4))
            tasks.append((0, src, src + 1, qs, qd, lev + 1, qi, base, prof, 0))
            moved = R.movx(rows[src], W, movx, pw, sc)
            rh = update_rh(sc, mode, pw, qs, movx, bw, lev + 1, moved[3][0])
            rows[src + 1] = R.cal(moved, queries[qi], qd, base, prof, sc, W, movx, rh, pw)
            nupd += 1
            nclamp += clamped(rows[src + 1])
            exp.append((src + 1, pack(rows[src + 1], bw, pw)))
            state[c] = (qd, qi)
        levels.append((tasks, exp))
    tasks, exp = [], []
    for c in range(0, nchain - 1, 2):
        src, dst = c * stride + depth, (c + 1) * stride + depth
        tasks.append((1, src, dst, 0, 0, 0, 0, 0, 0, 0))
        exp.append((dst, pack(R.merge(rows[src], rows[dst], W, pw), bw, pw)))
    levels.append((tasks, exp))
    return dict(sc=sc, pw=pw, blk=blk, nrows=nchain * stride, queries=queries, qblob=qblob, qoff=qoff, qlen=qlen, levels=levels,
                share=nclamp / nupd, nupd=nupd)


# ---- sweep programs (test_poa_sweep_gpu.py's scheme) ---------------------------------------------------------------------------------
SWEEP_BANDWIDTHS = (16, 64, 256, 176, 512)        # register forms, then the run-time-width form


def chain_program(rng, n, bw, slen, query):
    """a backbone of n nodes with two-way bubbles, band offsets advancing ~1 per node and clamped to slen - bw, so a long program ends with
    rpos + bw == slen (the byte-wise tail of rows_fetch_codes; cells beyond the read's end); bases unrelated to the read but for short stretches"""
    tasks = [(2, 0, 2, 0, 0, 0, 0, 0, 0, 0)]
    blk_of, rpos, mpos, nxt = 2, 0, -1, 3
    cap = max(slen - bw, 0)
    for i in range(n):
        follow = (i // 9) % 3 == 0
        base = int(query[min(rpos + bw // 2, slen - 1)]) if follow else int(rng.integers(4))
        step = int(rng.choice([0, 1, 1, 1, 2, 3]))
        nr = min(rpos + step, cap)
        if i % 7 == 3:
            a, b, m = nxt, nxt + 1, nxt + 2
            nxt += 3
            tasks.append((0, blk_of, a, rpos, nr, mpos + 2, 0, base, int(rng.integers(4)), 0))
            tasks.append((0, blk_of, b, rpos, nr, mpos + 2, 0, (base + 1) & 3, int(rng.integers(4)), 0))
            nr2 = min(nr + 1, cap)
            mb = int(rng.integers(4))
            tasks.append((0, a, m, nr, nr2, mpos + 3, 0, mb, int(rng.integers(4)), 0))
            tasks.append((0, b, 1, nr, nr2, mpos + 3, 0, mb, int(rng.integers(4)), 0))
            tasks.append((1, 1, m, 0, 0, 0, 0, 0, 0, 0))
            blk_of, rpos, mpos = m, nr2, mpos + 2
        else:
            tasks.append((0, blk_of, nxt, rpos, nr, mpos + 2, 0, base, int(rng.integers(4)), 0))
            blk_of, rpos, mpos = nxt, nr, mpos + 1
            nxt += 1
        if rpos + bw >= slen and i % 5 == 0:
            tasks.append((4, blk_of, 0, rpos, 0, 1000 + i, 0, 0, 0, 0))
    tasks.append((3, blk_of, 0, rpos, 0, 7777, 0, 0, 0, 0))
    return np.array(tasks, dtype=P.TASK_DTYPE), nxt, rpos


@functools.lru_cache(maxsize=None)
def sweep_batch(name, bw, mode, nprog=24):
    """24 programs of 50 - 300 nodes, slen in [bw + 50, bw + 400], with the oracle's rows and results.  Every third program is as long as it takes
    to end with rpos + bw == slen."""
    sc = dict(SETS[name], alnmode=mode)
    rng = np.random.default_rng([bw, mode, _seed(name), 7])
    tasks, progs, queries, qoff, qlen, ends = [], [], [], [], [], 0
    tacc = bacc = qacc = 0
    for k in range(nprog):
        slen = int(rng.integers(bw + 50, bw + 401))
        q = sat_read(rng, slen)
        n = int(rng.integers(50, 301)) if k % 3 else 300
        if k % 3 == 0:
            slen = min(slen, bw + 200)         # 300 nodes advance the band ~ 1.3 cells each: the band reaches the read's end
            q = q[:slen].copy()
        t, nb, rpos = chain_program(rng, n, bw, slen, q)
        ends += int(rpos + bw == slen)
        t["query"] = k
        tasks.append(t)
        progs.append((tacc, len(t), bacc, 0))
        tacc += len(t)
        bacc += nb
        queries.append(q)
        qoff.append(qacc)
        qlen.append(slen)
        qacc += slen
    tasks, progs = np.concatenate(tasks), np.array(progs, dtype=P.PROG_DTYPE)
    queries, qoff, qlen = np.concatenate(queries), np.array(qoff, np.uint64), np.array(qlen, np.uint32)
    pw = piecewise(sc, bw)
    orows, ores = P.oracle_sweep(tasks, progs, queries, qoff, qlen, sc, bw, bacc, pw)
    blk = P.block_bytes(bw, pw)
    upd = np.unique(np.concatenate([tasks["dst"][int(p["first_task"]):int(p["first_task"]) + int(p["ntasks"])][
        tasks["op"][int(p["first_task"]):int(p["first_task"]) + int(p["ntasks"])] == 0].astype(np.int64) + int(p["first_block"]) for p in progs]))
    us = orows.reshape(bacc, blk)[upd, :bw].view(np.int8)
    share = float(np.mean(((us == 127) | (us == -128)).any(axis=1)))
    return dict(sc=sc, pw=pw, blk=blk, tasks=tasks, progs=progs, queries=queries, qoff=qoff, qlen=qlen, nblocks=bacc, orows=orows, ores=ores,
                share=share, ends=ends)


# ---- the run-time-width merge at 8192 columns (W = 512: row_merge re-bases its int16 offsets every 256 vectors, bsalign.h:2496) --------
MERGE_BW = 8192
# a long extension: in global mode the cells of a row the alignment has not reached cost gape1 each, so a lane's 512 cells sum to -51 200 -- past
# int16 unless row_merge re-bases after 256 vectors.  With the re-basing in place no int16 sum of this program saturates: the saturation
# itself is what draw_merge_s16_cases is there for.
MERGE_SC = dict(M=20, X=-40, refbonus=1, O=-20, E=-100, Q=0, P=0, T=20, alnmode=S.MODE_GLOBAL)
SC_KEYS = ("M", "X", "refbonus", "O", "E", "Q", "P", "T")


def draw_merge8192_program():
    """a handful of nodes: two branches of three nodes each from the head, merged in one node (make_golden_rows_sat.py stores it in the fixture)"""
    rng = np.random.default_rng(8192)
    slen = MERGE_BW + 64
    q = sat_read(rng, slen)
    tasks = [(2, 0, 2, 0, 0, 0, 0, 0, 0, 0)]
    for br, (first, bases, offs) in enumerate(((3, (0, 1, 2), (0, 2, 3)), (6, (3, 3, 0), (1, 1, 3)))):
        src, ro = 2, 0
        for k, (b, nr) in enumerate(zip(bases, offs)):
            tasks.append((0, src, first + k, ro, nr, k + 1, 0, b, (k + br) & 3, 0))
            src, ro = first + k, nr
    # both branches end at band offset 3; the merge node takes one more step from each (the second through the temporary block 1)
    tasks.append((0, 5, 9, 3, 4, 4, 0, 1, 0, 0))
    tasks.append((0, 8, 1, 3, 4, 4, 0, 1, 0, 0))
    tasks.append((1, 1, 9, 0, 0, 0, 0, 0, 0, 0))
    tasks.append((4, 9, 0, 4, 0, 99, 0, 0, 0, 0))
    return dict(tasks=np.array(tasks, dtype=P.TASK_DTYPE), query=q, slen=slen, nblocks=10, sc=dict(MERGE_SC))


def run_program(R, prog, bw):
    """a task program through the row functions of one side, as align_rd_bspoacore drives them (block 0: the moved row) -> {block: row}"""
    sc, q = prog["sc"], prog["query"]
    W, pw, mode = bw // 16, piecewise(prog["sc"], bw), prog["sc"]["alnmode"]
    rows = {}
    for t in prog["tasks"]:
        op, src, dst = int(t["op"]), int(t["src"]), int(t["dst"])
        if op == 2:
            rows[dst] = R.init(sc, bw, mode)
        elif op == 0:
            movx = int(t["qoff_dst"]) - int(t["qoff_src"])
            rows[0] = R.movx(rows[src], W, movx, pw, sc)
            rh = update_rh(sc, mode, pw, int(t["qoff_src"]), movx, bw, int(t["toff"]), rows[0][3][0])
            rows[dst] = R.cal(rows[0], q, int(t["qoff_dst"]), int(t["base"]), int(t["prof"]), sc, W, movx, rh, pw)
        elif op == 1:
            rows[dst] = R.merge(rows[src], rows[dst], W, pw)
    return rows


# ---- row_merge where its int16 sums saturate ------------------------------------------------------------------------------------------
S16_BW = 4096        # W = 256: one whole stretch between two re-basings


def draw_merge_s16_cases(n=2):
    """pairs of rows made by hand for row_merge alone (the reference is the authority on any input; ubegs are set per lane, which is all
    row_merge reads).  Every lane falls by a full byte per cell for nearly all of the 256 cells between two re-basings, from bases that lie
    0, 1, 2, ... or far more than 32767 apart, so that in the last cells of the stretch the int16 sums t + e of BOTH rows run into -32768:
    the merged es there is what the saturated sums give (0 where both rows sit at -32768, whatever their e), not what exact sums would.
    That is as far as int16 saturation can be seen in a result of the reference.  A sum t that saturates at -32768 belongs to the lower row
    and never decides a maximum; one that saturates at +32767 changes the merged us, and the reference's row_merge checks those against
    exact sums as it goes and aborts (bsalign.h:2551-2562), so no lane climbs here.  -> [(packed row, packed row)], piecewise 1"""
    W, out = S16_BW // 16, []
    apart = (0, 0, 0, -1, -1, 1, 1, 2, -2, 3, -3, 60, -100, 127, 40000, -70000)
    for k in range(n):
        rng = np.random.default_rng([16, k])
        pair, base = [], rng.integers(-1000, 1000, 16)
        for side in range(2):
            r = new_row(S16_BW)
            us, es = r[0].reshape(W, 16), r[1].reshape(W, 16)
            us[:] = -128
            for j in range(16):
                if k and rng.random() < 0.5:           # a few cells that are not -128: the sums just reach -32768, or just do not
                    us[rng.integers(0, W, 3), j] = rng.integers(-128, -120, 3)
                es[:, j] = rng.choice([-128, -100, -40, -3, -1], W, p=[0.1, 0.1, 0.3, 0.3, 0.2])
            r[3][:16] = base + (np.array(apart)[rng.permutation(16)] if side else 0)
            r[3][16] = int(rng.integers(-100000, 0))
            pair.append(pack(r, S16_BW, 1))
        out.append(tuple(pair))
    return out


def merge_without_int16(a, b):
    """row_merge's es of two piecewise-1 rows of S16_BW columns in exact arithmetic (no int16 saturation; the final byte clamp kept): what
    the recorded rows must differ from for the cases to say anything about s16"""
    W = S16_BW // 16
    ra, rb = unpack(a, S16_BW, 1), unpack(b, S16_BW, 1)
    ta = ra[3][:16].astype(np.int64) + np.cumsum(ra[0].reshape(W, 16).astype(np.int64), axis=0)
    tb = rb[3][:16].astype(np.int64) + np.cumsum(rb[0].reshape(W, 16).astype(np.int64), axis=0)
    me = np.maximum(ta + ra[1].reshape(W, 16), tb + rb[1].reshape(W, 16))
    return np.clip(me - np.maximum(ta, tb), -128, 127).astype(np.int8).reshape(-1)


def load_s16_cases():
    """-> [(row, row, the reference's merged row)] from the fixture"""
    g = np.load(FIXTURE)
    return [(a, b, m) for (a, b), m in zip(g["s16_in"], g["s16_out"])]


# ---- tests/golden/rows_sat.npz (make_golden_rows_sat.py): the REFERENCE's rows in this regime ----------------------------------------
FIX_SETS = ("default",) + tuple(SETS)
FIX_CHAINS, FIX_STEPS = 2, 12


def draw_fixture_plan():
    """what make_golden_rows_sat.py records, in order: (set, bw, mode, chain) -> the read and per step (movx, base, prof).  The fixture stores
    all of it, and the tests take the plan from the file (load_fixture), never from here."""
    plan = []
    for name in FIX_SETS:
        sc = DEFAULT if name == "default" else SETS[name]
        for bw in (BANDWIDTHS if name == "default" else bandwidths(name)):
            W = bw // 16
            for mode in MODES:
                for ch in range(FIX_CHAINS):
                    rng = np.random.default_rng([_seed(name), bw, mode, ch, 99])
                    qlen = bw + 150
                    q = sat_read(rng, qlen)
                    steps, rbeg = [], 0
                    for st in range(FIX_STEPS):
                        movx = int(rng.choice(movx_menu(W, bw) + [1, 2, 3, 2, 3, 2, 3])) if st else 0
                        if rbeg + movx + bw > qlen:            # the reference only guarantees profile rows up to qlen (bsalign.h:2147)
                            movx = 0
                        rbeg += movx
                        steps.append((movx, int(rng.integers(4)), int(rng.integers(4)), None))
                    plan.append(dict(name=name, sc={k: sc[k] for k in SC_KEYS}, bw=bw, mode=mode, chain=ch, query=q, steps=steps))
    return plan


def run_fixture_chain(R, c, feed=None, rhs=None):
    """one chain of the plan through the row functions of R -> list of packed rows: init, then per step moved, new, merged (of moved and new:
    two progenitors of one node, bspoa.h:2263-2272) and (row_max index, score).  With feed (the recorded rows) every call gets the RECORDED
    input, so one difference does not spread.  rh is computed as dpalign_row_update_bspoa does and must be the recorded one, where one is
    recorded; rhs collects it."""
    sc, bw, mode = c["sc"], c["bw"], c["mode"]
    W, pw = bw // 16, piecewise(sc, bw)
    row = R.init(sc, bw, mode)
    out = [pack(row, bw, pw)]
    rbeg = 0
    for st, (movx, base, prof, rec_rh) in enumerate(c["steps"]):
        k = 1 + 4 * st                                  # out[k .. k + 3]: moved, new, merged, row_max of this step
        if feed is not None:
            row = unpack(feed[0] if st == 0 else feed[k - 3], bw, pw)
        moved = R.movx(row, W, movx, pw, sc)
        out.append(pack(moved, bw, pw))
        if feed is not None:
            moved = unpack(feed[k], bw, pw)
        rh = update_rh(sc, mode, pw, rbeg, movx, bw, st, moved[3][0])
        assert rec_rh is None or rh == rec_rh, (c["name"], bw, mode, st, rh, rec_rh)
        if rhs is not None:
            rhs.append(rh)
        rbeg += movx
        new = R.cal(moved, c["query"], rbeg, base, prof, sc, W, movx, rh, pw)
        out.append(pack(new, bw, pw))
        if feed is not None:
            new = unpack(feed[k + 1], bw, pw)
        out.append(pack(R.merge(moved, new, W, pw), bw, pw))
        out.append(np.array(R.rowmax(new, W), dtype=np.int32).view(np.uint8))
        row = new
    return out


@functools.lru_cache(maxsize=None)
def load_fixture():
    """everything from the file alone -> (list of (plan entry, recorded rows as run_fixture_chain lists them), the 8192-column merge program,
    its recorded blocks {block: used bytes}).  A set whose scoring is no longer the one recorded makes this fail: regenerate."""
    g = np.load(FIXTURE)
    names = [str(x) for x in g["set_names"]]
    blob, off, qblob = g["rows"], g["row_off"], g["queries"]
    recs, qo = [], 0
    for i, (si, bw, mode, ch, qlen) in enumerate(g["meta"].tolist()):
        name = names[si]
        sc = dict(zip(SC_KEYS, g["scores"][si].tolist()))
        now = DEFAULT if name == "default" else SETS[name]
        assert all(sc[k] == now[k] for k in SC_KEYS), "tests/golden/rows_sat.npz: %s was recorded under another scoring (make_golden_rows_sat.py)" % name
        c = dict(name=name, sc=sc, bw=bw, mode=mode, chain=ch, query=qblob[qo:qo + qlen].copy(), steps=[tuple(x) for x in g["steps"][i].tolist()])
        qo += qlen
        pw = piecewise(sc, bw)
        n, b = used_bytes(bw, pw), blob[int(off[i]):int(off[i + 1])]
        rows, o = [b[:n]], n
        for _ in c["steps"]:
            rows += [b[o:o + n], b[o + n:o + 2 * n], b[o + 2 * n:o + 3 * n], b[o + 3 * n:o + 3 * n + 8]]
            o += 3 * n + 8
        assert o == len(b)
        recs.append((c, rows))
    have = set((c["name"], c["bw"], c["mode"]) for c, _ in recs)
    want = set((n, bw, m) for n in FIX_SETS for bw in (BANDWIDTHS if n == "default" else bandwidths(n)) for m in MODES)
    assert have == want, "tests/golden/rows_sat.npz does not cover the sets of rows_sat_cases.py (make_golden_rows_sat.py)"
    msc = dict(zip(SC_KEYS + ("alnmode",), g["merge_score"].tolist()))
    assert msc == MERGE_SC
    mp = dict(tasks=g["merge_tasks"].view(P.TASK_DTYPE).copy(), query=g["merge_query"], slen=len(g["merge_query"]), nblocks=10, sc=msc)
    return recs, mp, {int(k): v for k, v in zip(g["merge_blocks"], g["merge_rows"])}
