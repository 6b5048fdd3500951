"""Seeded random POA programs, scorings and the score guard's boundary, for tests/test_poa_random_cpu.py and tests/test_poa_random_gpu.py.

Programs are made in the TASK form (poa_support.TASK_DTYPE), so that the lane-exact oracle (orc_sweep_run) runs them as they are and, through
poa_support.tasks_to_graph, the scalar statement (orc_wf_*) and both device kernels (k_poa_wf, k_poa_gen) run the same program.

A program (generate):
* a backbone whose nodes now and then split into 2 - 5 branches of unequal length (0 - 50 nodes; at most one branch of a bubble is the bare
  edge) that re-join in one node: in-degrees 1 ... 5, so up to three partial nodes chained in front of a merge.  Branches are emitted one after
  the other, so the first inputs of a merge lie as many nodes back in completion order as the later branches hold; with `long_branch` one bubble
  has later branches of 34 or more nodes: further back than the forward pass's ring (8 / 16 rows) and than the walk's ring of 32 nodes;
* band offsets follow the query position of the path the query was copied from (so the alignment stays inside the band and the walk is long):
  per node they move by 0, 1 or 2 cells, in `jumpy` programs now and then by 3 ... bw + 8 cells (moved rows with synthetic cells, dead rows).
  Every branch follows its own depth, so the inputs of one merge arrive with different qoff_src.  Offsets are clamped to [0, max(slen - bw, 0)];
* prof bit 0 (the node's refbonus bit) is random per node; a node repeats the base of the node before it with probability 1 / 4; prof bit 1
  (IN_SAME) says whether the two bases are equal, as the binding sets it (bsa_pog.cpp) -- the walk recomputes that bit from the bases, so a walk
  over rows made with another bit leaves the rows at once.  Two programs of a set of 64 (`wild`) have the bit random all the same: its rows are compared
  like any other's, and its walk only has to end the same way on both sides;
* end candidates of both kinds: op 4 on one node in five among those whose band reaches the read's end, op 3 on the last node;
* the query is a noisy copy (support.mutate) of ONE path through the graph; one program in seven has uniform noise instead (low scores, ties);
  `short` programs have slen < bw.

validate() checks what the kernels rely on; every test calls it before a program goes anywhere.  random_coverage() gives the in-edges small
coverages (1 ... 4) in the one edge table that both the oracle's walk and the device read.

Scorings: draw_scoring() and BOUNDARY are classified by the library's own bsa_poa_graph_supported / bsa_poa_graph_gen_supported (host functions
of libbsalign_hip.so, which loads without a GPU) -- the guard is not restated here."""
import ctypes as C
import functools

import numpy as np

import poa_support as P
import support as S

HEAD = 2          # block 0: scratch, 1: merge temporary, 2: the head's row


# ---- programs ------------------------------------------------------------------------------------------------------------------------
def _topology(rng, nnodes, long_branch):
    """-> segments: ("node", base, bonus) | ("bubble", [[(base, bonus), ...] per branch], (base, bonus) of the merge node)"""
    segs, n, prev = [], 0, 4

    def nb(pv):
        b = pv if (pv < 4 and rng.random() < 0.25) else int(rng.integers(4))
        return b, int(rng.integers(2))
    want_long = long_branch
    while n < nnodes:
        force = want_long and n >= nnodes // 3
        if force or (n > 2 and rng.random() < 1.0 / 6):
            ways = int(rng.choice([2, 2, 2, 3, 3, 4, 5]))
            lens = [int(rng.choice([1, 1, 2, 2, 3, 5, 8, int(rng.integers(10, 41))])) for _ in range(ways)]
            if rng.random() < 0.3:
                lens[int(rng.integers(ways))] = 0
            if force:
                lens[0] = int(rng.integers(1, 6)); lens[1] = int(rng.integers(34, 51))
                want_long = False
            brs = []
            for ln in lens:
                pv, br = prev, []
                for _ in range(ln):
                    b = nb(pv); br.append(b); pv = b[0]
                brs.append(br)
            m = nb(prev)
            segs.append(("bubble", brs, m)); prev = m[0]; n += sum(lens) + 1
        else:
            b = nb(prev)
            segs.append(("node", b[0], b[1])); prev = b[0]; n += 1
    return segs


def generate(seed, index, bw, nnodes, mode_hint=1, slen_target=None, short=False, noise=None, wild=None, jumpy=None, long_branch=False, eps=None, pre_frac=0.5):
    """one program: dict(tasks, query, slen, bandwidth, nblocks, seed, index, flags ...).  Everything follows from (seed, index) and the arguments."""
    rng = np.random.default_rng([int(seed), int(index)])
    noise = (rng.random() < 1.0 / 7) if noise is None else noise
    wild = (rng.random() < 1.0 / 24) if wild is None else wild
    jumpy = (rng.random() < 0.2) if jumpy is None else jumpy
    eps = float(rng.choice([0.03, 0.08, 0.15])) if eps is None else eps
    segs = _topology(rng, nnodes, long_branch)
    # the path the query is copied from
    path, pick = [], []
    for sg in segs:
        if sg[0] == "node":
            path.append(sg[1]); pick.append(-1)
        else:
            k = int(rng.integers(len(sg[1])))
            pick.append(k)
            path.extend(b for b, _ in sg[1][k]); path.append(sg[2][0])
    core = S.mutate(rng, np.array(path, np.uint8), eps)
    if short:
        core = core[:max(int(rng.integers(max(bw // 4, 2), bw)), 1)]
        if len(core) == 0:
            core = rng.integers(0, 4, size=max(bw // 2, 1)).astype(np.uint8)
    extra = int(rng.integers(0, 40)) if slen_target is None else max(int(slen_target) - len(core), 0)
    pre = 0 if short else int(extra * pre_frac)
    query = np.concatenate([rng.integers(0, 4, size=pre), core, rng.integers(0, 4, size=0 if short else extra - pre)]).astype(np.uint8)
    slen = len(query)
    if noise:
        query = rng.integers(0, 4, size=slen).astype(np.uint8)
    cap = max(slen - bw, 0)
    ratio = len(core) / max(len(path), 1)
    total = max(len(path), 1)

    def step(r, depth):
        want = max(int(pre + depth * ratio) - bw // 2, (cap * depth) // (2 * total))
        if jumpy and rng.random() < 1.0 / 150:
            st = int(rng.integers(3, bw + 9)) if rng.random() < 0.3 else int(rng.integers(3, 9))
        elif r < want:
            st = int(rng.choice([1, 2, 2, 2]))
        elif r > want:
            st = int(rng.choice([0, 0, 1]))
        else:
            st = int(rng.choice([0, 1, 1, 1, 2]))
        return min(max(r + st, 0), cap)

    tasks = [(2, 0, HEAD, 0, 0, 0, 0, 0, 0, 0)]
    nxt = [3]
    base_of = {HEAD: 4}

    def prof(bonus, b, src):
        same = int(rng.integers(2)) if wild else int(b == base_of[src])
        return bonus | (same << 1)

    def update(src, dst_tmp, dst, b, bonus, r0, r1, depth):
        tasks.append((0, src, dst_tmp, r0, r1, depth, 0, b, prof(bonus, b, src), 0))
        base_of[dst] = b

    def cand(blk, r):
        if r + bw >= slen and rng.random() < 0.2:
            tasks.append((4, blk, 0, r, 0, 1000 + blk, 0, 0, 0, 0))

    cur, rpos, depth = HEAD, 0, 0          # (depth = the node's position on its path: the task's toff is the source's depth + 1, v->mpos)
    for sg, k in zip(segs, pick):
        if sg[0] == "node":
            blk = nxt[0]; nxt[0] += 1
            nr = step(rpos, depth + 1)
            update(cur, blk, blk, sg[1], sg[2], rpos, nr, depth + 1)
            cur, rpos, depth = blk, nr, depth + 1
            cand(cur, rpos)
            continue
        ends = []
        for br in sg[1]:
            c, r, d = cur, rpos, depth
            for b, bonus in br:
                blk = nxt[0]; nxt[0] += 1
                nr = step(r, d + 1)
                update(c, blk, blk, b, bonus, r, nr, d + 1)
                c, r, d = blk, nr, d + 1
            ends.append((c, r, d))
        m = nxt[0]; nxt[0] += 1
        dm = ends[k][2] + 1
        rm = step(max(e[1] for e in ends), dm)
        for j, (c, r, d) in enumerate(ends):
            update(c, m if j == 0 else 1, m, sg[2][0], sg[2][1], r, rm, d + 1)
            if j:
                tasks.append((1, 1, m, 0, 0, 0, 0, 0, 0, 0))
        cur, rpos, depth = m, rm, dm
        cand(cur, rpos)
    tasks.append((3, cur, 0, rpos, 0, 1000 + cur, 0, 0, 0, 0))          # (a node has one graph id, whichever candidate names it)
    return dict(tasks=np.array(tasks, dtype=P.TASK_DTYPE), query=query, slen=slen, bandwidth=bw, nblocks=nxt[0], seed=int(seed), index=int(index),
                noise=bool(noise), wild=bool(wild), jumpy=bool(jumpy), short=bool(short), long_branch=bool(long_branch), mode_hint=mode_hint)


def validate(pg):
    """the invariants the oracle and the kernels rely on, as plain assertions: a generator bug must stop here, on the CPU.
    -> the program's graph form (nodes, edges, cands, blocks)"""
    t, bw, slen, nb = pg["tasks"], int(pg["bandwidth"]), int(pg["slen"]), int(pg["nblocks"])
    assert bw >= 16 and bw % 16 == 0
    assert slen >= 1 and len(pg["query"]) == slen and pg["query"].dtype == np.uint8 and int(pg["query"].max()) < 4
    cap = max(slen - bw, 0)
    assert len(t) >= 2 and int(t[0]["op"]) == 2 and int(t[0]["dst"]) == HEAD
    rpos, done, open_dst, used, nreal, indeg = {HEAD: 0}, {HEAD}, None, set(), 1, {}
    ncand = 0
    i = 1
    while i < len(t):
        k = t[i]
        op, src, dst, q0, q1 = (int(k[f]) for f in ("op", "src", "dst", "qoff_src", "qoff_dst"))
        assert int(k["query"]) == 0 and 0 <= op <= 4 and op != 2, (i, op)
        assert src < nb and dst < nb
        if op == 0:
            assert src in done and src >= HEAD, (i, "source not defined before use", src)
            assert q0 == rpos[src] and q1 >= q0 and q1 <= cap, (i, "band offsets", q0, q1, rpos[src], cap)
            assert int(k["base"]) < 4 and int(k["prof"]) < 4 and int(k["toff"]) <= P.IN_PRESENT >> 4
            used.add(src)
            if dst == 1:
                assert open_dst is not None and i + 1 < len(t) and int(t[i + 1]["op"]) == 1 and int(t[i + 1]["src"]) == 1 and int(t[i + 1]["dst"]) == open_dst, (i, "update into the temporary without its merge")
                assert q1 == rpos[open_dst] and int(k["base"]) == base and (int(k["prof"]) & 1) == bonus, (i, "inputs of one node disagree")
                indeg[open_dst] += 1
                i += 2
                continue
            assert dst > HEAD and dst not in done and dst not in used, (i, "completion order", dst)
            open_dst, base, bonus = dst, int(k["base"]), int(k["prof"]) & 1
            rpos[dst] = q1; done.add(dst); indeg[dst] = 1; nreal += 1
        elif op == 1:
            assert False, (i, "merge without an update into the temporary in front of it")
        else:
            assert src in done and q0 == rpos[src], (i, "candidate", src)
            if op == 4:
                assert rpos[src] + bw >= slen and slen - 1 - rpos[src] >= 0, (i, "end candidate outside its band")
            used.add(src); ncand += 1
        i += 1
    assert ncand >= 1 and max(indeg.values(), default=0) <= 5
    nodes, edges, cands, blocks = P.tasks_to_graph(t)
    npart = sum(max(d - 2, 0) for d in indeg.values())
    assert len(nodes) == nreal + npart and len(edges) == sum(indeg.values()) and len(cands) == ncand and int((blocks != 0).sum()) == nreal
    assert int(nodes[0]["n_in"]) == 0 and int(nodes[0]["base"]) == 4
    validate_graph(nodes, edges, cands, slen, bw)
    return nodes, edges, cands, blocks


def validate_graph(nodes, edges, cands, slen, bw):
    """the argument checks of bsa_poa_graph_host, plus the band offsets"""
    n = len(nodes)
    idx = np.arange(n)
    assert (nodes["rpos"] <= max(slen - bw, 0)).all()
    for j in ("in0", "in1"):
        pres = (nodes[j + "_tk"] & P.IN_PRESENT) != 0
        assert (nodes[j + "_src"][pres] < idx[pres]).all()
        plain = pres & ((nodes[j + "_tk"] & P.IN_MERGE) == 0)
        assert (nodes["rpos"][plain] - nodes[j + "_movx"][plain] == nodes["rpos"][nodes[j + "_src"][plain]]).all(), "movx against the source's band offset"
        mg = pres & ((nodes[j + "_tk"] & P.IN_MERGE) != 0)
        assert (nodes["rpos"][mg] == nodes["rpos"][nodes[j + "_src"][mg]]).all() and (nodes["gnode"][nodes[j + "_src"][mg]] == 0xFFFFFFFF).all()
    assert ((nodes["first_in"].astype(np.int64) + nodes["n_in"]) <= len(edges)).all()
    for i in np.nonzero(nodes["n_in"])[0]:
        e = edges[int(nodes[i]["first_in"]):int(nodes[i]["first_in"]) + int(nodes[i]["n_in"])]
        assert (e["src"] < i).all() and (e["src_rpos"] == nodes["rpos"][e["src"]]).all()
    assert len(cands) and (cands["node"] < n).all() and (cands["kind"] <= 1).all()


def random_coverage(seed, index, edges):
    """edges["cov"] <- 1 ... 4 (ties are common).  The one table goes to the oracle's walk and to the device."""
    rng = np.random.default_rng([int(seed), int(index), 77])
    edges["cov"] = rng.integers(1, 5, size=len(edges)).astype(np.uint32)
    return edges


def graph_of(pg):
    """validate + graph form with random coverages, kept with the program"""
    if "graph" not in pg:
        nodes, edges, cands, blocks = validate(pg)
        random_coverage(pg["seed"], pg["index"], edges)
        pg["graph"] = (nodes, edges, cands, blocks)
    return pg["graph"]


def in_degrees(pg):
    nodes = graph_of(pg)[0]
    return np.bincount(nodes["n_in"][nodes["gnode"] != 0xFFFFFFFF], minlength=6)


def max_input_distance(pg):
    """the furthest a plain (not MERGE) input lies back in completion order: what decides between the forward ring and the read-back from HBM"""
    nodes = graph_of(pg)[0]
    d = 0
    for j in ("in0", "in1"):
        plain = ((nodes[j + "_tk"] & P.IN_PRESENT) != 0) & ((nodes[j + "_tk"] & P.IN_MERGE) == 0)
        if plain.any():
            d = max(d, int((np.arange(len(nodes))[plain] - nodes[j + "_src"][plain]).max()))
    return d


# the narrow sets the GPU tests launch: per bandwidth 64 programs of mixed length in one launch
NARROW_BW = (16, 32, 64, 96, 128, 176, 256)
NARROW_SEED = 20260
NARROW_N = 64


@functools.lru_cache(maxsize=None)
def narrow_set(bw, n=NARROW_N, seed=NARROW_SEED):
    out = []
    for k in range(n):
        rng = np.random.default_rng([seed, bw, k])
        nn = int(rng.integers(30, 360 + 2 * bw))
        pg = generate(seed + bw, k, bw, nn, short=(k % 9 == 4), wild=(k % 32 == 7), long_branch=(k % 4 == 1 and nn >= 120))
        graph_of(pg)
        out.append(pg)
    return out


# the wide ones: (columns, nodes) per cells-a-thread class of k_poa_gen (1024 threads: C = 1, 2, 4, 8, 16, 32)
WIDE = ((704, 700, 1), (1504, 900, 2), (3008, 700, 4), (6000, 500, 8), (12000, 400, 16), (18000, 300, 32))
WIDE_SEED = 31337


@functools.lru_cache(maxsize=None)
def wide_program(bw, nnodes, variant=0):
    """slen of the band's size plus a few hundred cells, so that rows move; branches as everywhere"""
    pg = generate(WIDE_SEED + bw, variant, bw, nnodes, slen_target=bw + 200 + 64 * variant, noise=False, wild=False, jumpy=(variant % 2 == 0), long_branch=True, eps=0.08)
    graph_of(pg)
    return pg


# ---- scorings ------------------------------------------------------------------------------------------------------------------------
def _sc(M, X, rb, O, E, Q=0, P_=0, T=20):
    return dict(M=M, X=X, refbonus=rb, O=O, E=E, Q=Q, P=P_, T=T)


def draw_scoring(rng):
    """(M, X, refbonus, O, E, Q, P, T): linear (O = 0), one-piece and two-piece gaps; about half of the draws fall outside the guard"""
    M, X, rb = int(rng.integers(1, 30)), -int(rng.integers(0, 60)), int(rng.integers(0, 4))
    kind = int(rng.integers(4))
    O = 0 if kind == 0 else -int(rng.integers(1, 20))
    E = -int(rng.integers(1, 12))
    Q = P_ = 0
    if kind >= 2:
        P_ = -int(rng.integers(0, -E)) if E < -1 else 0
        Q = O - int(rng.integers(1, 14))
    return _sc(M, X, rb, O, E, Q, P_, int(rng.choice([0, 5, 20, 60])))


# Scorings the guard took until these tests: m + 2 n <= 128 held, yet the seed of band cell 0 over the head's row (rh - (m + n) + X with rh the cost of
# the leading nodes) fell below -128 while still above its alternative, and the reference stores it into a byte lane: its rows wrap, the absolute
# scores do not (first seen at bandwidth 176, narrow_set(176)[27], global and extend mode).  The guard's head-seed term refuses them now.
REGRESSION = (_sc(2, -61, 0, -3, -2), _sc(2, -62, 1, -3, -2), _sc(2, -62, 1, -3, -2, -8, -1))

# ... and scorings with a large match score and no open cost: the vertical difference of band cell 0 over the head's row saturates in the reference
# (first seen at bandwidth 16, narrow_set(16)[45], every mode): refused by the guard's second head term now.
REGRESSION_VERTICAL = (_sc(50, -32, 0, 0, 0), _sc(61, -6, 0, 0, -1), _sc(63, -32, 0, 0, 0), _sc(41, -43, 0, 0, 0), _sc(49, -25, 0, 0, -2))

# For every inequality of the guard one scoring that meets it with equality and one that breaks it by the smallest step, per gap model where the
# term depends on it.  (m = M + refbonus + 1, n = -X, g = the dearer gap's open + extend, ge = -E.)  `inside`: what the library is expected to
# say (tests assert that it does, then use its answer).  Two terms cannot be met with equality inside the guard: with m + 3 g <= 64 and
# m + 2 n <= 128 the sum n + m + g is at most 86 over the scorings tests/test_poa_random_cpu.py::test_terms_that_cannot_bind tries, by the second head term (65 with an open cost, by the first), so n + m + g <= 100 and min(X, -g) - 1 - m - g >= -100 never bind;
# for them the list holds the scorings that come closest from inside ("near") and the equality / by-one points, which other terms refuse.
# gape1 <= gape2 cannot fail either where it is asked: the two-piece model is only chosen with gape2 > gape1 (bsa_get_piecewise), so with
# gape2 <= gape1 the scoring is one-piece and inside.  `bw`: the term depends on the width (k_poa_wf only; k_poa_gen takes the scoring).
BOUNDARY = [
    dict(term="m+3g<=64", side="eq", inside=True, sc=_sc(2, -6, 1, -18, -2)),
    dict(term="m+3g<=64", side="over", inside=False, sc=_sc(2, -6, 1, -19, -2)),
    dict(term="m+3g<=64", side="eq", inside=True, sc=_sc(57, -6, 0, 0, -2)),
    dict(term="m+3g<=64", side="over", inside=False, sc=_sc(58, -6, 0, 0, -2)),
    dict(term="m+3g<=64", side="eq", inside=True, sc=_sc(2, -6, 1, -3, -2, -19, -1)),
    dict(term="m+3g<=64", side="over", inside=False, sc=_sc(2, -6, 1, -3, -2, -20, -1)),
    dict(term="m+2n<=128", side="eq", inside=True, sc=_sc(2, -62, 1, 0, -2)),          # (binds without an open cost only: with one the head-seed term is tighter)
    dict(term="m+2n<=128", side="over", inside=False, sc=_sc(3, -62, 1, 0, -2)),
    dict(term="go+ge+m+n+63<=128", side="eq", inside=True, sc=_sc(2, -56, 1, -3, -2)),
    dict(term="go+ge+m+n+63<=128", side="over", inside=False, sc=_sc(2, -57, 1, -3, -2)),
    dict(term="go+ge+m+n+63<=128", side="eq", inside=True, sc=_sc(2, -56, 1, -3, -2, -8, -1)),
    dict(term="go+ge+m+n+63<=128", side="over", inside=False, sc=_sc(2, -57, 1, -3, -2, -8, -1)),
    dict(term="go+ge+m+n+63<=128", side="over", inside=False, sc=_sc(2, -61, 0, -3, -2)),          # REGRESSION[0]
    dict(term="2m+n+go+ge<=126", side="eq", inside=True, sc=_sc(49, -24, 0, 0, -2)),          # (binds without an open cost only)
    dict(term="2m+n+go+ge<=126", side="over", inside=False, sc=_sc(49, -25, 0, 0, -2)),
    dict(term="2m+n+go+ge<=126", side="over", inside=False, sc=_sc(50, -32, 0, 0, 0)),          # REGRESSION_VERTICAL
    dict(term="n+m+g<=100", side="near", inside=True, sc=_sc(41, -42, 0, 0, 0)),
    dict(term="n+m+g<=100", side="near", inside=True, sc=_sc(20, -30, 0, -10, -4)),
    dict(term="n+m+g<=100", side="eq", inside=False, sc=_sc(2, -62, 1, -32, -2)),
    dict(term="n+m+g<=100", side="over", inside=False, sc=_sc(2, -62, 1, -33, -2)),
    dict(term="min(X,-g)-1-m-g>=-100", side="near", inside=True, sc=_sc(39, -43, 1, 0, -1, T=5)),
    dict(term="min(X,-g)-1-m-g>=-100", side="eq", inside=False, sc=_sc(2, -62, 1, -31, -2)),
    dict(term="min(X,-g)-1-m-g>=-100", side="over", inside=False, sc=_sc(2, -62, 1, -30, -4)),
    dict(term="(bw/16)ge<=60", side="eq", inside=True, sc=_sc(2, -6, 1, -2, -10), bw=96),
    dict(term="(bw/16)ge<=60", side="over", inside=False, sc=_sc(2, -6, 1, -2, -11), bw=96, gen=True),
    dict(term="(bw/16)ge<=60", side="eq", inside=True, sc=_sc(2, -6, 1, -3, -4), bw=240),
    dict(term="(bw/16)ge<=60", side="over", inside=False, sc=_sc(2, -6, 1, -3, -4), bw=256, gen=True),
    dict(term="gape1<=gape2", side="eq", inside=True, sc=_sc(2, -6, 1, -3, -2, -8, -2)),
    dict(term="gape1<=gape2", side="over", inside=True, sc=_sc(2, -6, 1, -3, -2, -8, -3)),
    dict(term="refbonus>=0", side="eq", inside=True, sc=_sc(2, -6, 0, -3, -2, -8, -1)),
    dict(term="refbonus>=0", side="over", inside=False, sc=_sc(2, -6, -1, -3, -2, -8, -1)),
]


def sweep_params(p, bandwidth):
    import bsalign_amd as B
    sp = B.SweepParams()
    sp.rows = B.RowsParams(int(p["alnmode"]), int(bandwidth), p["M"], p["X"], p["refbonus"], p["O"], p["E"], p["Q"], p["P"])
    sp.T = int(p["T"])
    return sp


def _lib():
    import bsalign_amd as B
    L = B.lib()
    L.bsa_poa_graph_gen_supported.argtypes = [C.POINTER(B.SweepParams)]
    L.bsa_poa_graph_gen_supported.restype = C.c_int
    L.bsa_poa_graph_supported.restype = C.c_int
    return L


def wf_supported(sc, bw, slen=2000, mode=1):
    """bsa_poa_graph_supported: the number of ring rows (> 0) when k_poa_wf takes the scoring at this width and read length"""
    return int(_lib().bsa_poa_graph_supported(C.byref(sweep_params(dict(sc, alnmode=mode), bw)), int(slen)))


def gen_supported(sc, bw, mode=1):
    return int(_lib().bsa_poa_graph_gen_supported(C.byref(sweep_params(dict(sc, alnmode=mode), bw))))


def piecewise(sc, bw):
    return int(S.oracle().orc_get_piecewise(sc["O"], sc["E"], sc["Q"], sc["P"], (int(bw) + 15) // 16 * 16))


def full_par(sc, mode):
    return P.par(alnmode=mode, **sc)


def sc_str(sc):
    return "M=%(M)d X=%(X)d refbonus=%(refbonus)d O=%(O)d E=%(E)d Q=%(Q)d P=%(P)d T=%(T)d" % sc


@functools.lru_cache(maxsize=None)
def drawn(seed=4242, n=400):
    rng = np.random.default_rng(seed)
    return tuple(draw_scoring(rng) for _ in range(n))


@functools.lru_cache(maxsize=None)
def scorings_for(pw, bw, wide=False):
    """three scorings of gap model `pw` that the library takes at this width (k_poa_wf, or k_poa_gen alone for `wide`): the first one from BOUNDARY
    (an `eq` / `near` entry), two drawn.  Deterministic."""
    ok = (lambda sc: gen_supported(sc, bw) == 1 and wf_supported(sc, bw) == 0) if wide else (lambda sc: wf_supported(sc, bw) > 0)
    edge = [b["sc"] for b in BOUNDARY if b["inside"] and b.get("bw", bw) == bw and piecewise(b["sc"], bw) == pw and ok(b["sc"])]
    assert edge, ("no boundary scoring for", pw, bw)
    rest = [sc for sc in drawn() if piecewise(sc, bw) == pw and ok(sc)]
    assert len(rest) >= 2, ("too few drawn scorings for", pw, bw)
    k = (bw // 16 + pw) % len(edge)
    j = (bw // 16) % (len(rest) - 1)
    return (edge[k], rest[j], rest[j + 1])


MODES = (0, 1, 2)


def width_term_cases():
    """the equality scorings of k_poa_wf's width term (bw / 16) x ge <= 60, each at the width it is stated for (240 columns is no NARROW_BW width)"""
    return [(b["bw"], b["sc"]) for b in BOUNDARY if b["term"] == "(bw/16)ge<=60" and b["inside"]]


def narrow_cases():
    """every (gap model, bandwidth, mode, scoring) the GPU tests launch over narrow_set(bandwidth)"""
    for pw in (0, 1, 2):
        for bw in NARROW_BW:
            for mode in MODES:
                for sc in scorings_for(pw, bw):
                    yield pw, bw, mode, sc
    for bw, sc in width_term_cases():
        for mode in MODES:
            yield piecewise(sc, bw), bw, mode, sc


def wide_cases():
    """every (gap model, columns, nodes, mode, scoring, variant) of the k_poa_gen tests: per instantiation two modes, each with a scoring of its own"""
    for pw in (0, 1, 2):
        for i, (bw, nn, c) in enumerate(WIDE):
            scs = scorings_for(pw, bw, wide=True)
            for j, mode in enumerate(((0, 1), (1, 2), (2, 0))[(i + pw) % 3]):
                yield pw, bw, nn, c, mode, scs[(i + j) % 3], j


# ---- the oracle on one program ---------------------------------------------------------------------------------------------------------
def oracle_run(pg, p, want_trace=True):
    """scalar statement: rows, u0, best end cell, walk (n < 0: the reference's own walk does not end on this input)"""
    nodes, edges, cands, blocks = graph_of(pg)
    bw = pg["bandwidth"]
    rows, u0 = P.oracle_wf_forward(nodes, pg["query"], p, bw)
    best = P.oracle_wf_best(nodes, cands, pg["slen"], p, bw, rows)
    out = dict(rows=rows, u0=u0, best=(int(best["maxscr"]), int(best["maxidx"]), int(best["maxoff"])))
    if want_trace:
        if best["maxidx"] < 0:          # (every candidate's row is dead: no walk; the device reports BSA_POA_ST_NOCAND)
            out.update(n=-3, ev=np.zeros(0, P.WF_EVENT), fin=(-1, -1))
            return out
        n, ev, fin = P.oracle_wf_trace(nodes, edges, pg["query"], p, bw, rows, u0, 0, int(best["maxidx"]), int(best["maxoff"]))
        assert n != -2
        out.update(n=int(n), ev=ev.copy(), fin=(int(fin[0]), int(fin[1])))
    return out


def lane_exact_check(pg, p, what="", recorded=False):
    """guard soundness on one program: the absolute-score statement, converted into the reference's row blocks, equals the lane-exact int8 rows
    byte for byte over the used part of every real block, and the best end cells agree (tests/test_oracle_wf.py::_check without the hash).
    recorded: a program of tests/golden/poa_sweep.npz, which carries no seed to validate and draw coverages by"""
    nodes, edges, cands, blocks = P.tasks_to_graph(pg["tasks"]) if recorded else graph_of(pg)
    bw, slen, nb = int(pg["bandwidth"]), int(pg["slen"]), int(pg["nblocks"])
    pw = piecewise(p, bw)
    rows, u0 = P.oracle_wf_forward(nodes, pg["query"], p, bw)
    mine = P.wf_rows_to_blocks(rows, u0, blocks, nb, bw, pw)
    t = pg["tasks"].copy(); t["query"] = 0
    orows, ores = P.oracle_sweep(t, np.array([(0, len(t), 0, 0)], dtype=P.PROG_DTYPE), pg["query"], np.zeros(1, np.uint64), np.array([slen], np.uint32), p, bw, nb, pw)
    blk, used = P.block_bytes(bw, pw), bw * (pw + 1) + 68
    real = blocks[blocks != 0]
    a, b = mine.reshape(nb, blk)[real, :used], orows.reshape(nb, blk)[real, :used]
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, "%s [%s] bw %d: row of block %d differs from the lane-exact rows, first byte %d" % (what, sc_str(p), bw, real[bad[0]], np.nonzero(a[bad[0]] != b[bad[0]])[0][0])
    best = P.oracle_wf_best(nodes, cands, slen, p, bw, rows)
    gidx = int(nodes[int(best["maxidx"])]["gnode"]) if best["maxidx"] >= 0 else -1
    want = (int(ores[0]["maxscr"]), int(ores[0]["maxidx"]), int(ores[0]["maxoff"]))
    assert (int(best["maxscr"]), gidx, int(best["maxoff"])) == want, "%s [%s] bw %d: best end cell %r, lane-exact %r" % (what, sc_str(p), bw, (int(best["maxscr"]), gidx, int(best["maxoff"])), want)


# ---- named programs of single tests (the CPU file runs the oracle's walk on every one of them) -------------------------------------------
def group_programs():
    """test_row_budget_groups: four small programs and one large one at 704 columns, the large one in the middle"""
    bw = 704
    small = [generate(WIDE_SEED, 100 + k, bw, 150 + 20 * k, slen_target=bw + 150, noise=False, wild=False, long_branch=True) for k in range(4)]
    big = generate(WIDE_SEED, 200, bw, 900, slen_target=bw + 300, noise=False, wild=False, long_branch=True)
    return [small[2], small[3], big, small[0], small[1]]


def program_272():
    """a width k_poa_wf does not have"""
    return generate(WIDE_SEED, 300, 272, 300, slen_target=500, noise=False, wild=False)


LDS_SLEN = 300000


def program_lds():
    """256 columns, which k_poa_wf has, and a read so long that its profile leaves no room for any ring in LDS: bsa_poa_graph_supported says 0 for the
    length alone.  The path lies at the read's start, the rest trails"""
    return generate(WIDE_SEED, 301, 256, 400, slen_target=LDS_SLEN, noise=False, wild=False, jumpy=False, pre_frac=0.0)


DEAD_SC, DEAD_MODE = _sc(1, -13, 2, 0, -5, T=0), 0


def program_dead():
    """REGRESSION (k_poa_wf): every end candidate on a dead row.  The third node's band jumps by more than the band's width, so its row and every row
    after it is dead (bspoa.h:2253-2259); the one candidate, on the last node, scores at or below SCORE_MIN.  The reference starts at SCORE_MIN and takes a
    candidate only when strictly greater: no best end cell, no walk.  k_poa_wf used to report that candidate (first seen in a random program at 96 columns
    with this scoring in global mode)"""
    bw, slen = 96, 260
    rng = np.random.default_rng(96)
    t = [(2, 0, HEAD, 0, 0, 0, 0, 0, 0, 0), (0, 2, 3, 0, 0, 1, 0, 1, 0, 0), (0, 3, 4, 0, 1, 2, 0, 2, 1, 0), (0, 4, 5, 1, 1 + bw + 8, 3, 0, 3, 0, 0)]
    r = 1 + bw + 8
    for k in range(6, 14):
        t.append((0, k - 1, k, r, r + 1, k - 2, 0, k & 3, k & 1, 0)); r += 1
    t.append((3, 13, 0, r, 0, 1013, 0, 0, 0, 0))
    return dict(tasks=np.array(t, dtype=P.TASK_DTYPE), query=rng.integers(0, 4, size=slen).astype(np.uint8), slen=slen, bandwidth=bw, nblocks=14, seed=96, index=0,
                noise=True, wild=False, jumpy=True, short=False, long_branch=False, mode_hint=0)
