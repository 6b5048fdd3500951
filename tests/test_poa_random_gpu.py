"""GPU parity of the two POA graph kernels (k_poa_wf, bsa_poa_wf.hip; k_poa_gen, bsa_poa_gen.hip) on the random programs, scorings and guard
boundary of tests/poa_random.py, all through bsa_poa_graph_host.  Every program is validated and run through the scalar statement
(oracle/bsalign_oracle_wf.c) before it goes to the device; then: best end cell, status == 0 exactly when the oracle's walk ends, every step and the
walk's end with the same random coverages, and for k_poa_wf every row cell and u0 byte for byte."""
import functools

import numpy as np
import pytest

import poa_random as R
import poa_support as P

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=256)
def _oracle(kind, bw, key, mode, sct):
    """the scalar statement on narrow_set(bw) / wide_program(bw, *key), once per (programs, mode, scoring)"""
    p = R.full_par(dict(sct), mode)
    pgs = R.narrow_set(bw) if kind == "narrow" else [R.wide_program(bw, *key)]
    return [R.oracle_run(pg, p) for pg in pgs]


def _pack(pgs):
    N, E, Cd, Q, PR = [], [], [], [], np.zeros(len(pgs), P.WF_PROG)
    n0 = e0 = c0 = q0 = v0 = 0
    for k, pg in enumerate(pgs):
        nodes, edges, cands, _ = R.graph_of(pg)
        cap = 4 * (pg["slen"] + len(nodes)) + 64
        PR[k] = (n0, len(nodes), e0, len(edges), c0, len(cands), pg["slen"], cap, q0, v0)
        N.append(nodes); E.append(edges); Cd.append(cands); Q.append(pg["query"])
        n0 += len(nodes); e0 += len(edges); c0 += len(cands); q0 += pg["slen"]; v0 += cap
    return np.concatenate(N), np.concatenate(E), np.concatenate(Cd), PR, np.concatenate(Q), v0


def _launch(ctx, pgs, sc, mode, bw, want_rows):
    nodes, edges, cands, PR, Q, cap = _pack(pgs)
    res, ev, rows, u0 = ctx.poa_graph_host(nodes, edges, cands, PR, Q, R.sweep_params(dict(sc, alnmode=mode), bw), cap, want_rows=want_rows)
    return res, ev, rows, u0, PR


def _compare(pgs, want, got, sc, mode, what, rows=True):
    """-> number of walks that ended.  Messages name seed, index, scoring and the first differing node and cell"""
    res, ev, drows, du0, PR = got
    ended = 0
    for k, (pg, o) in enumerate(zip(pgs, want)):
        tag = "%s: seed %d index %d bw %d mode %d [%s]" % (what, pg["seed"], pg["index"], pg["bandwidth"], mode, R.sc_str(sc))
        r, pr = res[k], PR[k]
        n0, nn = int(pr["first_node"]), int(pr["nnodes"])
        if rows:
            a, b = drows[n0:n0 + nn].view(np.uint64), o["rows"].view(np.uint64)
            bad = np.nonzero((a != b).any(axis=1))[0]
            assert len(bad) == 0, (tag, "first differing node", int(bad[0]), "of", nn, "cell", int(np.nonzero(a[bad[0]] != b[bad[0]])[0][0]),
                                   "device", drows[n0 + bad[0]][int(np.nonzero(a[bad[0]] != b[bad[0]])[0][0])], "oracle", o["rows"][bad[0]][int(np.nonzero(a[bad[0]] != b[bad[0]])[0][0])])
            assert np.array_equal(du0[n0:n0 + nn], o["u0"]), (tag, "u0 of node", int(np.nonzero(du0[n0:n0 + nn] != o["u0"])[0][0]))
        assert (int(r["maxscr"]), int(r["maxidx"]), int(r["maxoff"])) == o["best"], (tag, "best end cell", (int(r["maxscr"]), int(r["maxidx"]), int(r["maxoff"])), o["best"])
        assert (int(r["status"]) == 0) == (o["n"] >= 0), (tag, "status", int(r["status"]), "oracle walk", o["n"])
        if o["n"] >= 0:
            mine = ev[int(pr["first_event"]):int(pr["first_event"]) + int(r["nevents"])]
            assert int(r["nevents"]) == o["n"], (tag, "nevents", int(r["nevents"]), o["n"])
            for f in ("node", "x", "bt"):
                d = np.nonzero(mine[f] != o["ev"][f])[0]
                assert len(d) == 0, (tag, "step", int(d[0]), f, "device", mine[int(d[0])], "oracle", o["ev"][int(d[0])])
            assert (int(r["fin_node"]), int(r["fin_x"])) == o["fin"], (tag, "walk's end", (int(r["fin_node"]), int(r["fin_x"])), o["fin"])
            ended += 1
    return ended


def _same_results(a, b):
    """two launches of the same programs: best end cell and status of every program; of every walk that ended its steps and its end (what a kernel
    leaves in the other fields of a walk that did not end is its own business)"""
    (ra, eva, _, _, PR), (rb, evb, _, _, _) = a, b
    for f in ("maxscr", "maxidx", "maxoff"):
        assert np.array_equal(ra[f], rb[f]), f
    assert np.array_equal(ra["status"] == 0, rb["status"] == 0)
    for k in np.nonzero(ra["status"] == 0)[0]:
        assert (int(ra[k]["nevents"]), int(ra[k]["fin_node"]), int(ra[k]["fin_x"])) == (int(rb[k]["nevents"]), int(rb[k]["fin_node"]), int(rb[k]["fin_x"])), int(k)
        e0, n = int(PR[k]["first_event"]), int(ra[k]["nevents"])
        assert np.array_equal(eva[e0:e0 + n], evb[e0:e0 + n]), int(k)


def _wf_name(pw, bw, rows_pass=True):
    """the instantiation bsa_poa_graph_run reports through bsa_ctx_last_kernel_name: ROWS 0 for the wavefront pass, else the 64-cell pieces of a row"""
    return "k_poa_wf<%d, %d>" % (pw, (1 if bw <= 64 else 2 if bw <= 128 else 4) if rows_pass else 0)


def _gen_name(pw, c, groups=1):
    return "k_poa_gen<%d, %d> x %d" % (pw, c, groups)


def _narrow(ctx, pw, bw, mode, sc, what, want_rows=True, kernel=None):
    pgs = R.narrow_set(bw)
    assert len(pgs) >= 64 and R.piecewise(sc, bw) == pw
    want = _oracle("narrow", bw, None, mode, tuple(sorted(sc.items())))
    got = _launch(ctx, pgs, sc, mode, bw, want_rows)
    assert ctx.last_kernel_names()[0] == (kernel or _wf_name(pw, bw)), (what, ctx.last_kernel_names())
    ended = _compare(pgs, want, got, sc, mode, what, rows=want_rows)
    assert ended >= len(pgs) * 0.95          # (tests/test_poa_random_cpu.py asserts this cap for the oracle alone)
    return got


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("bw", R.NARROW_BW)
@pytest.mark.parametrize("pw", [0, 1, 2])
def test_k_poa_wf_every_instantiation(ctx, pw, bw, mode):
    """k_poa_wf<PW, ROWS>: PW through the gap model, ROWS 1 / 2 / 4 through the bandwidth (widths that are no power of two among them), three modes;
    64 programs of mixed length side by side in one launch; three in-guard scorings, the first from the guard's boundary"""
    for sc in R.scorings_for(pw, bw):
        assert R.wf_supported(sc, bw, max(pg["slen"] for pg in R.narrow_set(bw)), mode) > 0
        _narrow(ctx, pw, bw, mode, sc, "k_poa_wf")


def test_k_poa_wf_width_term_at_equality(ctx):
    """(bw / 16) x ge = 60 at the widths the boundary list states it for (96 and 240 columns), every mode"""
    cases = R.width_term_cases()
    assert sorted(bw for bw, _ in cases) == [96, 240]
    for bw, sc in cases:
        for mode in R.MODES:
            assert R.wf_supported(sc, bw, max(pg["slen"] for pg in R.narrow_set(bw)), mode) > 0
            _narrow(ctx, R.piecewise(sc, bw), bw, mode, sc, "k_poa_wf, width term met with equality")


def _first(pw, bw):
    return R.scorings_for(pw, bw)[(pw + bw // 16) % 3]


@pytest.mark.parametrize("bw", [32, 96, 176, 256])
@pytest.mark.parametrize("pw", [0, 1, 2])
def test_both_forward_passes_and_the_ring(ctx, pw, bw, monkeypatch):
    """the anti-diagonal wavefront (BSA_POA_FWD=wf: k_poa_wf<PW, 0>) and the row-at-a-time pass with rings of 2 and 16 rows give the rows, results and
    steps of the default launch (ring 16 for a launch of this size, 8 for thousands of programs).  The programs generated with long_branch have one
    bubble whose second branch holds 34 - 50 nodes, emitted after the first: the merge's first input lies more than 32 nodes back in completion order
    (asserted), so the read-back from HBM runs at ring 8 and 16 without any knob"""
    sc, mode = _first(pw, bw), (pw + bw // 16) % 3
    assert sum(R.max_input_distance(pg) > 16 for pg in R.narrow_set(bw)) >= 8
    base = _narrow(ctx, pw, bw, mode, sc, "default")
    for env in (("BSA_POA_FWD", "wf"), ("BSA_POA_FWD_RING", "2"), ("BSA_POA_FWD_RING", "16"), ("BSA_POA_FWD_RING", "8")):
        with monkeypatch.context() as m:
            m.setenv(*env)
            got = _narrow(ctx, pw, bw, mode, sc, "%s=%s" % env, kernel=_wf_name(pw, bw, rows_pass=env[0] != "BSA_POA_FWD"))
        _same_results(got, base)
        assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3]), env


@pytest.mark.parametrize("shift", [40, -40])
@pytest.mark.parametrize("bw", [16, 64, 128, 256])
def test_walk_windows_off_their_place(ctx, bw, shift, monkeypatch):
    """BSA_POA_WIN_SHIFT: the traceback's row windows that many cells off their place, random coverages (ties among the in-edges): same steps"""
    pw = (bw // 16) % 3
    sc, mode = _first(pw, bw), (bw // 32) % 3
    monkeypatch.setenv("BSA_POA_WIN_SHIFT", str(shift))
    _narrow(ctx, pw, bw, mode, sc, "BSA_POA_WIN_SHIFT=%d" % shift)


@pytest.mark.parametrize("bw", [16, 96, 256])
@pytest.mark.parametrize("pw", [0, 1, 2])
def test_k_poa_gen_on_the_narrow_programs_equals_k_poa_wf(ctx, pw, bw, monkeypatch):
    """BSA_POA_FORCE_GEN=1 on the programs of the first test: one cell a thread, several programs side by side; results and steps equal the oracle's
    and k_poa_wf's"""
    sc, mode = R.scorings_for(pw, bw)[0], (pw + 1) % 3
    base = _narrow(ctx, pw, bw, mode, sc, "k_poa_wf", want_rows=False)
    monkeypatch.setenv("BSA_POA_FORCE_GEN", "1")
    got = _narrow(ctx, pw, bw, mode, sc, "k_poa_gen forced", want_rows=False, kernel=_gen_name(pw, 1))
    _same_results(got, base)


@pytest.mark.parametrize("bw,nn,c", R.WIDE)
@pytest.mark.parametrize("pw", [0, 1, 2])
def test_k_poa_gen_every_instantiation_over_branching_graphs(ctx, pw, bw, nn, c):
    """k_poa_gen<PW, C>: C = 1 ... 32 cells a thread through bands of 704 ... 18 000 columns, three gap models, two modes each: programs with branches,
    merges of up to five inputs, moved rows and a read of the band's size"""
    n = 0
    for pw_, bw_, nn_, c_, mode, sc, variant in R.wide_cases():
        if (pw_, bw_) != (pw, bw):
            continue
        pg = R.wide_program(bw, nn, variant)
        assert R.piecewise(sc, bw) == pw and (bw + 1023) // 1024 <= c and R.wf_supported(sc, bw, pg["slen"], mode) == 0 and R.gen_supported(sc, bw, mode) == 1
        want = _oracle("wide", bw, (nn, variant), mode, tuple(sorted(sc.items())))
        assert want[0]["n"] > 0
        got = _launch(ctx, [pg], sc, mode, bw, False)
        assert ctx.last_kernel_names()[0] == _gen_name(pw, c), ctx.last_kernel_names()
        assert _compare([pg], want, got, sc, mode, "k_poa_gen C=%d" % c, rows=False) == 1
        n += 1
    assert n == 2


def test_row_budget_groups(ctx, monkeypatch):
    """BSA_POA_GEN_WS_GB so small that one call of five wide programs splits into three launches, the middle one a single program above the budget:
    the results and steps of the unsplit call.  The value comes from the programs' nnodes x (bw x 8 + 4) bytes of rows; the number of launches is
    the library's own count (bsa_ctx_last_kernel_name: "... x 3"), one for the unsplit call"""
    bw, sc, mode = 704, R.scorings_for(2, 704, wide=True)[1], 1
    pgs = R.group_programs()
    p = R.full_par(sc, mode)
    want = [R.oracle_run(pg, p) for pg in pgs]                      # (graph_of validates)
    nn = [len(R.graph_of(pg)[0]) for pg in pgs]
    rowb = bw * 8 + 4
    budget = (nn[0] + nn[1]) * rowb + rowb // 2
    assert nn[2] * rowb > budget and (nn[3] + nn[4]) * rowb <= budget and (nn[0] + nn[1] + nn[2]) * rowb > budget
    assert R.gen_supported(sc, bw, mode) == 1 and R.wf_supported(sc, bw, 2000, mode) == 0
    whole = _launch(ctx, pgs, sc, mode, bw, False)
    assert ctx.last_kernel_names()[0] == _gen_name(2, 1, 1)
    assert _compare(pgs, want, whole, sc, mode, "unsplit", rows=False) == len(pgs)
    monkeypatch.setenv("BSA_POA_GEN_WS_GB", repr(budget / 1073741824.0))
    split = _launch(ctx, pgs, sc, mode, bw, False)
    assert ctx.last_kernel_names()[0] == _gen_name(2, 1, 3), ctx.last_kernel_names()
    assert _compare(pgs, want, split, sc, mode, "three groups", rows=False) == len(pgs)
    _same_results(split, whole)


def test_outside_the_guard_is_refused(ctx):
    """every boundary scoring on the outside, the regression scorings and a few drawn ones: BSA_E_UNSUPPORTED, raised as BsaError, no result"""
    import bsalign_amd as B
    outs = [(b["sc"], b.get("bw", 128)) for b in R.BOUNDARY if not b["inside"] and not b.get("gen")]
    outs += [(sc, 128) for sc in R.REGRESSION + R.REGRESSION_VERTICAL]
    outs += [(sc, 128) for sc in R.drawn() if R.gen_supported(sc, 128) == 0][:6]
    assert len(outs) >= 20
    for sc, bw in outs:
        pgs = R.narrow_set(bw if bw in R.NARROW_BW else 128)[:2]
        for pg in pgs:
            R.graph_of(pg)
        with pytest.raises(B.BsaError) as e:
            _launch(ctx, pgs, sc, 1, pgs[0]["bandwidth"], False)
        assert e.value.code == -6, (R.sc_str(sc), e.value.code)


def test_only_the_narrow_kernel_declines(ctx):
    """(bw / 16) x ge above 60, a width k_poa_wf does not have, a read whose profile leaves no LDS for its rings: the call goes through k_poa_gen and
    equals the oracle"""
    cases = [(b["sc"], b["bw"]) for b in R.BOUNDARY if b.get("gen")]
    assert len(cases) >= 2
    for sc, bw in cases:
        assert R.wf_supported(sc, bw) == 0 and R.gen_supported(sc, bw) == 1
        _narrow(ctx, R.piecewise(sc, bw), bw, 1, sc, "k_poa_gen behind a declined k_poa_wf", want_rows=False, kernel=_gen_name(R.piecewise(sc, bw), 1))
    sc = R.BOUNDARY[0]["sc"]
    for pg, mode, what in ((R.program_272(), 2, "272 columns"), (R.program_lds(), 1, "no LDS for a read of %d" % R.LDS_SLEN)):
        bw = pg["bandwidth"]
        want = [R.oracle_run(pg, R.full_par(sc, mode))]
        assert R.wf_supported(sc, bw, pg["slen"], mode) == 0 and R.gen_supported(sc, bw, mode) == 1
        assert bw > 256 or R.wf_supported(sc, bw, 2000, mode) > 0          # (declined for the read's length alone)
        got = _launch(ctx, [pg], sc, mode, bw, False)
        assert ctx.last_kernel_names()[0] == _gen_name(R.piecewise(sc, bw), 1)
        assert _compare([pg], want, got, sc, mode, what, rows=False) == 1


def test_regression_no_candidate_on_dead_rows(ctx, monkeypatch):
    """R.program_dead: the only end candidate sits on a dead row and scores at or below SCORE_MIN.  The reference takes none (strictly greater than its
    start value): status NOCAND (3), no best end cell, on k_poa_wf -- which used to report the candidate -- and on k_poa_gen"""
    pg, sc, mode = R.program_dead(), R.DEAD_SC, R.DEAD_MODE
    want = [R.oracle_run(pg, R.full_par(sc, mode))]
    assert want[0]["best"][1] < 0
    for force in (False, True):
        if force:
            monkeypatch.setenv("BSA_POA_FORCE_GEN", "1")
        got = _launch(ctx, [pg], sc, mode, pg["bandwidth"], not force)
        assert ctx.last_kernel_names()[0] == (_gen_name(0, 1) if force else _wf_name(0, 96))
        _compare([pg], want, got, sc, mode, "dead rows", rows=not force)
        r = got[0][0]
        assert (int(r["status"]), int(r["maxidx"]), int(r["maxoff"]), int(r["nevents"])) == (3, -1, -1, 0), r
