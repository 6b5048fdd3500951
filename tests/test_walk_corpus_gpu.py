"""GPU parity of every traceback walker on the corpus of walk_cases.py: record fields, status and every CIGAR word against the CPU oracle, bit for bit.

The pairs aim at the walkers' slow paths -- insertions that open outside a code window, deletion runs that outlive it (up to 150 rows in a moving band,
300 in a whole-query band, so whole tiles of 64 rows without a match column), the same run at every phase of a tile and of the query window's refill,
62 .. 129 CIGAR tokens with a long run as the token that is held back across a flush, I and D runs with no match between them, paths on the first
column of the band for hundreds of rows, and leading and trailing runs of 60 and 300 in the three modes.  test_walk_corpus_cpu.py shows on the oracle
alone that the batches hold all that.

One test covers one (walker, bandwidth) and loops over scorings and groups.  Each asserts the traceback kernel's name and that NO pair was handed over
to the literal kernels (ctx.last_handover() == 0): a code walker that gives up on a long gap would otherwise pass every parity test, the literal
kernels answering for it.  The one batch made of the pairs a code walker declines by design (walk_cases.decline) asserts the opposite: as many
hand-overs as the list is long.  The knobs are set before the call; every plan is made after them.
Sweep density: step 7 at every bandwidth (no test needed the fallback to step 9)."""
import numpy as np
import pytest

import support as S
import walk_cases as W

pytestmark = pytest.mark.gpu


def _fields(rec):
    return np.array([rec[f] for f in rec.dtype.names], dtype=np.int32)


def _align(ctx, cases, mode, scname, bw):
    """-> (trace kernel, forward kernel, hand-overs); every pair equal to the oracle"""
    import bsalign_amd as B
    out, cigs, status = ctx.align_batch([(c.q, c.t) for c in cases], B.make_params(mode, bw, *W.SC[scname]))
    names, handed = ctx.last_kernel_names(), ctx.last_handover()
    assert len(status) == len(cases) == len(cigs)
    bad = []
    for k, c in enumerate(cases):
        res, cig, n, _ = W.oracle(c, mode, scname, bw)
        if not (n >= 0 and status[k] == 0 and np.array_equal(_fields(out[k]), res) and np.array_equal(cigs[k], cig)):
            bad.append("%s status %d\n  gpu %s %s\n  orc %s %s" % (c.name, status[k], _fields(out[k]), S.cigar_str(cigs[k])[:100], res, S.cigar_str(cig)[:100]))
    assert not bad, "%d/%d pairs differ (mode %d bw %d %s, %s / %s, %d handed over)\n%s" % (
        len(bad), len(cases), mode, bw, scname, names[0], names[1], handed, "\n".join(bad[:6]))
    return names[1], names[0], handed


def _run_align(ctx, bw, scnames, walker, modes=W.MODES):
    for scname in scnames:
        for mode in modes:
            trace, fwd, handed = _align(ctx, W.cases(bw, scname, mode), mode, scname, bw)
            assert trace == walker.get(scname, walker[""]), (trace, fwd, scname, mode, bw)
            assert handed == 0, (handed, trace, scname, mode, bw)
        named = W.decline(bw, scname)
        if named:
            trace, fwd, handed = _align(ctx, named, W.G, scname, bw)
            assert trace == walker.get(scname, walker[""]) and handed == len(named), (handed, len(named), trace, scname, bw)


ONE_PIECE = ("affine", "go4", "linear")
TWO_PIECE = ("twopiece", "twopiece19", "twopiece23")


@pytest.mark.parametrize("bw", [64, 128, 256])
def test_trace_codes_wave(ctx, monkeypatch, bw):
    """k_align8_trace_codes_wave<4 | 8 | 8,1 | 16>: default dispatch; at bandwidth 128 -gapo 3 takes code format 1 (two-bit D / Od fields, the benchmark's
    path), -gapo 4 and linear gaps the four planes"""
    for knob in ("BSA_ALIGN8_TRACE_WAVE", "BSA_ALIGN8_TRACE_SIMPLE", "BSA_ALIGN8_LITERAL"):
        monkeypatch.delenv(knob, raising=False)
    _run_align(ctx, bw, ONE_PIECE, {"": "k_align8_trace_codes_wave"})
    if bw == 128:
        for scname in ("affine", "go4"):
            trace, fwd, handed = _align(ctx, W.long_gap(bw, scname), W.G, scname, bw)
            assert ("two-bit" in fwd) == (scname == "affine"), (scname, fwd)


@pytest.mark.parametrize("bw", [64, 128, 256])
def test_trace_codes_pair_per_lane(ctx, monkeypatch, bw):
    """BSA_ALIGN8_TRACE_WAVE=0: k_align8_trace_codes_lds<4 | 8> (ring of 32 rows, serviced every 8 steps) at 64 / 128, k_align8_trace_codes_simple<16> at 256"""
    monkeypatch.setenv("BSA_ALIGN8_TRACE_WAVE", "0")
    _run_align(ctx, bw, ONE_PIECE, {"": "k_align8_trace_codes_simple" if bw == 256 else "k_align8_trace_codes_lds"})


@pytest.mark.parametrize("bw", [64, 128])
def test_trace_codes_simple(ctx, monkeypatch, bw):
    """BSA_ALIGN8_TRACE_SIMPLE=1: k_align8_trace_codes_simple<4 | 8>"""
    monkeypatch.setenv("BSA_ALIGN8_TRACE_SIMPLE", "1")
    _run_align(ctx, bw, ONE_PIECE, {"": "k_align8_trace_codes_simple"})


@pytest.mark.parametrize("bw,wave", [(128, "1"), (64, "1"), (256, "1"), (128, "0")])
def test_trace_codes2(ctx, monkeypatch, bw, wave):
    """two-piece gaps: k_align8_trace_codes2_wave at 128, k_align8_trace_codes2<4 | 16> at 64 / 256 and <8> at 128 with BSA_ALIGN8_TRACE_WAVE=0; the batch of
    pairs decided at query column 0 is the one that is handed over.  (2, -6, -3, -2, -8, -1) and (2, -6, -6, -2, -19, -1) run these walkers;
    (2, -6, -6, -2, -23, -1) lies outside the compact path's guard (m + 3 g = 74 > 64, bsa_align8_x_supported), so a banded batch under it runs the
    row-record kernels: the same pairs, the literal traceback's name, and nothing to hand over"""
    if wave == "0":
        monkeypatch.setenv("BSA_ALIGN8_TRACE_WAVE", "0")
    else:
        monkeypatch.delenv("BSA_ALIGN8_TRACE_WAVE", raising=False)
    _run_align(ctx, bw, TWO_PIECE, {"": "k_align8_trace_codes2_wave" if (bw, wave) == (128, "1") else "k_align8_trace_codes2", "twopiece23": "k_align8_backcal"})


@pytest.mark.parametrize("trace1", ["0", "1"])
def test_literal_row_records(ctx, monkeypatch, trace1):
    """BSA_ALIGN8_LITERAL=1: the row-record traceback, two waves a walk and (BSA_ALIGN8_TRACE1=1) one; it declines nothing, the named list included"""
    monkeypatch.setenv("BSA_ALIGN8_LITERAL", "1")
    if trace1 == "1":
        monkeypatch.setenv("BSA_ALIGN8_TRACE1", "1")
    else:
        monkeypatch.delenv("BSA_ALIGN8_TRACE1", raising=False)
    for scname in ("affine", "linear", "twopiece"):
        for mode in W.MODES:
            trace, fwd, handed = _align(ctx, W.cases(128, scname, mode) + (W.decline(128, scname) if mode == W.G else []), mode, scname, 128)
            assert trace == "k_align8_backcal" and handed == 0, (trace, fwd, handed, scname, mode)


@pytest.mark.parametrize("how", ["lane", "wave"])
def test_trace_sys_whole_query_bands(ctx, monkeypatch, how):
    """bandwidth 0, queries above 256 bases: k_align8_trace_sys<., WAVE> with runs of up to 300; the benchmark's scoring, and one outside the static guard
    (k_align8_fwd_sys<CHK>)"""
    monkeypatch.setenv("BSA_ALIGN8_SYS_TRACE", how)
    for scname in ("affine", "chk"):
        for mode in W.MODES:
            cases = W.cases(0, scname, mode)
            assert all(len(c.q) > 256 for c in cases)
            trace, fwd, handed = _align(ctx, cases, mode, scname, 0)
            assert trace == "k_align8_trace_sys" and ("<CHK>" in fwd) == (scname == "chk") and "k_align8_fwd_sys" in fwd, (trace, fwd)
            assert handed == 0, (handed, scname, mode, how)


def _edit(ctx, cases, mode, bw):
    out, cigs, status = ctx.edit_batch([(c.q, c.t) for c in cases], mode, bw)
    names = ctx.last_kernel_names()
    bad = []
    for k, c in enumerate(cases):
        res, cig, n, _ = W.oracle(c, mode, "edit", bw)
        if not (n >= 0 and status[k] == 0 and np.array_equal(_fields(out[k]), res) and np.array_equal(cigs[k], cig)):
            bad.append("%s status %d\n  gpu %s %s\n  orc %s %s" % (c.name, status[k], _fields(out[k]), S.cigar_str(cigs[k])[:100], res, S.cigar_str(cig)[:100]))
    assert not bad, "%d/%d pairs differ (edit, mode %d bw %d, %s / %s)\n%s" % (len(bad), len(cases), mode, bw, names[0], names[1], "\n".join(bad[:6]))
    return names[1], names[0]


EDIT_WALKERS = {
    "default": ({}, "k_edit_trace_wave"),
    "wave": ({"BSA_EDIT_TRACE_WAVE": "1"}, "k_edit_trace_wave"),
    "wave-untiled": ({"BSA_EDIT_TRACE_WAVE": "1", "BSA_EDIT_TILED": "0"}, "k_edit_trace_wave"),
    "lane": ({"BSA_EDIT_TRACE_WAVE": "0", "BSA_EDIT_TRACE_COOP": "0"}, "k_edit_trace"),
    "coop": ({"BSA_EDIT_TRACE_WAVE": "0", "BSA_EDIT_TRACE_COOP": "1"}, "k_edit_trace"),
    "lanes16": ({"BSA_EDIT_TRACE_LANES": "16"}, "k_edit_trace"),
}


@pytest.mark.parametrize("bw", [64, 128, 256, 0])
@pytest.mark.parametrize("walker", list(EDIT_WALKERS))
def test_edit_walkers(ctx, monkeypatch, walker, bw):
    """k_edit_trace_wave<TILED> (default dispatch: three dwords a row of the tiled format at 64 / 128 / 256; BSA_EDIT_TRACE_WAVE=1: rows as they are, with
    and without BSA_EDIT_TILED=0) and k_edit_trace<COOP> (64-column ring window; plain, cooperative, 16 pairs a wave).  Bandwidth 0 is the band of a
    1300-base query: wider than the 256 columns the wave walker keeps around the diagonal.  All groups in global mode, the overhangs in all three"""
    for knob in ("BSA_EDIT_TRACE_WAVE", "BSA_EDIT_TILED", "BSA_EDIT_TRACE_COOP", "BSA_EDIT_TRACE_LANES", "BSA_EDIT_GRP", "BSA_EDIT_GRP32", "BSA_EDIT_FWD_LANES"):
        monkeypatch.delenv(knob, raising=False)
    env, want = EDIT_WALKERS[walker]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for mode in W.MODES:
        trace, fwd = _edit(ctx, W.cases(bw, "edit", mode), mode, bw)
        assert trace.split(" ")[0] == want, (trace, fwd, walker, mode, bw)
    if walker == "default" and bw:
        # one launch class at this width (test_edit_gpu.test_rows_tiled_eight_at_a_time): the forward kernel and the walker share the tiled rows
        cases = [c for c in W.cases(bw, "edit", W.G) if len(c.q) > bw and (len(c.q) + len(c.t) - 1) // len(c.t) + 1 <= bw]
        assert len(cases) > 100
        trace, fwd = _edit(ctx, cases, W.G, bw)
        assert "tiled" in trace and "tiled" in fwd, (trace, fwd)
