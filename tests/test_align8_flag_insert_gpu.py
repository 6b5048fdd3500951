"""GPU parity of the absolute-score forward DP (bsa_align8_x.hip, x_forward_abs) whose one-bit traceback flags are inserted from the high byte of a packed int16
difference: records, status and CIGAR words of every pair against the oracle, bit for bit, in the style of test_align8_m3_gpu.py (whose batches and oracle
answers are shared where the scoring is one of its own).

The insert is exact while the difference lies in 0 .. 256 (bsa_align8_flag_span), so the cases aim at large differences and at the cells a fix-up overwrites:
the largest m + n the guard admits, the largest |cfirst| (the cell entering behind the band end lies that far below its neighbour), the benchmark's scoring, a
scoring with -gapo = 4 (four planes at bandwidth 128: D and Od are one-bit flags), linear gaps (constant R and Od), bands that stay, move by two and more and
jump, many rows at rbeg = 0 (the first-cell rule, where cell 0 keeps the saturating comparison), queries shorter than the band (pad cells), both bandwidths,
the three modes, whole pairs and row segments.
(Overlap mode with match scores above 50 on pairs without a match is left out as in test_align8_m3_gpu.py: there the traceback and the oracle disagree
whichever forward kernel ran.)"""
import numpy as np
import pytest

import support as S
import test_align8_m3_gpu as T

pytestmark = pytest.mark.gpu

MODES = T.MODES
SCORINGS = dict(T.SCORINGS)
SCORINGS.update({
    "mn28": (28, -28, -1, -1, 0, 0),          # m + n = 56, the largest inside 63 + 2 ge + n + m + 2 g <= 125 with go, ge >= 1; cfirst = -33
    "cfirst61": (56, 0, -1, -1, 0, 0),        # cfirst = min(smin, -g) - 1 - smax - g = -61, the lowest with go, ge >= 1
})
_ORACLE = {}


def _oracle(tag, pairs, mode, scname, bw):
    if scname in T.SCORINGS:
        return T._oracle(tag, pairs, mode, scname, bw)
    key = (tag, mode, scname, bw)
    if key not in _ORACLE:
        _ORACLE[key] = [S.oracle_align(q, t, mode, bw, *SCORINGS[scname]) for q, t in pairs]
    return _ORACLE[key]


def _check(ctx, tag, mode, scname, bw):
    import bsalign_amd as B
    pairs = T._batch(tag)
    par = B.make_params(mode, bw, *SCORINGS[scname])
    span = B.align8_flag_span(par)[0]
    assert 0 < span <= 256, (scname, bw, span)          # the library's own guard takes the scoring, and the inserts are exact for it
    out, cigs, status = ctx.align_batch(pairs, par)
    fwd = ctx.last_kernel_names()[0]
    assert len(status) == len(pairs) == len(cigs)
    bad = []
    for k, ((q, t), (res, cig, n)) in enumerate(zip(pairs, _oracle(tag, pairs, mode, scname, bw))):
        if n == S.ORC_ERR_TRACE:
            ok = bool(status[k] & B.ST_TRACE)
        else:
            got = np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)
            ok = status[k] == 0 and np.array_equal(got, res) and np.array_equal(cigs[k], cig)
        if not ok:
            bad.append("pair %d qlen %d tlen %d status %d: gpu %s oracle %s" % (k, len(q), len(t), status[k], out[k], res))
    assert not bad, "%d/%d pairs differ (%s mode %d bw %d %s, %s)\n%s" % (len(bad), len(pairs), tag, mode, bw, scname, fwd, "\n".join(bad[:5]))
    assert "absolute scores" in fwd, fwd
    return fwd


def _launch(monkeypatch, xq, layout):
    """layout: "two-bit" (bandwidth 128, -gapo <= 3), "planes128" (the four planes at 128: asked for where the scoring would take two-bit fields, and as whole
    pairs with the four-lane shape), "planes256\""""
    if layout == "planes128":
        monkeypatch.setenv("BSA_ALIGN8_DO2", "0")
    else:
        monkeypatch.delenv("BSA_ALIGN8_DO2", raising=False)
    T._launch(monkeypatch, xq, planes128=(layout == "planes128"))
    return 256 if layout == "planes256" else 128


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("layout", ["two-bit", "planes128", "planes256"])
@pytest.mark.parametrize("scname", ["mn28", "cfirst61"])
def test_scorings_with_the_largest_differences(ctx, monkeypatch, xq, layout, scname):
    """related pairs in the three modes, and the batch of band moves (rows that stay at rbeg = 0, moves of two and more, jumps, ragged lengths)"""
    bw = _launch(monkeypatch, xq, layout)
    for mode in MODES:
        fwd = _check(ctx, "related", mode, scname, bw)
        assert ("two-bit" in fwd) == (layout == "two-bit"), fwd
        assert fwd.startswith("k_align8_fwd_xq (" if xq == "1" else "k_align8_fwd_x ("), fwd
    for mode in MODES:
        _check(ctx, "moves", mode, scname, bw)


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("layout", ["two-bit", "planes128", "planes256"])
def test_every_flag_plane_on_band_moves(ctx, monkeypatch, xq, layout):
    """the benchmark's scoring, -gapo = 4 (D and Od as one-bit flags at bandwidth 128 without being asked for) and linear gaps on the batch of band moves"""
    for scname in ("affine", "paper", "linear"):
        # (-gapo = 4 has no two-bit fields: its whole pairs at bandwidth 128 need the four-lane shape asked for, like the planes of the other scorings)
        bw = _launch(monkeypatch, xq, "planes128" if scname == "paper" and layout == "two-bit" else layout)
        for mode in MODES:
            fwd = _check(ctx, "moves", mode, scname, bw)
            if layout == "two-bit" and scname == "affine":
                assert "two-bit" in fwd, fwd


@pytest.mark.parametrize("bw", [128, 256])
def test_pad_cells(ctx, monkeypatch, bw):
    """queries shorter than the band on the moving-band kernels: the pad code's score (-63 - 2 gape) is the low end of S~ in the bound"""
    monkeypatch.setenv("BSA_ALIGN8_NO_STATIC", "1")
    for scname in ("mn28", "cfirst61", "paper"):
        T._launch(monkeypatch, "0", planes128=(bw == 128 and scname == "paper"))
        for mode in MODES:
            fwd = _check(ctx, "short%d" % bw, mode, scname, bw)
            assert fwd.startswith("k_align8_fwd_x ("), fwd
