"""GPU parity of the absolute-score forward DP (bsa_align8_x.hip, x_forward_abs) on the rows whose band does not move by exactly one cell: records, status and
CIGAR words of every pair against the oracle, bit for bit, in the style of test_align8_flag_insert_gpu.py.

Such rows run blocks behind wave-level branches: the flag fix-up in its constant form while every live pair of the wave moved by at most two, the general loop
beside a move of three and more, and the first-cell rule: a shortcut while every such row of the wave stays at rbeg > 0, the rule itself otherwise, whose two
values for the rbeg = 0 fix-up are formed only in a wave that has a row at rbeg = 0.
test_align8_rare_rows_cpu.py has the batches and shows that each holds the rows it is meant to hold: "only2" runs the constant form alone, "rsj" (rush, stay and
jump pairs) the general loop, stalls behind the first column and jumps, "mixed" puts both kinds into one wave, so that the general loop has to agree with the
constant masks on the pairs that moved by at most two.  Scorings: the benchmark's, gap open -1 and -2 (a zero two-bit field at the band end becomes 2 and 1),
-gapo = 4 (four planes) and linear gaps; both bandwidths; the three modes; whole pairs and row segments of 64 rows; the mixed launch.
The oracle's answers are computed once per (pair, mode, scoring, bandwidth) and shared by the batches that hold the pair."""
import numpy as np
import pytest

import support as S
import test_align8_flag_insert_gpu as F
import test_align8_m3_gpu as T
import test_align8_rare_rows_cpu as R

pytestmark = pytest.mark.gpu

MODES = T.MODES
SCORINGS = {k: T.SCORINGS[k] for k in ("affine", "paper", "linear")}
SCORINGS.update({
    "go1": (2, -6, -1, -2, 0, 0),          # two-bit fields, a patched zero field reads 2
    "go2": (2, -6, -2, -2, 0, 0),          # ... reads 1
})
_ORACLE = {}


def _oracle(pairs, mode, scname, bw):
    out = []
    for q, t in pairs:
        key = (id(q), id(t), mode, scname, bw)          # (the batches are built once and kept: R.batch)
        if key not in _ORACLE:
            _ORACLE[key] = S.oracle_align(q, t, mode, bw, *SCORINGS[scname])
        out.append(_ORACLE[key])
    return out


def _check(ctx, tag, mode, scname, bw):
    import bsalign_amd as B
    pairs = R.batch(tag)
    out, cigs, status = ctx.align_batch(pairs, B.make_params(mode, bw, *SCORINGS[scname]))
    fwd = ctx.last_kernel_names()[0]
    assert len(status) == len(pairs) == len(cigs)
    bad = []
    for k, ((q, t), (res, cig, n)) in enumerate(zip(pairs, _oracle(pairs, mode, scname, bw))):
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


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("scname,layout", [("affine", "two-bit"), ("go1", "two-bit"), ("go2", "two-bit"), ("affine", "planes128"), ("paper", "planes128"),
                                           ("linear", "two-bit"), ("affine", "planes256"), ("go1", "planes256"), ("paper", "planes256"), ("linear", "planes256")])
def test_rare_rows(ctx, monkeypatch, xq, scname, layout):
    """every batch in the three modes; whole pairs (xq 0) and row segments of 64 rows (xq 1).  ("two-bit" asks for nothing: linear gaps have the four planes there.)"""
    bw = F._launch(monkeypatch, xq, layout)
    for mode in MODES:
        for tag in ("only2", "rsj", "mixed"):
            fwd = _check(ctx, tag, mode, scname, bw)
            assert ("two-bit" in fwd) == (layout == "two-bit" and scname != "linear"), fwd
            assert fwd.startswith("k_align8_fwd_xq (" if xq == "1" else "k_align8_fwd_x ("), fwd


def test_rare_rows_mixed_launch(ctx, monkeypatch):
    """k_align8_fwd_x_mix: the four-lane blocks run the absolute-score form beside eight-lane blocks in the difference form"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "0")
    monkeypatch.setenv("BSA_ALIGN8_X_N8", "40")
    for mode in MODES:
        fwd = _check(ctx, "all", mode, "paper", 128)
        assert "k_align8_fwd_x_mix" in fwd, fwd
