"""GPU parity of the absolute-score forward DP (bsa_align8_x.hip, x_forward_abs) on the rows whose slots are shifted two to an instruction (x_slots_up for a row
that stays, x_slots_down for every cell of a move beyond one): records, status and CIGAR words of every pair against the oracle, bit for bit.

test_align8_pair_shift_cpu.py has the batches and shows that each holds the rows it is meant to hold: stalls at rbeg = 0 and above, moves of two and three, a stall
followed at once by a move of two in the same pair, both kinds inside one group of sixteen with the odd pairs first and last of the group, and segments of 64 rows
that begin on a stall, on a move of two and on a move of three.  Global mode, targets of 600 rows, bandwidth 128 (two-bit fields, and the four planes) and 256, the
benchmark's scoring; whole pairs, row segments of 64 rows, the mixed launch.  The oracle's answers are computed once per (pair, bandwidth) and shared."""
import numpy as np
import pytest

import support as S
import test_align8_flag_insert_gpu as F
import test_align8_pair_shift_cpu as P

pytestmark = pytest.mark.gpu

SC = (2, -6, -3, -2, 0, 0)
TAGS = ("stalls", "twos", "stall2", "both")
_ORACLE = {}


def _check(ctx, tag, bw):
    import bsalign_amd as B
    pairs = P.batch(tag)
    out, cigs, status = ctx.align_batch(pairs, B.make_params(B.MODE_GLOBAL, bw, *SC))
    fwd = ctx.last_kernel_names()[0]
    assert len(status) == len(pairs) == len(cigs)
    bad = []
    for k, (q, t) in enumerate(pairs):
        key = (id(q), id(t), bw)
        if key not in _ORACLE:
            _ORACLE[key] = S.oracle_align(q, t, S.MODE_GLOBAL, bw, *SC)
        res, cig, n = _ORACLE[key]
        if n == S.ORC_ERR_TRACE:
            ok = bool(status[k] & B.ST_TRACE)
        else:
            got = np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)
            ok = status[k] == 0 and np.array_equal(got, res) and np.array_equal(cigs[k], cig)
        if not ok:
            bad.append("pair %d qlen %d tlen %d status %d: gpu %s oracle %s" % (k, len(q), len(t), status[k], out[k], res))
    assert not bad, "%d/%d pairs differ (%s bw %d, %s)\n%s" % (len(bad), len(pairs), tag, bw, fwd, "\n".join(bad[:5]))
    assert "absolute scores" in fwd, fwd
    return fwd


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("layout", ["two-bit", "planes128", "planes256"])
def test_pair_shift(ctx, monkeypatch, xq, layout):
    """whole pairs (xq 0) and row segments of 64 rows (xq 1)"""
    bw = F._launch(monkeypatch, xq, layout)
    for tag in TAGS:
        fwd = _check(ctx, tag, bw)
        assert ("two-bit" in fwd) == (layout == "two-bit"), fwd
        assert fwd.startswith("k_align8_fwd_xq (" if xq == "1" else "k_align8_fwd_x ("), fwd


def test_pair_shift_mixed_launch(ctx, monkeypatch):
    """k_align8_fwd_x_mix: the four-lane blocks run the absolute-score form beside eight-lane blocks in the difference form (the batch's last eight pairs)"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "0")
    monkeypatch.setenv("BSA_ALIGN8_DO2", "0")
    monkeypatch.setenv("BSA_ALIGN8_X_N8", "8")
    for tag in TAGS:
        fwd = _check(ctx, tag, 128)
        assert "k_align8_fwd_x_mix" in fwd, fwd
