"""GPU parity of the absolute-score forward DP (bsa_align8_x.hip, x_forward_abs) where its integer row target of global steering meets the reference's double
expression: records, status and every CIGAR word against the oracle, bit for bit.

The kernel steps {k, r} of (i + jl) qlen = k tlen + r from row to row and uses k; a wave with a live row that has r = 0 takes the double expression for that
renewal and hands its state on through it (test_align8_row_target_cpu.py has the arithmetic).  The batches choose the lengths so that this happens on every
renewal, on every fourth, on the first alone, and differently in the pairs of one wave:
    equal     qlen = tlen: r = 0 on every row
    three4    qlen = 3 tlen / 4, tlen divisible by four: r = 0 on every fourth row, i.e. in one lane of four at every renewal
    coprime   gcd(qlen, tlen) = 1: r = 0 at row 0 alone
    mixed     the three kinds in turn, pair by pair, so that any group of sixteen holds all of them
Global mode, bandwidth 128 and 256, the benchmark's scoring and linear gaps (2, -6, 0, -3, 0, 0), 64 pairs a batch, targets of 256, 257, 384, 512 and 1000 rows
(257: no three4); the moving-band kernels asked for where no query is longer than the band (BSA_ALIGN8_NO_STATIC; the in-place kernel has no absolute form); whole pairs, row segments of 64 rows and the mixed launch (bandwidth 128, the benchmark's scoring with the four planes: the launch's condition).
The oracle's answers are computed once per (pair, scoring, bandwidth) and shared by the batches that hold the pair."""
import math

import numpy as np
import pytest

import support as S
import test_align8_m3_gpu as T

pytestmark = pytest.mark.gpu

TLENS = (256, 257, 384, 512, 1000)
NPAIRS = 64
SCORINGS = {"affine": (2, -6, -3, -2, 0, 0), "linear": (2, -6, 0, -3, 0, 0)}
_PAIRS, _ORACLE = {}, {}


def _coprime_len(tlen, k):
    """a query length near tlen, coprime to it, that varies with k"""
    n = tlen - 40 + (k % 23) * 3
    while math.gcd(n, tlen) != 1:
        n += 1
    return n


def pairs(tlen, kind):
    """the batches by (target length, kind); built once and never changed"""
    key = (tlen, kind)
    if key not in _PAIRS:
        if kind == "mixed":
            kinds = ("equal", "three4", "coprime") if tlen % 4 == 0 else ("equal", "coprime")
            _PAIRS[key] = [pairs(tlen, kinds[k % len(kinds)])[k] for k in range(NPAIRS)]
        else:
            out = []
            for k in range(NPAIRS):
                q, t = S.synth_pair(7000 + k, tlen + 200)
                qlen = {"equal": tlen, "three4": 3 * tlen // 4, "coprime": _coprime_len(tlen, k)}[kind]
                assert len(q) >= qlen
                out.append((q[:qlen].copy(), t[:tlen].copy()))
            _PAIRS[key] = out
    return _PAIRS[key]


def test_batches_hold_the_lengths_they_claim():
    for tlen in TLENS:
        for q, t in pairs(tlen, "equal"):
            assert len(q) == len(t) == tlen
        for k, (q, t) in enumerate(pairs(tlen, "coprime")):
            assert len(t) == tlen and math.gcd(len(q), tlen) == 1
            assert [a for a in range(tlen) if a * len(q) % tlen == 0] == [0]
        if tlen % 4 == 0:
            for q, t in pairs(tlen, "three4"):
                assert 4 * len(q) == 3 * tlen and [a for a in range(8) if a * len(q) % tlen == 0] == [0, 4]
        mixed = pairs(tlen, "mixed")
        for w in range(0, NPAIRS, 16):
            ratios = {(len(q) == tlen, 4 * len(q) == 3 * tlen) for q, t in mixed[w:w + 16]}
            assert len(ratios) == (3 if tlen % 4 == 0 else 2)


def _check(ctx, tlen, kind, scname, bw):
    import bsalign_amd as B
    batch = pairs(tlen, kind)
    out, cigs, status = ctx.align_batch(batch, B.make_params(B.MODE_GLOBAL, bw, *SCORINGS[scname]))
    fwd = ctx.last_kernel_names()[0]
    assert len(status) == len(batch) == len(cigs)
    bad = []
    for k, (q, t) in enumerate(batch):
        key = (id(q), id(t), scname, bw)
        if key not in _ORACLE:
            _ORACLE[key] = S.oracle_align(q, t, S.MODE_GLOBAL, bw, *SCORINGS[scname])
        res, cig, n = _ORACLE[key]
        if n == S.ORC_ERR_TRACE:
            ok = bool(status[k] & B.ST_TRACE)
        else:
            got = np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)
            ok = status[k] == 0 and np.array_equal(got, res) and np.array_equal(cigs[k], cig)
        if not ok:
            bad.append("pair %d qlen %d tlen %d status %d: gpu %s oracle %s" % (k, len(q), len(t), status[k], out[k], res))
    assert not bad, "%d/%d pairs differ (tlen %d %s bw %d %s, %s)\n%s" % (len(bad), len(batch), tlen, kind, bw, scname, fwd, "\n".join(bad[:5]))
    assert "absolute scores" in fwd, fwd
    return fwd


def _kinds(tlen):
    return ("equal", "three4", "coprime", "mixed") if tlen % 4 == 0 else ("equal", "coprime", "mixed")


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("bw", [128, 256])
@pytest.mark.parametrize("scname", ["affine", "linear"])
def test_row_target(ctx, monkeypatch, xq, bw, scname):
    """whole pairs (xq 0) and row segments of 64 rows (xq 1)"""
    monkeypatch.delenv("BSA_ALIGN8_DO2", raising=False)
    monkeypatch.setenv("BSA_ALIGN8_NO_STATIC", "1")
    T._launch(monkeypatch, xq)
    for tlen in TLENS:
        for kind in _kinds(tlen):
            fwd = _check(ctx, tlen, kind, scname, bw)
            # (a plan none of whose queries is longer than the band has no buffer for row segments: whole pairs whatever is asked for)
            segments = xq == "1" and max(len(q) for q, t in pairs(tlen, kind)) > bw
            assert fwd.startswith("k_align8_fwd_xq (" if segments else "k_align8_fwd_x ("), fwd


def test_row_target_mixed_launch(ctx, monkeypatch):
    """k_align8_fwd_x_mix: the four-lane blocks run the absolute-score form beside eight-lane blocks in the difference form"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "0")
    monkeypatch.setenv("BSA_ALIGN8_DO2", "0")
    monkeypatch.setenv("BSA_ALIGN8_X_N8", "24")
    monkeypatch.setenv("BSA_ALIGN8_NO_STATIC", "1")
    for tlen in TLENS:
        for kind in _kinds(tlen):
            fwd = _check(ctx, tlen, kind, "affine", 128)
            assert "k_align8_fwd_x_mix" in fwd, fwd
