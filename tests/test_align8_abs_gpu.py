"""GPU parity of the absolute-score form of the forward DP (bsa_align8_x.hip, x_forward_abs): one-piece and linear gaps at bandwidth 128 (four lanes per
pair, two-bit D / Od fields or four planes) and 256 (eight lanes).  Every pair is compared with the oracle (record, CIGAR, status), none is left out; every case
but the short queries (whose plans have no segment buffer: whole pairs only) runs as whole pairs (BSA_ALIGN8_XQ=0) and in row segments of 64 rows
(BSA_ALIGN8_XQ=1, BSA_ALIGN8_XQ_SEG=64), and every case asserts from the kernel name which launch family ran and that it ran the absolute form.  The oracle's answers are computed once per batch and shared between the cases.

Whole pairs at bandwidth 128 with four planes: a batch this small would go to the eight-lane shape (eight cells a half, which has no absolute form), so these
cases ask for four lanes (BSA_ALIGN8_X_LANES=4); the mixed launch has a case of its own.  The exact-arithmetic guard admits no matrix with
smin + gapo < -63 (63 + 2 ge + n + m + 2 g <= 125 caps n at 55 with m = 1, ge = 1), so the general matrices below are two of tests/matrix_support.py's inside it."""
import os

import numpy as np
import pytest

import matrix_support as MS
import support as S

pytestmark = pytest.mark.gpu

BWS = (128, 256)
MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)
# (M, X, O, E, Q, P, matrix)
SCORINGS = {
    "affine": (2, -6, -3, -2, 0, 0, None),          # the benchmark's
    "open1": (2, -6, -1, -2, 0, 0, None),           # -gapo = 1: the spare field value is 2
    "open2": (3, -4, -2, -1, 0, 0, None),
    "paper": (2, -2, -4, -2, 0, 0, None),           # -gapo = 4: the four planes
    "linear": (2, -6, 0, -3, 0, 0, None),
    "asym": (0, 0, -3, -2, 0, 0, MS.GENERAL["asym"]),
    "transition": (0, 0, -2, -2, 0, 0, MS.GENERAL["transition"]),
}
_ORACLE = {}


def _oracle(tag, pairs, mode, scname, bw):
    key = (tag, mode, scname, bw)
    if key not in _ORACLE:
        sc = SCORINGS[scname]
        _ORACLE[key] = [S.oracle_align(q, t, mode, bw, *sc[:6], mtx=sc[6]) for q, t in pairs]
    return _ORACLE[key]


def _run(ctx, pairs, mode, scname, bw=128):
    import bsalign_amd as B
    sc = SCORINGS[scname]
    par = B.make_params(mode, bw, *sc[:6]) if sc[6] is None else B.make_params(mode, bw, *sc[:6], matrix=sc[6])
    out, cigs, status = ctx.align_batch(pairs, par)
    return out, cigs, status, ctx.last_kernel_names()[0]


def _check_all(ctx, tag, pairs, mode, scname, bw=128, want_family=True):
    import bsalign_amd as B
    out, cigs, status, fwd = _run(ctx, pairs, mode, scname, bw)
    assert len(status) == len(pairs)
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
    xq = os.environ.get("BSA_ALIGN8_XQ")
    if xq is not None and want_family:
        assert fwd.startswith("k_align8_fwd_xq (" if xq == "1" else "k_align8_fwd_x"), (xq, fwd)
        assert xq == "1" or not fwd.startswith("k_align8_fwd_xq"), (xq, fwd)
    return fwd


def _rand(rng, n):
    return rng.integers(0, 4, size=max(int(n), 1)).astype(np.uint8)


def _related(rng, lt, lq, eps):
    t = _rand(rng, lt)
    q = S.mutate(rng, t, eps)
    q = q[:lq] if lq <= len(q) else np.concatenate([q, _rand(rng, lq - len(q))])
    return (q if len(q) else np.array([0], dtype=np.uint8)), t


def _two_bit(scname):
    return -SCORINGS[scname][2] in (1, 2, 3)


def _segments(monkeypatch, xq, scname="affine", bw=128):
    monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    if xq == "0" and bw == 128 and not _two_bit(scname) and scname != "linear":
        monkeypatch.setenv("BSA_ALIGN8_X_LANES", "4")          # whole pairs, four planes: the four-lane shape (module docstring)
    else:
        monkeypatch.delenv("BSA_ALIGN8_X_LANES", raising=False)


_CACHE = {}


def _batch(tag, bw=128):
    """the batches of this file, built once"""
    if tag == "short":
        tag = "short%d" % bw
    if tag in _CACHE:
        return _CACHE[tag]
    if tag == "related":
        rng = np.random.default_rng(8100)
        pairs = []
        for k in range(200):
            lt = int(rng.integers(300, 2001))
            pairs.append(_related(rng, lt, int(lt * rng.uniform(0.9, 1.1)), float(rng.uniform(0.05, 0.15))))
    elif tag == "rebase":
        # identical sequences (the fastest growth), unrelated ones (the fastest decline), one repeated base against a random query, and a
        # related pair: 6 kbp each = 93 rebases at the default period, 750 at the forced one, 93 hand-overs
        rng = np.random.default_rng(8200)
        t = _rand(rng, 6000)
        pairs = [(t.copy(), t), (_rand(rng, 6000), _rand(rng, 6000)), (_rand(rng, 6000), np.full(6000, 2, np.uint8)), _related(rng, 6000, 6100, 0.1)]
        t2 = _rand(rng, 6011)
        pairs += [(t2.copy(), t2), (_rand(rng, 5000), _rand(rng, 6003))]
    elif tag == "moves":
        rng = np.random.default_rng(8300)
        pairs = []
        for ratio in (18, 20, 33, 64, 127, 128, 129, 200, 400):
            for lt in (9, 24, 70, 130):
                pairs.append((_rand(rng, lt * ratio + int(rng.integers(0, 17))), _rand(rng, lt)))
                pairs.append(_related(rng, 600, 590, 0.05))
        for ratio in (2.0, 3.0, 5.0, 0.5, 0.3):
            for _ in range(6):
                lt = int(rng.integers(20, 400))
                pairs.append((_rand(rng, lt * ratio), _rand(rng, lt)))
    elif tag.startswith("short"):
        rng = np.random.default_rng(8400 + bw)
        pairs = []
        for lq in range(1, bw):
            for lt in (max(lq // 2, 1), lq + 9, 3 * lq + 40) if lq % 8 in (0, 1, 7) else (lq,):
                pairs.append(_related(rng, lt, lq, 0.1))
    else:
        raise KeyError(tag)
    _CACHE[tag] = pairs
    return pairs


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("bw", BWS)
@pytest.mark.parametrize("scname", list(SCORINGS))
def test_modes_and_scorings(ctx, monkeypatch, xq, bw, scname):
    """200 related pairs of 300 .. 2000 bp at error rates 0.05 .. 0.15, all three modes: two-bit fields (bandwidth 128, -gapo 1 .. 3), four planes, linear gaps"""
    _segments(monkeypatch, xq, scname, bw)
    for mode in MODES:
        fwd = _check_all(ctx, "related", _batch("related"), mode, scname, bw)
        assert ("two-bit" in fwd) == (bw == 128 and _two_bit(scname)), fwd


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("bw", BWS)
@pytest.mark.parametrize("period", [None, "8"])
def test_rebase(ctx, monkeypatch, xq, bw, period):
    """scores that grow and fall as fast as the scoring allows, over many rebases; with the period forced to its minimum of 8 rows a rebase lands
    on every hand-over row, on refill rows and on rows whose band does not move by one"""
    if period:
        monkeypatch.setenv("BSA_ALIGN8_ABS_R", period)
    for scname in ("affine", "asym", "paper", "linear"):
        _segments(monkeypatch, xq, scname, bw)
        for mode in MODES:
            fwd = _check_all(ctx, "rebase", _batch("rebase"), mode, scname, bw)
            assert "[rebase every %s rows]" % (period or "64") in fwd, fwd
    if period:
        for scname in ("affine", "linear"):
            _segments(monkeypatch, xq, scname, bw)
            fwd = _check_all(ctx, "moves", _batch("moves"), S.MODE_GLOBAL, scname, bw)
            assert "[rebase every 8 rows]" in fwd, fwd


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("bw", BWS)
def test_band_moves(ctx, monkeypatch, xq, bw):
    """length ratios 0.3 .. 400: rows that do not move, moves of two and more, jumps past the whole band; pairs that move one column a row share
    their waves with them"""
    for scname in ("affine", "open1", "paper", "linear"):
        _segments(monkeypatch, xq, scname, bw)
        for mode in MODES:
            _check_all(ctx, "moves", _batch("moves"), mode, scname, bw)


@pytest.mark.parametrize("bw", BWS)
def test_queries_shorter_than_the_band(ctx, monkeypatch, bw):
    """queries of 1 .. bw - 1 bases on the moving-band kernels: the columns beyond the query's end take the table's fifth entry (code 4), so the
    absolute form runs for them too.  Whole pairs only: a plan whose bands all cover their queries has no segment buffer"""
    monkeypatch.setenv("BSA_ALIGN8_NO_STATIC", "1")
    for scname in ("affine", "asym", "paper", "linear"):
        _segments(monkeypatch, "0", scname, bw)
        for mode in MODES:
            fwd = _check_all(ctx, "short", _batch("short", bw), mode, scname, bw)
            assert fwd.startswith("k_align8_fwd_x ("), fwd


def test_mixed_launch(ctx, monkeypatch):
    """k_align8_fwd_x_mix (bandwidth 128, four planes, whole pairs): the four-lane blocks run the absolute form beside eight-lane blocks in the difference form"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "0")
    monkeypatch.setenv("BSA_ALIGN8_X_N8", "70")
    pairs = _batch("related") + _batch("moves")
    for mode in MODES:
        fwd = _check_all(ctx, "related+moves", pairs, mode, "paper", 128)
        assert "k_align8_fwd_x_mix" in fwd, fwd


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("bw,scname", [(128, "affine"), (128, "paper"), (128, "linear"), (256, "affine"), (256, "linear")])
def test_both_forms_give_the_same_batch(ctx, monkeypatch, xq, bw, scname):
    """BSA_ALIGN8_ABS=0 keeps the difference form: records, CIGARs and status are identical to the default's"""
    _segments(monkeypatch, xq, scname, bw)
    pairs = _batch("related")[:80] + _batch("moves") + _batch("rebase")[:2]
    for mode in MODES:
        out1, cig1, st1, fwd1 = _run(ctx, pairs, mode, scname, bw)
        monkeypatch.setenv("BSA_ALIGN8_ABS", "0")
        out0, cig0, st0, fwd0 = _run(ctx, pairs, mode, scname, bw)
        monkeypatch.delenv("BSA_ALIGN8_ABS")
        assert "absolute scores" in fwd1 and "absolute scores" not in fwd0, (fwd1, fwd0)
        assert np.array_equal(st1, st0)
        assert all(out1[k] == out0[k] for k in range(len(pairs)))
        assert all(np.array_equal(a, b) for a, b in zip(cig1, cig0))
