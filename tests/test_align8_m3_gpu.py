"""GPU parity of the absolute-score forward DP with three-operand maxima in the biased frame (bsa_align8_x.hip, x_forward_abs<.., M3>): records, status and
CIGAR words (with the offsets that cut them out of the arena) of every pair against the oracle, bit for bit, and from the kernel name which form of the maxima
ran and with which rebase period.  Batches are 64 .. 200 pairs of 300 .. 700 rows: at least four rebase periods at R = 64, dozens at the forced R = 8.  The
oracle's answers are computed once per (batch, mode, scoring, bandwidth).

The int16 scores are compared as f16, which orders the patterns 0x0400 .. 0x7BFF as integers do; the cases aim at what could leave that range or break the
frame's book-keeping: scorings at the edge of the bound, rows that rise and fall as fast as the scoring allows, bands that jump (the row starts again from
absolute values), rows that do not move, queries shorter than the band, dead lanes beside live ones, and the hand-over of the biased state between row segments."""
import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.gpu

MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)
M3, INT = "[three-operand maxima, biased frame]", "[integer maxima]"
# (M, X, O, E, Q, P); s = max(go, m + go + 2 ge)
SCORINGS = {
    "affine": (2, -6, -3, -2, 0, 0),          # the benchmark's, s = 9
    "paper": (2, -2, -4, -2, 0, 0),           # -gapo = 4: four planes at bandwidth 128
    "linear": (2, -6, 0, -3, 0, 0),
    "s56": (53, -2, -1, -1, 0, 0),            # bandwidth 256: 56 (256 + 8) + 512 = 15296 <= 15359, the largest s of the biased frame (R = 8)
    "s57": (54, -2, -1, -1, 0, 0),            # bandwidth 256: 57 (256 + 8) + 512 = 15560: the smallest s that keeps the integer maxima
    "s58": (55, -1, -1, -1, 0, 0),            # the largest s inside the guard with a mismatch and go, ge >= 1 (63 + 2 ge + n + m + 2 g <= 125): the biased frame at
                                              # bandwidth 128 (58 (128 + 64) + 512 = 11648), the integer maxima at 256
    "s59lin": (57, -1, 0, -1, 0, 0),          # ... with linear gaps
}
_ORACLE, _CACHE = {}, {}


def _rand(rng, n):
    return rng.integers(0, 4, size=max(int(n), 1)).astype(np.uint8)


def _related(rng, lt, lq, eps):
    t = _rand(rng, lt)
    q = S.mutate(rng, t, eps)
    q = q[:lq] if lq <= len(q) else np.concatenate([q, _rand(rng, lq - len(q))])
    return (q if len(q) else np.array([0], dtype=np.uint8)), t


def _batch(tag):
    if tag in _CACHE:
        return _CACHE[tag]
    if tag == "related":
        rng = np.random.default_rng(9100)
        pairs = []
        for k in range(96):
            lt = int(rng.integers(300, 701))
            pairs.append(_related(rng, lt, int(lt * rng.uniform(0.9, 1.1)), float(rng.uniform(0.03, 0.2))))
    elif tag == "drift":
        # identical pairs: every row rises by m + 2 ge in the frame; no match at all: it falls by go a step; one base against a random query; 64 pairs, ragged
        rng = np.random.default_rng(9200)
        pairs = []
        for k in range(16):
            n = int(rng.integers(300, 701))
            t = _rand(rng, n)
            pairs.append((t.copy(), t))
            pairs.append((np.zeros(n, np.uint8), np.full(n + int(rng.integers(0, 40)), 1, np.uint8)))
            pairs.append((_rand(rng, n), np.full(n, 2, np.uint8)))
            pairs.append((_rand(rng, n), _rand(rng, n)))
    elif tag == "moves":
        # queries far longer than their targets (the band rushes: moves of two and more, jumps past all it held), targets longer than their queries (rows
        # that do not move), ordinary pairs in between, and lengths that differ inside every wave: rows past a short target run beside live ones
        rng = np.random.default_rng(9300)
        pairs = []
        for ratio in (20, 64, 127, 128, 129, 200, 257, 400):
            for lt in (9, 24, 70):
                pairs.append((_rand(rng, lt * ratio + int(rng.integers(0, 17))), _rand(rng, lt)))
                pairs.append(_related(rng, 500, 490, 0.05))
        for ratio in (2.0, 3.0, 5.0, 0.5, 0.3, 0.2):
            for _ in range(5):
                lt = int(rng.integers(300, 700))
                pairs.append((_rand(rng, lt * ratio), _rand(rng, lt)))
        for k in range(34):
            lt = int(rng.integers(1, 700))
            pairs.append(_related(rng, lt, max(int(lt * rng.uniform(0.8, 1.2)), 1), 0.1))
    elif tag.startswith("short"):
        bw = int(tag[5:])
        rng = np.random.default_rng(9400 + bw)
        pairs = []
        for lq in list(range(1, bw, 5)) + [bw - 1]:
            for lt in (max(lq // 2, 1), lq + 9, 3 * lq + 300):
                pairs.append(_related(rng, lt, lq, 0.1))
    else:
        raise KeyError(tag)
    _CACHE[tag] = pairs
    return pairs


def _oracle(tag, pairs, mode, scname, bw):
    key = (tag, mode, scname, bw)
    if key not in _ORACLE:
        _ORACLE[key] = [S.oracle_align(q, t, mode, bw, *SCORINGS[scname]) for q, t in pairs]
    return _ORACLE[key]


def _check(ctx, tag, mode, scname, bw, form=M3, rows=None):
    import bsalign_amd as B
    pairs = _batch(tag)
    out, cigs, status = ctx.align_batch(pairs, B.make_params(mode, bw, *SCORINGS[scname]))
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
    assert "absolute scores" in fwd and form in fwd, fwd
    if rows is not None:
        assert "[rebase every %d rows]" % rows in fwd, fwd
    return fwd


def _launch(monkeypatch, xq, planes128=False):
    """whole pairs ("0") or row segments of 64 rows ("1"); four planes at bandwidth 128 as whole pairs need the four-lane shape asked for (a batch this small would
    go to the eight-lane one, which has no absolute form)"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    if xq == "0" and planes128:
        monkeypatch.setenv("BSA_ALIGN8_X_LANES", "4")
    else:
        monkeypatch.delenv("BSA_ALIGN8_X_LANES", raising=False)


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("case", ["two-bit", "planes", "bw256", "linear128", "linear256"])
def test_benchmark_scoring(ctx, monkeypatch, xq, case):
    """the benchmark's scoring in the three modes: bandwidth 128 with two-bit fields and with the four planes, bandwidth 256, and linear gaps at both"""
    bw = 256 if case.endswith("256") else 128
    scname = "linear" if case.startswith("linear") else "affine"
    if case == "planes":
        monkeypatch.setenv("BSA_ALIGN8_DO2", "0")
    _launch(monkeypatch, xq, planes128=(case == "planes"))
    for mode in MODES:
        fwd = _check(ctx, "related", mode, scname, bw, M3, 64)
        assert ("two-bit" in fwd) == (case == "two-bit"), fwd
        assert fwd.startswith("k_align8_fwd_xq (" if xq == "1" else "k_align8_fwd_x ("), fwd


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("scname,bw,form,rows", [("s56", 256, M3, 8), ("s57", 256, INT, 64), ("s58", 128, M3, 64), ("s59lin", 128, M3, 64), ("s58", 256, INT, 64)])
def test_scorings_at_the_edge_of_the_bound(ctx, monkeypatch, xq, scname, bw, form, rows):
    """the largest s that the biased frame takes at bandwidth 256 (at R = 8, all it has left), the smallest that falls back to the integer maxima there, and the
    largest s of the guard at bandwidth 128; the kernel name says which form ran.  Identical pairs and pairs without a match drive the frame as far from its
    origin as these scorings can between two rebases.
    (The drift batch runs in global and extend mode here.  In overlap mode its pairs without a match end in a two-column alignment under a match score this
    large, and for those the device traceback and the oracle disagree whichever forward kernel ran -- the packed one and the build before this form included;
    test_drift has the overlap mode of that batch under the scorings where the two agree.)"""
    _launch(monkeypatch, xq)
    for mode in MODES:
        _check(ctx, "related", mode, scname, bw, form, rows)
    for mode in (S.MODE_GLOBAL, S.MODE_EXTEND):
        _check(ctx, "drift", mode, scname, bw, form, rows)


@pytest.mark.parametrize("bw", [128, 256])
@pytest.mark.parametrize("period", [None, "8"])
def test_drift(ctx, monkeypatch, bw, period):
    """drift in both directions at the full period (the frame travels as far as the bound allows) and at the shortest"""
    if period:
        monkeypatch.setenv("BSA_ALIGN8_ABS_R", period)
    for scname in ("affine", "paper", "linear"):
        _launch(monkeypatch, "0", planes128=(bw == 128 and scname == "paper"))
        for mode in MODES:
            _check(ctx, "drift", mode, scname, bw, M3, int(period or 64))


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("bw", [128, 256])
def test_band_moves_and_ragged_lengths(ctx, monkeypatch, xq, bw):
    """band jumps (the row starts again from absolute values above the frame's origin), moves of two and more, rows that do not move, lengths that differ inside a wave"""
    for scname, period in (("affine", None), ("affine", "8"), ("linear", None), ("s56" if bw == 256 else "s58", None)):
        if period:
            monkeypatch.setenv("BSA_ALIGN8_ABS_R", period)
        else:
            monkeypatch.delenv("BSA_ALIGN8_ABS_R", raising=False)
        _launch(monkeypatch, xq)
        for mode in MODES:
            _check(ctx, "moves", mode, scname, bw, M3)


@pytest.mark.parametrize("bw", [128, 256])
def test_queries_shorter_than_the_band(ctx, monkeypatch, bw):
    """queries of 1 .. bw - 1 bases on the moving-band kernels (whole pairs: such plans have no segment buffer): the columns beyond the query's end take the padding
    code, whose score enters the maxima like any other"""
    monkeypatch.setenv("BSA_ALIGN8_NO_STATIC", "1")
    for scname in ("affine", "paper", "linear"):
        _launch(monkeypatch, "0", planes128=(bw == 128 and scname == "paper"))
        for mode in MODES:
            fwd = _check(ctx, "short%d" % bw, mode, scname, bw, M3)
            assert fwd.startswith("k_align8_fwd_x ("), fwd


def test_mixed_launch(ctx, monkeypatch):
    """k_align8_fwd_x_mix: the four-lane blocks run the biased frame beside eight-lane blocks in the difference form"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "0")
    monkeypatch.setenv("BSA_ALIGN8_X_N8", "40")
    for tag in ("related", "moves"):
        for mode in MODES:
            fwd = _check(ctx, tag, mode, "paper", 128, M3, 64)
            assert "k_align8_fwd_x_mix" in fwd, fwd
