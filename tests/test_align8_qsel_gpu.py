"""GPU parity of the forward kernels' query window (bsa_align8_x.hip, QWIN: sixteen cells a half, one-piece and linear gaps, bandwidth
128 and 256): the window holds one byte-permute selector per band column, W + 16 columns from the band offset of the last refill, and is
rebuilt for every live pair of the wave when one of them has moved 17 columns.  What the other GPU tests do not force: queries shorter than
the band, a band that moves by more than the refill distance in one row, queries that end inside the window's padding, and a row-segment
hand-over right behind a refill.  Every pair is compared with the oracle (record, CIGAR, status), none is left out."""
import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.gpu

SCORINGS = {
    "affine": (2, -6, -3, -2, 0, 0),      # the benchmark's: two-bit D / Od fields at bandwidth 128
    "paper": (2, -2, -4, -2, 0, 0),       # -gapo = 4: the four planes
    "linear": (2, -6, 0, -3, 0, 0),
}
MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)


def _check_all(ctx, pairs, mode, bw, sc):
    import bsalign_amd as B
    out, cigs, status = ctx.align_batch(pairs, B.make_params(mode, bw, *sc))
    assert len(status) == len(pairs)
    bad = []
    for k, (q, t) in enumerate(pairs):
        res, cig, n = S.oracle_align(q, t, mode, bw, *sc)
        if n == S.ORC_ERR_TRACE:
            ok = bool(status[k] & B.ST_TRACE)
        else:
            got = np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)
            ok = status[k] == 0 and np.array_equal(got, res) and np.array_equal(cigs[k], cig)
        if not ok:
            bad.append("pair %d qlen %d tlen %d status %d: gpu %s oracle %s" % (k, len(q), len(t), status[k], out[k], res))
    assert not bad, "%d/%d pairs differ (mode %d bw %d sc %s)\n%s" % (len(bad), len(pairs), mode, bw, sc, "\n".join(bad[:5]))
    return ctx.last_kernel_names()[0]


def _rand(rng, n):
    return rng.integers(0, 4, size=max(int(n), 1)).astype(np.uint8)


def _related(rng, lt, lq, eps):
    """a target of lt bases and a query of lq derived from it (cut or continued at random)"""
    t = _rand(rng, lt)
    q = S.mutate(rng, t, eps)
    q = q[:lq] if lq <= len(q) else np.concatenate([q, _rand(rng, lq - len(q))])
    return (q if len(q) else np.array([0], dtype=np.uint8)), t


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("scname", list(SCORINGS))
def test_queries_shorter_than_the_band(ctx, monkeypatch, xq, scname):
    """the band never moves and the window's first (only) fill reaches past the query's end into the padding from its first column on"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    monkeypatch.setenv("BSA_ALIGN8_NO_STATIC", "1")          # the moving-band kernels, not the band held in place
    rng = np.random.default_rng(7100 + len(scname))
    for bw in (128, 256):
        pairs = []
        for lq in [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, bw // 2, bw - 17, bw - 16, bw - 1]:
            for lt in (max(lq // 2, 1), lq, lq + 9, 3 * lq + 40):
                pairs.append(_related(rng, lt, lq, 0.1))
        for mode in MODES:
            _check_all(ctx, pairs, mode, bw, SCORINGS[scname])


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("scname", ["affine", "linear"])
def test_band_moves_past_the_refill_distance_in_one_row(ctx, monkeypatch, xq, scname):
    """queries 18 to 400 times their targets: the global steering moves the band by 17 and more columns a row (a refill on every row), by more
    than a whole band (the jump path), and pairs that move one column a row share their waves with them"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    rng = np.random.default_rng(7200 + len(scname))
    pairs = []
    for ratio in (18, 20, 33, 64, 127, 128, 129, 200, 400):
        for lt in (9, 24, 70, 130):
            pairs.append((_rand(rng, lt * ratio + int(rng.integers(0, 17))), _rand(rng, lt)))
            pairs.append(_related(rng, 600, 590, 0.05))
    for ratio in (2.0, 3.0, 5.0, 0.5, 0.3):          # the moves of test_length_mismatch_and_jumps, at these bandwidths
        for _ in range(6):
            lt = int(rng.integers(20, 400))
            pairs.append((_rand(rng, lt * ratio), _rand(rng, lt)))
    for bw in (128, 256):
        for mode in MODES:
            _check_all(ctx, pairs, mode, bw, SCORINGS[scname])


@pytest.mark.parametrize("xq", ["0", "1"])
def test_query_ends_inside_the_windows_padding(ctx, monkeypatch, xq):
    """query lengths bw - 16 .. bw + 34: the band reaches the query's end while the window's sixteen columns behind it are padding, and a refill
    at the last band offsets reads behind the staged query's end"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
    rng = np.random.default_rng(7300)
    for bw in (128, 256):
        pairs = []
        for lq in list(range(bw - 16, bw + 35)) + [bw + 47, bw + 48, bw + 49, 2 * bw, 2 * bw + 15, 2 * bw + 16, 2 * bw + 17]:
            pairs.append(_related(rng, lq + int(rng.integers(-8, 9)), lq, 0.1))
            pairs.append(_related(rng, 2 * lq, lq, 0.1))
        for sc in (SCORINGS["affine"], SCORINGS["linear"]):
            for mode in MODES:
                _check_all(ctx, pairs, mode, bw, sc)


@pytest.mark.parametrize("seg", ["64", "72", "80", "88", "104"])
def test_row_segment_cut_right_behind_a_refill(ctx, monkeypatch, seg):
    """k_align8_fwd_xq hands a pair's band state on at every multiple of `seg` rows, the window is not part of it: the next segment starts with a
    refill.  Refills fall every 13 to 16 rows counted from the segment's start, so with these segment lengths (4 x 16, 4 x 16 + 8, 5 x 16, ...) and
    pairs whose bands move at different rates the cut falls on the row of a refill, on the row behind one and on every row in between"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "1")
    monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", seg)
    rng = np.random.default_rng(7400 + int(seg))
    cut = int(seg)
    pairs = []
    for lt in [cut, cut + 1, 2 * cut - 1, 2 * cut, 2 * cut + 1, 3 * cut + 5, 5 * cut, 1000, 1500]:
        for eps in (0.0, 0.1, 0.2):
            for r in (1.0, 0.9, 1.1, 1.5):
                pairs.append(_related(rng, lt, int(lt * r), eps))
    for bw in (128, 256):
        for sc in (SCORINGS["affine"], SCORINGS["linear"]):
            for mode in MODES:
                fwd = _check_all(ctx, pairs, mode, bw, sc)
                assert "k_align8_fwd_xq" in fwd, fwd
