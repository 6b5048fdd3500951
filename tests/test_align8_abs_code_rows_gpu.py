"""The code rows of the absolute-score forward DP (bsa_align8_x.hip, x_forward_abs) against rows recorded from the build whose flags were accumulated by a
saturating subtraction and a multiply-add a cell (tests/golden/abs_code_rows.npz, written by tests/golden/make_abs_code_rows.py): byte for byte, every block of
every row of every pair within its tlen, for the three layouts of a code row (two-bit D / Od fields, four planes at bandwidth 128, four planes at 256).  The
traceback reads only the cells of an alignment's path; this compares all of them, the pad cells and the cells behind the band end included."""
import numpy as np
import pytest

import abs_code_rows_support as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    g = np.load(A.GOLDEN)
    qo, to = ([0] + [int(v) for v in np.cumsum(g[key], dtype=np.int64)] for key in ("qlen", "tlen"))
    pairs = [(g["q"][qo[k]:qo[k + 1]], g["t"][to[k]:to[k + 1]]) for k in range(len(g["qlen"]))]
    return g, pairs


@pytest.mark.parametrize("layout", list(A.LAYOUTS))
def test_code_rows_are_the_recorded_ones(ctx, monkeypatch, golden, layout):
    g, pairs = golden
    bw, sc, env = A.LAYOUTS[layout]
    for k in A.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**A.ENV, **env}.items():
        monkeypatch.setenv(k, v)
    name, status, rows = A.code_rows(ctx, pairs, layout)
    assert "absolute scores" in name and ("two-bit" in name) == (layout == "two-bit"), name
    assert np.array_equal(status, g["status_" + layout]), (status, g["status_" + layout])
    want = g["rows_" + layout]
    cw = bw // 128
    assert sum(r.size for r in rows) == want.size == int(g["tlen"].sum()) * 16 * cw
    bad, at = [], 0
    for k, r in enumerate(rows):
        w = want[at:at + r.size].reshape(r.shape)
        at += r.size
        if not np.array_equal(r, w):
            y, b, d = (int(v[0]) for v in np.nonzero(r != w))
            bad.append("pair %d (qlen %d, tlen %d): %d rows differ, first row %d block %d dword %d: %08x, recorded %08x"
                       % (k, len(pairs[k][0]), len(pairs[k][1]), int((r != w).any(axis=(1, 2)).sum()), y, b, d, r[y, b, d], w[y, b, d]))
    assert not bad, "%s (%s)\n%s" % (layout, name, "\n".join(bad[:8]))
