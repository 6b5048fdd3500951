"""bsa_align8_flag_span (bsa_align8_x.hip) on the grid of scorings of test_align8_m3_bound_cpu.py, host only.  The absolute-score forward DP turns "two int16
scores are equal" into a flag bit from the high byte of their difference, which is exact while the difference lies in 0 .. 256.  The function derives the
largest difference a stored cell can see for a scoring; here it is set against a direct enumeration of the derivation's terms (the comment above the
function has the derivation), and wherever the launcher picks the absolute-score form the span must fit."""
import ctypes as C

import pytest

import bsalign_amd as B

LIMIT = 256
P = 63          # -BSA_EPI8_MIN = BSA_EPI8_MAX: the sentinels, the pad code and the clamp of the first-cell rule
MS = tuple(range(0, 67))
XS = (0, -1, -2, -3, -6, -20, -55)
OS = tuple(range(0, -23, -1))
ES = tuple(range(0, -23, -1))


def _terms(M, X, O, E):
    """the derivation's terms, spelt out: m, n, go, ge as magnitudes"""
    m, n, go, ge = M, -X, -O, -E
    s_lo, s_hi = -max(n, P) + 2 * ge, m + 2 * ge          # S~ = S - 2 gape: a mismatch or the pad code at the low end
    s1 = m + go + 2 * ge                                  # a step between computed neighbours, along a row or down a column
    v = max(s1, P + ge)                                   # ... down a column, the first-cell rule's clamp included
    return (
        v - s_lo,                # M: f - d <= (Lf - A) - S~          (E - d <= s1 - S~ is never larger)
        s_hi + go + go,          # D: d - E <= (A - U) + S~ + go
        v + go + go,             # D: f - E <= (Lf - A) + (A - U) + go
        s_hi + P - ge,           # D, row -1: E is the sentinel, P - ge below its diagonal predecessor
        v + P - ge,              # D, row -1: f - E
        go,                      # R, Od
    )


@pytest.fixture(scope="module")
def grid():
    """(bw, M, X, O, E) -> (form, span, terms) for every scoring of the grid that the exact-arithmetic kernel takes"""
    mp = pytest.MonkeyPatch()
    mp.delenv("BSA_ALIGN8_ABS", raising=False)
    mp.delenv("BSA_ALIGN8_ABS_R", raising=False)
    try:
        L = B.lib()
        form_fn, span_fn = L.bsa_align8_abs_form_internal, L.bsa_align8_flag_span_internal
        rows = C.c_uint32(0)
        terms = (C.c_uint32 * len(B.FLAG_SPAN_TERMS))()
        out = {}
        for bw in (128, 256):
            for M in MS:
                for X in XS:
                    par = B.make_params(B.MODE_GLOBAL, bw, M, X, 0, 0)
                    for O in OS:
                        par.gapo1 = O
                        for E in ES:
                            par.gape1 = E
                            form = form_fn(C.byref(par), C.byref(rows))
                            if form >= 0:
                                span = span_fn(C.byref(par), terms)
                                out[(bw, M, X, O, E)] = (form, span, tuple(terms))
    finally:
        mp.undo()
    return out


def test_the_span_fits_wherever_the_absolute_form_runs(grid):
    assert len(grid) > 15000
    picked = {k: v for k, v in grid.items() if v[0] in (1, 2)}
    assert len(picked) == len(grid)          # (nothing inside the guard keeps the difference form: test_align8_m3_bound_cpu.py)
    bad = [(k, v) for k, v in picked.items() if not 0 < v[1] <= LIMIT]
    assert not bad, bad[:10]


def test_the_span_is_the_maximum_of_the_enumerated_terms(grid):
    bad = []
    for (bw, M, X, O, E), (form, span, terms) in grid.items():
        want = _terms(M, X, O, E)
        if terms != want or span != max(want):
            bad.append(((bw, M, X, O, E), span, terms, want))
    assert not bad, bad[:10]


def test_the_guard_keeps_every_term_below_127(grid):
    """63 + 2 ge + n + m + 2 g <= 125 and m + 3 g + 2 ge <= 100 bound every term by 126: a wide margin below 256, at both bandwidths alike"""
    top = max(v[1] for v in grid.values())
    assert top <= 126, top
    assert {k[1:]: v[1:] for k, v in grid.items() if k[0] == 128} == {k[1:]: v[1:] for k, v in grid.items() if k[0] == 256}
    # the benchmark's scoring: V = max(2 + 3 + 4, 63 + 2) = 65; f - d <= 65 + 63 - 4, d - E <= 6 + 6, f - E <= 65 + 6, row -1: 6 + 63 - 2 and 65 + 63 - 2
    assert B.align8_flag_span(B.make_params(B.MODE_GLOBAL, 128, 2, -6, -3, -2)) == (126, (124, 12, 71, 67, 126, 3))


def test_outside_the_form(monkeypatch):
    two_piece = B.make_params(B.MODE_GLOBAL, 128, 2, -6, -3, -2, -8, -1)
    assert B.align8_flag_span(two_piece)[0] == -1
    monkeypatch.setenv("BSA_ALIGN8_ABS", "0")
    assert B.align8_flag_span(B.make_params(B.MODE_GLOBAL, 128, 2, -6, -3, -2))[0] == 0
