"""bsa_align8_abs_rows (bsa_align8_x.hip) on a grid of scorings, host only: which form of the absolute-score forward DP a scoring gets and with which rebase
period R.  With s = max(go, m + go + 2 ge) a row's values lie within s (bw + R) + 512 of the frame's origin R rows after a rebase.  The three-operand maxima
compare int16 scores as f16, which is the integer order for the patterns 0x0400 .. 0x7BFF only; their frame sits at 0x4000, so that form needs
s (bw + R) + 512 <= 15359 (= 0x7BFF - 0x4000, the smaller side).  A scoring that has no R >= 8 there must be given the integer maxima, whose int16 frame
at 0 needs s (bw + R) + 512 <= 32767."""
import ctypes as C

import pytest

import bsalign_amd as B

BOUND_M3, BOUND_INT = 15359, 32767
MS = tuple(range(0, 67))
XS = (0, -1, -2, -3, -6, -20, -55)
OS = tuple(range(0, -23, -1))
ES = tuple(range(0, -23, -1))


def _span(s, bw, r):
    return s * (bw + r) + 512


@pytest.fixture(scope="module")
def grid():
    """(bw, M, X, O, E) -> (form, rows) for every scoring of the grid that the exact-arithmetic kernel takes"""
    mp = pytest.MonkeyPatch()
    mp.delenv("BSA_ALIGN8_ABS", raising=False)
    mp.delenv("BSA_ALIGN8_ABS_R", raising=False)
    try:
        L = B.lib()
        fn = L.bsa_align8_abs_form_internal
        rows = C.c_uint32(0)
        out = {}
        for bw in (128, 256):
            for M in MS:
                for X in XS:
                    par = B.make_params(B.MODE_GLOBAL, bw, M, X, 0, 0)
                    for O in OS:
                        par.gapo1 = O
                        for E in ES:
                            par.gape1 = E
                            form = fn(C.byref(par), C.byref(rows))
                            if form >= 0:
                                out[(bw, M, X, O, E)] = (form, rows.value)
    finally:
        mp.undo()
    return out


def _s(M, O, E):
    return max(-O, M - O - 2 * E)


def test_the_grid_covers_both_forms(grid):
    forms = {bw: {f for (b, *_), (f, _) in grid.items() if b == bw} for bw in (128, 256)}
    assert len(grid) > 15000
    assert forms[128] == {2}, forms          # bandwidth 128: s <= 100 inside the guard, and 100 (128 + 8) + 512 <= 15359
    assert forms[256] == {1, 2}, forms
    assert {r for (f, r) in grid.values()} <= {8, 16, 32, 64}


def test_every_scoring_meets_the_bound_of_its_form(grid):
    bad = []
    for (bw, M, X, O, E), (form, r) in grid.items():
        s = _s(M, O, E)
        if form == 2:
            ok = r >= 8 and _span(s, bw, r) <= BOUND_M3 and (r == 64 or _span(s, bw, 2 * r) > BOUND_M3)
        elif form == 1:
            # the integer form only where the biased frame has no period at all, and then inside int16
            ok = r >= 8 and _span(s, bw, 8) > BOUND_M3 and _span(s, bw, r) <= BOUND_INT and (r == 64 or _span(s, bw, 2 * r) > BOUND_INT)
        else:
            ok = False          # the difference form: nothing inside the guard needs it (s (256 + 8) + 512 <= 32767 up to s = 122)
        if not ok:
            bad.append(((bw, M, X, O, E), s, form, r))
    assert not bad, bad[:10]


def test_thresholds(grid):
    s_of = lambda k: _s(k[1], k[3], k[4])
    top = {bw: max(s_of(k) for k, (f, _) in grid.items() if k[0] == bw and f == 2) for bw in (128, 256)}
    low = min(s_of(k) for k, (f, _) in grid.items() if k[0] == 256 and f == 1)
    assert top[256] == 56 and low == 57, (top, low)          # 56 (256 + 8) + 512 = 15296, 57 (256 + 8) + 512 = 15560
    assert top[128] == max(s_of(k) for k in grid if k[0] == 128)
    # the benchmark's scoring keeps the full period at both widths
    assert grid[(128, 2, -6, -3, -2)] == (2, 64) and grid[(256, 2, -6, -3, -2)] == (2, 64)


def test_period_hook_and_switch(monkeypatch):
    par = B.make_params(B.MODE_GLOBAL, 128, 2, -6, -3, -2)
    monkeypatch.setenv("BSA_ALIGN8_ABS_R", "8")
    assert B.align8_abs_form(par) == (2, 8)
    monkeypatch.delenv("BSA_ALIGN8_ABS_R")
    monkeypatch.setenv("BSA_ALIGN8_ABS", "0")
    assert B.align8_abs_form(par) == (0, 0)
    monkeypatch.delenv("BSA_ALIGN8_ABS")
    assert B.align8_abs_form(par) == (2, 64)
    two_piece = B.make_params(B.MODE_GLOBAL, 128, 2, -6, -3, -2, -8, -1)
    assert B.align8_abs_form(two_piece)[0] == -1
