"""GPU parity of the forward DP (bsa_align8_x.hip) on the rows where the noise sum of band steering decides the band's move, and on both sides of the mask
behind which cell 0's M flag is formed again: records, status and CIGAR words of every pair against the oracle, bit for bit, and with BSA_MODE_BAND_MARGIN the
margins, which depend on every row's band offset.

test_align8_steer_sum_cpu.py has the corpus (stretches of 25 .. 40 % errors, runs of 20 .. 60 bases on either side, queries at 3 / 4 and 5 / 4 of the target's
length, targets of 256 .. 1000 rows) and shows on the oracle alone that it holds rows with noisy above its floor of 16, rows the band moves by one BECAUSE of
noisy, rows it moves by 0 or 2 against such a noisy, rows at rbeg = 0 and stalls at rbeg > 0 directly followed by a row that moves by one.  The batches put
rough pairs first and last in a group of sixteen plain ones, and plain pairs first and last among rough ones.

Scorings: the benchmark's, linear gaps 2,-6,0,-3, and the largest |gape| that the absolute-score form with three-operand maxima takes at bandwidth 128 (asked of
bsa_align8_x_choice_internal); bandwidths 128 (two-bit fields and the four planes) and 256, the three modes, whole pairs and row segments of 64 rows, the mixed
launch, and BSA_MODE_SCORE_ONLY.  The sum of the difference form (two-piece gaps, bandwidth 64) is unchanged; those shapes run once each, for the prefix
maximum they share.  The oracle's answers are computed once per (pair, mode, bandwidth, scoring) and shared."""
import numpy as np
import pytest

import band_margin_cases as K
import support as S
import test_align8_flag_insert_gpu as F
import test_align8_steer_sum_cpu as P

pytestmark = pytest.mark.gpu

MODES = (S.MODE_GLOBAL, S.MODE_OVERLAP, S.MODE_EXTEND)
TAGS = ("rough_ends", "plain_ends")
_ORACLE = {}


def _scoring(name):
    return {"bench": P.SC_BENCH, "linear": P.SC_LINEAR, "two-piece": P.SC_TWO}[name] if name != "maxgape" else P.max_gape_scoring()


def _oracle(q, t, mode, bw, sc):
    key = (id(q), id(t), mode, bw, sc)
    if key not in _ORACLE:
        _ORACLE[key] = S.oracle_align(q, t, mode, bw, *sc, want_begs=True)
    return _ORACLE[key]


def _check(ctx, tag, mode, bw, sc, absolute=True, with_margins=True):
    """records, status, CIGAR words and margins of a batch against the oracle; -> (forward kernel's name, pairs handed over to the literal kernels)"""
    import bsalign_amd as B
    pairs = P.batch(tag)
    if with_margins:
        out, cigs, status, margins = ctx.align_batch(pairs, B.make_params(mode, bw, *sc), margins=True)
    else:
        out, cigs, status = ctx.align_batch(pairs, B.make_params(mode, bw, *sc))
        margins = None
    fwd, handed = ctx.last_kernel_names()[0], ctx.last_handover()
    assert len(status) == len(pairs) == len(cigs) and (margins is None or len(margins) == len(pairs))
    bad = []
    for k, (q, t) in enumerate(pairs):
        res, cig, n, begs = _oracle(q, t, mode, bw, sc)
        if n == S.ORC_ERR_TRACE:
            ok = bool(status[k] & B.ST_TRACE)
        else:
            got = np.array([out[k][f] for f in out.dtype.names], dtype=np.int32)
            want = K.margin_ref(len(q), len(t), bw, res, cig, begs)
            ok = status[k] == 0 and np.array_equal(got, res) and np.array_equal(cigs[k], cig) and (margins is None or int(margins[k]) == want)
        if not ok:
            bad.append("pair %d qlen %d tlen %d status %d margin %s: gpu %s oracle %s" % (k, len(q), len(t), status[k], None if margins is None else margins[k], out[k], res))
    assert not bad, "%d/%d pairs differ (%s mode %d bw %d %s, %s)\n%s" % (len(bad), len(pairs), tag, mode, bw, sc, fwd, "\n".join(bad[:5]))
    assert ("absolute scores" in fwd) == absolute, fwd
    return fwd, handed


@pytest.mark.parametrize("xq", ["0", "1"])
@pytest.mark.parametrize("layout", ["two-bit", "planes128", "planes256"])
@pytest.mark.parametrize("scname", ["bench", "linear", "maxgape"])
def test_steer_sum(ctx, monkeypatch, xq, layout, scname):
    """whole pairs (xq 0) and row segments of 64 rows (xq 1) of the absolute-score form, the three modes"""
    bw = F._launch(monkeypatch, xq, layout)
    sc = _scoring(scname)
    for tag in TAGS:
        for mode in MODES:
            fwd, handed = _check(ctx, tag, mode, bw, sc)
            print(tag, mode, bw, sc, fwd, "handed over", handed)
            assert ("two-bit" in fwd) == (layout == "two-bit" and scname == "bench"), fwd
            assert fwd.startswith("k_align8_fwd_xq (" if xq == "1" else "k_align8_fwd_x ("), fwd
            assert "three-operand maxima" in fwd, fwd
            assert handed == 0, (handed, tag, mode, bw, scname)


def test_steer_sum_mixed_launch(ctx, monkeypatch):
    """k_align8_fwd_x_mix: the four-lane blocks run the absolute-score form beside eight-lane blocks in the difference form (the batch's last eight pairs)"""
    monkeypatch.setenv("BSA_ALIGN8_XQ", "0")
    monkeypatch.setenv("BSA_ALIGN8_DO2", "0")
    monkeypatch.setenv("BSA_ALIGN8_X_N8", "8")
    # (one-piece gaps only: linear gaps have no mixed launch; the second scoring is the largest |gape| with an opening penalty)
    for sc in (P.SC_BENCH, P.max_gape_scoring(opens=(-1,))):
        for tag in TAGS:
            for mode in MODES:
                fwd, handed = _check(ctx, tag, mode, 128, sc, with_margins=False)
                assert "k_align8_fwd_x_mix" in fwd, (fwd, sc)


@pytest.mark.parametrize("case", ["two-piece", "bw64"])
def test_difference_form_shapes(ctx, monkeypatch, case):
    """two-piece gaps at bandwidth 128 and the benchmark's scoring at bandwidth 64 (x_forward: its own sum, the shared prefix maximum), whole pairs and row segments"""
    bw, sc = (128, _scoring("two-piece")) if case == "two-piece" else (64, _scoring("bench"))
    for xq in ("0", "1"):
        monkeypatch.setenv("BSA_ALIGN8_XQ", xq)
        monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
        for tag in TAGS:
            for mode in MODES:
                fwd, handed = _check(ctx, tag, mode, bw, sc, absolute=False)
                assert fwd.startswith("k_align8_fwd_x"), fwd


@pytest.mark.parametrize("bw", [128, 256])
def test_score_only(ctx, bw):
    """BSA_MODE_SCORE_ONLY: score, qe and te of every pair against the oracle (the forward-only kernels steer the band with the same rule)"""
    import bsalign_amd as B
    for scname in ("bench", "linear", "maxgape"):
        sc = _scoring(scname)
        for tag in TAGS:
            pairs = P.batch(tag)
            for mode in MODES:
                so, sst = ctx.align_scores(pairs, B.make_params(mode, bw, *sc))
                fwd = ctx.last_kernel_names()[0]
                assert "score-only" in fwd, fwd
                for k, (q, t) in enumerate(pairs):
                    res, cig, n, begs = _oracle(q, t, mode, bw, sc)
                    if n == S.ORC_ERR_TRACE:
                        continue
                    got = (int(so[k]["score"]), int(so[k]["qe"]), int(so[k]["te"]))
                    assert sst[k] == 0 and got == (int(res[0]), int(res[2]), int(res[4])), (tag, scname, mode, bw, k, got, res)
