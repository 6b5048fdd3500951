"""CPU: the helpers of the plan / run surface tests (plan_surface_cases.py) -- the arena checker rejects every kind of broken arena it is
there to find, expected() agrees with the reference's recorded results, and the corpora hold what the GPU tests rely on."""
import os

import numpy as np
import pytest

import plan_surface_cases as PC
import support as S

SENT = PC.SENTINEL


def _arena(cigs, cap, extra=64, upto=None):
    """a correct arena of `cap` words and `extra` guard words: the pairs whose words end at or below `upto` (default cap) written"""
    off = np.zeros(len(cigs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cigs])
    words = np.full(cap + extra, SENT, dtype=np.uint32)
    lim = cap if upto is None else upto
    for k, c in enumerate(cigs):
        if int(off[k + 1]) <= lim:
            words[int(off[k]):int(off[k + 1])] = c
    return words, off


def _cigs():
    rng = np.random.default_rng(1)
    cigs = [((rng.integers(1, 200, int(m)).astype(np.uint32) << 4) | rng.choice([0, 1, 2], int(m)).astype(np.uint32)) for m in (5, 1, 0, 9, 3, 0, 7)]
    return cigs, int(sum(len(c) for c in cigs))


@pytest.mark.parametrize("cap_of", [lambda t: t + 10, lambda t: t, lambda t: t - 1, lambda t: t // 2, lambda t: 1, lambda t: 0])
def test_check_arena_accepts_a_correct_arena(cap_of):
    cigs, total = _cigs()
    cap = cap_of(total)
    words, off = _arena(cigs, cap)
    fitting = sum(1 for k, c in enumerate(cigs) if len(c) and int(off[k + 1]) <= cap)
    assert PC.check_arena(words, cap, SENT, off, cigs, True) == fitting
    # after an overflow a fitting pair may be missing where the route does not promise it
    words, off = _arena(cigs, cap, upto=cap // 2)
    assert PC.check_arena(words, cap, SENT, off, cigs, False) <= fitting


def test_check_arena_rejects_a_word_written_at_the_capacity():
    cigs, total = _cigs()
    words, off = _arena(cigs, total - 1)
    words[total - 1] = cigs[-1][-1]             # the last pair's last word, right where it would go in a larger arena
    with pytest.raises(AssertionError, match="capacity"):
        PC.check_arena(words, total - 1, SENT, off, cigs, True)
    words, off = _arena(cigs, total)
    words[total + 63] = 16
    with pytest.raises(AssertionError, match="capacity"):
        PC.check_arena(words, total, SENT, off, cigs, True)


def test_check_arena_rejects_a_pair_half_written():
    cigs, total = _cigs()
    words, off = _arena(cigs, total)
    words[int(off[3]) + 4:int(off[4])] = SENT
    with pytest.raises(AssertionError, match="pair 3"):
        PC.check_arena(words, total, SENT, off, cigs, False)
    # ... and the head of a pair that does not fit
    words, off = _arena(cigs, total - 1)
    words[int(off[6]):total - 1] = cigs[6][:-1]
    with pytest.raises(AssertionError, match="pair 6"):
        PC.check_arena(words, total - 1, SENT, off, cigs, False)


def test_check_arena_rejects_words_at_another_pairs_offset():
    cigs, total = _cigs()
    words, off = _arena(cigs, total)
    words[int(off[3]):int(off[3]) + 3] = cigs[4]
    words[int(off[3]) + 3:int(off[4])] = SENT
    words[int(off[4]):int(off[5])] = SENT
    with pytest.raises(AssertionError, match="pair 3"):
        PC.check_arena(words, total, SENT, off, cigs, False)


def test_check_arena_rejects_a_short_or_unordered_offset_array():
    cigs, total = _cigs()
    words, off = _arena(cigs, total)
    with pytest.raises(AssertionError, match="entries"):
        PC.check_arena(words, total, SENT, off[:-1], cigs, True)
    bad = off.copy()
    bad[3], bad[4] = off[4], off[3]
    with pytest.raises(AssertionError, match="running sum"):
        PC.check_arena(words, total, SENT, bad, cigs, True)
    seven = np.full(len(off), 7, dtype=np.uint64)
    with pytest.raises(AssertionError, match="running sum"):
        PC.check_arena(words, total, SENT, seven, cigs, True)


def test_check_arena_rejects_a_missing_fitting_pair_when_all_must_be_present():
    cigs, total = _cigs()
    words, off = _arena(cigs, total)
    words[int(off[4]):int(off[5])] = SENT
    assert PC.check_arena(words, total, SENT, off, cigs, False) == 4
    with pytest.raises(AssertionError, match="pair 4"):
        PC.check_arena(words, total, SENT, off, cigs, True)


def _golden(name):
    g = np.load(os.path.join(S.ROOT, "tests", "golden", name))
    groups = {}
    for k in range(int(g["n"][0])):
        groups.setdefault(tuple(int(x) for x in g["meta_%d" % k]), []).append(k)
    return g, groups


@pytest.mark.parametrize("name,kind", [("align8.npz", "align"), ("edit.npz", "edit")])
def test_expected_agrees_with_the_recorded_reference_results(name, kind):
    g, groups = _golden(name)
    done = 0
    for meta, ks in groups.items():
        pairs = [(g["q_%d" % k], g["t_%d" % k]) for k in ks]
        rec, cigs, off, st = PC.expected(pairs, kind, meta[0], meta[1], tuple(meta[2:8]) if kind == "align" else None)
        assert not st.any() and len(off) == len(ks) + 1
        for i, k in enumerate(ks):
            assert np.array_equal(rec[i], g["res_%d" % k]) and np.array_equal(cigs[i], g["cig_%d" % k]), (meta, k)
            assert int(off[i + 1]) - int(off[i]) == len(g["cig_%d" % k])
            done += 1
    assert done > 60


def test_expected_gives_bad_and_empty_pairs_a_zero_record_and_no_words():
    c = PC.small()
    for cfg in PC.CONFIGS:
        rec, cigs, off, st = PC.expected(c.pairs, *cfg, key="small")
        assert st[PC.EMPTY_QUERY] == PC.ST_EMPTY and st[PC.EMPTY_TARGET] == PC.ST_EMPTY and st[PC.BAD_BASE] == PC.ST_BAD_BASE
        assert int(np.count_nonzero(st)) == 3
        for k in (PC.EMPTY_QUERY, PC.EMPTY_TARGET, PC.BAD_BASE):
            assert not rec[k].any() and len(cigs[k]) == 0 and off[k] == off[k + 1]
        assert all(len(cigs[k]) > 0 for k in c.good())
        assert int(off[-1]) == sum(len(x) for x in cigs) > 64 and len(cigs[-1]) > 0          # (a capacity of total - 1 leaves the last pair out)


def test_corpora_have_the_shapes_the_gpu_tests_rely_on():
    c = PC.small()
    assert len(c) == PC.N_SMALL == 96
    good = c.good()
    assert len(good) == 93 and min(c.qlen[good]) >= 30 and max(c.tlen) == 1500 and min(c.tlen[good]) == 40
    assert c.qlen[PC.EMPTY_QUERY] == 0 and c.tlen[PC.EMPTY_TARGET] == 0 and 9 in c.pairs[PC.BAD_BASE][0]
    assert c.toff[PC.SHARES_TO] == c.toff[PC.SHARES_FROM] and c.tlen[PC.SHARES_TO] == c.tlen[PC.SHARES_FROM]
    for k, (q, t) in enumerate(c.pairs):
        assert np.array_equal(c.seqs[int(c.qoff[k]):int(c.qoff[k]) + len(q)], q) and np.array_equal(c.seqs[int(c.toff[k]):int(c.toff[k]) + len(t)], t)
    # no pair the compact traceback hands over: the device-pointer calls would flag it (that the reference's traceback terminates on every pair
    # is expected()'s own assertion, above for small() and in the GPU tests for the other corpora)
    assert not any(PC.needs_handover(*c.pairs[k]) for k in good)
    d = PC.same_lengths(1)
    assert np.array_equal(d.qlen, c.qlen) and np.array_equal(d.tlen, c.tlen) and np.array_equal(d.toff, c.toff) and np.array_equal(d.qoff, c.qoff)
    assert len(d.seqs) == len(c.seqs) and not np.array_equal(d.seqs, c.seqs) and d.good() == good
    assert not any(PC.needs_handover(*d.pairs[k]) for k in good)
    s = PC.short_many()
    assert len(s) == PC.N_SHORT == 16400 > 16384 and min(s.tlen) == 20 and max(s.tlen) == 40 and min(s.qlen) >= 19
