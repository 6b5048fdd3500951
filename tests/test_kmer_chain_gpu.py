"""GPU: the device k-mer chainer (bsa_kmer_chain_batch) word for word against the host chainer (bsa_kmer_chain), and
bsa_kmer_edit_batch2 with BSA_KMER_CHAIN_DEVICE byte for byte against bsa_kmer_edit_batch.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import kmer_chain_cases as KC
import kmer_support as K
import support as S
from test_kmer_cpu import golden_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    import bsalign_amd as B
    c = B.Context(0)
    yield c
    c.close()


def _check_against_host(ctx, pairs, ksz, names=None, on_host=0):
    got, st = ctx.kmer_chain_batch(pairs, ksz=ksz, with_status=True)
    ms, dev, host = ctx.last_kmer_chain_ms()
    assert host == on_host and dev == len(pairs) - on_host, (dev, host)
    rc, maps, off, want_st = KC.host_arena(pairs, ksz)
    assert np.array_equal(st, want_st)
    for k in range(len(pairs)):
        want = maps[int(off[k]):int(off[k + 1])]
        assert len(got[k]) == len(want) and np.array_equal(got[k], want), (names[k] if names else k, ksz, len(got[k]), len(want))
    return got


def test_fixture_pairs_equal_the_host_chainer(ctx):
    cases = list(golden_cases())
    with_anchors = 0
    for ksz in sorted({c[1] for c in cases}):
        sel = [(c[2], c[3]) for c in cases if c[1] == ksz]
        got = _check_against_host(ctx, sel, ksz)
        with_anchors += sum(1 for g in got if len(g))
    assert with_anchors >= len(cases) // 2          # (the pairs at k-mer size 3 have no chain on the host either; most others do)


@pytest.mark.parametrize("ksz", [8, 11, 13, 15, 20])
def test_named_cases_equal_the_host_chainer(ctx, ksz):
    cs = KC.cases(ksz)
    got = _check_against_host(ctx, [(q, t) for _, q, t in cs], ksz, names=[c[0] for c in cs])
    by = {c[0]: g for c, g in zip(cs, got)}
    assert len(by["identical"]) > 1800 and len(by["revcomp"]) == 0 and len(by["polyA"]) == 0 and len(by["polyA_k"]) == 0
    assert len(by["L10000_d05"]) > 100 and len(by["L30000_d05"]) > 300 and len(by["L10000_d40"]) < 100 and len(by["staircase"]) > 0


def test_random_batch_equals_the_host_chainer(ctx):
    rng = np.random.default_rng(77)
    pairs = []
    for it in range(300):
        L = int(rng.integers(20, 4000))
        T = rng.integers(0, 4, L).astype(np.uint8)
        Q = S.mutate(rng, T, float(rng.choice([0.0, 0.05, 0.15, 0.40])))
        if it % 7 == 3 and len(Q) > 400:
            a = int(rng.integers(50, len(Q) - 100))
            Q = np.concatenate([Q[:a], rng.integers(0, 4, int(rng.integers(30, 600))).astype(np.uint8), Q[a:]])
        pairs.append((Q, T))
    for ksz in (8, 13):
        _check_against_host(ctx, pairs, ksz)


def test_pair_above_the_limit_goes_to_the_host(ctx):
    rng = np.random.default_rng(3)
    T = rng.integers(0, 4, KC.DEV_MAX // 2 + 40).astype(np.uint8)
    Q = T.copy()
    Q[::97] = (Q[::97] + 1) & 3
    small = rng.integers(0, 4, 800).astype(np.uint8)
    got = _check_against_host(ctx, [(small.copy(), small), (Q, T)], 13, on_host=1)
    assert len(got[1]) > 1000
    # a pair whose slice does not fit the workspace limit is the host's as well; chunks of a few pairs give the same words
    import bsalign_amd as B
    t2 = rng.integers(0, 4, 20000).astype(np.uint8)
    pairs = [(S.mutate(rng, t2[:3000], 0.05), t2[:3000]) for _ in range(9)] + [(t2.copy(), t2)]
    assert B.lib().bsa_ctx_set_workspace_limit(ctx.h, C.c_size_t(300000)) == 0
    try:
        _check_against_host(ctx, pairs, 13, on_host=1)
    finally:
        B.lib().bsa_ctx_set_workspace_limit(ctx.h, C.c_size_t(0))


def test_arena_too_small_n_zero_and_no_status(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(12)
    T = rng.integers(0, 4, 2000).astype(np.uint8)
    bad = T.copy()
    bad[5] = 4
    pairs = [(S.mutate(rng, T, 0.05), T), (np.zeros(0, np.uint8), T), (bad, T), (T, np.zeros(0, np.uint8)), (S.mutate(rng, T, 0.1), T)]
    rc, maps, off, st = KC.host_arena(pairs, 13)
    need = int(off[-1])
    assert need > 0
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    fn = B.lib().bsa_kmer_chain_batch
    n = len(pairs)
    for cap, want_rc in ((need, 0), (need - 1, KC.E_CIGAR_CAP), (0, KC.E_CIGAR_CAP)):
        m = np.full(max(cap, 1) + 1, 0xABABABABABABABAB, dtype=np.uint64)
        o = np.zeros(n + 1, dtype=np.uint64)
        rc = fn(ctx.h, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, 13, B._p(m) if cap else None, cap, B._p(o), None)     # status == NULL
        assert rc == want_rc and int(o[n]) == need
        if rc == 0:
            assert np.array_equal(o, off) and np.array_equal(m[:need], maps) and m[need] == 0xABABABABABABABAB
        else:
            assert np.all(m == 0xABABABABABABABAB)
    got, gst = ctx.kmer_chain_batch(pairs, ksz=13, with_status=True)
    assert list(gst) == [0, KC.ST_EMPTY, KC.ST_BAD_BASE, KC.ST_EMPTY, 0] and [len(g) for g in got][1:4] == [0, 0, 0]
    # n == 0
    o = np.full(1, 5, dtype=np.uint64)
    assert fn(ctx.h, None, 0, None, None, None, None, 0, 13, None, 0, B._p(o), None) == 0 and o[0] == 0
    assert ctx.kmer_chain_batch([], ksz=13) == []
    # k-mer size 0: no anchors, the status still says what the pair is
    got, gst = ctx.kmer_chain_batch(pairs, ksz=0, with_status=True)
    assert all(len(g) == 0 for g in got) and list(gst) == [0, KC.ST_EMPTY, KC.ST_BAD_BASE, KC.ST_EMPTY, 0]


def _edit_both(ctx, pairs, ksz, arena):
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    n = len(pairs)
    par = B.KmerParams()
    par.ksz, par.threads = ksz, 0
    res = []
    for flags in (None, B.KMER_CHAIN_DEVICE):
        out = np.zeros(n, dtype=B.RESULT_DTYPE)
        st = np.zeros(n, dtype=np.uint32)
        cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16 if arena else 0
        cig = np.zeros(max(cap, 1), dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        args = [ctx.h, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(par), B._p(out),
                B._p(cig) if arena else None, cap, B._p(off) if arena else None, B._p(st)]
        rc = B.lib().bsa_kmer_edit_batch(*args) if flags is None else B.lib().bsa_kmer_edit_batch2(*args, flags)
        assert rc == 0
        res.append((out.tobytes(), cig[:int(off[n])].tobytes(), off.tobytes(), st.tobytes()))
    return res


@pytest.mark.parametrize("arena", [True, False])
def test_edit_batch2_is_byte_identical_on_the_fixture(ctx, arena):
    cases = list(golden_cases())
    for ksz in sorted({c[1] for c in cases}):
        a, b = _edit_both(ctx, [(c[2], c[3]) for c in cases if c[1] == ksz], ksz, arena)
        assert a == b, ksz
        assert ctx.last_kmer_chain_ms()[2] == 0


@pytest.mark.parametrize("arena", [True, False])
def test_edit_batch2_is_byte_identical_on_a_random_batch(ctx, arena):
    rng = np.random.default_rng(31 + arena)
    pairs = []
    for it in range(3000):
        L = int(rng.integers(30, 700))
        T = rng.integers(0, 4, L).astype(np.uint8)
        Q = T.copy()
        m = rng.random(L) < float(rng.choice([0.0, 0.03, 0.10, 0.40]))
        Q[m] = (Q[m] + rng.integers(1, 4, int(m.sum()))) & 3
        if it % 5 == 1:
            a = int(rng.integers(0, L))
            Q = np.concatenate([Q[:a], rng.integers(0, 4, int(rng.integers(1, 80))).astype(np.uint8), Q[a:]])
        if it % 11 == 4:
            Q = np.delete(Q, slice(L // 3, L // 3 + int(rng.integers(1, 40))))
        pairs.append((Q, T))
    # the pairs the two calls must treat alike: empty sides, a base code above 3 (on an anchor column and off it), sequences shorter than k
    T = rng.integers(0, 4, 600).astype(np.uint8)
    b1, b2 = T.copy(), T.copy()
    b1[300] = 4
    b2[0] = 200
    pairs += [(np.zeros(0, np.uint8), T), (T, np.zeros(0, np.uint8)), (b1, T), (T, b2), (b2, b1), (T[:9].copy(), T), (T.copy(), T)]
    a, b = _edit_both(ctx, pairs, 11, arena)
    assert a[3] == b[3], "status differs"
    assert a[0] == b[0], "records differ"
    assert a[2] == b[2] and a[1] == b[1], "CIGAR words differ"
    ms, dev, host = ctx.last_kmer_chain_ms()
    assert dev == len(pairs) and host == 0


def test_python_keyword_and_unknown_flag(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(2)
    T = rng.integers(0, 4, 2500).astype(np.uint8)
    pairs = [(S.mutate(rng, T, 0.08), T) for _ in range(6)]
    o1, c1, s1 = ctx.kmer_edit_batch(pairs, ksz=13)
    o2, c2, s2 = ctx.kmer_edit_batch(pairs, ksz=13, device_chain=True)
    assert np.array_equal(o1, o2) and np.array_equal(s1, s2) and all(np.array_equal(x, y) for x, y in zip(c1, c2))
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    par = B.KmerParams()
    par.ksz, par.threads = 13, 0
    out = np.zeros(len(pairs), dtype=B.RESULT_DTYPE)
    assert B.lib().bsa_kmer_edit_batch2(ctx.h, B._p(seqs), seqs.size, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), len(pairs), C.byref(par),
                                        B._p(out), None, 0, None, None, 4) == -2
