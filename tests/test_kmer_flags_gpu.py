"""GPU: the k-mer calls with BSA_MODE_SEQ2BIT / BSA_MODE_QSTRAND.  bsa_kmer_chain_batch2 word for word against the host chainer (bsa_kmer_chain) on the
logical pairs, bsa_kmer_edit_batch2 byte for byte against bsa_kmer_edit_batch (no flags) on the host-made 1 B/base blob that holds the logical pairs.
Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import kmer_chain_cases as KC
import kmer_flags_cases as F
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


def _chain2(ctx, b, ksz, flags=None, cap=None, seqs_bytes=None):
    """bsa_kmer_chain_batch2 on a built batch -> (rc, [anchors of pair k], maps_off, status)"""
    import bsalign_amd as B
    n = len(b.qlen)
    if cap is None:
        cap = int(np.minimum(b.qlen, b.tlen).sum()) + 1
    maps = np.zeros(max(cap, 1), dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    st = np.full(max(n, 1), 0xEE, dtype=np.uint32)
    rc = B.lib().bsa_kmer_chain_batch2(ctx.h, B._p(b.seqs), b.seqs.nbytes if seqs_bytes is None else seqs_bytes, B._p(b.qoff), B._p(b.qlen), B._p(b.toff), B._p(b.tlen),
                                       n, ksz, B._p(maps), cap, B._p(off), B._p(st), b.flags if flags is None else flags)
    got = [maps[int(off[k]):int(off[k + 1])].copy() for k in range(n)] if rc == 0 else None
    return rc, got, off, st[:n]


def _check_chain(ctx, pairs, strands, ksz, packed, want=None, names=None, on_host=0, guards=False):
    """the flagged call on the stored blob against the host arena of the logical pairs"""
    b = F.build(pairs, strands, packed, guards=guards)
    rc, got, off, st = _chain2(ctx, b, ksz)
    assert rc == 0
    ms, dev, host = ctx.last_kmer_chain_ms()
    assert host == on_host and dev == len(pairs) - on_host, (dev, host)
    wrc, maps, woff, want_st = want if want is not None else KC.host_arena(pairs, ksz)
    assert np.array_equal(st, want_st)                       # (no pair here has a base code above 3, so packed input changes no status)
    assert np.array_equal(off, woff)
    for k in range(len(pairs)):
        w = maps[int(woff[k]):int(woff[k + 1])]
        assert len(got[k]) == len(w) and np.array_equal(got[k], w), (names[k] if names else k, ksz, packed, strands is not None, len(got[k]), len(w))
    return b, got


@pytest.mark.parametrize("ksz", [8, 13, 15, 20])
def test_named_cases_equal_the_host_chainer(ctx, ksz):
    names, pairs, strands = F.named_pairs(ksz)
    want = KC.host_arena(pairs, ksz)
    for combo, packed, strand in F.COMBOS:
        _, got = _check_chain(ctx, pairs, strands if strand else None, ksz, packed, want=want, names=names)
        by = dict(zip(names, got))
        for name in ("identical", "identical/marked", "L10000_d05/marked", "staircase/marked"):
            assert len(by[name]) > (1800 if name.startswith("identical") else 0), (combo, name)
        assert len(by["revcomp"]) == 0 and len(by["revcomp/marked"]) == 0 and len(by["polyA/marked"]) == 0
    # the stored bytes of `revcomp`, marked: the query the call chains is the target itself
    sq, t = next((q, t) for name, q, t in KC.cases(ksz) if name == "revcomp")
    for combo, packed, strand in F.COMBOS:
        if strand:
            _, got = _check_chain(ctx, [(F.revcomp(sq), t), (sq, t)], [True, False], ksz, packed)
            assert len(got[0]) > 1800 and len(got[1]) == 0
            i = np.arange(len(t), dtype=np.uint64)
            assert np.all(np.isin(got[0], (i << np.uint64(32)) | i))


def test_random_batch_equals_the_host_chainer(ctx):
    pairs, strands = F.random_pairs()
    for ksz in (8, 13):
        want = KC.host_arena(pairs, ksz)
        for combo, packed, strand in F.COMBOS:
            _, got = _check_chain(ctx, pairs, strands if strand else None, ksz, packed, want=want)
            marked = [len(g) for g, s in zip(got, strands) if s]
            assert 3 * sum(1 for c in marked if c) >= len(marked)


def test_a_read_stored_once_serves_both_strands_and_guards_are_not_read(ctx):
    rng = np.random.default_rng(21)
    r = rng.integers(0, 4, 2000).astype(np.uint8)
    ta = S.mutate(rng, r, 0.04)
    tb = F.revcomp(r)                                        # target B is the read's reverse complement: the marked pair chains B against B
    short = rng.integers(0, 4, 37).astype(np.uint8)
    pairs = [(r, ta), (F.revcomp(r), tb), (F.revcomp(r), S.mutate(rng, tb, 0.08)), (short, F.revcomp(short)), (F.revcomp(short), F.revcomp(short))]
    strands = [False, True, True, False, True]
    for ksz in (8, 13):
        want = KC.host_arena(pairs, ksz)
        b, got = _check_chain(ctx, pairs, strands, ksz, False, want=want)
        assert b.shared >= 2
        i = np.arange(2000, dtype=np.uint64)
        assert len(got[1]) > 1800 and np.all(np.isin(got[1], (i << np.uint64(32)) | i)) and len(got[0]) > 100
        b, got = _check_chain(ctx, pairs, strands, ksz, True, want=want, guards=True)
        assert b.shared >= 2 and int(b.seqs[0]) == F.FRONT_GUARD and int(b.seqs[-1]) == F.BACK_GUARD
        for k in range(len(pairs)):
            assert (int(b.qoff[k]) & ~F.QOFF_REVCOMP) % 4 and int(b.toff[k]) % 4
        # the words in front of the first read and behind the last one hold no base of any read: their content changes nothing
        b.seqs[0] = ~b.seqs[0]
        b.seqs[-1] = 0
        rc, got2, off2, st2 = _chain2(ctx, b, ksz)
        assert rc == 0 and np.array_equal(off2, want[2]) and all(np.array_equal(x, y) for x, y in zip(got, got2)) and np.array_equal(st2, want[3])
        par_ok = _edit_flagged(ctx, b, ksz, True, True)
        b.seqs[0] = ~b.seqs[0]
        b.seqs[-1] = F.BACK_GUARD
        assert _edit_flagged(ctx, b, ksz, True, True) == par_ok == _edit_plain(ctx, b, ksz, True)


def test_pairs_the_device_does_not_take_go_to_the_host(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(3)
    T = rng.integers(0, 4, KC.DEV_MAX // 2 + 40).astype(np.uint8)
    Q = T.copy()
    Q[::97] = (Q[::97] + 1) & 3
    small = rng.integers(0, 4, 800).astype(np.uint8)
    _, got = _check_chain(ctx, [(small.copy(), small), (Q, T)], [False, True], 13, True, on_host=1)
    assert len(got[1]) > 1000
    _, got = _check_chain(ctx, [(small.copy(), small), (Q, T)], [True, False], 13, True, on_host=1)
    assert len(got[1]) > 1000
    t2 = rng.integers(0, 4, 20000).astype(np.uint8)
    pairs = [(S.mutate(rng, t2[:3000], 0.05), t2[:3000]) for _ in range(9)] + [(S.mutate(rng, t2, 0.02), t2)]
    strands = [k % 2 == 1 for k in range(10)]
    assert B.lib().bsa_ctx_set_workspace_limit(ctx.h, C.c_size_t(300000)) == 0
    try:
        _, got = _check_chain(ctx, pairs, strands, 13, True, on_host=1)
        assert len(got[9]) > 500
        _check_chain(ctx, pairs, strands, 13, False, on_host=1)
    finally:
        B.lib().bsa_ctx_set_workspace_limit(ctx.h, C.c_size_t(0))


def _edit_call(ctx, seqs, qoff, qlen, toff, tlen, ksz, arena, flags):
    import bsalign_amd as B
    n = len(qlen)
    par = B.KmerParams()
    par.ksz, par.threads = ksz, 0
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.full(max(n, 1), 0xEE, dtype=np.uint32)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16 if arena else 0
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    args = [ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(par), B._p(out),
            B._p(cig) if arena else None, cap, B._p(off) if arena else None, B._p(st)]
    rc = B.lib().bsa_kmer_edit_batch(*args) if flags is None else B.lib().bsa_kmer_edit_batch2(*args, flags)
    assert rc == 0, rc
    return out.tobytes(), cig[:int(off[n])].tobytes(), off.tobytes(), st[:n].tobytes()


def _edit_plain(ctx, b, ksz, arena):
    """the expectation: bsa_kmer_edit_batch, no flags, on the host-made 1 B/base blob of the logical pairs"""
    return _edit_call(ctx, *b.plain, ksz, arena, None)


def _edit_flagged(ctx, b, ksz, arena, device):
    import bsalign_amd as B
    res = _edit_call(ctx, b.seqs, b.qoff, b.qlen, b.toff, b.tlen, ksz, arena, b.flags | (B.KMER_CHAIN_DEVICE if device else 0))
    if device:
        assert ctx.last_kmer_chain_ms()[1:] == (len(b.qlen), 0)
    return res


def _edit_cross(ctx, pairs, strands, ksz, arena, combos=F.COMBOS):
    want = None
    for combo, packed, strand in combos:
        b = F.build(pairs, strands if strand else None, packed)
        if want is None:
            want = _edit_plain(ctx, b, ksz, arena)
        for device in (True, False):
            got = _edit_flagged(ctx, b, ksz, arena, device)
            assert got[3] == want[3], ("status differs", combo, device, ksz)
            assert got[0] == want[0], ("records differ", combo, device, ksz)
            assert got[2] == want[2] and got[1] == want[1], ("CIGAR words differ", combo, device, ksz)


@pytest.mark.parametrize("arena", [True, False])
def test_edit_batch2_is_byte_identical_on_the_fixture(ctx, arena):
    cases = list(golden_cases())
    for ksz in sorted({c[1] for c in cases}):
        pairs = [(c[2], c[3]) for c in cases if c[1] == ksz]
        _edit_cross(ctx, pairs + pairs, [False] * len(pairs) + [True] * len(pairs), ksz, arena)


@pytest.mark.parametrize("arena", [True, False])
def test_edit_batch2_is_byte_identical_on_a_random_batch(ctx, arena):
    pairs, strands = F.random_edit_pairs(31 + arena)
    _edit_cross(ctx, pairs, strands, 11, arena)
    # base codes above 3 exist at 1 B/base only: unmarked as in the plain call (chained on their bytes), marked where q' is defined
    bp, bs = F.bad_base_tail()
    _edit_cross(ctx, pairs[:200] + bp, strands[:200] + bs, 11, arena, combos=F.COMBOS[:1])


def test_marked_query_with_a_bad_base_is_flagged_and_empty(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(8)
    T = rng.integers(0, 4, 600).astype(np.uint8)
    bad = T.copy()
    bad[300] = 4
    b = F.build([(T, T), (T, T)], [False, True], False)
    b.seqs = np.concatenate([b.seqs, bad])                   # the stored query of a third pair: marked, a code above 3
    b.qoff = np.append(b.qoff, np.uint64((len(b.seqs) - 600) | F.QOFF_REVCOMP))
    b.qlen = np.append(b.qlen, np.uint32(600))
    b.toff = np.append(b.toff, b.toff[0])
    b.tlen = np.append(b.tlen, np.uint32(600))
    rc, got, off, st = _chain2(ctx, b, 11)
    assert rc == 0 and list(st) == [0, 0, KC.ST_BAD_BASE] and len(got[2]) == 0 and len(got[0]) > 500
    for device in (True, False):
        for arena in (True, False):
            out, cig, coff, est = _edit_flagged(ctx, b, 11, arena, device)
            out = np.frombuffer(out, dtype=B.RESULT_DTYPE)
            coff = np.frombuffer(coff, dtype=np.uint64)
            assert list(np.frombuffer(est, dtype=np.uint32)) == [0, 0, KC.ST_BAD_BASE]
            assert out[2].tobytes() == bytes(40) and out[0]["mat"] == 600
            if arena:
                assert coff[3] == coff[2] and coff[2] > coff[1] > 0


def test_flags_and_errors(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(2)
    T = rng.integers(0, 4, 2500).astype(np.uint8)
    pairs = [(S.mutate(rng, T, 0.08), T) for _ in range(6)]
    want = KC.host_arena(pairs, 13)
    # QSTRAND with no pair marked is the plain call
    for packed in (False, True):
        b = F.build(pairs, [False] * 6, packed)
        rc, got, off, st = _chain2(ctx, b, 13)
        assert rc == 0 and np.array_equal(off, want[2]) and np.array_equal(np.concatenate(got), want[1]) and not st.any()
        for device in (True, False):
            assert _edit_flagged(ctx, b, 13, True, device) == _edit_plain(ctx, b, 13, True)
    # unknown bits
    b = F.build(pairs, None, False)
    par = B.KmerParams()
    par.ksz, par.threads = 13, 0
    out = np.zeros(len(pairs), dtype=B.RESULT_DTYPE)
    args = [ctx.h, B._p(b.seqs), b.seqs.nbytes, B._p(b.qoff), B._p(b.qlen), B._p(b.toff), B._p(b.tlen), len(pairs), C.byref(par), B._p(out), None, 0, None, None]
    for bad in (4, 2, 0x400, 0x1000, 0x4000, B.MODE_SEQ2BIT | 4):
        assert B.lib().bsa_kmer_edit_batch2(*args, bad) == -2, bad
    for bad in (1, 4, 0x400, 0x1000, B.MODE_QSTRAND | 1):
        assert _chain2(ctx, b, 13, flags=bad)[0] == -2, bad
    # bit 63 without QSTRAND is an offset outside the blob
    bq = F.build(pairs, [True] * 6, False)
    assert _chain2(ctx, bq, 13, flags=0)[0] == -2
    args = [ctx.h, B._p(bq.seqs), bq.seqs.nbytes, B._p(bq.qoff), B._p(bq.qlen), B._p(bq.toff), B._p(bq.tlen), len(pairs), C.byref(par), B._p(out), None, 0, None, None]
    assert B.lib().bsa_kmer_edit_batch2(*args, B.KMER_CHAIN_DEVICE) == -2 and B.lib().bsa_kmer_edit_batch2(*args, 0) == -2
    assert B.lib().bsa_kmer_edit_batch2(*args, B.MODE_QSTRAND) == 0
    # SEQ2BIT: whole words only, and no read past 4 * seqs_bytes bases
    bp = F.build(pairs, None, True)
    assert _chain2(ctx, bp, 13, seqs_bytes=bp.seqs.nbytes - 4)[0] == -2
    assert _chain2(ctx, bp, 13, seqs_bytes=bp.seqs.nbytes - 8)[0] == -2          # the last read ends in the last word
    bp.tlen[5] += np.uint32(4 * bp.seqs.nbytes - (int(bp.toff[5]) + int(bp.tlen[5])) + 1)
    assert _chain2(ctx, bp, 13)[0] == -2
    pargs = [ctx.h, B._p(bp.seqs), bp.seqs.nbytes, B._p(bp.qoff), B._p(bp.qlen), B._p(bp.toff), B._p(bp.tlen), len(pairs), C.byref(par), B._p(out), None, 0, None, None]
    assert B.lib().bsa_kmer_edit_batch2(*pargs, B.MODE_SEQ2BIT) == -2
    pargs[2] = bp.seqs.nbytes - 4
    assert B.lib().bsa_kmer_edit_batch2(*pargs, B.MODE_SEQ2BIT | B.KMER_CHAIN_DEVICE) == -2
    # arena too small: maps_off[n] says what a retry needs
    b = F.build(pairs, [k % 2 == 1 for k in range(6)], True)
    need = int(KC.host_arena(pairs, 13)[2][-1])
    rc, _, off, _ = _chain2(ctx, b, 13, cap=need - 1)
    assert rc == KC.E_CIGAR_CAP and int(off[6]) == need
    assert _chain2(ctx, b, 13, cap=need)[0] == 0


def test_python_keywords_equal_the_c_call(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(4)
    T = rng.integers(0, 4, 2500).astype(np.uint8)
    stored = [(S.mutate(rng, T, 0.08) if k % 2 == 0 else F.revcomp(S.mutate(rng, T, 0.08)), T) for k in range(6)]
    strands = [k % 2 == 1 for k in range(6)]
    logical = [(F.revcomp(q) if s else q, t) for (q, t), s in zip(stored, strands)]
    want = KC.host_arena(logical, 13)
    o0, c0, s0 = ctx.kmer_edit_batch(logical, ksz=13)
    for seq2bit in (False, True):
        got, st = ctx.kmer_chain_batch(stored, ksz=13, with_status=True, seq2bit=seq2bit, strands=strands)
        b = F.Batch()
        b.seqs, b.qoff, b.qlen, b.toff, b.tlen = B.pack_pairs(stored, seq2bit, strands)
        b.flags = B.MODE_QSTRAND | (B.MODE_SEQ2BIT if seq2bit else 0)
        rc, cgot, off, cst = _chain2(ctx, b, 13)
        assert rc == 0 and np.array_equal(st, cst) and all(np.array_equal(x, y) for x, y in zip(got, cgot))
        assert np.array_equal(np.concatenate(got), want[1]) and all(len(g) > 100 for g in got)
        for dev in (False, True):
            o, c, s = ctx.kmer_edit_batch(stored, ksz=13, device_chain=dev, seq2bit=seq2bit, strands=strands)
            assert np.array_equal(o, o0) and np.array_equal(s, s0) and all(np.array_equal(x, y) for x, y in zip(c, c0))
    got = ctx.kmer_chain_batch(logical, ksz=13, seq2bit=True)
    assert np.array_equal(np.concatenate(got), want[1])
