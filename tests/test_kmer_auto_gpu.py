"""GPU: the k-mer calls with BSA_KMER_STRAND_AUTO.  bsa_kmer_chain_batch2 word for word against the host chainer (bsa_kmer_chain) run on (q, t) and on a
host-made (revcomp(q), t) -- reverse exactly when the second list is longer --, bsa_kmer_edit_batch2 byte for byte against bsa_kmer_edit_batch (no flags)
on a host-made 1 B/base blob that holds each pair on its expected strand.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import kmer_auto_cases as A
import kmer_chain_cases as KC
import kmer_flags_cases as F
import support as S

pytestmark = pytest.mark.gpu
LAYOUTS = (("bytes", False, False), ("packed", True, True))          # name, packed, guard words


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


def _chain2(ctx, b, ksz, flags, cap=None, status=True):
    """bsa_kmer_chain_batch2 on a built batch -> (rc, [anchors of pair k], maps_off, status)"""
    import bsalign_amd as B
    n = len(b.qlen)
    if cap is None:
        cap = int(np.minimum(b.qlen, b.tlen).sum()) + 1
    maps = np.zeros(max(cap, 1), dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    st = np.full(max(n, 1), 0xEE, dtype=np.uint32)
    rc = B.lib().bsa_kmer_chain_batch2(ctx.h, B._p(b.seqs), b.seqs.nbytes, B._p(b.qoff), B._p(b.qlen), B._p(b.toff), B._p(b.tlen),
                                       n, ksz, B._p(maps), cap, B._p(off), B._p(st) if status else None, flags)
    got = [maps[int(off[k]):int(off[k + 1])].copy() for k in range(n)] if rc == 0 else None
    return rc, got, off, st[:n]


def _check_auto(ctx, pairs, ksz, packed, guards, want, names=None, on_host=0):
    """the flagged call on the stored pairs against the host expectation -> (batch, anchors, strands)"""
    b = F.build(pairs, None, packed, guards=guards)
    rc, got, off, st = _chain2(ctx, b, ksz, b.flags | A.KMER_STRAND_AUTO)
    assert rc == 0
    ms, dev, host = ctx.last_kmer_chain_ms()
    assert host == on_host and dev == len(pairs) - on_host, (dev, host)
    woff, per, wst, wstrands = want
    found = (st & np.uint32(A.ST_REVCOMP)) != 0
    for k in range(len(pairs)):
        who = (names[k] if names else k, ksz, packed)
        assert bool(found[k]) == bool(wstrands[k]), ("strand", who, len(got[k]), len(per[k]))
        assert len(got[k]) == len(per[k]) and np.array_equal(got[k], per[k]), ("anchors", who, len(got[k]), len(per[k]))
    assert np.array_equal(off, woff)
    assert np.array_equal(st & ~np.uint32(A.ST_REVCOMP), wst)
    return b, got, found


@pytest.mark.parametrize("ksz", [8, 13, 15, 20])
def test_named_cases_equal_the_host_chainer_on_the_better_strand(ctx, ksz):
    names, pairs = A.named_pairs(ksz)
    want = A.expected(pairs, ksz)
    by = dict(zip(names, range(len(names))))
    for layout, packed, guards in LAYOUTS:
        _, got, found = _check_auto(ctx, pairs, ksz, packed, guards, want, names=names)
        assert not found[by["identical"]] and found[by["identical/rc"]] and len(got[by["identical/rc"]]) > 1800
        assert found[by["revcomp"]] and not found[by["revcomp/rc"]]
        assert not found[by["palindrome"]] and not found[by["tie_with_anchors"]] and len(got[by["tie_with_anchors"]]) > 500
        assert not found[by["both_fwd_wins"]] and found[by["both_rev_wins"]] and len(got[by["both_rev_wins"]]) > 20
        assert not found[by["empty_q"]] and not found[by["short_t/rc"]] and not found[by["polyA"]]


@pytest.mark.parametrize("ksz", [8, 13])
def test_random_batch_equals_the_host_chainer_on_the_better_strand(ctx, ksz):
    pairs, flip = A.random_pairs()
    want = A.expected(pairs, ksz)
    for layout, packed, guards in LAYOUTS:
        _, _, found = _check_auto(ctx, pairs, ksz, packed, guards, want)
        assert 3 * int((found & flip).sum()) >= int(flip.sum())


def test_pairs_the_device_does_not_take_are_chained_twice_on_the_host(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(3)
    t2 = rng.integers(0, 4, 20000).astype(np.uint8)
    pairs = [(S.mutate(rng, t2[:3000], 0.05), t2[:3000]) for _ in range(8)] + [(S.mutate(rng, t2, 0.02), t2), (F.revcomp(S.mutate(rng, t2, 0.03)), t2)]
    pairs = [(F.revcomp(q) if k % 3 == 1 else q, t) for k, (q, t) in enumerate(pairs)]
    want = A.expected(pairs, 13)
    assert want[3][9] and not want[3][8] and want[3][1] and len(want[1][9]) > 500
    # a 3 000-base pair asks for about 0.16 MB of the workspace, a 20 000-base pair for about 1.05 MB: the limit lies between the two
    assert B.lib().bsa_ctx_set_workspace_limit(ctx.h, C.c_size_t(600000)) == 0
    try:
        for layout, packed, guards in LAYOUTS:
            _check_auto(ctx, pairs, 13, packed, guards, want, on_host=2)
    finally:
        B.lib().bsa_ctx_set_workspace_limit(ctx.h, C.c_size_t(0))
    _check_auto(ctx, pairs, 13, False, False, want, on_host=0)


def _edit_call(ctx, seqs, qoff, qlen, toff, tlen, ksz, flags):
    import bsalign_amd as B
    n = len(qlen)
    par = B.KmerParams()
    par.ksz, par.threads = ksz, 0
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.full(max(n, 1), 0xEE, dtype=np.uint32)
    cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    args = [ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(par), B._p(out), B._p(cig), cap, B._p(off), B._p(st)]
    rc = B.lib().bsa_kmer_edit_batch(*args) if flags is None else B.lib().bsa_kmer_edit_batch2(*args, flags)
    assert rc == 0, rc
    return out.tobytes(), cig[:int(off[n])].tobytes(), off.tobytes(), st[:n].copy()


def _edit_cross(ctx, pairs, ksz, layouts):
    """the flagged edit call on the stored pairs, both chain routes, against the plain call on the pairs put on their expected strand by the host"""
    import bsalign_amd as B
    strands = A.expected(pairs, ksz)[3]
    want = _edit_call(ctx, *B.pack_pairs(A.on_strand(pairs, strands)), ksz, None)
    want_st = want[3] | np.where(strands, np.uint32(A.ST_REVCOMP), np.uint32(0)).astype(np.uint32)
    for layout, packed, guards in layouts:
        b = F.build(pairs, None, packed, guards=guards)
        for device in (True, False):
            got = _edit_call(ctx, b.seqs, b.qoff, b.qlen, b.toff, b.tlen, ksz, b.flags | A.KMER_STRAND_AUTO | (B.KMER_CHAIN_DEVICE if device else 0))
            if device:
                assert ctx.last_kmer_chain_ms()[1:] == (len(pairs), 0)
            assert np.array_equal(got[3], want_st), ("status differs", layout, device, np.flatnonzero(got[3] != want_st)[:8])
            assert got[0] == want[0], ("records differ", layout, device)
            assert got[2] == want[2] and got[1] == want[1], ("CIGAR words differ", layout, device)
    return strands, want


def test_edit_batch2_is_byte_identical_on_a_random_batch(ctx):
    pairs, flip = A.random_edit_pairs(31)
    strands, _ = _edit_cross(ctx, pairs, 11, LAYOUTS)
    assert 3 * int((strands & flip).sum()) >= int(flip.sum())


def test_edit_batch2_chains_bad_base_pairs_forward(ctx):
    import bsalign_amd as B
    pairs, _ = A.random_edit_pairs(32)
    bp, _ = F.bad_base_tail()
    both = pairs[:200] + bp
    strands, want = _edit_cross(ctx, both, 11, LAYOUTS[:1])
    assert not strands[200:].any() and strands[:200].any()
    # the tail is what the call without the flag returns for it, with no ST_REVCOMP
    b = F.build(both, None, False)
    for device in (True, False):
        flags = B.KMER_CHAIN_DEVICE if device else 0
        plain = _edit_call(ctx, b.seqs, b.qoff, b.qlen, b.toff, b.tlen, 11, flags)
        auto = _edit_call(ctx, b.seqs, b.qoff, b.qlen, b.toff, b.tlen, 11, flags | A.KMER_STRAND_AUTO)
        assert np.array_equal(auto[3][200:], plain[3][200:]) and (plain[3][200:] & KC.ST_BAD_BASE).all()
        assert auto[0][40 * 200:] == plain[0][40 * 200:]
        po, ao = np.frombuffer(plain[2], np.uint64), np.frombuffer(auto[2], np.uint64)
        assert np.array_equal(ao[200:] - ao[200], po[200:] - po[200])
        assert auto[1][4 * int(ao[200]):] == plain[1][4 * int(po[200]):]


def test_flagged_call_agrees_with_its_own_strands_as_marks(ctx):
    names, pairs = A.named_pairs(13)
    rp, _ = A.random_pairs(60)
    pairs = pairs + rp
    for layout, packed, guards in LAYOUTS:
        b = F.build(pairs, None, packed, guards=guards)
        rc, got, off, st = _chain2(ctx, b, 13, b.flags | A.KMER_STRAND_AUTO)
        assert rc == 0
        found = (st & np.uint32(A.ST_REVCOMP)) != 0
        assert found.any() and not found.all()
        b.qoff = b.qoff | np.where(found, np.uint64(F.QOFF_REVCOMP), np.uint64(0)).astype(np.uint64)
        rc2, got2, off2, st2 = _chain2(ctx, b, 13, b.flags | F.MODE_QSTRAND)
        assert rc2 == 0 and np.array_equal(off, off2) and np.array_equal(st & ~np.uint32(A.ST_REVCOMP), st2)
        assert all(np.array_equal(x, y) for x, y in zip(got, got2))


def test_argument_errors(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(2)
    T = rng.integers(0, 4, 2500).astype(np.uint8)
    pairs = [(S.mutate(rng, T, 0.08), T) for _ in range(4)]
    b = F.build(pairs, None, False)
    auto = A.KMER_STRAND_AUTO
    assert _chain2(ctx, b, 13, auto)[0] == 0
    assert _chain2(ctx, b, 13, auto | F.MODE_QSTRAND)[0] == -2
    assert _chain2(ctx, b, 13, auto, status=False)[0] == -2
    assert _chain2(ctx, b, 13, auto | 4)[0] == -2
    par = B.KmerParams()
    par.ksz, par.threads = 13, 0
    out = np.zeros(len(pairs), dtype=B.RESULT_DTYPE)
    st = np.zeros(len(pairs), dtype=np.uint32)

    def edit(bb, flags, status=True):
        return B.lib().bsa_kmer_edit_batch2(ctx.h, B._p(bb.seqs), bb.seqs.nbytes, B._p(bb.qoff), B._p(bb.qlen), B._p(bb.toff), B._p(bb.tlen), len(bb.qlen), C.byref(par),
                                            B._p(out), None, 0, None, B._p(st) if status else None, flags)
    for dev in (0, B.KMER_CHAIN_DEVICE):
        assert edit(b, auto | dev) == 0
        assert edit(b, auto | dev | F.MODE_QSTRAND) == -2
        assert edit(b, auto | dev, status=False) == -2
        assert edit(b, auto | dev | 4) == -2
    # bit 63 stays part of the offset: outside the blob
    bq = F.build(pairs, [True] * 4, False)
    assert _chain2(ctx, bq, 13, auto)[0] == -2 and edit(bq, auto) == -2 and edit(bq, auto | B.KMER_CHAIN_DEVICE) == -2
    # no pairs at all
    e = F.Batch()
    e.seqs, e.qoff, e.toff = np.zeros(8, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    e.qlen, e.tlen = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    assert _chain2(ctx, e, 13, auto)[0] == 0 and edit(e, auto) == 0
    # arena too small: maps_off[n] counts the chosen strand's anchors
    sp = [(F.revcomp(q) if k % 2 else q, t) for k, (q, t) in enumerate(pairs)]
    need = int(A.expected(sp, 13)[0][-1])
    bs = F.build(sp, None, True)
    rc, _, off, _ = _chain2(ctx, bs, 13, bs.flags | auto, cap=need - 1)
    assert rc == KC.E_CIGAR_CAP and int(off[4]) == need
    assert need > sum(len(f) for f in A.both_strands(sp, 13)[0]) + 1000          # not the forward lists: two of the four pairs are stored reverse
    assert _chain2(ctx, bs, 13, bs.flags | auto, cap=need)[0] == 0


def test_unflagged_calls_are_unchanged(ctx):
    names, pairs, strands = F.named_pairs(13)
    wrc, maps, woff, wst = KC.host_arena(pairs, 13)
    for st_arg in (None, strands):
        b = F.build(pairs, st_arg, False)
        rc, got, off, st = _chain2(ctx, b, 13, b.flags)
        assert rc == 0 and np.array_equal(off, woff) and np.array_equal(st, wst) and np.array_equal(np.concatenate(got), maps)


def test_python_keywords(ctx):
    import bsalign_amd as B
    pairs, flip = A.random_pairs(40)
    off, per, wst, wstrands = A.expected(pairs, 13)
    for seq2bit in (False, True):
        got, st, found = ctx.kmer_chain_batch(pairs, ksz=13, with_status=True, seq2bit=seq2bit, auto_strand=True)
        assert found.dtype == bool and np.array_equal(found, wstrands) and np.array_equal(st, wst)
        assert all(np.array_equal(x, y) for x, y in zip(got, per))
        got2, found2 = ctx.kmer_chain_batch(pairs, ksz=13, seq2bit=seq2bit, auto_strand=True)
        assert np.array_equal(found2, wstrands) and all(np.array_equal(x, y) for x, y in zip(got2, per))
        o0, c0, s0 = ctx.kmer_edit_batch(A.on_strand(pairs, wstrands), ksz=13)
        for dev in (False, True):
            o, c, s = ctx.kmer_edit_batch(pairs, ksz=13, device_chain=dev, seq2bit=seq2bit, auto_strand=True)
            assert np.array_equal((s & B.ST_REVCOMP) != 0, wstrands) and np.array_equal(s & ~np.uint32(B.ST_REVCOMP), s0)
            assert np.array_equal(o, o0) and all(np.array_equal(x, y) for x, y in zip(c, c0))
