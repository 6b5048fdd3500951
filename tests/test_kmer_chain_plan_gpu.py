"""GPU: the resident form of the k-mer chain call, bsa_kmer_chain_plan_create / bsa_kmer_chain_run (include/bsalign_hip.h), word for word against the host
chainer (per-pair bsa_kmer_chain through kmer_chain_cases.host_arena, on q or on a host-made revcomp(q)) and against the host-pointer call
(Context.kmer_chain_batch) with the same flags.  Every run gets output buffers filled with 0xA5 bytes and an arena allocated larger than it needs, so that
an element a run leaves unwritten, or a word it writes where it must not, shows.  Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import kmer_auto_cases as A
import kmer_chain_cases as KC
import kmer_flags_cases as F
import support as S

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5A5A5A5A5
GUARD = 64                        # words allocated behind what a complete run needs
E_ARG, E_UNSUPPORTED = -2, -6
_OPEN_PLANS = []


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()
    while _OPEN_PLANS:                                         # a plan goes before its context, also after a failed test
        _OPEN_PLANS.pop().close()


@pytest.fixture(scope="module")
def ctx():
    import bsalign_amd as B
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tight_ctx():
    """a workspace that holds three 3000-base pairs (about 96 KB of slices each)"""
    import bsalign_amd as B
    c = B.Context(0, workspace_limit=300000)
    yield c
    c.close()


def _filled(nbytes):
    import torch
    return torch.full((max((nbytes + 7) // 8 * 8, 8),), 0xA5, dtype=torch.uint8, device="cuda")


def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _plan(ctx, qoff, qlen, toff, tlen, ksz, flags=0):
    import bsalign_amd as B
    p = B.KmerChainPlan(ctx, qoff, qlen, toff, tlen, ksz=ksz, flags=flags)
    _OPEN_PLANS.append(p)
    return p


def _run(ctx, plan, d_seqs, alloc, cap, status=True, null_maps=False, want_rc=0):
    """one run with every output prefilled with 0xA5 bytes and an arena of `cap` words at the front of an allocation of `alloc`:
    -> (maps_off, status or None, the whole allocation as uint64)"""
    import torch
    import bsalign_amd as B
    n = plan.n
    assert 0 <= cap <= alloc and not (null_maps and cap)
    d_maps, d_off, d_st = _filled(alloc * 8), _filled((n + 1) * 8), _filled(n * 4)
    torch.cuda.synchronize()
    rc = B.lib().bsa_kmer_chain_run(plan.h, C.c_void_p(d_seqs.data_ptr()), None if null_maps else C.c_void_p(d_maps.data_ptr()), cap,
                                    C.c_void_p(d_off.data_ptr()), C.c_void_p(d_st.data_ptr()) if status else None)
    assert rc == want_rc, (rc, ctx_error(ctx))
    ctx.sync()
    torch.cuda.synchronize()
    off = d_off.cpu().numpy()[:(n + 1) * 8].view(np.uint64)
    st = d_st.cpu().numpy()[:n * 4].view(np.uint32)
    words = d_maps.cpu().numpy()[:alloc * 8].view(np.uint64)
    if not status:
        assert np.all(d_st.cpu().numpy() == 0xA5)
    return off, (st if status else None), words


def ctx_error(ctx):
    import bsalign_amd as B
    return (B.lib().bsa_last_error(ctx.h) or b"").decode()


def _check(got, per, woff, wst, cap, what=""):
    """the arena contract: offsets and status exact, pair k's words there iff off[k + 1] <= cap, every other word of the allocation untouched"""
    off, st, words = got
    assert np.array_equal(off, woff), (what, "maps_off", off[:8], woff[:8])
    if st is not None:
        bad = np.flatnonzero(st != wst)
        assert bad.size == 0, (what, "status of pair %d is %#x, expected %#x" % (bad[0], st[bad[0]], wst[bad[0]]))
    untouched = np.ones(len(words), dtype=bool)
    present = 0
    for k in range(len(per)):
        a, b = int(woff[k]), int(woff[k + 1])
        assert b - a == len(per[k])
        if b <= cap:
            assert np.array_equal(words[a:b], per[k]), (what, "anchors of pair", k, b - a)
            untouched[a:b] = False
            present += 1
    assert np.all(words[untouched] == SENT), (what, "a word outside the pairs that fit was written", int(np.flatnonzero(untouched & (words != SENT))[0]), cap)
    return present


def _split(maps, off):
    return [maps[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


_REF = {}


def _host(key, pairs, ksz):
    """per-pair bsa_kmer_chain on the host, once per key -> (per-pair anchors, maps_off, status)"""
    if key not in _REF:
        rc, maps, off, st = KC.host_arena(pairs, ksz)
        assert rc == 0
        _REF[key] = (_split(maps, off), off, st)
    return _REF[key]


def _full_run(ctx, plan, d_seqs, want, what="", status=True):
    per, woff, wst = want
    need = int(woff[-1])
    got = _run(ctx, plan, d_seqs, need + GUARD, need + GUARD, status=status)
    assert _check(got, per, woff, wst, need + GUARD, what) == len(per)
    return got


# ---- 1. words, offsets, status ----------------------------------------------------------------------------------------------------------
def _mixed_pairs(ksz):
    """the named cases of at most 4000 bases and 40 random pairs: lengths 0, below the k-mer, the k-mer, 20 .. 4000; 0 / 5 / 15 / 40 % divergence;
    every fifth with an inserted block; a base code above 3, an empty query, an empty target"""
    k = min(ksz, 15)
    names, pairs = [], []
    for name, q, t in KC.cases(ksz, with_long=False):
        if len(q) <= 4000 and len(t) <= 4000:
            names.append(name)
            pairs.append((q, t))
    rng = np.random.default_rng(500 + ksz)
    lens = [0, k - 1, k, 20, 21, 4000] + [int(x) for x in rng.integers(20, 4000, 31)]
    for it, L in enumerate(lens):
        T = rng.integers(0, 4, L).astype(np.uint8)
        Q = S.mutate(rng, T, float((0.0, 0.05, 0.15, 0.40)[it % 4])) if L else T.copy()
        if it % 5 == 2 and len(Q) > 400:
            a = int(rng.integers(50, len(Q) - 100))
            Q = np.concatenate([Q[:a], rng.integers(0, 4, int(rng.integers(30, 600))).astype(np.uint8), Q[a:]])[:4000]
        names.append("random%d_L%d" % (it, L))
        pairs.append((Q, T))
    T = rng.integers(0, 4, 1500).astype(np.uint8)
    bad = S.mutate(rng, T, 0.03)
    bad[len(bad) // 2] = 4
    names += ["bad_base", "no_query", "no_target"]
    pairs += [(bad, T), (np.zeros(0, np.uint8), T), (T, np.zeros(0, np.uint8))]
    return names, pairs


@pytest.mark.parametrize("ksz", [8, 13, 15, 20])
def test_words_offsets_and_status_equal_the_host_chainer(ctx, ksz):
    import torch
    import bsalign_amd as B
    names, pairs = _mixed_pairs(ksz)
    assert max(max(len(q), len(t)) for q, t in pairs) <= 4000
    want = _host(("mixed", ksz), pairs, ksz)
    per, woff, wst = want
    by = dict(zip(names, range(len(names))))
    assert len(per[by["identical"]]) > 1800 and len(per[by["crossing"]]) > 0 and sum(1 for p in per if len(p)) >= 20
    assert wst[by["bad_base"]] == KC.ST_BAD_BASE and wst[by["no_query"]] == KC.ST_EMPTY and wst[by["no_target"]] == KC.ST_EMPTY
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    assert B.kmer_chain_words_bound(qlen, tlen) >= int(woff[-1])
    d_seqs = _upload(seqs)
    plan = _plan(ctx, qoff, qlen, toff, tlen, ksz)
    assert plan.chunks() == 1
    _full_run(ctx, plan, d_seqs, want, "ksz %d" % ksz)
    _full_run(ctx, plan, d_seqs, want, "ksz %d, no status" % ksz, status=False)
    # the Python form: torch tensors, the arena's size is the capacity (bsa_kmer_chain_words_bound always suffices)
    n = len(pairs)
    d_maps = _filled(B.kmer_chain_words_bound(qlen, tlen) * 8).view(torch.int64)
    d_off, d_st = _filled((n + 1) * 8).view(torch.int64), _filled(n * 4).view(torch.int32)[:n]
    torch.cuda.synchronize()
    plan.run(d_seqs, d_maps, d_off, d_st)
    ctx.sync()
    off = d_off.cpu().numpy().view(np.uint64)[:n + 1]
    assert np.array_equal(off, woff) and np.array_equal(d_st.cpu().numpy().view(np.uint32), wst)
    assert np.array_equal(d_maps.cpu().numpy().view(np.uint64)[:int(woff[-1])], np.concatenate(per))
    # the host-pointer call says the same
    got, gst = ctx.kmer_chain_batch(pairs, ksz=ksz, with_status=True)
    assert np.array_equal(gst, wst) and all(np.array_equal(x, y) for x, y in zip(got, per))
    plan.close()


def test_kmer_size_zero_gives_status_and_no_anchors(ctx):
    import bsalign_amd as B
    names, pairs = _mixed_pairs(13)
    pairs = pairs[-8:]
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    plan = _plan(ctx, qoff, qlen, toff, tlen, 0)
    off, st, words = _run(ctx, plan, _upload(seqs), GUARD, GUARD)
    assert np.all(off == 0) and np.all(words == SENT)
    assert np.array_equal(st, np.array([KC.host_status(q, t) for q, t in pairs], dtype=np.uint32)) and st.any()
    plan.close()


# ---- 2. chunks ----------------------------------------------------------------------------------------------------------------------------
def _ten_pairs():
    rng = np.random.default_rng(3)
    t2 = rng.integers(0, 4, 20000).astype(np.uint8)
    return [(S.mutate(rng, t2[300 * k:300 * k + 3000], 0.05), t2[300 * k:300 * k + 3000].copy()) for k in range(10)], t2


def test_chunks_carry_the_offsets_and_pairs_the_device_cannot_take_are_refused(ctx, tight_ctx):
    import bsalign_amd as B
    pairs, t2 = _ten_pairs()
    pairs[4] = (np.zeros(0, np.uint8), pairs[4][1])           # a status word in the middle of a later chunk
    want = _host("ten", pairs, 13)
    assert int(want[1][-1]) > 10000 and want[2][4] == KC.ST_EMPTY
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    d_seqs = _upload(seqs)
    plan = _plan(tight_ctx, qoff, qlen, toff, tlen, 13)
    assert plan.chunks() >= 3
    _full_run(tight_ctx, plan, d_seqs, want, "chunks")
    ms, dev, host = tight_ctx.last_kmer_chain_ms()
    assert ms > 0 and (dev, host) == (10, 0)
    # the same pairs in one chunk on the context without a limit
    one = _plan(ctx, qoff, qlen, toff, tlen, 13)
    assert one.chunks() == 1
    _full_run(ctx, one, d_seqs, want, "one chunk")
    # BSA_KMER_STRAND_AUTO slices are larger: more chunks, the same carry
    sp = [(F.revcomp(q) if k % 3 == 1 else q, t) for k, (q, t) in enumerate(pairs)]
    woff, per, wst, wstrands = A.expected(sp, 13)
    bs = B.pack_pairs(sp)
    auto = _plan(tight_ctx, *bs[1:], 13, A.KMER_STRAND_AUTO)
    assert auto.chunks() >= plan.chunks() and wstrands[1] and not wstrands[0]
    need = int(woff[-1])
    got = _run(tight_ctx, auto, _upload(bs[0]), need + GUARD, need)
    _check(got, per, woff, wst | np.where(wstrands, np.uint32(A.ST_REVCOMP), np.uint32(0)).astype(np.uint32), need, "auto chunks")
    # no host route behind a run: a pair whose slice alone exceeds the workspace limit is refused, and named
    big = pairs[:2] + [(t2.copy(), t2)]
    bq = B.pack_pairs(big)
    with pytest.raises(B.BsaError) as e:
        B.KmerChainPlan(tight_ctx, *bq[1:], ksz=13)
    assert e.value.code == E_UNSUPPORTED and "pair 2" in str(e.value)
    _plan(ctx, *bq[1:], 13).close()                           # (without the limit the same plan is fine)
    # ... and so is a pair above the device route's length; metadata only, no sequence exists
    half = KC.DEV_MAX // 2 + 40
    qo, to = np.array([0, 100], np.uint64), np.array([50, 100 + half], np.uint64)
    ql, tl = np.array([50, half], np.uint32), np.array([50, half], np.uint32)
    with pytest.raises(B.BsaError) as e:
        B.KmerChainPlan(ctx, qo, ql, to, tl, ksz=13)
    assert e.value.code == E_UNSUPPORTED and "pair 1" in str(e.value)
    _plan(ctx, qo, ql - np.uint32(40), to, tl - np.uint32(40), 13).close()          # qlen + tlen == DEV_MAX is taken


# ---- 3. the arena contract -------------------------------------------------------------------------------------------------------------
def _five_pairs():
    rng = np.random.default_rng(12)
    T = rng.integers(0, 4, 2000).astype(np.uint8)
    bad = T.copy()
    bad[5] = 4
    return [(S.mutate(rng, T, 0.05), T), (np.zeros(0, np.uint8), T), (bad, T), (T, np.zeros(0, np.uint8)), (S.mutate(rng, T, 0.1), T)]


def test_arena_contract_for_any_capacity(ctx):
    import bsalign_amd as B
    pairs = _five_pairs()
    per, woff, wst = _host("five", pairs, 13)
    need = int(woff[-1])
    assert list(wst) == [0, KC.ST_EMPTY, KC.ST_BAD_BASE, KC.ST_EMPTY, 0] and 0 < int(woff[2]) < need and int(woff[1]) == int(woff[4])
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    d_seqs = _upload(seqs)
    plan = _plan(ctx, qoff, qlen, toff, tlen, 13)
    o2 = int(woff[2])
    for cap, null_maps, fitting in ((need, False, 5), (need - 1, False, 4), (o2, False, 4), (o2 + 1, False, 4), (0, False, 0), (0, True, 0),
                                    (o2 - 1, False, 0), (need + GUARD, False, 5)):
        got = _run(ctx, plan, d_seqs, need + GUARD, cap, null_maps=null_maps)
        assert _check(got, per, woff, wst, cap, "cap %d%s" % (cap, " (NULL arena)" if null_maps else "")) == fitting
    plan.close()


# ---- 4. re-runs -----------------------------------------------------------------------------------------------------------------------------
def _substituted(rng, T, rate):
    Q = T.copy()
    m = rng.random(len(T)) < rate
    Q[m] = (Q[m] + rng.integers(1, 4, int(m.sum()))) & 3
    return Q


def test_a_run_leaves_nothing_behind(ctx):
    import torch
    import bsalign_amd as B
    rng = np.random.default_rng(41)
    lens = [2500, 0, 900, 12, 3100, 1700]
    blobs = []
    for rate in (0.04, 0.12):                                  # two sets of sequences with the same lengths
        pairs = []
        for L in lens:
            T = rng.integers(0, 4, L).astype(np.uint8)
            pairs.append((_substituted(rng, T, rate), T))
        blobs.append(pairs)
    wa, wb = _host("rerun_a", blobs[0], 13), _host("rerun_b", blobs[1], 13)
    assert int(wa[1][-1]) != int(wb[1][-1]) and int(wb[1][-1]) > 0
    sa, qoff, qlen, toff, tlen = B.pack_pairs(blobs[0])
    sb = B.pack_pairs(blobs[1])[0]
    da, db = _upload(sa), _upload(sb)
    plan = _plan(ctx, qoff, qlen, toff, tlen, 13)
    _full_run(ctx, plan, da, wa, "first blob")
    _full_run(ctx, plan, db, wb, "second blob, same lengths")
    # a short run, then a full one
    need = int(wa[1][-1])
    got = _run(ctx, plan, da, need + GUARD, int(wa[1][1]) + 3)
    assert _check(got, *wa, int(wa[1][1]) + 3, "short run") < len(lens)
    _full_run(ctx, plan, da, wa, "after a short run")
    # two chain plans of one context in turn (another k-mer size, other pairs, the strand flag)
    five = _five_pairs()
    wf = _host("five8", five, 8)
    s5 = B.pack_pairs(five)
    other = _plan(ctx, *s5[1:], 8)
    d5 = _upload(s5[0])
    for it in range(2):
        _full_run(ctx, other, d5, wf, "other plan, turn %d" % it)
        _full_run(ctx, plan, db, wb, "first plan, turn %d" % it)
    # a chain run, an align run, the chain run again
    ap = [(q, t) for q, t in blobs[0] if 0 < len(q) <= 1000]
    s_al = B.pack_pairs(ap)
    align = B.AlignPlan(ctx, *s_al[1:], B.make_params(B.MODE_GLOBAL, 128))
    _OPEN_PLANS.append(align)
    na = len(ap)
    d_al, d_out, d_cig = _upload(s_al[0]), _filled(na * 40), _filled(4 * (int(s_al[2].sum() + s_al[4].sum()) + 2 * na + 16))
    d_coff, d_ast = _filled((na + 1) * 8), _filled(na * 4)
    _full_run(ctx, plan, da, wa, "before the align run")
    torch.cuda.synchronize()
    align.run(d_al, d_out, d_cig.view(torch.int32), d_coff, d_ast)
    _full_run(ctx, plan, da, wa, "after the align run")
    ctx.sync()
    assert np.all(d_ast.cpu().numpy()[:na * 4].view(np.uint32) == 0) and int(d_coff.cpu().numpy()[:(na + 1) * 8].view(np.uint64)[na]) > 0
    align.close()
    # no pairs at all: the one offset is written
    z64, z32 = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    empty = _plan(ctx, z64, z32, z64, z32, 13)
    assert empty.chunks() == 0
    off, st, words = _run(ctx, empty, da, GUARD, GUARD)
    assert list(off) == [0] and np.all(words == SENT)
    assert ctx.last_kmer_chain_ms() == (0.0, 0, 0)
    for p in (plan, other, empty):
        p.close()


# ---- 5. flags -----------------------------------------------------------------------------------------------------------------------------
def _flag_pairs(seed=9):
    rng = np.random.default_rng(seed)
    pairs = []
    for L, div in ((1800, 0.05), (33, 0.0), (2600, 0.15), (0, 0.0), (700, 0.40), (1250, 0.0), (14, 0.0), (3999, 0.05)):
        T = rng.integers(0, 4, L).astype(np.uint8)
        pairs.append((S.mutate(rng, T, div) if div else T.copy(), T))
    return pairs


def test_seq2bit_reads_the_callers_words_in_place(ctx):
    import torch
    import bsalign_amd as B
    pairs = _flag_pairs()
    want = _host("flags", pairs, 13)
    words, qoff, qlen, toff, tlen = B.pack_pairs(pairs, seq2bit=True)          # lead 3: reads at odd base offsets
    assert int(qoff[0]) == 3 and len({int(x) % 32 for x in np.concatenate([qoff, toff])}) > 4
    whole = torch.cat([torch.full((8,), 0xFF, dtype=torch.uint8, device="cuda"), _upload(words), torch.full((8,), 0xFF, dtype=torch.uint8, device="cuda")])
    d_seqs = whole[8:]                                        # a view that starts 8 bytes into a larger tensor
    assert d_seqs.data_ptr() == whole.data_ptr() + 8 and d_seqs.data_ptr() % 8 == 0
    plan = _plan(ctx, qoff, qlen, toff, tlen, 13, B.MODE_SEQ2BIT)
    _full_run(ctx, plan, d_seqs, want, "seq2bit")
    got, gst = ctx.kmer_chain_batch(pairs, ksz=13, with_status=True, seq2bit=True)
    assert np.array_equal(gst, want[2]) and all(np.array_equal(x, y) for x, y in zip(got, want[0]))
    # a blob of 64-bit words that starts in the middle of one is refused
    _run(ctx, plan, whole[12:], GUARD, GUARD, want_rc=E_ARG)
    plan.close()


def test_qstrand_marks_a_read_that_is_stored_once(ctx):
    import bsalign_amd as B
    rng = np.random.default_rng(21)
    r = rng.integers(0, 4, 2000).astype(np.uint8)
    # logical pairs: r against a forward overlap, revcomp(r) against a target on the other strand -- build() stores the marked query as r, once
    logical = [(r, S.mutate(rng, r, 0.04)), (F.revcomp(r), S.mutate(rng, F.revcomp(r), 0.04))]
    strands = [False, True]
    more, ms = F.random_pairs(20, seed=5)
    logical, strands = logical + more, strands + ms
    want = _host("qstrand", logical, 13)
    assert len(want[0][1]) > 1000 and sum(1 for p, s in zip(want[0], strands) if s and len(p)) >= 4
    for packed in (False, True):
        b = F.build(logical, strands, packed, guards=packed)
        assert b.shared == 1 and int(b.qoff[1]) == int(b.qoff[0]) | F.QOFF_REVCOMP
        plan = _plan(ctx, b.qoff, b.qlen, b.toff, b.tlen, 13, b.flags)
        _full_run(ctx, plan, _upload(b.seqs), want, "qstrand, packed %d" % packed)
        plan.close()
    got, gst = ctx.kmer_chain_batch([(sq, t) for sq, (_, t) in zip(F.build(logical, strands).stored, logical)], ksz=13, with_status=True, strands=strands)
    assert np.array_equal(gst, want[2]) and all(np.array_equal(x, y) for x, y in zip(got, want[0]))


@pytest.mark.parametrize("packed", [False, True])
def test_strand_auto_finds_the_strands(ctx, packed):
    import bsalign_amd as B
    stored = [(q, t) for _, q, t in A.extra_cases()]                            # a 0-against-0 tie (empty_both), a tie with anchors, both strands chaining
    fp = _flag_pairs(10)
    stored += [(F.revcomp(q) if k % 2 else q, t) for k, (q, t) in enumerate(fp)]
    if not packed:
        bad = fp[0][0].copy()
        bad[7] = 9
        stored.append((F.revcomp(bad), fp[0][1]))                             # a base code above 3: forward only
    key = ("auto", packed)
    if key not in _REF:
        _REF[key] = A.expected(stored, 13)
    woff, per, wst, wstrands = _REF[key]
    assert wstrands.any() and not wstrands.all() and any(len(p) == 0 and not s for p, s in zip(per, wstrands))
    full = wst | np.where(wstrands, np.uint32(A.ST_REVCOMP), np.uint32(0)).astype(np.uint32)
    b = F.build(stored, None, packed, guards=packed)
    flags = b.flags | A.KMER_STRAND_AUTO
    plan = _plan(ctx, b.qoff, b.qlen, b.toff, b.tlen, 13, flags)
    d_seqs = _upload(b.seqs)
    _full_run(ctx, plan, d_seqs, (per, woff, full), "auto, packed %d" % packed)
    got, gst, found = ctx.kmer_chain_batch(stored, ksz=13, with_status=True, seq2bit=packed, auto_strand=True)
    assert np.array_equal(found, wstrands) and np.array_equal(gst, wst) and all(np.array_equal(x, y) for x, y in zip(got, per))
    # the strands are reported in d_status: without it the run is refused
    _run(ctx, plan, d_seqs, GUARD, GUARD, status=False, want_rc=E_ARG)
    plan.close()


def test_flag_errors_at_create(ctx):
    import bsalign_amd as B
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(_flag_pairs()[:2])
    for flags in (B.MODE_QSTRAND | B.KMER_STRAND_AUTO, 0x400, B.MODE_SEQ2BIT | 1, 0x80000000):
        with pytest.raises(B.BsaError) as e:
            B.KmerChainPlan(ctx, qoff, qlen, toff, tlen, ksz=13, flags=flags)
        assert e.value.code == E_ARG, hex(flags)
    h = C.c_void_p()
    assert B.lib().bsa_kmer_chain_plan_create(ctx.h, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), 2, 13, 0, None) == E_ARG
    assert B.lib().bsa_kmer_chain_plan_create(ctx.h, None, B._p(qlen), B._p(toff), B._p(tlen), 2, 13, 0, C.byref(h)) == E_ARG and not h.value
    plan = _plan(ctx, qoff, qlen, toff, tlen, 13)
    d_seqs = _upload(seqs)
    off = _filled(3 * 8)
    run = B.lib().bsa_kmer_chain_run
    assert run(plan.h, C.c_void_p(d_seqs.data_ptr()), None, 0, None, None) == E_ARG                              # no d_maps_off
    assert run(plan.h, C.c_void_p(d_seqs.data_ptr()), None, 5, C.c_void_p(off.data_ptr()), None) == E_ARG        # a capacity and no arena
    assert run(plan.h, None, None, 0, C.c_void_p(off.data_ptr()), None) == E_ARG                                 # no blob
    plan.close()


# ---- 6. timing ----------------------------------------------------------------------------------------------------------------------------
def test_timing_accessor_reports_the_run(ctx):
    import bsalign_amd as B
    pairs = _five_pairs()
    want = _host("five", pairs, 13)
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    ctx.kmer_chain_batch(pairs[:2], ksz=13)                    # what an earlier host-pointer call recorded is replaced
    plan = _plan(ctx, qoff, qlen, toff, tlen, 13)
    _full_run(ctx, plan, _upload(seqs), want, "timing")
    ctx.sync()
    ms, dev, host = ctx.last_kmer_chain_ms()
    assert ms > 0 and (dev, host) == (len(pairs), 0)
    assert ctx.last_kmer_chain_ms() == (ms, dev, host)         # asking twice gives the same answer
    ctx.kmer_chain_batch(pairs[:2], ksz=13)
    assert ctx.last_kmer_chain_ms()[1:] == (2, 0)
    plan.close()
