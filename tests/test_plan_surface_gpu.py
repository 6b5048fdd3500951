"""GPU: the CIGAR arena and re-run contract of the device-pointer calls bsa_align_run / bsa_edit_run (include/bsalign_hip.h, at bsa_align_run),
and what the host-pointer calls report when their arena is too small.

The device-pointer calls are asynchronous and cannot report a short arena: the guards of the gather kernels (k_cigar_collect, k_cigar_final,
k_cigar_final_direct in bsa_api.hip) are all that keeps a wrong cigar_cap_words from a write behind the caller's buffer.  Every run here gets
output buffers filled with 0xA5 bytes and an arena with 64 guard words behind it, on every route the words can take (PC.check_arena states
what must hold).  Plans are re-run on other sequences of the same lengths and take turns on one context, so that state a run leaves in the
plan or the context (band states of the row-segment kernel, workspace slots, scan carries) would show.
Every test runs under a time limit of its own."""
import ctypes as C
import faulthandler
import re

import numpy as np
import pytest

import kmer_support as K
import plan_surface_cases as PC
import support as S
from test_kmer_cpu import oracle_segment

pytestmark = pytest.mark.gpu

SENT = PC.SENTINEL
GUARD = 64
ROWRECORDS = 0x100


_OPEN_PLANS = []


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)          # a hung kernel ends the process instead of the session
    yield
    faulthandler.cancel_dump_traceback_later()
    # a test that failed has not closed its plans, and its traceback keeps them alive beyond the module's contexts: a plan must not be
    # destroyed after its context, so they go here
    while _OPEN_PLANS:
        _OPEN_PLANS.pop().close()


@pytest.fixture(scope="module")
def ctx():
    import bsalign_amd as B
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tight_ctx():
    """a context whose workspace holds a fraction of the `small` corpus (about 5 MB of slots): with BSA_PIPELINE=1 its plans run in two
    halves on two streams"""
    import bsalign_amd as B
    c = B.Context(0, workspace_limit=2 << 20)
    yield c
    c.close()


def _filled(nbytes):
    import torch
    return torch.full((max(nbytes, 8),), 0xA5, dtype=torch.uint8, device="cuda")


def _make_plan(ctx, kind, corp, mode, bw, scoring):
    import bsalign_amd as B
    if kind == "align":
        plan = B.AlignPlan(ctx, corp.qoff, corp.qlen, corp.toff, corp.tlen, B.make_params(mode, bw, *scoring))
    else:
        plan = B.EditPlan(ctx, corp.qoff, corp.qlen, corp.toff, corp.tlen, mode, bw)
    _OPEN_PLANS.append(plan)
    return plan


def _run(ctx, plan, kind, d_seqs, alloc_words, cap):
    """one run with every output prefilled with 0xA5 bytes and an arena of `cap` words at the front of an allocation of alloc_words:
    -> (records (n, 10) int32, cigar_off uint64, status uint32, the whole allocation as uint32)"""
    import torch
    import bsalign_amd as B
    n = plan.n
    assert 0 <= cap <= alloc_words
    d_out, d_off, d_st, d_cig = _filled(n * 40), _filled((n + 1) * 8), _filled(n * 4), _filled(alloc_words * 4)
    torch.cuda.synchronize()
    fn = B.lib().bsa_align_run if kind == "align" else B.lib().bsa_edit_run
    ctx._chk(fn(plan.h, C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_cig.data_ptr()), cap,
                C.c_void_p(d_off.data_ptr()), C.c_void_p(d_st.data_ptr())))
    ctx.sync()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()[:n * 40].view(np.int32).reshape(n, 10)
    off = d_off.cpu().numpy()[:(n + 1) * 8].view(np.uint64)
    st = d_st.cpu().numpy()[:n * 4].view(np.uint32)
    words = d_cig.cpu().numpy()[:alloc_words * 4].view(np.uint32)
    return out, off, st, words


def _check(got, exp, cap, all_fitting_present, what):
    out, off, st, words = got
    rec, cigs, eoff, est = exp
    bad = np.flatnonzero(st != est)
    assert bad.size == 0, "%s: status of pair %d is %#x, expected %#x" % (what, bad[0], st[bad[0]], est[bad[0]])
    bad = np.flatnonzero((out != rec).any(axis=1))
    assert bad.size == 0, "%s: record of pair %d is %s, expected %s" % (what, bad[0], out[bad[0]], rec[bad[0]])
    assert np.array_equal(off, eoff), "%s: cigar_off differs from the large-arena run's (first at %d)" % (what, int(np.flatnonzero(off != eoff)[0]))
    return PC.check_arena(words, cap, SENT, off, cigs, all_fitting_present)


def _upload(corp):
    import torch
    return torch.from_numpy(corp.seqs).cuda()


# ---- a. every output element is written -----------------------------------------------------------------------------------------------
RUN_CONFIGS = {
    "align-bw128-affine": ("align", S.MODE_GLOBAL, 128, PC.SCORINGS["affine"], "k_align8_fwd_x"),
    "align-bw0-systolic": ("align", S.MODE_GLOBAL, 0, PC.SCORINGS["affine"], "k_align8_fwd_sys"),
    "edit-bw256-global": ("edit", S.MODE_GLOBAL, 256, None, "k_edit"),
    "edit-bw0-extend": ("edit", S.MODE_EXTEND, 0, None, "k_edit"),
}


@pytest.mark.parametrize("name", list(RUN_CONFIGS))
def test_every_output_element_is_written(ctx, name):
    """d_out, d_cigar_off, d_status and the arena start as 0xA5 bytes: after the run every record, every status word (the zero records and
    flags of the empty and the bad-base pairs included), all n + 1 offsets and all words equal the oracle's, and the arena behind
    cigar_off[n] is untouched"""
    kind, mode, bw, scoring, kernel = RUN_CONFIGS[name]
    corp = PC.small()
    exp = PC.expected(corp.pairs, kind, mode, bw, scoring, key="small")
    total = int(exp[2][-1])
    plan = _make_plan(ctx, kind, corp, mode, bw, scoring)
    got = _run(ctx, plan, kind, _upload(corp), total + 1000 + GUARD, total + 1000)
    assert kernel in ctx.last_kernel_names()[0], ctx.last_kernel_names()
    assert _check(got, exp, total + 1000, True, name) == len(corp.good())
    plan.close()


# ---- b. short arenas on every gather route ----------------------------------------------------------------------------------------------
# the environment variables that force each route (BSA_CHUNK_PAIRS and BSA_PIPELINE are read when the plan is created, BSA_CIGAR_VIA_ARENA at the run)
ROUTES = {
    "direct": {},                                                      # one chunk, one stream: k_cigar_final_direct
    "arena": {"BSA_CIGAR_VIA_ARENA": "1"},                             # one chunk through the staging arena: k_cigar_collect, k_cigar_final
    "chunks": {"BSA_CHUNK_PAIRS": "7"},                                # 14 chunks on one stream, the scan carry handed from chunk to chunk
    # plan_chunks at this size: everything fits the workspace and n < 4096, so two_halves stays false and nbuf 1 -- the 14 chunks share one
    # region and one stream.  The plan and its launches are those of "chunks": the route shows that the switch alone changes nothing here
    "pipeline": {"BSA_PIPELINE": "1", "BSA_CHUNK_PAIRS": "7"},
    # with tight_ctx: the batch needs more than the 2 MB the workspace may take, so plan_chunks cuts it into chunks of half the budget
    # (two_halves true, nbuf 2): forward passes on the context stream, walkers, scans and k_cigar_collect on the auxiliary one.  Nothing
    # exposes two_halves or nbuf; the test tells the case from the launch count, see there
    "two_streams": {"BSA_PIPELINE": "1"},
}
VARIANTS = {
    "base": {"align": ("align", S.MODE_GLOBAL, 128, PC.SCORINGS["affine"]), "edit": ("edit", S.MODE_GLOBAL, 256, None)},
    "twopiece": {"align": ("align", S.MODE_GLOBAL, 128, PC.SCORINGS["twopiece"])},             # 8-bit codes, another trace kernel
    "rowrecords": {"align": ("align", S.MODE_GLOBAL | ROWRECORDS, 128, PC.SCORINGS["affine"])},    # the literal k_align8_backcal
}
SHORT_CASES = [(kind, route, "base") for kind in ("align", "edit") for route in ROUTES] + \
              [("align", route, variant) for variant in ("twopiece", "rowrecords") for route in ("direct", "chunks")]


def _short_arena_rounds(ctx, plan, kind, d_seqs, exp, direct, what):
    total = int(exp[2][-1])
    with_words = sum(1 for c in exp[1] if len(c))
    assert total > 2 and with_words > 2
    for cap in (total, total - 1, total // 2, 1, 0, total):          # (the last: a short run leaves nothing behind in the plan)
        got = _run(ctx, plan, kind, d_seqs, total + GUARD, cap)
        present = _check(got, exp, cap, direct or cap >= total, "%s, capacity %d of %d" % (what, cap, total))
        if cap >= total:
            assert present == with_words
        else:
            assert present < with_words


@pytest.mark.parametrize("kind,route,variant", SHORT_CASES)
def test_short_arena_on_every_gather_route(ctx, tight_ctx, monkeypatch, kind, route, variant):
    """capacities total, total - 1, total / 2, 1 and 0 (a non-NULL pointer), then total again on the same plan: records, status and all of
    cigar_off are the large-arena run's whatever the capacity, no word at or above the capacity is touched, a pair's range holds its words or
    none -- on the direct route every pair that ends inside the arena is there, on the others which of them are is unspecified after an overflow"""
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    c = tight_ctx if route == "two_streams" else ctx
    _, mode, bw, scoring = VARIANTS[variant][kind]
    corp = PC.small()
    exp = PC.expected(corp.pairs, kind, mode & 3, bw, scoring, key="small")
    plan = _make_plan(c, kind, corp, mode, bw, scoring)
    d_seqs = _upload(corp)
    _short_arena_rounds(c, plan, kind, d_seqs, exp, route == "direct", "%s %s %s" % (kind, route, variant))
    launches = c.last_kernel_ms()[1]                  # forward launches of the last run, one event pair a chunk
    if route in ("direct", "arena"):
        assert launches == 1
    elif route in ("chunks", "pipeline"):
        assert launches == (len(corp) + 6) // 7
    fwd, trace = c.last_kernel_names()
    if route == "two_streams":
        # the same context without BSA_PIPELINE cuts the batch into chunks of the whole budget.  Had plan_chunks not reached two_halves (a pair
        # above half the budget), the pipelined plan would be cut by the whole budget too and be that plan, launch for launch: more launches
        # than it means chunks of half the budget, which is the two_halves case
        monkeypatch.delenv("BSA_PIPELINE")
        one_stream = _make_plan(c, kind, corp, mode, bw, scoring)
        total = int(exp[2][-1])
        _check(_run(c, one_stream, kind, d_seqs, total + GUARD, total), exp, total, True, "%s on one stream" % kind)
        assert 1 < c.last_kernel_ms()[1] < launches, (c.last_kernel_ms()[1], launches)
        one_stream.close()
    if variant == "twopiece":
        assert "two-piece" in fwd and "8-bit traceback codes" in fwd, fwd
    if variant == "rowrecords":
        assert "k_align8_backcal" in trace, trace
    plan.close()


@pytest.mark.parametrize("route", ["direct", "arena"])
def test_short_arena_with_the_tiled_scans(ctx, monkeypatch, route):
    """16 400 pairs, just above the 16 384 counts at which the exclusive scans run in tiles over many blocks (k_scan_tile_*): the scan into
    d_cigar_off on both routes, the scan by position with its carry on the arena route.  300 pairs against the oracle, the rest against the
    large-arena run.  Measured on an MI355X: 0.11 s for the direct route, which also builds the corpus, and 0.03 s for the arena route (the pairs
    are 20 to 40 bases, so the kernels are short; the time is the host building and checking 16 400 pairs)."""
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    corp = PC.short_many()
    n = len(corp)
    sc = PC.SCORINGS["affine"]
    plan = _make_plan(ctx, "align", corp, S.MODE_GLOBAL, 0, sc)
    d_seqs = _upload(corp)
    big = int(corp.qlen.sum() + corp.tlen.sum()) + 2 * n
    out, off, st, words = _run(ctx, plan, "align", d_seqs, big + GUARD, big)
    assert not st.any() and off[0] == 0 and (np.diff(off.astype(np.int64)) > 0).all() and int(off[n]) <= big
    for k in np.random.default_rng(3).choice(n, size=300, replace=False):
        res, cig, m = S.oracle_align(*corp.pairs[k], S.MODE_GLOBAL, 0, *sc)
        assert np.array_equal(out[k], res) and np.array_equal(words[int(off[k]):int(off[k + 1])], cig), k
    assert (words[int(off[n]):] == SENT).all()
    exp = (out, [words[int(off[k]):int(off[k + 1])] for k in range(n)], off, st)
    _short_arena_rounds(ctx, plan, "align", d_seqs, exp, route == "direct", "short_many %s" % route)
    plan.close()


# ---- c. the host-pointer calls report the words needed -----------------------------------------------------------------------------------
def _host_call(fn, ctx, corp, par, cap, flags=None):
    """a host-pointer batch call with cigar_off prefilled with 7s and GUARD sentinel words behind an arena of `cap` words"""
    import bsalign_amd as B
    B.lib()                                      # (the library takes a fresh snapshot of the BSA_* variables when a test has changed one)
    n = len(corp)
    out = np.full((n, 10), -1, dtype=np.int32)
    st = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    coff = np.full(n + 1, 7, dtype=np.uint64)
    cig = np.full(cap + GUARD, SENT, dtype=np.uint32)
    args = [ctx.h, corp.seqs.ctypes.data, corp.seqs.size, corp.qoff.ctypes.data, corp.qlen.ctypes.data, corp.toff.ctypes.data, corp.tlen.ctypes.data, n,
            C.byref(par), out.ctypes.data, cig.ctypes.data, cap, coff.ctypes.data, st.ctypes.data]
    rc = fn(*args) if flags is None else fn(*args, flags)
    return rc, out, cig, coff, st


def _kmer_expected(corp):
    rec, cigs = [], []
    for q, t in corp.pairs:
        r, c, _ = K.kmer_host(13, q, t, oracle_segment)
        rec.append(r)
        cigs.append(c.astype(np.uint32))
    off = np.zeros(len(cigs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cigs])
    return np.array(rec, dtype=np.int32), cigs, off, np.zeros(len(cigs), dtype=np.uint32)


HOST_CALLS = ["align-one-plan", "align-two-slices", "align-width-classes", "edit", "kmer-edit", "kmer-edit-device-chain"]


@pytest.mark.parametrize("call", HOST_CALLS)
def test_host_calls_report_the_words_needed(ctx, monkeypatch, capfd, call):
    """BSA_E_CIGAR_CAP from a host-pointer call: cigar_off[n] is the number of words the batch needs, whatever the caller's array held, nothing
    is written behind the arena, and the call repeated with that capacity gives the oracle's results"""
    import bsalign_amd as B
    L = B.lib()
    flags, align = None, call.startswith("align")
    if align:
        corp = PC.mixed_whole_query() if call == "align-width-classes" else PC.small()
        bw = 0 if call == "align-width-classes" else 128
        par = B.make_params(S.MODE_GLOBAL, bw, *PC.SCORINGS["affine"])
        exp = PC.expected(corp.pairs, "align", S.MODE_GLOBAL, bw, PC.SCORINGS["affine"], key="mixed" if bw == 0 else "small")
        fn = L.bsa_align_batch
        if call != "align-width-classes":
            monkeypatch.setenv("BSA_BATCH_SLICES", "2" if call == "align-two-slices" else "1")      # (the variable that chooses between the two paths)
        if call != "align-one-plan":
            monkeypatch.setenv("BSA_API_TIMING", "1")          # the sliced path and every sub-batch of a width class say on stderr that they ran
    elif call == "edit":
        corp = PC.small()
        par = B.EditParams()
        par.mode, par.bandwidth = S.MODE_GLOBAL, 256
        exp = PC.expected(corp.pairs, "edit", S.MODE_GLOBAL, 256, None, key="small")
        fn = L.bsa_edit_batch
    else:
        small = PC.small()
        corp = PC.Corpus([small.pairs[k] for k in small.good()[:32]])
        par = B.KmerParams()
        par.ksz, par.threads = 13, 4
        exp = _kmer_expected(corp)
        fn, flags = (L.bsa_kmer_edit_batch2, B.KMER_CHAIN_DEVICE) if call == "kmer-edit-device-chain" else (L.bsa_kmer_edit_batch, None)
    rec, cigs, eoff, est = exp
    n, total = len(corp), int(eoff[-1])
    caps = [total - 1]
    if call == "align-two-slices":
        # the cut of align_batch_sliced: the first pairs that hold half of the bases
        tot, acc, h = int(corp.qlen.sum() + corp.tlen.sum()), 0, 0
        while h < n and acc < tot // 2:
            acc += int(corp.qlen[h]) + int(corp.tlen[h])
            h += 1
        tot_a = int(eoff[h])
        assert 0 < h < n and 1 < tot_a < total - 1
        caps += [tot_a - 1, tot_a // 2, (tot_a + total) // 2, tot_a]          # below slice A's own total; between slice A's total and the batch's
    capfd.readouterr()
    for cap in caps:
        rc, out, cig, coff, st = _host_call(fn, ctx, corp, par, cap, flags)
        assert rc == -5, (call, cap, rc)
        assert int(coff[n]) == total, "%s, capacity %d: cigar_off[n] is %d, the batch needs %d words" % (call, cap, int(coff[n]), total)
        assert (cig[cap:] == SENT).all(), (call, cap)
    err = capfd.readouterr().err
    if call == "align-two-slices":
        assert "in two slices" in err
    if call == "align-width-classes":
        # the query lengths cover all four classes of the whole-query dispatch (16-column steps: up to 64, 128, 256 columns, and above, which
        # is also where a class goes whose widened kernel this scoring does not have); the call went down as one sub-batch per class, each a
        # batch of one plan that reports its pairs -- not as the one plan of "align-one-plan"
        cols = (np.maximum(corp.qlen, 1).astype(np.int64) + 15) // 16 * 16
        classes = len(set(np.digitize(cols, [64, 128, 256], right=True).tolist()))
        subs = [int(m) for m in re.findall(r"\[bsa_align_batch\] (\d+) pairs, mode", err)]
        assert classes == 4 and 1 < len(subs) <= classes and sum(subs) == n, (classes, subs)
    rc, out, cig, coff, st = _host_call(fn, ctx, corp, par, int(coff[n]), flags)
    assert rc == 0 and np.array_equal(coff, eoff) and np.array_equal(st, est) and np.array_equal(out, rec), (call, rc)
    assert PC.check_arena(cig, total, SENT, coff, cigs, True) == sum(1 for c in cigs if len(c))
    if align:
        # no pair of `small` needs the hand-over to the literal kernels (PC.needs_handover; the mixed corpus runs at bandwidth 0, which that
        # screen does not cover) ...
        assert ctx.last_handover() == 0 or call == "align-width-classes"
        # ... unless the test asks for it: every fifth pair (of every sub-batch) re-run and spliced into an arena of exactly the words needed
        monkeypatch.setenv("BSA_DEBUG_HANDOVER", "5")
        rc, out, cig, coff, st = _host_call(fn, ctx, corp, par, total, flags)
        assert rc == 0 and ctx.last_handover() >= n // 5 - 3
        assert np.array_equal(coff, eoff) and np.array_equal(st, est) and np.array_equal(out, rec)
        assert PC.check_arena(cig, total, SENT, coff, cigs, True) == sum(1 for c in cigs if len(c))


# ---- d. a plan re-run on new sequences ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RUN_CONFIGS))
def test_plan_rerun_on_new_sequences(ctx, monkeypatch, name):
    """one plan over the lengths of `small`, run on three blobs of other bases in turn: every run gives the oracle's results for its own blob.
    The 8-bit plan at bandwidth 128 runs the forward pass in 64-row segments (BSA_ALIGN8_XQ=1, BSA_ALIGN8_XQ_SEG=64), which hand the band
    state from segment to segment through a buffer of the context"""
    kind, mode, bw, scoring, kernel = RUN_CONFIGS[name]
    if name == "align-bw128-affine":
        monkeypatch.setenv("BSA_ALIGN8_XQ", "1")
        monkeypatch.setenv("BSA_ALIGN8_XQ_SEG", "64")
        kernel = "fwd_xq"
    plan = _make_plan(ctx, kind, PC.small(), mode, bw, scoring)
    for seed in (1, 2, 1):
        corp = PC.same_lengths(seed)
        exp = PC.expected(corp.pairs, kind, mode, bw, scoring, key="same_lengths_%d" % seed)
        total = int(exp[2][-1])
        got = _run(ctx, plan, kind, _upload(corp), total + GUARD, total)
        assert kernel in ctx.last_kernel_names()[0], ctx.last_kernel_names()
        assert _check(got, exp, total, True, "%s, blob %d" % (name, seed)) == len(corp.good())
    plan.close()


# ---- e. plans taking turns on one context ------------------------------------------------------------------------------------------------
def test_plans_taking_turns_on_one_context(ctx):
    """an 8-bit plan at bandwidth 128, an edit plan on the wave-per-pair kernel and an 8-bit plan with two-piece gaps at bandwidth 64 share one
    context's workspace and row-segment buffer, with a k-mer chaining call in between: every run gives the oracle's results, and the second
    run of a plan gives the bytes of its first"""
    import bsalign_amd as B
    small = PC.small()
    rng = np.random.default_rng(24)
    long_pairs = []
    for k in range(24):
        T = rng.integers(0, 4, size=int(rng.integers(1100, 4001))).astype(np.uint8)
        long_pairs.append((S.mutate(rng, T, (0.02, 0.1, 0.2)[k % 3]), T))
    longs = PC.Corpus(long_pairs)
    cases = {
        "A": ("align", small, S.MODE_GLOBAL, 128, PC.SCORINGS["affine"], "small"),
        "E": ("edit", longs, S.MODE_GLOBAL, 0, None, "long24"),
        "B": ("align", small, S.MODE_GLOBAL, 64, PC.SCORINGS["twopiece"], "small"),
    }
    plans = {k: _make_plan(ctx, v[0], v[1], *v[2:5]) for k, v in cases.items()}
    seqs = {k: _upload(v[1]) for k, v in cases.items()}
    chain_pairs = [small.pairs[k] for k in small.good()[:8]]
    want_chain = [K.kmer_chain(13, q, t) for q, t in chain_pairs]
    first = {}
    for turn, name in enumerate("AEBAE"):
        kind, corp, mode, bw, scoring, key = cases[name]
        exp = PC.expected(corp.pairs, kind, mode, bw, scoring, key=key)
        total = int(exp[2][-1])
        got = _run(ctx, plans[name], kind, seqs[name], total + GUARD, total)
        assert _check(got, exp, total, True, "turn %d, plan %s" % (turn, name)) == len(corp.good())
        if name in first:
            assert all(np.array_equal(a, b) for a, b in zip(first[name], got)), (turn, name)
        first.setdefault(name, got)
        if turn in (1, 3):
            chains = ctx.kmer_chain_batch(chain_pairs, ksz=13)
            assert all(np.array_equal(a, b) for a, b in zip(chains, want_chain))
    for p in plans.values():
        p.close()
