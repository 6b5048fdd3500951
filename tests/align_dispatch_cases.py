"""The 8-bit aligner's dispatch as recorded behaviour: the one list of cases that tests/golden/make_golden_align_dispatch.py records (once, against a
named commit's library) and tests/test_align_dispatch_gpu.py replays on the library under test.  A case is a batch of 48 pairs, a parameter
set, BSA_* knobs and a way of calling; what is kept of it is the return code, ctx.last_kernel_names(), ctx.last_handover() and a SHA-256 over the
result records, status words, cigar_off and CIGAR words -- which kernels a configuration runs and every byte they leave, not why.
Building the list needs no GPU; run_case() does."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np

G, O, E = 0, 1, 2
MODE_NAMES = {G: "global", O: "overlap", E: "extend"}
ROWRECORDS, SCORE_ONLY = 0x100, 0x400
E_CIGAR_CAP = -5
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_dispatch.json")
N_PAIRS = 48          # three waves at sixteen pairs a wave: a lane group is not alone in its block

SC = {
    "linear": (2, -6, 0, -3, 0, 0),
    "affine": (2, -6, -3, -2, 0, 0),
    "twopiece": (2, -6, -3, -2, -8, -1),
    "gapo4": (2, -6, -4, -2, 0, 0),            # code format 0 with every knob at its default
    "big": (10, -30, -20, -10, 0, 0),          # bsa_align8_sys_supported answers 2 (test_align8_gpu.py BIG_SCORINGS)
    # gap costs the checked whole-query kernel flags pairs for (test_align8_gpu.py::test_checked_systolic_kernel_flags_...): real hand-overs
    "clamp0": (40, -40, -20, -25, 0, 0),
    "clamp1": (20, -40, -25, -15, 0, 0),
    "clamp2": (5, -60, -3, -60, 0, 0),
    "clamp3": (37, -59, -13, -1, 0, 0),
}


def _mutate(rng, T, div):
    """substitutions, insertions and deletions at a total rate div (23 : 31 : 46, the synthetic generator's split), vectorised"""
    L = len(T)
    hit = rng.random(L) < div
    kind = rng.choice(3, size=L, p=(0.23, 0.31, 0.46))
    sub, ins, dele = hit & (kind == 0), hit & (kind == 1), hit & (kind == 2)
    Q = T.copy()
    Q[sub] = (Q[sub] + 1 + rng.integers(0, 3, int(sub.sum())).astype(np.uint8)) & 3
    reps = np.where(dele, 0, np.where(ins, 2, 1))
    out = np.repeat(Q, reps)
    second = np.cumsum(reps)[ins] - 1          # the copy behind an inserted-after base becomes a fresh base
    out[second] = rng.integers(0, 4, len(second)).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def pairs(seed, tlo=150, thi=400, qlo=0, qhi=0):
    """48 pairs: targets of tlo..thi uniform bases, queries the target at 10 % divergence; qhi: the query cut to a length drawn from qlo..qhi"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N_PAIRS):
        T = rng.integers(0, 4, size=int(rng.integers(tlo, thi + 1))).astype(np.uint8)
        Q = _mutate(rng, T, 0.10)
        if qhi:
            ql = int(rng.integers(qlo, qhi + 1))
            Q = Q[:ql] if len(Q) >= ql else np.concatenate([Q, rng.integers(0, 4, size=ql - len(Q)).astype(np.uint8)])
        out.append((Q, T))
    return tuple(out)


def moving(seed, bw):
    """every query longer than the band"""
    p = pairs(seed, max(150, bw + 64), 400)
    assert all(len(q) > bw for q, _ in p)
    return p


def static(seed, bw):
    """no query longer than the band: static_band"""
    return pairs(seed, 150, 400, bw // 2, bw)


def mixed_classes(seed):
    """queries of 50, 100, 200 and 400 in one batch: at bandwidth 0 four sub-batches"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(N_PAIRS):
        T = rng.integers(0, 4, size=(50, 100, 200, 400)[k % 4]).astype(np.uint8)
        Q = _mutate(rng, T, 0.10)
        ql = len(T)
        Q = Q[:ql] if len(Q) >= ql else np.concatenate([Q, rng.integers(0, 4, size=ql - len(Q)).astype(np.uint8)])
        out.append((Q, T))
    return tuple(out)


def _case(cid, prs, mode, bw, sc, flags=0, env=None, status=True, arena="full", call="batch", seq2bit=False, eqx=False, strands=False, margin=False):
    return dict(id=cid, pairs=prs, mode=mode, bw=bw, sc=sc, flags=flags, env=dict(env or {}), status=status, arena=arena, call=call,
                seq2bit=seq2bit, eqx=eqx, strands=strands, margin=margin)


KNOBS = [
    ("pk", {"BSA_ALIGN8_FWD": "pk"}, 0),
    ("literal", {"BSA_ALIGN8_LITERAL": "1"}, 0),
    ("rowrecords", {}, ROWRECORDS),
    ("do2-0", {"BSA_ALIGN8_DO2": "0"}, 0),
    ("lanes4", {"BSA_ALIGN8_X_LANES": "4"}, 0),
    ("lanes8", {"BSA_ALIGN8_X_LANES": "8"}, 0),
    ("xq", {"BSA_ALIGN8_XQ": "1", "BSA_ALIGN8_XQ_SEG": "64"}, 0),
]


def _build():
    cs = []
    seed = [1000]

    def nxt():
        seed[0] += 1
        return seed[0]

    def add(cid, prs, mode, bw, sc, **kw):
        cs.append(_case(cid, prs, mode, bw, sc, **kw))

    # the register widths with every gap model, moving and static bands, all three modes
    for bw in (64, 128, 256):
        for sc in ("linear", "affine", "twopiece"):
            for shape, mk in (("moving", moving), ("static", static)):
                prs = mk(nxt(), bw)
                for mode in (G, O, E):
                    add("bw%d-%s-%s-%s" % (bw, sc, shape, MODE_NAMES[mode]), prs, mode, bw, sc)
    # the same at bandwidth 128 under the knobs of the compact path
    for name, env, flags in KNOBS:
        for sc in ("linear", "affine", "twopiece"):
            for shape, mk in (("moving", moving), ("static", static)):
                prs = mk(nxt(), 128)
                for mode in (G, O, E):
                    add("bw128-%s-%s-%s-%s" % (name, sc, shape, MODE_NAMES[mode]), prs, mode, 128, sc, flags=flags, env=env)
    for shape, mk in (("moving", moving), ("static", static)):
        prs = mk(nxt(), 128)
        for mode in (G, O, E):
            add("bw128-gapo4-%s-%s" % (shape, MODE_NAMES[mode]), prs, mode, 128, "gapo4")
    # whole-query bands in one width class, widened to a register width or not
    for top in (64, 128, 256):
        prs = pairs(nxt(), 150, 400, top // 2 + 1, top)
        for mode in (G, O, E):
            add("bw0-class%d-%s" % (top, MODE_NAMES[mode]), prs, mode, 0, "affine")
            add("bw0-class%d-nowiden-%s" % (top, MODE_NAMES[mode]), prs, mode, 0, "affine", env={"BSA_ALIGN8_WIDEN": "0"})
    # a bandwidth the register kernels do not have
    for shape, prs in (("inside", pairs(nxt(), 150, 400, 40, 80)), ("longer", moving(nxt(), 80))):
        for mode in (G, O, E):
            add("bw80-%s-%s" % (shape, MODE_NAMES[mode]), prs, mode, 80, "affine")
    # whole-query bands above 256 columns: the systolic path and what keeps a batch off it
    longq = pairs(nxt(), 300, 600, 300, 600)
    for mode in (G, O, E):
        add("sys-%s" % MODE_NAMES[mode], longq, mode, 0, "affine")
        add("sys-off-%s" % MODE_NAMES[mode], longq, mode, 0, "affine", env={"BSA_ALIGN8_SYS": "0"})
        add("sys-chk1-%s" % MODE_NAMES[mode], longq, mode, 0, "affine", env={"BSA_ALIGN8_SYS_CHK": "1"})
        add("sys-big-%s" % MODE_NAMES[mode], longq, mode, 0, "big")
        add("sys-big-chk0-%s" % MODE_NAMES[mode], longq, mode, 0, "big", env={"BSA_ALIGN8_SYS_CHK": "0"})
        add("sys-twopiece-%s" % MODE_NAMES[mode], longq, mode, 0, "twopiece")
    mid = pairs(nxt(), 150, 400, 140, 250)          # two-piece gaps: the systolic kernel starts above 128 columns
    for mode in (G, O, E):
        add("sys-twopiece-from128-%s" % MODE_NAMES[mode], mid, mode, 0, "twopiece")
    # score only
    for shape, mk in (("moving", moving), ("static", static)):
        prs = mk(nxt(), 128)
        for mode in (G, O, E):
            add("score-affine-%s-%s" % (shape, MODE_NAMES[mode]), prs, mode, 128, "affine", flags=SCORE_ONLY, arena="none")
            add("score-twopiece-%s-%s" % (shape, MODE_NAMES[mode]), prs, mode, 128, "twopiece", flags=SCORE_ONLY, arena="none")
            add("score-affine-pk-%s-%s" % (shape, MODE_NAMES[mode]), prs, mode, 128, "affine", flags=SCORE_ONLY, arena="none", env={"BSA_ALIGN8_FWD": "pk"})
    # four width classes in one batch, with and without a status array and a CIGAR arena
    mix = mixed_classes(nxt())
    for mode in (G, O):
        for status in (True, False):
            for arena in ("full", "none"):
                add("classes-%s-%s-%s" % (MODE_NAMES[mode], "status" if status else "nostatus", arena), mix, mode, 0, "affine", status=status, arena=arena)
    add("classes-short-arena", mix, G, 0, "affine", arena="short")
    # the hand-over, forced on the compact path and real on the checked systolic one
    hand = moving(nxt(), 128)
    for status in (True, False):
        add("handover-debug-%s" % ("status" if status else "nostatus"), hand, G, 128, "affine", env={"BSA_DEBUG_HANDOVER": "3"}, status=status)
    add("handover-debug-score", hand, G, 128, "affine", env={"BSA_DEBUG_HANDOVER": "3"}, flags=SCORE_ONLY, arena="none")
    for sc in ("clamp0", "clamp1", "clamp2", "clamp3"):
        add("handover-%s" % sc, longq, O, 0, sc)
        add("handover-%s-nostatus" % sc, longq, O, 0, sc, status=False)
        add("handover-%s-short-arena" % sc, longq, O, 0, sc, arena="short")
    # the two-slice driver
    for mode in (G, O):
        add("slices-%s" % MODE_NAMES[mode], hand, mode, 128, "affine", env={"BSA_BATCH_SLICES": "2"})
    add("slices-debug-handover", hand, G, 128, "affine", env={"BSA_BATCH_SLICES": "2", "BSA_DEBUG_HANDOVER": "3"})
    # the modes that are the plan's business alone, on the compact path and across a hand-over
    for name, kw in (("eqx", dict(eqx=True)), ("qstrand", dict(strands=True)), ("seq2bit", dict(seq2bit=True)), ("margin", dict(margin=True))):
        add("%s-compact" % name, hand, G, 128, "affine", **kw)
        add("%s-handover" % name, hand, G, 128, "affine", env={"BSA_DEBUG_HANDOVER": "3"}, **kw)
    # the plan / run surface
    add("plan-twice", hand, G, 128, "affine", call="plan-twice")
    add("plan-nostatus", hand, G, 128, "affine", call="plan", status=False)
    add("plan-sys-twice", longq, O, 0, "affine", call="plan-twice")
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


CASES = _build()


def _strands(case):
    return [bool((k * 7 + 3) % 5 < 2) for k in range(len(case["pairs"]))] if case["strands"] else None


def _params(B, case):
    par = B.make_params(case["mode"] | case["flags"], case["bw"], *SC[case["sc"]])
    par.mode |= (B.MODE_SEQ2BIT if case["seq2bit"] else 0) | (B.MODE_CIGAR_EQX if case["eqx"] else 0) | (B.MODE_QSTRAND if case["strands"] else 0) \
        | (B.MODE_BAND_MARGIN if case["margin"] else 0)
    return par


def _digest(out, st, off, cig, cap):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(out).tobytes())
    h.update(np.ascontiguousarray(st).tobytes())
    h.update(np.ascontiguousarray(off).tobytes())
    h.update(np.ascontiguousarray(cig[:min(int(off[-1]), cap)]).tobytes())
    return h.hexdigest()


def _batch(B, ctx, case, par, cap):
    """one bsa_align_batch through the C-ABI as bound by bsalign_amd.lib(): a status array and a CIGAR arena only where the case has them"""
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(list(case["pairs"]), case["seq2bit"], _strands(case))
    n = len(qlen)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    want = case["arena"] != "none"
    rc = B.lib().bsa_align_batch(ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(par), B._p(out),
                                 B._p(cig) if want else None, cap if want else 0, B._p(off) if want else None, B._p(st) if case["status"] else None)
    return rc, out, st, off, cig


def _plan(B, ctx, case, par, cap):
    """bsa_align_plan_create, then bsa_align_run once or twice on device-resident buffers; the second run's outputs are the ones kept"""
    import torch
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(list(case["pairs"]), case["seq2bit"], _strands(case))
    n = len(qlen)
    plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, par)
    try:
        d_seqs = torch.from_numpy(seqs.view(np.uint8)).cuda()
        for _ in range(2 if case["call"] == "plan-twice" else 1):
            d_out = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
            d_off = torch.zeros((n + 1) * 8, dtype=torch.uint8, device="cuda")
            d_st = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
            d_cig = torch.zeros(cap, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rc = B.lib().bsa_align_run(plan.h, C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_cig.data_ptr()), cap,
                                       C.c_void_p(d_off.data_ptr()), C.c_void_p(d_st.data_ptr()) if case["status"] else None)
            ctx.sync()
            torch.cuda.synchronize()
        return (rc, d_out.cpu().numpy().view(np.int32), d_st.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64),
                d_cig.cpu().numpy().view(np.uint32))
    finally:
        plan.close()


def run_case(ctx, case):
    """-> {rc, fwd, trace, handover, sha256, words}: words is cigar_off[n].  A "short" arena is one word smaller than what a first call with a
    full arena needed: that first call's hand-over count is kept as well (the path the short call fails on depends on it)."""
    import bsalign_amd as B
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        par = _params(B, case)
        n = len(case["pairs"])
        cap = sum(len(q) + len(t) for q, t in case["pairs"]) + 2 * n + 16
        rec = {}
        fn = _batch if case["call"] == "batch" else _plan
        if case["arena"] == "short":
            rc, out, st, off, cig = fn(B, ctx, case, par, cap)
            assert rc == 0, (case["id"], rc)
            rec["full_handover"] = ctx.last_handover()
            cap = int(off[-1]) - 1
        rc, out, st, off, cig = fn(B, ctx, case, par, cap)
        fwd, trace = ctx.last_kernel_names()
        # (bsa_align_run and a BSA_MODE_ROWRECORDS batch leave the context's hand-over count as the call before them left it)
        handover = None if case["call"] != "batch" or (case["flags"] & ROWRECORDS) else ctx.last_handover()
        rec.update(rc=int(rc), fwd=fwd, trace=trace, handover=handover, sha256=_digest(out, st, off, cig, cap), words=int(off[-1]))
        return rec
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        B.lib()          # (the library takes its snapshot of the knobs again)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)
