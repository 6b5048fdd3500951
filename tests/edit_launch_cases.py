"""The edit-distance launchers (bsa_edit.hip: edit_choose and the launch tables) as recorded behaviour: the one list of cases that
tests/golden/make_golden_edit_launch.py records (once, against a named commit's library) and tests/test_edit_launch_gpu.py replays on the library under
test.  A case is a small batch, a mode and bandwidth, BSA_EDIT_* knobs and a way of calling; what is kept of it is the return code,
ctx.last_kernel_names() and a SHA-256 over the result records, status words, cigar_off and every CIGAR word -- which kernels a configuration runs and
every byte they leave, not why.  The count thresholds of the choice are tests/test_edit_choice_cpu.py's business: no case here needs a large batch.
Building the list needs no GPU; run_case() does."""
import ctypes as C
import functools
import json
import os

import numpy as np

from align_dispatch_cases import E, G, MODE_NAMES, O, SCORE_ONLY, _digest, _mutate

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edit_launch.json")

KNOBS = [
    ("default", {}),
    ("tiled0", {"BSA_EDIT_TILED": "0"}),
    ("grp32-0", {"BSA_EDIT_GRP32": "0"}),
    ("grp0", {"BSA_EDIT_GRP": "0"}),
    ("grp1", {"BSA_EDIT_GRP": "1"}),
    ("fwdlanes16", {"BSA_EDIT_FWD_LANES": "16"}),
    ("wave0", {"BSA_EDIT_TRACE_WAVE": "0"}),
    ("coop0", {"BSA_EDIT_TRACE_COOP": "0"}),
    ("tracelanes16", {"BSA_EDIT_TRACE_LANES": "16"}),
]


@functools.lru_cache(maxsize=None)
def pairs(seed, n, tlo, thi, qlo=0, qhi=0):
    """n pairs: targets of tlo..thi uniform bases, queries the target at 10 % divergence; qhi: the query cut or filled to a length drawn from qlo..qhi"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        T = rng.integers(0, 4, size=int(rng.integers(tlo, thi + 1))).astype(np.uint8)
        Q = _mutate(rng, T, 0.10)
        if qhi:
            ql = int(rng.integers(qlo, qhi + 1))
            Q = Q[:ql] if len(Q) >= ql else np.concatenate([Q, rng.integers(0, 4, size=ql - len(Q)).astype(np.uint8)])
        out.append((Q, T))
    return tuple(out)


def banded(seed, bw):
    """every query longer than the band, so the class of the batch is the band; fewer pairs for the wide bands"""
    p = pairs(seed, 48 if bw <= 256 else 24 if bw == 512 else 16, bw + 100, bw + 400)
    assert all(len(q) > bw for q, _ in p)
    return p


def query_ladder(seed):
    """one pair each with a query of 100, 1100, 4100, 8200 and 16400 bases: whole-query bands of a register class and of each class of the wave-per-pair kernel"""
    return tuple(pairs(seed + k, 1, 2000, 3000, ql, ql)[0] for k, ql in enumerate((100, 1100, 4100, 8200, 16400)))


def _case(cid, prs, mode, bw, flags=0, env=None, call="batch"):
    return dict(id=cid, pairs=prs, mode=mode, bw=bw, flags=flags, env=dict(env or {}), call=call)


def _build():
    cs = []

    def add(cid, prs, mode, bw, **kw):
        cs.append(_case(cid, prs, mode, bw, **kw))

    # global mode, one band class that fills its chunk: by default and under every knob of the choice
    for bw in (64, 128, 256, 512, 1024):
        prs = banded(3000 + bw, bw)
        for name, env in KNOBS:
            add("global-bw%d-%s" % (bw, name), prs, G, bw, env=env)
    # whole-query bands: a register class and every class of the wave-per-pair kernel in one batch
    ladder = query_ladder(3100)
    for mode in (O, E):
        add("ladder-%s" % MODE_NAMES[mode], ladder, mode, 0)
    # a moving band above 1024 columns: the generic kernel
    wide = pairs(3200, 8, 2600, 3000)
    assert all(len(q) > 2048 for q, _ in wide)
    add("moving-bw2048", wide, G, 2048)
    add("moving-bw2048-genlanes4", wide, G, 2048, env={"BSA_EDIT_GEN_LANES": "4"})
    # score only: the register widths in global and extend mode (extend: the band is the whole query), and one class above 1024 columns
    for bw in (64, 256, 1024):
        add("score-global-bw%d" % bw, banded(3000 + bw, bw), G, bw, flags=SCORE_ONLY)
        add("score-extend-bw%d" % bw, pairs(3300 + bw, 16, 300, 1200, bw - 60, bw), E, 0, flags=SCORE_ONLY)
    add("score-extend-wide", pairs(3400, 8, 1500, 2000, 1400, 1600), E, 0, flags=SCORE_ONLY)
    # several classes in one chunk: row format 0
    mix = tuple(pairs(3500 + k, 1, ql, ql, ql, ql)[0] for k, ql in enumerate((70, 150, 300, 600) * 12))          # whole-query bands of 128, 192, 320 and 640 columns
    add("classes-global", mix, G, 0)
    add("classes-global-nomerge", mix, G, 0, env={"BSA_EDIT_NO_MERGE": "1"})
    # one plan, run twice
    add("plan-twice-bw128", banded(3000 + 128, 128), G, 128, call="plan-twice")
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    assert all(len(c["pairs"]) <= 128 and all(70 <= len(t) <= 3000 for _, t in c["pairs"]) for c in cs)
    return cs


CASES = _build()


def _batch(B, ctx, case, par, cap):
    """one bsa_edit_batch through the C-ABI; score only: no CIGAR arena"""
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(list(case["pairs"]))
    n = len(qlen)
    out = np.zeros(n, dtype=B.RESULT_DTYPE)
    st = np.zeros(n, dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    want = not (case["flags"] & SCORE_ONLY)
    rc = B.lib().bsa_edit_batch(ctx.h, B._p(seqs), seqs.nbytes, B._p(qoff), B._p(qlen), B._p(toff), B._p(tlen), n, C.byref(par), B._p(out),
                                B._p(cig) if want else None, cap if want else 0, B._p(off) if want else None, B._p(st))
    return rc, out, st, off, cig


def _plan(B, ctx, case, par, cap):
    """bsa_edit_plan_create, then bsa_edit_run twice on device-resident buffers; the second run's outputs are the ones kept"""
    import torch
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(list(case["pairs"]))
    n = len(qlen)
    plan = B.EditPlan(ctx, qoff, qlen, toff, tlen, par.mode, par.bandwidth)
    try:
        d_seqs = torch.from_numpy(seqs.view(np.uint8)).cuda()
        for _ in range(2):
            d_out = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
            d_off = torch.zeros((n + 1) * 8, dtype=torch.uint8, device="cuda")
            d_st = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
            d_cig = torch.zeros(cap, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rc = B.lib().bsa_edit_run(plan.h, C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_cig.data_ptr()), cap,
                                      C.c_void_p(d_off.data_ptr()), C.c_void_p(d_st.data_ptr()))
            ctx.sync()
            torch.cuda.synchronize()
        return (rc, d_out.cpu().numpy().view(np.int32), d_st.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64),
                d_cig.cpu().numpy().view(np.uint32))
    finally:
        plan.close()


def run_case(ctx, case):
    """-> {rc, fwd, trace, sha256, words}: words is cigar_off[n]"""
    import bsalign_amd as B
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        par = B.EditParams()
        par.mode, par.bandwidth = case["mode"] | case["flags"], case["bw"]
        n = len(case["pairs"])
        cap = sum(len(q) + len(t) for q, t in case["pairs"]) + 2 * n + 16
        rc, out, st, off, cig = (_batch if case["call"] == "batch" else _plan)(B, ctx, case, par, cap)
        fwd, trace = ctx.last_kernel_names()
        return dict(rc=int(rc), fwd=fwd, trace=trace, sha256=_digest(out, st, off, cig, cap), words=int(off[-1]))
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
