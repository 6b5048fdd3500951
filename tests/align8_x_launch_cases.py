"""The launches of the exact-arithmetic forward kernels (bsa_align8_x.hip: x_choose / x_run) that tests/align_dispatch_cases.py does not reach, as recorded
behaviour: row segments at bandwidth 64 and 256 and with two-piece gaps, the difference form, short rebase periods, integer maxima, the mix of lane counts,
eight lanes at bandwidth 64, the in-place kernels switched off, score only at every width.  The same kind of case and the same run_case() as that list;
the fixture is tests/golden/align8_x_launch.json (tests/golden/make_golden_align_dispatch.py --list x-launch, from the library of the commit the file
names), the replay tests/test_align8_x_launch_gpu.py.  Building the list needs no GPU."""
import json
import os

from align_dispatch_cases import E, G, MODE_NAMES, O, SC, SCORE_ONLY, _case, moving, run_case, static  # noqa: F401  (run_case: for the recorder and the replay)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align8_x_launch.json")

# two scorings that take the absolute-score form with INTEGER maxima at bandwidth 256 (bsa_align8_abs_form: form 1, 64 rows): s = 57, 57 (256 + 8) + 512 = 15560
SC.setdefault("s57", (54, -2, -1, -1, 0, 0))           # tests/test_align8_m3_gpu.py's "s57"
SC.setdefault("s57lin", (53, -1, 0, -2, 0, 0))         # linear gaps: s = m + 2 ge
XQ = {"BSA_ALIGN8_XQ": "1", "BSA_ALIGN8_XQ_SEG": "64"}          # row segments of 64 rows whatever the batch size


def _build():
    cs = []
    seed = [2000]

    def nxt():
        seed[0] += 1
        return seed[0]

    def add(cid, prs, mode, bw, sc, env=None, **kw):
        cs.append(_case(cid, prs, mode, bw, sc, env=env, **kw))

    def xq_tag(env):
        return "xq" if "BSA_ALIGN8_XQ" in env else "whole"

    # forced row segments at 64 and 256: the <8, 4> and <16, 8> instances, absolute at 256
    for bw in (64, 256):
        for sc in ("linear", "affine"):
            prs = moving(nxt(), bw)
            for mode in (G, O, E):
                add("xq-bw%d-%s-%s" % (bw, sc, MODE_NAMES[mode]), prs, mode, bw, sc, env=XQ)
    # two-piece row segments: <8, 4, 2> at 64, <8, 8, 2> at 128
    for bw, env in ((64, XQ), (128, dict(XQ, BSA_ALIGN8_X2_LANES="8"))):
        prs = moving(nxt(), bw)
        for mode in (G, O, E):
            add("xq-bw%d-twopiece-%s" % (bw, MODE_NAMES[mode]), prs, mode, bw, "twopiece", env=env)
    # the difference form where the absolute one would run (gapo4: code format 0 with the other knobs at their defaults)
    for bw, scs in ((128, ("linear", "affine", "gapo4")), (256, ("linear", "affine"))):
        for sc in scs:
            prs = moving(nxt(), bw)
            for env in ({"BSA_ALIGN8_ABS": "0"}, dict(XQ, BSA_ALIGN8_ABS="0")):
                for mode in (G, O, E):
                    add("abs0-bw%d-%s-%s-%s" % (bw, sc, xq_tag(env), MODE_NAMES[mode]), prs, mode, bw, sc, env=env)
    # short rebase periods
    for bw in (128, 256):
        for sc in ("affine", "linear"):
            prs = moving(nxt(), bw)
            for env in ({"BSA_ALIGN8_ABS_R": "8"}, dict(XQ, BSA_ALIGN8_ABS_R="8")):
                for mode in (G, E):
                    add("absr8-bw%d-%s-%s-%s" % (bw, sc, xq_tag(env), MODE_NAMES[mode]), prs, mode, bw, sc, env=env)
    # integer maxima (bandwidth 256 alone)
    for sc in ("s57", "s57lin"):
        prs = moving(nxt(), 256)
        for env in ({}, XQ):
            for mode in (G, E):
                add("intmax-%s-%s-%s" % (sc, xq_tag(env), MODE_NAMES[mode]), prs, mode, 256, sc, env=env)
    # the mix of four- and eight-lane blocks at 128, and its two degenerate ends
    for sc in ("affine", "gapo4"):
        prs = moving(nxt(), 128)
        for env in ({"BSA_ALIGN8_X_N8": "16"}, {"BSA_ALIGN8_X_N8": "16", "BSA_ALIGN8_ABS": "0"}):
            for mode in (G, O, E):
                add("mix16-%s-%s-%s" % (sc, "abs0" if "BSA_ALIGN8_ABS" in env else "abs", MODE_NAMES[mode]), prs, mode, 128, sc, env=env)
    prs = moving(nxt(), 128)
    for n8 in (0, 48):
        add("mix%d-affine-global" % n8, prs, G, 128, "affine", env={"BSA_ALIGN8_X_N8": str(n8)})
    # eight lanes per pair at 64: whole pairs, also where row segments are asked for
    for sc in ("linear", "affine"):
        prs = moving(nxt(), 64)
        for env in ({"BSA_ALIGN8_X_LANES": "8"}, {"BSA_ALIGN8_X_LANES": "8", "BSA_ALIGN8_XQ": "1"}):
            for mode in (G, O):
                add("lanes8-bw64-%s-%s-%s" % (sc, xq_tag(env), MODE_NAMES[mode]), prs, mode, 64, sc, env=env)
    # static batches with the in-place kernels switched off
    for bw in (64, 128, 256):
        for sc in ("linear", "affine", "twopiece"):
            add("nostatic-bw%d-%s-global" % (bw, sc), static(nxt(), bw), G, bw, sc, env={"BSA_ALIGN8_NO_STATIC": "1"})
    # score only
    for bw in (64, 256):
        for sc in ("linear", "affine"):
            for shape, mk in (("moving", moving), ("static", static)):
                prs = mk(nxt(), bw)
                for mode in (G, E):
                    add("score-bw%d-%s-%s-%s" % (bw, sc, shape, MODE_NAMES[mode]), prs, mode, bw, sc, flags=SCORE_ONLY, arena="none")
    for bw in (64, 128, 256):
        for sc in ("linear", "affine"):
            prs = moving(nxt(), bw)
            for mode in (G, E):
                add("score-xq-bw%d-%s-%s" % (bw, sc, MODE_NAMES[mode]), prs, mode, bw, sc, flags=SCORE_ONLY, arena="none", env=XQ)
        add("score-nostatic-bw%d-affine-global" % bw, static(nxt(), bw), G, bw, "affine", flags=SCORE_ONLY, arena="none", env={"BSA_ALIGN8_NO_STATIC": "1"})
    # one plan, run twice, in row segments
    add("plan-twice-bw256-xq", moving(nxt(), 256), G, 256, "affine", env=XQ, call="plan-twice")
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    assert not any("BSA_ALIGN8_XQ_SPIN_CAP" in c["env"] for c in cs)          # (a wait that gives up makes the digest depend on timing)
    return cs


X_CASES = _build()


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)
