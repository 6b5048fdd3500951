"""Generate tests/golden/rows_sat.npz: the row functions of the REAL reference (oracle/_ref: ref_row_init / _movx / _cal / _merge / _max over
profiles of ref_set_query_prof[_hpc]) under the scorings of tests/rows_sat_cases.py, where its int8 arithmetic clamps and wraps, and under the
default scoring at every bandwidth and mode.  Per chain of rows_sat_cases.draw_fixture_plan(): the inputs (scoring, bandwidth, mode, read and per
step movx, base, profile, rh) and the row after row_init and, per step, the planes and ubegs[0..16] after row_movx, row_cal and row_merge and
what row_max returns.  Also the 8192-column merge program (tasks, read, scoring) and the reference's blocks of its branch ends and merged node, and the hand-made
row pairs of draw_merge_s16_cases with what the reference's row_merge makes of them.
The tests read everything from the file.  Run in the build container:  python tests/golden/make_golden_rows_sat.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import rows_sat_cases as RS  # noqa: E402
import support as S  # noqa: E402


def main():
    assert S.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    R = RS.RefRows()
    plan = RS.draw_fixture_plan()
    rows, off, steps, meta = [], [0], [], []
    for c in plan:
        rhs = []
        b = np.concatenate(RS.run_fixture_chain(R, c, rhs=rhs))
        rows.append(b)
        off.append(off[-1] + len(b))
        steps.append([(m, ba, pr, rh) for (m, ba, pr, _), rh in zip(c["steps"], rhs)])
        meta.append((RS.FIX_SETS.index(c["name"]), c["bw"], c["mode"], c["chain"], len(c["query"])))
    scores = [[(RS.DEFAULT if n == "default" else RS.SETS[n])[k] for k in RS.SC_KEYS] for n in RS.FIX_SETS]
    mp = RS.draw_merge8192_program()
    pw = RS.piecewise(mp["sc"], RS.MERGE_BW)
    blocks = RS.run_program(R, mp, RS.MERGE_BW)
    keep = (5, 8, 9)           # the two branch ends and the merged node
    s16 = RS.draw_merge_s16_cases()
    s16_out = [RS.pack(R.merge(RS.unpack(a, RS.S16_BW, 1), RS.unpack(b, RS.S16_BW, 1), RS.S16_BW // 16, 1), RS.S16_BW, 1) for a, b in s16]
    out = dict(set_names=np.array(RS.FIX_SETS), scores=np.array(scores, np.int32), meta=np.array(meta, np.int32), steps=np.array(steps, np.int32),
               queries=np.concatenate([c["query"] for c in plan]), rows=np.concatenate(rows), row_off=np.array(off, np.int64),
               merge_tasks=mp["tasks"].view(np.uint8), merge_query=mp["query"], merge_score=np.array([mp["sc"][k] for k in RS.SC_KEYS + ("alnmode",)], np.int32),
               merge_blocks=np.array(keep, np.int32), merge_rows=np.stack([RS.pack(blocks[k], RS.MERGE_BW, pw) for k in keep]),
               s16_in=np.stack([np.stack(p) for p in s16]), s16_out=np.stack(s16_out))
    np.savez_compressed(RS.FIXTURE, **out)
    print("wrote %s: %d chains, %d bytes of rows, %d bytes on disk" % (RS.FIXTURE, len(plan), off[-1], os.path.getsize(RS.FIXTURE)))


if __name__ == "__main__":
    main()
