#!/usr/bin/env python3
"""No GPU: what a second round inside the window gains, on simulated reads, with the Python statements of the passes and the host consensus caller.

For every window: a truth of `window` bases, a draft that is the truth with `--draft-err` errors, `--depth` reads that are the truth with
`--read-err` errors (substitutions : insertions : deletions as 4 : 3 : 3).  Round 1 aligns every read against the draft (an unbanded global DP, cost
1 a mismatch and 1 a gap unit, the traceback order of bsa_window_realign_*), cuts the guide to diagonal ends, and goes through window_msa_ref, the
host consensus caller and window_stitch_ref (vote 0, min_cov 1).  Round 2 goes through window_realign_ref and the same three again.  The identity of
a called sequence is 1 - (its edit distance to the truth) / (the truth's length), summed over the windows.

Prints ONE JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("windows", type=int, nargs="?", default=300)
    ap.add_argument("window", type=int, nargs="?", default=100)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--read-err", type=float, default=0.10)
    ap.add_argument("--draft-err", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import window_msa_cases as W
    import window_realign_cases as R
    rng = np.random.default_rng(args.seed)
    w, e = args.window, args.read_err
    dist = lambda a, b: R.banded_dp(a, b, 0, 1, 1, banded=False)[0]
    tot = dict(truth=0, draft=0, round1=0, round2=0)
    better = worse = same = dead = 0
    for _ in range(args.windows):
        truth = rng.integers(0, 4, w).astype(np.uint8)
        draft = R.mutate(rng, truth, 0.4 * args.draft_err, 0.3 * args.draft_err, 0.3 * args.draft_err)[:w]
        ps = []
        for _ in range(args.depth):
            read = R.mutate(rng, truth, 0.4 * e, 0.3 * e, 0.3 * e)
            _, steps, _ = R.banded_dp(read, draft, 0, 1, 1, banded=False)
            dg = [i for i, op in enumerate(steps) if op == R.OP_M]
            if not dg:
                continue
            lead, kept = steps[:dg[0]], steps[dg[0]:dg[-1] + 1]
            q0, t0 = lead.count(R.OP_I), lead.count(R.OP_D)
            qn = sum(1 for op in kept if op != R.OP_D)
            ps.append((t0, R.runs(kept), read[q0:q0 + qn]))
        b = W.make([(draft, None, ps)], max(w, len(draft)))
        st1, _ = R.stitched(b)
        seq1 = st1.seq[:int(st1.seq_off[-1])]
        rb = R.from_round1(b, st1)
        r = R.window_realign_ref(rb, R.par(2 * w, 2 * w, 0, 1, 1), 0)
        dead += int((r.pstatus & 0xFF != 0).sum())
        st2, _ = R.stitched(R.round2_batch(rb, r, 2 * w))
        seq2 = st2.seq[:int(st2.seq_off[-1])]
        d0, d1, d2 = dist(draft, truth), dist(seq1, truth), dist(seq2, truth)
        tot["truth"] += len(truth); tot["draft"] += d0; tot["round1"] += d1; tot["round2"] += d2
        better += d2 < d1; worse += d2 > d1; same += d2 == d1
    ident = lambda d: round(1.0 - d / tot["truth"], 5)
    print(json.dumps({"config": vars(args), "truth_bases": tot["truth"], "edits": {k: int(tot[k]) for k in ("draft", "round1", "round2")},
                      "identity": {k: ident(tot[k]) for k in ("draft", "round1", "round2")},
                      "windows_better": int(better), "windows_worse": int(worse), "windows_same": int(same), "pieces_not_realigned": dead}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
