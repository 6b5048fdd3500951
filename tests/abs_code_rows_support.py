"""Code rows of the absolute-score forward DP (bsa_align8_x.hip, x_forward_abs) for one small batch per code layout, read back from the traceback slots: shared
by tests/golden/make_abs_code_rows.py, which records them, and test_align8_abs_code_rows_gpu.py, which compares."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abs_code_rows.npz")
# layout -> (bandwidth, (M, X, O, E, Q, P), environment of the launch); whole pairs, moving band even where a query is shorter than the band
LAYOUTS = {
    "two-bit": (128, (2, -6, -3, -2, 0, 0), {}),                                 # M | R << 8 | two-bit D / Od fields << 16 per reference block
    "planes128": (128, (2, -2, -4, -2, 0, 0), {"BSA_ALIGN8_X_LANES": "4"}),      # -gapo = 4: M | D << 8 | R << 16 | Od << 24
    "planes256": (256, (2, -6, -3, -2, 0, 0), {}),                               # sixteen cells a block: M | D << 16, R | Od << 16
}
ENV = {"BSA_ALIGN8_XQ": "0", "BSA_ALIGN8_NO_STATIC": "1"}
ENV_KEYS = ("BSA_ALIGN8_XQ", "BSA_ALIGN8_NO_STATIC", "BSA_ALIGN8_X_LANES", "BSA_ALIGN8_DO2", "BSA_ALIGN8_X_N8", "BSA_ALIGN8_ABS", "BSA_ALIGN8_ABS_R", "BSA_ALIGN8_XQ_SEG")


def make_pairs():
    """32 pairs of about 200 rows: related pairs, queries shorter than the band (pad cells, every row at rbeg = 0), queries far longer than their targets (moves of
    two and more, jumps), targets longer than their queries (rows that do not move), unrelated pairs"""
    rng = np.random.default_rng(20250)
    rand = lambda n: rng.integers(0, 4, size=max(int(n), 1)).astype(np.uint8)

    def related(lt, lq, eps):
        t = rand(lt)
        q = t.copy()
        flip = rng.random(lt) < eps
        q[flip] = (q[flip] + rng.integers(1, 4, size=int(flip.sum()))) & 3
        q = np.delete(q, np.nonzero(rng.random(lt) < eps / 2)[0])
        q = q[:lq] if lq <= len(q) else np.concatenate([q, rand(lq - len(q))])
        return q.astype(np.uint8), t

    pairs = []
    for k in range(14):
        lt = int(rng.integers(150, 231))
        pairs.append(related(lt, int(lt * rng.uniform(0.9, 1.1)), float(rng.uniform(0.03, 0.2))))
    for lq in (5, 40, 90, 127, 200, 255):
        pairs.append(related(200, lq, 0.1))
    for lt, ratio in ((60, 20), (24, 64), (9, 200), (70, 5), (100, 3)):
        pairs.append((rand(lt * ratio + 3), rand(lt)))
    for lq, lt in ((200, 230), (300, 230), (520, 230)):
        pairs.append(related(lt, lq, 0.05))
    while len(pairs) < 32:
        n = int(rng.integers(150, 231))
        pairs.append((rand(n), rand(n + 7)))
    return pairs


def code_rows(ctx, pairs, layout):
    """(forward kernel's name, status words, [uint32 array (tlen, 16 blocks, CW dwords) per pair]) of one run of `pairs` at `layout`; the caller has set the environment"""
    import torch
    import bsalign_amd as B
    bw, sc, _ = LAYOUTS[layout]
    n = len(pairs)
    seqs, qoff, qlen, toff, tlen = B.pack_pairs(pairs)
    plan = B.AlignPlan(ctx, qoff, qlen, toff, tlen, B.make_params(B.MODE_GLOBAL, bw, *sc))
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(seqs).to(dev)
    d_out = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    d_cig = torch.zeros(int(qlen.sum() + tlen.sum()) + 64, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    plan.run(d_seqs, d_out, d_cig, d_off, d_st)
    ctx.sync()
    name = ctx.last_kernel_names()[0]
    # (every pair is live in the forward pass; the traceback flags the ones whose band cannot reach the end of a far longer query, after the rows are written)
    cw = bw // 128
    rows = []
    for k in range(n):
        tl = int(tlen[k])
        begs = ((tl + 2) * 4 + 255) & ~255
        slot = plan.debug_slot(k, begs + ((tl + 3) // 4 * 4) * 64 * cw)
        # tiled (bsa_common.h): groups of four rows, inside a group [block][row % 4][cw dwords]; rows past tlen in the last group are not the pair's
        g = slot[begs:].view(np.uint32).reshape(-1, 16, 4, cw)
        rows.append(g.transpose(0, 2, 1, 3).reshape(-1, 16, cw)[:tl].copy())
    plan.close()
    return name, d_st.cpu().numpy().astype(np.uint32), rows
