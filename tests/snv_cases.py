"""The SNV caller's definition in Python (snv_ref: bsa_msa_call_snvs of include/bsalign_msa.h, the reference's call_snvs_bspoa) and the cases the CPU
and GPU tests share: the fixture of the real reference (tests/golden/snv.npz), random windows, hand-made shapes, and the diploid closing loop.

Every float operation is a numpy float32 operation (one rounding each, never fused), every double operation Python's float, and exp / log are the
C library's through math -- the libm the host form uses -- so the statement is exact, not approximate: the tests compare without a tolerance."""
import math
import os

import numpy as np

import window_msa_cases as W

SNV_DTYPE = np.dtype([("mpos", np.uint32), ("cpos", np.uint32), ("lpos", np.uint32), ("qual", np.uint32), ("covn", np.uint16), ("refn", np.uint16),
                      ("altn", np.uint16), ("refb", np.uint8), ("altb", np.uint8)])
SNV_WINDOW_DTYPE = np.dtype([("status", np.uint32), ("nsnv", np.uint32), ("nsites", np.uint32), ("pexp", np.float32)])
SNV_PARAMS = np.dtype([("min_varcnt", np.int32), ("min_covfrq", np.float32), ("min_snvqlt", np.uint32), ("skip_first_row", np.uint32)])
ST_OK, ST_BAD_RECORD, ST_TOO_DEEP, ST_TOO_LONG, ST_NOT_CALLED = 0, 1, 2, 3, 4
NO_IDXS = 0xFFFFFFFFFFFFFFFF
F32 = np.float32
STEP, MIN_PROB, DEFAULT_RATE, GRID = F32(0.0005), F32(0.01), F32(0.01), 100
SYMBOLS = ("bsa_msa_call_snvs", "bsa_msa_snv_text", "bsa_snv_model_create", "bsa_snv_model_destroy", "bsa_window_snv_run", "bsa_window_snv_batch")

_LF = [0.0]
for _k in range(1, 1001):
    _LF.append(_LF[-1] + math.log(_k))


def need_symbols():
    """every test of the SNV caller is about these: without them in the library none has anything to say, and each fails"""
    import bsalign_amd as B
    for name in SYMBOLS:
        assert hasattr(B.lib(), name), "the library does not export " + name


def params(min_varcnt=3, min_covfrq=0.5, min_snvqlt=5, skip_first_row=0):
    return np.array([(min_varcnt, min_covfrq, min_snvqlt, skip_first_row)], dtype=SNV_PARAMS)


def binom_log(n, m, p):
    return math.log(p) * m + math.log(1 - p) * (n - m) + (_LF[n] - _LF[m] - _LF[n - m])


def top2(cnt):
    m1, m2 = (0, 1) if cnt[0] >= cnt[1] else (1, 0)
    for i in (2, 3):
        if cnt[i] > cnt[m1]:
            m1, m2 = i, m1
        elif cnt[i] > cnt[m2]:
            m2 = i
    return m1, m2


def mincov_of(realnseq, min_covfrq):
    f = F32(realnseq) * F32(min_covfrq)
    return int(F32(2) if 2 > f else f) & 0xFFFF


def qual_of(covn, altn, pexp):
    q = -(float(F32(binom_log(covn, altn, float(pexp)))) / math.log(10))
    return 1000 if q >= 1000 else int(q) if q > 0 else 0


def spread(altn, covn):
    """what one (altn, covn) entry adds to the grid for a count of one: {bin: weight}, or None off the grid"""
    pexp = F32(1.0 * altn / covn)
    j = int(pexp / STEP)
    if not 0 < j < GRID:
        return None
    row = {}
    for k in range(j):
        prob = F32(math.exp(binom_log(covn, altn, float(pexp - STEP * F32(k)))))
        row[j - k] = prob
        if prob <= MIN_PROB:
            break
    for k in range(1, GRID - j):
        prob = F32(math.exp(binom_log(covn, altn, float(pexp + STEP * F32(k)))))
        row[j + k] = prob
        if prob <= MIN_PROB:
            break
    return row


def snv_ref(cols, nall, nseq, par):
    """-> (SNV_DTYPE records in column order, the estimated rate as float32, the number of sites, the grid sums)"""
    par = np.asarray(par, dtype=SNV_PARAMS).reshape(-1)[0]
    cols = np.asarray(cols, dtype=np.uint8).reshape(-1, nall + 3)
    mlen = cols.shape[0]
    assert nseq <= 1000 and mlen <= 65535 and nseq <= nall
    r0 = int(par["skip_first_row"])
    realnseq = max(nseq - r0, 0)
    mincov = mincov_of(realnseq, par["min_covfrq"])
    rows = cols[:, r0:nseq] if nseq > r0 else cols[:, :0]
    cnt = np.stack([(rows == c).sum(axis=1) for c in range(5)], axis=1)
    covn = cnt.sum(axis=1)
    tops = [top2(c) for c in cnt.tolist()]
    hist = {}
    nsites = 0
    for i in range(mlen):
        m1, m2 = tops[i]
        if cnt[i, m1] + cnt[i, m2] >= mincov:
            nsites += 1
            key = (int(cnt[i, m2]), int(covn[i]))
            hist[key] = hist.get(key, 0) + 1
    psums = [F32(0)] * GRID
    for (altn, cov) in sorted(hist):                           # ascending altn * realnseq + covn - 1
        row = spread(altn, cov) if altn >= 1 else None
        if row is None:
            continue
        for b, wgt in row.items():
            psums[b] = psums[b] + F32(hist[(altn, cov)]) * wgt
    best, pexp = F32(1), DEFAULT_RATE
    for i in range(GRID):
        if best < psums[i]:
            pexp, best = F32(i) * STEP, psums[i]
    out = []
    cpos = lpos = 0
    for i in range(mlen):
        m1, m2 = tops[i]
        refn, altn = int(cnt[i, m1]), int(cnt[i, m2])
        if altn >= int(par["min_varcnt"]) and refn + altn >= mincov:
            qual = qual_of(int(covn[i]), altn, pexp)
            if qual >= int(par["min_snvqlt"]):
                out.append((i, cpos, lpos, qual, int(covn[i]), refn, altn, m1, m2))
        cpos += int(cols[i, nall] < 4)
        lpos += int(cols[i, nall - 1] < 4)
    return np.array(out, dtype=SNV_DTYPE), pexp, nsites, psums


# ---- the fixture of the real reference -------------------------------------------------------------------------------------------------------------------
def golden():
    """-> [(cols (mlen, nall + 3), nall, nseq, the SNP lines as bytes, the records as int rows mpos cpos qual covn refn altn refb altb, the rate x 10000)]"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snv.npz"))
    out = []
    for k in range(int(g["nsets"])):
        nall, nseq, mlen, prob = (int(x) for x in g["meta_%d" % k])
        cols = g["cols_%d" % k]
        assert cols.shape == (mlen, nall + 3)
        out.append((cols, nall, nseq, g["snp_%d" % k].tobytes(), g["snv_%d" % k], prob))
    return out


GOLDEN_FIELDS = ("mpos", "cpos", "qual", "covn", "refn", "altn", "refb", "altb")


def compact_consensus(cols, nall):
    m = cols[:, nall] < 4
    return cols[m, nall], cols[m, nall + 1]


# ---- random and hand-made windows ------------------------------------------------------------------------------------------------------------------------
def random_window(rng, mlen, nall, nseq, err=0.03, nhet=3, gaps=0.1, junk=True):
    """columns of a window: mostly unanimous rows with errors at rate err (codes 0 .. 4), nhet columns split between two bases, a share of insertion
    columns (most rows 4, consensus 4, last row 4), a few rows that start late or end early (5, 6) and, with junk, the odd code above 6; the rows
    from nseq on do not vote and hold anything"""
    cols = np.zeros((mlen, nall + 3), dtype=np.uint8)
    if mlen == 0:
        return cols
    base = rng.integers(0, 4, mlen)
    cols[:, :nall] = base[:, None]
    ins = rng.random(mlen) < gaps
    cols[ins, :nall] = 4
    few = rng.random((mlen, nall)) < 0.08
    cols[:, :nall] = np.where(ins[:, None] & few, rng.integers(0, 4, (mlen, nall)), cols[:, :nall])
    e = rng.random((mlen, nall)) < err
    cols[:, :nall] = np.where(e, rng.integers(0, 5, (mlen, nall)), cols[:, :nall])
    for i in rng.choice(mlen, size=min(nhet, mlen), replace=False):
        share = rng.choice([0.5, 0.3, 0.15])
        alt = (base[i] + 1 + rng.integers(0, 3)) % 4
        cols[i, :nall] = np.where(rng.random(nall) < share, alt, base[i])
    for r in range(nall):
        if rng.random() < 0.3:
            k = int(rng.integers(0, mlen // 4 + 1))
            cols[:k, r] = 5
        if rng.random() < 0.3:
            k = int(rng.integers(0, mlen // 4 + 1))
            cols[mlen - k:, r] = 6
    if junk:
        j = rng.random((mlen, nall)) < 0.01
        cols[:, :nall] = np.where(j, rng.integers(7, 256, (mlen, nall)), cols[:, :nall])
    if nall > nseq:
        cols[:, nseq:nall] = rng.integers(0, 8, (mlen, nall - nseq))
    cols[:, nall - 1] = np.where(ins, 4, rng.integers(0, 4, mlen)) if nall > nseq else cols[:, nall - 1]
    cols[:, nall] = np.where(ins, 4, base)
    cols[:, nall + 1] = rng.integers(0, 91, mlen)
    cols[:, nall + 2] = rng.integers(0, 91, mlen)
    return cols


def pack(windows, gap=0):
    """[(cols, nseq)] -> (blob, cwin records): the windows one behind the other, `gap` junk bytes between them"""
    rec = np.zeros(len(windows), dtype=W.CNS_WINDOW_DTYPE)
    parts, acc = [], 0
    for g, (cols, nseq) in enumerate(windows):
        if gap and g:
            parts.append(np.full(gap, 0x03, np.uint8))
            acc += gap
        rec[g] = (acc, NO_IDXS, 0, cols.shape[1] - 3, nseq, nseq, cols.shape[0])
        parts.append(cols.reshape(-1))
        acc += cols.size
    return np.concatenate([np.zeros(0, np.uint8)] + parts).copy(), rec


def readable(w, cols_cap):
    if int(w["idxs_off"]) != NO_IDXS or int(w["nall"]) < 1 or int(w["nseq"]) > int(w["nall"]) or int(w["mlen"]) >= 1 << 28:
        return False
    end = int(w["cols_off"]) + int(w["mlen"]) * (int(w["nall"]) + 3)
    return end < 1 << 64 and end <= cols_cap


def status_of(w, cols_cap, max_rows, cst):
    if not readable(w, cols_cap):
        return ST_BAD_RECORD
    if int(w["nseq"]) > max_rows:
        return ST_TOO_DEEP
    if int(w["mlen"]) > 65535:
        return ST_TOO_LONG
    return ST_NOT_CALLED if cst else ST_OK


def window_snv_expect(blob, rec, cols_cap, cst, max_rows, par, call):
    """the outputs of a complete bsa_window_snv_* run, window by window through `call` (cols, nall, nseq, par) -> (records, pexp, nsites, ...)
    -> (all records, offsets, SNV_WINDOW_DTYPE records)"""
    out, off, wrec = [], [0], np.zeros(len(rec), dtype=SNV_WINDOW_DTYPE)
    for g, w in enumerate(rec):
        st = status_of(w, cols_cap, max_rows, 0 if cst is None else int(cst[g]))
        snv = np.zeros(0, SNV_DTYPE)
        wrec[g] = (st, 0, 0, 0.0)
        if st == ST_OK:
            nall, mlen, o = int(w["nall"]), int(w["mlen"]), int(w["cols_off"])
            res = call(blob[o:o + mlen * (nall + 3)].reshape(mlen, nall + 3), nall, int(w["nseq"]), par)
            snv = res[0]
            wrec[g] = (st, len(snv), res[2], res[1])
        out.append(snv)
        off.append(off[-1] + len(snv))
    return np.concatenate([np.zeros(0, SNV_DTYPE)] + out), np.array(off, dtype=np.uint64), wrec


# ---- the diploid closing loop ----------------------------------------------------------------------------------------------------------------------------
def diploid_loop(seed=11, w=100, n=2000, nreads=10):
    """a truth of n bases, a second haplotype with substitutions at least 30 bases apart and 20 from every window border (draft coordinates), a draft
    with small edits, nreads error-free reads of each haplotype in turn -> (truth, hap2, draft, the words of a read against the draft, the sites in
    draft coordinates, the reads, one alignment record for all of them)"""
    import cigar_windows_cases as CWC
    rng = np.random.default_rng(seed)
    truth, draft, ws = W.edited_draft(rng, n, w)
    # truth position -> draft position over the M words, and how far the nearest edit is
    t2d, clean = {}, {}
    i = d = 0
    for x in ws:
        ln, op = int(x) >> 4, int(x) & 15
        if op == CWC.M:
            for k in range(ln):
                t2d[i + k] = d + k
                clean[i + k] = min(k, ln - 1 - k)
            i += ln
            d += ln
        elif op == CWC.I:
            i += ln
        else:
            d += ln
    sites, last = [], -1000
    for i in sorted(t2d):
        dpos = t2d[i]
        near_sub = any(0 <= i + k < len(truth) and (i + k) in t2d and draft[t2d[i + k]] != truth[i + k] for k in range(-6, 7))
        if clean[i] >= 6 and not near_sub and 20 <= dpos % w <= w - 21 and dpos - last >= 30:
            sites.append((i, dpos))
            last = dpos
    hap2 = truth.copy()
    for i, _ in sites:
        hap2[i] = (hap2[i] + 1 + rng.integers(0, 3)) % 4
    reads = [truth if r % 2 == 0 else hap2 for r in range(2 * nreads)]
    return truth, hap2, draft, ws, [dpos for _, dpos in sites], reads, CWC.record(0, 0, ws), rng


def dump_golden(k, path):
    """set k of the fixture as the flat file tools/snv_replay.cpp reads"""
    cols, nall, nseq, snp, recs, prob = golden()[k]
    with open(path, "wb") as f:
        f.write(np.array([nall, nseq, cols.shape[0], len(recs), len(snp)], dtype=np.uint32).tobytes())
        f.write(np.ascontiguousarray(cols).tobytes())
        f.write(np.ascontiguousarray(recs, dtype=np.int64).tobytes())
        f.write(snp)
