"""bsa_window_cns_* (include/bsalign_hip.h): the definition in Python (window_cns_ref) -- the live predicate and its statuses in Python integers, the
HOST consensus caller (bsa_msa_call_consensus) for every live window, the compaction and its arena contract -- and the builders of the batches the
tests upload: random MSAs, one window for every way of failing the predicate, a fixed batch for the arena contract.  No GPU is used here."""
import numpy as np

from window_msa_cases import CNS_WINDOW_DTYPE, NO_IDXS, PAR7

ST_OK, ST_BAD_RECORD, ST_TOO_DEEP, ST_NO_ROOM = 0, 1, 2, 3
FILL = 0xA5
U64 = 1 << 64
SYMBOLS = ("bsa_cns_model_create", "bsa_cns_model_destroy", "bsa_window_cns_run", "bsa_window_cns_batch")
PAR_OTHER = np.array([0.05, 0.02, 0.3, 0.1, 0.5, 0.25, 0.1], dtype=np.float32)      # another psub (and other rates)


def need_symbols():
    """every test of bsa_window_cns_* begins here: without the symbols none of them has anything to say, and each fails"""
    import bsalign_amd as B
    for name in SYMBOLS:
        assert hasattr(B.lib(), name), "the library does not export " + name


def first_clauses(w, cols_cap, out_cap, max_rows):
    """the clauses of the live predicate that need no sum, in the header's order -> the first status that fails (Python integers: nothing wraps)"""
    cols_off, idxs_off, out_off = int(w["cols_off"]), int(w["idxs_off"]), int(w["out_off"])
    nall, nseq, nmax, mlen = int(w["nall"]), int(w["nseq"]), int(w["nmax"]), int(w["mlen"])
    if idxs_off != NO_IDXS or nseq > nall or nmax > nall or mlen >= 1 << 31:
        return ST_BAD_RECORD
    nbytes = mlen * (nall + 3)
    if cols_off + nbytes >= U64 or out_off + mlen >= U64:
        return ST_BAD_RECORD
    if nseq > max_rows:
        return ST_TOO_DEEP
    if cols_off + nbytes > cols_cap or out_off + mlen > out_cap:
        return ST_NO_ROOM
    return ST_OK


def statuses(records, cols_cap, out_cap, max_rows):
    """-> the status of every window: the first clauses, then the workspace clause t[g + 1] <= min(out_cap, cols_cap / 4) with t the exclusive sum of
    mlen over the windows that pass the clauses in front of it"""
    st = [first_clauses(w, cols_cap, out_cap, max_rows) for w in records]
    limit, t = min(out_cap, cols_cap // 4), 0
    for g, w in enumerate(records):
        if st[g] == ST_OK:
            t += int(w["mlen"])
            if t > limit:
                st[g] = ST_NO_ROOM
    return st


def pack_offsets(clen):
    off = np.zeros(len(clen) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(clen, dtype=np.uint64), dtype=np.uint64)
    return off


class Ref:
    """what a run must leave: status, clen, score a window; the column arena; the three output arrays (out_cap bytes, FILL where no window wrote);
    seq_off; the three compact arrays (seq_cap bytes, FILL where nothing was copied)"""


def window_cns_ref(cols, records, cols_cap, out_cap, seq_cap, max_rows, par):
    """cols: the arena as uploaded (at least cols_cap bytes; bytes no live window owns come back as they are)"""
    from bsalign_amd import msa as MSA
    r = Ref()
    n = len(records)
    r.status = np.array(statuses(records, cols_cap, out_cap, max_rows), dtype=np.uint32).reshape(n)
    r.clen, r.score = np.zeros(n, np.uint32), np.zeros(n, np.float64)
    r.cols = np.array(cols, dtype=np.uint8).reshape(-1).copy()
    r.cns, r.qlt, r.alt = (np.full(out_cap, FILL, np.uint8) for _ in range(3))
    for g, w in enumerate(records):
        if r.status[g] != ST_OK or int(w["mlen"]) == 0:
            continue
        c0, nall, mlen, o = int(w["cols_off"]), int(w["nall"]), int(w["mlen"]), int(w["out_off"])
        mine = r.cols[c0:c0 + mlen * (nall + 3)].copy()
        cns, qlt, alt, score = MSA.call_consensus(mine, None, nall, int(w["nseq"]), int(w["nmax"]), mlen, par)
        r.cols[c0:c0 + mlen * (nall + 3)] = mine
        k = len(cns)
        r.clen[g], r.score[g] = k, score
        r.cns[o:o + k], r.qlt[o:o + k], r.alt[o:o + k] = cns, qlt, alt
    r.seq_off = pack_offsets(r.clen)
    r.seq, r.seq_qlt, r.seq_alt = (np.full(seq_cap, FILL, np.uint8) for _ in range(3))
    for g, w in enumerate(records):
        a, b, o = int(r.seq_off[g]), int(r.seq_off[g + 1]), int(w["out_off"])
        if b <= seq_cap and b > a:
            r.seq[a:b], r.seq_qlt[a:b], r.seq_alt[a:b] = r.cns[o:o + b - a], r.qlt[o:o + b - a], r.alt[o:o + b - a]
    return r


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------
def random_msa(rng, nall, mlen, eps=0.12):
    """an (mlen, nall + 3) MSA as bsa_window_msa_* writes one: a template of bases, rows that copy it with substitutions and gaps and are outside the
    window (5) at their ends, the three consensus bytes 4 0 0"""
    cols = np.zeros((mlen, nall + 3), dtype=np.uint8)
    truth = rng.integers(0, 4, mlen).astype(np.uint8)
    ins = rng.random(mlen) < 0.1                               # an insertion column: most rows hold a gap
    for r in range(nall):
        row = truth.copy()
        err = rng.random(mlen) < eps
        row[err] = rng.integers(0, 5, size=int(err.sum()))
        row[ins & (rng.random(mlen) < 0.8)] = 4
        if mlen >= 4 and rng.random() < 0.4:
            row[:int(rng.integers(1, max(2, mlen // 8)))] = 5
        if mlen >= 4 and rng.random() < 0.4:
            row[mlen - int(rng.integers(1, max(2, mlen // 8))):] = 5
        cols[:, r] = row
    cols[:, nall] = 4
    return cols


def make_batch(windows, gap=0):
    """windows: (cols of shape (mlen, nall + 3), nseq, nmax) -> (the blob, the records as bsa_window_msa_* numbers them: cols_off the running bytes
    with `gap` unowned FILL bytes in front of every window, out_off the running mlen)"""
    rec = np.zeros(len(windows), dtype=CNS_WINDOW_DTYPE)
    parts, cacc, oacc = [], 0, 0
    for g, (cols, nseq, nmax) in enumerate(windows):
        mlen, nall = cols.shape[0], cols.shape[1] - 3
        if gap:
            parts.append(np.full(gap, FILL, np.uint8))
            cacc += gap
        rec[g] = (cacc, NO_IDXS, oacc, nall, nseq, nmax, mlen)
        parts.append(cols.reshape(-1))
        cacc += cols.size
        oacc += mlen
    return np.concatenate([np.zeros(0, np.uint8)] + parts), rec


NALLS = (1, 2, 4, 5, 63, 64, 65, 67, 257)
MLENS = (1, 2, 63, 64, 65, 200)


def host_form_batches():
    """name -> (blob, records): every nall with every mlen, nseq and nmax nall and nall - 1 in turn, several depths in one batch; and one window of
    8193 columns at nall 3 (more than one piece of k_cns_finish's chain of origins)"""
    out = {}
    rng = np.random.default_rng(4207)
    for i, mlen in enumerate(MLENS):
        ws = []
        for j, nall in enumerate(NALLS):
            less = max(nall - 1, 0)
            nseq, nmax = [(nall, nall), (less, nall), (less, less)][(i + j) % 3]
            ws.append((random_msa(rng, nall, mlen), nseq, nmax))
        out["mlen_%d" % mlen] = make_batch(ws)
    out["long_window"] = make_batch([(random_msa(rng, 3, 8193), 3, 3), (random_msa(rng, 3, 5), 2, 3)])
    return out


def dead_batch():
    """live windows alternating with one window for each way of failing the predicate -> (blob, records, cols_cap, out_cap, max_rows, the expected
    status of every window, the dead windows' names).  The last window passes every other clause and exceeds the workspace clause: a window without
    rows (3 bytes a column) whose cols_cap / 3 columns lie inside both arenas and take the pass's own sum above min(out_cap, cols_cap / 4)."""
    rng = np.random.default_rng(97)
    max_rows = 6
    live = lambda: (random_msa(rng, 5, int(rng.integers(3, 40))), 5, 5)
    names = ["idxs_off", "nseq_above_nall", "nmax_above_nall", "nall_max", "mlen_2_31", "cols_off_wraps", "past_cols_cap", "past_out_cap", "too_deep"]
    ws = []
    for _ in names:
        ws += [live(), (random_msa(rng, 5, 7), 5, 5)]
    ws.append(live())
    blob, rec = make_batch(ws)
    cols_cap = len(blob)
    out_cap = max(int(rec["out_off"][-1]) + int(rec["mlen"][-1]), cols_cap // 3)
    want = [ST_OK] * len(ws) + [ST_NO_ROOM]

    def dead(name, status, **fields):
        g = 2 * names.index(name) + 1
        for k, v in fields.items():
            rec[g][k] = v
        want[g] = status
        return g
    dead("idxs_off", ST_BAD_RECORD, idxs_off=0)
    dead("nseq_above_nall", ST_BAD_RECORD, nseq=6)
    dead("nmax_above_nall", ST_BAD_RECORD, nmax=6)
    dead("nall_max", ST_NO_ROOM, nall=0xFFFFFFFF, nseq=1, nmax=1, mlen=1)          # (a stride of 2^32 + 2 bytes: two in 32 bits)
    dead("mlen_2_31", ST_BAD_RECORD, mlen=1 << 31)
    dead("cols_off_wraps", ST_BAD_RECORD, cols_off=U64 - 16)                       # (cols_off + 7 * 8 wraps to 40)
    g = dead("past_cols_cap", ST_NO_ROOM)
    rec[g]["cols_off"] = cols_cap + 1 - 7 * 8
    g = dead("past_out_cap", ST_NO_ROOM)
    rec[g]["out_off"] = out_cap + 1 - 7
    dead("too_deep", ST_TOO_DEEP, nall=9, nseq=7, nmax=7, mlen=3, cols_off=0)       # (36 bytes at 0: readable, and not to be read)
    last = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    last[0] = (0, NO_IDXS, 0, 0, 0, 0, cols_cap // 3)
    assert first_clauses(last[0], cols_cap, out_cap, max_rows) == ST_OK and cols_cap // 3 > min(out_cap, cols_cap // 4)
    return blob, np.concatenate([rec, last]), cols_cap, out_cap, max_rows, want, names + ["workspace"]


def arena_batch():
    """eight windows, depths and lengths mixed, one of them without columns"""
    rng = np.random.default_rng(311)
    shapes = [(4, 30), (2, 1), (9, 64), (3, 0), (65, 17), (5, 100), (1, 33), (6, 48)]
    return make_batch([(random_msa(rng, nall, mlen), nall, nall) for nall, mlen in shapes])


def header_example_cns():
    """the worked example of bsa_window_cns_* in include/bsalign_hip.h, typed in by hand: the 12 columns of the bsa_window_msa_* example with vote 1
    (nseq = nmax = 3), the default rates -> (the 72 bytes, the record, cns, qlt, alt, the consensus bytes of the 12 columns)"""
    row0 = [0, 1, 2, 3, 2, 2, 0, 1, 2, 3, 0, 1]
    row1 = [5, 5, 2, 3, 1, 4, 4, 1, 2, 3, 5, 5]
    drow = [0, 1, 2, 3, 4, 4, 0, 1, 2, 3, 0, 1]
    cols = np.array([[row0[i], row1[i], drow[i], 4, 0, 0] for i in range(12)], dtype=np.uint8).reshape(-1)
    rec = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    rec[0] = (0, NO_IDXS, 0, 3, 3, 3, 12)
    cns = [0, 1, 2, 3, 2, 0, 1, 2, 3, 0, 1]
    qlt = [90, 90, 90, 90, 2, 10, 90, 90, 90, 90, 90]
    alt = [0, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0]
    called = [0, 1, 2, 3, 2, 4, 0, 1, 2, 3, 0, 1]
    cq = [90, 90, 90, 90, 2, 4, 10, 90, 90, 90, 90, 90]
    ca = [0, 0, 0, 0, 5, 5, 5, 0, 0, 0, 0, 0]
    return cols, rec, np.array(cns, np.uint8), np.array(qlt, np.uint8), np.array(alt, np.uint8), np.array([called, cq, ca], np.uint8)
