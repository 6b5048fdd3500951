"""No GPU: the Python statement of bsa_window_cns_* (window_cns_cases.window_cns_ref) against the worked example of include/bsalign_hip.h typed in byte
by byte, every clause of the live predicate violated one at a time, the compaction's offsets and arena contract on hand-made lengths, and the symbols
the library must export."""
import numpy as np

import window_cns_cases as WC
from window_msa_cases import CNS_WINDOW_DTYPE, NO_IDXS, PAR7


def test_the_library_exports_the_calls():
    WC.need_symbols()
    import bsalign_amd as B
    assert hasattr(B.lib(), "bsa_window_cns_step_internal")
    assert (B.CNS_ST_OK, B.CNS_ST_BAD_RECORD, B.CNS_ST_TOO_DEEP, B.CNS_ST_NO_ROOM) == (0, 1, 2, 3)
    assert hasattr(B.Context, "cns_model") and hasattr(B.Context, "window_cns_run") and hasattr(B.Context, "window_cns")


def test_reference_on_the_header_example():
    WC.need_symbols()
    cols, rec, cns, qlt, alt, called = WC.header_example_cns()
    r = WC.window_cns_ref(cols, rec, 72, 12, 11, 3, PAR7)
    assert r.status.tolist() == [0] and r.clen.tolist() == [11] and r.seq_off.tolist() == [0, 11]
    assert np.array_equal(r.cns[:11], cns) and np.array_equal(r.qlt[:11], qlt) and np.array_equal(r.alt[:11], alt)
    assert r.cns[11] == WC.FILL and r.qlt[11] == WC.FILL and r.alt[11] == WC.FILL          # room mlen, clen bytes written
    assert np.array_equal(r.cols.reshape(12, 6)[:, 3:].T, called)
    assert np.array_equal(r.cols.reshape(12, 6)[:, :3], cols.reshape(12, 6)[:, :3])
    assert np.array_equal(r.seq, cns) and np.array_equal(r.seq_qlt, qlt) and np.array_equal(r.seq_alt, alt)
    assert abs(r.score[0] - -9.314772669729516) < 1e-9
    # the same columns with the draft not voting: nothing is called a gap
    rec[0]["nseq"] = rec[0]["nmax"] = 2
    r = WC.window_cns_ref(cols, rec, 72, 12, 12, 2, PAR7)
    assert r.clen.tolist() == [12] and r.cns.tolist() == [0, 1, 2, 3, 2, 2, 0, 1, 2, 3, 0, 1]


def _rec(**kw):
    w = np.zeros(1, dtype=CNS_WINDOW_DTYPE)
    w[0] = (64, NO_IDXS, 10, 5, 5, 4, 7)                     # 7 columns of 8 bytes at 64, 7 bytes out at 10
    for k, v in kw.items():
        w[0][k] = v
    return w[0]


def test_each_clause_of_the_predicate():
    WC.need_symbols()
    cols_cap, out_cap, rows = 64 + 56, 17, 5
    f = lambda w, cc=cols_cap, oc=out_cap, mr=rows: WC.first_clauses(w, cc, oc, mr)
    assert f(_rec()) == WC.ST_OK                              # both ranges end exactly at their caps, nseq == max_rows
    assert f(_rec(idxs_off=0)) == WC.ST_BAD_RECORD
    assert f(_rec(nseq=6)) == WC.ST_BAD_RECORD
    assert f(_rec(nmax=6)) == WC.ST_BAD_RECORD
    assert f(_rec(mlen=1 << 31)) == WC.ST_BAD_RECORD
    assert f(_rec(mlen=(1 << 31) - 1)) == WC.ST_NO_ROOM
    assert f(_rec(cols_off=(1 << 64) - 56)) == WC.ST_BAD_RECORD            # cols_off + 56 == 2^64
    assert f(_rec(cols_off=(1 << 64) - 57)) == WC.ST_NO_ROOM
    assert f(_rec(out_off=(1 << 64) - 7)) == WC.ST_BAD_RECORD
    assert f(_rec(nall=0xFFFFFFFF, nseq=1, nmax=1, mlen=1, cols_off=0)) == WC.ST_NO_ROOM      # 2^32 + 2 bytes
    assert f(_rec(nall=0xFFFFFFFF, nseq=1, nmax=1, mlen=1, cols_off=0), cc=(1 << 32) + 2) == WC.ST_OK
    assert f(_rec(), mr=4) == WC.ST_TOO_DEEP
    assert f(_rec(nseq=6), mr=4) == WC.ST_BAD_RECORD          # the first clause that fails
    assert f(_rec(), cc=cols_cap - 1) == WC.ST_NO_ROOM
    assert f(_rec(), oc=out_cap - 1) == WC.ST_NO_ROOM
    assert f(_rec(), cc=cols_cap - 1, mr=4) == WC.ST_TOO_DEEP
    assert f(_rec(mlen=0, cols_off=cols_cap, out_off=out_cap)) == WC.ST_OK      # an empty window is live
    # the workspace clause: t is the sum of mlen over the windows that pass the clauses in front of it
    ws = np.zeros(4, dtype=CNS_WINDOW_DTYPE)
    ws[0] = (0, NO_IDXS, 0, 0, 0, 0, 10)                      # no rows: 3 bytes a column
    ws[1] = (0, 0, 0, 0, 0, 0, 10)                            # dead: adds nothing to t
    ws[2] = (0, NO_IDXS, 0, 0, 0, 0, 5)
    ws[3] = (0, NO_IDXS, 0, 0, 0, 0, 0)
    assert WC.statuses(ws, 64, 16, 0) == [0, 1, 0, 0]         # min(16, 64 / 4) = 16 >= 15
    assert WC.statuses(ws, 60, 16, 0) == [0, 1, 0, 0]         # 15
    assert WC.statuses(ws, 59, 16, 0) == [0, 1, 3, 3]         # 14 < 15; the empty window behind it: t[4] = 15 too
    assert WC.statuses(ws, 64, 14, 0) == [0, 1, 3, 3]
    assert WC.statuses(ws, 39, 16, 0) == [3, 1, 3, 3]         # 9 < 10


def test_compaction_offsets_and_arena():
    WC.need_symbols()
    assert WC.pack_offsets([3, 0, 5, 1]).tolist() == [0, 3, 3, 8, 9] and WC.pack_offsets([]).tolist() == [0]
    blob, rec = WC.arena_batch()
    out_cap = int(rec["mlen"].sum())
    full = WC.window_cns_ref(blob, rec, len(blob), out_cap, out_cap, 65, PAR7)
    assert np.all(full.status == 0) and full.clen[3] == 0 and np.all(full.clen <= rec["mlen"])
    need = int(full.seq_off[-1])
    assert need == int(full.clen.sum()) and np.all(full.seq[:need] < 4) and np.all(full.seq[need:] == WC.FILL)
    for g in range(len(rec)):
        a, b, o = int(full.seq_off[g]), int(full.seq_off[g + 1]), int(rec[g]["out_off"])
        assert np.array_equal(full.seq[a:b], full.cns[o:o + b - a]) and np.array_equal(full.seq_qlt[a:b], full.qlt[o:o + b - a])
    cut = int(full.seq_off[5]) + 1                            # one byte into window 5: windows 0 .. 4 are copied, nothing of 5 .. 7
    short = WC.window_cns_ref(blob, rec, len(blob), out_cap, cut, 65, PAR7)
    assert np.array_equal(short.seq_off, full.seq_off) and np.array_equal(short.seq[:cut - 1], full.seq[:cut - 1]) and short.seq[cut - 1] == WC.FILL
    none = WC.window_cns_ref(blob, rec, len(blob), out_cap, 0, 65, PAR7)
    assert np.array_equal(none.seq_off, full.seq_off) and len(none.seq) == 0


def test_dead_batch_is_what_it_says():
    WC.need_symbols()
    blob, rec, cols_cap, out_cap, max_rows, want, names = WC.dead_batch()
    assert WC.statuses(rec, cols_cap, out_cap, max_rows) == want and len(names) == 10
    assert want[0::2] == [0] * 10 and all(want[1:-1:2]) and want[-1] == WC.ST_NO_ROOM
    assert sorted(set(want)) == [0, 1, 2, 3]
