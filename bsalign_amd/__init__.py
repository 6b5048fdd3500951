"""bsalign_amd -- Python binding of libbsalign_hip.so (the MI355X implementation of bsalign's DP hot path).

This package is plumbing for tests / bench.py: it loads the in-tree C-ABI library
(include/bsalign_hip.h) with ctypes and mirrors its entry points.  There is NO CPU
fallback anywhere: if the library is missing or no GPU is usable every compute call
raises.  The host-side drop-in for C callers is include/bsalign_compat.h.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSA_LIB_PATH") or os.path.join(_HERE, "libbsalign_hip.so")      # BSA_LIB_PATH: development builds

MODE_GLOBAL, MODE_OVERLAP, MODE_EXTEND = 0, 1, 2
MODE_ROWRECORDS, MODE_SCORE_ONLY, MODE_SEQ2BIT = 0x100, 0x400, 0x800       # flags OR-ed into the mode (include/bsalign_hip.h)
MODE_CIGAR_EQX = 0x1000                                                   # ... M words leave as runs of = and X
MODE_QSTRAND = 0x2000                                                     # ... bit 63 of qoff[k] is the query's strand
MODE_BAND_MARGIN = 0x4000                                                 # ... status[k] >> ST_MARGIN_SHIFT is the pair's band margin (8-bit aligner only)
ST_MARGIN_SHIFT, ST_MARGIN_NONE = 16, 0xFFFF                              # ST_MARGIN_NONE: no band edge constrained the path, or the pair has no CIGAR
QOFF_REVCOMP = 1 << 63                                                    # in qoff[k], with MODE_QSTRAND: align the reverse complement of the stored query
CIGAR_M, CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 0, 1, 2, 7, 8
ST_BAD_BASE, ST_EMPTY, ST_TRACE, ST_DEVICE = 1, 2, 4, 8
KMER_CHAIN_DEVICE = 1                                                      # bsa_kmer_edit_batch2: the anchors come from the device chainer
KMER_STRAND_AUTO = 2                                                       # bsa_kmer_chain_batch2 / bsa_kmer_edit_batch2: the call finds each pair's strand ...
ST_REVCOMP = 16                                                            # ... and sets this status bit where it used the reverse complement of the stored query
WINDOW_NONE = 0xFFFFFFFF                                                   # bsa_cigar_windows_*: all four fields of a window without an aligned column
PIECE_ST_NOT_ON_PATH = 1                                                   # bsa_piece_cigars_*: a piece whose ends are not aligned columns of its pair

E_NAMES = {0: "OK", -1: "BSA_E_NODEVICE", -2: "BSA_E_ARG", -3: "BSA_E_NOMEM", -4: "BSA_E_HIP",
           -5: "BSA_E_CIGAR_CAP", -6: "BSA_E_UNSUPPORTED"}


class BsaError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__("%s (%d) %s" % (E_NAMES.get(code, "?"), code, msg))


class AlignParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("bandwidth", C.c_uint32), ("matrix", C.c_int8 * 16),
                ("gapo1", C.c_int8), ("gape1", C.c_int8), ("gapo2", C.c_int8), ("gape2", C.c_int8)]


class RowTask(C.Structure):
    _fields_ = [("op", C.c_uint32), ("src", C.c_uint32), ("dst", C.c_uint32), ("qoff_src", C.c_uint32), ("qoff_dst", C.c_uint32),
                ("toff", C.c_uint32), ("query", C.c_uint32), ("base", C.c_uint8), ("prof", C.c_uint8), ("reserved", C.c_uint16)]


class RowsParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("bandwidth", C.c_uint32), ("M", C.c_int8), ("X", C.c_int8), ("refbonus", C.c_int8),
                ("gapo1", C.c_int8), ("gape1", C.c_int8), ("gapo2", C.c_int8), ("gape2", C.c_int8)]


ROW_TASK_DTYPE = np.dtype([("op", np.uint32), ("src", np.uint32), ("dst", np.uint32), ("qoff_src", np.uint32), ("qoff_dst", np.uint32),
                           ("toff", np.uint32), ("query", np.uint32), ("base", np.uint8), ("prof", np.uint8), ("reserved", np.uint16)])


class SweepParams(C.Structure):
    _fields_ = [("rows", RowsParams), ("T", C.c_int32)]


SWEEP_PROG_DTYPE = np.dtype([("first_task", np.uint32), ("ntasks", np.uint32), ("first_block", np.uint32), ("reserved", np.uint32)])
SWEEP_RESULT_DTYPE = np.dtype([("maxscr", np.int32), ("maxidx", np.int32), ("maxoff", np.int32), ("reserved", np.int32)])
# the wavefront sweep's program (include/bsalign_hip.h: bsa_poa_node_t, bsa_poa_edge_t, bsa_poa_cand_t, bsa_poa_prog_t, ...)
POA_CELL_DTYPE = np.dtype([("h", np.int32), ("e", np.int8), ("q", np.int8), ("tag", np.uint16)])
POA_NODE_DTYPE = np.dtype([("rpos", np.uint32), ("gnode", np.uint32), ("first_in", np.uint32), ("n_in", np.uint16), ("base", np.uint8), ("flags", np.uint8),
                           ("in0_src", np.uint32), ("in0_movx", np.uint32), ("in0_tk", np.uint32), ("in1_src", np.uint32), ("in1_movx", np.uint32), ("in1_tk", np.uint32),
                           ("r0", np.uint32), ("r1", np.uint32)])
POA_EDGE_DTYPE = np.dtype([("src", np.uint32), ("cov", np.uint32), ("src_rpos", np.uint32), ("reserved", np.uint32)])
POA_CAND_DTYPE = np.dtype([("node", np.uint32), ("kind", np.uint32)])
POA_EVENT_DTYPE = np.dtype([("node", np.uint32), ("x", np.int32), ("bt", np.uint32)])
POA_PROG_DTYPE = np.dtype([("first_node", np.uint32), ("nnodes", np.uint32), ("first_edge", np.uint32), ("nedges", np.uint32), ("first_cand", np.uint32), ("ncands", np.uint32),
                           ("slen", np.uint32), ("event_cap", np.uint32), ("query_off", np.uint64), ("first_event", np.uint64)])
POA_RESULT_DTYPE = np.dtype([("maxscr", np.int32), ("maxidx", np.int32), ("maxoff", np.int32), ("status", np.int32), ("nevents", np.int32),
                             ("fin_node", np.int32), ("fin_x", np.int32), ("reserved", np.int32)])
ROW_OP_UPDATE, ROW_OP_MERGE, ROW_OP_INIT, ROW_OP_SCORE_TAIL, ROW_OP_SCORE_END = 0, 1, 2, 3, 4


class EditParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("bandwidth", C.c_uint32)]


class KmerParams(C.Structure):
    """bsa_kmer_params_t: k-mer size (the reference's CLI default is 13) and host threads (0 = all)"""
    _fields_ = [("ksz", C.c_uint32), ("threads", C.c_uint32)]


class SELECT_PARAMS(C.Structure):
    """bsa_select_params_t (bsa_window_select_*): at most max_depth pieces a window (0: no cap), a piece spans min_span target columns or more, its
    pair has mat * ident_den >= ident_num * aln (ident_den 0: no test), seed decides among pieces of equal span"""
    _fields_ = [("max_depth", C.c_uint32), ("min_span", C.c_uint32), ("ident_num", C.c_uint32), ("ident_den", C.c_uint32), ("seed", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class REALIGN_PARAMS(C.Structure):
    """bsa_realign_params_t (bsa_window_realign_*): round 2's window size (a window's stitched sequence is at most that long), the longest piece, the
    smallest band margin a piece may have, and the costs of a mismatch and of a gap unit"""
    _fields_ = [("window2", C.c_uint32), ("max_len", C.c_uint32), ("min_margin", C.c_uint32), ("x", C.c_uint32), ("g", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def realign_params(window2, max_len=1024, min_margin=8, x=1, g=1):
    """a bsa_realign_params_t"""
    return REALIGN_PARAMS(int(window2), int(max_len), int(min_margin), int(x), int(g))


RESULT_DTYPE = np.dtype([(n, np.int32) for n in ("score", "qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln")])
# bsa_piece_t (bsa_window_pieces_*): a read's piece in one window of the draft
PIECE_DTYPE = np.dtype([("pair", np.uint32), ("q_first", np.uint32), ("len", np.uint32), ("t_first", np.uint32), ("t_last", np.uint32), ("reserved", np.uint32),
                        ("base_off", np.uint64)])

_lib = None


# bsa_cns_window_t (include/bsalign_msa.h): what bsa_window_msa_* writes and bsa_msa_call_consensus_batch takes
CNS_WINDOW_DTYPE = np.dtype([("cols_off", np.uint64), ("idxs_off", np.uint64), ("out_off", np.uint64),
                             ("nall", np.uint32), ("nseq", np.uint32), ("nmax", np.uint32), ("mlen", np.uint32)])
# d_status of bsa_window_cns_*: the first clause of the live predicate that a window fails (BSA_CNS_ST_*)
CNS_ST_OK, CNS_ST_BAD_RECORD, CNS_ST_TOO_DEEP, CNS_ST_NO_ROOM = 0, 1, 2, 3
# bsa_stitch_t (bsa_window_stitch_*): a window's status, its emitted bases, its units of each kind, the draft bases kept, its words
STITCH_DTYPE = np.dtype([(n, np.uint32) for n in ("status", "slen", "eq", "x", "ins", "del", "kept", "ncig")])
STITCH_ST_CALLED, STITCH_ST_DRAFT, STITCH_ST_BAD_RECORD = 0, 1, 2
# bsa_snv_t (bsa_msa_call_snvs, bsa_window_snv_*): a call's column, its position in the consensus and in the last row (the draft), its quality, the
# column's coverage and the two alleles' counts and bases; bsa_snv_window_t: a window's status, calls, sites and estimated error rate;
# bsa_snv_params_t with the reference's defaults
SNV_DTYPE = np.dtype([("mpos", np.uint32), ("cpos", np.uint32), ("lpos", np.uint32), ("qual", np.uint32), ("covn", np.uint16), ("refn", np.uint16),
                      ("altn", np.uint16), ("refb", np.uint8), ("altb", np.uint8)])
SNV_WINDOW_DTYPE = np.dtype([("status", np.uint32), ("nsnv", np.uint32), ("nsites", np.uint32), ("pexp", np.float32)])
SNV_PARAMS = np.dtype([("min_varcnt", np.int32), ("min_covfrq", np.float32), ("min_snvqlt", np.uint32), ("skip_first_row", np.uint32)])
SNV_ST_OK, SNV_ST_BAD_RECORD, SNV_ST_TOO_DEEP, SNV_ST_TOO_LONG, SNV_ST_NOT_CALLED = 0, 1, 2, 3, 4
# d_pstatus of bsa_window_realign_*: 0, or the first clause a piece fails (BSA_REALIGN_ST_*); REALIGN_ST_EDGE is a flag beside 0
REALIGN_ST_OK, REALIGN_ST_NO_WINDOW, REALIGN_ST_BAD_PIECE, REALIGN_ST_TOO_LONG, REALIGN_ST_EMPTY_SPAN, REALIGN_ST_OFF_BAND, REALIGN_ST_NO_DIAG = 0, 1, 2, 3, 4, 5, 6
REALIGN_ST_EDGE = 0x100


def snv_params(min_varcnt=3, min_covfrq=0.5, min_snvqlt=5, skip_first_row=0):
    """a bsa_snv_params_t as a SNV_PARAMS array of one record"""
    return np.array([(min_varcnt, min_covfrq, min_snvqlt, skip_first_row)], dtype=SNV_PARAMS)
DIAGDP_PROB_DTYPE = np.dtype([("seq0", np.uint64), ("seq1", np.uint64), ("mats0", np.uint64, (4,)), ("mats1", np.uint64, (4,)),
                              ("out0", np.uint64), ("out1", np.uint64), ("mlen", np.uint32), ("mbeg", np.uint32), ("mend", np.uint32), ("W", np.uint32)])


def build():
    """compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)"""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "all"], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libbsalign_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                               "there is no CPU fallback")
        # PyTorch ships its own copy of the HIP runtime: when torch is imported AFTER this library has loaded the system's
        # libamdhip64 the process ends up with two runtimes and torch finds no GPU.  Loading torch first makes the
        # library bind to the copy torch uses (BSA_NO_TORCH_PRELOAD=1 skips this, e.g. for host-only helper processes).
        if "torch" not in sys.modules and not os.environ.get("BSA_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        vp, u8p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
        L.bsa_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.bsa_ctx_destroy.argtypes = [vp]
        L.bsa_ctx_destroy.restype = None
        L.bsa_ctx_set_stream.argtypes = [vp, vp]
        L.bsa_ctx_set_workspace_limit.argtypes = [vp, C.c_size_t]
        L.bsa_ctx_sync.argtypes = [vp]
        L.bsa_last_error.argtypes = [vp]
        L.bsa_last_error.restype = C.c_char_p
        L.bsa_ctx_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double)]
        L.bsa_ctx_last_trace_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
        L.bsa_ctx_last_margin_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
        L.bsa_ctx_last_kernel_name.argtypes = [vp, C.c_int]
        L.bsa_ctx_last_kernel_name.restype = C.c_char_p
        L.bsa_ctx_last_handover.argtypes = [vp]
        L.bsa_ctx_last_handover.restype = C.c_long
        L.bsa_set_score_matrix.argtypes = [C.POINTER(C.c_int8), C.c_int8, C.c_int8]
        L.bsa_set_score_matrix.restype = None
        L.bsa_align_batch.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, u64p, u32p, C.c_size_t, C.POINTER(AlignParams),
                                      vp, u32p, C.c_size_t, u64p, u32p]
        L.bsa_align_plan_create.argtypes = [vp, u64p, u32p, u64p, u32p, C.c_size_t, C.POINTER(AlignParams), C.POINTER(vp)]
        if hasattr(L, "bsa_align8_abs_form_internal"):          # (a BSA_LIB_PATH build from before it: everything else still runs)
            L.bsa_align8_abs_form_internal.argtypes = [C.POINTER(AlignParams), C.POINTER(C.c_uint32)]
        if hasattr(L, "bsa_align8_row_target_internal"):
            L.bsa_align8_row_target_internal.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32,
                                                         C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]
        if hasattr(L, "bsa_align8_flag_span_internal"):
            L.bsa_align8_flag_span_internal.argtypes = [C.POINTER(AlignParams), C.POINTER(C.c_uint32)]
        if hasattr(L, "bsa_align8_x_choice_internal"):
            L.bsa_align8_x_choice_internal.argtypes = [C.POINTER(AlignParams), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint64, C.c_int,
                                                       C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        if hasattr(L, "bsa_align8_trace_choice_internal"):
            L.bsa_align8_trace_choice_internal.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.bsa_align_plan_destroy.argtypes = [vp]
        L.bsa_align_plan_destroy.restype = None
        L.bsa_align_plan_cells.argtypes = [vp]
        L.bsa_align_plan_cells.restype = C.c_double
        L.bsa_align_run.argtypes = [vp, u8p, vp, u32p, C.c_size_t, u64p, u32p]
        L.bsa_synth_stride.argtypes = [C.c_uint32]
        L.bsa_synth_stride.restype = C.c_size_t
        L.bsa_synth_pairs_host.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t, C.c_uint32, C.c_uint32, u8p, u32p]
        L.bsa_synth_pairs_dev.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_size_t, C.c_uint32, C.c_uint32, u8p, u32p]
        L.bsa_seq_pack2bit.argtypes = [vp, u8p, C.c_uint64, u64p, u32p]
        if hasattr(L, "bsa_edit_batch"):
            L.bsa_edit_batch.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, u64p, u32p, C.c_size_t, C.POINTER(EditParams),
                                         vp, u32p, C.c_size_t, u64p, u32p]
            L.bsa_edit_plan_create.argtypes = [vp, u64p, u32p, u64p, u32p, C.c_size_t, C.POINTER(EditParams), C.POINTER(vp)]
            L.bsa_edit_plan_destroy.argtypes = [vp]
            L.bsa_edit_plan_destroy.restype = None
            L.bsa_edit_plan_cells.argtypes = [vp]
            L.bsa_edit_plan_cells.restype = C.c_double
            L.bsa_edit_run.argtypes = [vp, u8p, vp, u32p, C.c_size_t, u64p, u32p]
        if hasattr(L, "bsa_edit_choice_internal"):
            L.bsa_edit_choice_internal.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(C.c_uint64), C.c_char_p, C.c_char_p, C.c_size_t]
        if hasattr(L, "bsa_seq16_internal"):
            L.bsa_seq16_internal.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, u8p, u32p]
        L.bsa_kmer_edit_batch.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, u64p, u32p, C.c_size_t, C.POINTER(KmerParams),
                                          vp, u32p, C.c_size_t, u64p, u32p]
        L.bsa_kmer_edit_batch2.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, u64p, u32p, C.c_size_t, C.POINTER(KmerParams),
                                           vp, u32p, C.c_size_t, u64p, u32p, C.c_uint32]
        L.bsa_kmer_chain_batch.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, u64p, u32p, C.c_size_t, C.c_uint32,
                                           u64p, C.c_size_t, u64p, u32p]
        L.bsa_kmer_chain_batch2.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, u64p, u32p, C.c_size_t, C.c_uint32,
                                            u64p, C.c_size_t, u64p, u32p, C.c_uint32]
        L.bsa_ctx_last_kmer_chain_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_long)]
        L.bsa_kmer_chain_plan_create.argtypes = [vp, u64p, u32p, u64p, u32p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.bsa_kmer_chain_plan_destroy.argtypes = [vp]
        L.bsa_kmer_chain_plan_destroy.restype = None
        L.bsa_kmer_chain_plan_chunks.argtypes = [vp]
        L.bsa_kmer_chain_plan_chunks.restype = C.c_uint32
        L.bsa_kmer_chain_words_bound.argtypes = [u32p, u32p, C.c_size_t]
        L.bsa_kmer_chain_words_bound.restype = C.c_uint64
        L.bsa_kmer_chain_run.argtypes = [vp, u8p, u64p, C.c_size_t, u64p, u32p]
        L.bsa_cigar_windows_bound.argtypes = [u32p, C.c_size_t, C.c_uint32]
        L.bsa_cigar_windows_bound.restype = C.c_uint64
        L.bsa_cigar_windows_run.argtypes = [vp, vp, u32p, u64p, C.c_size_t, C.c_uint32, vp, C.c_size_t, u64p]
        L.bsa_cigar_windows_batch.argtypes = [vp, vp, u32p, u64p, C.c_size_t, C.c_uint32, vp, C.c_size_t, u64p]
        if hasattr(L, "bsa_window_pieces_run"):                 # (a BSA_LIB_PATH build from before it: everything else still runs)
            L.bsa_window_pieces_run.argtypes = [vp, u8p, u64p, u32p, vp, u64p, C.c_size_t, C.c_uint32, u64p, C.c_size_t, C.c_uint32,
                                                vp, C.c_size_t, u64p, u8p, C.c_size_t, u64p]
            L.bsa_window_pieces_batch.argtypes = [vp, u8p, C.c_size_t, u64p, u32p, vp, u64p, C.c_size_t, C.c_uint32, u64p, C.c_size_t, C.c_uint32,
                                                  vp, C.c_size_t, u64p, u8p, C.c_size_t, u64p]
        if hasattr(L, "bsa_window_select_run"):
            L.bsa_window_select_run.argtypes = [vp, vp, u64p, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.POINTER(SELECT_PARAMS), vp, C.c_size_t, u64p, u32p, u32p]
            L.bsa_window_select_batch.argtypes = L.bsa_window_select_run.argtypes
            L.bsa_window_select_step_internal.argtypes = [vp, C.c_int] + L.bsa_window_select_run.argtypes[1:]
        if hasattr(L, "bsa_piece_cigars_run"):
            L.bsa_piece_cigars_bound.argtypes = [u64p, C.c_size_t, C.c_size_t]
            L.bsa_piece_cigars_bound.restype = C.c_uint64
            L.bsa_piece_cigars_run.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
            L.bsa_piece_cigars_batch.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
        if hasattr(L, "bsa_window_msa_run"):
            L.bsa_window_msa_bound.argtypes = [u64p, C.c_size_t, C.c_uint32, C.c_uint64]
            L.bsa_window_msa_bound.restype = C.c_uint64
            L.bsa_window_msa_run.argtypes = [vp, vp, u64p, C.c_size_t, C.c_size_t, u8p, C.c_size_t, u32p, C.c_size_t, u64p, u8p, u64p, u32p,
                                             C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_size_t, u64p, vp]
            L.bsa_window_msa_batch.argtypes = L.bsa_window_msa_run.argtypes
        if hasattr(L, "bsa_window_cns_run"):
            L.bsa_cns_model_create.argtypes = [vp, vp, C.POINTER(vp)]
            L.bsa_cns_model_destroy.argtypes = [vp]
            L.bsa_cns_model_destroy.restype = None
            L.bsa_window_cns_run.argtypes = [vp, vp, u8p, C.c_size_t, vp, C.c_size_t, C.c_uint32, u8p, u8p, u8p, C.c_size_t, u32p, vp, u32p,
                                             u8p, u8p, u8p, C.c_size_t, u64p]
            L.bsa_window_cns_batch.argtypes = L.bsa_window_cns_run.argtypes
            L.bsa_window_cns_step_internal.argtypes = [vp, C.c_int] + L.bsa_window_cns_run.argtypes[1:]
        if hasattr(L, "bsa_window_stitch_run"):
            L.bsa_window_stitch_run.argtypes = [vp, u8p, C.c_size_t, vp, C.c_size_t, u32p, C.c_uint32, u8p, u8p, u8p, C.c_size_t, u64p, u32p, C.c_size_t, u64p, vp]
            L.bsa_window_stitch_batch.argtypes = L.bsa_window_stitch_run.argtypes
            L.bsa_window_stitch_step_internal.argtypes = [vp, C.c_int] + L.bsa_window_stitch_run.argtypes[1:]
        if hasattr(L, "bsa_window_realign_run"):
            L.bsa_window_realign_run.argtypes = [vp, vp, u64p, C.c_size_t, C.c_size_t, u8p, C.c_size_t, C.c_uint32, u8p, C.c_size_t, u64p, u32p, C.c_size_t, u64p,
                                                 C.POINTER(REALIGN_PARAMS), vp, u32p, C.c_size_t, u64p, u32p, u32p, u64p, u32p]
            L.bsa_window_realign_batch.argtypes = L.bsa_window_realign_run.argtypes
            L.bsa_window_realign_step_internal.argtypes = [vp, C.c_int] + L.bsa_window_realign_run.argtypes[1:]
        L.bsa_snv_model_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
        L.bsa_snv_model_destroy.argtypes = [vp]
        L.bsa_snv_model_destroy.restype = None
        L.bsa_window_snv_run.argtypes = [vp, vp, u8p, C.c_size_t, vp, C.c_size_t, u32p, vp, vp, C.c_size_t, u64p, vp]
        L.bsa_window_snv_step_internal.argtypes = [vp, C.c_int] + L.bsa_window_snv_run.argtypes[1:]
        L.bsa_window_snv_batch.argtypes = [vp, C.c_uint32, u8p, C.c_size_t, vp, C.c_size_t, u32p, vp, vp, C.c_size_t, u64p, vp]
        L.bsa_rows_block_bytes.argtypes = [C.c_uint32, C.c_int8, C.c_int8, C.c_int8, C.c_int8]
        L.bsa_rows_block_bytes.restype = C.c_size_t
        L.bsa_rows_run.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, C.POINTER(RowsParams)]
        L.bsa_sweep_run.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp, vp, C.POINTER(SweepParams), vp]
        L.bsa_sweep_host.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.POINTER(SweepParams), vp, C.c_size_t, vp]
        L.bsa_poa_graph_supported.argtypes = [C.POINTER(SweepParams), C.c_uint32]
        L.bsa_poa_graph_host.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(SweepParams),
                                         vp, vp, C.c_size_t, vp, vp]
        L.bsa_poa_graph_run.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_uint32, C.POINTER(SweepParams), vp, vp, vp, vp, vp, vp]
        L.bsa_align_debug_rows.argtypes = [vp, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.bsa_diagdp_batch.argtypes = [vp, u8p, C.c_size_t, vp, C.c_size_t, u8p, C.c_size_t]
        L.bsa_diagdp_last_ms.argtypes = [vp]
        L.bsa_diagdp_last_ms.restype = C.c_double
        L.bsa_env_reload.restype = None
        _lib = L
    _sync_env()
    return _lib


_env_seen = None


def _sync_env():
    """the library reads its BSA_* knobs once; a test that flips one inside this process gets a fresh snapshot"""
    global _env_seen
    cur = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("BSA_")))
    if cur != _env_seen:
        _lib.bsa_env_reload()
        _env_seen = cur


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def make_params(mode=MODE_GLOBAL, bandwidth=128, M=2, X=-6, O=-3, E=-2, Q=0, P=0, matrix=None):
    p = AlignParams()
    p.mode, p.bandwidth = mode, bandwidth
    if matrix is None:
        lib().bsa_set_score_matrix(p.matrix, M, X)
    else:
        for i in range(16):
            p.matrix[i] = int(matrix[i])
    p.gapo1, p.gape1, p.gapo2, p.gape2 = O, E, Q, P
    return p


def align8_abs_form(par):
    """what the 8-bit forward launcher decides for a scoring at par.bandwidth 128 or 256 (bsa_align8_abs_rows; host only): (form, rows) with form -1 = not
    taken by the exact-arithmetic kernel, 0 = difference form, 1 = absolute scores with integer maxima, 2 = with three-operand maxima in the biased frame,
    and rows the rebase period"""
    rows = C.c_uint32(0)
    form = lib().bsa_align8_abs_form_internal(C.byref(par), C.byref(rows))
    return int(form), int(rows.value)


def align8_row_target(a, tlen, qlen, stride=4, steps=0):
    """the row target of global steering as the absolute-score forward DP forms it in integers (bsa_align8_row_target_internal; host only), for uint32 arrays of
    rows a < tlen: (value int32, fallback bool), fallback where the row asks the reference's double expression (a * qlen divides by tlen, or qlen * tlen >= 2**52 or
    a length of 2**31 and more: outside the bound of the integer form's proof).  steps > 0: the state is
    taken by division up to `steps` strides in front of the row and stepped to it, as the kernels do"""
    import numpy as np
    a, tlen, qlen = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, tlen, qlen))
    assert a.shape == tlen.shape == qlen.shape and a.ndim == 1
    value, fb = np.empty(len(a), np.int32), np.empty(len(a), np.uint8)
    u32p = C.POINTER(C.c_uint32)
    rc = lib().bsa_align8_row_target_internal(a.ctypes.data_as(u32p), tlen.ctypes.data_as(u32p), qlen.ctypes.data_as(u32p), len(a), stride, steps,
                                              value.ctypes.data_as(C.POINTER(C.c_int32)), fb.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise ValueError("align8_row_target: a row outside its target or a target of length 0")
    return value, fb.astype(bool)


FLAG_SPAN_TERMS = ("M: f - d", "D: d - E", "D: f - E", "D: d - E, row -1", "D: f - E, row -1", "R, Od")


def align8_flag_span(par):
    """largest difference a one-bit flag insert of the absolute-score forward DP sees in a stored cell, for a scoring at par.bandwidth (bsa_align8_flag_span;
    host only): (span, terms) with terms the FLAG_SPAN_TERMS it is the maximum of; span 0 = the difference form, -1 = not taken by the exact-arithmetic kernel"""
    terms = (C.c_uint32 * len(FLAG_SPAN_TERMS))()
    span = lib().bsa_align8_flag_span_internal(C.byref(par), terms)
    return int(span), tuple(int(v) for v in terms)


X_CHOICE_FIELDS = ("form", "W", "L", "pw", "do2", "score", "abs", "m3", "wps", "rebase_rows", "grid", "groups", "nseg", "seg_rows", "spin_cap", "rmask", "ctl_bytes",
                   "state_bytes", "n8", "nb8", "gap_model", "xq_need")
X_NONE, X_STATIC, X_SEG, X_WHOLE, X_MIX = range(5)


def align8_x_choice(par, count, max_tlen, static_band=False, code_fmt=0, score=False, xq_bytes=0, cus=256):
    """what the 8-bit exact-arithmetic forward launcher would launch for a chunk of `count` pairs of par's scoring at par.bandwidth (x_choose; host only, under the
    BSA_ALIGN8_* knobs as they stand): a dict of X_CHOICE_FIELDS plus "name" and "launch" (False: the launcher returns an error); xq_need is what bsa_align_run
    sizes the row-segment buffer to"""
    out = (C.c_uint64 * len(X_CHOICE_FIELDS))()
    name = C.create_string_buffer(400)
    rc = lib().bsa_align8_x_choice_internal(C.byref(par), count, max_tlen, int(static_band), code_fmt, int(score), xq_bytes, cus, out, name, len(name))
    if rc < 0:
        raise ValueError("bsa_align8_x_choice_internal: bad arguments")
    d = dict(zip(X_CHOICE_FIELDS, (int(v) for v in out)))
    d.update(name=name.value.decode(), launch=rc == 1)
    return d


TRACE_CHOICE_FIELDS = ("form", "W", "fmt", "lanes", "pairs_per_block", "grid")
TR_NONE, TR_WAVE, TR_LDS, TR_SIMPLE, TR_CODES2, TR_CODES2_WAVE = range(6)


def align8_trace_choice(bw, pw, code_fmt, count, cus=256):
    """what the traceback launcher of the compact path would launch for a chunk of `count` pairs at bandwidth bw with gap model pw (0 linear, 1 affine, 2 two
    pieces) over slots of code format code_fmt (trace_choose; host only, under the BSA_ALIGN8_TRACE_* knobs as they stand): a dict of TRACE_CHOICE_FIELDS
    (lanes: pairs per wave of the LDS walker, else 0) plus "name" and "launch" (False: the launcher returns an error)"""
    out = (C.c_uint64 * len(TRACE_CHOICE_FIELDS))()
    name = C.create_string_buffer(200)
    rc = lib().bsa_align8_trace_choice_internal(bw, pw, code_fmt, count, cus, out, name, len(name))
    if rc < 0:
        raise ValueError("bsa_align8_trace_choice_internal: bad arguments")
    d = dict(zip(TRACE_CHOICE_FIELDS, (int(v) for v in out)))
    d.update(name=name.value.decode(), launch=rc == 1)
    return d


EDIT_CHOICE_FIELDS = tuple("fwd%d_%s" % (i, f) for i in (0, 1) for f in ("form", "n", "tiled", "track", "lanes", "grid", "block")) \
    + ("trace_form", "trace_tiled", "trace_lanes", "trace_grid", "row_fmt")
E_NONE, E_REG, E_GRP, E_GRP32, E_WIDE, E_GEN = range(6)
T_NONE, T_WAVE, T_PLAIN, T_COOP = range(4)


def edit_choice(bw, wide, count, mode=MODE_GLOBAL, bandwidth=0, score=False, alone=True, cus=256, occ_plain=8, occ_coop=8):
    """what the edit launchers would launch for a launch class of `count` pairs (edit_choose; host only, under the BSA_EDIT_* knobs as they stand): a band of bw
    columns, or bw 0 and the class's words per lane `wide`; alone: the class fills its chunk; occ_plain / occ_coop: the waves of k_edit_trace<false> / <true> a
    CU keeps.  A dict of EDIT_CHOICE_FIELDS (fwd1_*: the generic kernel beside the wave-per-pair one) plus "fwd_name", "trace_name" and "launch"."""
    out = (C.c_uint64 * len(EDIT_CHOICE_FIELDS))()
    fwd, trace = C.create_string_buffer(200), C.create_string_buffer(200)
    rc = lib().bsa_edit_choice_internal(bw, wide, count, mode, bandwidth, int(score), int(alone), cus, occ_plain, occ_coop, out, fwd, trace, 200)
    if rc < 0:
        raise ValueError("bsa_edit_choice_internal: bad arguments")
    d = dict(zip(EDIT_CHOICE_FIELDS, (int(v) for v in out)))
    d.update(fwd_name=fwd.value.decode(), trace_name=trace.value.decode(), launch=rc == 1)
    return d


def seq16(blob, off, length, i, packed=False, rev=0, padcode=0):
    """the sixteen staged codes of positions [i, i + 16) of the sequence of `length` bases at `off` of `blob`, as every staging kernel reads them
    (bsa_seq16_internal: the host side of the kernels' reader; no device).  blob: uint8 codes and a byte offset, or (packed) uint64 BSA_MODE_SEQ2BIT
    words and a base offset; rev: 0 forwards, 1 the reverse complement, 2 forwards as a plan with MODE_QSTRAND reads an unmarked query.
    -> (uint8[16], whether a code above 3 was met)"""
    b = np.ascontiguousarray(blob, dtype=np.uint64 if packed else np.uint8)
    out, bad = np.zeros(16, dtype=np.uint8), C.c_uint32(0)
    rc = lib().bsa_seq16_internal(C.c_void_p(b.ctypes.data), off, length, i, int(packed), rev, padcode, out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(bad))
    if rc != 0:
        raise ValueError("bsa_seq16_internal: bad arguments")
    return out, bool(bad.value)


def pack2bit(codes):
    """codes (one base per byte) -> uint64 words in the BSA_MODE_SEQ2BIT layout (the reference's BaseBank.bits): base i at bits
    62 - 2 (i % 32) of word i / 32, each code taken as c & 3, the bits behind the last base zero"""
    c = np.ascontiguousarray(codes, dtype=np.uint8).ravel()
    nw = (c.size + 31) // 32
    buf = np.zeros(nw * 32, dtype=np.uint64)
    buf[:c.size] = c & 3
    shift = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
    return np.bitwise_or.reduce(buf.reshape(nw, 32) << shift, axis=1).astype(np.uint64)


def unpack2bit(words, off, n):
    """bases [off, off + n) of BSA_MODE_SEQ2BIT words -> uint8 codes"""
    i = np.uint64(off) + np.arange(n, dtype=np.uint64)
    w = np.asarray(words, dtype=np.uint64)[(i >> np.uint64(5)).astype(np.intp)]
    return ((w >> (np.uint64(62) - np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3)).astype(np.uint8)


def revcomp(codes):
    """the reverse complement of base codes (A 0, C 1, G 2, T 3): out[i] = 3 - codes[len - 1 - i], what BSA_MODE_QSTRAND aligns for a
    marked query.  Codes above 3 are not bases: they come back as (3 - c) mod 256, above 3 as well."""
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    return (np.uint8(3) - c[::-1]).astype(np.uint8)


def pack_pairs(pairs, seq2bit=False, strands=None, lead=3):
    """[(q, t), ...] of uint8 code arrays -> (seqs blob, qoff, qlen, toff, tlen).
    seq2bit: the blob is uint64 words (pack2bit) and the offsets are base offsets; the sequences start `lead` bases into the first word
    and have 3 bases between them, so that they start at every position in a word, as a caller's reads do (the last one ends in the last word).
    strands (a bool per pair, BSA_MODE_QSTRAND): every query is stored once, forward, as given; where strands[k] is true QOFF_REVCOMP
    is OR-ed into qoff[k] -- the call then aligns revcomp(q) for that pair."""
    if strands is not None:
        if len(strands) != len(pairs):
            raise ValueError("pack_pairs: one strand per pair")
        seqs, qoff, qlen, toff, tlen = pack_pairs(pairs, seq2bit, None, lead)
        qoff = qoff | np.where(np.asarray(strands, dtype=bool), np.uint64(QOFF_REVCOMP), np.uint64(0)).astype(np.uint64)
        return seqs, qoff, qlen, toff, tlen
    if seq2bit:
        n = len(pairs)
        qlen = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
        tlen = np.array([len(t) for _, t in pairs], dtype=np.uint32)
        qoff = np.zeros(n, dtype=np.uint64)
        toff = np.zeros(n, dtype=np.uint64)
        gap = np.zeros(3, dtype=np.uint8)
        parts, acc = [np.zeros(lead, dtype=np.uint8)], lead
        for k, (q, t) in enumerate(pairs):
            qoff[k] = acc
            parts += [_np(q, np.uint8), gap]
            acc += len(q) + 3
            toff[k] = acc
            parts += [_np(t, np.uint8)] + ([gap] if k + 1 < n else [])
            acc += len(t) + (3 if k + 1 < n else 0)
        words = pack2bit(np.concatenate(parts))
        return (words if words.size else np.zeros(1, dtype=np.uint64)), qoff, qlen, toff, tlen
    n = len(pairs)
    qlen = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
    tlen = np.array([len(t) for _, t in pairs], dtype=np.uint32)
    qoff = np.zeros(n, dtype=np.uint64)
    toff = np.zeros(n, dtype=np.uint64)
    parts, acc = [], 0
    for k, (q, t) in enumerate(pairs):
        qoff[k] = acc
        parts.append(_np(q, np.uint8))
        acc += len(q)
        toff[k] = acc
        parts.append(_np(t, np.uint8))
        acc += len(t)
    seqs = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    if seqs.size == 0:
        seqs = np.zeros(1, dtype=np.uint8)
    return seqs, qoff, qlen, toff, tlen


def expand_eqx(words, q, t, qb=0, tb=0):
    """the BSA_MODE_CIGAR_EQX form of a plain CIGAR (include/bsalign_hip.h): every M word replaced, in place, by the maximal runs of
    CIGAR_EQ and CIGAR_X over its columns -- column j of an M word that starts at query position qp and target position tp is = when
    q[qp + j] == t[tp + j].  Positions start at the record's qb, tb; M / = / X consume a base of both, I a query base, D a target base.
    Pure numpy; words: uint32 (len << 4 | op)."""
    q = np.asarray(q, dtype=np.uint8)
    t = np.asarray(t, dtype=np.uint8)
    out = []
    qp, tp = int(qb), int(tb)
    for w in np.asarray(words, dtype=np.uint32).tolist():
        op, ln = w & 15, w >> 4
        if op == CIGAR_M and ln:
            mis = q[qp:qp + ln] != t[tp:tp + ln]
            if len(mis) != ln:
                raise ValueError("expand_eqx: an M word runs past the end of a sequence")
            cut = np.flatnonzero(mis[1:] != mis[:-1]) + 1
            edges = np.concatenate([[0], cut, [ln]])
            for a, b in zip(edges[:-1].tolist(), edges[1:].tolist()):
                out.append(((b - a) << 4) | (CIGAR_X if mis[a] else CIGAR_EQ))
        else:
            out.append(w)
        if op in (CIGAR_M, CIGAR_EQ, CIGAR_X):
            qp += ln
            tp += ln
        elif op == CIGAR_I:
            qp += ln
        elif op == CIGAR_D:
            tp += ln
    return np.array(out, dtype=np.uint32)


def collapse_eqx(words):
    """every run of neighbouring = / X words merged back into one M word: the plain CIGAR of the same alignment"""
    out = []
    run = 0
    for w in np.asarray(words, dtype=np.uint32).tolist():
        if (w & 15) in (CIGAR_EQ, CIGAR_X):
            run += w >> 4
            continue
        if run:
            out.append((run << 4) | CIGAR_M)
            run = 0
        out.append(w)
    if run:
        out.append((run << 4) | CIGAR_M)
    return np.array(out, dtype=np.uint32)


DIAGDP_WALK_DTYPE = np.dtype([("nsteps", "<u4"), ("score", "<i4"), ("xi", "<i4"), ("yi", "<i4"), ("status", "<u4"), ("reserved", "<u4"), ("first_word", "<u8")])


class Context:
    """one context per (thread, device) -- bsa_ctx_create / bsa_ctx_destroy"""

    def __init__(self, device=0, workspace_limit=0):
        h = C.c_void_p()
        rc = lib().bsa_ctx_create(device, C.byref(h))
        if rc != 0:
            raise BsaError(rc, "bsa_ctx_create: no usable GPU; this library has no CPU fallback")
        self.h = h
        self._models = []
        if workspace_limit:
            lib().bsa_ctx_set_workspace_limit(self.h, workspace_limit)

    def close(self):
        if self.h:
            for m in getattr(self, "_models", []):              # (a model is closed with its context)
                m.close()
            self._models = []
            lib().bsa_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise BsaError(rc, (lib().bsa_last_error(self.h) or b"").decode())

    def set_stream(self, stream_ptr):
        self._chk(lib().bsa_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def sync(self):
        self._chk(lib().bsa_ctx_sync(self.h))

    def last_kernel_ms(self):
        ms, n, cells = C.c_double(), C.c_long(), C.c_double()
        self._chk(lib().bsa_ctx_last_kernel_ms(self.h, C.byref(ms), C.byref(n), C.byref(cells)))
        return ms.value, n.value, cells.value

    def last_trace_ms(self):
        ms, n = C.c_double(), C.c_long()
        self._chk(lib().bsa_ctx_last_trace_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_margin_ms(self):
        """average duration of the BSA_MODE_BAND_MARGIN pass's launches in the last run (0 launches without the flag)"""
        ms, n = C.c_double(), C.c_long()
        self._chk(lib().bsa_ctx_last_margin_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_handover(self):
        """pairs of the last align_batch call that were re-run through the literal kernels"""
        return int(lib().bsa_ctx_last_handover(self.h))

    def last_kernel_names(self):
        return lib().bsa_ctx_last_kernel_name(self.h, 0).decode(), lib().bsa_ctx_last_kernel_name(self.h, 1).decode()

    def _batch(self, fn, pairs, par, cigar_cap=None, seq2bit=False, strands=None):
        seqs, qoff, qlen, toff, tlen = pack_pairs(pairs, seq2bit, strands)
        n = len(pairs)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        if cigar_cap is None:
            cigar_cap = int(qlen.sum() + tlen.sum()) + 2 * n + 16
        cig = np.zeros(cigar_cap, dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        rc = fn(self.h, _p(seqs), seqs.nbytes, _p(qoff), _p(qlen), _p(toff), _p(tlen), n, C.byref(par),
                _p(out), _p(cig), cigar_cap, _p(off), _p(status))
        self._chk(rc)
        cigs = [cig[int(off[k]):int(off[k + 1])].copy() for k in range(n)]
        return out, cigs, status[:n]

    def align_batch(self, pairs, par, cigar_cap=None, seq2bit=False, eqx=False, strands=None, margins=False):
        """host-pointer form of bsa_align_batch: returns (results, [cigar arrays], status); seq2bit: the sequences go down
        2-bit packed (pack_pairs(..., seq2bit=True), BSA_MODE_SEQ2BIT OR-ed into par.mode); eqx: BSA_MODE_CIGAR_EQX OR-ed in,
        the CIGARs come back with = / X words (the default cigar_cap holds them: a word covers at least one column); strands (a bool
        per pair): BSA_MODE_QSTRAND OR-ed in, the queries go down as given and pair k aligns revcomp(q) where strands[k] is true;
        margins: BSA_MODE_BAND_MARGIN OR-ed in, returns (results, [cigar arrays], status, margins) -- the band margins as a uint16 array of
        their own (ST_MARGIN_NONE where no band edge constrained the path) beside the status masked to its low half"""
        if seq2bit or eqx or strands is not None or margins:
            par = AlignParams.from_buffer_copy(par)
            par.mode |= (MODE_SEQ2BIT if seq2bit else 0) | (MODE_CIGAR_EQX if eqx else 0) | (MODE_QSTRAND if strands is not None else 0) | (MODE_BAND_MARGIN if margins else 0)
        out, cigs, status = self._batch(lib().bsa_align_batch, pairs, par, cigar_cap, seq2bit, strands)
        if margins:
            return out, cigs, status & np.uint32(0xFFFF), (status >> np.uint32(ST_MARGIN_SHIFT)).astype(np.uint16)
        return out, cigs, status

    def align_scores(self, pairs, par, seq2bit=False, strands=None):
        """bsa_align_batch with BSA_MODE_SCORE_ONLY OR-ed into par.mode and no CIGAR arena: returns (results, status); score, qe and te as
        align_batch returns them, the fields only a traceback finds are -1; strands as in align_batch"""
        sp = AlignParams.from_buffer_copy(par)
        sp.mode = par.mode | MODE_SCORE_ONLY | (MODE_SEQ2BIT if seq2bit else 0) | (MODE_QSTRAND if strands is not None else 0)
        seqs, qoff, qlen, toff, tlen = pack_pairs(pairs, seq2bit, strands)
        n = len(pairs)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        self._chk(lib().bsa_align_batch(self.h, _p(seqs), seqs.nbytes, _p(qoff), _p(qlen), _p(toff), _p(tlen), n, C.byref(sp),
                                        _p(out), None, 0, None, _p(status)))
        return out, status[:n]

    def sweep_host(self, tasks, progs, queries, qoff, qlen, par, nblocks, want_rows=True):
        """host-pointer form of the POA sweep (bsa_sweep_host): tasks ROW_TASK_DTYPE, progs SWEEP_PROG_DTYPE,
        queries one base per byte; returns (row blocks as uint8 [nblocks * block_bytes] or None, results)"""
        L = lib()
        tasks = np.ascontiguousarray(tasks, dtype=ROW_TASK_DTYPE)
        progs = np.ascontiguousarray(progs, dtype=SWEEP_PROG_DTYPE)
        queries = np.ascontiguousarray(queries, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        qlen = np.ascontiguousarray(qlen, dtype=np.uint32)
        r = par.rows
        blk = L.bsa_rows_block_bytes(r.bandwidth, r.gapo1, r.gape1, r.gapo2, r.gape2)
        rows = np.zeros(nblocks * blk, dtype=np.uint8) if want_rows else None
        res = np.zeros(len(progs), dtype=SWEEP_RESULT_DTYPE)
        rc = L.bsa_sweep_host(self.h, tasks.ctypes.data, len(tasks), progs.ctypes.data, len(progs), queries.ctypes.data,
                              qoff.ctypes.data, qlen.ctypes.data, len(qlen), C.byref(par),
                              rows.ctypes.data if want_rows else None, nblocks, res.ctypes.data)
        self._chk(rc)
        return rows, res

    def poa_graph_host(self, nodes, edges, cands, progs, queries, par, events_cap, want_rows=False):
        """host-pointer form of the wavefront sweep + device traceback (bsa_poa_graph_host): nodes POA_NODE_DTYPE, edges
        POA_EDGE_DTYPE, cands POA_CAND_DTYPE, progs POA_PROG_DTYPE, queries one base per byte.
        -> (results POA_RESULT_DTYPE, events POA_EVENT_DTYPE [events_cap], rows POA_CELL_DTYPE [nnodes, bw] or None, u0 or None)"""
        L = lib()
        nodes = np.ascontiguousarray(nodes, dtype=POA_NODE_DTYPE); edges = np.ascontiguousarray(edges, dtype=POA_EDGE_DTYPE)
        cands = np.ascontiguousarray(cands, dtype=POA_CAND_DTYPE); progs = np.ascontiguousarray(progs, dtype=POA_PROG_DTYPE)
        queries = np.ascontiguousarray(queries, dtype=np.uint8)
        bw = (par.rows.bandwidth + 15) // 16 * 16
        res = np.zeros(len(progs), dtype=POA_RESULT_DTYPE)
        ev = np.zeros(max(events_cap, 1), dtype=POA_EVENT_DTYPE)
        rows = np.zeros((len(nodes), bw), dtype=POA_CELL_DTYPE) if want_rows else None
        u0 = np.zeros(len(nodes), dtype=np.int32) if want_rows else None
        rc = L.bsa_poa_graph_host(self.h, nodes.ctypes.data, len(nodes), edges.ctypes.data, len(edges), cands.ctypes.data, len(cands),
                                  progs.ctypes.data, len(progs), queries.ctypes.data, queries.size, C.byref(par), res.ctypes.data, ev.ctypes.data, events_cap,
                                  rows.ctypes.data if want_rows else None, u0.ctypes.data if want_rows else None)
        self._chk(rc)
        return res, ev, rows, u0

    def diagdp_batch(self, planes, probs, matrix_bytes):
        """anti-diagonal u8 DP of the MSA refinement (bsa_diagdp_batch): planes = uint8 blob in the reference's layout,
        probs = DIAGDP_PROB_DTYPE array; returns the matrix buffer (uint8, rows outside 2 mbeg .. 2 mend - 1 zero)"""
        L = lib()
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        probs = np.ascontiguousarray(probs, dtype=DIAGDP_PROB_DTYPE)
        matrix = np.zeros(matrix_bytes, dtype=np.uint8)
        self._chk(L.bsa_diagdp_batch(self.h, planes.ctypes.data, planes.size, probs.ctypes.data, len(probs), matrix.ctypes.data, matrix.size))
        return matrix

    def diagdp_walk_batch(self, planes, probs):
        """the same DP followed by the traceback on the device (bsa_diagdp_walk_batch): no matrix comes back.
        -> (walk records, list of uint8 step arrays: 0 diagonal, 1 x - 1, 2 y - 1)"""
        L = lib()
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        probs = np.ascontiguousarray(probs, dtype=DIAGDP_PROB_DTYPE)
        n = len(probs)
        walks = np.zeros(n, dtype=DIAGDP_WALK_DTYPE)
        cap = int(sum((2 * (int(p["mend"]) - int(p["mbeg"])) + 2 + 15) // 16 for p in probs)) + 1
        words = np.zeros(cap, dtype=np.uint32)
        L.bsa_diagdp_walk_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
        self._chk(L.bsa_diagdp_walk_batch(self.h, planes.ctypes.data, planes.size, probs.ctypes.data, n, walks.ctypes.data, words.ctypes.data, cap))
        steps = []
        for k in range(n):
            ns, fw = int(walks[k]["nsteps"]), int(walks[k]["first_word"])
            w = words[fw:fw + (ns + 15) // 16]
            st = ((w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).astype(np.uint8).reshape(-1)[:ns]
            steps.append(st)
        return walks, steps

    def diagdp_last_ms(self):
        return float(lib().bsa_diagdp_last_ms(self.h))

    def edit_batch(self, pairs, mode=MODE_GLOBAL, bandwidth=0, cigar_cap=None, seq2bit=False, eqx=False, strands=None):
        """host-pointer form of bsa_edit_batch; seq2bit / eqx / strands as in align_batch"""
        p = EditParams()
        p.mode = mode | (MODE_SEQ2BIT if seq2bit else 0) | (MODE_CIGAR_EQX if eqx else 0) | (MODE_QSTRAND if strands is not None else 0)
        p.bandwidth = bandwidth
        return self._batch(lib().bsa_edit_batch, pairs, p, cigar_cap, seq2bit, strands)

    def edit_scores(self, pairs, mode=MODE_GLOBAL, bandwidth=0, seq2bit=False, strands=None):
        """bsa_edit_batch with BSA_MODE_SCORE_ONLY OR-ed into the mode and no CIGAR arena: returns (results, status); score, qe and te as
        edit_batch returns them, the fields only a traceback finds are -1; strands as in align_batch"""
        p = EditParams()
        p.mode, p.bandwidth = mode | MODE_SCORE_ONLY | (MODE_SEQ2BIT if seq2bit else 0) | (MODE_QSTRAND if strands is not None else 0), bandwidth
        seqs, qoff, qlen, toff, tlen = pack_pairs(pairs, seq2bit, strands)
        n = len(pairs)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        self._chk(lib().bsa_edit_batch(self.h, _p(seqs), seqs.nbytes, _p(qoff), _p(qlen), _p(toff), _p(tlen), n, C.byref(p),
                                       _p(out), None, 0, None, _p(status)))
        return out, status[:n]

    def seq_pack2bit(self, d_codes, d_bits, d_bad=None):
        """bsa_seq_pack2bit on torch tensors: d_codes (uint8, one base per byte) -> d_bits (int64 / uint64, at least
        ceil(n / 32) elements) in the BSA_MODE_SEQ2BIT layout; d_bad (int32, one element, cleared by the caller) is set to 1 when a
        code is above 3.  Asynchronous on the context's stream."""
        n = d_codes.numel()
        if d_bits.numel() * d_bits.element_size() < (n + 31) // 32 * 8:
            raise ValueError("seq_pack2bit: d_bits holds fewer than ceil(n / 32) words")
        self._chk(lib().bsa_seq_pack2bit(self.h, C.c_void_p(d_codes.data_ptr()), n, C.c_void_p(d_bits.data_ptr()),
                                         C.c_void_p(d_bad.data_ptr() if d_bad is not None else 0)))

    def kmer_edit_batch(self, pairs, ksz=13, threads=0, cigar_cap=None, device_chain=False, seq2bit=False, strands=None, auto_strand=False):
        """k-mer anchored edit alignment (the reference's kmer_striped_seqedit_pairwise, bsalign.h:1209) of a batch;
        device_chain: the anchors come from the device chainer (bsa_kmer_edit_batch2 with KMER_CHAIN_DEVICE), same results;
        seq2bit / strands as in edit_batch (bsa_kmer_edit_batch2 with MODE_SEQ2BIT / MODE_QSTRAND in its flags): the queries are stored as
        given and pair k aligns revcomp(q) where strands[k] is true.  auto_strand (KMER_STRAND_AUTO, not together with strands): the call finds
        every pair's strand -- reverse where revcomp(q) chains to more anchors than q -- and status & ST_REVCOMP says which pairs aligned revcomp(q)"""
        if auto_strand and strands is not None:
            raise ValueError("kmer_edit_batch: auto_strand finds the strands itself, strands= gives them: pass one of the two")
        p = KmerParams()
        p.ksz, p.threads = ksz, threads
        flags = (KMER_CHAIN_DEVICE if device_chain else 0) | (MODE_SEQ2BIT if seq2bit else 0) | (MODE_QSTRAND if strands is not None else 0) | (KMER_STRAND_AUTO if auto_strand else 0)
        if not flags:
            return self._batch(lib().bsa_kmer_edit_batch, pairs, p, cigar_cap)
        fn = lib().bsa_kmer_edit_batch2
        return self._batch(lambda *a: fn(*a, flags), pairs, p, cigar_cap, seq2bit, strands)

    def kmer_chain_batch(self, pairs, ksz=13, with_status=False, seq2bit=False, strands=None, auto_strand=False):
        """bsa_kmer_chain_batch: the anchors of every pair (query offset << 32 | target offset, in query order) as a list of uint64 arrays,
        chained on the device; with_status: (anchors, status) -- ST_EMPTY / ST_BAD_BASE pairs have none.  seq2bit / strands as in edit_batch
        (bsa_kmer_chain_batch2): where strands[k] is true the anchors are those of revcomp(q) against t, query offsets in revcomp(q).
        auto_strand (KMER_STRAND_AUTO, not together with strands): the call finds every pair's strand and additionally returns them as a bool
        array (from ST_REVCOMP, which is masked out of the status): (anchors, strands) or (anchors, status, strands)"""
        if auto_strand and strands is not None:
            raise ValueError("kmer_chain_batch: auto_strand finds the strands itself, strands= gives them: pass one of the two")
        seqs, qoff, qlen, toff, tlen = pack_pairs(pairs, seq2bit, strands)
        n = len(pairs)
        cap = int(np.minimum(qlen, tlen).sum()) + 1
        maps = np.zeros(cap, dtype=np.uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        flags = (MODE_SEQ2BIT if seq2bit else 0) | (MODE_QSTRAND if strands is not None else 0) | (KMER_STRAND_AUTO if auto_strand else 0)
        if flags:
            self._chk(lib().bsa_kmer_chain_batch2(self.h, _p(seqs), seqs.nbytes, _p(qoff), _p(qlen), _p(toff), _p(tlen), n, ksz,
                                                  _p(maps), cap, _p(off), _p(status), flags))
        else:
            self._chk(lib().bsa_kmer_chain_batch(self.h, _p(seqs), seqs.nbytes, _p(qoff), _p(qlen), _p(toff), _p(tlen), n, ksz,
                                                 _p(maps), cap, _p(off), _p(status)))
        res = [maps[int(off[k]):int(off[k + 1])].copy() for k in range(n)]
        if auto_strand:
            found = (status[:n] & np.uint32(ST_REVCOMP)) != 0
            status = status & ~np.uint32(ST_REVCOMP)
            return (res, status[:n], found) if with_status else (res, found)
        return (res, status[:n]) if with_status else res

    def last_kmer_chain_ms(self):
        """(kernel ms, pairs chained on the device, pairs chained on the host) of the last kmer_chain_batch / kmer_edit_batch(device_chain=True),
        or of the last KmerChainPlan.run (waits for that run's last chunk)"""
        ms, a, b = C.c_double(), C.c_long(), C.c_long()
        self._chk(lib().bsa_ctx_last_kmer_chain_ms(self.h, C.byref(ms), C.byref(a), C.byref(b)))
        return ms.value, a.value, b.value

    def cigar_windows(self, results, cigars, window):
        """bsa_cigar_windows_batch on what align_batch / edit_batch return (the record array and the list of CIGAR arrays): every alignment
        cut at the borders of windows of `window` target bases.  Returns a list of (nw, 4) uint32 arrays, row r of pair k = (t_first, q_first,
        t_last, q_last) of window results[k]["tb"] // window + r, all four WINDOW_NONE where the window holds no aligned column."""
        n = len(cigars)
        out = _np(results, RESULT_DTYPE)
        if len(out) != n:
            raise ValueError("cigar_windows: one CIGAR per record")
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c in cigars], dtype=np.uint64)
        cig = _np(np.concatenate([np.zeros(0, np.uint32)] + [_np(c, np.uint32) for c in cigars]), np.uint32)
        window = int(window)
        # the records needed, from the definition: (te - 1) // w - tb // w + 1 for a pair with tb >= 0, te > tb and words
        tb, te = out["tb"].astype(np.int64), out["te"].astype(np.int64)
        has = (tb >= 0) & (te > tb) & (np.diff(off.astype(np.int64)) > 0)
        cap = int(np.where(has, (te - 1) // max(window, 1) - tb // max(window, 1) + 1, 0).sum())
        win = np.zeros((max(cap, 1), 4), dtype=np.uint32)
        woff = np.zeros(n + 1, dtype=np.uint64)
        self._chk(lib().bsa_cigar_windows_batch(self.h, _p(out), _p(cig) if len(cig) else None, _p(off), n, window, _p(win), cap, _p(woff)))
        return [win[int(woff[k]):int(woff[k + 1])].copy() for k in range(n)]

    def cigar_windows_run(self, d_out, d_cigar, d_cigar_off, n, window, d_win, win_cap, d_win_off):
        """bsa_cigar_windows_run on torch tensors (plumbing only), asynchronous on the context's stream: d_out, d_cigar, d_cigar_off as a complete
        AlignPlan.run / EditPlan.run left them; d_win: room for win_cap records of 16 bytes, or None with win_cap 0 for a count-only run;
        d_win_off: n + 1 64-bit words.  Pair k's records are d_win[d_win_off[k] : d_win_off[k + 1]] where d_win_off[k + 1] <= win_cap;
        d_win_off[n] is the number of records a complete run needs (cigar_windows_bound always suffices)."""
        if d_win is not None and d_win.numel() * d_win.element_size() < 16 * win_cap:
            raise ValueError("cigar_windows_run: d_win holds fewer than win_cap records")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_cigar_windows_run(self.h, ptr(d_out), ptr(d_cigar), ptr(d_cigar_off), n, int(window), ptr(d_win), win_cap, ptr(d_win_off)))

    def window_pieces(self, pairs, windows, window, gbase, nwin, seq2bit=False, strands=None):
        """bsa_window_pieces_batch on the pairs an align_batch / edit_batch call took and what Context.cigar_windows made of its results (the
        per-pair (nw, 4) arrays): the window records turned window-major, with the reads' bases.  The blob is packed exactly as align_batch packs
        it (pack_pairs; seq2bit / strands as there), gbase and nwin as from window_gbase.  Returns a list over the nwin windows of
        (pieces, codes): pieces a PIECE_DTYPE array in ascending record order, codes a list of uint8 arrays, codes[j] = q'[q_first : q_first + len)
        of pieces[j] -- the strand that was aligned, one base a byte."""
        n = len(pairs)
        if len(windows) != n:
            raise ValueError("window_pieces: one window array per pair")
        seqs, qoff, qlen, _, _ = pack_pairs(pairs, seq2bit, strands)
        flags = (MODE_SEQ2BIT if seq2bit else 0) | (MODE_QSTRAND if strands is not None else 0)
        gbase = _np(gbase, np.uint64)
        if len(gbase) != n:
            raise ValueError("window_pieces: one gbase per pair")
        window, nwin = int(window), int(nwin)
        woff = np.zeros(n + 1, dtype=np.uint64)
        woff[1:] = np.cumsum([len(x) for x in windows], dtype=np.uint64)
        win = _np(np.concatenate([np.zeros((0, 4), np.uint32)] + [_np(x, np.uint32).reshape(-1, 4) for x in windows]), np.uint32)
        # exact caps, from the definition
        k = np.repeat(np.arange(n), np.diff(woff.astype(np.int64)))
        tf, qf, tl, ql = (win[:, c].astype(np.uint64) for c in range(4))
        gb = gbase[k] if n else np.zeros(0, np.uint64)
        ok = (tf != WINDOW_NONE) & (tf <= tl) & (qf <= ql) & (ql < qlen[k]) & (gb < np.uint64(max(nwin, 0)))
        ok &= np.where(ok, gb, np.uint64(0)) + tf // np.uint64(max(window, 1)) < np.uint64(max(nwin, 0))
        pcap, bcap = int(ok.sum()), int((ql - qf + np.uint64(1))[ok].sum())
        piece = np.zeros(max(pcap, 1), dtype=PIECE_DTYPE)
        bases = np.zeros(max(bcap, 1), dtype=np.uint8)
        poff, boff = np.zeros(nwin + 1, dtype=np.uint64), np.zeros(nwin + 1, dtype=np.uint64)
        self._chk(lib().bsa_window_pieces_batch(self.h, _p(seqs), seqs.nbytes, _p(qoff), _p(qlen), _p(win) if len(win) else None, _p(woff), n, window,
                                                _p(gbase), nwin, flags, _p(piece), pcap, _p(poff), _p(bases), bcap, _p(boff)))
        res = []
        for g in range(nwin):
            ps = piece[int(poff[g]):int(poff[g + 1])].copy()
            res.append((ps, [bases[int(x["base_off"]):int(x["base_off"]) + int(x["len"])].copy() for x in ps]))
        return res

    def window_pieces_run(self, d_seqs, d_qoff, d_qlen, d_win, d_win_off, n, window, d_gbase, nwin, flags, d_piece, piece_cap, d_piece_off,
                          d_bases, bases_cap, d_base_off):
        """bsa_window_pieces_run on torch tensors (plumbing only), asynchronous on the context's stream: d_seqs, d_qoff, d_qlen as the aligner's
        plan took them, d_win, d_win_off as a complete cigar_windows_run left them, d_gbase n 64-bit words; flags: MODE_SEQ2BIT | MODE_QSTRAND as
        in the plan's mode.  d_piece: room for piece_cap records of 32 bytes, d_bases: bases_cap bytes (either None with cap 0: a count-only run);
        d_piece_off, d_base_off: nwin + 1 64-bit words each.  Window g is written where d_piece_off[g + 1] <= piece_cap and
        d_base_off[g + 1] <= bases_cap; the last entries are what a complete run needs."""
        if d_piece is not None and d_piece.numel() * d_piece.element_size() < 32 * piece_cap:
            raise ValueError("window_pieces_run: d_piece holds fewer than piece_cap records")
        if d_bases is not None and d_bases.numel() * d_bases.element_size() < bases_cap:
            raise ValueError("window_pieces_run: d_bases holds fewer than bases_cap bytes")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_window_pieces_run(self.h, ptr(d_seqs), ptr(d_qoff), ptr(d_qlen), ptr(d_win), ptr(d_win_off), n, int(window), ptr(d_gbase),
                                              nwin, int(flags), ptr(d_piece), piece_cap, ptr(d_piece_off), ptr(d_bases), bases_cap, ptr(d_base_off)))

    def window_select_run(self, d_piece, d_piece_off, nwin, piece_cap, d_out, n, par, d_sel, sel_cap, d_sel_off, d_sel_src=None, d_ncand=None):
        """bsa_window_select_run on torch tensors (plumbing only), asynchronous on the context's stream: d_piece, d_piece_off as window_pieces_run
        left them, with room for piece_cap records; d_out the aligner's n records, or None (par.ident_den is then 0); par a SELECT_PARAMS, read at
        the call.  d_sel: room for sel_cap records of 32 bytes, or None with sel_cap 0 for a count-only run; d_sel_off: nwin + 1 64-bit words;
        d_sel_src: sel_cap 32-bit words or None; d_ncand: nwin 32-bit words or None.  Window g's selected records are
        d_sel[d_sel_off[g] : d_sel_off[g + 1]] where d_sel_off[g + 1] <= sel_cap; d_sel_off[nwin] is what a complete run needs."""
        size = lambda t: t.numel() * t.element_size()
        if d_piece is not None and size(d_piece) < 32 * piece_cap:
            raise ValueError("window_select_run: d_piece holds fewer than piece_cap records")
        if d_piece_off is not None and size(d_piece_off) < 8 * (nwin + 1):
            raise ValueError("window_select_run: d_piece_off holds fewer than nwin + 1 offsets")
        if d_out is not None and size(d_out) < 40 * n:
            raise ValueError("window_select_run: d_out holds fewer than n records")
        if d_sel is not None and size(d_sel) < 32 * sel_cap:
            raise ValueError("window_select_run: d_sel holds fewer than sel_cap records")
        if d_sel_off is not None and size(d_sel_off) < 8 * (nwin + 1):
            raise ValueError("window_select_run: d_sel_off holds fewer than nwin + 1 offsets")
        if d_sel_src is not None and size(d_sel_src) < 4 * sel_cap:
            raise ValueError("window_select_run: d_sel_src holds fewer than sel_cap entries")
        if d_ncand is not None and size(d_ncand) < 4 * nwin:
            raise ValueError("window_select_run: d_ncand holds fewer than nwin entries")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_window_select_run(self.h, ptr(d_piece), ptr(d_piece_off), nwin, piece_cap, ptr(d_out), n, C.byref(par), ptr(d_sel), sel_cap,
                                              ptr(d_sel_off), ptr(d_sel_src), ptr(d_ncand)))

    def window_select(self, windows_out, max_depth=0, min_span=0, min_ident=None, results=None, seed=0):
        """bsa_window_select_batch on what Context.window_pieces returned (the list over the windows of (pieces, codes)): the pieces that take part.
        A piece needs min_span target columns or more; with min_ident = (num, den) and results, the aligner's record array, its pair needs
        mat * den >= num * aln; of the candidates left at most max_depth a window are kept (0: all), the widest, ties by mix32(pair ^ seed) and then
        by the index.  Returns (selected, src): selected a list over the windows of (pieces, codes) in the shape Context.piece_cigars and
        Context.window_msa take, src a list of index arrays, src[g][i] the index in windows_out[g] of selected[g]'s piece i."""
        nwin = len(windows_out)
        piece = _np(np.concatenate([np.zeros(0, PIECE_DTYPE)] + [_np(ps, PIECE_DTYPE) for ps, _ in windows_out]), PIECE_DTYPE)
        npiece = len(piece)
        poff = np.zeros(nwin + 1, dtype=np.uint64)
        poff[1:] = np.cumsum([len(ps) for ps, _ in windows_out], dtype=np.uint64)
        par = SELECT_PARAMS(int(max_depth), int(min_span), 0, 0, int(seed))
        out = None
        if min_ident is not None:
            if results is None:
                raise ValueError("window_select: min_ident needs results")
            par.ident_num, par.ident_den = int(min_ident[0]), int(min_ident[1])
            out = _np(results, RESULT_DTYPE)
        sel = np.zeros(max(npiece, 1), dtype=PIECE_DTYPE)
        src = np.zeros(max(npiece, 1), dtype=np.uint32)
        soff = np.zeros(nwin + 1, dtype=np.uint64)
        self._chk(lib().bsa_window_select_batch(self.h, _p(piece) if npiece else None, _p(poff), nwin, npiece, _p(out) if out is not None else None,
                                                len(out) if out is not None else 0, C.byref(par), _p(sel), npiece, _p(soff), _p(src), None))
        selected, idx = [], []
        for g, (ps, cs) in enumerate(windows_out):
            a, b = int(soff[g]), int(soff[g + 1])
            j = src[a:b].astype(np.int64) - int(poff[g])
            selected.append((sel[a:b].copy(), [cs[int(x)] for x in j]))
            idx.append(j)
        return selected, idx

    def piece_cigars(self, results, cigars, windows_out):
        """bsa_piece_cigars_batch on what align_batch / edit_batch returned (the record array and the list of CIGAR arrays) and what
        Context.window_pieces made of them (the list over the windows of (pieces, codes)): every piece's own CIGAR words, the stretch of its pair's
        words from the piece's first to its last aligned column.  Returns a list over the windows of lists of (words, status), one for each piece
        of the window in its order: words a uint32 array, status 0, or PIECE_ST_NOT_ON_PATH and no words for a piece whose ends are not aligned
        columns of its pair (none on what cigar_windows and window_pieces return)."""
        n = len(cigars)
        out = _np(results, RESULT_DTYPE)
        if len(out) != n:
            raise ValueError("piece_cigars: one CIGAR per record")
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c in cigars], dtype=np.uint64)
        cig = _np(np.concatenate([np.zeros(0, np.uint32)] + [_np(c, np.uint32) for c in cigars]), np.uint32)
        piece = _np(np.concatenate([np.zeros(0, PIECE_DTYPE)] + [_np(ps, PIECE_DTYPE) for ps, _ in windows_out]), PIECE_DTYPE)
        npiece = len(piece)
        poff = np.zeros(npiece + 1, dtype=np.uint64)
        status = np.zeros(max(npiece, 1), dtype=np.uint32)
        cap = piece_cigars_bound(off, npiece)                  # enough for pieces that do not overlap; any others say what they need
        for _ in range(2):
            pcig = np.zeros(max(cap, 1), dtype=np.uint32)
            rc = lib().bsa_piece_cigars_batch(self.h, _p(out), _p(cig) if len(cig) else None, _p(off), n, _p(piece) if npiece else None, npiece,
                                              _p(pcig), cap, _p(poff), _p(status))
            if rc != -5 or int(poff[npiece]) <= cap:
                break
            cap = int(poff[npiece])
        self._chk(rc)
        res, j = [], 0
        for ps, _ in windows_out:
            res.append([(pcig[int(poff[i]):int(poff[i + 1])].copy(), int(status[i])) for i in range(j, j + len(ps))])
            j += len(ps)
        return res

    def piece_cigars_run(self, d_out, d_cigar, d_cigar_off, n, d_piece, d_npiece, piece_cap, d_pcig, pcig_cap, d_pcig_off, d_pstatus=None):
        """bsa_piece_cigars_run on torch tensors (plumbing only), asynchronous on the context's stream: d_out, d_cigar, d_cigar_off as a complete
        AlignPlan.run / EditPlan.run left them; d_piece as a complete window_pieces_run left it, with room for piece_cap records; d_npiece: one
        64-bit word on the device, the pieces there are (d_piece_off[nwin:]); d_pcig: room for pcig_cap words, or None with pcig_cap 0 for a
        count-only run; d_pcig_off: piece_cap + 1 64-bit words; d_pstatus: piece_cap 32-bit words or None.  Piece j's words are
        d_pcig[d_pcig_off[j] : d_pcig_off[j + 1]] where d_pcig_off[j + 1] <= pcig_cap; d_pcig_off[piece_cap] is what a complete run needs."""
        if d_pcig is not None and d_pcig.numel() * d_pcig.element_size() < 4 * pcig_cap:
            raise ValueError("piece_cigars_run: d_pcig holds fewer than pcig_cap words")
        if d_pcig_off is not None and d_pcig_off.numel() * d_pcig_off.element_size() < 8 * (piece_cap + 1):
            raise ValueError("piece_cigars_run: d_pcig_off holds fewer than piece_cap + 1 offsets")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_piece_cigars_run(self.h, ptr(d_out), ptr(d_cigar), ptr(d_cigar_off), n, ptr(d_piece), ptr(d_npiece), piece_cap,
                                             ptr(d_pcig), pcig_cap, ptr(d_pcig_off), ptr(d_pstatus)))

    def window_msa(self, windows_out, guides, drafts, window, vote=False, seq2bit=False):
        """bsa_window_msa_batch on what Context.window_pieces returned (the list over the windows of (pieces, codes)), what Context.piece_cigars
        made of it (the list over the windows of lists of (words, status)) and one code array a window, the window's slice of the draft (at most
        `window` bases of it count): every window's draft-anchored MSA.  Returns a list over the windows of (cols, cwin): cols an (mlen, depth + 4)
        uint8 array -- a row of it is one column of the MSA: the depth piece rows, the draft row, the three consensus bytes 4 0 0 -- and cwin the
        window's CNS_WINDOW_DTYPE record, cols_off and out_off counted over the whole call.  vote: the draft row votes too (nseq = depth + 1);
        seq2bit: the drafts go to the device 2-bit packed (the same columns)."""
        nwin = len(windows_out)
        if len(guides) != nwin or len(drafts) != nwin:
            raise ValueError("window_msa: one list of guides and one draft per window")
        piece = _np(np.concatenate([np.zeros(0, PIECE_DTYPE)] + [_np(ps, PIECE_DTYPE) for ps, _ in windows_out]), PIECE_DTYPE).copy()
        poff = np.zeros(nwin + 1, dtype=np.uint64)
        poff[1:] = np.cumsum([len(ps) for ps, _ in windows_out], dtype=np.uint64)
        codes = [_np(c, np.uint8) for _, cs in windows_out for c in cs]
        words = [_np(ws, np.uint32) for gs in guides for ws, _ in gs]
        if len(codes) != len(piece) or len(words) != len(piece):
            raise ValueError("window_msa: one code array and one guide per piece")
        boff = np.zeros(len(piece) + 1, dtype=np.uint64)
        boff[1:] = np.cumsum([len(c) for c in codes], dtype=np.uint64)
        piece["base_off"] = boff[:-1]                           # the codes as they are laid out here
        bases = _np(np.concatenate([np.zeros(0, np.uint8)] + codes), np.uint8)
        pcoff = np.zeros(len(piece) + 1, dtype=np.uint64)
        pcoff[1:] = np.cumsum([len(w) for w in words], dtype=np.uint64)
        pcig = _np(np.concatenate([np.zeros(0, np.uint32)] + words), np.uint32)
        dl = [_np(d, np.uint8) for d in drafts]
        dlen = np.array([len(d) for d in dl], dtype=np.uint32)
        doff = np.zeros(nwin, dtype=np.uint64)
        doff[1:] = np.cumsum(dlen[:-1], dtype=np.uint64)
        draft = _np(np.concatenate([np.zeros(1, np.uint8)] + dl)[1:], np.uint8) if nwin else np.zeros(0, np.uint8)
        if seq2bit:
            draft = pack2bit(draft)
        draft = draft if draft.size else np.zeros(1, np.uint64 if seq2bit else np.uint8)
        coff = np.zeros(nwin + 1, dtype=np.uint64)
        cwin = np.zeros(max(nwin, 1), dtype=CNS_WINDOW_DTYPE)
        cols, cap = np.zeros(1, dtype=np.uint8), 0
        for _ in range(2):                                     # a count-only call says what is needed
            rc = lib().bsa_window_msa_batch(self.h, _p(piece) if len(piece) else None, _p(poff), nwin, len(piece), _p(bases) if len(bases) else None, len(bases),
                                            _p(pcig) if len(pcig) else None, len(pcig), _p(pcoff), _p(draft), _p(doff), _p(dlen), int(window),
                                            MODE_SEQ2BIT if seq2bit else 0, 1 if vote else 0, _p(cols) if cap else None, cap, _p(coff), _p(cwin))
            if rc != -5 or int(coff[nwin]) <= cap:
                break
            cap = int(coff[nwin])
            cols = np.zeros(cap, dtype=np.uint8)
        self._chk(rc)
        res = []
        for g in range(nwin):
            w = cwin[g]
            res.append((cols[int(coff[g]):int(coff[g + 1])].reshape(int(w["mlen"]), int(w["nall"]) + 3).copy(), w.copy()))
        return res

    def window_msa_run(self, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcig_off, d_draft, d_doff, d_dlen,
                       window, flags, vote, d_cols, cols_cap, d_cols_off, d_cwin):
        """bsa_window_msa_run on torch tensors (plumbing only), asynchronous on the context's stream: d_piece, d_piece_off, d_bases as a complete
        window_pieces_run left them, d_pcig, d_pcig_off as a complete piece_cigars_run left them for the same piece_cap; d_draft the draft (1 B/base,
        or 2-bit packed words with MODE_SEQ2BIT in flags), d_doff (64-bit) and d_dlen (32-bit) one entry a window (window_drafts); vote 0 or 1.
        d_cols: room for cols_cap bytes, or None with cols_cap 0 for a count-only run; d_cols_off: nwin + 1 64-bit words; d_cwin: nwin records of
        40 bytes (CNS_WINDOW_DTYPE).  Window g's columns are d_cols[d_cols_off[g] : d_cols_off[g + 1]] where d_cols_off[g + 1] <= cols_cap;
        d_cols_off[nwin] is what a complete run needs."""
        if d_cols is not None and d_cols.numel() * d_cols.element_size() < cols_cap:
            raise ValueError("window_msa_run: d_cols holds fewer than cols_cap bytes")
        if d_cols_off is not None and d_cols_off.numel() * d_cols_off.element_size() < 8 * (nwin + 1):
            raise ValueError("window_msa_run: d_cols_off holds fewer than nwin + 1 offsets")
        if d_cwin is not None and d_cwin.numel() * d_cwin.element_size() < 40 * nwin:
            raise ValueError("window_msa_run: d_cwin holds fewer than nwin records")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_window_msa_run(self.h, ptr(d_piece), ptr(d_piece_off), nwin, piece_cap, ptr(d_bases), bases_cap, ptr(d_pcig), pcig_cap,
                                           ptr(d_pcig_off), ptr(d_draft), ptr(d_doff), ptr(d_dlen), int(window), int(flags), int(vote),
                                           ptr(d_cols), cols_cap, ptr(d_cols_off), ptr(d_cwin)))

    def cns_model(self, par7):
        """bsa_cns_model_create: the consensus model of the seven rates (bsa_cns_params_t: psub pins pdel piex pdex hins hdel) resident on the device,
        for window_cns_run; closed with the context (or by its own close())."""
        m = CnsModel(self, par7)
        self._models.append(m)
        return m

    def window_cns_run(self, model, d_cols, cols_cap, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, d_score=None, d_status=None,
                       d_seq=None, d_seq_qlt=None, d_seq_alt=None, seq_cap=0, d_seq_off=None):
        """bsa_window_cns_run on torch tensors (plumbing only), asynchronous on the context's stream: d_cols and d_cwin as window_msa_run left them,
        cols_cap and out_cap the room of d_cols and of each of d_cns, d_qlt, d_alt; max_rows the largest nseq of the records; d_clen (32-bit),
        d_score (float64) and d_status (32-bit) one entry a window.  With d_seq_off (nwin + 1 64-bit words) the windows' called bases are packed:
        window g's are d_seq[d_seq_off[g] : d_seq_off[g + 1]] where d_seq_off[g + 1] <= seq_cap, likewise d_seq_qlt and d_seq_alt (either may be
        None); d_seq_off[nwin] is what a complete run needs."""
        size = lambda t: t.numel() * t.element_size()
        if d_cols is not None and size(d_cols) < cols_cap:
            raise ValueError("window_cns_run: d_cols holds fewer than cols_cap bytes")
        if d_cwin is not None and size(d_cwin) < 40 * nwin:
            raise ValueError("window_cns_run: d_cwin holds fewer than nwin records")
        if any(t is not None and size(t) < out_cap for t in (d_cns, d_qlt, d_alt)):
            raise ValueError("window_cns_run: an output array holds fewer than out_cap bytes")
        if any(t is not None and size(t) < w * nwin for t, w in ((d_clen, 4), (d_score, 8), (d_status, 4))):
            raise ValueError("window_cns_run: d_clen, d_score or d_status holds fewer than nwin entries")
        if any(t is not None and size(t) < seq_cap for t in (d_seq, d_seq_qlt, d_seq_alt)):
            raise ValueError("window_cns_run: a compact array holds fewer than seq_cap bytes")
        if d_seq_off is not None and size(d_seq_off) < 8 * (nwin + 1):
            raise ValueError("window_cns_run: d_seq_off holds fewer than nwin + 1 offsets")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_window_cns_run(self.h, model.h if model is not None else None, ptr(d_cols), cols_cap, ptr(d_cwin), nwin, int(max_rows),
                                           ptr(d_cns), ptr(d_qlt), ptr(d_alt), out_cap, ptr(d_clen), ptr(d_score), ptr(d_status),
                                           ptr(d_seq), ptr(d_seq_qlt), ptr(d_seq_alt), seq_cap, ptr(d_seq_off)))

    def window_cns(self, msas, par7, max_rows=None):
        """bsa_window_cns_batch on what Context.window_msa returned (the list over the windows of (cols, cwin)): every window's consensus and the
        polished sequence of the call.  Returns (a list over the windows of (cns, qlt, alt, score, status, cols) -- the called bases, both quality
        strings, the log probability of the best path, CNS_ST_*, and the window's columns with their three consensus bytes written --,
        (seq, seq_qlt, seq_alt, seq_off): the windows' called bases and qualities one behind the other, window g's at seq_off[g] : seq_off[g + 1]).
        max_rows: the largest nseq the call accepts (default: the largest of the records)."""
        nwin = len(msas)
        cwin = np.zeros(max(nwin, 1), dtype=CNS_WINDOW_DTYPE)
        parts, cacc, oacc = [], 0, 0
        for g, (cols, rec) in enumerate(msas):
            cols = _np(cols, np.uint8).reshape(-1)
            cwin[g] = (cacc, 0xFFFFFFFFFFFFFFFF, oacc, rec["nall"], rec["nseq"], rec["nmax"], rec["mlen"])
            parts.append(cols)
            cacc += cols.size
            oacc += int(rec["mlen"])
        blob = _np(np.concatenate([np.zeros(0, np.uint8)] + parts), np.uint8).copy()
        if max_rows is None:
            max_rows = int(cwin["nseq"][:nwin].max()) if nwin else 0
        par7 = np.ascontiguousarray(par7, np.float32)
        cns, qlt, alt = (np.zeros(max(oacc, 1), np.uint8) for _ in range(3))
        clen, score, status = np.zeros(max(nwin, 1), np.uint32), np.zeros(max(nwin, 1), np.float64), np.zeros(max(nwin, 1), np.uint32)
        soff = np.zeros(nwin + 1, dtype=np.uint64)
        seq, sq, sa, cap = None, None, None, 0
        for _ in range(2):                                     # a count-only call says what is needed
            rc = lib().bsa_window_cns_batch(self.h, _p(par7), _p(blob) if cacc else None, cacc, _p(cwin), nwin, int(max_rows), _p(cns), _p(qlt), _p(alt), oacc,
                                            _p(clen), _p(score), _p(status), _p(seq) if cap else None, _p(sq) if cap else None, _p(sa) if cap else None, cap, _p(soff))
            if rc != -5 or int(soff[nwin]) <= cap:
                break
            cap = int(soff[nwin])
            seq, sq, sa = (np.zeros(cap, dtype=np.uint8) for _ in range(3))
        self._chk(rc)
        res = []
        for g in range(nwin):
            w = cwin[g]
            o, n, c0 = int(w["out_off"]), int(clen[g]), int(w["cols_off"])
            res.append((cns[o:o + n].copy(), qlt[o:o + n].copy(), alt[o:o + n].copy(), float(score[g]), int(status[g]),
                        blob[c0:c0 + parts[g].size].reshape(int(w["mlen"]), int(w["nall"]) + 3).copy()))
        empty = np.zeros(0, np.uint8)
        return res, (seq if cap else empty, sq if cap else empty.copy(), sa if cap else empty.copy(), soff)

    def window_stitch_run(self, d_cols, cols_cap, d_cwin, nwin, d_cns_status, min_cov, d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, d_rec):
        """bsa_window_stitch_run on torch tensors (plumbing only), asynchronous on the context's stream: d_cols and d_cwin as window_msa_run wrote and
        window_cns_run filled them, d_cns_status that run's d_status (or None: every window counts as called).  Window g's stitched bases are
        d_seq[d_seq_off[g] : d_seq_off[g + 1]] where d_seq_off[g + 1] <= seq_cap (likewise d_seq_qlt and d_seq_alt, either may be None), its = / X / I / D
        words d_cig[d_cig_off[g] : d_cig_off[g + 1]] where d_cig_off[g + 1] <= cig_cap (32-bit words); d_rec: nwin records of 32 bytes (STITCH_DTYPE).
        d_seq_off[nwin] and d_cig_off[nwin] are what a complete run needs; None arenas with caps 0 make a count-only run."""
        size = lambda t: t.numel() * t.element_size()
        if d_cols is not None and size(d_cols) < cols_cap:
            raise ValueError("window_stitch_run: d_cols holds fewer than cols_cap bytes")
        if d_cwin is not None and size(d_cwin) < 40 * nwin:
            raise ValueError("window_stitch_run: d_cwin holds fewer than nwin records")
        if d_cns_status is not None and size(d_cns_status) < 4 * nwin:
            raise ValueError("window_stitch_run: d_cns_status holds fewer than nwin entries")
        if any(t is not None and size(t) < seq_cap for t in (d_seq, d_seq_qlt, d_seq_alt)):
            raise ValueError("window_stitch_run: a sequence array holds fewer than seq_cap bytes")
        if d_cig is not None and size(d_cig) < 4 * cig_cap:
            raise ValueError("window_stitch_run: d_cig holds fewer than cig_cap words")
        if any(t is not None and size(t) < 8 * (nwin + 1) for t in (d_seq_off, d_cig_off)):
            raise ValueError("window_stitch_run: d_seq_off or d_cig_off holds fewer than nwin + 1 offsets")
        if d_rec is not None and size(d_rec) < 32 * nwin:
            raise ValueError("window_stitch_run: d_rec holds fewer than nwin records")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_window_stitch_run(self.h, ptr(d_cols), cols_cap, ptr(d_cwin), nwin, ptr(d_cns_status), int(min_cov), ptr(d_seq), ptr(d_seq_qlt), ptr(d_seq_alt),
                                              seq_cap, ptr(d_seq_off), ptr(d_cig), cig_cap, ptr(d_cig_off), ptr(d_rec)))

    def window_stitch(self, cns_out, min_cov=1, status=None):
        """bsa_window_stitch_batch on what Context.window_cns returned -- its list over the windows of (cns, qlt, alt, score, status, cols), cols the
        window's (mlen, nall + 3) columns with their consensus bytes -- or on a list of (cols, cwin) pairs with `status`, one CNS_ST_* a window (None:
        every window counts as called): every window's stitched sequence, the consensus where at least min_cov reads cover a column and the draft
        elsewhere, and its = / X / I / D words against the draft.  Returns (a list over the windows of (seq, qlt, alt, words, rec) with rec the
        window's STITCH_DTYPE record, (seq, seq_qlt, seq_alt, seq_off, cig, cig_off): the windows' bases, qualities and words one behind the other)."""
        nwin = len(cns_out)
        cwin = np.zeros(max(nwin, 1), dtype=CNS_WINDOW_DTYPE)
        cst = None if (status is None and nwin and len(cns_out[0]) == 2) else np.zeros(max(nwin, 1), np.uint32)
        parts, cacc = [], 0
        for g, item in enumerate(cns_out):
            if len(item) == 2:
                cols = _np(item[0], np.uint8)
                if cols.ndim != 2:
                    cols = cols.reshape(int(item[1]["mlen"]), int(item[1]["nall"]) + 3)
                if cst is not None:
                    cst[g] = int(status[g])
            else:
                cols = _np(item[5], np.uint8)
                cst[g] = int(item[4]) if status is None else int(status[g])
            if cols.ndim != 2 or cols.shape[1] < 4:
                raise ValueError("window_stitch: a window's columns are an (mlen, nall + 3) array")
            cwin[g] = (cacc, 0xFFFFFFFFFFFFFFFF, 0, cols.shape[1] - 3, 0, 0, cols.shape[0])
            parts.append(cols.reshape(-1))
            cacc += cols.size
        blob = _np(np.concatenate([np.zeros(0, np.uint8)] + parts), np.uint8).copy()
        soff, coff = np.zeros(nwin + 1, dtype=np.uint64), np.zeros(nwin + 1, dtype=np.uint64)
        rec = np.zeros(max(nwin, 1), dtype=STITCH_DTYPE)
        seq, sq, sa, cig, scap, ccap = None, None, None, None, 0, 0
        for _ in range(2):                                     # a count-only call says what is needed
            rc = lib().bsa_window_stitch_batch(self.h, _p(blob) if cacc else None, cacc, _p(cwin), nwin, _p(cst) if cst is not None else None, int(min_cov),
                                               _p(seq) if scap else None, _p(sq) if scap else None, _p(sa) if scap else None, scap, _p(soff),
                                               _p(cig) if ccap else None, ccap, _p(coff), _p(rec))
            if rc != -5 or (int(soff[nwin]) <= scap and int(coff[nwin]) <= ccap):
                break
            scap, ccap = int(soff[nwin]), int(coff[nwin])
            seq, sq, sa = (np.zeros(max(scap, 1), dtype=np.uint8) for _ in range(3))
            cig = np.zeros(max(ccap, 1), dtype=np.uint32)
        self._chk(rc)
        empty = np.zeros(0, np.uint8)
        seq, sq, sa = (a[:scap] if scap else empty.copy() for a in (seq, sq, sa))
        cig = cig[:ccap] if ccap else np.zeros(0, np.uint32)
        res = []
        for g in range(nwin):
            a, b, c, d = int(soff[g]), int(soff[g + 1]), int(coff[g]), int(coff[g + 1])
            res.append((seq[a:b].copy(), sq[a:b].copy(), sa[a:b].copy(), cig[c:d].copy(), rec[g].copy()))
        return res, (seq, sq, sa, soff, cig, coff)

    def window_realign_run(self, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, window, d_seq, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, par,
                           d_piece2, d_pcig2, pcig2_cap, d_pcig2_off, d_pstatus, d_cost, d_doff2, d_dlen2):
        """bsa_window_realign_run on torch tensors (plumbing only), asynchronous on the context's stream: d_piece, d_piece_off, d_bases as
        window_pieces_run (or window_select_run) left them, `window` that round's window size, d_seq, d_seq_off, d_cig, d_cig_off as window_stitch_run
        left them for the same windows, par a REALIGN_PARAMS (realign_params).  d_piece2: piece_cap records of 32 bytes; d_pcig2: room for pcig2_cap
        32-bit words, or None with pcig2_cap 0 for a count-only run; d_pcig2_off: piece_cap + 1 64-bit words; d_pstatus and d_cost (or None): piece_cap
        32-bit words; d_doff2 (64-bit) and d_dlen2 (32-bit): one entry a window.  Round 2 is window_msa_run(d_piece2, d_piece_off, nwin, piece_cap,
        d_bases, bases_cap, d_pcig2, pcig2_cap, d_pcig2_off, d_seq, d_doff2, d_dlen2, par.window2, 0, vote, ...)."""
        size = lambda t: t.numel() * t.element_size()
        if any(t is not None and size(t) < 32 * piece_cap for t in (d_piece, d_piece2)):
            raise ValueError("window_realign_run: d_piece or d_piece2 holds fewer than piece_cap records")
        if any(t is not None and size(t) < 8 * (nwin + 1) for t in (d_piece_off, d_seq_off, d_cig_off)):
            raise ValueError("window_realign_run: d_piece_off, d_seq_off or d_cig_off holds fewer than nwin + 1 offsets")
        if d_bases is not None and size(d_bases) < bases_cap:
            raise ValueError("window_realign_run: d_bases holds fewer than bases_cap bytes")
        if d_seq is not None and size(d_seq) < seq_cap:
            raise ValueError("window_realign_run: d_seq holds fewer than seq_cap bytes")
        if d_cig is not None and size(d_cig) < 4 * cig_cap:
            raise ValueError("window_realign_run: d_cig holds fewer than cig_cap words")
        if d_pcig2 is not None and size(d_pcig2) < 4 * pcig2_cap:
            raise ValueError("window_realign_run: d_pcig2 holds fewer than pcig2_cap words")
        if d_pcig2_off is not None and size(d_pcig2_off) < 8 * (piece_cap + 1):
            raise ValueError("window_realign_run: d_pcig2_off holds fewer than piece_cap + 1 offsets")
        if any(t is not None and size(t) < 4 * piece_cap for t in (d_pstatus, d_cost)):
            raise ValueError("window_realign_run: d_pstatus or d_cost holds fewer than piece_cap entries")
        if (d_doff2 is not None and size(d_doff2) < 8 * nwin) or (d_dlen2 is not None and size(d_dlen2) < 4 * nwin):
            raise ValueError("window_realign_run: d_doff2 or d_dlen2 holds fewer than nwin entries")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        self._chk(lib().bsa_window_realign_run(self.h, ptr(d_piece), ptr(d_piece_off), nwin, piece_cap, ptr(d_bases), bases_cap, int(window), ptr(d_seq), seq_cap,
                                               ptr(d_seq_off), ptr(d_cig), cig_cap, ptr(d_cig_off), C.byref(par), ptr(d_piece2), ptr(d_pcig2), pcig2_cap,
                                               ptr(d_pcig2_off), ptr(d_pstatus), ptr(d_cost), ptr(d_doff2), ptr(d_dlen2)))

    def window_realign(self, windows_out, stitch_out, window, par):
        """bsa_window_realign_batch on what Context.window_pieces or Context.window_select returned (the list over the windows of (pieces, codes)) and
        what Context.window_stitch returned for the same windows: every piece aligned again, against its window's stitched sequence.  `window` is the
        window size of that round, par a REALIGN_PARAMS (realign_params).  Returns the three things Context.window_msa takes, in the shape it takes
        them -- (pieces, guides, drafts): the list over the windows of (piece records, codes) with t_first and t_last positions in the window's
        stitched sequence and the codes cut to the re-aligned piece, the list over the windows of lists of (words, status) with status a
        REALIGN_ST_* value (REALIGN_ST_EDGE set beside 0), and one code array a window, its stitched sequence.  A piece that is
        not re-aligned has len 0, no codes and no words: a dead row of round 2."""
        nwin = len(windows_out)
        _, (seq, _, _, soff, cig, coff) = stitch_out
        if len(soff) != nwin + 1 or len(coff) != nwin + 1:
            raise ValueError("window_realign: the stitch of the same windows")
        piece = _np(np.concatenate([np.zeros(0, PIECE_DTYPE)] + [_np(ps, PIECE_DTYPE) for ps, _ in windows_out]), PIECE_DTYPE).copy()
        P = len(piece)
        poff = np.zeros(nwin + 1, dtype=np.uint64)
        poff[1:] = np.cumsum([len(ps) for ps, _ in windows_out], dtype=np.uint64)
        codes = [_np(c, np.uint8) for _, cs in windows_out for c in cs]
        if len(codes) != P:
            raise ValueError("window_realign: one code array per piece")
        boff = np.zeros(P + 1, dtype=np.uint64)
        boff[1:] = np.cumsum([len(c) for c in codes], dtype=np.uint64)
        piece["base_off"] = boff[:-1]                           # the codes as they are laid out here
        bases = _np(np.concatenate([np.zeros(0, np.uint8)] + codes), np.uint8)
        seq, cig = _np(seq, np.uint8), _np(cig, np.uint32)
        soff, coff = _np(soff, np.uint64), _np(coff, np.uint64)
        piece2 = np.zeros(max(P, 1), dtype=PIECE_DTYPE)
        off2 = np.zeros(P + 1, dtype=np.uint64)
        pst, cost = np.zeros(max(P, 1), np.uint32), np.zeros(max(P, 1), np.uint32)
        doff2, dlen2 = np.zeros(max(nwin, 1), np.uint64), np.zeros(max(nwin, 1), np.uint32)
        words, cap = None, 0
        for _ in range(2):                                     # a count-only call says what is needed
            rc = lib().bsa_window_realign_batch(self.h, _p(piece) if P else None, _p(poff), nwin, P, _p(bases) if len(bases) else None, len(bases), int(window),
                                                _p(seq) if len(seq) else None, len(seq), _p(soff), _p(cig) if len(cig) else None, len(cig), _p(coff), C.byref(par),
                                                _p(piece2), _p(words) if cap else None, cap, _p(off2), _p(pst), _p(cost), _p(doff2), _p(dlen2))
            if rc != -5 or int(off2[P]) <= cap:
                break
            cap = int(off2[P])
            words = np.zeros(cap, dtype=np.uint32)
        self._chk(rc)
        pieces, guides, drafts = [], [], []
        for g in range(nwin):
            a, b = int(poff[g]), int(poff[g + 1])
            cs = []
            for j in range(a, b):
                lead = int(piece2[j]["base_off"]) - int(piece[j]["base_off"])
                cs.append(codes[j][lead:lead + int(piece2[j]["len"])].copy())
            pieces.append((piece2[a:b].copy(), cs))
            guides.append([(words[int(off2[j]):int(off2[j + 1])].copy() if cap else np.zeros(0, np.uint32), int(pst[j])) for j in range(a, b)])
            drafts.append(seq[int(doff2[g]):int(doff2[g]) + int(dlen2[g])].copy())
        return pieces, guides, drafts

    def snv_model(self, max_rows):
        """bsa_snv_model_create: the SNV caller's tables for windows of up to max_rows voting rows (at most 1000) resident on the device, for
        window_snv_run; closed with the context (or by its own close())."""
        m = SnvModel(self, max_rows)
        self._models.append(m)
        return m

    def window_snv_run(self, model, d_cols, cols_cap, d_cwin, nwin, d_cns_status, par, d_snv, snv_cap, d_snv_off, d_rec):
        """bsa_window_snv_run on torch tensors (plumbing only), asynchronous on the context's stream: d_cols and d_cwin as window_msa_run wrote and
        window_cns_run filled them, d_cns_status that run's d_status (or None: every window counts), par a SNV_PARAMS record (snv_params()).  Window
        g's calls are the 24-byte records (SNV_DTYPE) d_snv[d_snv_off[g] : d_snv_off[g + 1]] where d_snv_off[g + 1] <= snv_cap (records);
        d_snv_off[nwin] is what a complete run needs; d_rec: nwin records of 16 bytes (SNV_WINDOW_DTYPE).  A None arena with cap 0 only counts."""
        size = lambda t: t.numel() * t.element_size()
        if d_cols is not None and size(d_cols) < cols_cap:
            raise ValueError("window_snv_run: d_cols holds fewer than cols_cap bytes")
        if d_cwin is not None and size(d_cwin) < 40 * nwin:
            raise ValueError("window_snv_run: d_cwin holds fewer than nwin records")
        if d_cns_status is not None and size(d_cns_status) < 4 * nwin:
            raise ValueError("window_snv_run: d_cns_status holds fewer than nwin entries")
        if d_snv is not None and size(d_snv) < 24 * snv_cap:
            raise ValueError("window_snv_run: d_snv holds fewer than snv_cap records")
        if d_snv_off is not None and size(d_snv_off) < 8 * (nwin + 1):
            raise ValueError("window_snv_run: d_snv_off holds fewer than nwin + 1 offsets")
        if d_rec is not None and size(d_rec) < 16 * nwin:
            raise ValueError("window_snv_run: d_rec holds fewer than nwin records")
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        par = None if par is None else np.ascontiguousarray(par, dtype=SNV_PARAMS).reshape(-1)[:1]
        self._chk(lib().bsa_window_snv_run(self.h, model.h if model is not None else None, ptr(d_cols), cols_cap, ptr(d_cwin), nwin, ptr(d_cns_status),
                                           _p(par) if par is not None else None, ptr(d_snv), snv_cap, ptr(d_snv_off), ptr(d_rec)))

    def window_snv(self, cns_out, par=None, max_rows=None, status=None, nseq=None):
        """bsa_window_snv_batch on what Context.window_cns returned -- its list over the windows of (cns, qlt, alt, score, status, cols) -- or on a list
        of (cols, cwin) pairs with `status`, one CNS_ST_* a window (None: every window counts).  The voting rows of window g are nseq[g] (an int serves
        all windows), by default the record's nseq of a (cols, cwin) pair and every row but the last -- the draft -- of a window_cns item.  par: a
        SNV_PARAMS record (default: snv_params()); max_rows: the depth of the model (default: the largest nseq).  Returns (a list over the windows of
        (snv, rec): the window's SNV_DTYPE records and its SNV_WINDOW_DTYPE record, (snv, snv_off) of the call)."""
        nwin = len(cns_out)
        par = snv_params() if par is None else np.ascontiguousarray(par, dtype=SNV_PARAMS).reshape(-1)[:1]
        cwin = np.zeros(max(nwin, 1), dtype=CNS_WINDOW_DTYPE)
        cst = None if (status is None and nwin and len(cns_out[0]) == 2) else np.zeros(max(nwin, 1), np.uint32)
        parts, cacc = [], 0
        for g, item in enumerate(cns_out):
            if len(item) == 2:
                cols = _np(item[0], np.uint8)
                if cols.ndim != 2:
                    cols = cols.reshape(int(item[1]["mlen"]), int(item[1]["nall"]) + 3)
                rows = int(item[1]["nseq"])
                if cst is not None:
                    cst[g] = int(status[g])
            else:
                cols = _np(item[5], np.uint8)
                rows = cols.shape[1] - 4 if cols.ndim == 2 else 0
                cst[g] = int(item[4]) if status is None else int(status[g])
            if cols.ndim != 2 or cols.shape[1] < 4:
                raise ValueError("window_snv: a window's columns are an (mlen, nall + 3) array")
            if nseq is not None:
                rows = int(nseq) if np.isscalar(nseq) else int(nseq[g])
            cwin[g] = (cacc, 0xFFFFFFFFFFFFFFFF, 0, cols.shape[1] - 3, rows, rows, cols.shape[0])
            parts.append(cols.reshape(-1))
            cacc += cols.size
        blob = _np(np.concatenate([np.zeros(0, np.uint8)] + parts), np.uint8).copy()
        if max_rows is None:
            max_rows = int(cwin["nseq"][:nwin].max()) if nwin else 0
        off = np.zeros(nwin + 1, dtype=np.uint64)
        rec = np.zeros(max(nwin, 1), dtype=SNV_WINDOW_DTYPE)
        snv, cap = None, 0
        for _ in range(2):                                     # a count-only call says what is needed
            rc = lib().bsa_window_snv_batch(self.h, int(max_rows), _p(blob) if cacc else None, cacc, _p(cwin), nwin, _p(cst) if cst is not None else None, _p(par),
                                            _p(snv) if cap else None, cap, _p(off), _p(rec))
            if rc != -5 or int(off[nwin]) <= cap:
                break
            cap = int(off[nwin])
            snv = np.zeros(cap, dtype=SNV_DTYPE)
        self._chk(rc)
        snv = snv[:cap] if cap else np.zeros(0, SNV_DTYPE)
        return [(snv[int(off[g]):int(off[g + 1])].copy(), rec[g].copy()) for g in range(nwin)], (snv, off)


class SnvModel:
    """the SNV caller's tables resident on the device -- bsa_snv_model_create / bsa_snv_model_destroy (Context.snv_model)"""

    def __init__(self, ctx, max_rows):
        h = C.c_void_p()
        ctx._chk(lib().bsa_snv_model_create(ctx.h, int(max_rows), C.byref(h)))
        self.h = h
        self.max_rows = int(max_rows)

    def close(self):
        if self.h:
            lib().bsa_snv_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CnsModel:
    """a consensus model resident on the device -- bsa_cns_model_create / bsa_cns_model_destroy (Context.cns_model)"""

    def __init__(self, ctx, par7):
        par7 = np.ascontiguousarray(par7, np.float32)
        if par7.shape != (7,):
            raise ValueError("cns_model: seven rates (psub pins pdel piex pdex hins hdel)")
        h = C.c_void_p()
        ctx._chk(lib().bsa_cns_model_create(ctx.h, _p(par7), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().bsa_cns_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mix32(x):
    """the 32-bit finaliser bsa_window_select_* hashes a pair with (include/bsalign_hip.h)"""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = x * 0x85EBCA6B & 0xFFFFFFFF
    x ^= x >> 13
    x = x * 0xC2B2AE35 & 0xFFFFFFFF
    return x ^ x >> 16


def window_gbase(target_id, target_len, window):
    """gbase for bsa_window_pieces_*: the drafts' windows numbered through -- target j's first window is the exclusive sum of ceil(target_len / window)
    over the targets in front of it.  target_id: for every pair the index of its target; -> (gbase per pair as uint64, nwin).  Host only."""
    window = int(window)
    if window <= 0:
        raise ValueError("window_gbase: window must be positive")
    tl = _np(target_len, np.uint64)
    per = (tl + np.uint64(window - 1)) // np.uint64(window)
    first = np.zeros(len(tl) + 1, dtype=np.uint64)
    first[1:] = np.cumsum(per, dtype=np.uint64)
    return first[_np(target_id, np.int64)].astype(np.uint64), int(first[-1])


def window_drafts(target_off, target_len, window):
    """doff, dlen for bsa_window_msa_*, the sibling of window_gbase: the drafts' windows numbered through as there, window m of target j is the
    slice that starts at target_off[j] + m * window and has target_len[j] - m * window bases left (the pass takes min(dlen, window) of them).
    target_off: where each target starts in the draft array (bytes, or bases of a packed one); -> (doff as uint64, dlen as uint32), one entry a
    window.  Host only."""
    window = int(window)
    if window <= 0:
        raise ValueError("window_drafts: window must be positive")
    to, tl = _np(target_off, np.uint64), _np(target_len, np.uint64)
    if len(to) != len(tl):
        raise ValueError("window_drafts: one offset per target")
    per = ((tl + np.uint64(window - 1)) // np.uint64(window)).astype(np.int64)
    j = np.repeat(np.arange(len(tl)), per)
    first = np.zeros(len(tl) + 1, dtype=np.int64)
    first[1:] = np.cumsum(per)
    m = (np.arange(int(first[-1]), dtype=np.int64) - first[j]).astype(np.uint64) * np.uint64(window)
    return (to[j] + m).astype(np.uint64), np.minimum(tl[j] - m, np.uint64(0xFFFFFFFF)).astype(np.uint32)


def cigar_windows_bound(tlen, window):
    """bsa_cigar_windows_bound: sum of ceil(tlen / window), a window arena (records) that always suffices; 0 for window == 0; host only"""
    tlen = _np(tlen, np.uint32)
    return int(lib().bsa_cigar_windows_bound(_p(tlen), len(tlen), int(window)))


def piece_cigars_bound(cigar_off, npiece):
    """bsa_piece_cigars_bound: the words the n + 1 offsets speak of plus npiece, a word arena that always suffices for pieces of which no two
    of a pair share a column (those of one cigar_windows call); host only"""
    off = _np(cigar_off, np.uint64)
    return int(lib().bsa_piece_cigars_bound(_p(off) if len(off) else None, max(len(off) - 1, 0), int(npiece)))


def window_msa_bound(piece_off, window, ins_units):
    """bsa_window_msa_bound: a column arena (bytes) that always suffices for the pieces of one chain -- window * (depth + 4) summed over the windows
    plus ins_units * (the largest depth + 4), ins_units the I units of all the alignments' words; host only"""
    off = _np(piece_off, np.uint64)
    return int(lib().bsa_window_msa_bound(_p(off) if len(off) else None, max(len(off) - 1, 0), int(window), int(ins_units)))


def synth_pairs_host(n, L, eps=0.10, seed=20240611, first_pair=0):
    """host (C) form of the synthetic generator: returns list of (q, t)"""
    stride = lib().bsa_synth_stride(L)
    seqs = np.zeros(2 * n * stride, dtype=np.uint8)
    qlen = np.zeros(n, dtype=np.uint32)
    rc = lib().bsa_synth_pairs_host(seed, first_pair, n, L, int(eps * 4294967296.0), _p(seqs), _p(qlen))
    if rc != 0:
        raise BsaError(rc)
    return [(seqs[(n + k) * stride:(n + k) * stride + qlen[k]].copy(), seqs[k * stride:k * stride + L].copy()) for k in range(n)]


class AlignPlan:
    """two-phase form (bsa_align_plan_create / bsa_align_run): host metadata once, device-resident data per run.
    Device buffers are torch tensors (plumbing only); the run is asynchronous on the context's stream.  With MODE_SEQ2BIT in
    par.mode, d_seqs holds 2-bit packed words (pack2bit) and the offsets are base offsets; with MODE_CIGAR_EQX the CIGAR words
    are = / X runs and d_cigar must hold the expanded words; with MODE_QSTRAND a qoff[k] with QOFF_REVCOMP OR-ed in aligns the
    reverse complement of the stored query; with MODE_BAND_MARGIN d_status is required and d_status[k] >> ST_MARGIN_SHIFT is the
    pair's band margin."""

    def __init__(self, ctx, qoff, qlen, toff, tlen, par):
        self.ctx = ctx
        self.n = len(qlen)
        self.qoff, self.qlen = _np(qoff, np.uint64), _np(qlen, np.uint32)
        self.toff, self.tlen = _np(toff, np.uint64), _np(tlen, np.uint32)
        self.par = par
        h = C.c_void_p()
        ctx._chk(lib().bsa_align_plan_create(ctx.h, _p(self.qoff), _p(self.qlen), _p(self.toff), _p(self.tlen),
                                             self.n, C.byref(par), C.byref(h)))
        self.h = h

    def cells(self):
        return lib().bsa_align_plan_cells(self.h)

    def run(self, d_seqs, d_out, d_cigar=None, d_cigar_off=None, d_status=None):
        cap = d_cigar.numel() if d_cigar is not None else 0
        self.ctx._chk(lib().bsa_align_run(self.h, C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                          C.c_void_p(d_cigar.data_ptr() if d_cigar is not None else 0), cap,
                                          C.c_void_p(d_cigar_off.data_ptr() if d_cigar_off is not None else 0),
                                          C.c_void_p(d_status.data_ptr() if d_status is not None else 0)))

    def debug_slot(self, pair, nbytes):
        """raw traceback slot of `pair` after a single-chunk run (band offsets + row records, layout in csrc/bsa_common.h)"""
        buf = np.zeros(nbytes, dtype=np.uint8)
        rowb = C.c_uint32()
        self.ctx._chk(lib().bsa_align_debug_rows(self.h, pair, _p(buf), nbytes, C.byref(rowb)))
        return buf

    def close(self):
        if self.h:
            lib().bsa_align_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EditPlan:
    """bsa_edit_plan_create / bsa_edit_run (striped_seqedit_pairwise on the device); mode may carry MODE_SCORE_ONLY, then run with d_cigar=None,
    MODE_SEQ2BIT (d_seqs 2-bit packed words, base offsets), MODE_CIGAR_EQX (= / X words) and MODE_QSTRAND (QOFF_REVCOMP in qoff[k])"""

    def __init__(self, ctx, qoff, qlen, toff, tlen, mode=MODE_GLOBAL, bandwidth=0):
        self.ctx = ctx
        self.n = len(qlen)
        self.qoff, self.qlen = _np(qoff, np.uint64), _np(qlen, np.uint32)
        self.toff, self.tlen = _np(toff, np.uint64), _np(tlen, np.uint32)
        self.par = EditParams()
        self.par.mode, self.par.bandwidth = mode, bandwidth
        h = C.c_void_p()
        ctx._chk(lib().bsa_edit_plan_create(ctx.h, _p(self.qoff), _p(self.qlen), _p(self.toff), _p(self.tlen),
                                            self.n, C.byref(self.par), C.byref(h)))
        self.h = h

    def cells(self):
        return lib().bsa_edit_plan_cells(self.h)

    def run(self, d_seqs, d_out, d_cigar=None, d_cigar_off=None, d_status=None):
        cap = d_cigar.numel() if d_cigar is not None else 0
        self.ctx._chk(lib().bsa_edit_run(self.h, C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                         C.c_void_p(d_cigar.data_ptr() if d_cigar is not None else 0), cap,
                                         C.c_void_p(d_cigar_off.data_ptr() if d_cigar_off is not None else 0),
                                         C.c_void_p(d_status.data_ptr() if d_status is not None else 0)))

    def close(self):
        if self.h:
            lib().bsa_edit_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmer_chain_words_bound(qlen, tlen):
    """bsa_kmer_chain_words_bound: sum of min(qlen, tlen), an anchor arena (64-bit words) that always suffices; host only"""
    qlen, tlen = _np(qlen, np.uint32), _np(tlen, np.uint32)
    if len(qlen) != len(tlen):
        raise ValueError("kmer_chain_words_bound: one tlen per qlen")
    return int(lib().bsa_kmer_chain_words_bound(_p(qlen), _p(tlen), len(qlen)))


class KmerChainPlan:
    """bsa_kmer_chain_plan_create / bsa_kmer_chain_run: kmer_chain_batch for a blob that is already on the device -- host metadata once, device
    pointers per run (torch tensors, plumbing only), asynchronous on the context's stream.  flags: MODE_SEQ2BIT (d_seqs 2-bit packed words,
    8-byte aligned, base offsets), MODE_QSTRAND (QOFF_REVCOMP in qoff[k]) or KMER_STRAND_AUTO (d_status required; ST_REVCOMP marks the reverse pairs).
    qoff / toff are offsets into d_seqs as the caller holds it; that they lie inside it is the caller's business.  Raises BsaError(-6) for a pair
    the device route does not take (qlen + tlen above 262144, or a slice larger than the workspace limit): there is no host route behind a run."""

    def __init__(self, ctx, qoff, qlen, toff, tlen, ksz=13, flags=0):
        self.ctx = ctx
        self.n = len(qlen)
        self.qoff, self.qlen = _np(qoff, np.uint64), _np(qlen, np.uint32)
        self.toff, self.tlen = _np(toff, np.uint64), _np(tlen, np.uint32)
        self.ksz, self.flags = ksz, flags
        h = C.c_void_p()
        ctx._chk(lib().bsa_kmer_chain_plan_create(ctx.h, _p(self.qoff), _p(self.qlen), _p(self.toff), _p(self.tlen), self.n, ksz, flags, C.byref(h)))
        self.h = h

    def chunks(self):
        """workspace chunks one run goes through"""
        return int(lib().bsa_kmer_chain_plan_chunks(self.h))

    def run(self, d_seqs, d_maps, d_maps_off, d_status=None):
        """d_maps: the anchor arena (its numel() 64-bit words are the capacity) or None for a count-only run; d_maps_off: n + 1 64-bit words;
        d_status: n 32-bit words or None.  Pair k's anchors are d_maps[d_maps_off[k] : d_maps_off[k + 1]] where d_maps_off[k + 1] <= capacity;
        d_maps_off[n] is the number of words a complete run needs."""
        cap = d_maps.numel() if d_maps is not None else 0
        self.ctx._chk(lib().bsa_kmer_chain_run(self.h, C.c_void_p(d_seqs.data_ptr()), C.c_void_p(d_maps.data_ptr() if d_maps is not None else 0), cap,
                                               C.c_void_p(d_maps_off.data_ptr()), C.c_void_p(d_status.data_ptr() if d_status is not None else 0)))

    def close(self):
        if self.h:
            lib().bsa_kmer_chain_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
