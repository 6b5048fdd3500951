/*
 * bsalign_hip.h -- C-ABI of libbsalign_hip.so: the MI355X (gfx950) implementation of
 * bsalign's banded striped DP hot path.
 *
 * Plain C types only: no HIP, torch or C++ types cross this boundary.  Every entry
 * point returns 0 on success or a negative BSA_E_* code (the reference abort()s
 * instead: bsalign.h:3882-3885, 1076-1079).  Nothing here falls back to a CPU
 * implementation: without a usable GPU every compute entry point fails with
 * BSA_E_NODEVICE.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   bsa_align_*   <- banded_striped_epi8_seqalign_pairwise   bsalign.h:3854 (one call per pair, main.c:323-326)
 *   bsa_edit_*    <- striped_seqedit_pairwise                bsalign.h:1046 (main.c:196-204)
 *   bsa_rows_*    <- dpalign_row_update_bspoa / dpalign_row_merge_bspoa  bspoa.h:2232-2272
 *                    (= banded_striped_epi8_seqalign_piecex_row_movx + _row_cal + _row_merge,
 *                     bsalign.h:2244, 3181, 2474)
 *   bsa_result_t  <- seqalign_result_t                       bsalign.h:213-218
 *   CIGAR words   <- u4v of (len << 4 | op)                  bsalign.h:61-69, 401-417
 * The reference has no batch interface (one pair per call, one thread); the batch
 * forms below are the device-sized equivalent of its per-pair loop.  The drop-in
 * single-pair functions with the reference's exact signatures live in
 * include/bsalign_compat.h and are thin wrappers over these.
 */
#ifndef BSALIGN_HIP_H
#define BSALIGN_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "bsalign_msa.h"           /* bsa_cns_window_t, the record bsa_window_msa_* writes */

#ifdef __cplusplus
extern "C" {
#endif

/* modes (bsalign.h:30-38) */
#define BSA_MODE_GLOBAL   0
#define BSA_MODE_OVERLAP  1
#define BSA_MODE_EXTEND   2
#define BSA_MODE_ROWRECORDS 0x100 /* flag: keep the reference-layout row records and the literal traceback even where the
                                      compact 4-bit-code path applies (global mode, 1-piece gaps, small scores) */
#define BSA_MODE_SCORE_ONLY 0x400 /* flag: score and end cell only, no traceback -- for the 8-bit aligner (bsa_align_batch / _plan_create /
                                      _run) and the edit aligner (bsa_edit_batch / _plan_create / _run) alike.  Every bsa_result_t gets
                                      score, qe and te exactly as the same call without the flag returns them (the reference's tie rules
                                      included); qb, tb, mat, mis, ins, del and aln would need a traceback and are set to -1, for flagged and
                                      empty pairs as well.  No CIGAR is returned: cigar / d_cigar may be NULL (cigar_cap_words 0), a given
                                      cigar_off / d_cigar_off gets n + 1 zeros.  status: the same bits as without the flag.
                                      8-bit aligner: BSA_ST_TRACE only where the band never reached the query end in global mode;
                                      bsa_align_batch hands such pairs over as it does without the flag -- a pair on which the reference's
                                      own traceback does not terminate is NOT flagged here, it simply has a score.  Fast (forward kernel
                                      alone, a fixed-size record a pair instead of code rows) with one-piece gaps at bandwidth 64, 128 and
                                      256 -- or whole-query bands of up to 256 columns -- inside the exact-arithmetic guard; every other
                                      parameter set runs the full path and drops what the traceback found.
                                      BSA_MODE_SCORE_ONLY | BSA_MODE_ROWRECORDS is BSA_E_ARG.
                                      Edit aligner: fast (forward kernel alone, the last row a pair instead of every row's planes) in
                                      global and extend mode at every bandwidth; overlap mode needs the walk's tb for its score
                                      (smin + te - tb) and runs the full path, dropping what the traceback found. */
#define BSA_MODE_SEQ2BIT 0x800    /* flag: the sequence blob is 2-bit packed -- for bsa_align_batch / _plan_create / _run and bsa_edit_batch /
                                      _plan_create / _run.  seqs / d_seqs then points to uint64_t words holding 32 bases each, MSB first:
                                      base i sits at bits 62 - 2 (i % 32) of word i / 32 (little-endian words).  Example: the 35 bases
                                      ACGT ACGT ... (codes 0 1 2 3 repeated) are word 0 = 0x1B1B1B1B1B1B1B1B and word 1 = 0x1800000000000000 (bases
                                      32..34 = A C G in its top six bits).  This is the layout of the reference's BaseBank.bits (dna.h,
                                      seq2bits / bits2bit), so a caller holding a BaseBank passes bnk->bits and its own read offsets.
                                      qoff[k] / toff[k] are BASE offsets into the words, any offset (a read need not start on a word or a
                                      byte); seqs_bytes is the size of the word array in bytes and must be a multiple of 8; every pair must
                                      have off + len <= 4 * seqs_bytes, else BSA_E_ARG.  d_seqs must be 8-byte aligned (bsa_align_run /
                                      bsa_edit_run: BSA_E_ARG otherwise).  Nothing is read behind the word that holds a pair's last base.
                                      Results, CIGAR words and status are bit-identical to the same call on the unpacked bytes, except that
                                      BSA_ST_BAD_BASE cannot occur.  Combines with BSA_MODE_SCORE_ONLY and BSA_MODE_ROWRECORDS.  Only the
                                      upload and the staging kernels see the packed form: the kernels behind them read the same staged
                                      1 B/base copy as without the flag.  Also taken by the k-mer calls bsa_kmer_chain_batch2 and
                                      bsa_kmer_edit_batch2 (in their `flags`, see there; bsa_kmer_edit_batch has no flags).  Not taken by the
                                      compat single-pair layer, the bsalign-hip CLI, bsa_shard_*, the POA or the rows API.  bsa_seq_pack2bit packs device-resident
                                      1 B/base codes. */
#define BSA_MODE_CIGAR_EQX 0x1000 /* flag: = / X CIGAR words -- for bsa_align_batch / _plan_create / _run and bsa_edit_batch / _plan_create /
                                      _run.  The reference defines the two ops (SEQALIGN_CIGAR_E / _X, bsalign.h:68-69) and prints them, but
                                      none of its aligners produce them: a diagonal step is always M (bsalign.h:3788).  With the flag the
                                      CIGAR of pair k is the CIGAR of the same call without it with every M word replaced, in place and in
                                      order, by the maximal runs of BSA_CIGAR_EQ and BSA_CIGAR_X that cover the same columns: column j of
                                      an M word that starts at query position qp and target position tp is = when query[qp + j] ==
                                      target[tp + j] as base codes, X otherwise.  Positions start at the record's qb, tb; M / = / X
                                      consume one base of both sequences, I one query base, D one target base.  I and D words are
                                      unchanged.  No word has length 0, no two neighbouring words have the same op, and merging every run
                                      of = / X words back into one M word gives the plain call's words exactly; the = lengths of a pair sum
                                      to its record's mat, the X lengths to its mis.  out[k] and status[k] are bit-identical to the call
                                      without the flag.  cigar_off, cigar_cap_words and BSA_E_CIGAR_CAP count the EXPANDED words (on
                                      BSA_E_CIGAR_CAP cigar_off[n] is the number of expanded words needed); a caller can bound them:
                                      expanded words <= plain words + 2 * mis, and never more than qlen + tlen.  A pair that returns no
                                      CIGAR without the flag (empty, bad base, BSA_ST_TRACE, BSA_ST_DEVICE) returns none with it.
                                      Combines with BSA_MODE_SEQ2BIT and BSA_MODE_ROWRECORDS; with BSA_MODE_SCORE_ONLY there is no CIGAR and
                                      the flag has no effect (not an error).  bsa_align_batch keeps it on every route it takes (two
                                      slices, width classes of whole-query bands, pairs handed over to the literal kernels).  The split
                                      is a pass over the words the traceback kernels leave, on the device, against the staged sequences
                                      (bsa_cigar_eqx.hip): without the flag no kernel of it is launched and nothing else changes.
                                      Not taken by bsa_kmer_edit_batch (its parameters have no mode, and bsa_kmer_assemble would have to
                                      merge = runs across anchors), the compat single-pair layer (its mode bits 4 / 8 / 16 are the
                                      reference's), the bsalign-hip CLI (its alignment strings already mark mismatches), the POA or the
                                      rows API.  bsa_shard_gather carries CIGAR words as opaque data and needs no flag. */

#define BSA_MODE_QSTRAND  0x2000  /* flag: bit 63 of qoff[k] is the query's strand -- for bsa_align_batch / _plan_create / _run and bsa_edit_batch /
                                      _plan_create / _run.  With the flag, qoff[k] & ~BSA_QOFF_REVCOMP is the offset of the stored query (bytes,
                                      or bases with BSA_MODE_SEQ2BIT) and qoff[k] & BSA_QOFF_REVCOMP says that pair k aligns the REVERSE
                                      COMPLEMENT q' of the stored qlen[k] bases: q'[i] = 3 - q[qlen - 1 - i] (codes A 0, C 1, G 2, T 3, so the
                                      complement is (~c) & 3 -- what the reference's dna.h does; its revseq_basebank builds such a copy on the
                                      host).  toff is untouched: only queries have a strand (reverse-complementing both sides is the mirrored
                                      forward alignment).  A read that takes part in many pairs, on either strand, is stored once.
                                      Everything returned for a marked pair is bit-identical to the same call WITHOUT the flag on a blob in
                                      which the caller stored q': all ten fields of bsa_result_t, the CIGAR words (read along q', also with
                                      BSA_MODE_CIGAR_EQX), cigar_off, status.  qb / qe are positions in q'; the interval on the stored strand
                                      is [qlen - qe, qlen - qb).  Example: a stored query of 100 bases, marked, comes back with qb = 10,
                                      qe = 95 -- the alignment covers q'[10, 95), which is the reverse complement of stored bases [5, 90);
                                      the first CIGAR word speaks of stored base 89, the last one of stored base 5.
                                      A marked pair whose stored 1 B/base query holds a code above 3 gets BSA_ST_BAD_BASE, exactly when the
                                      unmarked pair would; a marked query of length 0 is BSA_ST_EMPTY.  A batch with the flag in which no
                                      pair is marked returns what the call without the flag returns.  Without the flag nothing changes: bit
                                      63 stays part of the offset (bsa_*_batch answers BSA_E_ARG, offsets outside the blob), the staging
                                      kernels launched are the ones without the strand test, no extra kernel runs and no extra workspace is
                                      taken.  Bounds are tested on, and reads made from, the masked offset; with BSA_MODE_SEQ2BIT nothing is
                                      read in front of the word that holds the stored query's first base nor behind the one that holds its
                                      last.  Combines with BSA_MODE_SCORE_ONLY, BSA_MODE_SEQ2BIT, BSA_MODE_ROWRECORDS, BSA_MODE_CIGAR_EQX and
                                      all three alignment modes; bsa_align_batch keeps it on every route it takes (two slices, width classes
                                      of whole-query bands, pairs handed over to the literal kernels, the checked whole-query kernel's
                                      re-runs).  Only the four staging kernels see the strand: they stage q' and everything behind them reads
                                      the staged copy as before.  Also taken by the k-mer calls bsa_kmer_chain_batch2 and bsa_kmer_edit_batch2 (in
                                      their `flags`: both chainers read a marked query mirrored and complemented, see there; bsa_kmer_edit_batch
                                      has no flags).  Not taken by the compat single-pair layer, the bsalign-hip CLI (the reference's command line has no
                                      strand option), the POA or the rows API.  Shards: the local_qoff arrays bsa_shard_scatter hands back
                                      are the caller's; OR-ing BSA_QOFF_REVCOMP into them before bsa_align_plan_create / bsa_edit_plan_create
                                      (with the flag in the mode) is the supported way to use strands with shards. */
#define BSA_QOFF_REVCOMP  (1ull << 63) /* only with BSA_MODE_QSTRAND */
#define BSA_MODE_BAND_MARGIN 0x4000 /* flag: status[k] >> BSA_ST_MARGIN_SHIFT is the BAND MARGIN of pair k -- how close its alignment came to the edge
                                      of its band -- for bsa_align_batch / _plan_create / _run.  The 8-bit aligner is a heuristic: its band of
                                      `bandwidth` columns slides with the scores (bsalign.h:3331-3349, 4007-4021), and where the true alignment drifts
                                      further than the band can follow the call still returns a well-formed record and CIGAR, of an alignment
                                      squeezed along the band's edge.  The margin says which pairs those are.
                                      status[k] & 0xFFFF, out[k], the CIGAR words and cigar_off are bit-identical to the same call without the flag.
                                      Definition.  B = roundup16(bandwidth ? bandwidth : qlen), the reference's effective width (bsalign.h:3861-3862),
                                      whatever width the kernel that runs has.  The path is the sequence of vertices (i, j) = (target bases, query
                                      bases consumed): it starts at (tb, qb), which counts, and follows the CIGAR of the plain call -- an M (or
                                      = / X) word of length L visits (i + k, j + k) for k = 1..L, an I word (i, j + k), a D word (i + k, j).  A
                                      vertex with i >= 1 and j >= 1 is the DP cell of target row r = i - 1 and query column c = j - 1; other
                                      vertices are skipped.  With b = the band offset of row r (the band covers columns [b, b + B)) the cell
                                      contributes c - b, its distance to the low edge, only if b > 0, and b + B - 1 - c, to the high edge, only
                                      if b + B < qlen: an edge that lies on an end of the query constrains nothing.  The margin is the minimum
                                      of all contributions (one below 0 -- a cell outside its row's band, which no traceback visits -- counts
                                      as 0), clamped to 0xFFFE.  It is BSA_ST_MARGIN_NONE when nothing contributed -- always so for whole-query
                                      bands, B >= qlen -- and when the pair returns no CIGAR (empty, bad base, BSA_ST_TRACE, BSA_ST_DEVICE).
                                      Margin 0: the path ran on an edge cell of a band that could have been somewhere else -- the pair to run
                                      again at a wider band.
                                      Example: bandwidth 16, query and target of 24 bases, qb = tb = 0, CIGAR 24M -- the cells (r, r) --, band
                                      offsets of rows 0..23 = 0 0 0 0 0 0 0 0 1 2 3 4 5 6 7 8 8 8 8 8 8 8 8 8.  The low edge counts on rows 8..23
                                      (b > 0): r - b = 7 on rows 8..15, then 8..15.  The high edge counts on rows 0..14 (b + 16 < 24):
                                      b + 15 - r = 15 down to 8 on rows 0..7, 8 on rows 8..14.  The margin is 7.  Had the CIGAR been 12M 4D 4I 8M,
                                      the deletion would run down column 11 to row 15 (b = 8: low 3) and the margin would be 3.
                                      status == NULL / d_status == NULL with the flag is BSA_E_ARG (the margin has nowhere else to go);
                                      BSA_MODE_BAND_MARGIN | BSA_MODE_SCORE_ONLY is BSA_E_ARG (there is no path).  Combines with all three alignment
                                      modes and with BSA_MODE_ROWRECORDS, BSA_MODE_SEQ2BIT, BSA_MODE_QSTRAND and BSA_MODE_CIGAR_EQX (= / X words
                                      count as M: the margin is the one without it).  bsa_align_batch keeps it on every route it takes (two
                                      slices, width classes of whole-query bands, pairs handed over to the literal kernels -- their margin comes
                                      from the re-run's own band --, the checked whole-query kernel's re-runs) and decides its hand-over from the
                                      low status half alone.  The margin is a pass over the band offsets and CIGAR words the forward and traceback
                                      kernels leave in a pair's workspace slot (bsa_band_margin.hip), after each chunk's traceback: without the
                                      flag no kernel of it is launched, no workspace is taken, no existing kernel changes and the upper status
                                      half stays 0.  bsa_ctx_last_margin_ms times it.
                                      bsa_edit_batch / bsa_edit_plan_create answer BSA_E_ARG to the flag for now: the test oracle has no hook for
                                      the edit aligner's band trajectory, so a value there could not be pinned against the reference.  Not taken
                                      by bsa_kmer_edit_batch, the compat single-pair layer, the bsalign-hip CLI, the POA or the rows API;
                                      bsa_shard_* carry status as the caller's own array. */
#define BSA_ST_MARGIN_SHIFT 16
#define BSA_ST_MARGIN_NONE  0xFFFFu

/* CIGAR op codes (bsalign.h:61-69) */
#define BSA_CIGAR_M 0
#define BSA_CIGAR_I 1
#define BSA_CIGAR_D 2
#define BSA_CIGAR_EQ 7      /* bsalign.h:68; only with BSA_MODE_CIGAR_EQX */
#define BSA_CIGAR_X  8      /* bsalign.h:69; only with BSA_MODE_CIGAR_EQX */

/* error codes */
#define BSA_OK            0
#define BSA_E_NODEVICE   (-1)   /* no HIP device / runtime failure at context creation */
#define BSA_E_ARG        (-2)   /* invalid argument (NULL pointer, bad mode, W == 0 ...) */
#define BSA_E_NOMEM      (-3)   /* device allocation failed / workspace limit too small for one pair */
#define BSA_E_HIP        (-4)   /* a HIP call failed (see bsa_last_error) */
#define BSA_E_CIGAR_CAP  (-5)   /* cigar arena too small; cigar_off[n] holds the required number of words.  Second use: bsa_kmer_chain_batch with
                                   an anchor arena that is too small (maps_cap); maps_off[n] then holds the required number of 64-bit words */
#define BSA_E_UNSUPPORTED (-6)  /* parameter combination not implemented on the device yet */

/* per-pair status bits written to the optional status array */
#define BSA_ST_OK          0u
#define BSA_ST_BAD_BASE    1u   /* a base code > 3 (the reference would index past matrix[16]) */
#define BSA_ST_EMPTY       2u   /* qlen == 0 or tlen == 0 */
#define BSA_ST_TRACE       4u   /* traceback left the stored band: the reference does not terminate on this input.
                                    With device pointers (bsa_align_run) the compact path also sets it for a pair its flags
                                    cannot decide (none seen in testing): resubmit such pairs with BSA_MODE_ROWRECORDS.
                                    bsa_align_batch does that itself. */
#define BSA_ST_DEVICE      8u   /* the device gave the pair up: a wave of the segmented forward pass waited for the previous segment's
                                    state longer than its bound (about two seconds) -- a fault, never an input property.  Result zeroed;
                                    bsa_align_batch returns BSA_E_HIP when any pair carries it.  bsa_align_run (device pointers) is
                                    asynchronous and returns BSA_OK: its caller finds the flag in the status array it passed. */
#define BSA_ST_REVCOMP    16u   /* this call used the REVERSE COMPLEMENT of the stored query.  Set only by bsa_kmer_chain_batch2 /
                                    bsa_kmer_edit_batch2 with BSA_KMER_STRAND_AUTO, which find the strand themselves; the bits above and the
                                    upper half (band margin) keep their meaning. */

/* == seqalign_result_t (bsalign.h:213-218): 10 x int32, [qb,qe) x [tb,te) half-open */
typedef struct {
	int32_t score;
	int32_t qb, qe;
	int32_t tb, te;
	int32_t mat, mis, ins, del, aln;
} bsa_result_t;

/* arguments of banded_striped_epi8_seqalign_pairwise that are shared by a batch (bsalign.h:399) */
typedef struct {
	int32_t  mode;        /* BSA_MODE_* */
	uint32_t bandwidth;   /* 0 => qlen of each pair; rounded up to a multiple of 16 (bsalign.h:3861-3862) */
	int8_t   matrix[16];  /* matrix[q*4+t] (bsalign.h:323) */
	int8_t   gapo1, gape1, gapo2, gape2; /* negative penalties as the reference's CLI stores them (main.c:283-288) */
} bsa_align_params_t;

typedef struct {
	int32_t  mode;        /* BSA_MODE_* */
	uint32_t bandwidth;   /* rounded to a multiple of 64 with the rules of bsalign.h:1055-1067 */
} bsa_edit_params_t;

typedef struct bsa_ctx bsa_ctx_t;

/* ---- context ------------------------------------------------------------------------------ */
int         bsa_ctx_create(int device, bsa_ctx_t **out);
void        bsa_ctx_destroy(bsa_ctx_t *ctx);
/* run on a caller-owned hipStream_t (passed as void*); NULL = the context's own stream */
int         bsa_ctx_set_stream(bsa_ctx_t *ctx, void *hip_stream);
/* cap the device scratch (traceback rows) the context may allocate; 0 = 80% of free memory */
int         bsa_ctx_set_workspace_limit(bsa_ctx_t *ctx, size_t bytes);
int         bsa_ctx_sync(bsa_ctx_t *ctx);
const char *bsa_last_error(bsa_ctx_t *ctx);
/* average duration (ms) of the dominant kernel's launches in the last *_run call, measured with HIP
 * events on the launch stream; *launches = number of launches averaged, *cells = band cells they covered */
int         bsa_ctx_last_kernel_ms(bsa_ctx_t *ctx, double *ms, long *launches, double *cells);
/* the same for the traceback launches of the last *_run call, and the names of the kernels behind the two timings
 * (traceback = 0: forward DP, 1: traceback) */
int         bsa_ctx_last_trace_ms(bsa_ctx_t *ctx, double *ms, long *launches);
const char *bsa_ctx_last_kernel_name(bsa_ctx_t *ctx, int traceback);
/* the same for the BSA_MODE_BAND_MARGIN pass of the last bsa_align_run call (one launch a workspace chunk; 0 launches without the flag) */
int         bsa_ctx_last_margin_ms(bsa_ctx_t *ctx, double *ms, long *launches);
/* pairs of the last bsa_align_batch call that the compact (code) path left undecided and the literal kernels re-ran
 * (the hand-over described at bsa_align_batch; with scores outside the static guard: the pairs the checked whole-query
 * kernel flagged) */
long        bsa_ctx_last_handover(bsa_ctx_t *ctx);
/* the device k-mer chainer in the last bsa_kmer_chain_batch / bsa_kmer_edit_batch2(BSA_KMER_CHAIN_DEVICE) call: time of its kernels (HIP events on the
 * context stream, summed over the workspace chunks), pairs it chained and pairs the host chained in the same call (any pointer may be NULL).
 * After bsa_kmer_chain_run (asynchronous): the same sum for that run, read once its last chunk has finished (the call waits for it), n and 0 */
int         bsa_ctx_last_kmer_chain_ms(bsa_ctx_t *ctx, double *ms, long *pairs_on_device, long *pairs_on_host);
void        bsa_set_score_matrix(int8_t matrix[16], int8_t mat, int8_t mis);   /* bsalign.h:323 */

/* ---- 8-bit banded striped pairwise alignment (A-rows) ------------------------------------------
 * Sequences: one base per byte, codes 0..3 (the reference's u1i* qseq/tseq), all pairs in one blob;
 * pair k uses seqs[qoff[k] .. qoff[k]+qlen[k]) and seqs[toff[k] .. toff[k]+tlen[k]).
 * Outputs: out[k]; CIGAR words of pair k at cigar[cigar_off[k] .. cigar_off[k+1]) (cigar_off has n+1
 * entries); status[k] = 0 or BSA_ST_* flags.  status may be NULL, but it is the only place a pair that stays UNDECIDED
 * can be reported (BSA_ST_TRACE: the reference's own traceback does not terminate on it, result zeroed): with status == NULL
 * bsa_align_batch returns BSA_E_UNSUPPORTED if any such pair is left, instead of BSA_OK with silent zeroed records.
 *
 * bsa_align_batch      : every pointer is HOST memory (copies in, runs, copies out, synchronises).
 * bsa_align_plan_*     : two-phase form for resident data -- the plan takes the HOST metadata
 *                        (offsets, lengths) once; bsa_align_run takes DEVICE pointers for the
 *                        sequence blob and all outputs and is asynchronous on the context stream.
 *
 * Whole-query bands (bandwidth 0, the reference CLI's default, or a bandwidth no shorter than any query): a plan
 * runs at ONE kernel width; when no query of the plan is longer than 256 bases it runs at 64 / 128 / 256 columns on
 * the fast path (same results as the reference's own width), otherwise on the slower run-time-width kernel.
 * bsa_align_batch groups the pairs of a mixed batch by width class itself; with bsa_align_plan_* group short and long
 * queries into separate plans. */
int bsa_align_batch(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                    const uint64_t *qoff, const uint32_t *qlen,
                    const uint64_t *toff, const uint32_t *tlen, size_t n,
                    const bsa_align_params_t *par,
                    bsa_result_t *out, uint32_t *cigar, size_t cigar_cap_words,
                    uint64_t *cigar_off, uint32_t *status);

typedef struct bsa_align_plan bsa_align_plan_t;
int  bsa_align_plan_create(bsa_ctx_t *ctx, const uint64_t *qoff, const uint32_t *qlen,
                           const uint64_t *toff, const uint32_t *tlen, size_t n,
                           const bsa_align_params_t *par, bsa_align_plan_t **out);
void bsa_align_plan_destroy(bsa_align_plan_t *plan);
/* total band cells of the plan: sum over pairs of tlen * bw_eff (the GCUPS numerator) */
double bsa_align_plan_cells(const bsa_align_plan_t *plan);
/* bsa_align_run is asynchronous and returns BSA_OK before a kernel has run, so it cannot report a CIGAR arena that is too small: the caller
 * compares d_cigar_off[n] with its capacity after the run.  With device pointers and ANY cigar_cap_words, short or not (0 with a non-NULL
 * d_cigar included):
 *   - d_out, d_status and all n + 1 entries of d_cigar_off are exactly those of a run with a large arena; every element of the three is
 *     written by every run (zero records and BSA_ST_* flags for the pairs without a result), whatever the buffers held;
 *   - d_cigar_off[n] is the number of words needed;
 *   - no word at an index at or above cigar_cap_words is touched, and none at or above d_cigar_off[n];
 *   - every pair's range [d_cigar_off[k], d_cigar_off[k + 1]) inside the arena holds either exactly that pair's words or is untouched;
 *   - with cigar_cap_words >= d_cigar_off[n] every pair is there;
 *   - a plan of one workspace chunk on one stream (the words go straight from the walkers' slots to the arena) writes every pair whose
 *     words end inside the arena;
 *   - on the other routes (several chunks, the two-stream pipeline, BSA_CIGAR_VIA_ARENA) the words pass through a staging arena of
 *     cigar_cap_words in processing order, so a pair can fit by pair order and not by processing order: WHICH of the fitting pairs are
 *     present after an overflow is unspecified.  Do not use a short run's words; run again with d_cigar_off[n] words.
 * A run leaves nothing behind that a later run reads: a plan may be run again on other sequences of the same lengths, after a short run,
 * and in turn with other plans of the same context.  bsa_edit_run has the same contract.
 * A plan runs the kernels that the BSA_* knobs chose when it was made (bsa_align_plan_create sizes the workspace slots for them): a knob that
 * picks a kernel path, changed between the two calls, does not reach a plan that already stands. */
int  bsa_align_run(bsa_align_plan_t *plan, const uint8_t *d_seqs,
                   bsa_result_t *d_out, uint32_t *d_cigar, size_t cigar_cap_words,
                   uint64_t *d_cigar_off, uint32_t *d_status);

/* ---- 2-bit striped edit-distance pairwise alignment (E-rows) --------------------------------- */
int bsa_edit_batch(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                   const uint64_t *qoff, const uint32_t *qlen,
                   const uint64_t *toff, const uint32_t *tlen, size_t n,
                   const bsa_edit_params_t *par,
                   bsa_result_t *out, uint32_t *cigar, size_t cigar_cap_words,
                   uint64_t *cigar_off, uint32_t *status);

typedef struct bsa_edit_plan bsa_edit_plan_t;
int  bsa_edit_plan_create(bsa_ctx_t *ctx, const uint64_t *qoff, const uint32_t *qlen,
                          const uint64_t *toff, const uint32_t *tlen, size_t n,
                          const bsa_edit_params_t *par, bsa_edit_plan_t **out);
void bsa_edit_plan_destroy(bsa_edit_plan_t *plan);
double bsa_edit_plan_cells(const bsa_edit_plan_t *plan);
/* the arena and re-run contract stated at bsa_align_run holds here word for word */
int  bsa_edit_run(bsa_edit_plan_t *plan, const uint8_t *d_seqs,
                  bsa_result_t *d_out, uint32_t *d_cigar, size_t cigar_cap_words,
                  uint64_t *d_cigar_off, uint32_t *d_status);

/* ---- k-mer anchored edit alignment (reference: kmer_striped_seqedit_pairwise, bsalign.h:1209-1536; CLI `edit -m kmer`) ---
 * Unique same-strand k-mers (ksz <= 15) shared by the two sequences are chained on the host (bsa_kmer_edit_batch2: or on the device); only the stretches
 * between consecutive anchors are aligned, every one of them by the device edit path (two bsa_edit_batch calls for
 * the whole batch: reversed heads and tails in EXTEND mode, gaps in GLOBAL mode), and the CIGAR of each pair is stitched together exactly as the
 * reference does it (including where it puts the anchor matches).  A pair without a usable chain is aligned globally.
 * All pointers are HOST memory; cigar/cigar_off/status follow bsa_edit_batch.
 * BSA_E_CIGAR_CAP (bsa_kmer_edit_batch and bsa_kmer_edit_batch2): the capacity is compared with the words of the STITCHED CIGARs, in which neighbouring
 * match runs are merged, and cigar_off[n] is that number -- a call with that capacity succeeds.  The error comes after the stitching: out[] and
 * status[] are already written then; cigar and cigar_off[0 .. n - 1] are not. */
typedef struct {
	uint32_t ksz;        /* k-mer size, values above 15 mean 15 (bsalign.h:1217); the CLI default is 13 (main.c:141) */
	uint32_t threads;    /* host threads for chaining and stitching; 0 = all hardware threads (or $BSA_KMER_THREADS) */
} bsa_kmer_params_t;

int bsa_kmer_edit_batch(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                        const uint64_t *qoff, const uint32_t *qlen,
                        const uint64_t *toff, const uint32_t *tlen, size_t n,
                        const bsa_kmer_params_t *par,
                        bsa_result_t *out, uint32_t *cigar, size_t cigar_cap_words,
                        uint64_t *cigar_off, uint32_t *status);

/* The host-only pieces of the above, usable without a GPU.
 * bsa_kmer_chain   : anchors of one pair in query order, maps[i] = query offset << 32 | target offset of the k-mer
 *                    (the reference's `maps`, bsalign.h:1431-1433); returns their number, 0 when the pair has to be
 *                    aligned as a whole, 0xFFFFFFFF when cap is too small (min(qlen, tlen) always suffices).
 * bsa_kmer_segments: the alignments the reference would run for these anchors (bsalign.h:1451-1530), at most kmap + 1.
 * bsa_kmer_assemble: result and CIGAR of the pair from the results of its segments. */
#define BSA_KMER_SEG_REVERSED 0x100u   /* head segment: both sequences are aligned reversed, SEQALIGN_MODE_KMER (bsalign.h:1489-1499) */
typedef struct {
	uint32_t qb, qe, tb, te;   /* the segment aligns query[qb, qe) with target[tb, te); a reversed head has qb = tb = 0 */
	uint32_t mode;             /* BSA_MODE_GLOBAL | BSA_MODE_EXTEND, optionally | BSA_KMER_SEG_REVERSED */
	uint32_t ml;               /* anchor matches emitted in front of this segment's CIGAR */
} bsa_kmer_seg_t;
uint32_t bsa_kmer_chain(uint32_t ksz, const uint8_t *q, uint32_t qlen, const uint8_t *t, uint32_t tlen, uint64_t *maps, uint32_t cap);
uint32_t bsa_kmer_segments(uint32_t ksz, const uint64_t *maps, uint32_t kmap, uint32_t qlen, uint32_t tlen, bsa_kmer_seg_t *segs);
int      bsa_kmer_assemble(const bsa_kmer_seg_t *segs, uint32_t nseg, const bsa_result_t *seg_out, const uint32_t *seg_cigar,
                           const uint64_t *seg_cigar_off, bsa_result_t *out, uint32_t *cigar, uint64_t cigar_cap_words, uint64_t *cigar_words);

/* bsa_kmer_chain_batch: the anchors of n pairs, chained on the DEVICE (bsa_kmer_dev.hip: one workgroup a pair -- k-mer extraction, radix sort, unique
 *                    same-strand hits, longest increasing subsequence, diagonal filter, both coverage tests).  All pointers are HOST memory (uploads,
 *                    runs, downloads, synchronises).  Pair k's anchors are maps[maps_off[k] .. maps_off[k + 1]) in query order, maps[i] = query
 *                    offset << 32 | target offset: exactly the count and the words bsa_kmer_chain(ksz, q, qlen, t, tlen, ...) returns for that pair.
 *                    Example: q = t = 100 random bases, ksz 13: up to 88 anchors i << 32 | i (those of k-mers that occur once).
 *                    0 anchors = align the whole pair globally.  ksz above 15 means 15; ksz == 0 or a sequence shorter than ksz: no anchors.
 *                    status (may be NULL): BSA_ST_EMPTY for qlen == 0 or tlen == 0, BSA_ST_BAD_BASE for a base code above 3; both get no anchors
 *                    (bsa_kmer_chain would chain the bytes of a bad-base pair; bsa_kmer_edit_batch2 does that, see below).
 *                    maps_cap (64-bit words) too small: BSA_E_CIGAR_CAP, maps_off[n] = the words needed, maps untouched; n = 0 is fine.
 *                    The device route takes every pair with qlen + tlen <= 262144; a longer pair, or one whose slice (about 17 bytes a base)
 *                    exceeds bsa_ctx_set_workspace_limit, is chained by the host code inside the same call -- same words, the caller sees no
 *                    difference but bsa_ctx_last_kmer_chain_ms.  Pairs go in chunks when the workspace does not hold them all.
 *                    Takes 1 B/base blobs and no strand marks: it IS bsa_kmer_chain_batch2 with flags 0, which takes BSA_MODE_SEQ2BIT blobs and
                    BSA_MODE_QSTRAND marks.  Neither takes device pointers: the form for a resident blob is bsa_kmer_chain_plan_create / bsa_kmer_chain_run below.
 * bsa_kmer_chain_batch2: the same call with `flags`, a subset of BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND | BSA_KMER_STRAND_AUTO (any other bit: BSA_E_ARG); the
 *                    first two mean exactly what they mean for bsa_align_batch, the third is described at its definition below.  SEQ2BIT: seqs are BaseBank.bits words, qoff / toff BASE offsets (any offset), seqs_bytes a multiple of
 *                    8 and off + len <= 4 * seqs_bytes, else BSA_E_ARG; BSA_ST_BAD_BASE cannot occur.  QSTRAND: bit 63 of qoff[k]
 *                    (BSA_QOFF_REVCOMP) marks pair k, which then chains q', q'[i] = 3 - q[qlen - 1 - i], against t; bounds are tested on the masked
 *                    offset, and without the flag bit 63 is an offset outside the blob (BSA_E_ARG).  maps, maps_off and status are bit-identical to
 *                    bsa_kmer_chain_batch on a 1 B/base blob in which the caller stored q' (or q) and t -- the query offsets in the anchor words are
 *                    positions in q'; the k-mer at q'[i, i + ksz) is the reverse complement of stored bases [qlen - ksz - i, qlen - i).  A batch with
 *                    QSTRAND and no pair marked returns what the plain call returns; a marked pair whose stored 1 B/base query holds a code above 3
 *                    has no q': BSA_ST_BAD_BASE and no anchors, as for the unmarked pair.  BSA_E_CIGAR_CAP / maps_off[n] as above.
 *                    Example: a read r of 2 000 bases is stored ONCE at offset 0; target A at offset 2000 overlaps it on the forward strand, target
 *                    B = the reverse complement of r (B[i] = 3 - r[1999 - i]) at offset 4000.  n = 2, qlen = tlen = {2000, 2000},
 *                    qoff = {0, 0 | BSA_QOFF_REVCOMP}, toff = {2000, 4000}, flags = BSA_MODE_QSTRAND.  Pair 1 chains q' = B against B: its anchors
 *                    are i << 32 | i for the positions i whose k-mer occurs once (nearly all of 0 .. 1987 at ksz 13) -- without the mark the pair
 *                    has no anchors at all, the chainer keeps same-strand k-mers only.  Pair 0 is what it is without the flag.
 *                    On the device only the first stage (k-mer extraction) sees the flags: a marked query is read mirrored with the roles of the
 *                    forward and the reverse-complement k-mer swapped; a packed k-mer comes from the one or two words that hold it, and nothing is
 *                    read in front of the word that holds a read's first base nor behind the one that holds its last.  A packed read goes up as
 *                    the words that hold it, a quarter of the bytes.  Pairs the device route does not take are chained by the host code on a
 *                    per-pair decoded copy: the same words.  bsa_ctx_last_kmer_chain_ms keeps its meaning.
 *                    Out of scope for the k-mer calls: BSA_MODE_CIGAR_EQX and BSA_MODE_SCORE_ONLY, a device-pointer or plan form of bsa_kmer_edit_batch2 (the
 *                    chain call has one: bsa_kmer_chain_plan_create / bsa_kmer_chain_run), the bsalign-hip CLI and the compat layer (both keep 1 B/base
 *                    forward-strand queries). */
int bsa_kmer_chain_batch(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                         const uint64_t *qoff, const uint32_t *qlen,
                         const uint64_t *toff, const uint32_t *tlen, size_t n,
                         uint32_t ksz, uint64_t *maps, size_t maps_cap,
                         uint64_t *maps_off /* n + 1 */, uint32_t *status /* may be NULL */);
int bsa_kmer_chain_batch2(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                          const uint64_t *qoff, const uint32_t *qlen,
                          const uint64_t *toff, const uint32_t *tlen, size_t n,
                          uint32_t ksz, uint64_t *maps, size_t maps_cap,
                          uint64_t *maps_off /* n + 1 */, uint32_t *status /* may be NULL */, uint32_t flags);

#define BSA_KMER_CHAIN_DEVICE 1u    /* flag of bsa_kmer_edit_batch2: step 1 of the batch (chains, then segment lists) takes its anchors from the device
                                       chainer above instead of the host threads.  Records, CIGAR words, cigar_off and status are bit-identical to
                                       bsa_kmer_edit_batch for ANY input: a pair with a base code above 3 is chained on its bytes exactly as the host
                                       code does, an empty pair has no anchors either way, and a pair above the device route's size limit is chained
                                       by the host inside the call.  bsa_kmer_segments, the two edit batches and bsa_kmer_assemble are the same code.
                                       Example: bsa_kmer_edit_batch2(ctx, ..., &par, out, cigar, cap, cigar_off, status, BSA_KMER_CHAIN_DEVICE).
                                       flags == 0 IS bsa_kmer_edit_batch (which calls this function with 0).
                                       flags may also carry BSA_MODE_SEQ2BIT and BSA_MODE_QSTRAND (0x800, 0x2000: no collision with bit 0), with or
                                       without BSA_KMER_CHAIN_DEVICE, with the meaning and the argument rules given at bsa_kmer_chain_batch2.  Records
                                       (qb / qe in q' coordinates), CIGAR words, cigar_off and status are then bit-identical to bsa_kmer_edit_batch on a
                                       1 B/base blob in which the caller stored q' (or q) and t, on either chain route.  The gap segments stay views into
                                       the caller's blob (gap [qb, qe) of a marked pair is stored bases [qlen - qe, qlen - qb) with BSA_QOFF_REVCOMP set,
                                       and bsa_edit_batch runs with the same flags); heads and tails are decoded per pair on the host threads.  One
                                       definition: a marked pair whose stored 1 B/base query holds a code above 3 has no q' -- BSA_ST_BAD_BASE, an
                                       all-zero record, no CIGAR words; unmarked pairs with such a code behave as without the flags.
                                       BSA_KMER_STRAND_AUTO (below) is the fourth flag.
                                       Any other bit is BSA_E_ARG: no BSA_MODE_CIGAR_EQX, BSA_MODE_SCORE_ONLY or other BSA_MODE_* flag is taken. */
#define BSA_KMER_STRAND_AUTO 2u     /* flag of bsa_kmer_chain_batch2 and bsa_kmer_edit_batch2 (no collision with BSA_KMER_CHAIN_DEVICE 1, BSA_MODE_SEQ2BIT
                                       0x800, BSA_MODE_QSTRAND 0x2000): the call FINDS each pair's strand.  With q the stored query, q' its reverse
                                       complement (q'[i] = 3 - q[qlen - 1 - i]), F the anchors bsa_kmer_chain returns for (q, t) and R those for (q', t),
                                       pair k is reverse exactly when |R| > |F|; a tie is forward, 0 against 0 included.  A reverse pair has
                                       BSA_ST_REVCOMP in status[k], which is why status == NULL is BSA_E_ARG with the flag; together with
                                       BSA_MODE_QSTRAND it is BSA_E_ARG, and bit 63 of qoff stays part of the offset (outside the blob: BSA_E_ARG).
                                       Combines with BSA_MODE_SEQ2BIT.  An empty pair, a sequence shorter than ksz and a 1 B/base pair with a code
                                       above 3 are forward and otherwise return what the call without the flag returns.
                                       bsa_kmer_chain_batch2: maps, maps_off and status & ~BSA_ST_REVCOMP are bit-identical to the call with
                                       BSA_MODE_QSTRAND and exactly the reverse pairs marked (query offsets of a reverse pair are positions in q');
                                       BSA_E_CIGAR_CAP and maps_off[n] count the chosen strand's anchors.  On the device both strands share the one
                                       sort: a run of two records with equal strand bits is a forward hit, with different bits (or a k-mer that is its
                                       own reverse complement) a hit against q'.
                                       bsa_kmer_edit_batch2, with or without BSA_KMER_CHAIN_DEVICE: step 1 chooses the strands, the rest is the
                                       BSA_MODE_QSTRAND route on a private marked copy of qoff -- records (qb / qe in q' coordinates), CIGAR words and
                                       cigar_off bit-identical to that call, status with BSA_ST_REVCOMP OR-ed in for the reverse pairs.
                                       Taken by bsa_kmer_chain_plan_create (device pointers, below); not by bsa_align_* / bsa_edit_* or their plans, the
                                       CLI or the compat layer.  To align the
                                       pairs on the strand found here, copy the bit into qoff and use BSA_MODE_QSTRAND there:
                                           bsa_kmer_chain_batch2(ctx, ..., qoff, ..., maps, cap, maps_off, status, BSA_KMER_STRAND_AUTO);
                                           for(k = 0; k < n; k++) if(status[k] & BSA_ST_REVCOMP) qoff[k] |= BSA_QOFF_REVCOMP;
                                           par.mode |= BSA_MODE_QSTRAND; bsa_align_batch(ctx, ..., qoff, ..., &par, out, cigar, cap, cigar_off, status); */
int bsa_kmer_edit_batch2(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                         const uint64_t *qoff, const uint32_t *qlen,
                         const uint64_t *toff, const uint32_t *tlen, size_t n,
                         const bsa_kmer_params_t *par,
                         bsa_result_t *out, uint32_t *cigar, size_t cigar_cap_words,
                         uint64_t *cigar_off, uint32_t *status, uint32_t flags);

/* bsa_kmer_chain_plan_* : bsa_kmer_chain_batch2 in the two-phase form for resident data, as bsa_align_plan_* is to bsa_align_batch: the plan takes the HOST
 *                    metadata once, bsa_kmer_chain_run takes DEVICE pointers for the sequence blob and all outputs.
 * flags, ksz       : flags is a subset of BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND | BSA_KMER_STRAND_AUTO, each meaning exactly what it means for
 *                    bsa_kmer_chain_batch2; any other bit is BSA_E_ARG, and so is QSTRAND together with STRAND_AUTO.  ksz above 15 means 15, ksz == 0 gives no
 *                    anchors anywhere (the status words are written all the same).  n == 0 is fine: the run writes d_maps_off[0] = 0.  With STRAND_AUTO
 *                    d_status == NULL is BSA_E_ARG from the run; with SEQ2BIT a d_seqs that is not 8-byte aligned is BSA_E_ARG from the run.
 * the blob         : the kernels read the caller's blob IN PLACE.  qoff / toff are the caller's own offsets into d_seqs, bytes, or base offsets with SEQ2BIT;
 *                    with QSTRAND bit 63 of qoff[k] is the strand bit.  Like bsa_align_plan_create the plan takes no blob size and cannot check bounds:
 *                    that every read lies inside the blob is a PRECONDITION.  With SEQ2BIT nothing is read in front of the word that holds a read's first
 *                    base nor behind the one that holds its last.
 * results          : d_maps[d_maps_off[k] .. d_maps_off[k + 1]), all of d_maps_off and d_status (BSA_ST_REVCOMP under STRAND_AUTO included) are bit-identical
 *                    to what bsa_kmer_chain_batch2 returns for the same pairs and flags on a host copy of the blob -- hence to per-pair bsa_kmer_chain on
 *                    q or q'.  A pair with a base code above 3 gets BSA_ST_BAD_BASE and no anchors, an empty pair BSA_ST_EMPTY and none.
 * no host route    : a run cannot read device memory on the host and stay asynchronous, so bsa_kmer_chain_plan_create returns BSA_E_UNSUPPORTED when a pair has
 *                    qlen + tlen > 262144, or when a pair's slice alone (about 16 bytes a base) exceeds the workspace limit in force at creation
 *                    (bsa_ctx_set_workspace_limit); bsa_last_error names the first such pair.  Send those pairs through bsa_kmer_chain_batch2.
 * asynchronous     : bsa_kmer_chain_run is asynchronous on the context stream and returns BSA_OK before a kernel has run.  It copies nothing between host
 *                    and device and does not synchronise: the pair tables went up when the plan was made, into memory the plan owns, and so were the
 *                    workspace chunks decided (bsa_kmer_chain_plan_chunks; one chunk unless the workspace limit forces more).  The workspace is the
 *                    context's scratch: a run that has to grow it may synchronise once.
 * arena            : the run cannot report an arena that is too small; the caller compares d_maps_off[n] with maps_cap afterwards
 *                    (bsa_kmer_chain_words_bound gives a maps_cap that always suffices).  For ANY maps_cap, 0 with a non-NULL d_maps and a NULL d_maps with
 *                    maps_cap 0 (a count-only run) included:
 *                      - all n + 1 entries of d_maps_off and all n of d_status are those of a run with a large arena, and every run writes every one of
 *                        them, whatever the buffers held;
 *                      - d_maps_off[n] is the number of words needed;
 *                      - pair k's words are written if and only if d_maps_off[k + 1] <= maps_cap, otherwise no word of its range is touched (the gather
 *                        writes straight into the caller's arena, in pair order: unlike bsa_align_run's, WHICH pairs are present is specified);
 *                      - no word at or above maps_cap, nor at or above d_maps_off[n], is touched.
 * re-run           : a run leaves nothing behind that a later run reads.  A plan may be run again on other sequences of the same lengths, after a short run,
 *                    and in turn with other chain, align and edit plans of the same context.  Destroy a plan before its context.
 * timing           : bsa_ctx_last_kmer_chain_ms after bsa_ctx_sync: the summed event time of the last run's chunks, pairs_on_device = n, pairs_on_host = 0.
 * Example          : a shard from bsa_shard_scatter, or bsa_synth_pairs_dev's blob, stays where it is --
 *                      bsa_kmer_chain_plan_create(ctx, qoff, qlen, toff, tlen, n, 13, BSA_KMER_STRAND_AUTO, &plan);
 *                      cap = bsa_kmer_chain_words_bound(qlen, tlen, n);             (hipMalloc d_maps: cap words, d_maps_off: n + 1, d_status: n)
 *                      bsa_kmer_chain_run(plan, d_seqs, d_maps, cap, d_maps_off, d_status); bsa_ctx_sync(ctx);
 *                    then 4 bytes a pair come down (d_status), BSA_ST_REVCOMP goes into qoff[k] as BSA_QOFF_REVCOMP, and bsa_align_plan_create with
 *                    BSA_MODE_QSTRAND aligns the same resident blob on the strands found.
 * Out of scope     : a resident form of bsa_kmer_edit_batch2 (its edit plans need the segments' lengths on the host), a host fallback inside the run. */
typedef struct bsa_kmer_chain_plan bsa_kmer_chain_plan_t;
int      bsa_kmer_chain_plan_create(bsa_ctx_t *ctx, const uint64_t *qoff, const uint32_t *qlen,
                                    const uint64_t *toff, const uint32_t *tlen, size_t n,
                                    uint32_t ksz, uint32_t flags, bsa_kmer_chain_plan_t **out);
void     bsa_kmer_chain_plan_destroy(bsa_kmer_chain_plan_t *plan);
uint32_t bsa_kmer_chain_plan_chunks(const bsa_kmer_chain_plan_t *plan);      /* workspace chunks one run goes through */
uint64_t bsa_kmer_chain_words_bound(const uint32_t *qlen, const uint32_t *tlen, size_t n);  /* sum of min(qlen, tlen): a maps_cap that always suffices; host only, no GPU */
int      bsa_kmer_chain_run(bsa_kmer_chain_plan_t *plan, const uint8_t *d_seqs,
                            uint64_t *d_maps, size_t maps_cap, uint64_t *d_maps_off /* n + 1 */, uint32_t *d_status /* n, may be NULL */);

/* bsa_cigar_windows_* : every alignment cut at the borders of windows of `window` target bases -- what a windowed polisher needs between its read-to-draft
 *                    alignment and its per-window POA: for every read, and for every window its alignment crosses, the read interval that belongs to that
 *                    window, from the first to the last aligned column inside it.  A pass over the PUBLIC outputs of a run (records, CIGAR words, offsets:
 *                    bsa_cigar_windows.hip) and nothing else, so it takes what bsa_align_run / bsa_align_batch and bsa_edit_run / bsa_edit_batch return in
 *                    any mode and on any kernel route: plain and BSA_MODE_CIGAR_EQX words, BSA_MODE_QSTRAND pairs (query positions are then in q', as
 *                    the record's are).  It touches no plan and changes no existing call.
 * columns          : every position is 0-based.  The alignment of pair k starts at (t, q) = (out[k].tb, out[k].qb) and follows its words
 *                    cigar[cigar_off[k] .. cigar_off[k + 1]).  A unit of an M, = or X word aligns target base t with query base q and then advances both: a
 *                    DIAGONAL COLUMN (t, q).  A unit of I advances q, a unit of D advances t, any other op code takes no step.
 * windows          : window m is the target positions [m w, (m + 1) w).  Pair k has nw_k = 0 windows when tb < 0 (score-only records), te <= tb or it has
 *                    no words; otherwise m0 = tb / w, m1 = (te - 1) / w, nw_k = m1 - m0 + 1, and record r of the pair speaks of window m0 + r.
 * a record         : bsa_window_t holds the first and the last diagonal column whose t lies in the window; all four fields are BSA_WINDOW_NONE when the
 *                    window holds none (a deletion covers it whole).  The read's piece for the window is q[q_first, q_last + 1).
 * Examples         : w = 10, tb = 7, qb = 3, words 5M 2I 4D 6M, te = 22: windows 0..2 --
 *                      window 0 {7, 3, 9, 5}; window 1 {10, 6, 19, 13} (the deletion t 12..15 lies inside it, the query jumps from 7 to 10 over the
 *                      insertion); window 2 {20, 14, 21, 15}.
 *                    w = 10, tb = 0, qb = 0, words 3M 25D 3M, te = 31: windows 0..3 --
 *                      window 0 {0, 0, 2, 2}; window 1 NONE; window 2 {28, 3, 29, 4}; window 3 {30, 5, 30, 5}.
 * inconsistent     : the words are the caller's own arrays and may consume more or less target than te - tb.  Columns in a window above m1 are ignored
 *                    (and, a record's positions being int32, so are columns at t >= 2^31); windows the words never reach are NONE; nothing is ever
 *                    written outside the pair's nw_k records.  Query positions are summed modulo 2^32.
 * _bound           : host only, no GPU.  The sum of ceil(tlen[k] / window) over the pairs: a win_cap that always suffices (0 for window == 0).
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation.  It may grow the context's scratch
 *                    once (4 bytes a pair for the counts; a run that has to grow it may synchronise once).  window == 0 and a NULL d_win_off, a NULL d_out,
 *                    d_cigar or d_cigar_off with n > 0, or a win_cap without a d_win are BSA_E_ARG.  n == 0 writes d_win_off[0] = 0.
 *                    Precondition: the run that produced d_cigar was complete (its cigar_cap_words >= d_cigar_off[n]): the words of every pair are read.
 * arena            : that of bsa_kmer_chain_run.  For ANY win_cap, 0 with a non-NULL d_win and a NULL d_win with win_cap 0 (a count-only run) included:
 *                      - all n + 1 entries of d_win_off are those of a run with a large arena, and every run writes every one of them;
 *                      - d_win_off[n] is the number of records needed;
 *                      - pair k's records are written if and only if d_win_off[k + 1] <= win_cap, otherwise none of its range is touched;
 *                      - no record at or above win_cap, nor at or above d_win_off[n], is touched;
 *                      - every record of a written pair is written, NONE records included.
 *                    A run leaves nothing behind that a later run reads.
 * _batch           : all pointers are HOST memory: uploads the records and the words cigar[cigar_off[0] .. cigar_off[n]), runs, downloads, synchronises.
 *                    win_off as from bsa_kmer_chain_batch: all n + 1 entries are written; win_cap too small: BSA_E_CIGAR_CAP, win_off[n] = the records
 *                    needed, win untouched.  A cigar_off that decreases is BSA_E_ARG.
 * Example          : a polisher's step on resident reads --
 *                      bsa_align_run(plan, d_seqs, d_out, d_cigar, cigar_cap, d_cigar_off, d_status);
 *                      cap = bsa_cigar_windows_bound(tlen, n, 500);                 (hipMalloc d_win: cap records, d_win_off: n + 1)
 *                      bsa_cigar_windows_run(ctx, d_out, d_cigar, d_cigar_off, n, 500, d_win, cap, d_win_off); bsa_ctx_sync(ctx);
 *                    then 16 bytes a window come down instead of the CIGAR arena. */
#define BSA_WINDOW_NONE 0xFFFFFFFFu
typedef struct { uint32_t t_first, q_first, t_last, q_last; } bsa_window_t;
uint64_t bsa_cigar_windows_bound(const uint32_t *tlen, size_t n, uint32_t window);
int      bsa_cigar_windows_run(bsa_ctx_t *ctx, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                               size_t n, uint32_t window, bsa_window_t *d_win, size_t win_cap, uint64_t *d_win_off /* n + 1 */);
int      bsa_cigar_windows_batch(bsa_ctx_t *ctx, const bsa_result_t *out, const uint32_t *cigar, const uint64_t *cigar_off,
                                 size_t n, uint32_t window, bsa_window_t *win, size_t win_cap, uint64_t *win_off /* n + 1 */);

/* bsa_window_pieces_* : the window records turned window-major, with the reads' bases -- what a windowed polisher's POA wants: for every window of the draft, the
 *                    pieces of the reads that cross it, as 1 B/base codes in the strand that was aligned.  bsa_cigar_windows_* leaves, for every read, the
 *                    windows it crosses; this pass buckets those records by window and gathers q'[q_first, q_last + 1) of every one of them from the resident
 *                    blob, so that neither the blob nor the window records have to come down and no host code slices, reverse-complements or unpacks a read.
 *                    A pass over public outputs (bsa_window_pieces.hip): it touches no plan and changes no existing call.
 * inputs           : d_seqs, d_qoff, d_qlen are the blob and the queries as the aligner's plan took them (BSA_MODE_SEQ2BIT and BSA_MODE_QSTRAND in `flags` as
 *                    in that plan's mode); d_win, d_win_off are what a COMPLETE bsa_cigar_windows_run left for the same n pairs (win_cap >= d_win_off[n]).
 * global windows   : gbase[k] is the global index of the window that holds target position 0 of pair k's target sequence.  The caller makes it: an exclusive
 *                    sum of ceil(target length / window) over its targets, looked up per pair -- so a pair's target slice must start on a window border
 *                    of its draft.  Windows are numbered 0 .. nwin - 1.
 * pieces           : record i of d_win, belonging to pair k (d_win_off[k] <= i < d_win_off[k + 1]), is a PIECE if and only if
 *                      t_first != BSA_WINDOW_NONE,  t_first <= t_last,  q_first <= q_last < qlen[k]  and  g = gbase[k] + t_first / window < nwin
 *                    (g formed without wrapping: a gbase[k] >= nwin has no piece).  The piece belongs to window g.  Every other record is ignored: NONE
 *                    records, and anything inconsistent in arrays that are the caller's own.  Nothing is ever read outside a read's qlen bases because of
 *                    a record.
 * order            : the pieces of window g are piece[piece_off[g] .. piece_off[g + 1]), in ascending order of their record index i (on what
 *                    bsa_cigar_windows_run writes a pair has one record a window, so this is ascending pair index).  The order is part of the contract: the
 *                    output of a call is a function of its inputs alone and identical from run to run.
 * a piece          : bsa_piece_t: pair = k; q_first = the record's, a position in q' (the strand that was aligned: the record's coordinates); len = q_last -
 *                    q_first + 1; t_first, t_last = the record's; reserved = 0; base_off: the piece's codes are bases[base_off .. base_off + len).
 * bases            : the bases of window g are bases[base_off[g] .. base_off[g + 1]): its pieces one after another in that order, no padding.  A piece's
 *                    base_off is absolute (an index into bases, not into the window's range).
 * codes            : one base a byte, q'[q_first .. q_first + len), q' the query as the aligner saw it through its staging kernels.  With s the stored query of
 *                    qlen[k] bases: an unmarked pair gives s[j] & 3; a pair marked with BSA_QOFF_REVCOMP (only with BSA_MODE_QSTRAND in flags) gives
 *                    (s[qlen - 1 - j] & 3) ^ 3; with BSA_MODE_SEQ2BIT the blob is BaseBank.bits words and qoff are base offsets, layout and rules as for
 *                    the align calls (d_seqs 8-byte aligned, bsa_window_pieces_run: BSA_E_ARG otherwise).  Nothing is read in front of the word (byte)
 *                    that holds a read's first base nor behind the one that holds its last.
 * flags            : a subset of BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND; any other bit is BSA_E_ARG.  Without BSA_MODE_QSTRAND bit 63 of qoff is part of the
 *                    offset (bsa_window_pieces_batch: BSA_E_ARG, offset outside the blob; bsa_window_pieces_run: a broken precondition).
 * Example          : window = 4, one target of 12 bases (windows 0..2, nwin = 3), two pairs on it, gbase = {0, 0}, flags = BSA_MODE_QSTRAND.
 *                      pair 0: stored ACGTACGTAC (0 1 2 3 0 1 2 3 0 1), qlen 10, unmarked: q' = the stored bases.
 *                              records 0..2: {1, 0, 3, 2}  {4, 3, 7, 6}  {8, 7, 10, 9}                     (t_first, q_first, t_last, q_last; windows 0, 1, 2)
 *                      pair 1: stored AACCGGT (0 0 1 1 2 2 3), qlen 7, marked: q' = ACCGGTT (0 1 1 2 2 3 3).
 *                              records 3..4: {5, 0, 7, 2}  {8, 3, 11, 6}                                    (windows 1, 2);  d_win_off = {0, 3, 5}
 *                    gives piece_off = {0, 1, 3, 5}, base_off = {0, 3, 10, 17} and
 *                      window 0: {pair 0, q_first 0, len 3, t 1..3,  base_off 0}   codes 0 1 2
 *                      window 1: {pair 0, q_first 3, len 4, t 4..7,  base_off 3}   codes 3 0 1 2        (record 1)
 *                                {pair 1, q_first 0, len 3, t 5..7,  base_off 7}   codes 0 1 1          (record 3: q'[0, 3), stored bases 6, 5, 4 complemented)
 *                      window 2: {pair 0, q_first 7, len 3, t 8..10, base_off 10}  codes 3 0 1          (record 2)
 *                                {pair 1, q_first 3, len 4, t 8..11, base_off 13}  codes 2 2 3 3        (record 4)
 *                    bases = 0 1 2 | 3 0 1 2 0 1 1 | 3 0 1 2 2 3 3.
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the context's
 *                    scratch (16 bytes a window for the counters, 16 bytes for every piece of piece_cap while both caps are non-zero; a run that has to
 *                    grow it may synchronise once; BSA_E_NOMEM when it cannot).
 * arenas (_run)    : the contract of bsa_kmer_chain_run and bsa_cigar_windows_run with the window as the unit and two arenas.  For ANY piece_cap and bases_cap,
 *                    0 with a non-NULL arena and a NULL arena with cap 0 (a count-only run) included:
 *                      - all nwin + 1 entries of d_piece_off and of d_base_off are those of a run with large arenas, and every run writes every one of them;
 *                      - d_piece_off[nwin] and d_base_off[nwin] are the pieces and the bytes a complete run needs;
 *                      - window g is written if and only if d_piece_off[g + 1] <= piece_cap and d_base_off[g + 1] <= bases_cap;
 *                      - a written window is written whole: every field of every piece record (reserved = 0) and every base;
 *                      - a window that is not written has no byte of either of its ranges touched;
 *                      - nothing at or above either cap, nor at or above either total, is touched;
 *                      - the caller's arenas are never used as scratch for windows that do not fit.
 *                    A run leaves nothing behind that a later run reads.  Caps that always suffice: d_win_off[n] pieces (bsa_cigar_windows_bound bounds
 *                    them) and the sum of qlen bytes when, as on what bsa_cigar_windows_run writes, a pair's pieces do not overlap.
 * _batch           : all pointers are HOST memory: checks every (qoff & ~strand bit) + qlen against seqs_bytes (4 * seqs_bytes bases with BSA_MODE_SEQ2BIT,
 *                    seqs_bytes then a multiple of 8) -- a read outside the blob is BSA_E_ARG, as is a win_off that decreases -- uploads the blob, the queries
 *                    and the records win[win_off[0] .. win_off[n]), runs, downloads, synchronises.  Both offset arrays are always written whole; if either cap
 *                    is too small: BSA_E_CIGAR_CAP, piece_off[nwin] and base_off[nwin] say what is needed, piece and bases are untouched.
 * errors (both)    : window == 0; a NULL piece_off or base_off; NULL inputs with n > 0; a cap without its arena; n or nwin above 0xFFFFFFF0: BSA_E_ARG.
 *                    n == 0 or nwin == 0 is fine: the offsets are all 0.
 * Example          : a polisher's step on resident reads --
 *                      bsa_align_run(plan, d_seqs, d_out, d_cigar, cigar_cap, d_cigar_off, d_status);
 *                      bsa_cigar_windows_run(ctx, d_out, d_cigar, d_cigar_off, n, 500, d_win, cap, d_win_off);
 *                      bsa_window_pieces_run(ctx, d_seqs, d_qoff, d_qlen, d_win, d_win_off, n, 500, d_gbase, nwin, plan_mode & (BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND),
 *                                            d_piece, cap, d_piece_off, d_bases, sum_qlen, d_base_off); bsa_ctx_sync(ctx);
 *                    then 32 bytes a piece and the pieces' codes come down, window by window, instead of the window records and the blob. */
typedef struct {
	uint32_t pair;             /* k: the pair the piece comes from */
	uint32_t q_first;          /* first base of the piece, a position in q' (the strand that was aligned: the record's coordinates) */
	uint32_t len;              /* q_last - q_first + 1 */
	uint32_t t_first, t_last;  /* the window record's first and last aligned target position */
	uint32_t reserved;         /* 0 */
	uint64_t base_off;         /* the piece's codes are bases[base_off .. base_off + len) */
} bsa_piece_t;                 /* 32 bytes */
int      bsa_window_pieces_run(bsa_ctx_t *ctx,
                               const uint8_t *d_seqs, const uint64_t *d_qoff, const uint32_t *d_qlen,
                               const bsa_window_t *d_win, const uint64_t *d_win_off, size_t n,
                               uint32_t window, const uint64_t *d_gbase /* n */, size_t nwin, uint32_t flags,
                               bsa_piece_t *d_piece, size_t piece_cap, uint64_t *d_piece_off /* nwin + 1 */,
                               uint8_t *d_bases, size_t bases_cap, uint64_t *d_base_off /* nwin + 1 */);
int      bsa_window_pieces_batch(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes,
                                 const uint64_t *qoff, const uint32_t *qlen,
                                 const bsa_window_t *win, const uint64_t *win_off, size_t n,
                                 uint32_t window, const uint64_t *gbase, size_t nwin, uint32_t flags,
                                 bsa_piece_t *piece, size_t piece_cap, uint64_t *piece_off,
                                 uint8_t *bases, size_t bases_cap, uint64_t *base_off);

/* bsa_window_select_* : which of a window's pieces take part -- the depth knob and the read filter of a windowed polisher.  bsa_window_pieces_* makes every piece
 *                    that crosses a window a row of its MSA; the two passes that cost the most (bsa_window_msa_*, bsa_window_cns_*) grow linearly with that
 *                    depth, one deep window (a collapsed repeat) holds a whole batch up, and a badly aligned read votes like any other.  This pass drops the
 *                    pieces that are too short and those of pairs whose identity is too low, and keeps at most max_depth of the rest, in front of any
 *                    expensive work.  A pass over public outputs (bsa_window_select.hip): it touches no plan and changes no existing call.
 * inputs           : d_piece, d_piece_off (nwin + 1) are what bsa_window_pieces_run left, piece_cap the room of d_piece; d_out (n records, or NULL) what the
 *                    aligner left for the pairs the pieces speak of.  d_sel must not overlap d_piece.
 * windows          : window g's pieces are piece[piece_off[g] .. piece_off[g + 1]).  A window with piece_off[g + 1] > piece_cap or piece_off[g + 1] <
 *                    piece_off[g] has no pieces (the rule of bsa_window_msa_* for depth 0).  This test is the only door to the piece records: nothing the
 *                    caller puts into the offsets makes the pass read outside piece_cap records.
 * candidates       : piece j of window g is a CANDIDATE if and only if
 *                      t_first <= t_last  and  len >= 1;
 *                      with sp = t_last - t_first (which cannot wrap):  min_span <= 1  or  sp >= min_span - 1;
 *                      and, if ident_den != 0 (the identity test; d_out == NULL is then BSA_E_ARG):  pair < n,  and with mat and aln read as int32 from
 *                      d_out[pair]:  aln > 0,  mat >= 0  and  (uint64)mat * ident_den >= (uint64)ident_num * (uint64)aln  (neither product can wrap).
 *                    Without the identity test `pair` is used in the hash below only, never as an index, and d_out is not read.
 * order            : candidate i is BETTER than candidate j if its sp is larger; or sp is equal and its h is smaller, h = mix32(pair ^ seed) with
 *                      mix32(x):  x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16;   (32-bit arithmetic)
 *                    or both are equal and i < j.  The hash is one of the pair, not of the piece: a read that wins a tie wins it in every window where it
 *                    ties, so neighbouring windows tend to keep the same reads.  (A rule by a piece's own indel balance would prefer the reads that agree
 *                    with the draft's length -- the one bias a polisher must not have.)
 * selected         : with C candidates, all of them if max_depth == 0 or C <= max_depth, otherwise the max_depth best.  d_ncand[g] = C.
 * output           : window g's selected records, copied verbatim -- all 32 bytes, base_off and reserved included -- in ascending j, are
 *                    sel[sel_off[g] .. sel_off[g + 1]); sel_src[i] is the index j in d_piece that record i came from; sel_off is the exclusive sum, in 64
 *                    bits, of the selected counts.  The output is a function of the inputs alone.
 * downstream       : d_sel and d_sel_off take the place of d_piece and d_piece_off in bsa_piece_cigars_run (d_npiece = d_sel_off + nwin, piece_cap = sel_cap)
 *                    and in bsa_window_msa_run; d_bases and bases_cap stay those bsa_window_pieces_run wrote -- the records' base_off are absolute and are
 *                    left alone (the bases of the dropped pieces stay where they are, unused).  With max_depth 0, min_span 0 and no identity test the
 *                    selected records of well-formed windows are the input records, and d_sel_off is d_piece_off rebased.
 * Example          : one window, seed 0, min_span 6, no identity test; the pieces as (pair, t_first..t_last):
 *                      j0 (0, 0..9)   j1 (1, 2..9)   j2 (2, 0..9)   j3 (3, 0..4)   j4 (4, 0..9)   j5 (5, 1..9)
 *                    j3 spans 5 columns and is no candidate: C = 5.  mix32 of the pairs 0, 2, 4 is 0x00000000, 0x30F4C306, 0x249CB285, so among the three
 *                    pieces with sp 9 the order is j0, j4, j2.  Selected, by max_depth:
 *                      0: {0, 1, 2, 4, 5}   1: {0}   2: {0, 4}   3: {0, 2, 4}   4: {0, 2, 4, 5}  (j5 with sp 8 goes before j1 with sp 7)
 *                    With seed 1, max_depth 2 gives {0, 2}.  Identity: with ident_num / ident_den = 4 / 5 a pair with (mat, aln) = (80, 100) or (8, 10)
 *                    passes, (79, 100) fails, (0, 0) fails.
 * arena            : the contract of bsa_window_pieces_run with one arena and the window as the unit.  For ANY sel_cap, 0 with a non-NULL d_sel and a NULL
 *                    d_sel with cap 0 (a count-only run) included:
 *                      - all nwin + 1 entries of d_sel_off are those of a run with a large arena and every run writes every one of them, and all nwin
 *                        entries of d_ncand if it is given;
 *                      - d_sel_off[nwin] is the number of records a complete run needs (piece_cap always suffices);
 *                      - window g's records are written, whole, if and only if d_sel_off[g + 1] <= sel_cap, with its d_sel_src entries if that array is given;
 *                      - a window that is not written has no byte of its range touched; nothing at or above sel_cap, nor at or above the total, is touched;
 *                      - the caller's arena is never used as scratch.
 *                    A run leaves nothing behind that a later run reads.
 * _run             : DEVICE pointers, `par` HOST memory that is read at the call; asynchronous on the context stream; no host/device copy, no synchronisation
 *                    -- except that it may grow the context's scratch (16 bytes a window and the scan's temporaries; a run that has to grow it may
 *                    synchronise once; BSA_E_NOMEM when it cannot).
 * _batch           : all pointers are HOST memory: uploads the piece_cap records, the offsets as they are (a piece_off that decreases is handled window by
 *                    window as stated above: it is no error) and, for the identity test, the n records; counts, downloads sel_off and ncand FIRST and
 *                    synchronises: sel_cap too small is BSA_E_CIGAR_CAP there, sel_off[nwin] = the records needed, sel and sel_src untouched.  Then the
 *                    selected records come down.
 * errors (both)    : a NULL ctx, par or d_sel_off; a NULL d_piece_off with nwin > 0; piece_cap without d_piece; sel_cap without d_sel; d_sel_src without
 *                    d_sel; ident_den != 0 without d_out; non-zero reserved; nwin, n, piece_cap or sel_cap above 0xFFFFFFF0: BSA_E_ARG.  nwin == 0 writes
 *                    d_sel_off[0] = 0 and nothing else.
 * Example          : a polisher's step on resident reads, at most 40 pieces a window of pairs that match in 7 of 10 columns or more --
 *                      bsa_window_pieces_run(ctx, d_seqs, d_qoff, d_qlen, d_win, d_win_off, n, 500, d_gbase, nwin, flags, d_piece, cap, d_piece_off, d_bases, bcap, ...);
 *                      bsa_select_params_t sp = { 40, 0, 7, 10, 0, { 0, 0, 0 } };
 *                      bsa_window_select_run(ctx, d_piece, d_piece_off, nwin, cap, d_out, n, &sp, d_sel, cap, d_sel_off, NULL, NULL);
 *                      bsa_piece_cigars_run(ctx, d_out, d_cigar, d_cigar_off, n, d_sel, d_sel_off + nwin, cap, d_pcig, cigar_cap + cap, d_pcig_off, NULL);
 *                      bsa_window_msa_run(ctx, d_sel, d_sel_off, nwin, cap, d_bases, bcap, d_pcig, ...);
 *                    and on as without the pass. */
typedef struct {
	uint32_t max_depth;             /* at most this many pieces a window; 0: no cap */
	uint32_t min_span;              /* a piece needs t_last - t_first + 1 >= min_span target columns; 0 and 1: no test */
	uint32_t ident_num, ident_den;  /* with d_out: the pair needs mat * ident_den >= ident_num * aln; ident_den 0: no test */
	uint32_t seed;                  /* decides among pieces of equal span */
	uint32_t reserved[3];           /* 0 */
} bsa_select_params_t;              /* 32 bytes */
int      bsa_window_select_run(bsa_ctx_t *ctx,
                               const bsa_piece_t *d_piece, const uint64_t *d_piece_off /* nwin + 1 */, size_t nwin, size_t piece_cap,
                               const bsa_result_t *d_out /* n, or NULL: no identity test */, size_t n,
                               const bsa_select_params_t *par /* HOST */,
                               bsa_piece_t *d_sel, size_t sel_cap, uint64_t *d_sel_off /* nwin + 1 */,
                               uint32_t *d_sel_src /* sel_cap, may be NULL */, uint32_t *d_ncand /* nwin, may be NULL */);
int      bsa_window_select_batch(bsa_ctx_t *ctx,
                                 const bsa_piece_t *piece, const uint64_t *piece_off /* nwin + 1 */, size_t nwin, size_t piece_cap,
                                 const bsa_result_t *out /* n, or NULL */, size_t n,
                                 const bsa_select_params_t *par,
                                 bsa_piece_t *sel, size_t sel_cap, uint64_t *sel_off /* nwin + 1 */,
                                 uint32_t *sel_src /* sel_cap, may be NULL */, uint32_t *ncand /* nwin, may be NULL */);

/* bsa_piece_cigars_* : every piece's own CIGAR words -- how the piece aligns to its window of the draft, which is what the POA's band placement takes as a
 *                    read's guide (bsa_pog_guide_t::sam, bsalign_poa.h).  bsa_window_pieces_* leaves, for every window, the reads' pieces and their codes;
 *                    the piece's alignment against the draft already exists: it is the stretch of its pair's CIGAR from the piece's first to its last
 *                    aligned column.  This pass cuts that stretch out for every piece, window by window, so that the CIGAR arena never has to come down.
 *                    A pass over public outputs (bsa_piece_cigars.hip): it touches no plan and changes no existing call, uses neither the window records
 *                    nor the window size, and so serves both aligners, plain and BSA_MODE_CIGAR_EQX words and BSA_MODE_QSTRAND pairs (positions in q').
 * inputs           : d_out, d_cigar, d_cigar_off are what a COMPLETE bsa_align_run / bsa_edit_run left for n pairs; d_piece and d_npiece = d_piece_off + nwin
 *                    are what a COMPLETE bsa_window_pieces_run left (its piece_cap >= d_piece_off[nwin]); piece_cap is the room of d_piece.
 * columns          : as in bsa_cigar_windows_*.  The alignment of pair k starts at (t, q) = (out[k].tb, out[k].qb); a unit of an M, = or X word is a DIAGONAL
 *                    COLUMN (t, q) and then advances both; a unit of I advances q, a unit of D advances t; any other op code takes no step.  t is summed in 64
 *                    bits, q modulo 2^32.  ALL of the pair's words count, also where they run on behind out[k].te.
 * a piece is cut   : piece j, with k = piece[j].pair, is CUT if and only if  k < n,  out[k].tb >= 0,  pair k has words (cigar_off[k + 1] > cigar_off[k]; a pair of
 *                    2^32 words or more counts as having none),  t_first <= t_last,  len >= 1,  and both (t_first, q_first) and (t_last, q_first + len - 1) are
 *                    diagonal columns of pair k's alignment (q_first + len - 1 modulo 2^32).  A cut piece has status 0.  Every other piece has no words and
 *                    status BSA_PIECE_ST_NOT_ON_PATH.  The pieces are the caller's own arrays: nothing inconsistent in them makes the pass read outside
 *                    pair k's words or write outside piece j's range.  On what bsa_cigar_windows_run and bsa_window_pieces_run write every piece is cut.
 * its words        : pair k's words in order, clipped to the units from the first of the two columns to the last, both included: a word that lies partly
 *                    outside keeps its op and the length that lies inside; words (or clippings) of length 0 and words of an op that takes no step are
 *                    dropped; nothing is merged (two adjacent M words stay two words); = and X stay = and X.  So the first and the last word are diagonal,
 *                    the lengths of the words that advance q sum to len (modulo 2^32) and those of the words that advance t to t_last - t_first + 1.
 * order            : piece j's words are pcig[pcig_off[j] .. pcig_off[j + 1]); j is the index bsa_window_pieces_run gave the piece (by window, then ascending
 *                    record), so window g's words are the contiguous range pcig[pcig_off[piece_off[g]] .. pcig_off[piece_off[g + 1]]).  The output is a
 *                    function of the inputs alone.
 * Example          : the first example of bsa_cigar_windows_*: tb = 7, qb = 3, words 5M 2I 4D 6M, cut at w = 10 into the pieces
 *                      {q_first 3, len 3, t 7..9}    -> 3M                 (the first three units of 5M)
 *                      {q_first 6, len 8, t 10..19}  -> 2M 2I 4D 4M        (the last two units of 5M, the whole gap words, the first four units of 6M)
 *                      {q_first 14, len 2, t 20..21} -> 2M                 (the last two units of 6M)
 *                    pcig_off = {0, 1, 5, 6}, status 0 0 0.  A piece {q_first 6, len 3, t 10..12} is not on the path (t 12 is deleted), nor is
 *                    {q_first 7, len 7, t 10..19} (t 10 aligns with q 6): no words, status 1.
 *                    For bsa_pog_place in refmode, with the window's slice of the draft as the backbone, the caller puts the piece's words between two D words
 *                    of its own: (t_first % w) D in front and (window's end - 1 - t_last) D behind (zero lengths left out) -- window [0, 10): 7D 3M;
 *                    window [10, 20): 2M 2I 4D 4M; window [20, 30): 2M 8D.
 * _bound           : host only, no GPU.  (cigar_off[n] - cigar_off[0]) + npiece: a pcig_cap that always suffices IF no two pieces of a pair share a column,
 *                    as is the case for the pieces of ONE bsa_cigar_windows_run (each of a pair's words then lands in at most one piece, plus one more
 *                    piece for every cut that falls inside it, and there are fewer cuts than pieces).  Pieces that overlap can need more: count first.
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the context's
 *                    scratch (512 bytes a pair for the index, 36 bytes for every piece of piece_cap; a run that has to grow it may synchronise once;
 *                    BSA_E_NOMEM when it cannot).  P = min(*d_npiece, piece_cap) is read on the device; launches are sized by piece_cap.  All piece_cap + 1
 *                    entries of d_pcig_off are written by every run, the entries above P equal the total d_pcig_off[P]; d_pstatus[j] (if not NULL) is
 *                    written for j < P.
 * arena (_run)     : that of bsa_kmer_chain_run, with the piece as the unit.  For ANY pcig_cap, 0 with a non-NULL d_pcig and a NULL d_pcig with cap 0 (a
 *                    count-only run) included:
 *                      - all entries of d_pcig_off are those of a run with a large arena;
 *                      - d_pcig_off[P] is the number of words needed;
 *                      - piece j's words are written, all of them, if and only if d_pcig_off[j + 1] <= pcig_cap, otherwise none of its range is touched;
 *                      - no word at or above pcig_cap, nor at or above the total, is touched;
 *                      - the caller's arena is never used as scratch.
 *                    A run leaves nothing behind that a later run reads.
 * _batch           : all pointers are HOST memory: uploads the records, the words cigar[cigar_off[0] .. cigar_off[n]) and the npiece pieces, runs, downloads,
 *                    synchronises.  pcig_off: all npiece + 1 entries are written; pstatus (npiece, may be NULL) likewise.  A cigar_off that decreases is
 *                    BSA_E_ARG.  pcig_cap too small: BSA_E_CIGAR_CAP, pcig_off[npiece] = the words needed, pcig untouched.  n == 0 or npiece == 0 is
 *                    fine: the offsets are 0 and every piece is not on a path.
 * errors (both)    : a NULL pcig_off; NULL d_out, d_cigar (_batch: only if the offsets speak of words) or d_cigar_off with n > 0; a NULL d_piece or
 *                    d_npiece with piece_cap > 0; a cap without its arena; n or the piece count (piece_cap, npiece) above 0xFFFFFFF0: BSA_E_ARG.
 * Example          : a polisher's step on resident reads --
 *                      bsa_align_run(plan, d_seqs, d_out, d_cigar, cigar_cap, d_cigar_off, d_status);
 *                      bsa_cigar_windows_run(ctx, d_out, d_cigar, d_cigar_off, n, 500, d_win, cap, d_win_off);
 *                      bsa_window_pieces_run(ctx, d_seqs, d_qoff, d_qlen, d_win, d_win_off, n, 500, d_gbase, nwin, flags, d_piece, cap, d_piece_off, ...);
 *                      bsa_piece_cigars_run(ctx, d_out, d_cigar, d_cigar_off, n, d_piece, d_piece_off + nwin, cap, d_pcig, cigar_cap + cap, d_pcig_off, NULL);
 *                    then codes and guides of every window come down window by window; blob, window records and CIGAR arena stay on the device. */
#define BSA_PIECE_ST_NOT_ON_PATH 1u
uint64_t bsa_piece_cigars_bound(const uint64_t *cigar_off, size_t n, size_t npiece);
int      bsa_piece_cigars_run(bsa_ctx_t *ctx,
                              const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off, size_t n,
                              const bsa_piece_t *d_piece, const uint64_t *d_npiece, size_t piece_cap,
                              uint32_t *d_pcig, size_t pcig_cap, uint64_t *d_pcig_off /* piece_cap + 1 */, uint32_t *d_pstatus /* piece_cap, may be NULL */);
int      bsa_piece_cigars_batch(bsa_ctx_t *ctx,
                                const bsa_result_t *out, const uint32_t *cigar, const uint64_t *cigar_off, size_t n,
                                const bsa_piece_t *piece, size_t npiece,
                                uint32_t *pcig, size_t pcig_cap, uint64_t *pcig_off /* npiece + 1 */, uint32_t *pstatus /* npiece, may be NULL */);

/* bsa_window_msa_* : every window's draft-anchored multiple alignment, in the `msacols` layout of bsalign_msa.h -- what bsa_msa_call_consensus_batch,
 *                    bsa_msa_text, bsa_msa_binary_write and bsa_msa_consensus take.  A window's pieces (bsa_window_pieces_*) with their guides
 *                    (bsa_piece_cigars_*) already are a multiple alignment against the window's slice of the draft: every piece row is anchored to draft
 *                    columns, and the only new columns are the insertion columns between draft columns.  This pass writes that alignment down as columns,
 *                    with the bsa_cns_window_t record of every window, so that the chain align -> windows -> pieces -> guides -> MSA -> consensus needs
 *                    neither the blob, the CIGAR arena, the pieces nor the guides on the host.
 *                    A pass over public outputs (bsa_window_msa.hip): it touches no plan and changes no existing call.
 * inputs           : d_piece, d_piece_off (nwin + 1), d_bases are what bsa_window_pieces_run left, piece_cap and bases_cap the room of d_piece and d_bases;
 *                    d_pcig, d_pcig_off (piece_cap + 1) what bsa_piece_cigars_run left for the same piece_cap, pcig_cap the room of d_pcig.
 * draft slice      : window g's slice is L = min(dlen[g], window) bases, base j = draft[doff[g] + j] & 3 at 1 B/base; with BSA_MODE_SEQ2BIT in flags draft is
 *                    BaseBank.bits words and doff a base offset, layout and rules as for the align calls (d_draft 8-byte aligned, _run: BSA_E_ARG otherwise).
 *                    The caller makes doff and dlen on the host from its targets' offsets and lengths (Python: window_drafts).  Precondition: the L bases
 *                    of every window lie inside the draft.
 * rows             : depth = piece_off[g + 1] - piece_off[g]; a window has depth 0 and no piece rows if piece_off[g + 1] > piece_cap or piece_off[g + 1] <
 *                    piece_off[g].  Row r < depth is piece piece_off[g] + r, row depth is the draft: nall = depth + 1 and a column is mrow = depth + 4 bytes
 *                    (nall rows, then the three consensus bytes).  The draft is the LAST row, so the caller decides whether it votes: nseq = depth leaves it
 *                    out (vote 0), nseq = depth + 1 counts it (vote 1).
 * a live piece     : piece j is LIVE if and only if all of these hold -- it has words and they are readable: pcig_off[j] < pcig_off[j + 1] <= pcig_cap; every
 *                    word's op is M, I, D, = or X; every word's length is at least 1; the first and the last word are diagonal; the lengths of the words
 *                    that advance q sum to len and those of the words that advance t to t_last - t_first + 1 (both sums in 64 bits); len >= 1; base_off + len
 *                    <= bases_cap; and, with a = t_first % window and b = a + (t_last - t_first), b < L.  This predicate is the only door to a piece's words
 *                    and codes: nothing the caller puts into these arrays makes the pass read outside them.  Every piece bsa_piece_cigars_run cuts from a
 *                    complete chain is live; a piece with BSA_PIECE_ST_NOT_ON_PATH has no words and is dead.
 * insertion columns: ins[j], 0 <= j < L, is the largest number of I units any live piece of the window has directly in front of draft column j (I words that
 *                    follow each other add up); ins[0] = 0 always, a guide starting on a diagonal word.  Draft column j is MSA column c[j] = j + ins[0] + ..
 *                    + ins[j]; mlen = L + the sum of ins (64 bits).  A window whose mlen would reach 2^31 has mlen 0 and no bytes.
 * a live row       : for a <= j <= b: at c[j] the piece's code & 3 if j is a diagonal column of its guide, 4 if the guide deletes j; for a < j the m >= 0 bases
 *                    the piece inserts in front of j go to the first m of the ins[j] columns in front of c[j], left-aligned and in read order, the others get
 *                    4.  Every column in front of c[a] -- the insertion columns in front of c[a] included -- and every column behind c[b] gets 5: the code 5
 *                    marks both ends of a read as the reference's MSA does (bspoa.h:3215-3234); 6 is never written.
 * other bytes      : a dead row is 5 throughout; the draft row holds its base at every c[j] and 4 in every insertion column; the three consensus bytes of
 *                    every column are written as 4, 0, 0.
 * not in any MSA   : I units that fall exactly between the last aligned column of one window and the first of the next are in no piece
 *                    (bsa_cigar_windows_* defines the pieces so) and therefore in no window's MSA.
 * Example          : window = 10, one window, L = 10, draft 0 1 2 3 0 1 2 3 0 1;
 *                      piece 0: t 0..9, words 4M 2I 6M,    codes 0 1 2 3 2 2 0 1 2 3 0 1;
 *                      piece 1: t 2..7, words 2M 1I 1D 3M, codes 2 3 1 1 2 3.
 *                    Only ins[4] = 2 is non-zero: mlen = 12, the draft columns are MSA columns 0 1 2 3 6 7 8 9 10 11, and
 *                      row 0 (piece 0)  0 1 2 3 2 2 0 1 2 3 0 1
 *                      row 1 (piece 1)  5 5 2 3 1 4 4 1 2 3 5 5      (its one inserted base left-aligned, then 4; draft column 4 deleted)
 *                      draft row        0 1 2 3 4 4 0 1 2 3 0 1
 *                    Column i is the 6 bytes row0[i] row1[i] draft[i] 4 0 0; the window is 72 bytes; cwin = {0, ~0, 0, nall 3, nseq = nmax = 2 + vote, mlen 12}.
 * d_cwin[g]        : the record bsa_msa_call_consensus_batch takes, written for every window by every run: cols_off = d_cols_off[g], idxs_off = ~0 (storage
 *                    order), out_off = the exclusive sum of mlen over the windows, nall = depth + 1, nseq = nmax = depth + vote, mlen.
 * _bound           : host only, no GPU.  The sum over the windows of window * (depth_g + 4), plus ins_units * (the largest depth + 4), saturating; piece_off is
 *                    the nwin + 1 offsets on the host, ins_units the I units of all the alignments' words (for instance the sum of out[k].ins).  It always
 *                    suffices for the pieces of ONE chain: bytes = sum of (L_g + sum of ins_g)(depth_g + 4) with L_g <= window; ins_g[j] is a maximum over the
 *                    window's pieces and so at most the sum of their I units in front of j; no two pieces of a pair share a column, so every I unit of a pair
 *                    lies in at most one piece, and all insertion columns together are at most ins_units, each of at most (largest depth + 4) bytes.  It is
 *                    loose where many reads insert at the same place; a count-only run (cols_cap 0) gives the exact need in d_cols_off[nwin].
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the context's
 *                    scratch (4 bytes for every draft column of nwin * window, 1 byte a piece of piece_cap, 32 bytes a window; a run that has to grow it
 *                    may synchronise once; BSA_E_NOMEM when it cannot).  window above 4096 is BSA_E_UNSUPPORTED (a window's line of ins / c stays in LDS;
 *                    polishers use 500).
 * arena            : the contract of bsa_window_pieces_run with one arena and the window as the unit.  For ANY cols_cap, 0 with a non-NULL d_cols and a NULL
 *                    d_cols with cols_cap 0 (a count-only run) included:
 *                      - all nwin + 1 entries of d_cols_off (bytes) and all nwin records of d_cwin are written and are those of a run with a large arena;
 *                      - d_cols_off[nwin] is the number of bytes needed;
 *                      - window g is written if and only if d_cols_off[g + 1] <= cols_cap;
 *                      - a written window is written whole: every byte of every column;
 *                      - a window that is not written has no byte of its range touched;
 *                      - nothing at or above cols_cap, nor at or above the total, is touched;
 *                      - the arena is never used as scratch.
 *                    The output is a function of the inputs alone; a run leaves nothing behind that a later run reads.
 * _batch           : all pointers are HOST memory; piece_cap is the number of pieces.  It uploads the pieces, codes, guides and the draft as far as the windows
 *                    speak of it, runs, downloads the offsets and records FIRST and synchronises: cols_cap too small is BSA_E_CIGAR_CAP there, cols_off[nwin]
 *                    = the bytes needed, cols untouched.  After it cols and cwin go to bsa_msa_call_consensus_batch as they are.
 * errors (both)    : window == 0; flag bits other than BSA_MODE_SEQ2BIT; vote > 1; a NULL piece_off, pcig_off or cols_off; with nwin > 0 a NULL draft, doff, dlen
 *                    or cwin; a cap without its arena; nwin or piece_cap above 0xFFFFFFF0: BSA_E_ARG.  nwin == 0 writes cols_off[0] = 0.
 * Example          : a polisher's step on resident reads, behind the three calls of the bsa_piece_cigars_* example --
 *                      bsa_window_msa_run(ctx, d_piece, d_piece_off, nwin, cap, d_bases, sum_qlen, d_pcig, cigar_cap + cap, d_pcig_off, d_draft, d_doff, d_dlen,
 *                                         500, 0, 0, d_cols, cols_cap, d_cols_off, d_cwin); bsa_ctx_sync(ctx);
 *                    then the MSA of every window, or only its consensus, comes down. */
uint64_t bsa_window_msa_bound(const uint64_t *piece_off /* nwin + 1, host */, size_t nwin, uint32_t window, uint64_t ins_units);
int      bsa_window_msa_run(bsa_ctx_t *ctx,
                            const bsa_piece_t *d_piece, const uint64_t *d_piece_off /* nwin + 1 */, size_t nwin, size_t piece_cap,
                            const uint8_t *d_bases, size_t bases_cap,
                            const uint32_t *d_pcig, size_t pcig_cap, const uint64_t *d_pcig_off /* piece_cap + 1 */,
                            const uint8_t *d_draft, const uint64_t *d_doff /* nwin */, const uint32_t *d_dlen /* nwin */,
                            uint32_t window, uint32_t flags /* BSA_MODE_SEQ2BIT or 0: the draft only */, uint32_t vote /* 0: nseq = depth; 1: the draft votes too */,
                            uint8_t *d_cols, size_t cols_cap, uint64_t *d_cols_off /* nwin + 1, bytes */, bsa_cns_window_t *d_cwin /* nwin */);
int      bsa_window_msa_batch(bsa_ctx_t *ctx,
                              const bsa_piece_t *piece, const uint64_t *piece_off /* nwin + 1 */, size_t nwin, size_t piece_cap,
                              const uint8_t *bases, size_t bases_cap,
                              const uint32_t *pcig, size_t pcig_cap, const uint64_t *pcig_off /* piece_cap + 1 */,
                              const uint8_t *draft, const uint64_t *doff /* nwin */, const uint32_t *dlen /* nwin */,
                              uint32_t window, uint32_t flags, uint32_t vote,
                              uint8_t *cols, size_t cols_cap, uint64_t *cols_off /* nwin + 1 */, bsa_cns_window_t *cwin /* nwin */);

/* bsa_window_cns_* : the consensus of every window's MSA where bsa_window_msa_run left it, and the windows' called bases packed into contiguous polished
 *                    sequence -- the last step of the chain align -> windows -> pieces -> guides -> MSA -> consensus.  The automaton is that of
 *                    bsa_msa_call_consensus_batch (bsalign_msa.h; bsa_cns_dev.hip's two kernels, unchanged, on the same tables): what differs is that the
 *                    columns and records are DEVICE memory, that the records are judged on the device, and that nothing but the polished sequence has to
 *                    come down.  A pass over public outputs (bsa_window_cns.hip): it touches no plan and changes no existing call.
 * the model        : bsa_cns_model_create builds the tables of the rates `par` as bsa_msa_call_consensus_batch does (the logarithms by the host's libm, the
 *                    all-zero entry of an absent read) and the table log(k!) at its full 1001 entries (entry k is a running sum from 0 and does not depend
 *                    on the table's length, so every entry is the one the host-pointer call uploads), and uploads both once with synchronous copies: it may
 *                    synchronise, and it is the only place where parameters cross to the device.  A model belongs to its context and is used by any number
 *                    of runs; destroy it when no run that uses it is in flight (bsa_ctx_sync) and before its context.  NULL is fine to destroy.
 * inputs           : d_cols and d_cwin are what bsa_window_msa_run left for nwin windows (any arrays of this layout serve); cols_cap is the room of d_cols.
 *                    max_rows is the caller's promise of the largest nseq -- the host knows it from piece_off and vote: the largest depth + vote -- and sizes
 *                    the automaton's LDS (16 bytes a row): a max_rows that needs more than 160 KB (about 9900 rows) is BSA_E_UNSUPPORTED.
 * outputs          : d_cns, d_qlt, d_alt of out_cap bytes each, the layout of bsa_msa_call_consensus_batch: window g's called bases, their qualities and
 *                    alternative qualities at [out_off, out_off + clen) of a range of room mlen (the rest of the range is not touched); d_clen[g] = clen,
 *                    d_score[g] = the log probability of the best path, d_status[g] = BSA_CNS_ST_* (d_score and d_status may be NULL).  The three consensus
 *                    bytes of every column of a live window are written as the host form writes them: called symbol (4: a gap), quality, alternative quality.
 * the live window  : window g runs if and only if ALL of the clauses below hold; they are tested on the device in 64-bit arithmetic that cannot wrap, and
 *                    d_status[g] reports the FIRST that fails --
 *                      BSA_CNS_ST_BAD_RECORD : idxs_off == ~0 (storage order only: the resident form takes no index blob);  nseq <= nall;  nmax <= nall;
 *                                              mlen < 2^31;  with the stride nall + 3 and mlen * stride formed in 64 bits, neither cols_off + mlen * stride
 *                                              nor out_off + mlen wraps;
 *                      BSA_CNS_ST_TOO_DEEP   : nseq <= max_rows;
 *                      BSA_CNS_ST_NO_ROOM    : cols_off + mlen * stride <= cols_cap;  out_off + mlen <= out_cap;  t[g + 1] <= min(out_cap, cols_cap / 4),
 *                                              where t is the pass's own exclusive sum of mlen over the windows that pass every clause in front of this one.
 *                    t is the workspace cursor and bounds the scratch from the host; on what bsa_window_msa_run writes t equals out_off, so the last clause
 *                    adds nothing there.  BSA_CNS_ST_OK is 0.  A window with mlen == 0 is live, with clen 0 and score 0.  This predicate is the only door to a
 *                    window's columns, its outputs and its workspace: nothing a caller puts into d_cwin makes the pass read or write outside [0, cols_cap)
 *                    of d_cols, outside [0, out_cap) of the three output arrays, or outside its scratch.  A window that is not live gets d_clen[g] = 0 and
 *                    d_score[g] = 0; no byte of its columns is touched (its three consensus bytes stay 4 0 0) and no byte of its output range.
 *                    The ranges of distinct live windows are expected to be disjoint, as the MSA pass makes them; where a caller makes them overlap, the
 *                    bytes in the overlap are unspecified and nothing else is affected.
 * compaction       : with d_seq_off (nwin + 1 entries) the exclusive sum of d_clen goes into it, and window g's bytes [out_off, out_off + clen) of d_cns,
 *                    d_qlt and d_alt are copied to [d_seq_off[g], d_seq_off[g + 1]) of d_seq, d_seq_qlt and d_seq_alt (either quality array may be NULL).
 *                    With bsa_window_pieces_*'s gbase numbering (Python: window_gbase) a draft's windows are consecutive, so its polished sequence is ONE
 *                    range: from d_seq_off of its first window to d_seq_off behind its last.  That range is what comes down.
 * arena            : the contract of bsa_window_pieces_run with the window as the unit.  For ANY seq_cap, 0 with non-NULL arrays and NULL arrays with
 *                    seq_cap 0 (a count-only run) included:
 *                      - all nwin + 1 entries of d_seq_off are written and are those of a run with a large arena; d_seq_off[nwin] is the bytes needed;
 *                      - window g is copied if and only if d_seq_off[g + 1] <= seq_cap; a copied window is copied whole;
 *                      - nothing at or above seq_cap is touched, and no byte of a window that is not copied.
 *                    With d_seq_off NULL nothing is packed (d_seq, d_seq_qlt, d_seq_alt NULL and seq_cap 0 then).
 * Example          : the 12 columns of the bsa_window_msa_* example with vote 1 (nseq = nmax = 3: the draft votes), the default rates 0.10 0.10 0.15 0.15
 *                    0.20 0.20 0.40, cwin = {0, ~0, 0, nall 3, nseq 3, nmax 3, mlen 12}, cols_cap 72, out_cap 12, max_rows 3 --
 *                      called symbol of the columns   0  1  2  3  2  4  0  1  2  3  0  1     (column 5: one inserted base against two gaps, called a gap)
 *                      their quality                 90 90 90 90  2  4 10 90 90 90 90 90
 *                      their alternative quality      0  0  0  0  5  5  5  0  0  0  0  0
 *                    these are the bytes 3, 4 and 5 of every column; status 0, clen = 11, and the first 11 bytes of the output ranges are
 *                      d_cns  0 1 2 3 2 0 1 2 3 0 1      d_qlt  90 90 90 90 2 10 90 90 90 90 90      d_alt  0 0 0 0 5 5 0 0 0 0 0
 *                    (the twelfth byte of each range is not touched); d_seq_off = {0, 11} and d_seq, d_seq_qlt, d_seq_alt hold the same 11 bytes from 0 on.
 *                    With vote 0 (nseq = nmax = 2) nothing is called a gap: clen = 12 and d_cns = row 0.
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the context's
 *                    scratch (a run that has to grow it may synchronise once; BSA_E_NOMEM when it cannot): about 80 bytes a window for the records and the
 *                    scans' temporaries, and 42 bytes for every column of min(out_cap, cols_cap / 4) + nwin -- 40 for the five masses, 2 for the packed
 *                    origins.  So the caps size the scratch: give out_cap as the sum of mlen (or bsa_window_msa_bound / 4 at most), not more.  At 100 000
 *                    pairs of 10 kbp, windows of 500 and depth 40 it is about 1.8 GB.  The output is a function of the inputs alone; a second run on columns
 *                    that already carry consensus bytes gives the same bytes; a run leaves nothing behind that a later run reads.
 * _batch           : all pointers are HOST memory and `par` takes the model's place.  It creates a model, uploads the columns, the records and the output
 *                    arrays as they are (so that a range no window owns comes down as it went up), runs, downloads clen, score, status and seq_off FIRST and
 *                    synchronises: seq_cap too small is BSA_E_CIGAR_CAP there, seq_off[nwin] = the bytes needed, cols and the six arrays untouched.  Then the
 *                    columns, the three output arrays and seq_off[nwin] bytes of the compact arrays come down.  It serves callers without device buffers and
 *                    the tests; it is not a second implementation.
 * errors (both)    : a NULL ctx or model (_batch: par); with nwin > 0 a NULL d_cwin, d_clen, d_cns, d_qlt or d_alt; a cap without its arena (cols_cap
 *                    without d_cols, seq_cap without d_seq); d_seq, d_seq_qlt, d_seq_alt or seq_cap given without d_seq_off; nwin above 0xFFFFFFF0; a model
 *                    of another context: BSA_E_ARG.  nwin == 0 writes d_seq_off[0] = 0 if d_seq_off is given, and nothing else.
 * Example          : behind the bsa_window_msa_run of that block's example, with the model made once --
 *                      bsa_cns_model_create(ctx, &par, &model);
 *                      bsa_window_cns_run(ctx, model, d_cols, cols_cap, d_cwin, nwin, 40 + vote, d_cns, d_qlt, d_alt, out_cap, d_clen, NULL, d_status,
 *                                         d_seq, d_seq_qlt, NULL, out_cap, d_seq_off); bsa_ctx_sync(ctx);
 *                    then draft j's polished bases are d_seq[d_seq_off[first window of j] .. d_seq_off[first window of j + 1]). */
#define BSA_CNS_ST_OK         0u
#define BSA_CNS_ST_BAD_RECORD 1u
#define BSA_CNS_ST_TOO_DEEP   2u
#define BSA_CNS_ST_NO_ROOM    3u
typedef struct bsa_cns_model bsa_cns_model_t;
int  bsa_cns_model_create(bsa_ctx_t *ctx, const bsa_cns_params_t *par, bsa_cns_model_t **out);
void bsa_cns_model_destroy(bsa_cns_model_t *m);          /* NULL is fine */
int  bsa_window_cns_run(bsa_ctx_t *ctx, const bsa_cns_model_t *model,
                        uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin, uint32_t max_rows,
                        uint8_t *d_cns, uint8_t *d_qlt, uint8_t *d_alt, size_t out_cap,     /* per window at out_off, room mlen each */
                        uint32_t *d_clen, double *d_score, uint32_t *d_status,               /* nwin each; d_score and d_status may be NULL */
                        uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off /* nwin + 1, or NULL: no compaction */);
int  bsa_window_cns_batch(bsa_ctx_t *ctx, const bsa_cns_params_t *par,
                          uint8_t *cols, size_t cols_cap, const bsa_cns_window_t *cwin, size_t nwin, uint32_t max_rows,
                          uint8_t *cns, uint8_t *qlt, uint8_t *alt, size_t out_cap,
                          uint32_t *clen, double *score, uint32_t *status,
                          uint8_t *seq, uint8_t *seq_qlt, uint8_t *seq_alt, size_t seq_cap, uint64_t *seq_off /* nwin + 1, or NULL */);

/* bsa_window_stitch_* : the stitched sequence of every window -- the consensus where enough reads cover a column, the draft where they do not -- and its
 *                    alignment to the draft as = / X / I / D words: what a polisher hands back, and what it changed.  bsa_window_cns_*'s own compaction
 *                    copies only the columns called as a base, so with vote 0 every column no read covers (a coverage hole, a contig end) and every
 *                    window that pass refuses loses its draft bases; this pass keeps them, without letting the draft vote anywhere else.
 *                    A pass over public outputs (bsa_window_stitch.hip): it touches no plan and changes no existing call.
 * inputs           : d_cols and d_cwin are what bsa_window_msa_run wrote and bsa_window_cns_run then filled with consensus bytes (any arrays of this layout
 *                    serve); cols_cap is the room of d_cols.  The columns are READ-ONLY here.  d_cns_status is the d_status of bsa_window_cns_run, nwin
 *                    entries, or NULL: every window counts as called.  That pass's per-window d_cns / d_qlt / d_alt ranges are not used at all: a caller
 *                    of this pass gives d_seq_off NULL there and skips its compaction.
 * readable record  : window g's record is READABLE if and only if all of these hold -- idxs_off == ~0;  nall >= 1;  mlen < 2^28 (so that a word's length
 *                    always fits);  with stride = nall + 3 and mlen * stride formed in 64 bits, cols_off + mlen * stride does not wrap and is <= cols_cap.
 *                    nseq and nmax are not looked at.  A record that is not readable has status BSA_STITCH_ST_BAD_RECORD, slen 0, no words and all counts
 *                    0.  This test is the only door to the columns: nothing a caller puts into d_cwin makes the pass read outside [0, cols_cap) of d_cols.
 * called window    : a readable window is CALLED (BSA_STITCH_ST_CALLED) if d_cns_status is NULL or d_cns_status[g] == 0, otherwise its status is
 *                    BSA_STITCH_ST_DRAFT.
 * a column's bytes : for column i with bytes b[0 .. nall + 3): d = b[nall - 1], the draft row -- the LAST row, as bsa_window_msa_run writes it; a
 *                    precondition, not something the pass checks --; c = b[nall], q = b[nall + 1], a = b[nall + 2], the called symbol and its two
 *                    qualities; cov = the number of rows r < nall - 1 with b[r] <= 4 (a row is absent at a column where its code is 5 or more).
 * covered column   : column i is COVERED if and only if the window is called and cov >= min_cov.
 * what it emits    : a covered column  -- to the sequence: base c with qualities q, a if c <= 3;  as a word unit: none if d > 3 and c > 3, I if d > 3,
 *                                         D if c > 3, = if c == d, X otherwise;
 *                    any other column  -- to the sequence: base d with qualities 0, 0 if d <= 3, and `kept` counts it;  as a unit: = if d <= 3, else none.
 * a window's output: slen = the emitted bases; eq, x, ins, del = the units of each kind (kept is part of eq); the words are the maximal runs of equal kind
 *                    over the emitted units in column order, len << 4 | op with the ops BSA_CIGAR_I, _D, _EQ, _X; ncig = their number.  Runs are never
 *                    merged across windows.  With window_gbase numbering a draft's words are the contiguous range d_cig[d_cig_off[first window] ..
 *                    d_cig_off[first window of the next draft]), its bases lie likewise in d_seq between the two d_seq_off entries.
 * invariants       : eq + x + ins == slen;  eq + x + del == the number of columns with d <= 3;  the word lengths per op sum to the counts.
 * and the consensus: with min_cov 0 every column of a called window is covered: d_seq, both quality arrays and d_seq_off of a batch of called windows are
 *                    then exactly what bsa_window_cns_run's compaction writes.  With vote 0 and min_cov 1 a base is taken from the consensus exactly where
 *                    at least one read spans the column.  A DRAFT window is the case "no column covered": its draft row, quality 0, one = word.
 * Example 1        : nall 2, nseq = nmax = 1 (vote 0), mlen 10, the default rates; piece row 5 5 5 3 2 1 5 5 5 5, draft row 0 1 2 3 0 1 2 3 0 1; the host
 *                    caller leaves the called bytes 4 4 4 3 2 1 4 4 4 4 and the quality bytes 0 0 0 90 90 90 0 0 0 0 (clen 3: seven draft bases are gone).
 *                      min_cov 0              : seq 3 2 1                 qlt 90 90 90                 words 3D 1= 1X 1= 4D   eq 2  x 1  ins 0  del 7  kept 0
 *                      min_cov 1              : seq 0 1 2 3 2 1 2 3 0 1   qlt 0 0 0 90 90 90 0 0 0 0   words 4= 1X 5=         eq 9  x 1  ins 0  del 0  kept 7
 *                      min_cov 2 or not called: seq 0 1 2 3 0 1 2 3 0 1   qlt all 0                    words 10=              eq 10 x 0  ins 0  del 0  kept 10
 *                    min_cov 0 is what the consensus pass packs.
 * Example 2        : the 12 columns of the bsa_window_cns_* example with vote 1 (nall 3; coverage 1 1 2 2 2 2 2 2 2 2 1 1) --
 *                      min_cov 0 or 1 : seq 0 1 2 3 2 0 1 2 3 0 1   qlt 90 90 90 90 2 10 90 90 90 90 90   words 4= 1I 6=   ins 1  kept 0
 *                      min_cov 2      : the same bases              qlt 0 0 90 90 2 10 90 90 90 0 0       words 4= 1I 6=   ins 1  kept 4
 *                      min_cov 3      : seq 0 1 2 3 0 1 2 3 0 1     qlt all 0                             words 10=        ins 0  kept 10
 *                    Column 5 is an insertion column called a gap: it emits nothing.
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the context's
 *                    scratch (a run that has to grow it may synchronise once; BSA_E_NOMEM when it cannot): 44 bytes a window and the scans' temporaries,
 *                    and 4 bytes -- the column's word -- for each of min(cols_cap / 4, max(seq_cap, cig_cap)) columns.  The windows whose columns fit that
 *                    many words (counted through the batch) have their columns read ONCE; the others are read a second time when the arenas are filled.
 *                    Disjoint windows sum to at most cols_cap / 4 columns, so caps of the sum of mlen read every column once.  The output is a function
 *                    of the inputs alone; a run leaves nothing behind that a later run reads.
 * arenas           : the house contract with the window as the unit and two arenas, d_seq (with d_seq_qlt, d_seq_alt; either may be NULL) and d_cig, that
 *                    are independent of each other.  For ANY seq_cap and cig_cap, 0 with a non-NULL arena and a NULL arena with cap 0 (count-only) included:
 *                      - all nwin + 1 entries of d_seq_off and of d_cig_off and all nwin records of d_rec are written and are those of a run with large
 *                        arenas; d_seq_off[nwin] and d_cig_off[nwin] say what a complete run needs;
 *                      - window g's bases (and the qualities that are given) are written, whole, if and only if d_seq_off[g + 1] <= seq_cap;
 *                      - window g's words are written, whole, if and only if d_cig_off[g + 1] <= cig_cap;
 *                      - no byte of a window that is not written is touched, nothing at or above a cap is touched, no arena is used as scratch.
 *                    The sum of mlen suffices for both caps: every base and every word takes at least one column.
 * _batch           : all pointers are HOST memory.  It uploads the columns, the records, the statuses and the arenas as they are, runs, downloads the offsets
 *                    and records FIRST and synchronises: a cap too small is BSA_E_CIGAR_CAP there, with both totals in seq_off[nwin] and cig_off[nwin] and
 *                    the arenas untouched.  Then seq_off[nwin] bytes of the sequence arrays and cig_off[nwin] words come down.
 * errors (both)    : a NULL ctx, d_seq_off or d_cig_off; with nwin > 0 a NULL d_cwin or d_rec; a cap without its arena (cols_cap without d_cols, seq_cap
 *                    without d_seq, cig_cap without d_cig); a quality array without d_seq; nwin above 0xFFFFFFF0: BSA_E_ARG.  nwin == 0 writes
 *                    d_seq_off[0] = d_cig_off[0] = 0 and nothing else.
 * Example          : behind the bsa_window_msa_run of that block's example, the consensus without its compaction, then the stitch --
 *                      bsa_window_cns_run(ctx, model, d_cols, cols_cap, d_cwin, nwin, 40, d_cns, d_qlt, d_alt, out_cap, d_clen, NULL, d_status,
 *                                         NULL, NULL, NULL, 0, NULL);
 *                      bsa_window_stitch_run(ctx, d_cols, cols_cap, d_cwin, nwin, d_status, 1, d_seq, d_seq_qlt, NULL, out_cap, d_seq_off,
 *                                            d_cig, out_cap, d_cig_off, d_rec); bsa_ctx_sync(ctx);
 *                    then draft j's polished bases are d_seq[d_seq_off[first window of j] .. d_seq_off[first window of j + 1]) and its differences to
 *                    the draft d_cig over the same two windows of d_cig_off; the sums of d_rec say whether another round is worth it. */
#define BSA_STITCH_ST_CALLED     0u   /* consensus used in every covered column */
#define BSA_STITCH_ST_DRAFT      1u   /* the consensus pass did not run this window: the draft row is kept whole */
#define BSA_STITCH_ST_BAD_RECORD 2u   /* the record's columns are not readable: the window contributes nothing */
typedef struct { uint32_t status, slen, eq, x, ins, del, kept, ncig; } bsa_stitch_t;   /* 32 bytes, one a window */
int  bsa_window_stitch_run(bsa_ctx_t *ctx,
                           const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
                           const uint32_t *d_cns_status /* nwin, what bsa_window_cns_run wrote; NULL: every window counts as called */,
                           uint32_t min_cov,
                           uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off /* nwin + 1 */,
                           uint32_t *d_cig, size_t cig_cap, uint64_t *d_cig_off /* nwin + 1 */,
                           bsa_stitch_t *d_rec /* nwin */);
int  bsa_window_stitch_batch(bsa_ctx_t *ctx,
                             const uint8_t *cols, size_t cols_cap, const bsa_cns_window_t *cwin, size_t nwin,
                             const uint32_t *cns_status /* nwin, or NULL */, uint32_t min_cov,
                             uint8_t *seq, uint8_t *seq_qlt, uint8_t *seq_alt, size_t seq_cap, uint64_t *seq_off /* nwin + 1 */,
                             uint32_t *cig, size_t cig_cap, uint64_t *cig_off /* nwin + 1 */,
                             bsa_stitch_t *rec /* nwin */);

/* bsa_window_snv_* : the SNVs of every window -- the columns where a second allele is too frequent to be sequencing error: bsa_msa_call_snvs
 *                    (bsalign_msa.h, the reference's call_snvs_bspoa) on the resident columns, a few records a window where the MSA is gigabytes.
 *                    The consensus keeps one allele a column; the evidence for the other is in the columns, and this pass reads it where it lies.
 *                    A pass over public outputs (bsa_window_snv.hip): it touches no plan and changes no existing call.
 * the model        : bsa_snv_model_create(ctx, max_rows, &model) uploads, once, everything that needs exp or log, computed by the host form's own code
 *                    so that host and device share one libm: the log-factorial table, log(p) and log(1 - p) in double of the 100 grid rates and of
 *                    0.01f, and for every (altn, covn), covn <= max_rows, whose own rate the host's float j admits to the grid (altn / covn below about
 *                    0.05) its row of float weights with the first bin and the number of bins, stored sparsely: 20 rows at max_rows 40, 24 500 rows and
 *                    under 10 MB at 1000.  max_rows above 1000 is BSA_E_UNSUPPORTED.  The model also sizes the kernels' LDS: 8.3 KB a wave at 40, 58 KB
 *                    at 1000 -- make it as deep as the windows are, not deeper.  A model serves any number of runs on its context.
 * inputs           : d_cols, d_cwin, cols_cap, d_cns_status as bsa_window_stitch_run takes them; the columns are READ-ONLY.  `par` is host memory, read
 *                    at the call (defaults 3, 0.5, 5, 0; the chain's windows have no placeholder row: skip_first_row 0).
 * a window's status: the readable-record test of bsa_window_stitch_run is the only door to the columns -- idxs_off == ~0, nall >= 1, mlen < 2^28, and
 *                    cols_off + mlen * (nall + 3), formed in 64 bits, neither wraps nor exceeds cols_cap -- and here nseq <= nall belongs to it: a
 *                    record that fails is BSA_SNV_ST_BAD_RECORD.  Then, in this order: nseq above the model's max_rows is BSA_SNV_ST_TOO_DEEP;  mlen >
 *                    65535 is BSA_SNV_ST_TOO_LONG;  a non-zero d_cns_status[g] is BSA_SNV_ST_NOT_CALLED (the consensus bytes are not valid; a NULL array:
 *                    every window counts).  A window with any status but BSA_SNV_ST_OK (0) has no records, nsites 0 and pexp 0.
 * outputs          : d_rec[g] = { status, nsnv, nsites, pexp }: the records, the columns that entered the estimate, the estimated rate;  window g's
 *                    records, bsa_snv_t as bsa_msa_call_snvs(cols + cols_off, NULL, nall, nseq, mlen, par, ...) writes them, in column order, at
 *                    d_snv[d_snv_off[g] .. d_snv_off[g + 1]).  lpos counts the bases of row nall - 1, the draft: window * w + lpos is the site in draft
 *                    coordinates, cpos the position in the window's consensus, mpos the column.  Every byte is the host form's.
 * arena            : the house contract with the window as the unit.  For ANY snv_cap, 0 with a non-NULL arena and a NULL arena with cap 0 (count-only)
 *                    included: all nwin + 1 entries of d_snv_off and all nwin records of d_rec are written and are those of a complete run;
 *                    d_snv_off[nwin] is the need; window g's records are written, whole, if and only if d_snv_off[g + 1] <= snv_cap; nothing else is
 *                    touched, the arena is not used as scratch.
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the
 *                    context's scratch (32 bytes a window and the scan's temporaries).  The columns are read twice by the wave that owns the window
 *                    (the counts and the estimate, then the calls at the estimated rate) and a third time only for windows that have calls and whose
 *                    records fit.  The output is a function of the inputs alone (the histogram is summed in integers); a run leaves nothing behind that
 *                    a later run reads, whatever its parameters.
 * _batch           : all pointers are HOST memory and max_rows takes the model's place.  It uploads the columns, the records, the statuses and the
 *                    arena as it is, runs, downloads the offsets and window records FIRST and synchronises: a cap too small is BSA_E_CIGAR_CAP there,
 *                    with the need in snv_off[nwin] and the arena untouched.  Then snv_off[nwin] records come down.
 * errors (both)    : a NULL ctx, model, par or d_snv_off; with nwin > 0 a NULL d_cwin or d_rec; a cap without its arena (cols_cap without d_cols,
 *                    snv_cap without d_snv); a model of another context; skip_first_row above 1 or min_covfrq outside [0, 65]; nwin or snv_cap above
 *                    0xFFFFFFF0: BSA_E_ARG.  nwin == 0 writes d_snv_off[0] = 0 and nothing else.
 * Example          : the five columns of bsa_msa_call_snvs's example (bsalign_msa.h) as one window, cwin = {0, ~0, 0, nall 4, nseq 4, nmax 4, mlen 5},
 *                    cols_cap 35, par = {1, 0.5, 1, 0}, max_rows 4 -- d_rec[0] = {0, 2, 3, 0.01f}, d_snv_off = {0, 2},
 *                      d_snv[0] = {mpos 1, cpos 1, lpos 1, qual 3, covn 4, refn 2, altn 2, refb 1, altb 3}
 *                      d_snv[1] = {mpos 3, cpos 2, lpos 3, qual 1, covn 4, refn 3, altn 1, refb 2, altb 0}
 *                    and behind the chain of the bsa_window_stitch_* example --
 *                      bsa_snv_model_create(ctx, 40, &snv_model);
 *                      bsa_window_snv_run(ctx, snv_model, d_cols, cols_cap, d_cwin, nwin, d_status, &par, d_snv, snv_cap, d_snv_off, d_rec); */
#define BSA_SNV_ST_OK         0u
#define BSA_SNV_ST_BAD_RECORD 1u
#define BSA_SNV_ST_TOO_DEEP   2u
#define BSA_SNV_ST_TOO_LONG   3u
#define BSA_SNV_ST_NOT_CALLED 4u
typedef struct { uint32_t status, nsnv, nsites; float pexp; } bsa_snv_window_t;          /* 16 bytes, one a window */
typedef struct bsa_snv_model bsa_snv_model_t;
int  bsa_snv_model_create(bsa_ctx_t *ctx, uint32_t max_rows, bsa_snv_model_t **out);
void bsa_snv_model_destroy(bsa_snv_model_t *m);          /* NULL is fine */
int  bsa_window_snv_run(bsa_ctx_t *ctx, const bsa_snv_model_t *model,
                        const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
                        const uint32_t *d_cns_status /* nwin, what bsa_window_cns_run wrote; NULL: every window counts */,
                        const bsa_snv_params_t *par,
                        bsa_snv_t *d_snv, size_t snv_cap, uint64_t *d_snv_off /* nwin + 1 */, bsa_snv_window_t *d_rec /* nwin */);
int  bsa_window_snv_batch(bsa_ctx_t *ctx, uint32_t max_rows,
                          const uint8_t *cols, size_t cols_cap, const bsa_cns_window_t *cwin, size_t nwin,
                          const uint32_t *cns_status /* nwin, or NULL */, const bsa_snv_params_t *par,
                          bsa_snv_t *snv, size_t snv_cap, uint64_t *snv_off /* nwin + 1 */, bsa_snv_window_t *rec /* nwin */);

/* bsa_window_realign_* : every piece of a window aligned again, against the sequence bsa_window_stitch_* called for that window -- what a SECOND round inside the
 *                    window needs.  Round 1's MSA is draft-anchored: every read was aligned on its own against a draft that is wrong in places, each piece's gaps
 *                    sit where that one alignment put them, and two reads that carry the same missing base at different places of a homopolymer split their
 *                    vote over two insertion columns.  This pass aligns every piece against its window's called sequence with one rule for every ambiguous gap
 *                    (the leftmost place) and leaves the result in the shape bsa_window_msa_run takes: piece records, guides whose first and last word are
 *                    diagonal, and the called sequence as the per-window draft.
 *                    A pass over public outputs (bsa_window_realign.hip): it touches no plan and changes no existing call.
 * inputs           : d_piece, d_piece_off (nwin + 1), d_bases are what bsa_window_pieces_run left (bsa_window_select_run's d_sel, d_sel_off with the same d_bases
 *                    serve equally), piece_cap and bases_cap the room of d_piece and d_bases; `window` is that round's window size; d_seq, d_seq_off, d_cig,
 *                    d_cig_off (nwin + 1 each) are what bsa_window_stitch_run left for the same windows, seq_cap and cig_cap the room of d_seq and d_cig.
 *                    `par` is host memory, read at the call.  Precondition: d_piece_off does not decrease (every pass in front writes it so); where it does,
 *                    nothing is read or written outside the caps, but which window a doubly claimed piece is lifted through is unspecified.
 * liftable window  : window g is LIFTABLE if and only if all of these hold -- d_seq_off[g] <= d_seq_off[g + 1] <= seq_cap;  slen = d_seq_off[g + 1] - d_seq_off[g]
 *                    <= window2;  d_cig_off[g] <= d_cig_off[g + 1] <= cig_cap;  every word has op I, D, = or X and a length of at least 1;  the units that consume
 *                    a sequence base (=, X, I) sum to slen;  the units that consume a draft column (=, X, D) sum to Ld <= window (both sums in 64 bits).  This
 *                    test is the only door to a window's words and bases.  A window that is not liftable has d_doff2[g] = 0, d_dlen2[g] = 0 and every piece of
 *                    it gets BSA_REALIGN_ST_NO_WINDOW; a liftable window has d_doff2[g] = d_seq_off[g], d_dlen2[g] = slen.
 * the lift         : draft column j of window g is the unit that consumes the j-th draft column, counting from 0; s(j) is the number of sequence-consuming
 *                    units in front of that unit, k(j) is 1 if the unit is = or X and 0 if it is D.  For a piece, a = t_first % window and b = a + (t_last -
 *                    t_first); its target is T = seq[d_seq_off[g] + u .. d_seq_off[g] + v] (inclusive) with u = s(a), v = s(b) + k(b) - 1, m = v - u + 1 bases.
 *                    Bases inserted in front of column a are not in the span, just as the piece's row is 5 in those columns.
 * a piece's status : the pieces of window g are piece_off[g] <= j < piece_off[g + 1] if piece_off[g] <= piece_off[g + 1] <= piece_cap, none otherwise; an index
 *                    below piece_cap that is in no window, or in a window that is not liftable, gets BSA_REALIGN_ST_NO_WINDOW.  A piece of a liftable window
 *                    is RE-ALIGNABLE if and only if all of these hold, and gets the status of the FIRST clause that fails, in this order, otherwise --
 *                      n = len >= 1 (_BAD_PIECE)  and  len <= max_len (_TOO_LONG);   base_off + len <= bases_cap, in 64 bits (_BAD_PIECE);   t_last >= t_first
 *                      (_BAD_PIECE);   b < Ld (_BAD_PIECE);   m >= 1 (_EMPTY_SPAN);   |m - n| <= 63 (_OFF_BAND);   margin = (63 - |m - n|) / 2 >= min_margin (_OFF_BAND).
 * the DP           : a global alignment of the n codes & 3 against the m bases & 3 of T that minimises the cost -- a mismatch x, a gap unit g, a match 0, both in
 *                    1 .. 255, linear gaps -- over the cells 0 <= i <= n, 0 <= jt <= m with dlo <= jt - i <= dlo + 63, dlo = min(0, m - n) - margin; every other
 *                    cell is unreachable.  That is 64 fixed diagonals: both corners are always inside and a path always exists.  The traceback goes from (n, m)
 *                    to (0, 0) and at every cell takes the FIRST step that explains the cell's value: the diagonal, then the target step (D), then the query
 *                    step (I).  Every ambiguous gap so lies at its leftmost place, for every read alike.  d_cost[j] is the value at (n, m) (0 for a piece that
 *                    is not re-alignable).  BSA_REALIGN_ST_EDGE, a flag bit beside status 0, is set if any cell of the path, the corners included, lies on
 *                    diagonal dlo or dlo + 63: the piece to run again with another band, as BSA_MODE_BAND_MARGIN reports for the aligner.
 * what leaves      : leading and trailing D and I steps are cut off; a path without a diagonal step is BSA_REALIGN_ST_NO_DIAG.  The words are the maximal runs
 *                    of the remaining steps, len << 4 | op with BSA_CIGAR_M, _I, _D (the MSA pass takes M; = / X would cost a second comparison for nothing).
 *                    d_piece2[j] keeps pair, has reserved = 0, q_first and base_off raised by the leading I units, len reduced by the leading and trailing I
 *                    units, t_first = u + the leading D units and t_last = v - the trailing D units: positions in the window's own round-1 sequence, window-
 *                    relative, so that nothing overflows and t_first % window2 is the column.  A piece with any status but 0 (or 0 | _EDGE) is DEAD: its
 *                    record is its input record with len = 0, and it has no words.  d_piece_off is reused unchanged in round 2: piece j stays row j -
 *                    piece_off[g] of window g, a dead piece is a dead row there, and every re-aligned piece is live under bsa_window_msa_run's predicate
 *                    with window = window2 and L = slen.
 * round 2          : bsa_window_msa_run(ctx, d_piece2, d_piece_off, nwin, piece_cap, d_bases, bases_cap, d_pcig2, pcig2_cap, d_pcig2_off, d_seq, d_doff2,
 *                    d_dlen2, par.window2, 0, vote, ...), then the consensus and the stitch as before, nothing coming down in between.  The words a round-2
 *                    stitch writes are against the ROUND-1 SEQUENCE, not against the original draft; composing the two word arenas is not part of this pass.
 * Example 1        : the window of bsa_window_stitch_*'s example 2 -- seq 0 1 2 3 2 0 1 2 3 0 1, words 4= 1I 6=, window 10 -- and a piece {pair 9, q_first 100,
 *                    len 6, t 32..37, base_off 0} with the codes 2 3 2 0 2 3, par = {window2 16, max_len 64, min_margin 8, x 1, g 1}: a = 2, b = 7, u = s(2) = 2,
 *                    v = s(7) + 1 - 1 = 8, T = 2 3 2 0 1 2 3, m = 7, margin 31; the cost is 1, the path 4M 1D 2M (the sequence's 1 is missing in the read),
 *                    d_piece2 = {9, 100, 6, t 2..8, 0, base_off 0}, status 0, d_doff2 = 0, d_dlen2 = 11.
 * Example 2        : a and b on D units: window 8, seq 0 1 2 3 0, words 2= 2D 3= 1D (Ld 8, slen 5), a piece {pair 3, q_first 10, len 5, t 2..7, base_off 0}
 *                    with the codes 1 2 3 0 2, window2 8: a = 2, b = 7, u = s(2) = 2, v = s(7) + 0 - 1 = 4, T = 2 3 0, m = 3, margin 30; the cost is 2, the
 *                    path 1I 3M 1I, both I steps are cut: words 3M, d_piece2 = {3, 11, 3, t 2..4, 0, base_off 1}.
 * _run             : DEVICE pointers; asynchronous on the context stream; no host/device copy, no synchronisation -- except that it may grow the context's
 *                    scratch (a run that has to grow it may synchronise once; BSA_E_NOMEM when it cannot): 20 bytes a piece of piece_cap, the scan's
 *                    temporaries, and (2 max_len + 63) / 4 bytes a piece for the paths (2 bits a step) -- make max_len as long as the pieces are, not longer.
 *                    max_len also sizes the DP kernel's LDS (a wave a piece: 16 bytes a row for the directions and the two sequences, about 11 KB at 600,
 *                    37 KB at 2048).  The DP of a piece runs once a run.
 * arena            : the contract of bsa_piece_cigars_run with the piece as the unit and piece_cap + 1 offsets.  For ANY pcig2_cap, 0 with a non-NULL d_pcig2 and
 *                    a NULL d_pcig2 with cap 0 (a count-only run) included:
 *                      - every entry of d_pcig2_off, d_pstatus, d_piece2, d_cost (if given), d_doff2 and d_dlen2 is written and is that of a run with a large
 *                        arena; d_pcig2_off[piece_cap] is the number of words needed;
 *                      - piece j's words are there, whole, if and only if d_pcig2_off[j + 1] <= pcig2_cap;
 *                      - nothing else is touched, nothing at or above pcig2_cap; the arena is never used as scratch.
 *                    The output is a function of the inputs alone; a run leaves nothing behind that a later run reads.  The sum over the pieces of 2 len + 63
 *                    words always suffices; a count-only run gives the exact need.
 * _batch           : all pointers are HOST memory.  It uploads the arrays as they are, runs, downloads the offsets, statuses and records FIRST and
 *                    synchronises: pcig2_cap too small is BSA_E_CIGAR_CAP there, pcig2_off[piece_cap] = the words needed, pcig2 untouched.
 * errors (both)    : window2 above 4096 (bsa_window_msa_run's limit) or max_len above 2048: BSA_E_UNSUPPORTED.  A NULL ctx or par; window, window2, max_len, x or
 *                    g of 0; x or g above 255; min_margin above 31; non-zero reserved; a NULL d_pcig2_off; with nwin > 0 a NULL d_piece_off, d_seq_off,
 *                    d_cig_off, d_doff2 or d_dlen2; with piece_cap > 0 a NULL d_piece, d_piece2 or d_pstatus; a cap without its arena; nwin, piece_cap or
 *                    pcig2_cap above 0xFFFFFFF0: BSA_E_ARG.  nwin == 0 writes d_pcig2_off[0 .. piece_cap] as 0 and every status BSA_REALIGN_ST_NO_WINDOW. */
#define BSA_REALIGN_ST_OK         0u
#define BSA_REALIGN_ST_NO_WINDOW  1u   /* in no window, or in a window that is not liftable */
#define BSA_REALIGN_ST_BAD_PIECE  2u   /* len 0, codes outside bases_cap, t_last < t_first, or b outside the window's draft columns */
#define BSA_REALIGN_ST_TOO_LONG   3u   /* len above max_len */
#define BSA_REALIGN_ST_EMPTY_SPAN 4u   /* the called sequence has no base on the piece's columns */
#define BSA_REALIGN_ST_OFF_BAND   5u   /* |m - n| above 63, or a margin below min_margin */
#define BSA_REALIGN_ST_NO_DIAG    6u   /* the best path has no diagonal step */
#define BSA_REALIGN_ST_EDGE   0x100u   /* flag beside status 0: the path touches the first or the last diagonal of the band */
typedef struct { uint32_t window2, max_len, min_margin, x, g, reserved[3]; } bsa_realign_params_t;   /* 32 bytes */
int  bsa_window_realign_run(bsa_ctx_t *ctx,
                            const bsa_piece_t *d_piece, const uint64_t *d_piece_off /* nwin + 1 */, size_t nwin, size_t piece_cap,
                            const uint8_t *d_bases, size_t bases_cap, uint32_t window,
                            const uint8_t *d_seq, size_t seq_cap, const uint64_t *d_seq_off /* nwin + 1 */,
                            const uint32_t *d_cig, size_t cig_cap, const uint64_t *d_cig_off /* nwin + 1 */,
                            const bsa_realign_params_t *par,
                            bsa_piece_t *d_piece2 /* piece_cap */, uint32_t *d_pcig2, size_t pcig2_cap, uint64_t *d_pcig2_off /* piece_cap + 1 */,
                            uint32_t *d_pstatus /* piece_cap */, uint32_t *d_cost /* piece_cap, or NULL */,
                            uint64_t *d_doff2 /* nwin */, uint32_t *d_dlen2 /* nwin */);
int  bsa_window_realign_batch(bsa_ctx_t *ctx,
                              const bsa_piece_t *piece, const uint64_t *piece_off /* nwin + 1 */, size_t nwin, size_t piece_cap,
                              const uint8_t *bases, size_t bases_cap, uint32_t window,
                              const uint8_t *seq, size_t seq_cap, const uint64_t *seq_off /* nwin + 1 */,
                              const uint32_t *cig, size_t cig_cap, const uint64_t *cig_off /* nwin + 1 */,
                              const bsa_realign_params_t *par,
                              bsa_piece_t *piece2 /* piece_cap */, uint32_t *pcig2, size_t pcig2_cap, uint64_t *pcig2_off /* piece_cap + 1 */,
                              uint32_t *pstatus /* piece_cap */, uint32_t *cost /* piece_cap, or NULL */,
                              uint64_t *doff2 /* nwin */, uint32_t *dlen2 /* nwin */);

/* ---- row-level kernels for the POA seq->graph DP (P4; reference bspoa.h:2232-2272) ----------------------------
 * The POA sweep calls, per graph edge u -> v, row_movx + row_cal on u's DP row (dpalign_row_update_bspoa) and, per
 * extra in-edge, row_merge (dpalign_row_merge_bspoa).  bsa_rows_run executes a batch of such INDEPENDENT tasks (one
 * topological level of many reads / windows) on device-resident row blocks.  A row block has exactly the reference's
 * layout and size (bspoa.h:1787-1793, 2217): us[bw] | es[bw] if piecewise >= 1 | qs[bw] if piecewise == 2 |
 * int32 ubegs[17], striped index (p % W) * 16 + p / W, padded to 16 bytes (bsa_rows_block_bytes). */
#define BSA_ROW_OP_UPDATE 0u   /* rows[dst] = row_cal(row_movx(rows[src], qoff_dst - qoff_src))   bspoa.h:2232 */
#define BSA_ROW_OP_MERGE  1u   /* rows[dst] = cell-wise max(rows[src], rows[dst])                  bspoa.h:2263 */
#define BSA_ROW_OP_INIT   2u   /* rows[dst] = row -1 of the read (row_init, bspoa.h:2226)                      */
typedef struct {
	uint32_t op;                  /* BSA_ROW_OP_* */
	uint32_t src, dst;            /* row block indices (u->mmidx, v->mmidx) */
	uint32_t qoff_src, qoff_dst;  /* band offsets (u->rpos, v->rpos) */
	uint32_t toff;                /* v->mpos: row number used by the left-boundary score */
	uint32_t query;               /* index into the query table */
	uint8_t  base;                /* v->base */
	uint8_t  prof;                /* (v->base == u->base) * 2 + v->bonus: which of the 4 profiles of bspoa.h:2199-2213 */
	uint16_t reserved;
} bsa_row_task_t;
typedef struct {
	int32_t  mode;                /* par->alnmode */
	uint32_t bandwidth;           /* multiple of 16, bandwidth / 16 in {1,2,4,8,16} */
	int8_t   M, X, refbonus;      /* par->M, par->X, par->refbonus */
	int8_t   gapo1, gape1, gapo2, gape2;
} bsa_rows_params_t;
size_t bsa_rows_block_bytes(uint32_t bandwidth, int8_t gapo1, int8_t gape1, int8_t gapo2, int8_t gape2);
/* all pointers are DEVICE memory; asynchronous on the context stream; tasks of one call must not depend on each other */
int bsa_rows_run(bsa_ctx_t *ctx, uint8_t *d_rows, const bsa_row_task_t *d_tasks, size_t ntasks,
                 const uint8_t *d_queries, const uint64_t *d_qoff, const uint32_t *d_qlen, const bsa_rows_params_t *par);

/* ---- the whole per-read sweep on the device (align_rd_bspoacore, bspoa.h:2515-2618) ----------
 * The reference walks the selected sub-graph with a stack and per-node in-degree counters; the visiting order depends
 * on the graph only, so the host flattens it into a program of row tasks (include/bsalign_poa_adapter.h does that from
 * the reference's own graph structures).  One program = one read against one graph; its tasks run in order on one
 * 16-lane DPP row, and many programs (POA windows) run concurrently.  Besides INIT / UPDATE / MERGE a program holds
 * the two places where the reference samples an end-of-alignment score:
 *   SCORE_TAIL  edge u -> tail (bspoa.h:2547-2577): H at the last band cell of u's row + the unaligned-tail gap + T,
 *               and in overlap mode the row maximum (row_max, bsalign.h:3213);
 *   SCORE_END   node v complete and its band reaches the read end, non-global modes (bspoa.h:2597-2606).
 * For both: src = the node's row block, qoff_src = its band offset (rpos), toff = the node index reported as maxidx.
 * A candidate replaces the running best only if strictly greater, in program order -- the reference's rule. */
#define BSA_ROW_OP_SCORE_TAIL 3u
#define BSA_ROW_OP_SCORE_END  4u
typedef struct {
	uint32_t first_task, ntasks;  /* this program's slice of the task array */
	uint32_t first_block;         /* task block indices are relative to this row block (mmidx 0 of the read's memp) */
	uint32_t reserved;
} bsa_sweep_prog_t;
typedef struct {
	int32_t maxscr, maxidx, maxoff; /* g->maxscr, g->maxidx, g->maxoff (bspoa.h:2227-2229); -2^30-ish, -1, -1 when no candidate */
	int32_t reserved;
} bsa_sweep_result_t;
typedef struct {
	bsa_rows_params_t rows;
	int32_t T;                    /* par->T: bonus for reaching the read end */
} bsa_sweep_params_t;
/* all pointers are DEVICE memory; asynchronous on the context stream */
/* Preconditions of the device-pointer entries (bsa_rows_run, bsa_sweep_run; bsa_sweep_host checks them and returns
 * BSA_E_ARG): every program has ntasks >= 1; first_task + ntasks stays inside the task array; first_block + src and
 * first_block + dst address row blocks inside d_rows; query indexes the query table.  A program with ntasks == 0 is skipped. */
int bsa_sweep_run(bsa_ctx_t *ctx, uint8_t *d_rows, const bsa_row_task_t *d_tasks, const bsa_sweep_prog_t *d_progs,
                  size_t nprogs, const uint8_t *d_queries, const uint64_t *d_qoff, const uint32_t *d_qlen,
                  const bsa_sweep_params_t *par, bsa_sweep_result_t *d_results);
/* ---- the per-read seq->graph DP as an anti-diagonal wavefront with the traceback on the device (P5 + P6) --------------------
 * Second form of the sweep (align_rd_bspoacore bspoa.h:2515-2618) that also replaces alignment2graph_bspoa's walk
 * (bspoa.h:2274-2513): the row blocks never leave the device, what comes back per read is the best end cell and the list
 * of traceback steps.  The band offset of every node is fixed before the sweep (prepare_rd_align_bspoa, bspoa.h:2168-2174),
 * so -- unlike the pairwise DP, whose band moves with the scores -- the dependencies between rows are known up front: one
 * wave runs one read, lane l owns node i (nodes in the order the reference completes them), walks its row cell by cell and
 * trails the rows it depends on by movx + 1 cells; rows of the nodes in flight live in an LDS ring, finished rows are
 * drained to HBM in 4-byte cells (H relative to the row's first cell, e, q) for the traceback.  Scores are absolute
 * integers: inside bsa_poa_graph_supported()'s guard none of the reference's int8 operations saturates, and the rows
 * equal the reference's block for block (tests/test_poa_graph_gpu.py through bsa_poa_graph_host's rows_out).
 *
 * A program = the selected sub-graph of one read:
 *   nodes   in completion order (node 0 = the head; every input of a node has a lower index).  A node carries two views:
 *           FORWARD: at most two inputs in[0..1]; an input is the row of node `src` moved by movx = rpos - rpos(src) and
 *           extended by one DP row (dpalign_row_update_bspoa, bspoa.h:2232), or -- kind MERGE -- the finished row of a
 *           PARTIAL node at the same rpos taken as it is (dpalign_row_merge_bspoa, bspoa.h:2263: the cell-wise maximum).
 *           A graph node with more than two selected in-edges is preceded by partial nodes (gnode = 0xFFFFFFFF) that
 *           fold its first in-edges, two at a time.
 *           TRACEBACK: its selected in-edges in the order of the reference's erev list with their coverage (edges[]).
 *   cands   the places where the reference samples an end-of-alignment score, in its visiting order (bspoa.h:2549-2603)
 * include/bsalign_poa_adapter.h builds programs from the reference's own graph. */
#define BSA_POA_IN_PRESENT 0x80000000u
#define BSA_POA_IN_MERGE   0x40000000u
#define BSA_POA_IN_SAME    0x20000000u   /* v->base == u->base: the profile without the homopolymer bonus (bspoa.h:2588) */
#define BSA_POA_IN_TOFF    0x0FFFFFFFu   /* v->mpos when the reference took the edge (left-boundary score, bspoa.h:2246-2248) */
typedef struct { uint32_t src, movx, toff_kind; } bsa_poa_input_t;
typedef struct {
	uint32_t rpos;                /* u->rpos */
	uint32_t gnode;               /* index of the node in the caller's graph; 0xFFFFFFFF for a partial node */
	uint32_t first_in;            /* traceback view: first in-edge record, relative to the program's edges */
	uint16_t n_in;
	uint8_t  base;                /* u->base (0..3; 4 = HEAD / TAIL sentinel) */
	uint8_t  flags;               /* bit 0: u->bonus */
	bsa_poa_input_t in[2];        /* forward view */
	uint32_t reserved[2];
} bsa_poa_node_t;                 /* 48 bytes */
typedef struct { uint32_t src, cov, src_rpos, reserved; } bsa_poa_edge_t;     /* local index of the predecessor, e->cov */
typedef struct { uint32_t node, kind; } bsa_poa_cand_t;                       /* kind 0: edge node -> tail, 1: node complete and its band reaches the read end */
typedef struct { uint32_t node; int32_t x; uint32_t bt; } bsa_poa_event_t;    /* one step of alignment2graph_bspoa: bt 0 M, 1 I, 2 D, 4 D2 (bsalign.h:40-50) */
typedef struct {
	uint32_t first_node, nnodes, first_edge, nedges, first_cand, ncands;
	uint32_t slen;                /* g->slen */
	uint32_t event_cap;           /* room for this program's events */
	uint64_t query_off;           /* its read (one base per byte, g->qseq + g->qb) inside the query blob */
	uint64_t first_event;
} bsa_poa_prog_t;                 /* 48 bytes */
#define BSA_POA_ST_OK     0
#define BSA_POA_ST_TRACE  1       /* the walk left the stored band / found no predecessor: the reference reads outside its rows or does not terminate there */
#define BSA_POA_ST_EVENTS 2       /* event_cap too small */
#define BSA_POA_ST_NOCAND 3       /* no end-of-alignment candidate (the reference would start its walk at node -1) */
typedef struct {
	int32_t maxscr, maxidx, maxoff;   /* g->maxscr, LOCAL index of g->maxidx, g->maxoff */
	int32_t status;                   /* BSA_POA_ST_* */
	int32_t nevents;
	int32_t fin_node, fin_x;          /* where the walk stopped: rs.tb = cpos of that node, rs.qb = fin_x (bspoa.h:2307-2311) */
	int32_t reserved;
} bsa_poa_result_t;
typedef struct { int32_t h; int8_t e, q; uint16_t tag; } bsa_poa_cell_t;      /* a row cell as rows_out returns it: absolute H, e = E - H, q = Q - H */
/* lanes a read of `max_slen` bases can use at this parameter set (a power of two up to 64), 0 = not supported: bandwidth above 256,
 * scores outside the exactness guard, or a read too long for the LDS.  Callers fall back to bsa_sweep_* then. */
int bsa_poa_graph_supported(const bsa_sweep_params_t *par, uint32_t max_slen);
/* 1 when bsa_poa_graph_run / _host take this parameter set at ANY bandwidth (up to 32768 columns): scores inside the same exactness guard, the
 * generic-width kernel of bsa_poa_gen.hip behind the same entry points (a workgroup per read, rows of 8 bytes a cell in the context's scratch,
 * as many programs side by side as $BSA_POA_GEN_WS_GB -- default 48 -- holds; rows_out is not available there).  A window's first aligned read
 * has the whole read as its band (bspoa.h:2045-2054, 2109-2111) and goes this way. */
int bsa_poa_graph_gen_supported(const bsa_sweep_params_t *par);
/* all pointers DEVICE memory, asynchronous on the context stream.  The steps of a walk leave the device as one word each,
 * node << 3 | bt (x is implied: it starts at maxoff and moves left with every M and I step): d_steps is scratch, program k walks
 * into d_steps[first_event .. + event_cap); when it is done its steps are appended to d_packed (capacity: the sum of all
 * event_cap), result.reserved = where, *d_packed_used = words in use (zeroed by the call).  bsa_poa_expand_steps turns a
 * program's words into bsa_poa_event_t on the host.  d_rows: (total nodes) x bw uint32 cells, d_u0: total nodes int32 (scratch
 * the traceback reads; pass NULL for both to use the context's own buffer). */
int bsa_poa_graph_run(bsa_ctx_t *ctx, const bsa_poa_node_t *d_nodes, size_t nnodes, const bsa_poa_edge_t *d_edges, const bsa_poa_cand_t *d_cands,
                      const bsa_poa_prog_t *d_progs, size_t nprogs, const uint8_t *d_queries, uint32_t max_slen, const bsa_sweep_params_t *par,
                      bsa_poa_result_t *d_results, uint32_t *d_steps, uint32_t *d_packed, uint64_t *d_packed_used, uint32_t *d_rows, int32_t *d_u0);
void bsa_poa_expand_steps(const uint32_t *steps, bsa_poa_result_t *res, bsa_poa_event_t *events);
/* HOST buffers in and out (uploads, runs, downloads, synchronises).  rows_out / u0_out (optional, tests): every node's row as
 * absolute cells, nnodes x bw, and its ubegs[0]. */
int bsa_poa_graph_host(bsa_ctx_t *ctx, const bsa_poa_node_t *nodes, size_t nnodes, const bsa_poa_edge_t *edges, size_t nedges,
                       const bsa_poa_cand_t *cands, size_t ncands, const bsa_poa_prog_t *progs, size_t nprogs,
                       const uint8_t *queries, size_t query_bytes, const bsa_sweep_params_t *par,
                       bsa_poa_result_t *results, bsa_poa_event_t *events, size_t events_cap, bsa_poa_cell_t *rows_out, int32_t *u0_out);

/* ---- batch scatter, host side (bsalign_amd/csrc/bsa_shard.cpp) ----------------
 * The pairs of one rank's contiguous range packed into the blob that travels to it: target k, then query k, each
 * padded to 16 bytes.  bsa_shard_pack fills out[0 .. bsa_shard_bytes) and every pair's offsets inside it (host memory,
 * `threads` host threads, 0 = as many as the machine has, at most 16). */
size_t bsa_shard_bytes(const uint32_t *qlen, const uint32_t *tlen, size_t first, size_t count);
int    bsa_shard_pack(const uint8_t *seqs, const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen,
                      size_t first, size_t count, uint8_t *out, size_t out_bytes, uint64_t *out_qoff, uint64_t *out_toff, unsigned threads);

/* ---- the exchange itself, for a C host: RCCL point-to-point messages over xGMI (bsalign_amd/csrc/bsa_shard_rccl.hip) -----------
 * One process per GPU.  Rank 0 calls bsa_shard_unique_id and ships the 128 bytes to the other ranks by whatever means the job has
 * (launcher environment, a file, MPI); every rank then creates its communicator on its own context.  RCCL (librccl.so.1) is loaded
 * at run time; with nranks == 1 nothing is loaded and both calls degenerate to copies.
 *   scatter   the root holds the batch in HOST memory; every rank gets its contiguous range [*first, *first + *count) -- ranges
 *             balanced by tlen x bandwidth --: the shard blob in DEVICE memory (*d_seqs, owned by the communicator, valid until the
 *             next scatter) with the pairs' lengths and offsets inside it (host arrays of `cap` entries), ready for
 *             bsa_align_plan_create / bsa_align_run.  Lengths travel as two broadcasts, the N - 1 shards as one ncclGroup of sends.
 *   gather    every rank hands in its range's results (DEVICE), CIGAR words (DEVICE) and CIGAR offsets (HOST, count + 1); the root
 *             receives all n records in input order, the CIGAR arena and its offsets (HOST).  Sizes travel as one ncclAllGather. */
typedef struct bsa_shard_comm bsa_shard_comm_t;
int  bsa_shard_unique_id(uint8_t id[128]);
int  bsa_shard_comm_create(bsa_ctx_t *ctx, int rank, int nranks, const uint8_t id[128], bsa_shard_comm_t **out);
void bsa_shard_comm_destroy(bsa_shard_comm_t *comm);
int  bsa_shard_scatter(bsa_shard_comm_t *comm, int root, const uint8_t *seqs, const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen,
                       size_t n, uint32_t bandwidth, size_t *first, size_t *count, uint8_t **d_seqs, size_t *blob_bytes,
                       uint32_t *local_qlen, uint32_t *local_tlen, uint64_t *local_qoff, uint64_t *local_toff, size_t cap);
int  bsa_shard_gather(bsa_shard_comm_t *comm, int root, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *cigar_off, size_t count,
                      bsa_result_t *out, uint32_t *cigar, size_t cigar_cap_words, uint64_t *out_cigar_off, size_t n);

/* ---- many windows in lock-step (bsalign_amd/csrc/bsa_batcher.hip) ----------------------------
 * One POA (end_bspoa, bspoa.h:4722-4776) is sequential in its reads, but windows are independent: a caller with many
 * of them runs each on a host thread of its own and lets every thread's sweep go through a batcher.  submit() has the
 * signature of the single-window backend of include/bsalign_poa_adapter.h (pass the batcher as `user`), is thread-safe
 * and BLOCKS until every participant that has not left is waiting in it; the last arrival executes all programs as one
 * device launch per distinct parameter set, then everybody returns with its results and row blocks.  A window that
 * has aligned its last read calls leave().  participants = number of windows (threads) that will submit. */
typedef struct bsa_sweep_batcher bsa_sweep_batcher_t;
int  bsa_sweep_batcher_create(bsa_ctx_t *ctx, uint32_t participants, bsa_sweep_batcher_t **out);
void bsa_sweep_batcher_destroy(bsa_sweep_batcher_t *b);
int  bsa_sweep_batcher_submit(void *batcher, const bsa_row_task_t *tasks, size_t ntasks, const uint8_t *query, uint32_t slen,
                              const bsa_sweep_params_t *par, uint8_t *rows_out, size_t nblocks, bsa_sweep_result_t *res);
void bsa_sweep_batcher_leave(bsa_sweep_batcher_t *b);
/* optional, first thing a window's thread does: from then on the thread computes only while it holds one of as many host slots
 * as the process has CPUs (cgroup quota, or $BSA_POA_HOST_THREADS); waiting in submit() hands the slot to another window */
void bsa_sweep_batcher_enter(bsa_sweep_batcher_t *b);
/* the same rendezvous for the graph form (sweep + traceback on the device, nothing but the steps comes back): signature of
 * bsa_poa_graph_backend_fn (include/bsalign_poa_adapter.h), `batcher` as user.  Declines with BSA_E_UNSUPPORTED, without
 * waiting, what bsa_poa_graph_supported declines; the window then submits the read through bsa_sweep_batcher_submit. */
int  bsa_poa_batcher_submit_graph(void *batcher, const bsa_poa_node_t *nodes, size_t nnodes, const bsa_poa_edge_t *edges, size_t nedges,
                                  const bsa_poa_cand_t *cands, size_t ncands, const uint8_t *query, uint32_t slen, const bsa_sweep_params_t *par,
                                  bsa_poa_result_t *res, bsa_poa_event_t *events, size_t events_cap);
/* out[0..7] = batches, device launches, programs, tasks, bytes uploaded, bytes downloaded, device microseconds, microseconds inside batches */
void bsa_sweep_batcher_stats(bsa_sweep_batcher_t *b, uint64_t out[8]);

/* HOST buffers in, HOST buffers out (uploads, runs, downloads, synchronises): what a single-window caller such as
 * the adapter uses.  rows_out (nblocks * bsa_rows_block_bytes, may be NULL) receives every row block so that host
 * traceback code (alignment2graph_bspoa, bspoa.h:2274) can read them as if the CPU had computed them. */
int bsa_sweep_host(bsa_ctx_t *ctx, const bsa_row_task_t *tasks, size_t ntasks, const bsa_sweep_prog_t *progs, size_t nprogs,
                   const uint8_t *queries, const uint64_t *qoff, const uint32_t *qlen, size_t nqueries,
                   const bsa_sweep_params_t *par, uint8_t *rows_out, size_t nblocks, bsa_sweep_result_t *results);

/* ---- synthetic read pairs (measurement inputs, SURVEY 8(d) / BASELINE.md 3) ---------------------
 * pair k: target = iid uniform ACGT of length L from splitmix64(seed ^ k*0x9E3779B97F4A7C15);
 * query = target with errors at rate err_q32 / 2^32 split sub:ins:del = 23:31:46.
 * Layout: target k at seqs[k*stride .. +L), query k at seqs[n*stride + k*stride .. +qlen[k]),
 * stride = bsa_synth_stride(L).  *_host fills host memory (no GPU needed); *_dev fills device
 * memory on the context stream and writes qlen to a device array. */
size_t bsa_synth_stride(uint32_t L);
/* ---- the anti-diagonal u8 DP of the MSA refinement (reference: maxmat_dp_diag_rowcal bspoa.h:3856-3896, driven by the
 * fill loop of remsa_pedit_rd_bspoacore bspoa.h:3925-3935; replaces that loop, the traceback that follows it stays the
 * caller's).  One problem = one read of a POA window against the window's column profile.  `planes` holds the ten byte
 * planes in the reference's own layout (bspoa.h:4213-4233): the offsets point at LOGICAL index 0 of a plane, which carries
 * 8 W bytes of padding in front of it and behind index mlen - 1 (seq planes: base codes, >= 4 = no base; mats planes: u8
 * counts).  `matrix` receives rows 2 mbeg .. 2 mend - 1 of the two difference planes (row r of a plane at out + r (16 W + 2),
 * cell c at byte 1 + c, guard cells at bytes 0 and 16 W + 1); other rows are not written.  All problems of a call share W
 * (1, 2 or 4: band of 16, 32 or 64 cells). */
typedef struct {
	uint64_t seq0, seq1;            /* read plane (x side), consensus plane (y side, reversed as the reference stores it) */
	uint64_t mats0[4], mats1[4];    /* mats[0][b], mats[1][b] */
	uint64_t out0, out1;            /* row 0 of matrix[0], matrix[1] inside `matrix` */
	uint32_t mlen, mbeg, mend, W;
} bsa_diagdp_prob_t;
int bsa_diagdp_batch(bsa_ctx_t *ctx, const uint8_t *planes, size_t planes_bytes, const bsa_diagdp_prob_t *probs, size_t n,
                     uint8_t *matrix, size_t matrix_bytes);
/* The same fill FOLLOWED BY THE TRACEBACK of remsa_pedit_rd_bspoacore (bspoa.h:3965-4040) on the device: the difference planes stay there
 * (2.1 bytes a cell: 12 GB for 64 windows of 64 reads x 22 k columns) and what comes back per problem is the walk from (mend - 1, mend - 1):
 * two bits a step -- 0 diagonal (x - 1, y - 1), 1 x - 1, 2 y - 1 -- sixteen steps a word from bit 0 up, problem k's words at
 * steps[first_word .. ], plus the score the reference returns (the sum over the diagonal steps) and where the walk stopped.  A caller
 * replays the steps to do what the reference does at every diagonal step (merge_nodes_bspoa, bspoa.h:4011-4022).  probs[k].out0 / out1 are
 * ignored (the planes are laid out by the library).  steps_cap_words >= sum over k of bsa_diagdp_walk_words(mbeg, mend). */
typedef struct { uint32_t nsteps; int32_t score; int32_t xi, yi; uint32_t status, reserved; uint64_t first_word; } bsa_diagdp_walk_t;    /* status 0 ok, 1 left the band, 2 no source explains a cell (the reference aborts) */
static inline uint64_t bsa_diagdp_walk_words(uint32_t mbeg, uint32_t mend){ return (2ull * (mend - mbeg) + 2 + 15) / 16; }
int bsa_diagdp_walk_batch(bsa_ctx_t *ctx, const uint8_t *planes, size_t planes_bytes, const bsa_diagdp_prob_t *probs, size_t n,
                          bsa_diagdp_walk_t *walks, uint32_t *steps, size_t steps_cap_words);
/* device time of the last bsa_diagdp_batch (staging + fill kernels), ms */
double bsa_diagdp_last_ms(bsa_ctx_t *ctx);

int bsa_synth_pairs_host(uint64_t seed, uint64_t first_pair, size_t n, uint32_t L, uint32_t err_q32,
                         uint8_t *seqs, uint32_t *qlen);
int bsa_synth_pairs_dev(bsa_ctx_t *ctx, uint64_t seed, uint64_t first_pair, size_t n, uint32_t L, uint32_t err_q32,
                        uint8_t *d_seqs, uint32_t *d_qlen);

/* device codes (one base per byte) -> BSA_MODE_SEQ2BIT words, asynchronous on the context stream: ceil(nbases / 32) words, each code
 * packed as c & 3, the bits behind the last base zero.  d_bad (device, may be NULL) is set to 1 when any code is above 3 and
 * left as it is otherwise (the caller clears it). */
int bsa_seq_pack2bit(bsa_ctx_t *ctx, const uint8_t *d_codes, uint64_t nbases, uint64_t *d_bits, uint32_t *d_bad);

#ifdef __cplusplus
}
#endif
#endif
