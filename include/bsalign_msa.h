/* bsalign_msa.h -- the POA's MSA formats on plain arrays (the data formats behind the path).
 *
 * The reference keeps a finished window's MSA as `msacols` (mrow = nseq + 3 bytes per column: one byte per read --
 * base 0..3, 4 = gap, 5 / 6 = outside the read --, then consensus, consensus quality, alternative-allele quality) and
 * `msaidxs` (the order of the columns), bspoa.h:131-132.  These functions take exactly those two arrays and produce /
 * parse the reference's two formats byte for byte; nothing here touches a BSPOA.
 *
 *   binary container   dump_binary_msa_bspoa        bspoa.h:1555-1586
 *                      load_binary_msa_bspoa_core   bspoa.h:1588-1650, post_load_binary_msa_bspoa :1652-1685
 *   text               print_msa_bspoa              bspoa.h:1491-1553 with its row builders :1329-1483 (colorful = 0)
 *
 * All functions return 0 or a negative BSA_E_* code (bsalign_hip.h); writers report the bytes they need in *need and
 * return BSA_E_CIGAR_CAP-style BSA_E_ARG only for bad arguments: a too small buffer is BSA_E_NOMEM with *need set.
 */
#ifndef BSALIGN_MSA_H
#define BSALIGN_MSA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Binary container: [0x81, u32 metalen, meta]  0x22, u32 mlen, u32 nseq, mlen x (nseq + 1) bytes (reads + consensus of
 * every column, in msaidxs order), mlen consensus qualities, mlen alternative qualities, 0xFF.  `cols` / `idxs` as the
 * reference holds them (idxs == NULL: columns in storage order); mrow = nseq + 3. */
int bsa_msa_binary_write(const uint8_t *cols, const uint32_t *idxs, uint32_t nseq, uint32_t mlen,
                         const char *meta, uint32_t metalen, uint8_t *out, size_t cap, size_t *need);

/* Parses one container (records up to and including the 0xFF terminator).  Outputs are optional; `cols` receives
 * mlen x (nseq + 3) bytes in file order (the reference's loader sets msaidxs to the identity).  Returns 0, BSA_E_ARG on
 * a truncated / malformed stream, BSA_E_NOMEM when cols_cap or meta_cap is too small (sizes still reported). */
int bsa_msa_binary_read(const uint8_t *in, size_t len, size_t *consumed, uint32_t *nseq, uint32_t *mlen,
                        uint8_t *cols, size_t cols_cap, char *meta, size_t meta_cap, uint32_t *metalen);

/* What post_load_binary_msa_bspoa derives from a loaded MSA: the consensus with its two quality strings (columns
 * whose consensus is a base), and optionally every read's bases (rdseqs: concatenated, rdoffs[nseq + 1]). */
int bsa_msa_consensus(const uint8_t *cols, const uint32_t *idxs, uint32_t nseq, uint32_t mlen,
                      uint8_t *cns, uint8_t *qlt, uint8_t *alt, uint32_t *clen,
                      uint8_t *rdseqs, uint64_t *rdoffs);

/* print_msa_bspoa(g, label, mbeg, mend, linewidth, colorful = 0, out) into a buffer.  var_mpos: the MSA columns the
 * reference marks with '~' in the ruler (g->var, ascending; NULL / 0 = none).  cns / qlt / alt: the consensus arrays
 * (g->cns, g->qlt, g->alt) the trailer lines print. */
int bsa_msa_text(const uint8_t *cols, const uint32_t *idxs, uint32_t nseq, uint32_t mlen,
                 const uint8_t *cns, const uint8_t *qlt, const uint8_t *alt,
                 const uint32_t *var_mpos, uint32_t nvar,
                 const char *label, uint32_t mbeg, uint32_t mend, uint32_t linewidth,
                 char *out, size_t cap, size_t *need);

/* Consensus calling of a window's MSA: cns_bspoa (bspoa.h:3457-3733) with its alignment-event table
 * (gen_cns_aln_event_table_bspoa, bspoa.h:142-204), sum_log_nums (:3413-3453) and the binomial / normal tail of the
 * alternative-allele quality (:3391-3411), on the same plain arrays.  A column DP over five states (consensus base A, C, G, T or
 * gap) whose transition score sums, over the reads, the log probability of the event each read shows (match, substitution,
 * insertion / deletion opened or extended, homopolymer variants), followed by the traceback, the consensus quality (phred of the
 * posterior of the chosen state) and the quality against the most frequent other allele.  Double precision in the reference's
 * own order of operations: with the same libm the bytes are the reference's.
 *   cols / idxs   as above, mrow = nall + 3; the three consensus bytes of every column are (over)written, as the reference does
 *   nseq          reads that vote in the DP (the reference: min(g->nmsa, g->nrds));   nmax: reads counted for the alternative
 *                 allele (g->nrds);   nall: read rows of a column (g->seqs->nseq)
 *   cns/qlt/alt   receive the columns whose consensus is a base (room for mlen each), *clen their number; *score the DP's log
 *                 probability (cns_bspoa's return value) */
typedef struct { float psub, pins, pdel, piex, pdex, hins, hdel; } bsa_cns_params_t;     /* BSPOAPar, bspoa.h:70; defaults 0.10 0.10 0.15 0.15 0.20 0.20 0.40 */
int bsa_msa_call_consensus(uint8_t *cols, const uint32_t *idxs, uint32_t nall, uint32_t nseq, uint32_t nmax, uint32_t mlen,
                           const bsa_cns_params_t *par, uint8_t *cns, uint8_t *qlt, uint8_t *alt, uint32_t *clen, double *score);

/* The same for MANY windows on the device (bsa_cns_dev.hip; needs a context of libbsalign_hip, include/bsalign_hip.h): window k's columns
 * start at cols + win[k].cols_off (mrow = nall + 3 as above), its column order at idxs + win[k].idxs_off (words; ~0: storage order), its
 * consensus / qualities go to cns / qlt / alt + win[k].out_off (room for mlen each), clen[k] / score[k] as above.  One wave runs a window's
 * columns (the automaton is sequential in them), the windows run side by side.  Every sum over the reads is formed in the host form's order
 * from the host's own logarithm tables, so it has the host's bits; the merges log(exp a + exp b) use the device's exp / log, which may
 * differ from the host libm's in the last place: consensus, both quality strings and the three bytes of every column are the host form's
 * (and the reference's) byte for byte on everything tested (tests/test_cns_gpu.py), score[k] to a relative 1e-12.
 * Returns BSA_E_UNSUPPORTED above ~9900 reads in a window (the per-read state lives in LDS). */
typedef struct { uint64_t cols_off, idxs_off, out_off; uint32_t nall, nseq, nmax, mlen; } bsa_cns_window_t;
struct bsa_ctx;
int bsa_msa_call_consensus_batch(struct bsa_ctx *ctx, uint8_t *cols, size_t cols_bytes, const uint32_t *idxs, size_t idxs_words,
                                 const bsa_cns_window_t *win, size_t nwin, const bsa_cns_params_t *par,
                                 uint8_t *cns, uint8_t *qlt, uint8_t *alt, size_t out_bytes, uint32_t *clen, double *score);

/* SNV calling of a window's MSA: call_snvs_bspoa (bspoa.h:4931-5049) on the same plain arrays, and print_snvs_bspoa (:5053-5089).  The third output of
 * the reference's `poa` command beside the MSA and the consensus: the columns where a second allele is too frequent to be sequencing error.
 *   cols / idxs   as above, mrow = nall + 3, READ-ONLY; byte nall of a column is the called consensus symbol (bsa_msa_call_consensus wrote it)
 *   nseq          rows 0 .. nseq - 1 vote (nseq <= nall); with par->skip_first_row row 0 does not (the reference drops the empty placeholder row its
 *                 command line makes), and realnseq = nseq - skip_first_row
 * Per column  : cnt[c] = voting rows with code c, c <= 4; covn = their sum (codes 5 and above are not there).  The top two among A C G T only:
 *               (m1, m2) = (0, 1) if cnt[0] >= cnt[1] else (1, 0); then for i = 2, 3: if cnt[i] > cnt[m1] { m2 = m1; m1 = i } else if cnt[i] > cnt[m2]
 *               { m2 = i }.  refn = cnt[m1], altn = cnt[m2].  mincov = (uint16) max(2, (float) realnseq * min_covfrq).
 * Error rate  : every column with refn + altn >= mincov is a SITE and adds one to the histogram entry (altn, covn).  On the grid p_i = i * 0.0005f,
 *               i < 100, every non-zero entry, in ascending (altn, covn), with pexp = (float)(1.0 * altn / covn) and j = (int)(pexp / 0.0005f), 0 < j <
 *               100, adds count * prob to the sums of the bins j - k and j + k, prob = (float) exp(B(covn, altn, pexp -/+ 0.0005f * k)), each direction
 *               ending behind the first prob <= 0.01f; float multiply, float add, not fused.  B(n, m, p) = log(p) m + log(1 - p) (n - m) + LF[n] -
 *               LF[m] - LF[n - m] in double, LF[k] = log(k!) by running summation.  The window's rate is the first grid value with the largest sum if
 *               that sum exceeds 1, else 0.01f.  (altn / covn must be below 0.05 to count: windows of 20 rows or fewer always get 0.01f.)
 * Calls       : a column is a call if altn >= min_varcnt, refn + altn >= mincov and qual >= min_snvqlt, qual = -((float) B(covn, altn, rate) / log(10))
 *               truncated, at most 1000.  Records come in column order.
 * The record  : mpos the column; cpos the number of columns in front whose consensus byte is below 4 (the reference's cpos: the position in the
 *               consensus); lpos the same count for row nall - 1 -- in the window chain that row is the draft, so window * w + lpos is the site in draft
 *               coordinates (the reference has no such field); refb = m1, refn, altb = m2, altn, covn, qual.
 * Returns BSA_E_UNSUPPORTED for nseq > 1000 (beyond the log-factorial table the reference's formula changes meaning) and for mlen > 65535 (its 16-bit
 * histogram would wrap); BSA_E_ARG for skip_first_row above 1 or min_covfrq outside [0, 65]; BSA_E_NOMEM with *nsnv = the records there are when
 * snv_cap is smaller (the first snv_cap are written).  *pexp, *nsites (optional): the estimated rate and the number of sites.
 * Example     : nall 4, nseq 4, mlen 5, defaults but min_varcnt 1, min_covfrq 0.5 (mincov 2), min_snvqlt 1; columns as rows | consensus --
 *                 column 0   0 0 0 0 | 0    cnt 4 0 0 0  covn 4  m1 A m2 C  refn 4 altn 0   a site; altn 0 < 1: no call
 *                 column 1   1 1 3 3 | 1    cnt 0 2 0 2  covn 4  m1 C m2 T  refn 2 altn 2   (T ties C and does not displace it)   a site; a candidate
 *                 column 2   4 4 5 2 | 4    cnt 0 0 1 0  covn 3  m1 G m2 A  refn 1 altn 0   (the two gaps count for covn only)    refn + altn 1 < 2
 *                 column 3   2 2 2 0 | 2    cnt 1 0 3 0  covn 4  m1 G m2 A  refn 3 altn 1   a site; a candidate
 *                 column 4   3 6 6 6 | 3    cnt 0 0 0 1  covn 1  m1 T m2 A  refn 1 altn 0   refn + altn 1 < 2
 *               three sites; 1 / 4 and 2 / 4 are not below 0.05, so no entry reaches the grid and the rate is 0.01f.
 *                 column 1: B(4, 2, 0.01) = 2 log 0.01 + 2 log 0.99 + log 6 = -7.4387, qual = (int) 3.2306 = 3: a call, mpos 1 cpos 1 lpos 1 C 2 T 2
 *                 column 3: B(4, 1, 0.01) = log 0.01 + 3 log 0.99 + log 4 = -3.2490, qual = (int) 1.4110 = 1: a call, mpos 3 cpos 2 lpos 3 G 3 A 1
 *               (cpos 2 at column 3: column 2's consensus is a gap; lpos 3: its last row is a base.) */
typedef struct { uint32_t mpos, cpos, lpos, qual; uint16_t covn, refn, altn; uint8_t refb, altb; } bsa_snv_t;       /* 24 bytes */
typedef struct { int32_t min_varcnt; float min_covfrq; uint32_t min_snvqlt; uint32_t skip_first_row; } bsa_snv_params_t;   /* defaults 3, 0.5, 5, 0 */
int bsa_msa_call_snvs(const uint8_t *cols, const uint32_t *idxs, uint32_t nall, uint32_t nseq, uint32_t mlen, const bsa_snv_params_t *par,
                      bsa_snv_t *snv, size_t snv_cap, size_t *nsnv, float *pexp, uint32_t *nsites);
/* print_snvs_bspoa: one `<label> SNP` line a record -- cpos, mpos, the five consensus bases in front and their qualities (+ '!'), reference base and
 * count, alternative base and count, the five bases behind and their qualities, covn, qual, the column's rows 0 .. nseq - 1 as "ACGT-.*".  cns / qlt:
 * the compact consensus and its quality (bsa_msa_consensus), clen bases.  Writers' convention: *need, BSA_E_NOMEM when cap is smaller. */
int bsa_msa_snv_text(const uint8_t *cols, const uint32_t *idxs, uint32_t nall, uint32_t nseq, uint32_t mlen,
                     const uint8_t *cns, const uint8_t *qlt, uint32_t clen, const bsa_snv_t *snv, size_t nsnv,
                     const char *label, char *out, size_t cap, size_t *need);

#ifdef __cplusplus
}
#endif
#endif
