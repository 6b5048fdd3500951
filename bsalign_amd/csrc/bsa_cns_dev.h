// bsa_cns_dev.h -- what the two callers of the consensus automaton share (bsa_cns_dev.hip: bsa_msa_call_consensus_batch on host pointers;
// bsa_window_cns.hip: bsa_window_cns_run on what bsa_window_msa_run left): the device records of a window and of the model, the size of the
// automaton's LDS, the model's tables and the one place that launches k_cns_dp and k_cns_finish.
#pragma once
#include "../../include/bsalign_msa.h"
#include "../../include/bsalign_hip.h"
#include <hip/hip_runtime.h>

struct CnsWinDev {
	uint64_t cols_off, idxs_off;               // window's columns in the blob; its column order in the index blob (words), ~0: storage order
	uint64_t out_off;                          // where its consensus / qualities go
	uint64_t mass_off, org_off;                // workspace: (mlen + 1) x 5 doubles; (mlen + 1) packed origins (3 bits a state)
	uint32_t nall, nseq, nmax, mlen;
};

struct CnsModelDev {
	double cost[5][26][5];                     // [anchor][event * 5 + symbol | 25][target]
	uint8_t next[5][25][5];
	uint8_t pad[7];
	double ln10, logp, log1mp, psub;
};

#define BSA_CNS_LF_FULL 1001u                  // log(k!) for k <= 1000: all the alternative quality ever reads (fewer_errors)

// k_cns_dp's dynamic LDS for windows of at most max_nseq voting rows; *nsp: the rows' stride.  More than 160 KB does not launch.
static inline size_t bsa_cns_lds_bytes(uint64_t max_nseq, uint32_t *nsp){
	const uint64_t n = ((max_nseq ? max_nseq : 1u) + 3u) & ~(uint64_t)3u;
	if(nsp) *nsp = (uint32_t)n;                // (a stride that does not fit is not used: the size below is far above the limit)
	return sizeof(double) * 650 + 640 + (size_t)n * 16;
}
#define BSA_CNS_LDS_MAX ((size_t)160 * 1024)

// the tables from the host's libm (bsa_cns_model_internal), in the layout the kernels read; lf[k] = log(k!) for k < nlf
void bsa_cns_model_fill_internal(const bsa_cns_params_t *par, CnsModelDev *mod, double *lf, uint32_t nlf);

// k_cns_dp (steps & 1) and k_cns_finish (steps & 2) for nwin windows on DEVICE pointers: the dynamic LDS for max_nseq rows, its attribute above
// 64 KB, the two launches.  d_idxs may be NULL when every record's idxs_off is ~0.  BSA_OK, BSA_E_UNSUPPORTED (the LDS), BSA_E_NOMEM, BSA_E_HIP.
int bsa_cns_launch_internal(hipStream_t st, uint8_t *d_cols, const uint32_t *d_idxs, const CnsWinDev *d_wins, size_t nwin, const CnsModelDev *d_model,
		const double *d_lf, uint8_t *d_ws, uint64_t max_nseq, uint8_t *d_cns, uint8_t *d_qlt, uint8_t *d_alt, uint32_t *d_clen, double *d_score, int steps);
