// bsa_window_snv.hip -- bsa_snv_model_create / _destroy, bsa_window_snv_run / _batch (include/bsalign_hip.h): the SNVs of every window's MSA where
// bsa_window_msa_run left it and bsa_window_cns_run filled it -- bsa_msa_call_snvs (bsa_snv.cpp, include/bsalign_msa.h) a wave a window.
//
// A pass over public outputs; the columns are read-only here.  Everything that needs exp or log comes from the host (bsa_snv_model_internal: the
// log-factorials, log(p) and log(1 - p) of the 101 rates, and for every (altn, covn) entry a window of the model's depth can hold its row of float
// weights on the grid), so the sums the device forms are the host's bit for bit.  The steps on the context stream:
//   prepare : a thread a window (k_window_snv_prepare) tests the readable record and the statuses and copies what the pass needs into the context's
//             scratch -- nothing reads the caller's record a second time;
//   count   : a wave a window (k_window_snv_count).  First time through the columns, in tiles of 64 whole columns in LDS, a lane a column: the
//             counts, the top two, and an integer atomic on the (altn, covn) histogram in LDS (an integer sum does not depend on order).  Then the
//             estimate, a lane a bin, over the non-zero entries in ascending (altn, covn) -- float multiply, float add, unfused, from the model's
//             rows.  Then the columns a second time, now with the rate: the calls are counted.  The window's record and its count are left;
//   scan    : the counts -> d_snv_off;
//   fill    : a wave a window (k_window_snv_fill), only windows that have calls and whose records fit: the columns once more, the same rules
//             (sv_tile_calls is the one copy), the records placed by ballot and prefix count.
// Why the columns again and not a word a column, as the stitch pass leaves: a column's word would need the two counts, the coverage and both bases
// -- 8 bytes a column, 342 MB of scratch at the benchmark's shape where this takes 32 bytes a window --; and the fill reads only windows with calls.
// (The second reading costs about what the first does: the windows in flight exceed the L2.  DESIGN 4.2t has the figures.)  The histogram and the
// staged tables live in dynamic LDS sized by the model.
// Plain C++; no kernel uses scratch memory.
#include "bsa_pass.h"

static_assert(sizeof(bsa_cns_window_t) == 40 && sizeof(bsa_snv_t) == 24 && sizeof(bsa_snv_window_t) == 16 && sizeof(bsa_snv_params_t) == 16, "the records' layouts");

// a wave's tile of whole columns: 8176 bytes behind up to 15 bytes of shift (bsa_window_stitch.hip has the same tile)
#define SV_LDS 8176u
#define SV_TILE_BYTES 8192u
#define SV_GRID 100u

struct sv_win_t { uint64_t cols_off; uint32_t nall, nseq, mlen, status; };
struct sv_model_dev_t {
	const double *lf, *lgp, *lg1p; const float *pgrid, *weights; const uint32_t *cmin, *rowbase, *desc;
	double ln10; uint32_t max_rows, amax, nrows, pad;
};
struct bsa_snv_model { bsa_ctx_t *ctx; uint8_t *buf; sv_model_dev_t dev; size_t lds_bytes; };
enum { SV_PREPARE = 1, SV_COUNT = 2, SV_FILL = 4 };

extern "C" int bsa_snv_model_internal(uint32_t max_rows, double *lfv, double *lgp, double *lg1p, float *pgrid, double *ln10, uint32_t *amax, uint32_t *cmin, uint32_t *rowbase,
		uint32_t *desc, float *weights, size_t *nrows, size_t *nweights);
extern "C" int bsa_snv_params_check_internal(const bsa_snv_params_t *par);

__global__ void __launch_bounds__(256) k_window_snv_prepare(const bsa_cns_window_t *cwin, const uint32_t *cns_status, uint64_t cols_cap, uint32_t nwin, uint32_t max_rows, sv_win_t *wd){
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if(g >= nwin) return;
	const bsa_cns_window_t w = cwin[g];
	sv_win_t d = { 0ull, 1u, 0u, 0u, BSA_SNV_ST_BAD_RECORD };
	if(w.idxs_off == ~0ull && w.nall >= 1u && w.nseq <= w.nall && w.mlen < (1u << 28)){
		const uint64_t bytes = (uint64_t)w.mlen * ((uint64_t)w.nall + 3u);               // (below 2^28 (2^32 + 2): the product does not wrap)
		if(w.cols_off <= ~0ull - bytes && w.cols_off + bytes <= cols_cap){
			d.status = w.nseq > max_rows ? BSA_SNV_ST_TOO_DEEP : w.mlen > 65535u ? BSA_SNV_ST_TOO_LONG : (cns_status && cns_status[g] != 0u) ? BSA_SNV_ST_NOT_CALLED : BSA_SNV_ST_OK;
			if(d.status == BSA_SNV_ST_OK){ d.cols_off = w.cols_off; d.nall = w.nall; d.nseq = w.nseq; d.mlen = w.mlen; }
		}
	}
	wd[g] = d;
}

// n bytes into LDS where dst and src are congruent modulo 16: 16-byte vectors over the aligned middle, single bytes in front and behind
static __device__ __forceinline__ void sv_stage(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane){
	uint32_t head = (uint32_t)((0u - (uintptr_t)src) & 15u);
	if(head > n) head = n;
	const uint32_t nv = (n - head) / 16u, tail = head + nv * 16u;
	if(lane < head) dst[lane] = src[lane];
	for(uint32_t i = lane; i < nv; i += 64u) ((uint4*)(dst + head))[i] = ((const uint4*)(src + head))[i];
	if(tail + lane < n) dst[tail + lane] = src[tail + lane];
}

// the bytes of a dword that are zero, and those that are 4 or less, as their top bits (no carry or borrow crosses a byte)
static __device__ __forceinline__ uint32_t sv_zero(uint32_t x){ return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
static __device__ __forceinline__ uint32_t sv_le4(uint32_t w){
	const uint32_t ge5 = ((w & 0x7F7F7F7Fu) | 0x80808080u) - 0x05050505u;
	return ~ge5 & ~w & 0x80808080u;
}

static __device__ __forceinline__ uint32_t sv_wave_sum(uint32_t v){
#pragma unroll
	for(int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// a column as the rules see it: the voting rows with code 0, 1, 2, 3, those with a code of 4 or less, the consensus byte and the last row's byte
struct sv_col_t { uint32_t c0, c1, c2, c3, covn, cns, dr; };

// the columns i0 .. i0 + n of a window, lane l that of column i0 + l (undefined for a lane without one); rows r0 .. nseq vote.
// tcols: the columns of a tile that fit the wave's LDS -- n <= tcols <= 64 -- or 0: a column does not fit, and the lanes go over the rows.
static __device__ __forceinline__ sv_col_t sv_tile_counts(const uint8_t *cols, const sv_win_t &w, uint32_t r0, uint32_t i0, uint32_t n, uint32_t tcols, uint8_t *lds, uint32_t lane){
	const uint64_t stride = (uint64_t)w.nall + 3u;
	const uint8_t *src = cols + w.cols_off + (uint64_t)i0 * stride;
	sv_col_t c = { 0u, 0u, 0u, 0u, 0u, 4u, 4u };
	if(tcols){
		const uint32_t s = (uint32_t)stride, shift = (uint32_t)((uintptr_t)src & 15u);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // (the reads of the tile in front are done before this one lands)
		__builtin_amdgcn_wave_barrier();
		sv_stage(lds + shift, src, n * s, lane);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		if(lane < n){
			// the rows [b0, b1) by aligned dwords, the bytes outside masked away (the tile is a multiple of 4 bytes: no dword leaves it)
			const uint32_t base = shift + lane * s, b0 = base + r0, b1 = base + w.nseq;
			for(uint32_t k = b0 & ~3u; k < b1; k += 4u){
				uint32_t m = 0x80808080u;
				if(k < b0) m <<= (b0 - k) * 8u;
				if(k + 4u > b1) m &= 0x80808080u >> ((k + 4u - b1) * 8u);
				const uint32_t x = *(const uint32_t*)(lds + k);
				c.c0 += (uint32_t)__popc(sv_zero(x) & m);
				c.c1 += (uint32_t)__popc(sv_zero(x ^ 0x01010101u) & m);
				c.c2 += (uint32_t)__popc(sv_zero(x ^ 0x02020202u) & m);
				c.c3 += (uint32_t)__popc(sv_zero(x ^ 0x03030303u) & m);
				c.covn += (uint32_t)__popc(sv_le4(x) & m);
			}
			c.dr = lds[base + w.nall - 1u]; c.cns = lds[base + w.nall];
		}
	} else {
		for(uint32_t j = 0; j < n; j++){
			const uint8_t *col = src + (uint64_t)j * stride;
			uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, tc = 0;
			for(uint32_t r = r0 + lane; r < w.nseq; r += 64u){
				const uint32_t b = col[r];
				t0 += b == 0u; t1 += b == 1u; t2 += b == 2u; t3 += b == 3u; tc += b <= 4u;
			}
			t0 = sv_wave_sum(t0); t1 = sv_wave_sum(t1); t2 = sv_wave_sum(t2); t3 = sv_wave_sum(t3); tc = sv_wave_sum(tc);
			if(lane == j){ c.c0 = t0; c.c1 = t1; c.c2 = t2; c.c3 = t3; c.covn = tc; c.dr = col[w.nall - 1u]; c.cns = col[w.nall]; }
		}
	}
	return c;
}

// the top two among A C G T, ties as the reference's order makes them fall
struct sv_top_t { uint32_t m1, m2, refn, altn; };
static __device__ __forceinline__ sv_top_t sv_top2(const sv_col_t &c){
	const bool s = c.c0 >= c.c1;
	uint32_t m1 = s ? 0u : 1u, m2 = s ? 1u : 0u, n1 = s ? c.c0 : c.c1, n2 = s ? c.c1 : c.c0;
	{ const bool a = c.c2 > n1, b = c.c2 > n2; m2 = a ? m1 : b ? 2u : m2; n2 = a ? n1 : b ? c.c2 : n2; m1 = a ? 2u : m1; n1 = a ? c.c2 : n1; }
	{ const bool a = c.c3 > n1, b = c.c3 > n2; m2 = a ? m1 : b ? 3u : m2; n2 = a ? n1 : b ? c.c3 : n2; m1 = a ? 3u : m1; n1 = a ? c.c3 : n1; }
	const sv_top_t t = { m1, m2, n1, n2 };
	return t;
}

static __device__ __forceinline__ uint32_t sv_tile_cols(uint32_t nall){
	const uint64_t stride = (uint64_t)nall + 3u;
	if(stride > SV_LDS) return 0u;
	const uint32_t fit = SV_LDS / (uint32_t)stride;
	return fit < 64u ? fit : 64u;
}

static __device__ __forceinline__ uint32_t sv_mincov(uint32_t realnseq, float min_covfrq){
	const float f = __fmul_rn((float)realnseq, min_covfrq);
	return (uint32_t)(2.0f > f ? 2.0f : f) & 0xFFFFu;                  // (min_covfrq <= 65 and realnseq <= 1000: below 2^16 anyway)
}

// the calls among the columns i0 .. i0 + n at the rate of bin `bin`: whether the lane's column (mpos i0 + lane) is one, its qual and the record's last
// two words, covn | refn << 16 and altn | refb << 16 | altb << 24 (cpos and lpos are the caller's to carry).  CN / DR: the ballots of the columns whose consensus byte / last row is a base.
static __device__ __forceinline__ bool sv_tile_calls(const uint8_t *cols, const sv_win_t &w, const sv_model_dev_t &md, const bsa_snv_params_t &par, uint32_t r0, uint32_t mincov,
		uint32_t bin, uint32_t i0, uint32_t n, uint32_t tcols, uint8_t *lds, uint32_t lane, uint32_t &qual, uint32_t &w4, uint32_t &w5, uint64_t &CN, uint64_t &DR){
	const sv_col_t c = sv_tile_counts(cols, w, r0, i0, n, tcols, lds, lane);
	const sv_top_t t = sv_top2(c);
	const uint32_t m1 = t.m1, m2 = t.m2, refn = t.refn, altn = t.altn;
	CN = __ballot(lane < n && c.cns < 4u);
	DR = __ballot(lane < n && c.dr < 4u);
	bool call = false;
	qual = 0u;
	if(lane < n && (int64_t)altn >= (int64_t)par.min_varcnt && refn + altn >= mincov){
		const double perm = __dsub_rn(__dsub_rn(md.lf[c.covn], md.lf[altn]), md.lf[c.covn - altn]);
		const double b = __dadd_rn(__dadd_rn(__dmul_rn(md.lgp[bin], (double)altn), __dmul_rn(md.lg1p[bin], (double)(c.covn - altn))), perm);
		const double q = -((double)__double2float_rn(b) / md.ln10);
		qual = q >= 1000.0 ? 1000u : q > 0.0 ? (uint32_t)q : 0u;
		call = qual >= par.min_snvqlt;
	}
	w4 = c.covn | refn << 16; w5 = altn | m1 << 16 | m2 << 24;
	return call;
}

// dynamic LDS of a wave: the tile, then cmin and rowbase (amax + 2 words each), then the histogram, two 16-bit counters a word
static __device__ __forceinline__ void sv_lds(uint8_t *base, const sv_model_dev_t &md, uint8_t *&tile, uint32_t *&cmin, uint32_t *&rowbase, uint32_t *&hist){
	tile = base; cmin = (uint32_t*)(base + SV_TILE_BYTES); rowbase = cmin + md.amax + 2u; hist = rowbase + md.amax + 2u;
}
static size_t sv_lds_bytes(uint32_t amax, size_t nrows){ return SV_TILE_BYTES + (size_t)(amax + 2u) * 8u + ((nrows + 1u) / 2u) * 4u; }

// a wave a window, a wave a workgroup
__global__ void __launch_bounds__(64) k_window_snv_count(uint32_t nwin, const sv_win_t *wd, const uint8_t *cols, const sv_model_dev_t md, const bsa_snv_params_t par,
		bsa_snv_window_t *rec, uint32_t *nsnvv, uint32_t *binv){
	extern __shared__ uint4 sv_dyn[];
	const uint32_t lane = threadIdx.x;
	uint8_t *lds; uint32_t *cmin, *rowbase, *hist;
	sv_lds((uint8_t*)sv_dyn, md, lds, cmin, rowbase, hist);
	for(uint32_t a = lane; a < md.amax + 2u; a += 64u){ cmin[a] = md.cmin[a]; rowbase[a] = md.rowbase[a]; }
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	for(uint64_t g = blockIdx.x; g < nwin; g += gridDim.x){
		const sv_win_t w = wd[g];
		uint32_t nsnv = 0, nsites = 0, bin = SV_GRID;
		if(w.status == BSA_SNV_ST_OK && w.mlen){
			const uint32_t r0 = par.skip_first_row, realnseq = w.nseq > r0 ? w.nseq - r0 : 0u, mincov = sv_mincov(realnseq, par.min_covfrq);
			const uint32_t tcols = sv_tile_cols(w.nall), step = tcols ? tcols : 64u;
			// the rows of the model this window can reach: altn 1 .. aw, aw the largest with cmin[aw] <= realnseq (cmin grows with altn)
			uint32_t aw = 0;
			while(aw < md.amax && cmin[aw + 1u] <= realnseq) aw++;
			const uint32_t nused = aw ? rowbase[aw + 1u] : 0u;
			for(uint32_t i = lane; i < (nused + 1u) / 2u; i += 64u) hist[i] = 0u;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			for(uint32_t i0 = 0; i0 < w.mlen; i0 += step){
				const uint32_t n = w.mlen - i0 < step ? w.mlen - i0 : step;
				const sv_col_t c = sv_tile_counts(cols, w, r0, i0, n, tcols, lds, lane);
				const sv_top_t t = sv_top2(c);
				const uint32_t refn = t.refn, altn = t.altn;
				const bool site = lane < n && refn + altn >= mincov;
				nsites += (uint32_t)__popcll(__ballot(site));
				if(site && altn >= 1u && altn <= aw && c.covn >= cmin[altn]){         // (covn <= realnseq <= max_rows: the row exists)
					const uint32_t slot = rowbase[altn] + c.covn - cmin[altn];
					atomicAdd(&hist[slot >> 1], 1u << ((slot & 1u) * 16u));               // (mlen <= 65535: a counter does not carry into its neighbour)
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			// the estimate: the lane's bins are lane and lane + 64; the entries in ascending row, which is ascending (altn, covn)
			float ps0 = 0.0f, ps1 = 0.0f;
			for(uint32_t rb = 0; rb < nused; rb += 64u){
				const uint32_t r = rb + lane;
				const uint32_t cnt = r < nused ? (hist[r >> 1] >> ((r & 1u) * 16u)) & 0xFFFFu : 0u;
				uint32_t woff = 0, fb = 0;
				if(cnt){ woff = md.desc[2u * r]; fb = md.desc[2u * r + 1u]; }
				uint64_t nz = __ballot(cnt != 0u);
				while(nz){
					const int b = __ffsll((long long)nz) - 1;
					nz &= nz - 1ull;
					const float fn = (float)(uint32_t)__builtin_amdgcn_readlane((int)cnt, b);
					const uint32_t wo = (uint32_t)__builtin_amdgcn_readlane((int)woff, b), f = (uint32_t)__builtin_amdgcn_readlane((int)fb, b);
					const uint32_t first = f & 0xFFu, nb = f >> 8;
					if(lane - first < nb) ps0 = __fadd_rn(ps0, __fmul_rn(fn, md.weights[wo + lane - first]));
					if(lane + 64u - first < nb) ps1 = __fadd_rn(ps1, __fmul_rn(fn, md.weights[wo + lane + 64u - first]));
				}
			}
			// the first bin with the largest sum, if that exceeds 1
			float bv = ps0; uint32_t bi = lane;
			if(lane + 64u < SV_GRID && ps1 > ps0){ bv = ps1; bi = lane + 64u; }
#pragma unroll
			for(int d = 32; d >= 1; d >>= 1){
				const float ov = __shfl_xor(bv, d); const uint32_t oi = (uint32_t)__shfl_xor((int)bi, d);
				if(ov > bv || (ov == bv && oi < bi)){ bv = ov; bi = oi; }
			}
			if(bv > 1.0f) bin = bi;
			// the columns again, with the rate
			for(uint32_t i0 = 0; i0 < w.mlen; i0 += step){
				const uint32_t n = w.mlen - i0 < step ? w.mlen - i0 : step;
				uint32_t qual, w4, w5; uint64_t CN, DR;
				const bool call = sv_tile_calls(cols, w, md, par, r0, mincov, bin, i0, n, tcols, lds, lane, qual, w4, w5, CN, DR);
				nsnv += (uint32_t)__popcll(__ballot(call));
			}
		}
		if(lane == 0){
			const bsa_snv_window_t r = { w.status, nsnv, nsites, w.status == BSA_SNV_ST_OK ? md.pgrid[bin] : 0.0f };
			rec[g] = r; nsnvv[g] = nsnv; binv[g] = bin;
		}
	}
}

// a wave a window, a wave a workgroup: the windows that have calls and whose records fit
__global__ void __launch_bounds__(64) k_window_snv_fill(uint32_t nwin, const sv_win_t *wd, const uint8_t *cols, const sv_model_dev_t md, const bsa_snv_params_t par,
		const uint32_t *binv, const uint64_t *snv_off, uint64_t snv_cap, bsa_snv_t *snv){
	extern __shared__ uint4 sv_dyn[];
	const uint32_t lane = threadIdx.x;
	const uint64_t lt = (1ull << lane) - 1ull;
	uint8_t *lds = (uint8_t*)sv_dyn;
	for(uint64_t g = blockIdx.x; g < nwin; g += gridDim.x){
		const sv_win_t w = wd[g];
		if(w.status != BSA_SNV_ST_OK || !w.mlen) continue;
		const uint64_t s0 = snv_off[g], s1 = snv_off[g + 1u];
		if(s1 > snv_cap || s1 <= s0) continue;
		const uint32_t r0 = par.skip_first_row, realnseq = w.nseq > r0 ? w.nseq - r0 : 0u, mincov = sv_mincov(realnseq, par.min_covfrq);
		const uint32_t tcols = sv_tile_cols(w.nall), step = tcols ? tcols : 64u, bin = binv[g];
		uint64_t sp = s0;
		uint32_t cpos = 0, lpos = 0;
		for(uint32_t i0 = 0; i0 < w.mlen && sp < s1; i0 += step){
			const uint32_t n = w.mlen - i0 < step ? w.mlen - i0 : step;
			uint32_t qual, w4, w5; uint64_t CN, DR;
			const bool call = sv_tile_calls(cols, w, md, par, r0, mincov, bin, i0, n, tcols, lds, lane, qual, w4, w5, CN, DR);
			const uint64_t C = __ballot(call);
			if(call){
				const uint64_t p = sp + (uint32_t)__popcll(C & lt);
				if(p < s1){
					uint32_t *o = (uint32_t*)(snv + p);                          // (the record's six words)
					o[0] = i0 + lane; o[1] = cpos + (uint32_t)__popcll(CN & lt); o[2] = lpos + (uint32_t)__popcll(DR & lt); o[3] = qual; o[4] = w4; o[5] = w5;
				}
			}
			sp += (uint32_t)__popcll(C);
			cpos += (uint32_t)__popcll(CN); lpos += (uint32_t)__popcll(DR);
		}
	}
}

extern "C" int bsa_snv_model_create(bsa_ctx_t *ctx, uint32_t max_rows, bsa_snv_model_t **out){
	if(out) *out = nullptr;
	if(!ctx) return BSA_E_ARG;
	if(!out){ bsa_ctx_set_error_internal(ctx, "bsa_snv_model_create: null argument"); return BSA_E_ARG; }
	if(max_rows > 1000u){ bsa_ctx_set_error_internal(ctx, "bsa_snv_model_create: max_rows above 1000, where the log-factorial table ends"); return BSA_E_UNSUPPORTED; }
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);                  // (also selects the context's device)
	if(rc != BSA_OK) return rc;
	size_t nrows = 0, nweights = 0; uint32_t amax = 0; double ln10 = 0;
	if((rc = bsa_snv_model_internal(max_rows, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nrows, &nweights)) != BSA_OK){
		bsa_ctx_set_error_internal(ctx, "bsa_snv_model_create: the grid rows are not ranges"); return rc;
	}
	const size_t o_lf = 0, o_lgp = o_lf + bsa_up256(1001u * 8u), o_lg1p = o_lgp + bsa_up256(101u * 8u), o_pg = o_lg1p + bsa_up256(101u * 8u), o_cmin = o_pg + bsa_up256(101u * 4u),
		o_rb = o_cmin + bsa_up256(((size_t)max_rows + 2u) * 4u), o_desc = o_rb + bsa_up256(((size_t)max_rows + 2u) * 4u), o_w = o_desc + bsa_up256(nrows * 8u),
		total = o_w + bsa_up256(nweights * 4u + 4u);
	std::vector<uint8_t> h;
	try { h.assign(total, 0); } catch(...){ return BSA_E_NOMEM; }
	if((rc = bsa_snv_model_internal(max_rows, (double*)(h.data() + o_lf), (double*)(h.data() + o_lgp), (double*)(h.data() + o_lg1p), (float*)(h.data() + o_pg), &ln10, &amax,
			(uint32_t*)(h.data() + o_cmin), (uint32_t*)(h.data() + o_rb), (uint32_t*)(h.data() + o_desc), (float*)(h.data() + o_w), &nrows, &nweights)) != BSA_OK) return rc;
	bsa_snv_model *m = new (std::nothrow) bsa_snv_model();
	if(!m) return BSA_E_NOMEM;
	if(hipMalloc((void**)&m->buf, total) != hipSuccess){
		(void)hipGetLastError(); delete m; bsa_ctx_set_error_internal(ctx, "bsa_snv_model_create: no device memory"); return BSA_E_NOMEM;
	}
	if(hipMemcpy(m->buf, h.data(), total, hipMemcpyHostToDevice) != hipSuccess){
		(void)hipGetLastError(); (void)hipFree(m->buf); delete m; bsa_ctx_set_error_internal(ctx, "bsa_snv_model_create: upload failed"); return BSA_E_HIP;
	}
	m->ctx = ctx;
	m->dev.lf = (const double*)(m->buf + o_lf); m->dev.lgp = (const double*)(m->buf + o_lgp); m->dev.lg1p = (const double*)(m->buf + o_lg1p);
	m->dev.pgrid = (const float*)(m->buf + o_pg); m->dev.weights = (const float*)(m->buf + o_w);
	m->dev.cmin = (const uint32_t*)(m->buf + o_cmin); m->dev.rowbase = (const uint32_t*)(m->buf + o_rb); m->dev.desc = (const uint32_t*)(m->buf + o_desc);
	m->dev.ln10 = ln10; m->dev.max_rows = max_rows; m->dev.amax = amax; m->dev.nrows = (uint32_t)nrows; m->dev.pad = 0;
	m->lds_bytes = sv_lds_bytes(amax, nrows);
	*out = m;
	return BSA_OK;
}

extern "C" void bsa_snv_model_destroy(bsa_snv_model_t *m){
	if(!m) return;
	if(m->buf) (void)hipFree(m->buf);
	delete m;
}

// the argument errors of both calls
static int sv_check(bsa_ctx_t *ctx, const bsa_snv_model_t *model, bool need_model, const void *cols, size_t cols_cap, const void *cwin, size_t nwin, const bsa_snv_params_t *par,
		const void *snv, size_t snv_cap, const void *snv_off, const void *rec){
	const char *msg = nullptr;
	if(!par || (need_model && !model) || !snv_off || (nwin && (!cwin || !rec)) || (cols_cap && !cols) || (snv_cap && !snv)) msg = "bsa_window_snv: null argument";
	else if(model && model->ctx != ctx) msg = "bsa_window_snv: the model belongs to another context";
	else if(bsa_snv_params_check_internal(par) != BSA_OK) msg = "bsa_window_snv: skip_first_row above 1 or min_covfrq outside [0, 65]";
	else if(nwin > 0xFFFFFFF0ull || snv_cap > 0xFFFFFFF0ull) msg = "too many windows or records";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	return BSA_OK;
}

// the steps of `steps`, in order (one alone only for tools/bench_window_snv.py, on the scratch a whole run left)
static int sv_run(bsa_ctx_t *ctx, hipStream_t st, int steps, const bsa_snv_model_t *model, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
		const uint32_t *d_cns_status, const bsa_snv_params_t &par, bsa_snv_t *d_snv, size_t snv_cap, uint64_t *d_snv_off, bsa_snv_window_t *d_rec){
	hipError_t e = hipSuccess;
	if(nwin == 0){
		e = bsa_launch_excl_scan(st, (const uint32_t*)nullptr, d_snv_off, 0u, nullptr, nullptr);          // d_snv_off[0] = 0
		if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_snv: launch failed"); return BSA_E_HIP; }
		return BSA_OK;
	}
	// scratch: 24 + 4 + 4 bytes a window and the scan's temporaries
	const size_t o_wd = 0, o_nsnv = o_wd + bsa_up256(nwin * sizeof(sv_win_t)), o_bin = o_nsnv + bsa_up256(nwin * 4u), o_tmp = o_bin + bsa_up256(nwin * 4u),
		total = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)nwin));
	void *bufv = nullptr;
	int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);              // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	sv_win_t *wd = (sv_win_t*)(b + o_wd);
	uint32_t *nsnvv = (uint32_t*)(b + o_nsnv), *binv = (uint32_t*)(b + o_bin);
	uint64_t *tmp = (uint64_t*)(b + o_tmp);
	const size_t most = (size_t)bsa_cus() * 32u;
	const dim3 waves((uint32_t)(nwin < most ? nwin : most));
	if(steps & SV_PREPARE){
		hipLaunchKernelGGL(k_window_snv_prepare, dim3((uint32_t)(((uint64_t)nwin + 255u) / 256u)), dim3(256), 0, st, d_cwin, d_cns_status, (uint64_t)cols_cap, (uint32_t)nwin,
			model->dev.max_rows, wd);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & SV_COUNT)){
		hipLaunchKernelGGL(k_window_snv_count, waves, dim3(64), model->lds_bytes, st, (uint32_t)nwin, (const sv_win_t*)wd, d_cols, model->dev, par, d_rec, nsnvv, binv);
		e = hipGetLastError();
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)nsnvv, d_snv_off, (uint32_t)nwin, nullptr, tmp);
	}
	if(e == hipSuccess && (steps & SV_FILL) && snv_cap){
		hipLaunchKernelGGL(k_window_snv_fill, waves, dim3(64), SV_TILE_BYTES, st, (uint32_t)nwin, (const sv_win_t*)wd, d_cols, model->dev, par, (const uint32_t*)binv,
			(const uint64_t*)d_snv_off, (uint64_t)snv_cap, d_snv);
		e = hipGetLastError();
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_snv: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

static int sv_run_checked(bsa_ctx_t *ctx, int steps, const bsa_snv_model_t *model, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
		const uint32_t *d_cns_status, const bsa_snv_params_t *par, bsa_snv_t *d_snv, size_t snv_cap, uint64_t *d_snv_off, bsa_snv_window_t *d_rec){
	if(!ctx) return BSA_E_ARG;
	int rc = sv_check(ctx, model, true, d_cols, cols_cap, d_cwin, nwin, par, d_snv, snv_cap, d_snv_off, d_rec);
	if(rc != BSA_OK) return rc;
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	return sv_run(ctx, stream, steps, model, d_cols, cols_cap, d_cwin, nwin, d_cns_status, *par, d_snv, snv_cap, d_snv_off, d_rec);
}

extern "C" int bsa_window_snv_run(bsa_ctx_t *ctx, const bsa_snv_model_t *model, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
		const uint32_t *d_cns_status, const bsa_snv_params_t *par, bsa_snv_t *d_snv, size_t snv_cap, uint64_t *d_snv_off, bsa_snv_window_t *d_rec){
	return sv_run_checked(ctx, SV_PREPARE | SV_COUNT | SV_FILL, model, d_cols, cols_cap, d_cwin, nwin, d_cns_status, par, d_snv, snv_cap, d_snv_off, d_rec);
}

// for tools/bench_window_snv.py: one step alone (step: 0 prepare, 1 the count with its scan, 2 the fill), once more, with the arguments of the
// context's last bsa_window_snv_run and on the scratch it left: nothing else may have used the context in between
extern "C" int bsa_window_snv_step_internal(bsa_ctx_t *ctx, int step, const bsa_snv_model_t *model, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin,
		size_t nwin, const uint32_t *d_cns_status, const bsa_snv_params_t *par, bsa_snv_t *d_snv, size_t snv_cap, uint64_t *d_snv_off, bsa_snv_window_t *d_rec){
	if(step < 0 || step > 2) return BSA_E_ARG;
	return sv_run_checked(ctx, 1 << step, model, d_cols, cols_cap, d_cwin, nwin, d_cns_status, par, d_snv, snv_cap, d_snv_off, d_rec);
}

struct sv_model_guard { bsa_snv_model_t *m = nullptr; ~sv_model_guard(){ bsa_snv_model_destroy(m); } };

extern "C" int bsa_window_snv_batch(bsa_ctx_t *ctx, uint32_t max_rows, const uint8_t *cols, size_t cols_cap, const bsa_cns_window_t *cwin, size_t nwin, const uint32_t *cns_status,
		const bsa_snv_params_t *par, bsa_snv_t *snv, size_t snv_cap, uint64_t *snv_off, bsa_snv_window_t *rec){
	if(!ctx) return BSA_E_ARG;
	int rc = sv_check(ctx, nullptr, false, cols, cols_cap, cwin, nwin, par, snv, snv_cap, snv_off, rec);
	if(rc != BSA_OK) return rc;
	if(max_rows > 1000u){ bsa_ctx_set_error_internal(ctx, "bsa_window_snv_batch: max_rows above 1000"); return BSA_E_UNSUPPORTED; }
	if(nwin == 0){ snv_off[0] = 0; return BSA_OK; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	sv_model_guard mg;                                                    // (declared in front of the stage: the stage waits for the stream before the model goes)
	if((rc = bsa_snv_model_create(ctx, max_rows, &mg.m)) != BSA_OK) return rc;
	// the arena goes up as it is: a range no window owns comes down as it went up
	bsa_stage_t in(ctx, stream);
	const size_t o_cols = in.part(cols_cap), o_cwin = in.part(nwin * sizeof(bsa_cns_window_t)), o_cst = in.part(cns_status ? nwin * 4u : 0u), o_off = in.part((nwin + 1u) * 8u),
		o_rec = in.part(nwin * sizeof(bsa_snv_window_t)), o_snv = in.part(snv_cap * sizeof(bsa_snv_t));
	if((rc = in.alloc("bsa_window_snv_batch: no device memory for the columns, the records and the outputs")) != BSA_OK) return rc;
	if(!in.up(o_cols, cols, cols_cap) || !in.up(o_cwin, cwin, nwin * sizeof(bsa_cns_window_t)) || (cns_status && !in.up(o_cst, cns_status, nwin * 4u))
			|| !in.up(o_snv, snv, snv_cap * sizeof(bsa_snv_t)))
		return in.fail("bsa_window_snv_batch: upload failed");
	rc = sv_run(ctx, stream, SV_PREPARE | SV_COUNT | SV_FILL, mg.m, cols_cap ? in.at<uint8_t>(o_cols) : nullptr, cols_cap, in.at<bsa_cns_window_t>(o_cwin), nwin,
		cns_status ? in.at<uint32_t>(o_cst) : nullptr, *par, snv_cap ? in.at<bsa_snv_t>(o_snv) : nullptr, snv_cap, in.at<uint64_t>(o_off), in.at<bsa_snv_window_t>(o_rec));
	if(rc != BSA_OK) return rc;
	if(!in.down(snv_off, o_off, (nwin + 1u) * 8u) || !in.down(rec, o_rec, nwin * sizeof(bsa_snv_window_t)) || !in.sync())
		return in.fail("bsa_window_snv_batch: download of the offsets and records failed");
	const uint64_t need = snv_off[nwin];                                  // (the offsets are down before the capacity is judged)
	if(need > snv_cap) return in.fail("bsa_window_snv_batch: snv_cap too small, snv_off[nwin] holds what is needed", BSA_E_CIGAR_CAP);
	if(!in.down(snv, o_snv, (size_t)need * sizeof(bsa_snv_t)) || !in.sync()) return in.fail("bsa_window_snv_batch: download of the results failed");
	return BSA_OK;
}
