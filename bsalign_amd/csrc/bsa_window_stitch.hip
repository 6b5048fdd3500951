// bsa_window_stitch.hip -- bsa_window_stitch_run / _batch (include/bsalign_hip.h): the stitched sequence of every window -- the consensus where enough
// reads cover a column, the draft where they do not -- and its alignment to the draft as = / X / I / D words.
//
// A pass over public outputs: the columns and the bsa_cns_window_t records as bsa_window_msa_run wrote them and bsa_window_cns_run filled them.  The
// columns are read-only here.  The steps on the context stream:
//   prepare : a thread a window (k_window_stitch_prepare) tests the readable record, copies what the pass needs of it into the context's scratch --
//             nothing reads the caller's record a second time -- and leaves mlen, or 0, for the scan;
//   scan    : bsa_scan.hip's exclusive scan of those values: t, the cursor of the column words;
//   cols    : a wave a window (k_window_stitch_cols) goes through the window's columns in tiles, classifies every column and leaves its 4-byte word
//             at t[g] + i; the window's counts go to d_rec, slen and ncig to the scans;
//   scans   : slen -> d_seq_off, ncig -> d_cig_off;
//   fill    : a wave a window (k_window_stitch_fill) over the column words only: bases to their places, every run's word to its place.
// The column words take 4 bytes for each of W = min(cols_cap / 4, max(seq_cap, cig_cap)) columns: the windows bsa_window_msa_run writes are disjoint and
// a column has at least 4 bytes, so their mlen sum to at most cols_cap / 4, and a caller who gives the sum of mlen as the caps (header: it always
// suffices) gets exactly that.  A window whose t[g + 1] lies above W -- records that overlap, or caps below the sum of mlen -- keeps no words: the
// fill classifies its columns again (ws_tile_words is the one copy of the rules, used by both kernels).  A count-only run has W = 0 and no fill.
// Plain C++; no kernel uses scratch memory.
#include "bsa_pass.h"

static_assert(sizeof(bsa_cns_window_t) == 40 && sizeof(bsa_stitch_t) == 32, "the records' layouts");

// a wave's tile of whole columns in LDS: 8176 bytes behind up to 15 bytes of shift (the tile lies in LDS as it lies in memory modulo 16), 8192 a wave
// and 32 KB a workgroup -- five workgroups a CU.  64 columns fit up to a stride of 127 bytes (nall 124), one column up to 8176 (nall 8173).
#define WS_LDS 8176u
// a column's word: bits 0..3 the unit's CIGAR op (0: no unit), WS_EMIT a base is emitted, WS_KEPT it is a kept draft base, then symbol, quality, alternative
#define WS_EMIT 0x10u
#define WS_KEPT 0x20u

struct ws_win_t { uint64_t cols_off; uint32_t nall, mlen, status, pad; };
enum { WS_PREPARE = 1, WS_COLS = 2, WS_FILL = 4 };

__global__ void __launch_bounds__(256) k_window_stitch_prepare(const bsa_cns_window_t *cwin, const uint32_t *cns_status, uint64_t cols_cap, uint32_t nwin, ws_win_t *wd,
		uint32_t *mlenv){
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if(g >= nwin) return;
	const bsa_cns_window_t w = cwin[g];
	ws_win_t d = { 0ull, 1u, 0u, BSA_STITCH_ST_BAD_RECORD, 0u };
	if(w.idxs_off == ~0ull && w.nall >= 1u && w.mlen < (1u << 28)){
		const uint64_t bytes = (uint64_t)w.mlen * ((uint64_t)w.nall + 3u);               // (below 2^28 (2^32 + 2): the product does not wrap)
		if(w.cols_off <= ~0ull - bytes && w.cols_off + bytes <= cols_cap){
			d.cols_off = w.cols_off; d.nall = w.nall; d.mlen = w.mlen;
			d.status = (cns_status && cns_status[g] != 0u) ? BSA_STITCH_ST_DRAFT : BSA_STITCH_ST_CALLED;
		}
	}
	wd[g] = d; mlenv[g] = d.mlen;
}

// n bytes into LDS where dst and src are congruent modulo 16: 16-byte vectors over the aligned middle, single bytes in front and behind, so that every
// vector lies inside the n bytes (n <= WS_LDS: at most 15 bytes at either end)
static __device__ __forceinline__ void ws_stage(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane){
	uint32_t head = (uint32_t)((0u - (uintptr_t)src) & 15u);
	if(head > n) head = n;
	const uint32_t nv = (n - head) / 16u, tail = head + nv * 16u;
	if(lane < head) dst[lane] = src[lane];
	for(uint32_t i = lane; i < nv; i += 64u) ((uint4*)(dst + head))[i] = ((const uint4*)(src + head))[i];
	if(tail + lane < n) dst[tail + lane] = src[tail + lane];
}

// the bytes of a dword that are 4 or less, as their top bits (no borrow crosses a byte: every byte is at least 0x80 before 5 is taken from it)
static __device__ __forceinline__ uint32_t ws_le4(uint32_t w){
	const uint32_t ge5 = ((w & 0x7F7F7F7Fu) | 0x80808080u) - 0x05050505u;
	return ~ge5 & ~w & 0x80808080u;
}

static __device__ __forceinline__ uint32_t ws_wave_sum(uint32_t v){
#pragma unroll
	for(int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// The rules of the header, once: the words of the columns i0 .. i0 + n of a readable window, lane l that of column i0 + l (0 for a lane without one).
// tcols: the columns of a tile that fit the wave's LDS -- n <= tcols <= 64 -- or 0: a column does not fit, and n <= 64 columns are taken one at a
// time with the lanes over the rows.
static __device__ __forceinline__ uint32_t ws_tile_words(const uint8_t *cols, const ws_win_t &w, uint32_t i0, uint32_t n, uint32_t tcols, uint8_t *lds, uint32_t min_cov,
		uint32_t lane){
	const uint64_t stride = (uint64_t)w.nall + 3u;
	const uint8_t *src = cols + w.cols_off + (uint64_t)i0 * stride;
	uint32_t cov = 0, d = 0, c = 0, q = 0, a = 0;
	if(tcols){
		const uint32_t s = (uint32_t)stride, shift = (uint32_t)((uintptr_t)src & 15u);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // (the reads of the tile in front are done before this one lands)
		__builtin_amdgcn_wave_barrier();
		ws_stage(lds + shift, src, n * s, lane);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		if(lane < n){
			// the piece rows [b0, b1) by aligned dwords, the bytes outside masked away (LDS is a multiple of 4 bytes: no dword leaves it)
			const uint32_t b0 = shift + lane * s, b1 = b0 + w.nall - 1u;
			for(uint32_t k = b0 & ~3u; k < b1; k += 4u){
				uint32_t m = 0x80808080u;
				if(k < b0) m <<= (b0 - k) * 8u;
				if(k + 4u > b1) m &= 0x80808080u >> ((k + 4u - b1) * 8u);
				cov += (uint32_t)__popc(ws_le4(*(const uint32_t*)(lds + k)) & m);
			}
			d = lds[b1]; c = lds[b1 + 1u]; q = lds[b1 + 2u]; a = lds[b1 + 3u];
		}
	} else {
		for(uint32_t j = 0; j < n; j++){
			const uint8_t *col = src + (uint64_t)j * stride;
			uint32_t cnt = 0;
			for(uint64_t r = lane; r < (uint64_t)w.nall - 1u; r += 64u) cnt += col[r] <= 4u ? 1u : 0u;
			cnt = ws_wave_sum(cnt);
			if(lane == j){ cov = cnt; d = col[w.nall - 1u]; c = col[w.nall]; q = col[(uint64_t)w.nall + 1u]; a = col[(uint64_t)w.nall + 2u]; }
		}
	}
	if(lane >= n) return 0u;
	if(w.status == BSA_STITCH_ST_CALLED && cov >= min_cov){
		const uint32_t kind = d > 3u ? (c > 3u ? 0u : (uint32_t)BSA_CIGAR_I) : c > 3u ? (uint32_t)BSA_CIGAR_D : c == d ? (uint32_t)BSA_CIGAR_EQ : (uint32_t)BSA_CIGAR_X;
		return c <= 3u ? (kind | WS_EMIT | c << 8 | q << 16 | a << 24) : kind;
	}
	return d <= 3u ? ((uint32_t)BSA_CIGAR_EQ | WS_EMIT | WS_KEPT | d << 8) : 0u;
}

// the columns of a tile: 64, fewer where 64 do not fit the wave's LDS, 0 where not even one does
static __device__ __forceinline__ uint32_t ws_tile_cols(uint32_t nall){
	const uint64_t stride = (uint64_t)nall + 3u;
	if(stride > WS_LDS) return 0u;
	const uint32_t fit = WS_LDS / (uint32_t)stride;
	return fit < 64u ? fit : 64u;
}

// does the lane's unit begin a run: its kind differs from that of the unit in front -- the nearest lane below with a unit, or the one the tiles in
// front left open (`open`, 0 at the window's start).  U: the ballot of the lanes with a unit.  Every lane calls it.
static __device__ __forceinline__ bool ws_run_start(uint32_t kind, uint64_t U, uint32_t open, uint32_t lane){
	const uint64_t below = U & ((1ull << lane) - 1ull);
	const uint32_t pk = (uint32_t)__shfl((int)kind, below ? 63 - __clzll((long long)below) : (int)lane);
	return kind != 0u && kind != (below ? pk : open);
}

// a wave a window, four a workgroup
__global__ void __launch_bounds__(256) k_window_stitch_cols(uint32_t nwin, const ws_win_t *wd, const uint64_t *t, uint64_t wcap, const uint8_t *cols, uint32_t min_cov,
		uint32_t *words, bsa_stitch_t *rec, uint32_t *slenv, uint32_t *ncigv){
	__shared__ uint4 tile[4][(WS_LDS + 16u) / 16u];
	const uint32_t lane = threadIdx.x & 63u;
	uint8_t *lds = (uint8_t*)tile[threadIdx.x >> 6];
	for(uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); g < nwin; g += (uint64_t)gridDim.x * 4u){
		const ws_win_t w = wd[g];
		uint32_t slen = 0, eq = 0, x = 0, ins = 0, del = 0, kept = 0, ncig = 0;
		if(w.status != BSA_STITCH_ST_BAD_RECORD && w.mlen){
			const uint32_t tcols = ws_tile_cols(w.nall), step = tcols ? tcols : 64u;
			const uint64_t t0 = t[g];
			const bool room = t[g + 1u] <= wcap;
			uint32_t open = 0;
			for(uint32_t i0 = 0; i0 < w.mlen; i0 += step){
				const uint32_t n = w.mlen - i0 < step ? w.mlen - i0 : step;
				const uint32_t word = ws_tile_words(cols, w, i0, n, tcols, lds, min_cov, lane);
				if(room && lane < n) words[t0 + i0 + lane] = word;
				const uint32_t kind = word & 15u;
				const uint64_t U = __ballot(kind != 0u);
				ncig += (uint32_t)__popcll(__ballot(ws_run_start(kind, U, open, lane)));
				slen += (uint32_t)__popcll(__ballot((word & WS_EMIT) != 0u));
				kept += (uint32_t)__popcll(__ballot((word & WS_KEPT) != 0u));
				eq += (uint32_t)__popcll(__ballot(kind == BSA_CIGAR_EQ));
				x += (uint32_t)__popcll(__ballot(kind == BSA_CIGAR_X));
				ins += (uint32_t)__popcll(__ballot(kind == BSA_CIGAR_I));
				del += (uint32_t)__popcll(__ballot(kind == BSA_CIGAR_D));
				if(U) open = (uint32_t)__shfl((int)kind, 63 - __clzll((long long)U));
			}
		}
		if(lane == 0){
			const bsa_stitch_t r = { w.status, slen, eq, x, ins, del, kept, ncig };
			rec[g] = r; slenv[g] = slen; ncigv[g] = ncig;
		}
	}
}

// a wave a window, four a workgroup, over the column words (a window that kept none classifies its columns again)
__global__ void __launch_bounds__(256) k_window_stitch_fill(uint32_t nwin, const ws_win_t *wd, const uint64_t *t, uint64_t wcap, const uint8_t *cols, uint32_t min_cov,
		const uint32_t *words, const uint64_t *seq_off, uint64_t seq_cap, const uint64_t *cig_off, uint64_t cig_cap, uint8_t *seq, uint8_t *seq_qlt, uint8_t *seq_alt,
		uint32_t *cig){
	__shared__ uint4 tile[4][(WS_LDS + 16u) / 16u];
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t lt = (1ull << lane) - 1ull;
	uint8_t *lds = (uint8_t*)tile[threadIdx.x >> 6];
	for(uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); g < nwin; g += (uint64_t)gridDim.x * 4u){
		const ws_win_t w = wd[g];
		if(w.status == BSA_STITCH_ST_BAD_RECORD || !w.mlen) continue;
		const uint64_t s0 = seq_off[g], s1 = seq_off[g + 1u], c0 = cig_off[g], c1 = cig_off[g + 1u];
		const bool fits_s = s1 <= seq_cap && s1 > s0, fits_c = c1 <= cig_cap && c1 > c0;      // each arena has its own test
		if(!fits_s && !fits_c) continue;
		const uint32_t tcols = ws_tile_cols(w.nall);
		const uint64_t t0 = t[g];
		const bool room = t[g + 1u] <= wcap;
		const uint32_t step = (room || !tcols) ? 64u : tcols;
		uint64_t sp = s0, cp = c0;                                      // where the next base and the next run's word go
		uint32_t open = 0, open_len = 0;                                  // the run the tiles in front left open: its kind (0: none) and units; its word is cp - 1
		for(uint32_t i0 = 0; i0 < w.mlen; i0 += step){
			const uint32_t n = w.mlen - i0 < step ? w.mlen - i0 : step;
			const uint32_t word = room ? (lane < n ? words[t0 + i0 + lane] : 0u) : ws_tile_words(cols, w, i0, n, tcols, lds, min_cov, lane);
			const uint64_t E = __ballot((word & WS_EMIT) != 0u);
			if(fits_s && (word & WS_EMIT)){
				const uint64_t p = sp + (uint32_t)__popcll(E & lt);
				if(p < s1){
					seq[p] = (uint8_t)(word >> 8);
					if(seq_qlt) seq_qlt[p] = (uint8_t)(word >> 16);
					if(seq_alt) seq_alt[p] = (uint8_t)(word >> 24);
				}
			}
			sp += (uint32_t)__popcll(E);
			const uint32_t kind = word & 15u;
			const uint64_t U = __ballot(kind != 0u);
			const bool start = ws_run_start(kind, U, open, lane);
			const uint64_t S = __ballot(start);
			const uint32_t rank = (uint32_t)__popcll(U & lt), nu = (uint32_t)__popcll(U);      // the units below the lane, and of the tile
			if(S){
				// the units in front of the tile's first start end the open run; every start but the last ends at the next start; the last stays open
				const uint32_t first = (uint32_t)__popcll(U & ((1ull << (__ffsll((long long)S) - 1)) - 1ull));
				if(fits_c && open && lane == 0 && cp - 1u < c1) cig[cp - 1u] = (open_len + first) << 4 | open;
				const uint64_t above = S & ~((2ull << lane) - 1ull);
				const uint32_t nr = (uint32_t)__shfl((int)rank, above ? __ffsll((long long)above) - 1 : (int)lane);
				const uint64_t p = cp + (uint32_t)__popcll(S & lt);
				if(fits_c && start && above && p < c1) cig[p] = (nr - rank) << 4 | kind;
				const int last = 63 - __clzll((long long)S);
				open = (uint32_t)__shfl((int)kind, last);
				open_len = nu - (uint32_t)__shfl((int)rank, last);
				cp += (uint32_t)__popcll(S);
			} else open_len += nu;
		}
		if(fits_c && open && lane == 0 && cp - 1u < c1) cig[cp - 1u] = open_len << 4 | open;
	}
}

// the argument errors of both calls
static int ws_check(bsa_ctx_t *ctx, const void *cols, size_t cols_cap, const void *cwin, size_t nwin, const void *seq, const void *seq_qlt, const void *seq_alt, size_t seq_cap,
		const void *seq_off, const void *cig, size_t cig_cap, const void *cig_off, const void *rec){
	const char *msg = nullptr;
	if(!seq_off || !cig_off || (nwin && (!cwin || !rec)) || (cols_cap && !cols) || (seq_cap && !seq) || (cig_cap && !cig)) msg = "bsa_window_stitch: null argument";
	else if(!seq && (seq_qlt || seq_alt)) msg = "bsa_window_stitch: a quality array without seq";
	else if(nwin > 0xFFFFFFF0ull) msg = "too many windows";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	return BSA_OK;
}

// the steps of `steps`, in order (one alone only for tools/bench_window_stitch.py, on the scratch a whole run left)
static int ws_run(bsa_ctx_t *ctx, hipStream_t st, int steps, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin, const uint32_t *d_cns_status,
		uint32_t min_cov, uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off, uint32_t *d_cig, size_t cig_cap, uint64_t *d_cig_off,
		bsa_stitch_t *d_rec){
	hipError_t e = hipSuccess;
	if(nwin == 0){
		e = bsa_launch_excl_scan(st, (const uint32_t*)nullptr, d_seq_off, 0u, nullptr, nullptr);          // d_seq_off[0] = 0
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)nullptr, d_cig_off, 0u, nullptr, nullptr);
		if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_stitch: launch failed"); return BSA_E_HIP; }
		return BSA_OK;
	}
	// scratch: 24 + 3 x 4 + 8 bytes a window and the scans' temporaries; then 4 bytes a column word
	const uint64_t wcap = std::min<uint64_t>((uint64_t)cols_cap / 4u, std::max<uint64_t>(seq_cap, cig_cap));
	if(wcap > ((uint64_t)1 << 40)){ bsa_ctx_set_error_internal(ctx, "bsa_window_stitch: no scratch for caps this large"); return BSA_E_NOMEM; }
	const size_t o_wd = 0, o_mlen = o_wd + bsa_up256(nwin * sizeof(ws_win_t)), o_slen = o_mlen + bsa_up256(nwin * 4u), o_ncig = o_slen + bsa_up256(nwin * 4u),
		o_t = o_ncig + bsa_up256(nwin * 4u), o_tmp = o_t + bsa_up256((nwin + 1u) * 8u), o_words = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)nwin)),
		total = o_words + bsa_up256((size_t)wcap * 4u);
	void *bufv = nullptr;
	int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);              // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	ws_win_t *wd = (ws_win_t*)(b + o_wd);
	uint32_t *mlenv = (uint32_t*)(b + o_mlen), *slenv = (uint32_t*)(b + o_slen), *ncigv = (uint32_t*)(b + o_ncig), *words = (uint32_t*)(b + o_words);
	uint64_t *t = (uint64_t*)(b + o_t), *tmp = (uint64_t*)(b + o_tmp);
	const size_t want = (nwin + 3u) / 4u, most = (size_t)bsa_cus() * 16u;
	const dim3 waves((uint32_t)(want < most ? want : most));
	if(steps & WS_PREPARE){
		hipLaunchKernelGGL(k_window_stitch_prepare, dim3((uint32_t)(((uint64_t)nwin + 255u) / 256u)), dim3(256), 0, st, d_cwin, d_cns_status, (uint64_t)cols_cap, (uint32_t)nwin, wd, mlenv);
		e = hipGetLastError();
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)mlenv, t, (uint32_t)nwin, nullptr, tmp);
	}
	if(e == hipSuccess && (steps & WS_COLS)){
		hipLaunchKernelGGL(k_window_stitch_cols, waves, dim3(256), 0, st, (uint32_t)nwin, (const ws_win_t*)wd, (const uint64_t*)t, wcap, d_cols, min_cov, words, d_rec, slenv, ncigv);
		e = hipGetLastError();
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)slenv, d_seq_off, (uint32_t)nwin, nullptr, tmp);
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)ncigv, d_cig_off, (uint32_t)nwin, nullptr, tmp);
	}
	if(e == hipSuccess && (steps & WS_FILL) && (seq_cap || cig_cap)){
		hipLaunchKernelGGL(k_window_stitch_fill, waves, dim3(256), 0, st, (uint32_t)nwin, (const ws_win_t*)wd, (const uint64_t*)t, wcap, d_cols, min_cov, (const uint32_t*)words,
			(const uint64_t*)d_seq_off, (uint64_t)seq_cap, (const uint64_t*)d_cig_off, (uint64_t)cig_cap, d_seq, d_seq_qlt, d_seq_alt, d_cig);
		e = hipGetLastError();
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_stitch: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

static int ws_run_checked(bsa_ctx_t *ctx, int steps, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin, const uint32_t *d_cns_status, uint32_t min_cov,
		uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off, uint32_t *d_cig, size_t cig_cap, uint64_t *d_cig_off, bsa_stitch_t *d_rec){
	if(!ctx) return BSA_E_ARG;
	int rc = ws_check(ctx, d_cols, cols_cap, d_cwin, nwin, d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, d_rec);
	if(rc != BSA_OK) return rc;
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	return ws_run(ctx, stream, steps, d_cols, cols_cap, d_cwin, nwin, d_cns_status, min_cov, d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, d_rec);
}

extern "C" int bsa_window_stitch_run(bsa_ctx_t *ctx, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin, const uint32_t *d_cns_status, uint32_t min_cov,
		uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off, uint32_t *d_cig, size_t cig_cap, uint64_t *d_cig_off, bsa_stitch_t *d_rec){
	return ws_run_checked(ctx, WS_PREPARE | WS_COLS | WS_FILL, d_cols, cols_cap, d_cwin, nwin, d_cns_status, min_cov, d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off,
		d_cig, cig_cap, d_cig_off, d_rec);
}

// for tools/bench_window_stitch.py: one step alone (step: 0 prepare with its scan, 1 the columns with the two scans, 2 the fill), once more, with the
// arguments of the context's last bsa_window_stitch_run and on the scratch it left: nothing else may have used the context in between
extern "C" int bsa_window_stitch_step_internal(bsa_ctx_t *ctx, int step, const uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
		const uint32_t *d_cns_status, uint32_t min_cov, uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off, uint32_t *d_cig, size_t cig_cap,
		uint64_t *d_cig_off, bsa_stitch_t *d_rec){
	if(step < 0 || step > 2) return BSA_E_ARG;
	return ws_run_checked(ctx, 1 << step, d_cols, cols_cap, d_cwin, nwin, d_cns_status, min_cov, d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, d_rec);
}

extern "C" int bsa_window_stitch_batch(bsa_ctx_t *ctx, const uint8_t *cols, size_t cols_cap, const bsa_cns_window_t *cwin, size_t nwin, const uint32_t *cns_status, uint32_t min_cov,
		uint8_t *seq, uint8_t *seq_qlt, uint8_t *seq_alt, size_t seq_cap, uint64_t *seq_off, uint32_t *cig, size_t cig_cap, uint64_t *cig_off, bsa_stitch_t *rec){
	if(!ctx) return BSA_E_ARG;
	int rc = ws_check(ctx, cols, cols_cap, cwin, nwin, seq, seq_qlt, seq_alt, seq_cap, seq_off, cig, cig_cap, cig_off, rec);
	if(rc != BSA_OK) return rc;
	if(nwin == 0){ seq_off[0] = 0; cig_off[0] = 0; return BSA_OK; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	// the arenas go up as they are: a range no window owns comes down as it went up
	bsa_stage_t in(ctx, stream);
	const size_t o_cols = in.part(cols_cap), o_cwin = in.part(nwin * sizeof(bsa_cns_window_t)), o_cst = in.part(cns_status ? nwin * 4u : 0u), o_soff = in.part((nwin + 1u) * 8u),
		o_coff = in.part((nwin + 1u) * 8u), o_rec = in.part(nwin * sizeof(bsa_stitch_t)), o_seq = in.part(seq_cap), o_sq = in.part(seq_qlt ? seq_cap : 0u),
		o_sa = in.part(seq_alt ? seq_cap : 0u), o_cig = in.part(cig_cap * 4u);
	if((rc = in.alloc("bsa_window_stitch_batch: no device memory for the columns, the records and the outputs")) != BSA_OK) return rc;
	if(!in.up(o_cols, cols, cols_cap) || !in.up(o_cwin, cwin, nwin * sizeof(bsa_cns_window_t)) || (cns_status && !in.up(o_cst, cns_status, nwin * 4u))
			|| !in.up(o_seq, seq, seq_cap) || (seq_qlt && !in.up(o_sq, seq_qlt, seq_cap)) || (seq_alt && !in.up(o_sa, seq_alt, seq_cap)) || !in.up(o_cig, cig, cig_cap * 4u))
		return in.fail("bsa_window_stitch_batch: upload failed");
	rc = ws_run(ctx, stream, WS_PREPARE | WS_COLS | WS_FILL, cols_cap ? in.at<uint8_t>(o_cols) : nullptr, cols_cap, in.at<bsa_cns_window_t>(o_cwin), nwin,
		cns_status ? in.at<uint32_t>(o_cst) : nullptr, min_cov, seq_cap ? in.at<uint8_t>(o_seq) : nullptr, (seq_cap && seq_qlt) ? in.at<uint8_t>(o_sq) : nullptr,
		(seq_cap && seq_alt) ? in.at<uint8_t>(o_sa) : nullptr, seq_cap, in.at<uint64_t>(o_soff), cig_cap ? in.at<uint32_t>(o_cig) : nullptr, cig_cap, in.at<uint64_t>(o_coff),
		in.at<bsa_stitch_t>(o_rec));
	if(rc != BSA_OK) return rc;
	if(!in.down(seq_off, o_soff, (nwin + 1u) * 8u) || !in.down(cig_off, o_coff, (nwin + 1u) * 8u) || !in.down(rec, o_rec, nwin * sizeof(bsa_stitch_t)) || !in.sync())
		return in.fail("bsa_window_stitch_batch: download of the offsets and records failed");
	const uint64_t need_s = seq_off[nwin], need_c = cig_off[nwin];        // (the offsets are down before the capacities are judged)
	if(need_s > seq_cap || need_c > cig_cap)
		return in.fail("bsa_window_stitch_batch: seq_cap or cig_cap too small, seq_off[nwin] and cig_off[nwin] hold what is needed", BSA_E_CIGAR_CAP);
	if(!in.down(seq, o_seq, (size_t)need_s) || (seq_qlt && !in.down(seq_qlt, o_sq, (size_t)need_s)) || (seq_alt && !in.down(seq_alt, o_sa, (size_t)need_s))
			|| !in.down(cig, o_cig, (size_t)need_c * 4u) || !in.sync())
		return in.fail("bsa_window_stitch_batch: download of the results failed");
	return BSA_OK;
}
