// bsa_window_msa.hip -- bsa_window_msa_run / _batch (include/bsalign_hip.h): every window's pieces and their guides turned into the window's
// draft-anchored MSA in the `msacols` layout (include/bsalign_msa.h) that bsa_msa_call_consensus_batch, bsa_msa_text and bsa_msa_binary_write take,
// with the bsa_cns_window_t record of every window.
//
// A pass over public outputs: the piece records and codes of bsa_window_pieces_run, the words and offsets of bsa_piece_cigars_run, and the caller's
// draft.  It knows no plan and no aligner.  Four steps on the context stream:
//   cols    : one wave a window (k_window_msa_cols), a lane a piece.  A lane tests its piece's live predicate (one walk over its words) and, if the
//             piece is live, walks once more and raises ins[j] in LDS with atomicMax (an integer maximum does not depend on the order).  The wave
//             then scans the line in place: c[j] = j + ins[0] + .. + ins[j], mlen = L + the sum (64 bits).  It leaves the line c (4 bytes a draft
//             column), mlen, the depth, the window's bytes and every piece's flag in the context's scratch.
//   scan    : the exclusive scans of bsa_scan.hip: the bytes (64-bit values) into d_cols_off, mlen into the records' out_off;
//   records : a thread a window writes d_cwin (k_window_msa_records);
//   fill    : a workgroup a window that fits (k_window_msa_fill).  A window's columns are one contiguous byte range.  The workgroup builds it
//             in LDS, a tile of whole columns (at most WM_TILE - 16 bytes) at a time, laid out as it lies in its 16-byte lines in the arena.
//             Defaults first (a thread 16 bytes: 5 in a piece row, 4 in the draft row, 4 0 0 behind), then the draft's bases, then every
//             live piece's symbols: a thread a piece, the pieces dealt out over the four waves.  The walk's state stays in registers from
//             tile to tile, so a guide is walked once.  The tile goes out with aligned 16-byte vector stores; only the bytes of a 16-byte
//             line that it shares with its neighbour go out one by one.  HBM sees no store with a stride of depth + 4.
//             A window of more than 256 rows is written in place with byte stores (no polisher makes one; every shape is served).
// A lane a piece, and not 16 lanes as in bsa_piece_cigars.hip: I words that follow each other (the pieces are the caller's own arrays) add up
// in front of ONE column, which a serial walk gets right without a segmented scan.  It is also why the fill is slow: the lanes
// of a wave leave the unit loop together, so a wave makes as many trips as its longest words ask for, each behind a load of its own.
// The piece's flag in scratch holds only what does not depend on the window (the words, the sums, the codes); the clause that does (b < L) is tested
// again from the record wherever the flag is read, so that piece_off arrays that put one piece into two windows cannot make two writers disagree.
// Plain C++ with vector loads and stores and LDS atomics; no kernel uses scratch memory.
#include "bsa_pass.h"
#include "../../include/bsalign_msa.h"
#include <vector>

#define WM_MAX_WINDOW 4096u        // the line of a window (4 bytes a draft column) stays in LDS
#define WM_TILE 8192u              // bytes of a window the fill builds in LDS at a time (a multiple of 4096: 256 threads of 16 bytes)
#define WM_MLEN_END 0x80000000ull  // a window whose mlen would reach this has mlen 0 and no bytes

static_assert(sizeof(bsa_cns_window_t) == 40 && sizeof(bsa_piece_t) == 32, "the records' layouts");

struct wm_in_t {
	const bsa_piece_t *piece; const uint64_t *piece_off; uint64_t piece_cap; const uint8_t *bases; uint64_t bases_cap;
	const uint32_t *pcig; uint64_t pcig_cap; const uint64_t *pcig_off; const uint8_t *draft; const uint64_t *doff; const uint32_t *dlen;
	uint32_t nwin, window, packed, vote;
};

// window g's first piece and depth: 0 rows where the offsets cannot be used
static __device__ __forceinline__ uint32_t wm_depth(const wm_in_t &in, uint32_t g, uint64_t *p0){
	const uint64_t x = in.piece_off[g], y = in.piece_off[g + 1u];
	*p0 = x;
	return (y > in.piece_cap || y < x) ? 0u : (uint32_t)(y - x);      // (piece_cap <= 0xFFFFFFF0)
}
static __device__ __forceinline__ uint32_t wm_draft_len(const wm_in_t &in, uint32_t g){ const uint32_t d = in.dlen[g]; return d < in.window ? d : in.window; }

// the clause of the live predicate that depends on the window: a = t_first % window, b = a + (t_last - t_first) < L.  -> a
static __device__ __forceinline__ bool wm_in_window(const bsa_piece_t &pc, uint32_t window, uint32_t L, uint32_t *a){
	if(pc.t_last < pc.t_first) return false;                  // (no words' lengths sum to t_last - t_first + 1 <= 0)
	*a = pc.t_first % window;
	return (uint64_t)*a + (pc.t_last - pc.t_first) < L;
}

// the clauses that do not: the words are there and readable, every one steps and has a length, the first and the last are diagonal, the two sums
// (64 bits), len >= 1 and the codes inside bases_cap.  Every word adds to one of the sums, so the walk ends after at most len + (t_last - t_first) + 2
// words whatever the offsets say.
static __device__ bool wm_words_ok(const wm_in_t &in, uint64_t j, const bsa_piece_t &pc){
	const uint64_t o0 = in.pcig_off[j], o1 = in.pcig_off[j + 1u];
	if(!(o0 < o1 && o1 <= in.pcig_cap)) return false;
	if(pc.len == 0u || pc.base_off > in.bases_cap || pc.len > in.bases_cap - pc.base_off) return false;
	const uint64_t want_q = pc.len, want_t = (uint64_t)(pc.t_last - pc.t_first) + 1u;
	if(!bsa_cig_diag(in.pcig[o0] & 15u) || !bsa_cig_diag(in.pcig[o1 - 1u] & 15u)) return false;
	uint64_t qs = 0, ts = 0;
	for(uint64_t i = o0; i < o1; i++){
		const uint32_t w = in.pcig[i], op = w & 15u, len = w >> 4;
		if(!bsa_cig_steps(op) || len == 0u) return false;
		qs += bsa_cig_qadd(op, len); ts += bsa_cig_tadd(op, len);
		if(qs > want_q || ts > want_t) return false;
	}
	return qs == want_q && ts == want_t;
}

// one wave a window.  LDS: the window's line, `window` words.
__global__ void __launch_bounds__(64) k_window_msa_cols(const wm_in_t in, uint8_t *live, uint32_t *cline, uint32_t *depthv, uint32_t *mlenv, uint64_t *bytesv){
	extern __shared__ uint32_t wm_ins[];
	const uint32_t lane = threadIdx.x;
	for(uint64_t gg = blockIdx.x; gg < in.nwin; gg += gridDim.x){
		const uint32_t g = (uint32_t)gg;
		uint64_t p0;
		const uint32_t depth = wm_depth(in, g, &p0), L = wm_draft_len(in, g);
		for(uint32_t j = lane; j < L; j += 64u) wm_ins[j] = 0u;
		__syncthreads();
		for(uint64_t r = lane; r < depth; r += 64u){
			const uint64_t j = p0 + r;
			const bsa_piece_t pc = in.piece[j];
			uint32_t a;
			if(!wm_in_window(pc, in.window, L, &a)) continue;      // (its flag is read nowhere for this window)
			const bool ok = wm_words_ok(in, j, pc);
			live[j] = ok ? 1u : 0u;
			if(!ok) continue;
			const uint64_t o0 = in.pcig_off[j], o1 = in.pcig_off[j + 1u];
			uint32_t col = a, run = 0;                             // the draft column the next word starts at, the I units in front of it
			for(uint64_t i = o0; i < o1; i++){
				const uint32_t w = in.pcig[i], op = w & 15u, len = w >> 4;
				if(op == BSA_CIGAR_I){ run += len; continue; }      // (I words that follow each other stand in front of one column; at most len units: 32 bits)
				if(run){ atomicMax(&wm_ins[col], run); run = 0u; }  // (col <= b < L: the sums were tested)
				col += len;
			}
		}
		__syncthreads();
		// c[j] = j + ins[0] + .. + ins[j], a lane a stretch of the line
		const uint32_t per = (L + 63u) / 64u, lo = lane * per < L ? lane * per : L, hi = lo + per < L ? lo + per : L;
		uint64_t s = 0;
		for(uint32_t j = lo; j < hi; j++) s += wm_ins[j];
		const uint64_t incl = bsa_wave_iscan<uint64_t>(s, lane);
		const uint64_t m = (uint64_t)L + __shfl(incl, 63);
		const bool fits = m < WM_MLEN_END;
		if(fits){
			uint64_t run = incl - s;
			for(uint32_t j = lo; j < hi; j++){ run += wm_ins[j]; wm_ins[j] = j + (uint32_t)run; }
		}
		__syncthreads();
		if(fits) for(uint32_t j = lane; j < L; j += 64u) cline[(uint64_t)g * in.window + j] = wm_ins[j];
		if(lane == 0u){ depthv[g] = depth; mlenv[g] = fits ? (uint32_t)m : 0u; bytesv[g] = fits ? m * ((uint64_t)depth + 4u) : 0ull; }
		__syncthreads();
	}
}

__global__ void __launch_bounds__(256) k_window_msa_records(uint32_t nwin, uint32_t vote, const uint32_t *depthv, const uint32_t *mlenv, const uint64_t *cols_off, const uint64_t *out_off,
		bsa_cns_window_t *cwin){
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if(g >= nwin) return;
	bsa_cns_window_t w;
	w.cols_off = cols_off[g]; w.idxs_off = ~0ull; w.out_off = out_off[g];
	w.nall = depthv[g] + 1u; w.nseq = w.nmax = depthv[g] + vote; w.mlen = mlenv[g];
	cwin[g] = w;
}

// a byte of a piece row, the draft row, the three consensus bytes
static __device__ __forceinline__ uint32_t wm_default(uint64_t row, uint32_t depth){ return row < depth ? 5u : row <= (uint64_t)depth + 1u ? 4u : 0u; }

// a live piece's walk, kept in registers between the tiles of its window: the word and the unit in it that come next, the draft column and the code
// the word starts at, the I units in front of it and their first code; a: the piece's first draft column
struct wm_walk_t { uint64_t i, o1; const uint8_t *code; uint32_t u, jd, qi, run, qrun, a; };

static __device__ __forceinline__ bool wm_walk_begin(const wm_in_t &in, const uint8_t *live, uint64_t j, uint32_t L, wm_walk_t *s){
	const bsa_piece_t pc = in.piece[j];
	uint32_t a;
	if(!wm_in_window(pc, in.window, L, &a) || !live[j]) return false;
	s->i = in.pcig_off[j]; s->o1 = in.pcig_off[j + 1u]; s->code = in.bases + pc.base_off;
	s->u = 0u; s->jd = a; s->qi = 0u; s->run = 0u; s->qrun = 0u; s->a = a;
	return true;
}

// where a symbol goes: a tile in LDS that starts with row 0 of column col_lo, or (DIRECT) the window's own bytes in the arena
template<bool DIRECT>
static __device__ __forceinline__ void wm_put(uint8_t *dst, uint64_t mrow, uint32_t col_lo, uint32_t col, uint64_t r, uint32_t val){
	if(DIRECT) dst[(uint64_t)col * mrow + r] = (uint8_t)val;
	else dst[(col - col_lo) * (uint32_t)mrow + (uint32_t)r] = (uint8_t)val;
}

// Row r's symbols in the columns col_lo .. col_hi; stops at the first unit that has a column behind col_hi and leaves it to the next call, which
// walks that unit again (its columns in front of the new col_lo are skipped there).  The tiles of a window go through its columns in order.
template<bool DIRECT>
static __device__ void wm_advance(wm_walk_t &s, const uint32_t *pcig, const uint32_t *c, uint8_t *dst, uint64_t mrow, uint64_t r, uint32_t col_lo, uint32_t col_hi){
	while(s.i < s.o1){
		const uint32_t w = pcig[s.i], op = w & 15u, len = w >> 4;
		if(op == BSA_CIGAR_I){ if(s.run == 0u) s.qrun = s.qi; s.run += len; s.qi += len; s.i++; continue; }
		const bool dg = op != BSA_CIGAR_D;
		for(; s.u < len; s.u++){
			const uint32_t jj = s.jd + s.u, cj = c[jj];              // (jj <= b < L: the piece is live)
			if(jj > s.a){                                          // the insertion columns in front of column jj: the piece's bases left-aligned, then 4
				const uint32_t cp = c[jj - 1u];
				if(cp + 1u > col_hi) return;
				const uint32_t end = cj <= col_hi ? cj : col_hi + 1u;
				for(uint32_t col = cp + 1u > col_lo ? cp + 1u : col_lo; col < end; col++){
					const uint32_t kk = col - cp - 1u;
					wm_put<DIRECT>(dst, mrow, col_lo, col, r, (s.u == 0u && kk < s.run) ? (uint32_t)(s.code[s.qrun + kk] & 3u) : 4u);
				}
			}
			if(cj > col_hi) return;
			if(cj >= col_lo) wm_put<DIRECT>(dst, mrow, col_lo, cj, r, dg ? (uint32_t)(s.code[s.qi + s.u] & 3u) : 4u);
		}
		s.jd += len; if(dg) s.qi += len; s.run = 0u; s.u = 0u; s.i++;
	}
}

static __device__ __forceinline__ uint32_t wm_draft_base(const wm_in_t &in, uint32_t g, uint32_t j){
	const uint64_t pos = in.doff[g] + j;
	return (in.packed ? (uint32_t)(((const uint64_t*)in.draft)[pos >> 5] >> (62u - 2u * (uint32_t)(pos & 31u))) : (uint32_t)in.draft[pos]) & 3u;
}

// One workgroup a window whose range ends inside the arena.  LDS: the tile (WM_TILE bytes), then the window's line c.  A window of up to 256 rows:
// a thread a piece for the whole window, tiles of whole columns.  A deeper one (its column alone may not fit a tile, and its pieces do not fit the
// threads) is written in place: defaults, a barrier, then the symbols with byte stores -- the slow way for a shape no polisher makes.
__global__ void __launch_bounds__(256) k_window_msa_fill(const wm_in_t in, const uint8_t *live, const uint32_t *cline, const uint32_t *mlenv, const uint64_t *cols_off,
		uint8_t *cols, uint64_t cols_cap){
	extern __shared__ uint4 wm_lds[];
	uint8_t *tile = (uint8_t*)wm_lds;
	uint32_t *c = (uint32_t*)(tile + WM_TILE);
	const uint32_t tid = threadIdx.x;
	for(uint64_t gg = blockIdx.x; gg < in.nwin; gg += gridDim.x){
		const uint32_t g = (uint32_t)gg;
		const uint64_t e0 = cols_off[g], e1 = cols_off[g + 1u];
		const uint32_t mlen = mlenv[g];
		uint64_t p0;
		const uint32_t depth = wm_depth(in, g, &p0), L = wm_draft_len(in, g);
		const uint64_t mrow = (uint64_t)depth + 4u;
		if(mlen == 0u || e1 > cols_cap || e1 < e0 || e1 - e0 != mlen * mrow) continue;      // (the offsets are this pass's own scan of the same bytes; the whole workgroup agrees)
		__syncthreads();
		for(uint32_t j = tid; j < L; j += 256u) c[j] = cline[(uint64_t)g * in.window + j];
		__syncthreads();
		uint8_t *dst = cols + e0;
		wm_walk_t s;
		if(depth > 256u){
			for(uint64_t p = tid; p < e1 - e0; p += 256u) dst[p] = (uint8_t)wm_default(p % mrow, depth);
			__syncthreads();
			for(uint32_t j = tid; j < L; j += 256u) dst[(uint64_t)c[j] * mrow + depth] = (uint8_t)wm_draft_base(in, g, j);
			for(uint64_t r = tid; r < depth; r += 256u)
				if(wm_walk_begin(in, live, p0 + r, L, &s)) wm_advance<true>(s, in.pcig, c, dst, mrow, r, 0u, mlen - 1u);
			continue;
		}
		const uint32_t r = (tid & 63u) * 4u + (tid >> 6);          // rows 0, 1, 2, 3 go to lane 0 of the four waves (measured against the first wave filled first)
		const bool walk = r < depth && wm_walk_begin(in, live, p0 + r, L, &s);
		const uint32_t mrow32 = depth + 4u, tc = (WM_TILE - 16u) / mrow32;      // whole columns a tile, at least 31
		for(uint32_t col_lo = 0; col_lo < mlen; col_lo += tc){
			const uint32_t col_hi = (mlen - col_lo < tc ? mlen : col_lo + tc) - 1u, nb = (col_hi - col_lo + 1u) * mrow32;
			uint8_t *gp = dst + (uint64_t)col_lo * mrow;              // the tile's first byte in the arena; sh: where it lies in its 16-byte line
			const uint32_t sh = (uint32_t)((uintptr_t)gp & 15u), tb = sh + nb;
			// defaults, 16 bytes a thread (the sh bytes in front are not the tile's and are not stored)
			for(uint32_t k = tid * 16u; k < tb; k += 4096u){
				const uint32_t skip = k < sh ? sh - k : 0u;
				uint32_t row = k < sh ? 0u : (k - sh) % mrow32;
				uint32_t q[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
				for(uint32_t b = 0; b < 16u; b++){
					uint32_t val = 0u;
					if(b >= skip){ val = wm_default(row, depth); if(++row == mrow32) row = 0u; }
					q[b >> 2] |= val << (8u * (b & 3u));
				}
				*(uint4*)(tile + k) = make_uint4(q[0], q[1], q[2], q[3]);
			}
			__syncthreads();
			for(uint32_t j = tid; j < L; j += 256u){
				const uint32_t cj = c[j];
				if(cj >= col_lo && cj <= col_hi) tile[sh + (cj - col_lo) * mrow32 + depth] = (uint8_t)wm_draft_base(in, g, j);
			}
			if(walk) wm_advance<false>(s, in.pcig, c, tile + sh, mrow, r, col_lo, col_hi);
			__syncthreads();
			// out: whole 16-byte lines with one store, the bytes of a line shared with a neighbour one by one
			for(uint32_t k = tid * 16u; k < tb; k += 4096u){
				if(k >= sh && k + 16u <= tb) *(uint4*)(gp - sh + k) = *(const uint4*)(tile + k);
				else for(uint32_t b = 0; b < 16u; b++){ if(k + b >= sh && k + b < tb) (gp - sh)[k + b] = tile[k + b]; }
			}
			__syncthreads();
		}
	}
}

// bytes = the sum over the windows of mlen_g (depth_g + 4), mlen_g = L_g + the sum of ins_g.  L_g <= window.  ins_g[j] is a maximum over the window's live
// pieces and so at most the sum of their I units in front of column j; of the pieces of ONE chain no two of a pair share a column, so every I unit of a
// pair's words lies in at most one piece, and the insertion columns of all windows together are at most ins_units, the I units of all the words.  Each of
// them costs at most max depth + 4 bytes.
extern "C" uint64_t bsa_window_msa_bound(const uint64_t *piece_off, size_t nwin, uint32_t window, uint64_t ins_units){
	if(!piece_off || !nwin) return 0;
	unsigned __int128 s = 0; uint64_t dmax = 0;
	for(size_t g = 0; g < nwin; g++){
		const uint64_t d = piece_off[g + 1] >= piece_off[g] ? piece_off[g + 1] - piece_off[g] : 0ull;
		if(d > dmax) dmax = d;
		s += (unsigned __int128)window * ((unsigned __int128)d + 4u);
	}
	s += (unsigned __int128)ins_units * ((unsigned __int128)dmax + 4u);
	return s > (unsigned __int128)~0ull ? ~0ull : (uint64_t)s;
}

// the pass's part of the context's scratch
struct wm_scratch_t { uint8_t *live; uint32_t *depth, *mlen; uint64_t *bytes, *out_off, *tmp; uint32_t *cline; };
static int wm_scratch(bsa_ctx_t *ctx, size_t nwin, size_t piece_cap, uint32_t window, wm_scratch_t *s){
	const size_t o_live = 0, o_depth = o_live + bsa_up256(piece_cap), o_mlen = o_depth + bsa_up256(nwin * 4u), o_bytes = o_mlen + bsa_up256(nwin * 4u),
		o_out = o_bytes + bsa_up256(nwin * 8u), o_tmp = o_out + bsa_up256((nwin + 1u) * 8u), o_line = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)nwin)),
		total = o_line + bsa_up256(nwin * (size_t)window * 4u);
	void *bufv = nullptr;
	const int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);      // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	s->live = b + o_live; s->depth = (uint32_t*)(b + o_depth); s->mlen = (uint32_t*)(b + o_mlen); s->bytes = (uint64_t*)(b + o_bytes);
	s->out_off = (uint64_t*)(b + o_out); s->tmp = (uint64_t*)(b + o_tmp); s->cline = (uint32_t*)(b + o_line);
	return BSA_OK;
}

enum { WM_COLS = 1, WM_SCAN = 2, WM_RECORDS = 4, WM_FILL = 8 };
// the steps of `steps`, in order (one alone only for tools/bench_window_msa.py, on the scratch a whole run left)
static int wm_launch(bsa_ctx_t *ctx, hipStream_t st, const wm_in_t &a, const wm_scratch_t &s, int steps, uint8_t *d_cols, size_t cols_cap, uint64_t *d_cols_off, bsa_cns_window_t *d_cwin){
	hipError_t e = hipSuccess;
	const size_t line = (((size_t)a.window * 4u) + 15u) & ~(size_t)15u, cus = (size_t)bsa_cus();
	if((steps & WM_COLS) && a.nwin){
		const size_t most = cus * 32u;
		hipLaunchKernelGGL(k_window_msa_cols, dim3((uint32_t)(a.nwin < most ? a.nwin : most)), dim3(64), line, st, a, s.live, s.cline, s.depth, s.mlen, s.bytes);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & WM_SCAN)){
		e = bsa_launch_excl_scan(st, (const uint64_t*)s.bytes, d_cols_off, a.nwin, nullptr, s.tmp);
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)s.mlen, s.out_off, a.nwin, nullptr, s.tmp);
	}
	if(e == hipSuccess && (steps & WM_RECORDS) && a.nwin){
		hipLaunchKernelGGL(k_window_msa_records, dim3((uint32_t)(((uint64_t)a.nwin + 255u) / 256u)), dim3(256), 0, st, a.nwin, a.vote, (const uint32_t*)s.depth, (const uint32_t*)s.mlen,
			(const uint64_t*)d_cols_off, (const uint64_t*)s.out_off, d_cwin);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & WM_FILL) && a.nwin && cols_cap){
		const size_t most = cus * 16u;
		hipLaunchKernelGGL(k_window_msa_fill, dim3((uint32_t)(a.nwin < most ? a.nwin : most)), dim3(256), WM_TILE + line, st, a, (const uint8_t*)s.live, (const uint32_t*)s.cline,
			(const uint32_t*)s.mlen, (const uint64_t*)d_cols_off, d_cols, (uint64_t)cols_cap);
		e = hipGetLastError();
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_msa: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

// the argument errors of both calls
static int wm_check(bsa_ctx_t *ctx, const void *piece, const void *piece_off, size_t nwin, size_t piece_cap, const void *bases, size_t bases_cap, const void *pcig, size_t pcig_cap,
		const void *pcig_off, const void *draft, const void *doff, const void *dlen, uint32_t window, uint32_t flags, uint32_t vote, const void *cols, size_t cols_cap,
		const void *cols_off, const void *cwin){
	const char *msg = nullptr;
	if(!piece_off || !pcig_off || !cols_off || (nwin && (!doff || !dlen || !cwin || !draft)) || (piece_cap && !piece) || (bases_cap && !bases) || (pcig_cap && !pcig) || (cols_cap && !cols))
		msg = "bsa_window_msa: null argument";
	else if(window == 0u) msg = "bsa_window_msa: window must be positive";
	else if(flags & ~(uint32_t)BSA_MODE_SEQ2BIT) msg = "bsa_window_msa: flags may hold BSA_MODE_SEQ2BIT only";
	else if(vote > 1u) msg = "bsa_window_msa: vote is 0 or 1";
	else if(nwin > 0xFFFFFFF0ull) msg = "too many windows";
	else if(piece_cap > 0xFFFFFFF0ull) msg = "too many pieces";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	if(window > WM_MAX_WINDOW){ bsa_ctx_set_error_internal(ctx, "bsa_window_msa: windows above 4096 bases are not supported"); return BSA_E_UNSUPPORTED; }
	return BSA_OK;
}

static int wm_run(bsa_ctx_t *ctx, int steps, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const uint8_t *d_bases, size_t bases_cap,
		const uint32_t *d_pcig, size_t pcig_cap, const uint64_t *d_pcig_off, const uint8_t *d_draft, const uint64_t *d_doff, const uint32_t *d_dlen,
		uint32_t window, uint32_t flags, uint32_t vote, uint8_t *d_cols, size_t cols_cap, uint64_t *d_cols_off, bsa_cns_window_t *d_cwin){
	if(!ctx) return BSA_E_ARG;
	int rc = wm_check(ctx, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcig_off, d_draft, d_doff, d_dlen, window, flags, vote, d_cols, cols_cap, d_cols_off, d_cwin);
	if(rc != BSA_OK) return rc;
	if((flags & BSA_MODE_SEQ2BIT) && ((uintptr_t)d_draft & 7u)){ bsa_ctx_set_error_internal(ctx, "bsa_window_msa_run: BSA_MODE_SEQ2BIT needs an 8-byte aligned d_draft"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	wm_scratch_t s;
	if((rc = wm_scratch(ctx, nwin, piece_cap, window, &s)) != BSA_OK) return rc;
	const wm_in_t a = { d_piece, d_piece_off, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcig_off, d_draft, d_doff, d_dlen, (uint32_t)nwin, window, (flags & BSA_MODE_SEQ2BIT) ? 1u : 0u, vote };
	return wm_launch(ctx, stream, a, s, steps, d_cols, cols_cap, d_cols_off, d_cwin);
}

extern "C" int bsa_window_msa_run(bsa_ctx_t *ctx, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const uint8_t *d_bases, size_t bases_cap,
		const uint32_t *d_pcig, size_t pcig_cap, const uint64_t *d_pcig_off, const uint8_t *d_draft, const uint64_t *d_doff, const uint32_t *d_dlen,
		uint32_t window, uint32_t flags, uint32_t vote, uint8_t *d_cols, size_t cols_cap, uint64_t *d_cols_off, bsa_cns_window_t *d_cwin){
	return wm_run(ctx, WM_COLS | WM_SCAN | WM_RECORDS | WM_FILL, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcig_off, d_draft, d_doff, d_dlen,
		window, flags, vote, d_cols, cols_cap, d_cols_off, d_cwin);
}

// for tools/bench_window_msa.py: one step alone (step: 0 cols, 1 scan, 2 records, 3 fill), once more, with the arguments of the context's last
// bsa_window_msa_run and on the scratch it left: nothing else may have used the context in between
extern "C" int bsa_window_msa_step_internal(bsa_ctx_t *ctx, int step, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const uint8_t *d_bases,
		size_t bases_cap, const uint32_t *d_pcig, size_t pcig_cap, const uint64_t *d_pcig_off, const uint8_t *d_draft, const uint64_t *d_doff, const uint32_t *d_dlen,
		uint32_t window, uint32_t flags, uint32_t vote, uint8_t *d_cols, size_t cols_cap, uint64_t *d_cols_off, bsa_cns_window_t *d_cwin){
	if(step < 0 || step > 3) return BSA_E_ARG;
	return wm_run(ctx, 1 << step, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, d_pcig, pcig_cap, d_pcig_off, d_draft, d_doff, d_dlen, window, flags, vote,
		d_cols, cols_cap, d_cols_off, d_cwin);
}

extern "C" int bsa_window_msa_batch(bsa_ctx_t *ctx, const bsa_piece_t *piece, const uint64_t *piece_off, size_t nwin, size_t piece_cap, const uint8_t *bases, size_t bases_cap,
		const uint32_t *pcig, size_t pcig_cap, const uint64_t *pcig_off, const uint8_t *draft, const uint64_t *doff, const uint32_t *dlen,
		uint32_t window, uint32_t flags, uint32_t vote, uint8_t *cols, size_t cols_cap, uint64_t *cols_off, bsa_cns_window_t *cwin){
	if(!ctx) return BSA_E_ARG;
	int rc = wm_check(ctx, piece, piece_off, nwin, piece_cap, bases, bases_cap, pcig, pcig_cap, pcig_off, draft, doff, dlen, window, flags, vote, cols, cols_cap, cols_off, cwin);
	if(rc != BSA_OK) return rc;
	if(nwin == 0){ cols_off[0] = 0; return BSA_OK; }
	// the draft goes up as far as the windows speak of it: bases (1 B/base) or whole words (packed)
	const bool pk = (flags & BSA_MODE_SEQ2BIT) != 0;
	uint64_t dend = 0;
	for(size_t g = 0; g < nwin; g++){
		const uint64_t L = dlen[g] < window ? dlen[g] : window;
		if(L == 0u) continue;
		if(doff[g] > ~0ull - L){ bsa_ctx_set_error_internal(ctx, "bsa_window_msa_batch: a draft slice wraps"); return BSA_E_ARG; }
		if(doff[g] + L > dend) dend = doff[g] + L;
	}
	const size_t dbytes = pk ? (size_t)((dend + 31u) / 32u) * 8u : (size_t)dend;
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	bsa_stage_t in(ctx, stream), res(ctx, stream);
	const size_t o_piece = in.part(piece_cap * sizeof(bsa_piece_t)), o_poff = in.part((nwin + 1u) * 8u), o_bases = in.part(bases_cap), o_pcig = in.part(pcig_cap * 4u),
		o_pcoff = in.part((piece_cap + 1u) * 8u), o_draft = in.part(dbytes + 8u), o_doff = in.part(nwin * 8u), o_dlen = in.part(nwin * 4u),
		o_coff = in.part((nwin + 1u) * 8u), o_cwin = in.part(nwin * sizeof(bsa_cns_window_t));
	if((rc = in.alloc("bsa_window_msa_batch: no device memory for the pieces, codes, guides and the draft")) != BSA_OK) return rc;
	if(!in.up(o_piece, piece, piece_cap * sizeof(bsa_piece_t)) || !in.up(o_poff, piece_off, (nwin + 1u) * 8u) || !in.up(o_bases, bases, bases_cap) || !in.up(o_pcig, pcig, pcig_cap * 4u)
			|| !in.up(o_pcoff, pcig_off, (piece_cap + 1u) * 8u) || !in.up(o_draft, draft, dbytes) || !in.up(o_doff, doff, nwin * 8u) || !in.up(o_dlen, dlen, nwin * 4u))
		return in.fail("bsa_window_msa_batch: upload failed");
	const wm_in_t a = { in.at<bsa_piece_t>(o_piece), in.at<uint64_t>(o_poff), piece_cap, in.at<uint8_t>(o_bases), bases_cap, in.at<uint32_t>(o_pcig), pcig_cap, in.at<uint64_t>(o_pcoff),
		in.at<uint8_t>(o_draft), in.at<uint64_t>(o_doff), in.at<uint32_t>(o_dlen), (uint32_t)nwin, window, pk ? 1u : 0u, vote };
	uint64_t *d_coff = in.at<uint64_t>(o_coff);
	wm_scratch_t s;
	if((rc = wm_scratch(ctx, nwin, piece_cap, window, &s)) != BSA_OK) return rc;
	if((rc = wm_launch(ctx, stream, a, s, WM_COLS | WM_SCAN | WM_RECORDS, nullptr, 0, d_coff, in.at<bsa_cns_window_t>(o_cwin))) != BSA_OK) return rc;
	if(!in.down(cols_off, o_coff, (nwin + 1u) * 8u) || !in.down(cwin, o_cwin, nwin * sizeof(bsa_cns_window_t)) || !in.sync()) return in.fail("bsa_window_msa_batch: download of the offsets failed");
	const uint64_t need = cols_off[nwin];                      // (the offsets and records are down before the capacity is judged)
	if(need > cols_cap) return in.fail("bsa_window_msa_batch: cols_cap too small, cols_off[nwin] holds the bytes needed", BSA_E_CIGAR_CAP);
	if(need == 0) return BSA_OK;
	const size_t o_cols = res.part(need);
	if((rc = res.alloc("bsa_window_msa_batch: no device memory for the columns")) != BSA_OK) return rc;
	if((rc = wm_launch(ctx, stream, a, s, WM_FILL, res.at<uint8_t>(o_cols), need, d_coff, nullptr)) != BSA_OK) return rc;
	if(!res.down(cols, o_cols, need) || !res.sync()) return res.fail("bsa_window_msa_batch: download of the columns failed");
	return BSA_OK;
}
