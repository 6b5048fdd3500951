// bsa_piece_cigars.hip -- bsa_piece_cigars_run / _batch (include/bsalign_hip.h): for every read piece that bsa_window_pieces_run left, the stretch of
// its pair's CIGAR between the piece's first and last aligned column, as words of its own -- the guide a windowed polisher's POA places the piece by.
//
// A pass over public outputs: the records, words and offsets of an align / edit run and the piece records.  It knows no plan, no window size and no
// window record: only the alignment and the piece's own coordinates.  Four steps on the context stream:
//   index : one wave a pair (k_piece_cigars_index) walks the pair's words in tiles of 64, a lane a word, and leaves the position (t: 64 bit, q: 32
//           bit) in front of every `stride`-th tile in the context's scratch: PCG_SAMPLES places of 16 bytes a pair, stride = ceil(tiles /
//           PCG_SAMPLES), so a pair of up to 64 * PCG_SAMPLES words has a place for every tile.  (The places are a fixed number a pair and not one
//           for every 64 words of the arena because the host never learns how many words the arena holds: d_cigar_off is device memory.)
//   count : 16 lanes a piece, four pieces a wave (k_piece_cigars_count).  The lanes read the pair's places, two each; a ballot finds the last one whose t
//           is not above t_first.  From that tile the group walks on, 16 words a step with prefix sums over its DPP row, until a diagonal word holds
//           t_first, tests q there, goes on to the word that holds t_last counting the words kept with a ballot and a popcount a step, and tests q
//           again.  It leaves the count, the first and the last word, the two in-word offsets and where the pair's words are (32 bytes) and the
//           status.  Groups at or above P = min(*d_npiece, piece_cap) leave a count of 0, so that
//   scan  : the 64-bit exclusive scan of bsa_scan.hip over all piece_cap counts writes every offset, those above P included;
//   fill  : 16 lanes a piece whose range ends inside the arena (k_piece_cigars_fill) copy from the first word to the last, clip both, and compact
//           dropped words away with a ballot prefix.
// A piece of a polisher's window is a few hundred bytes of work, and whoever does it mostly waits for loads.  So count and fill put four pieces into
// a wave, stride over the pieces with a grid of 16 blocks a CU, and issue together the loads that do not depend on each other (measured against a
// wave a piece).
// What a piece costs: one load of at most PCG_SAMPLES places, at most `stride` tiles in front of its first word, and the words from the tile its
// first word lies in to its last word, twice (count and fill).  Where the piece lies inside its pair does not matter while stride is 1.
// Target positions are summed in 64 bits, query positions wrap in 32.  No LDS, no atomics; plain C++ with vector loads and stores, DPP row moves
// (bsa_dpp.h) and wave intrinsics only.
#include "bsa_pass.h"
#include "bsa_dpp.h"
#include <vector>

#define PCG_SAMPLES 32u            // index places a pair (32: a lane of a group of 16 reads two)
#ifndef PCG_INDEX_TILES
#define PCG_INDEX_TILES 4u         // tiles the index kernel loads together
#endif
#define PCG_MAX_WORDS 0xFFFFFFFFull  // a pair of more words is cut nowhere: word indices and counts are 32 bit

// a cut piece: its first word (index in the pair), the units in front of its first column in that word, the units in front of its last column in its
// last word, its words (cnt == 0: not cut); the pair's first word in the arena, its words and the piece's last word, so that the fill needs neither
// piece nor pair and loads nothing behind the piece
struct pcg_info_t { uint32_t x, a, b, cnt; uint64_t c0; uint32_t c, y; };
static_assert(sizeof(pcg_info_t) == 32 && sizeof(bsa_piece_t) == 32, "32 bytes of scratch a piece; bsa_piece_t is 32 bytes");

// Sums without the LDS crossbar: prefix sums inside a DPP row of 16 lanes with four DPP moves (row_iscan16 of bsa_dpp.h, all lanes of the row active);
// a row's total is its lane 15.  A word's length is below 2^28, so 64 of them sum to less than 2^34: where target lengths are summed, the low 20 and
// the high 8 bits are summed apart, each in 32 bits.
static __device__ __forceinline__ uint32_t pcg_lane(uint32_t v, int l){ return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
static __device__ __forceinline__ uint32_t pcg_sum(uint32_t v){                            // the sum over the wave, modulo 2^32, in scalar registers (all 64 lanes active)
	const uint32_t x = (uint32_t)row_iscan16((int)v);
	return pcg_lane(x, 15) + pcg_lane(x, 31) + pcg_lane(x, 47) + pcg_lane(x, 63);
}
static __device__ __forceinline__ uint64_t pcg_sum_len(uint32_t v){ return (uint64_t)pcg_sum(v & 0xFFFFFu) + ((uint64_t)pcg_sum(v >> 20) << 20); }

// the words of pair k, 0 where it has no alignment to cut: tb < 0, no words, offsets that decrease, too many words
static __device__ __forceinline__ uint64_t pcg_words(const bsa_result_t *out, const uint64_t *coff, uint32_t k){
	const uint64_t c0 = coff[k], c1 = coff[k + 1u];
	if(out[k].tb < 0 || c1 <= c0 || c1 - c0 > PCG_MAX_WORDS) return 0ull;
	return c1 - c0;
}
static __device__ __forceinline__ uint32_t pcg_stride(uint32_t tiles){ return (tiles + PCG_SAMPLES - 1u) / PCG_SAMPLES; }

// one wave a pair: idx[k * PCG_SAMPLES + s] = (t low, t high, q, 0) in front of tile s * stride.  PCG_INDEX_TILES tiles a trip: their loads do not
// depend on each other, and a wave that walks a pair alone has nothing else to hide a load behind.
__global__ void __launch_bounds__(256) k_piece_cigars_index(const bsa_result_t *out, const uint32_t *cigar, const uint64_t *coff, uint32_t n, uint4 *idx){
	const uint32_t k = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
	if(k >= n) return;
	const uint64_t c = pcg_words(out, coff, k);
	if(c == 0u) return;
	const uint32_t tiles = (uint32_t)((c + 63u) >> 6), stride = pcg_stride(tiles);
	const uint32_t *src = cigar + coff[k];
	uint4 *dst = idx + (size_t)k * PCG_SAMPLES;
	uint64_t tp = (uint32_t)out[k].tb; uint32_t qp = (uint32_t)out[k].qb;
	uint32_t next = 0, s = 0;                              // the next tile that has a place, and the place
	for(uint32_t t0 = 0; t0 < tiles; t0 += PCG_INDEX_TILES){
		uint32_t word[PCG_INDEX_TILES];
#pragma unroll
		for(int u = 0; u < (int)PCG_INDEX_TILES; u++){
			const uint64_t i = (uint64_t)(t0 + u) * 64u + lane;
			word[u] = i < c ? src[i] : 0u;
		}
#pragma unroll
		for(int u = 0; u < (int)PCG_INDEX_TILES; u++){
			if(t0 + u == next && next < tiles){
				if(lane == 0u && s < PCG_SAMPLES) dst[s] = make_uint4((uint32_t)tp, (uint32_t)(tp >> 32), qp, 0u);
				next += stride; s++;
			}
			const uint32_t op = word[u] & 15u, len = word[u] >> 4;
			qp += pcg_sum(bsa_cig_qadd(op, len));
			tp += pcg_sum_len(bsa_cig_tadd(op, len));
		}
	}
}

// 16 lanes a piece, four pieces a wave, a grid of at most 16 blocks a CU striding over the pieces (see the fill).  A group is a DPP row, so the prefix
// sums of its 16 words are four DPP moves and a row broadcast gives their total; a ballot's 16 bits of the group stand for the wave's.  What does
// not depend on each other is loaded together: the record, the offsets and the pair's places (two a lane; all PCG_SAMPLES of them are the pair's own
// scratch whether written or not, and only the first ns are looked at), then 64 words of the walk, four a lane.  Everything a group decides on is
// the same in its 16 lanes; groups leave the loops at different times (a ballot then has no bits for the lanes that left).
static __device__ __forceinline__ uint32_t pcg_grp(uint64_t ballot, uint32_t sh){ return (uint32_t)(ballot >> sh) & 0xFFFFu; }
static __device__ __forceinline__ uint32_t pcg_row_total(uint32_t x){ return (uint32_t)DPP_BCAST((int)x, 15); }      // lane 15 of the row, in every lane of it
__global__ void __launch_bounds__(256) k_piece_cigars_count(const bsa_result_t *out, const uint32_t *cigar, const uint64_t *coff, uint32_t n,
		const bsa_piece_t *piece, const uint64_t *npiece, uint32_t piece_cap, const uint4 *idx, uint32_t *cnt, pcg_info_t *info, uint32_t *pstatus){
	const uint32_t gl = threadIdx.x & 15u, sh = threadIdx.x & 48u;          // the lane in its group, the group's first lane in the wave
	const uint64_t np = *npiece, ngrp = (uint64_t)gridDim.x * 16u;
	for(uint64_t j = blockIdx.x * 16u + (threadIdx.x >> 4); j < piece_cap; j += ngrp){
		if(j >= np){ if(gl == 0u) cnt[j] = 0u; continue; }
		const bsa_piece_t pc = piece[j];
		const uint32_t k = pc.pair;
		const uint64_t tf = pc.t_first, tl = pc.t_last;
		const uint32_t qf = pc.q_first, ql = pc.q_first + pc.len - 1u;      // (modulo 2^32, as the columns' q)
		pcg_info_t r = { 0u, 0u, 0u, 0u, 0ull, 0u, 0u };
		uint64_t c = 0, c0 = 0;
		uint4 s0 = make_uint4(0u, 0u, 0u, 0u), s1 = s0;
		if(k < n){
			c0 = coff[k];
			const uint64_t c1 = coff[k + 1u];
			const int32_t tb = out[k].tb;
			s0 = idx[(size_t)k * PCG_SAMPLES + gl]; s1 = idx[(size_t)k * PCG_SAMPLES + 16u + gl];
			if(tb >= 0 && c1 > c0 && c1 - c0 <= PCG_MAX_WORDS && tf <= tl && pc.len != 0u) c = c1 - c0;
		}
		if(c != 0u){
			const uint32_t tiles = (uint32_t)((c + 63u) >> 6), stride = pcg_stride(tiles), ns = (tiles + stride - 1u) / stride;
			const uint32_t *src = cigar + c0;
			const uint64_t st0 = ((uint64_t)s0.y << 32) | s0.x, st1 = ((uint64_t)s1.y << 32) | s1.x;
			const uint32_t at0 = pcg_grp(__ballot(gl < ns && st0 <= tf), sh), at1 = pcg_grp(__ballot(16u + gl < ns && st1 <= tf), sh);      // (t never decreases: a prefix)
			if((at0 | at1) != 0u){
				const uint32_t sl = at1 ? 47u - (uint32_t)__clz((int)at1) : 31u - (uint32_t)__clz((int)at0);      // the last place not above t_first
				const int from = (int)(sh + (sl & 15u));
				uint64_t tp = __shfl(sl >= 16u ? st1 : st0, from); uint32_t qp = __shfl(sl >= 16u ? s1.z : s0.z, from);      // the positions in front of the tile
				bool havex = false, stop = false; uint32_t x = 0, a = 0, kept = 0;
				for(uint64_t w0 = (uint64_t)sl * stride * 64u; w0 < c && !stop; w0 += 64u){
					uint32_t word[4];
#pragma unroll
					for(int u = 0; u < 4; u++){ const uint64_t i = w0 + 16u * u + gl; word[u] = i < c ? src[i] : 0u; }
#pragma unroll
					for(int u = 0; u < 4; u++){
						if(tp > tl){ stop = true; break; }                     // behind the last column
						const uint64_t i = w0 + 16u * u + gl;
						const uint32_t op = word[u] & 15u, len = word[u] >> 4;
						const bool dg = bsa_cig_diag(op);
						const uint32_t qa = bsa_cig_qadd(op, len), ta = bsa_cig_tadd(op, len);
						const uint32_t qi = (uint32_t)row_iscan16((int)qa), tlo = (uint32_t)row_iscan16((int)(ta & 0xFFFFFu)), thi = (uint32_t)row_iscan16((int)(ta >> 20));
						const uint64_t ti = (uint64_t)tlo + ((uint64_t)thi << 20);
						const uint64_t tn = tp + (uint64_t)pcg_row_total(tlo) + ((uint64_t)pcg_row_total(thi) << 20);      // behind the 16 words
						const uint64_t ts = tp + ti - ta;                      // where this lane's word starts
						const uint32_t qs = qp + qi - qa;
						const bool col = dg && len != 0u;
						if(!havex){
							const uint32_t hit = pcg_grp(__ballot(col && ts <= tf && tf - ts < len), sh);      // (at most one lane: diagonal words share no t)
							if(hit != 0u){
								const int lx = __ffs((int)hit) - 1;
								const uint32_t d = (uint32_t)(tf - ts);
								if(__shfl(qs + d, (int)sh + lx) != qf){ stop = true; break; }      // the right t with another q
								havex = true; x = (uint32_t)(w0 + 16u * u) + (uint32_t)lx; a = __shfl(d, (int)sh + lx);
							} else if(tn > tf){ stop = true; break; }          // t_first lies in a deletion
						}
						if(havex){
							const uint32_t hit = pcg_grp(__ballot(col && ts <= tl && tl - ts < len), sh);
							const int ly = hit != 0u ? __ffs((int)hit) - 1 : 15;
							kept += (uint32_t)__popc(pcg_grp(__ballot(bsa_cig_steps(op) && len != 0u && i >= x && gl <= (uint32_t)ly), sh));
							if(hit != 0u){
								const uint32_t d = (uint32_t)(tl - ts);
								if(__shfl(qs + d, (int)sh + ly) == ql){
									r.x = x; r.a = a; r.b = __shfl(d, (int)sh + ly); r.cnt = kept; r.c0 = c0; r.c = (uint32_t)c; r.y = (uint32_t)(w0 + 16u * u) + (uint32_t)ly;
								}
								stop = true; break;
							}
						}
						tp = tn; qp += pcg_row_total(qi);
					}
				}
			}
		}
		if(gl == 0u){
			cnt[j] = r.cnt; info[j] = r;
			if(pstatus) pstatus[j] = r.cnt ? 0u : BSA_PIECE_ST_NOT_ON_PATH;
		}
	}
}

// 16 lanes a piece, four pieces a wave, a grid of at most 16 blocks a CU striding over the pieces (as k_window_pieces_gather): a piece of a polisher's
// window has some tens of words, and four of them in a wave keep four times the loads in flight.  A piece is written whole or not at all: when its
// range ends inside the arena (off[j + 1] <= cap), so with cap == 0 `pcig` is never dereferenced (it may be NULL: a count-only run).  Everything the
// fill needs to know of the pair is in the count kernel's 32 bytes.  64 words a trip, four a lane, loaded together; a ballot's 16 bits of the group
// give every kept word its place.  (Groups leave the loops at different times: a ballot then has no bits for the lanes that left, and a group only
// looks at its own.)
__global__ void __launch_bounds__(256) k_piece_cigars_fill(const uint32_t *cigar, const uint64_t *npiece, uint32_t piece_cap, const pcg_info_t *info, const uint64_t *off,
		uint32_t *pcig, uint64_t cap){
	const uint32_t gl = threadIdx.x & 15u, sh = threadIdx.x & 48u;          // the lane in its group, the group's first lane in the wave
	const uint64_t np = *npiece, P = np < piece_cap ? np : piece_cap, ngrp = (uint64_t)gridDim.x * 16u;
	for(uint64_t j = blockIdx.x * 16u + (threadIdx.x >> 4); j < P; j += ngrp){
		const pcg_info_t r = info[j];
		const uint64_t o0 = off[j], o1 = off[j + 1u];
		if(r.cnt == 0u || o1 > cap || o1 - o0 != (uint64_t)r.cnt) continue;      // (the offsets are this pass's own scan of the same counts)
		const uint32_t *src = cigar + r.c0;
		uint32_t *dst = pcig + o0;
		uint32_t done = 0;
		for(uint64_t w0 = r.x; w0 <= r.y && done < r.cnt; w0 += 64u){
			uint32_t word[4];
#pragma unroll
			for(int u = 0; u < 4; u++){ const uint64_t i = w0 + 16u * u + gl; word[u] = i <= r.y ? src[i] : 0u; }      // (y < c: inside the pair's words)
#pragma unroll
			for(int u = 0; u < 4; u++){
				const uint32_t op = word[u] & 15u, len = word[u] >> 4;
				const bool keep = bsa_cig_steps(op) && len != 0u;
				const uint32_t m = (uint32_t)(__ballot(keep) >> sh) & 0xFFFFu;
				const uint32_t at = done + (uint32_t)__popc(m & ((1u << gl) - 1u));
				if(keep && at < r.cnt){
					uint32_t nl = at == r.cnt - 1u ? r.b + 1u : len;         // the last word ends with the last column
					if(at == 0u) nl -= r.a;                                // the first word starts with the first
					dst[at] = (nl << 4) | op;
				}
				done += (uint32_t)__popc(m);
			}
		}
	}
}

extern "C" uint64_t bsa_piece_cigars_bound(const uint64_t *cigar_off, size_t n, size_t npiece){
	uint64_t s = npiece;
	if(cigar_off && n && cigar_off[n] > cigar_off[0]) s += cigar_off[n] - cigar_off[0];
	return s;
}

// the pass's part of the context's scratch: cnt | the scan's tiles | info | idx
struct pcg_scratch_t { uint32_t *cnt; uint64_t *tmp; pcg_info_t *info; uint4 *idx; };
static int pcg_scratch(bsa_ctx_t *ctx, size_t n, size_t piece_cap, pcg_scratch_t *s){
	const size_t o_cnt = 0, o_tmp = o_cnt + bsa_up256(piece_cap * 4u), o_info = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)piece_cap)),
		o_idx = o_info + bsa_up256(piece_cap * sizeof(pcg_info_t)), total = o_idx + bsa_up256(n * PCG_SAMPLES * sizeof(uint4));
	void *bufv = nullptr;
	const int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);      // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	s->cnt = (uint32_t*)(b + o_cnt); s->tmp = (uint64_t*)(b + o_tmp); s->info = (pcg_info_t*)(b + o_info); s->idx = (uint4*)(b + o_idx);
	return BSA_OK;
}

struct pcg_in_t { const bsa_result_t *out; const uint32_t *cigar; const uint64_t *coff; uint32_t n; const bsa_piece_t *piece; const uint64_t *npiece; uint32_t piece_cap; };

enum { PCG_INDEX = 1, PCG_COUNT = 2, PCG_SCAN = 4, PCG_FILL = 8 };
// the steps of `steps`, in order (one alone only for tools/bench_piece_cigars.py, on the scratch a whole run left)
static int pcg_launch(bsa_ctx_t *ctx, hipStream_t st, const pcg_in_t &a, const pcg_scratch_t &s, int steps, uint32_t *d_pcig, size_t pcig_cap, uint64_t *d_pcig_off, uint32_t *d_pstatus){
	const dim3 block(256), pairs((a.n + 3u) / 4u);
	hipError_t e = hipSuccess;
	if((steps & PCG_INDEX) && a.n && a.piece_cap){
		hipLaunchKernelGGL(k_piece_cigars_index, pairs, block, 0, st, a.out, a.cigar, a.coff, a.n, s.idx);
		e = hipGetLastError();
	}
	const dim3 pieces = bsa_grid16(a.piece_cap);               // count and fill
	if(e == hipSuccess && (steps & PCG_COUNT) && a.piece_cap){
		hipLaunchKernelGGL(k_piece_cigars_count, pieces, block, 0, st, a.out, a.cigar, a.coff, a.n, a.piece, a.npiece, a.piece_cap, (const uint4*)s.idx, s.cnt, s.info, d_pstatus);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & PCG_SCAN)) e = bsa_launch_excl_scan(st, s.cnt, d_pcig_off, a.piece_cap, nullptr, s.tmp);
	if(e == hipSuccess && (steps & PCG_FILL) && a.n && a.piece_cap && pcig_cap){
		hipLaunchKernelGGL(k_piece_cigars_fill, pieces, block, 0, st, a.cigar, a.npiece, a.piece_cap, (const pcg_info_t*)s.info, (const uint64_t*)d_pcig_off, d_pcig, (uint64_t)pcig_cap);
		e = hipGetLastError();
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_piece_cigars: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

// the argument errors of both calls
static int pcg_check(bsa_ctx_t *ctx, const void *out, const void *coff, size_t n, const void *piece, size_t pieces, const void *pcig, size_t pcig_cap, const void *pcig_off){
	const char *msg = nullptr;
	if(!pcig_off || (n && (!out || !coff)) || (pieces && !piece) || (pcig_cap && !pcig)) msg = "bsa_piece_cigars: null argument";
	else if(n > 0xFFFFFFF0ull) msg = "too many pairs";
	else if(pieces > 0xFFFFFFF0ull) msg = "too many pieces";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	return BSA_OK;
}

static int pcg_run(bsa_ctx_t *ctx, int steps, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off, size_t n,
		const bsa_piece_t *d_piece, const uint64_t *d_npiece, size_t piece_cap, uint32_t *d_pcig, size_t pcig_cap, uint64_t *d_pcig_off, uint32_t *d_pstatus){
	if(!ctx) return BSA_E_ARG;
	int rc = pcg_check(ctx, d_out, d_cigar_off, n, d_piece, piece_cap, d_pcig, pcig_cap, d_pcig_off);
	if(rc != BSA_OK) return rc;
	if((n && !d_cigar) || (piece_cap && !d_npiece)){ bsa_ctx_set_error_internal(ctx, "bsa_piece_cigars_run: null argument"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	pcg_scratch_t s;
	if((rc = pcg_scratch(ctx, n, piece_cap, &s)) != BSA_OK) return rc;
	const pcg_in_t a = { d_out, d_cigar, d_cigar_off, (uint32_t)n, d_piece, d_npiece, (uint32_t)piece_cap };
	return pcg_launch(ctx, stream, a, s, steps, d_pcig, pcig_cap, d_pcig_off, d_pstatus);
}

extern "C" int bsa_piece_cigars_run(bsa_ctx_t *ctx, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off, size_t n,
		const bsa_piece_t *d_piece, const uint64_t *d_npiece, size_t piece_cap, uint32_t *d_pcig, size_t pcig_cap, uint64_t *d_pcig_off, uint32_t *d_pstatus){
	return pcg_run(ctx, PCG_INDEX | PCG_COUNT | PCG_SCAN | PCG_FILL, d_out, d_cigar, d_cigar_off, n, d_piece, d_npiece, piece_cap, d_pcig, pcig_cap, d_pcig_off, d_pstatus);
}

// for tools/bench_piece_cigars.py: one step alone (step: 0 index, 1 count, 2 scan, 3 fill), once more, with the arguments of the context's last
// bsa_piece_cigars_run and on the scratch it left: nothing else may have used the context in between
extern "C" int bsa_piece_cigars_step_internal(bsa_ctx_t *ctx, int step, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off, size_t n,
		const bsa_piece_t *d_piece, const uint64_t *d_npiece, size_t piece_cap, uint32_t *d_pcig, size_t pcig_cap, uint64_t *d_pcig_off, uint32_t *d_pstatus){
	if(step < 0 || step > 3) return BSA_E_ARG;
	return pcg_run(ctx, 1 << step, d_out, d_cigar, d_cigar_off, n, d_piece, d_npiece, piece_cap, d_pcig, pcig_cap, d_pcig_off, d_pstatus);
}

extern "C" int bsa_piece_cigars_batch(bsa_ctx_t *ctx, const bsa_result_t *out, const uint32_t *cigar, const uint64_t *cigar_off, size_t n,
		const bsa_piece_t *piece, size_t npiece, uint32_t *pcig, size_t pcig_cap, uint64_t *pcig_off, uint32_t *pstatus){
	if(!ctx) return BSA_E_ARG;
	int rc = pcg_check(ctx, out, cigar_off, n, piece, npiece, pcig, pcig_cap, pcig_off);
	if(rc != BSA_OK) return rc;
	std::vector<uint64_t> coff;
	if((rc = bsa_rebase_offsets(ctx, cigar_off, n, coff, "bsa_piece_cigars_batch: cigar_off decreases")) != BSA_OK) return rc;
	const uint64_t w0 = n ? cigar_off[0] : 0ull, words = coff[n], np64 = npiece;          // only the words the offsets speak of go up
	if(words && !cigar){ bsa_ctx_set_error_internal(ctx, "bsa_piece_cigars_batch: null argument"); return BSA_E_ARG; }
	if(n == 0 || npiece == 0){                                 // no alignment, or nothing to cut
		for(size_t j = 0; j <= npiece; j++) pcig_off[j] = 0;
		if(pstatus) for(size_t j = 0; j < npiece; j++) pstatus[j] = BSA_PIECE_ST_NOT_ON_PATH;
		return BSA_OK;
	}
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	bsa_stage_t in(ctx, stream), res(ctx, stream);
	const size_t o_out = in.part(n * sizeof(bsa_result_t)), o_coff = in.part((n + 1) * 8), o_np = in.part(8), o_poff = in.part((npiece + 1) * 8), o_st = in.part(npiece * 4),
		o_piece = in.part(npiece * sizeof(bsa_piece_t)), o_cig = in.part(words * 4 + 4);
	if((rc = in.alloc("bsa_piece_cigars_batch: no device memory for the records, words and pieces")) != BSA_OK) return rc;
	if(!in.up(o_out, out, n * sizeof(bsa_result_t)) || !in.up(o_coff, coff.data(), (n + 1) * 8) || !in.up(o_np, &np64, 8) || !in.up(o_piece, piece, npiece * sizeof(bsa_piece_t))
			|| !in.up(o_cig, words ? cigar + w0 : nullptr, words * 4)) return in.fail("bsa_piece_cigars_batch: upload failed");
	const pcg_in_t a = { in.at<bsa_result_t>(o_out), in.at<uint32_t>(o_cig), in.at<uint64_t>(o_coff), (uint32_t)n, in.at<bsa_piece_t>(o_piece), in.at<uint64_t>(o_np), (uint32_t)npiece };
	uint64_t *d_poff = in.at<uint64_t>(o_poff);
	pcg_scratch_t s;
	if((rc = pcg_scratch(ctx, n, npiece, &s)) != BSA_OK) return rc;
	if((rc = pcg_launch(ctx, stream, a, s, PCG_INDEX | PCG_COUNT | PCG_SCAN, nullptr, 0, d_poff, in.at<uint32_t>(o_st))) != BSA_OK) return rc;
	if(!in.down(pcig_off, o_poff, (npiece + 1) * 8) || (pstatus && !in.down(pstatus, o_st, npiece * 4)) || !in.sync()) return in.fail("bsa_piece_cigars_batch: download of the offsets failed");
	const uint64_t need = pcig_off[npiece];                    // (the offsets are down before the capacity is judged)
	if(need > pcig_cap) return in.fail("bsa_piece_cigars_batch: pcig_cap too small, pcig_off[npiece] holds the words needed", BSA_E_CIGAR_CAP);
	if(need == 0) return BSA_OK;
	const size_t o_pcig = res.part(need * 4);
	if((rc = res.alloc("bsa_piece_cigars_batch: no device memory for the words")) != BSA_OK) return rc;
	if((rc = pcg_launch(ctx, stream, a, s, PCG_FILL, res.at<uint32_t>(o_pcig), need, d_poff, nullptr)) != BSA_OK) return rc;
	if(!res.down(pcig, o_pcig, need * 4) || !res.sync()) return res.fail("bsa_piece_cigars_batch: download of the words failed");
	return BSA_OK;
}
