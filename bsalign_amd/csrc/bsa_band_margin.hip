// bsa_band_margin.hip -- BSA_MODE_BAND_MARGIN (include/bsalign_hip.h): how close every alignment came to the edge of its band.
//
// A pass over what the forward and traceback kernels leave in a pair's slot, not part of any walker: without the flag the kernel is
// not launched.  Every slot family whose band can move -- compact one- and two-piece codes, row records, the run-time-width kernel,
// the int32 kernel, the lane-exact packed kernel and its row-segment form -- starts with int32 begs[tlen + 2], begs[r + 1] = band offset
// of target row r (bsa_common.h), which no walker writes; the walkers leave the CIGAR words at the slot's tail.  A whole-query band
// (B >= qlen: the widened register kernels, the systolic kernel, static bands of any kernel) is answered without touching the slot.
//
// One wave a pair.  The definition walks vertices; this walks TARGET ROWS: on vertex row i the path holds the query positions
// enter_i .. leave_i, an interval, so the row's nearest cell to the low edge is enter_i and to the high edge leave_i.  The path takes
// T = (target bases its words consume) steps from row to row; step s, inside word k at offset d = s - (target bases in front of k),
// gives  enter of row tb + s  =  qs_k + d (M) or qs_k (D)  and  leave of row tb + s - 1  =  qs_k + d - 1 (M) or qs_k (D),  qs_k the query
// position at which word k starts.  Words are taken in tiles of 64, a lane a word, with wave prefix sums of the bases they consume
// (bsa_pass.h: bsa_wave_iscan and the rules of a CIGAR word, as in bsa_cigar_eqx.hip); the steps of a tile are then taken 64 at a time, a lane a step: a binary search over the tile's
// inclusive target sums (six lane-indexed shuffles) finds the step's word -- two identical 10 kbp reads are ONE word and 157 such
// trips, never one lane's loop -- and the lane reads begs[i] and begs[i - 1], coalesced over the wave.  The start vertex's row and
// the last row's leave are added once a pair.  O(tlen + words) a pair; 4 bytes a row and the words are read once.
//
// No LDS allocation, no scratch; plain C++ with vector loads and stores only.
#include "bsa_pass.h"

static __device__ __forceinline__ bool bm_is_ins(uint32_t w){ return (w & 15u) == BSA_CIGAR_I && (w >> 4) != 0u; }

#define BM_NOTHING 0x7FFFFFFF

// the margin of one pair (the same value in every lane).  begs: the slot's front, tl + 2 entries of which [0, tl] are read; src: the
// pair's c plain (or = / X) words; B < ql.
static __device__ __forceinline__ uint32_t bm_pair(const int *begs, const uint32_t *src, uint32_t c, uint32_t ql, uint32_t tl, uint32_t B,
		uint32_t qb, uint32_t tb, uint32_t lane){
	const int hi_lim = (int)(ql - B);          // the high edge of a row counts where b + B < qlen: b < hi_lim
	int best = BM_NOTHING;
	uint32_t tp = 0, qp = qb;                  // target steps taken / query position in front of the tile
	for(uint32_t w0 = 0; w0 < c; w0 += 64u){
		const uint32_t idx = w0 + lane;
		const uint32_t w = idx < c ? src[idx] : 0u, nx = idx + 1u < c ? src[idx + 1u] : 0u;
		const uint32_t op = w & 15u, len = w >> 4;
		const uint32_t qa = bsa_cig_qadd(op, len), ta = bsa_cig_tadd(op, len);
		const uint32_t qi = bsa_wave_iscan(qa, lane), ti = bsa_wave_iscan(ta, lane);
		const uint32_t qs = qp + qi - qa, te = ti - ta;                                     // the word's query position / the tile's target steps in front of it
		const uint32_t tile_t = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(ti, 63));
		for(uint32_t s0 = 0; s0 < tile_t; s0 += 64u){
			const uint32_t sl = s0 + lane + 1u;                                             // this lane's step, counted inside the tile from 1
			uint32_t k = 0;                                                                 // first word whose inclusive sum reaches it (words that take no step have their predecessor's sum)
#pragma unroll
			for(uint32_t st = 32u; st; st >>= 1){ const uint32_t v = __shfl(ti, (int)(k + st - 1u)); if(v < sl) k += st; }
			const uint32_t kw = __shfl(w, (int)k), kq = __shfl(qs, (int)k), kt = __shfl(te, (int)k), kn = __shfl(nx, (int)k);
			const uint32_t i = tb + tp + sl;                                                // vertex row the step enters
			if(sl <= tile_t && i <= tl){
				const uint32_t d = sl - kt, klen = kw >> 4;
				const bool dg = bsa_cig_diag(kw & 15u);
				const uint32_t enter = dg ? kq + d : kq, leave = dg ? kq + d - 1u : kq;
				const int bi = begs[i], bp = begs[i - 1u];
				if(bi > 0){
					if(enter >= 1u) best = min(best, (int)(enter - 1u) - bi);
					else if(d == klen && bm_is_ins(kn)) best = min(best, -bi);              // (the row is entered at j = 0 and an insertion follows: its first counted cell is column 0)
				}
				if(i >= 2u && leave >= 1u && bp < hi_lim) best = min(best, bp + (int)B - (int)leave);
			}
		}
		tp += tile_t; qp += (uint32_t)__shfl(qi, 63);
	}
	// the start vertex's row (its low side) and the last row (its high side)
	if(tb >= 1u && tb <= tl){
		const int b = begs[tb];
		if(b > 0){
			if(qb >= 1u) best = min(best, (int)(qb - 1u) - b);
			else if(bm_is_ins(src[0])) best = min(best, -b);
		}
	}
	const uint32_t il = tb + tp;
	if(il >= 1u && il <= tl && qp >= 1u){
		const int b = begs[il];
		if(b < hi_lim) best = min(best, b + (int)B - (int)qp);
	}
#pragma unroll
	for(int d = 32; d >= 1; d >>= 1) best = min(best, __shfl_xor(best, d));
	return best == BM_NOTHING ? (uint32_t)BSA_ST_MARGIN_NONE : (uint32_t)min(max(best, 0), 0xFFFE);
}

// after a chunk's traceback, before anything rewrites cnt[] (BSA_MODE_CIGAR_EQX) or the slots: status[pair] |= margin << 16
__global__ void __launch_bounds__(256) k_band_margin(const uint8_t *rows, const uint64_t *slot_off, const uint64_t *slot_end, uint32_t first, uint32_t count,
		const uint32_t *cnt, const uint32_t *order, const uint32_t *qlen, const uint32_t *tlen, const bsa_result_t *out, uint32_t bandwidth, uint32_t *status){
	const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if(g >= count) return;
	const uint32_t ppos = first + g, pair = order[ppos];
	const uint32_t c = cnt[ppos], ql = qlen[pair], tl = tlen[pair];
	const uint64_t B64 = ((uint64_t)(bandwidth ? bandwidth : ql) + 15u) & ~(uint64_t)15;      // the reference's width (bsalign.h:3861-3862)
	uint32_t m = BSA_ST_MARGIN_NONE;
	const uint64_t so = slot_off[ppos], se = slot_end[ppos];
	// a moving band, a CIGAR, and words and band offsets that lie inside the pair's own slot
	if(B64 < ql && c != 0u && se >= so && bsa_begs_bytes(tl) + (uint64_t)c * 4u <= se - so){
		const int32_t qb = out[pair].qb, tb = out[pair].tb;
		if(qb >= 0 && tb >= 0) m = bm_pair((const int*)(rows + so), (const uint32_t*)(rows + se) - c, c, ql, tl, (uint32_t)B64, (uint32_t)qb, (uint32_t)tb, lane);
	}
	if(lane == 0) status[pair] = (status[pair] & 0xFFFFu) | (m << BSA_ST_MARGIN_SHIFT);
}

hipError_t bsa_launch_band_margin(const uint8_t *rows, const uint64_t *slot_off, const uint64_t *slot_end, uint32_t first, uint32_t count, const uint32_t *cnt,
		const uint32_t *order, const uint32_t *qlen, const uint32_t *tlen, const bsa_result_t *out, uint32_t bandwidth, uint32_t *status, hipStream_t st){
	if(count == 0) return hipSuccess;
	hipLaunchKernelGGL(k_band_margin, dim3((count + 3) / 4), dim3(256), 0, st, rows, slot_off, slot_end, first, count, cnt, order, qlen, tlen, out, bandwidth, status);
	return hipGetLastError();
}
