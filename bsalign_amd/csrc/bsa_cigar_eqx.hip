// bsa_cigar_eqx.hip -- BSA_MODE_CIGAR_EQX (include/bsalign_hip.h): every M word of a CIGAR split into the maximal runs of = and X.
//
// A pass over the words the traceback kernels left at the tails of their slots, not part of any walker: without the flag none of
// these kernels is launched.  One wave a pair, in tiles of 64 words: lane i takes word i, a wave prefix sum (bsa_pass.h) of the bases the
// words consume (seeded with the record's qb / tb; the input holds M, I and D words only, so the test here is op == M, not the wider bsa_cig_diag) gives it its start positions in the staged 1 B/base copies, and it compares its M
// word's columns eight at a time.  k_cigar_eqx_count counts the expanded words (run_pipeline scans them into offsets); the EQX
// forms of k_cigar_collect and k_cigar_final_direct repeat the walk and write each word's runs at the pair's offset plus an
// exclusive prefix of the per-word counts.  The two walks are one function (eqx_walk<EMIT>), so they cannot disagree; the emitting
// form still checks every index against the pair's counted total before it stores.
//
// No LDS, no scratch; plain C++ with vector loads and stores only.
#include "bsa_pass.h"

// An M word of up to EQX_LANE_COLS columns stays on its lane: its mismatch bits are one 64-bit mask, its runs a popcount.  A longer
// word (two identical 10 kbp sequences are ONE word of 10 000 columns) is taken by the whole wave, EQX_TRIP_COLS columns a trip,
// eight per lane, runs across lanes and trips stitched.
#define EQX_LANE_COLS 64u
#define EQX_TRIP_COLS 512u

// mismatch bits of eight columns: bit j = (q[j] != t[j]).  Two unaligned 8-byte loads; they may reach up to 7 bytes behind a
// sequence's last base, which the staged copies' padding covers (at least 16 bytes: bsa_api.hip qpad / tpad, the edit plan's
// + 16) -- the caller masks the bits behind its word's end.  Staged codes are 0..3, so a byte of the XOR is nonzero iff its
// two low bits are; the four flag bits of a dword are gathered by one multiplication (byte j -> bit 24 + j, no two partial products meet).
static __device__ __forceinline__ uint32_t eqx_mis8(const uint8_t *q, const uint8_t *t){
	uint64_t a, b;
	__builtin_memcpy(&a, q, 8); __builtin_memcpy(&b, t, 8);
	uint64_t x = a ^ b;
	x = (x | (x >> 1)) & 0x0101010101010101ull;
	return (((uint32_t)x * 0x01020408u) >> 24) | ((((uint32_t)(x >> 32) * 0x01020408u) >> 24) << 4);
}

static __device__ __forceinline__ uint32_t eqx_op(uint32_t mis){ return mis & 1u ? (uint32_t)BSA_CIGAR_X : (uint32_t)BSA_CIGAR_EQ; }

// one M word of `len` > EQX_LANE_COLS columns by the whole wave; returns its number of runs (the same in every lane).
// A column s > 0 whose mismatch bit differs from column s - 1 starts a run and closes the one before it: EMIT writes the closed
// run there (run k of the word at dst[o0 + k]; runs alternate, so run k's op is column 0's bit ^ k) and lane 0 the last one.
template<bool EMIT>
static __device__ __forceinline__ uint32_t eqx_long(const uint8_t *q, const uint8_t *t, uint32_t len, uint32_t *dst, uint32_t o0, uint32_t dcap, uint32_t lane){
	uint32_t nst = 0;          // runs closed so far
	uint32_t rs = 0;           // EMIT: start column of the open run
	uint32_t prev = 0, m0 = 0; // mismatch bit of the column in front of this trip / of column 0
	for(uint32_t b = 0; b < len; b += EQX_TRIP_COLS){
		const uint32_t c0 = b + lane * 8u;
		const uint32_t nv = c0 < len ? min(len - c0, 8u) : 0u;
		const uint32_t vm = 0xFFu >> (8u - nv);
		uint32_t bits = 0;
		if(nv) bits = eqx_mis8(q + c0, t + c0) & vm;
		uint32_t pb = __shfl_up(bits, 1) >> 7;
		if(lane == 0) pb = prev;
		if(b == 0){ m0 = __shfl(bits, 0) & 1u; if(lane == 0) pb = bits & 1u; }        // (column 0 starts the first run and closes none)
		uint32_t st = (bits ^ ((bits << 1) | pb)) & vm;
		const uint32_t ns = __popc(st);
		const uint32_t inc = bsa_wave_iscan(ns, lane);
		const uint32_t tot = __shfl(inc, 63);
		if(EMIT){
			// the run a lane's first start closes began at the last start on a lower lane, or at rs (start columns grow with the lane: a running maximum)
			const uint32_t ls = st ? c0 + (31u - (uint32_t)__clz((int)st)) : 0u;
			uint32_t pm = ls;
#pragma unroll
			for(uint32_t d = 1; d < 64u; d <<= 1){ const uint32_t u = __shfl_up(pm, d); if(lane >= d) pm = max(pm, u); }
			uint32_t ps = __shfl_up(pm, 1);
			if(lane == 0) ps = 0;
			ps = max(ps, rs);
			rs = max(rs, (uint32_t)__shfl(pm, 63));
			uint32_t k = nst + inc - ns;
			while(st){
				const uint32_t s = c0 + (uint32_t)__ffs((int)st) - 1u;
				st &= st - 1u;
				if(o0 + k < dcap) dst[o0 + k] = ((s - ps) << 4) | eqx_op(m0 ^ k);
				ps = s; k++;
			}
		}
		nst += tot;
		prev = (uint32_t)__shfl(bits, 63) >> 7;
	}
	if(EMIT && lane == 0 && o0 + nst < dcap) dst[o0 + nst] = ((len - rs) << 4) | eqx_op(m0 ^ nst);
	return nst + 1u;
}

// the walk over a pair's `c` plain words at src: returns the number of expanded words; EMIT writes them to dst[0 .. dcap).
// q / t: the pair's staged sequences, ql / tl their lengths, qp / tp the record's qb / tb.  An M word whose columns would leave
// either sequence (a record and a CIGAR that do not belong together -- not seen) is passed on as it is instead of being read.
template<bool EMIT>
static __device__ __forceinline__ uint32_t eqx_walk(const uint32_t *src, uint32_t c, const uint8_t *q, const uint8_t *t, uint32_t ql, uint32_t tl,
		uint32_t qp, uint32_t tp, uint32_t *dst, uint32_t dcap, uint32_t lane){
	uint32_t ob = 0;           // expanded words in front of this tile
	for(uint32_t w0 = 0; w0 < c; w0 += 64u){
		const uint32_t i = w0 + lane;
		const bool have = i < c;
		const uint32_t w = have ? src[i] : 0u;
		const uint32_t op = w & 15u, len = w >> 4;
		const uint32_t qa = (op == BSA_CIGAR_M || op == BSA_CIGAR_I) ? len : 0u, ta = (op == BSA_CIGAR_M || op == BSA_CIGAR_D) ? len : 0u;
		const uint32_t qi = bsa_wave_iscan(qa, lane), ti = bsa_wave_iscan(ta, lane);
		const uint32_t qs = qp + qi - qa, ts = tp + ti - ta;          // where this lane's word starts
		qp += (uint32_t)__shfl(qi, 63); tp += (uint32_t)__shfl(ti, 63);
		const bool isM = have && op == BSA_CIGAR_M && len != 0u && qs <= ql && ts <= tl && len <= ql - qs && len <= tl - ts;
		const bool lng = isM && len > EQX_LANE_COLS;
		uint64_t mm = 0, st = 0;
		uint32_t nrun = have ? 1u : 0u;
		if(isM && !lng){
			for(uint32_t j = 0; j < len; j += 8u) mm |= (uint64_t)eqx_mis8(q + qs + j, t + ts + j) << j;
			const uint64_t vm = ~0ull >> (64u - len);
			mm &= vm;
			st = (mm ^ (mm << 1)) & vm & ~1ull;                       // columns that start a run, column 0 apart
			nrun = 1u + (uint32_t)__popcll(st);
		}
		if(lng) nrun = 0u;                                            // (counted below, by the wave)
		const uint32_t inc = bsa_wave_iscan(nrun, lane);
		const uint32_t eo = inc - nrun, tile_short = __shfl(inc, 63);
		uint32_t extra = 0, long_total = 0;                           // runs of long words on lower lanes / in this tile
		uint64_t lm = __ballot(lng);
		while(lm){
			const int L = __ffsll((unsigned long long)lm) - 1;
			lm &= lm - 1ull;
			const uint32_t wl = __shfl(len, L), wq = __shfl(qs, L), wt = __shfl(ts, L), wo = __shfl(eo, L);
			const uint32_t nl = eqx_long<EMIT>(q + wq, t + wt, wl, dst, ob + wo + long_total, dcap, lane);
			if((int)lane > L) extra += nl;
			long_total += nl;
		}
		if(EMIT && have && !lng){
			uint32_t o = ob + eo + extra;
			if(!isM){ if(o < dcap) dst[o] = w; }
			else {
				uint32_t s0 = 0, bit = (uint32_t)mm & 1u;
				while(st){
					const uint32_t s = (uint32_t)__ffsll((unsigned long long)st) - 1u;
					st &= st - 1ull;
					if(o < dcap) dst[o] = ((s - s0) << 4) | eqx_op(bit);
					o++; s0 = s; bit ^= 1u;
				}
				if(o < dcap) dst[o] = ((len - s0) << 4) | eqx_op(bit);
			}
		}
		ob += tile_short + long_total;
	}
	return ob;
}

// after a chunk's traceback, before the scan: cnt[ppos] (plain words) -> cnt_plain[ppos], the expanded count in its place
__global__ void __launch_bounds__(256) k_cigar_eqx_count(const uint8_t *rows, const uint64_t *slot_end, uint32_t first, uint32_t count,
		uint32_t *cnt, uint32_t *cnt_plain, EqxSeqs s){
	const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if(g >= count) return;
	const uint32_t ppos = first + g;
	const uint32_t c = cnt[ppos];
	if(lane == 0) cnt_plain[ppos] = c;
	if(c == 0u) return;
	const uint32_t pair = s.order[ppos];
	const uint32_t *src = (const uint32_t*)(rows + slot_end[ppos]) - c;
	const uint32_t n = eqx_walk<false>(src, c, s.qst + s.qpoff[pair], s.tst + s.tpoff[pair], s.qlen[pair], s.tlen[pair],
		(uint32_t)s.out[pair].qb, (uint32_t)s.out[pair].tb, nullptr, 0u, lane);
	if(lane == 0) cnt[ppos] = n;
}

// k_cigar_collect with the expansion on the way into the staging arena (several chunks: the slots are gone when the final offsets are known)
__global__ void __launch_bounds__(256) k_cigar_collect_eqx(const uint8_t *rows, const uint64_t *slot_end, uint32_t first, uint32_t count,
		const uint32_t *cnt, const uint32_t *cnt_plain, const uint64_t *off, uint32_t *tmp, uint64_t cap, EqxSeqs s){
	const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if(g >= count) return;
	const uint32_t ppos = first + g;
	const uint32_t c = cnt_plain[ppos], ce = cnt[ppos];
	const uint64_t o = off[ppos];
	if(c == 0u || o + ce > cap) return;
	const uint32_t pair = s.order[ppos];
	const uint32_t *src = (const uint32_t*)(rows + slot_end[ppos]) - c;
	(void)eqx_walk<true>(src, c, s.qst + s.qpoff[pair], s.tst + s.tpoff[pair], s.qlen[pair], s.tlen[pair],
		(uint32_t)s.out[pair].qb, (uint32_t)s.out[pair].tb, tmp + o, ce, lane);
}

// k_cigar_final_direct with the expansion: a plan of one chunk, from the slot tails straight to the caller's arena
__global__ void __launch_bounds__(256) k_cigar_final_direct_eqx(const uint8_t *rows, const uint64_t *slot_end, const uint32_t *cnt_pair, const uint64_t *pos_pair,
		const uint32_t *cnt_plain, const uint64_t *dst_off, uint32_t *dst, uint64_t cap, uint32_t n, EqxSeqs s){
	const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if(g >= n) return;
	const uint64_t pos = pos_pair[g];
	const uint32_t c = cnt_plain[pos], ce = cnt_pair[g];
	const uint64_t d = dst_off[g];
	if(c == 0u || d + ce > cap) return;
	const uint32_t *src = (const uint32_t*)(rows + slot_end[pos]) - c;
	(void)eqx_walk<true>(src, c, s.qst + s.qpoff[g], s.tst + s.tpoff[g], s.qlen[g], s.tlen[g],
		(uint32_t)s.out[g].qb, (uint32_t)s.out[g].tb, dst + d, ce, lane);
}

hipError_t bsa_launch_cigar_eqx_count(const uint8_t *rows, const uint64_t *slot_end, uint32_t first, uint32_t count, uint32_t *cnt, uint32_t *cnt_plain,
		const EqxSeqs &s, hipStream_t st){
	if(count == 0) return hipSuccess;
	hipLaunchKernelGGL(k_cigar_eqx_count, dim3((count + 3) / 4), dim3(256), 0, st, rows, slot_end, first, count, cnt, cnt_plain, s);
	return hipGetLastError();
}
hipError_t bsa_launch_cigar_collect_eqx(const uint8_t *rows, const uint64_t *slot_end, uint32_t first, uint32_t count, const uint32_t *cnt, const uint32_t *cnt_plain,
		const uint64_t *off, uint32_t *tmp, uint64_t cap, const EqxSeqs &s, hipStream_t st){
	if(count == 0) return hipSuccess;
	hipLaunchKernelGGL(k_cigar_collect_eqx, dim3((count + 3) / 4), dim3(256), 0, st, rows, slot_end, first, count, cnt, cnt_plain, off, tmp, cap, s);
	return hipGetLastError();
}
hipError_t bsa_launch_cigar_final_direct_eqx(const uint8_t *rows, const uint64_t *slot_end, const uint32_t *cnt_pair, const uint64_t *pos_pair, const uint32_t *cnt_plain,
		const uint64_t *dst_off, uint32_t *dst, uint64_t cap, uint32_t n, const EqxSeqs &s, hipStream_t st){
	if(n == 0) return hipSuccess;
	hipLaunchKernelGGL(k_cigar_final_direct_eqx, dim3((n + 3) / 4), dim3(256), 0, st, rows, slot_end, cnt_pair, pos_pair, cnt_plain, dst_off, dst, cap, n, s);
	return hipGetLastError();
}
