// bsa_kmer_dev.hip -- the k-mer chainer of bsa_kmer.cpp (chain()) on the device: one workgroup per pair, many pairs side by side.
//
// The stages are those of the host code and give the same anchors word for word (tests/test_kmer_chain_gpu.py):
//   (a) every lane rebuilds the canonical k-mer in front of its position from the ksz bytes there (no dependency between positions) and writes
//       the host's 64-bit record  kmer << 34 | offset << 2 | from-the-target << 1 | reverse-strand-is-canonical;
//   (b) a stable LSD radix sort of the records by k-mer, five bits a pass, between the two halves of the pair's workspace slice: every lane owns a
//       contiguous piece of the array and a column of the 32 x 256 counter table in LDS, so neither the counting nor the scatter needs an atomic;
//       runs of exactly two records from different sequences on the same strand are the hits (with the host's zero-sentinel quirk);
//   (c) the hits are ordered by query offset by writing target offset + 1 at index `query offset` of a zeroed array (the keys are unique) and
//       compacting that array in order;
//   (d) the longest increasing subsequence over the target offsets with the reference's literal predecessor rule: a dependent chain, run by ONE
//       lane with the tail array (index and target offset) and the first predecessors in the LDS the sort no longer needs;
//   (e) the backward walk with the first coverage test (the same lane), then the iterated diagonal filter across the workgroup: integer sum and
//       truncating mean, the element of rank e / 2 by bisection on the diagonal's value, var = max(3 |median - mean|, 50), until nothing is dropped;
//       an ordered compaction and the second coverage test;
//   (f) per-pair counts, a scan (k_kmer_scan) and a gather (k_kmer_gather) into the packed arena.
// A byte above 3 enters the forward k-mer the way the host's rolling update lets it (OR of byte << 2 j under the mask), so that bsa_kmer_edit_batch2
// can reproduce bsa_kmer_edit_batch on such pairs; bsa_kmer_chain_batch asks for no anchors there instead (`literal` = 0).
//
// BSA_MODE_SEQ2BIT / BSA_MODE_QSTRAND (bsa_kmer_chain_batch2, bsa_kmer_edit_batch2): k_kmer_chain<PK, QS> -- only the bad-base scan and stage (a) differ,
// everything from the sort on reads the same records.  <false, false> is the kernel without flags, statement for statement.
//   QS  a marked query stands for q', q'[i] = 3 - q[qlen - 1 - i]: the k-mer of q' at position p is the reverse complement of the stored k-mer at
//       nq - 1 - p, so the lane reads the mirrored position and swaps the roles of its two k-mers.  A marked query with a code above 3 has no q':
//       BSA_ST_BAD_BASE and no anchors, whatever `literal` says.
//   PK  the sequences are 2-bit words, 32 bases each from the top bit down (bsa_common.h), offsets are base offsets: the forward k-mer comes from the
//       one or two words that hold it (funnel shift), its reverse complement from a bit reversal with the bits of each pair swapped back -- no
//       loop over bases, no bad-base scan, no word read that holds no base of the read.
//
// BSA_KMER_STRAND_AUTO: k_kmer_chain<PK, false, true> finds the pair's strand itself.  Stages (a) and (b) are those of <PK, false>: the unmarked records,
// ONE sort.  A run of exactly two records with different flg is a forward hit (qo, to) when the dir bits are equal and a hit (nq - 1 - qo, to) against
// q' when they differ -- or when the k-mer is its own reverse complement, whose dir is 0 on both strands (even ksz).  Those are the records the QS
// kernel would have sorted for a marked query: the same canonical k-mers, dir flipped (but for those k-mers), positions
// mirrored, and the query record still ahead of the target record inside a run (the sort is stable and the query records come first) -- so the run
// boundaries and the zero-sentinel test `i + 2 == n && kmer == 0` are the same for both strands.  Stages (c) to (e) are one function (kc_chain_hits),
// called once per strand: the forward pass keeps its hits in the 8 min(qlen, tlen) extra bytes behind the slice's halves so that the sorted records
// survive it, its anchors then move there, and the reverse pass runs with the layout of the other kernels.  Reverse exactly when it has MORE anchors;
// a pair with a base code above 3 is chained forward only.
#include "bsa_pass.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>


#define KC_THREADS   256
#define KC_BITS      5u                  // radix digit
#define KC_TAIL_CAP  3072u               // LIS tail entries (index, target offset) kept in LDS; longer tails go on in the slice
#define KC_PREV_CAP  4000u               // predecessors of the first hits kept in LDS
#define KC_LDS_WORDS (2u * KC_TAIL_CAP + KC_PREV_CAP)       // 40 KB: four workgroups a CU
static_assert((32u * KC_THREADS) + (32u * KC_THREADS) / 32u <= KC_LDS_WORDS, "the padded counter table of the sort fits the same LDS");
#define KC_NONE 0xFFFFFFFFu

// one pair of a launch: offsets into the packed sequence bytes and into the workspace
struct KcPair { uint64_t qoff, toff, slot; uint32_t qlen, tlen, cmin, rc; };       // rc: the query is marked (QS kernels only)

// a pair's slice: two halves of this many bytes (each holds qlen + tlen records; what else lives there is smaller, see the kernel)
static inline __host__ __device__ size_t kc_half_bytes(uint32_t qlen, uint32_t tlen){ return ((((size_t)qlen + tlen) * 8u + 15u) & ~(size_t)15u) + 16u; }

__device__ __forceinline__ uint32_t kc_block_sum(uint32_t v, uint32_t *red){
	for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	__syncthreads();
	if((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	uint32_t s = 0;
	for(uint32_t k = 0; k < KC_THREADS / 64; k++) s += red[k];
	return s;
}
__device__ __forceinline__ uint32_t kc_block_excl_scan(uint32_t v, uint32_t *red, uint32_t &total){
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	uint32_t inc = v;
	for(uint32_t o = 1; o < 64; o <<= 1){ const uint32_t t = __shfl_up(inc, o); if(lane >= o) inc += t; }
	__syncthreads();
	if(lane == 63) red[w] = inc;
	__syncthreads();
	uint32_t base = 0, tot = 0;
	for(uint32_t k = 0; k < KC_THREADS / 64; k++){ const uint32_t x = red[k]; if(k < w) base += x; tot += x; }
	total = tot;
	return base + inc - v;
}
__device__ __forceinline__ uint32_t kc_pad(uint32_t i){ return i + (i >> 5); }        // counter table: a lane's 32 consecutive entries start in different banks

// the 2 ksz bits (ksz <= 15) of a packed sequence from base offset o on; the second word is read only where the k-mer reaches into it
__device__ __forceinline__ uint32_t kc_kmer2bit(const uint64_t *__restrict__ W, uint64_t o, uint32_t ksz){
	const uint64_t wi = o >> 5;
	const uint32_t s = ((uint32_t)o & 31u) << 1;
	uint64_t x = W[wi] << s;
	if(s + 2u * ksz > 64u) x |= W[wi + 1] >> (64u - s);           // (s > 0 here)
	return (uint32_t)(x >> (64u - 2u * ksz));
}
// reverse complement of a k-mer: the 2-bit groups in reverse order (bit reversal, then the two bits of every group swapped back), complemented
__device__ __forceinline__ uint32_t kc_revcomp2bit(uint32_t fwd, uint32_t ksz){
	uint32_t r = __brev(fwd);
	r = ((r & 0xAAAAAAAAu) >> 1) | ((r & 0x55555555u) << 1);
	return (~r) >> ((16u - ksz) << 1);
}

// Runs of exactly two records with different flg and equal dir (REV: different dir -- a hit against q', at the mirrored query position) in the sorted
// records `src`: target offset + 1 at index `query offset` of the zeroed `slotq`.  A run of k-mer 0 that reaches the end is never closed (the host's
// zeroed sentinel).  A k-mer that is its own reverse complement (even ksz only) has dir 0 on either strand of either sequence: its run is a hit
// forward AND against q'.
template <bool REV>
__device__ __forceinline__ void kc_mark_hits(const uint64_t *src, uint32_t nrec, uint32_t *slotq, uint32_t qlen, uint32_t nq, uint32_t ksz){
	const uint32_t tid = threadIdx.x;
	for(uint32_t i = tid; i < qlen; i += KC_THREADS) slotq[i] = 0;
	__syncthreads();
	for(uint32_t i = tid; i + 1u < nrec; i += KC_THREADS){
		const uint64_t r = src[i], r1 = src[i + 1];
		const uint32_t k = (uint32_t)(r >> 34);
		if((uint32_t)(r1 >> 34) != k) continue;
		if(i > 0 && (uint32_t)(src[i - 1] >> 34) == k) continue;
		if(i + 2u < nrec){ if((uint32_t)(src[i + 2] >> 34) == k) continue; }
		else if(k == 0) continue;
		if((((uint32_t)r ^ (uint32_t)r1) & 2u) == 0) continue;
		if constexpr (REV){ if((((uint32_t)r ^ (uint32_t)r1) & 1u) == 0 && kc_revcomp2bit(k, ksz) != k) continue; }
		else if((((uint32_t)r ^ (uint32_t)r1) & 1u) != 0) continue;
		const uint64_t kq = ((uint32_t)r & 2u) ? r1 : r, kt = ((uint32_t)r & 2u) ? r : r1;
		const uint32_t qs = (uint32_t)(kq >> 2), to = (uint32_t)(kt >> 2);
		const uint32_t qo = REV ? nq - 1u - qs : qs;
		if(qo < qlen) slotq[qo] = to + 1u;
	}
	__syncthreads();
}

// Stages (c) to (e) and the second coverage test on the hits `slotq` holds (it may be the start of `work`); `hits` (nh <= min(qlen, tlen) words) and `work`
// (13 nh bytes) are distinct.  Where the chain reaches the end, done(anchors, where they are) is called by every lane; an early return means no anchors.
template <typename Done>
__device__ __forceinline__ void kc_chain_hits(const uint32_t *slotq, uint64_t *hits, uint64_t *work, uint32_t qlen, uint32_t tlen, uint32_t ksz, uint32_t cmin,
		uint32_t *lds, uint32_t *red, uint32_t *s_flag, Done done){
	const uint32_t tid = threadIdx.x;
	// (c) the hits in query order: compact slotq into `hits`
	uint32_t nh;
	{
		const uint32_t per = (qlen + KC_THREADS - 1u) / KC_THREADS;
		const uint32_t b0 = min(tid * per, qlen), e0 = min(b0 + per, qlen);
		uint32_t c = 0;
		for(uint32_t i = b0; i < e0; i++) c += slotq[i] != 0;
		uint32_t w = kc_block_excl_scan(c, red, nh);
		for(uint32_t i = b0; i < e0; i++){ const uint32_t v = slotq[i]; if(v){ hits[w ++] = (uint64_t)i << 32 | (v - 1u); } }
	}
	__syncthreads();
	if(nh * ksz < cmin) return;
	// `work` now: [out: nh u64 (the LIS tail beyond its LDS part until then)] [prev: nh u32] [keep: nh bytes] -- 13 nh <= 6.5 (qlen + tlen) bytes
	uint64_t *outp = work;
	uint32_t *gtail = (uint32_t*)work;                    // index at [m], target offset at [nh + m]
	uint32_t *gprev = (uint32_t*)(work + nh);
	uint8_t  *keep  = (uint8_t*)(gprev + nh);
	for(uint32_t i = tid; i < nh; i += KC_THREADS) keep[i] = 0;
	__syncthreads();
	// (d) + first half of (e): one lane
	if(tid == 0){
		uint32_t *tl_i = lds, *tl_v = lds + KC_TAIL_CAP, *pv = lds + 2u * KC_TAIL_CAP;
		auto set_tail = [&](uint32_t m, uint32_t i, uint32_t v){ if(m < KC_TAIL_CAP){ tl_i[m] = i; tl_v[m] = v; } else { gtail[m] = i; gtail[nh + m] = v; } };
		auto tail_v = [&](uint32_t m){ return m < KC_TAIL_CAP ? tl_v[m] : gtail[nh + m]; };
		auto tail_i = [&](uint32_t m){ return m < KC_TAIL_CAP ? tl_i[m] : gtail[m]; };
		auto set_prev = [&](uint32_t i, uint32_t v){ if(i < KC_PREV_CAP) pv[i] = v; else gprev[i] = v; };
		auto get_prev = [&](uint32_t i){ return i < KC_PREV_CAP ? pv[i] : gprev[i]; };
		uint32_t len = 1, first_v = (uint32_t)hits[0], last_v = first_v, last_i = 0;
		set_tail(0, 0, first_v); set_prev(0, KC_NONE);
		uint32_t nxt = nh > 1 ? (uint32_t)hits[1] : 0;
		for(uint32_t i = 1; i < nh; i++){
			const uint32_t tv = nxt;
			if(i + 1u < nh) nxt = (uint32_t)hits[i + 1];
			if(tv > last_v){
				set_prev(i, last_i);
				set_tail(len, i, tv); len ++;
				last_v = tv; last_i = i;
			} else if(tv <= first_v){
				set_prev(i, KC_NONE);
				set_tail(0, i, tv);
				first_v = tv;
				if(len == 1){ last_v = tv; last_i = i; }
			} else {
				uint32_t b = 0, e = len;
				while(b < e){
					const uint32_t m = b + ((e - b) >> 1), mv = tail_v(m);
					if(tv > mv) b = m + 1;
					else if(tv < mv) e = m;
					else { b = m; break; }
				}
				if(b == 0 || b >= len) b = b == 0 ? 1 : len - 1;       // (cannot happen: first_v < tv <= last_v)
				set_prev(i, get_prev(tail_i(b - 1)));                // as written in the reference: the predecessor of that tail, not the tail
				set_tail(b, i, tv);
				if(b == len - 1u){ last_v = tv; last_i = i; }
			}
		}
		uint32_t cov = 0, e = KC_NONE, m = last_i;
		while(m != KC_NONE && m < nh){
			const uint32_t tf = (uint32_t)hits[m];
			keep[m] = 1;
			cov += (tf + ksz <= e) ? ksz : e - tf;
			e = tf;
			m = get_prev(m);
		}
		*s_flag = cov >= cmin;
	}
	__syncthreads();
	if(!*s_flag) return;
	// (e) the diagonal filter across the workgroup (a lane always looks at the same hits)
	for(;;){
		uint32_t e = 0, tot = 0;
		for(uint32_t i = tid; i < nh; i += KC_THREADS) if(keep[i]){ const uint64_t h = hits[i]; tot += (uint32_t)(h >> 32) - (uint32_t)h; e ++; }
		e = kc_block_sum(e, red);
		tot = kc_block_sum(tot, red);
		if(e * ksz < cmin) break;
		const int mean = (int)tot / (int)e;
		const uint32_t rank = e / 2u;
		int lo = -(int)tlen, hi = (int)qlen;                    // the element of rank e / 2: the smallest v with more than `rank` diagonals <= v
		while(lo < hi){
			const int mid = lo + ((hi - lo) >> 1);
			uint32_t c = 0;
			for(uint32_t i = tid; i < nh; i += KC_THREADS) if(keep[i]){ const uint64_t h = hits[i]; c += (int)((uint32_t)(h >> 32) - (uint32_t)h) <= mid; }
			c = kc_block_sum(c, red);
			if(c > rank) hi = mid; else lo = mid + 1;
		}
		const int median = lo;
		const int var = max(abs(median - mean) * 3, 50);
		uint32_t dropped = 0;
		for(uint32_t i = tid; i < nh; i += KC_THREADS) if(keep[i]){
			const uint64_t h = hits[i];
			const int d = (int)((uint32_t)(h >> 32) - (uint32_t)h);
			if(abs(d - mean) > var){ keep[i] = 0; dropped ++; }
		}
		dropped = kc_block_sum(dropped, red);
		if(dropped == 0) break;
	}
	__syncthreads();
	// final compaction (in order) and the second coverage test
	uint32_t w_tot;
	{
		const uint32_t per = (nh + KC_THREADS - 1u) / KC_THREADS;
		const uint32_t b0 = min(tid * per, nh), e0 = min(b0 + per, nh);
		uint32_t c = 0;
		for(uint32_t i = b0; i < e0; i++) c += keep[i] != 0;
		uint32_t w = kc_block_excl_scan(c, red, w_tot);
		for(uint32_t i = b0; i < e0; i++) if(keep[i]) outp[w ++] = hits[i];
	}
	__syncthreads();
	uint32_t cov = 0;
	for(uint32_t i = tid; i < w_tot; i += KC_THREADS){
		const uint32_t tf = (uint32_t)outp[i], e = i ? (uint32_t)outp[i - 1] + ksz : 0u;
		cov += (tf >= e + ksz) ? ksz : tf + ksz - e;
	}
	cov = kc_block_sum(cov, red);
	done(cov < cmin ? 0u : w_tot, outp);
}


template <bool PK, bool QS, bool AUTO>
__global__ __launch_bounds__(KC_THREADS) void k_kmer_chain(const uint8_t *__restrict__ seqs, const KcPair *__restrict__ pairs, uint8_t *ws, uint32_t ksz,
		uint32_t literal, uint32_t *cnt_out, uint64_t *res_off, uint32_t *status){
	__shared__ uint32_t lds[KC_LDS_WORDS];
	__shared__ uint32_t red[KC_THREADS / 64];
	__shared__ uint32_t s_flag;
	const uint32_t tid = threadIdx.x, pair = blockIdx.x;
	const KcPair P = pairs[pair];
	const uint8_t *q = seqs + P.qoff, *t = seqs + P.toff;
	const uint32_t qlen = P.qlen, tlen = P.tlen, cmin = P.cmin;
	const uint32_t nq = qlen >= ksz ? qlen - ksz + 1u : 0u, nt = tlen >= ksz ? tlen - ksz + 1u : 0u, nrec = nq + nt;
	const size_t half = kc_half_bytes(qlen, tlen);
	uint64_t *src = (uint64_t*)(ws + P.slot), *dst = (uint64_t*)(ws + P.slot + half);

	// base codes above 3 (the whole of both sequences, also where no k-mer fits)
	uint32_t bad = 0, noq = 0;                                 // noq: a marked query that has no reverse complement
	if constexpr (!PK){
		uint32_t any = 0;
		for(uint32_t i = tid; i < qlen; i += KC_THREADS) any |= q[i];
		if constexpr (QS) noq = (P.rc && __syncthreads_or(any > 3u)) ? 1u : 0u;
		for(uint32_t i = tid; i < tlen; i += KC_THREADS) any |= t[i];
		bad = __syncthreads_or(any > 3u) ? 1u : 0u;
	}
	const uint32_t st = (bad ? BSA_ST_BAD_BASE : 0u) | ((qlen == 0 || tlen == 0) ? BSA_ST_EMPTY : 0u);
	if(tid == 0){ if(status) status[pair] = st; cnt_out[pair] = 0; res_off[pair] = P.slot; }
	if(nrec == 0 || nq == 0 || nt == 0 || (bad && !literal) || noq) return;

	// (a) canonical k-mers, lanes over positions
	if constexpr (PK || QS){
		const uint32_t mask = 0xFFFFFFFFu >> ((16u - ksz) << 1);
		const uint64_t *W = (const uint64_t*)seqs;
		for(uint32_t i = tid; i < nrec; i += KC_THREADS){
			const uint32_t flg = i >= nq, p = flg ? i - nq : i;
			const bool mir = QS && !flg && P.rc;
			const uint32_t ps = mir ? nq - 1u - p : p;           // the stored k-mer that is the reverse complement of q' at p
			uint32_t fwd = 0, rev = 0;
			if constexpr (PK){
				fwd = kc_kmer2bit(W, (flg ? P.toff : P.qoff) + ps, ksz);
				rev = kc_revcomp2bit(fwd, ksz);
			} else {
				const uint8_t *s = (flg ? t : q) + ps;
				for(uint32_t m = 0; m < ksz; m++){
					const uint32_t b = s[m];
					fwd |= b << ((ksz - 1u - m) << 1);
					rev |= ((~b) & 3u) << (m << 1);
				}
				fwd &= mask;
			}
			if(mir){ const uint32_t x = fwd; fwd = rev; rev = x; }
			const uint32_t dir = rev < fwd;
			const uint64_t kmer = (dir ? rev : fwd) & 0x3FFFFFFFu;
			src[i] = kmer << 34 | (uint64_t)p << 2 | (uint64_t)(flg << 1) | dir;
		}
	} else {
		const uint32_t mask = 0xFFFFFFFFu >> ((16u - ksz) << 1);
		for(uint32_t i = tid; i < nrec; i += KC_THREADS){
			const uint32_t flg = i >= nq, p = flg ? i - nq : i;
			const uint8_t *s = (flg ? t : q) + p;
			uint32_t fwd = 0, rev = 0;
			for(uint32_t m = 0; m < ksz; m++){
				const uint32_t b = s[m];
				fwd |= b << ((ksz - 1u - m) << 1);
				rev |= ((~b) & 3u) << (m << 1);
			}
			fwd &= mask;
			const uint32_t dir = rev < fwd;
			const uint64_t kmer = (dir ? rev : fwd) & 0x3FFFFFFFu;
			src[i] = kmer << 34 | (uint64_t)p << 2 | (uint64_t)(flg << 1) | dir;
		}
	}
	__syncthreads();

	// (b) stable LSD radix sort on the 2 ksz k-mer bits
	{
		const uint32_t per = (nrec + KC_THREADS - 1u) / KC_THREADS;
		const uint32_t b0 = min(tid * per, nrec), e0 = min(b0 + per, nrec);
		const uint32_t passes = (2u * ksz + KC_BITS - 1u) / KC_BITS;
		for(uint32_t p = 0; p < passes; p++){
			const uint32_t sh = 34u + p * KC_BITS;
			for(uint32_t d = 0; d < 32u; d++) lds[kc_pad(d * KC_THREADS + tid)] = 0;
			for(uint32_t i = b0; i < e0; i++) lds[kc_pad((uint32_t)((src[i] >> sh) & 31u) * KC_THREADS + tid)] ++;
			__syncthreads();
			uint32_t sum = 0;
			for(uint32_t j = 0; j < 32u; j++){ const uint32_t x = kc_pad(32u * tid + j), v = lds[x]; lds[x] = sum; sum += v; }
			uint32_t total;
			const uint32_t base = kc_block_excl_scan(sum, red, total);
			for(uint32_t j = 0; j < 32u; j++) lds[kc_pad(32u * tid + j)] += base;
			__syncthreads();
			for(uint32_t i = b0; i < e0; i++){
				const uint64_t r = src[i];
				const uint32_t x = kc_pad((uint32_t)((r >> sh) & 31u) * KC_THREADS + tid);
				const uint32_t w = lds[x];
				lds[x] = w + 1u;
				if(w < nrec) dst[w] = r;
			}
			__syncthreads();
			uint64_t *sw = src; src = dst; dst = sw;
		}
	}
	// src: the sorted records; dst: free
	if constexpr (!AUTO){
		kc_mark_hits<false>(src, nrec, (uint32_t*)dst, qlen, nq, ksz);
		// the hits go to `src` (the sorted records are no longer needed)
		kc_chain_hits((const uint32_t*)dst, src, dst, qlen, tlen, ksz, cmin, lds, red, &s_flag, [&](uint32_t c, const uint64_t *outp){
			if(tid == 0){ cnt_out[pair] = c; res_off[pair] = P.slot + (size_t)((const uint8_t*)outp - (ws + P.slot)); }
		});
	} else {
		// forward: the hits go behind the two halves, so the sorted records survive; the anchors follow them there
		uint64_t *fwd = (uint64_t*)(ws + P.slot + 2u * half);
		uint32_t cf = 0, cr = 0;
		kc_mark_hits<false>(src, nrec, (uint32_t*)dst, qlen, nq, ksz);
		kc_chain_hits((const uint32_t*)dst, fwd, dst, qlen, tlen, ksz, cmin, lds, red, &s_flag, [&](uint32_t c, const uint64_t *outp){
			cf = c;
			for(uint32_t i = tid; i < c; i += KC_THREADS) fwd[i] = outp[i];
		});
		__syncthreads();
		// reverse: as the other kernels, the hits over the records
		if(!bad){
			kc_mark_hits<true>(src, nrec, (uint32_t*)dst, qlen, nq, ksz);
			kc_chain_hits((const uint32_t*)dst, src, dst, qlen, tlen, ksz, cmin, lds, red, &s_flag, [&](uint32_t c, const uint64_t *){ cr = c; });
		}
		if(tid == 0){
			const bool rv = cr > cf;                            // a tie is forward
			cnt_out[pair] = rv ? cr : cf;
			res_off[pair] = P.slot + (rv ? (size_t)((uint8_t*)dst - (ws + P.slot)) : 2u * half);
			if(rv && status) status[pair] = st | BSA_ST_REVCOMP;
		}
	}
}

// (f) exclusive scan of the per-pair counts (one workgroup; off has n + 1 entries) ...
__global__ __launch_bounds__(KC_THREADS) void k_kmer_scan(const uint32_t *__restrict__ cnt, uint32_t *off, uint32_t n){
	__shared__ uint32_t red[KC_THREADS / 64];
	const uint32_t tid = threadIdx.x, per = (n + KC_THREADS - 1u) / KC_THREADS;
	const uint32_t b0 = min(tid * per, n), e0 = min(b0 + per, n);
	uint32_t c = 0, total;
	for(uint32_t i = b0; i < e0; i++) c += cnt[i];
	uint32_t w = kc_block_excl_scan(c, red, total);
	for(uint32_t i = b0; i < e0; i++){ off[i] = w; w += cnt[i]; }
	if(tid == 0) off[n] = total;
}
// ... and the gather of every pair's anchors into the packed arena
__global__ __launch_bounds__(KC_THREADS) void k_kmer_gather(const uint8_t *__restrict__ ws, const uint64_t *__restrict__ res_off, const uint32_t *__restrict__ cnt,
		const uint32_t *__restrict__ off, uint64_t *arena, uint64_t arena_cap){
	const uint32_t pair = blockIdx.x, c = cnt[pair];
	const uint64_t *s = (const uint64_t*)(ws + res_off[pair]);
	const uint64_t o = off[pair];
	for(uint32_t i = threadIdx.x; i < c; i += KC_THREADS) if(o + i < arena_cap) arena[o + i] = s[i];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// the largest pair the device route takes (qlen + tlen); longer pairs are chained by the host code in the same call
extern "C" uint32_t bsa_kmer_dev_max_internal(void){ return 1u << 18; }

static uint32_t kc_min_cover(uint32_t qlen, uint32_t tlen, uint32_t ksz){       // bsa_kmer.cpp: min_cover (double arithmetic on the host, as there)
	uint32_t c = (uint32_t)(std::min(qlen, tlen) * 0.05 + 1);
	return std::min(c, 2 * ksz);
}
// what one pair needs of the scratch: its slice, its packed bytes, its share of the arena and of the tables
// (automatic: a BSA_KMER_STRAND_AUTO launch, whose slice also keeps the forward strand's anchors behind the two halves)
static inline size_t kc_auto_bytes(uint32_t qlen, uint32_t tlen){ return (8u * (size_t)std::min(qlen, tlen) + 15u) & ~(size_t)15u; }
static size_t kc_pair_bytes(uint32_t qlen, uint32_t tlen, bool automatic){
	return 2u * kc_half_bytes(qlen, tlen) + 256u + ((size_t)qlen + tlen) + 8u * (size_t)std::min(qlen, tlen) + sizeof(KcPair) + 32u + (automatic ? kc_auto_bytes(qlen, tlen) : 0u);
}

// Chains the pairs idx[0 .. m) on the device.  *arena_out (malloc'd, the caller frees it) holds their anchors packed, those of idx[j] at off[j] .. off[j + 1);
// st (m entries, may be NULL) gets BSA_ST_EMPTY / BSA_ST_BAD_BASE; fits[j] = 0 marks a pair that alone is larger than the workspace (left to the host, no anchors
// here).  *ms: the kernels' time by HIP events.
// flags: BSA_MODE_SEQ2BIT -- seqs are 2-bit words and the offsets base offsets: a chunk uploads, for every read, the words that hold it, as they are (a
// quarter of the bytes); BSA_MODE_QSTRAND -- bit 63 of qoff[k] marks the pair, the stored bytes or words go up unchanged and the kernel reads them mirrored;
// BSA_KMER_STRAND_AUTO (not with QSTRAND) -- the <PK, false, true> kernels, 8 min(qlen, tlen) more bytes a slice, and st[j] carries BSA_ST_REVCOMP where the
// anchors are those of the reverse strand.
extern "C" int bsa_kmer_chain_dev_internal(bsa_ctx_t *ctx, const uint8_t *seqs, const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen,
		const uint32_t *idx, size_t m, uint32_t ksz, uint32_t literal, uint32_t flags, uint64_t **arena_out, uint64_t *off, uint32_t *st, uint8_t *fits, double *ms){
	const bool pk = (flags & BSA_MODE_SEQ2BIT) != 0, qs = (flags & BSA_MODE_QSTRAND) != 0, au = (flags & BSA_KMER_STRAND_AUTO) != 0;
	if(au && qs) return BSA_E_ARG;
	const uint64_t qmask = qs ? ~BSA_QOFF_REVCOMP : ~0ull;
	auto kern = au ? (pk ? k_kmer_chain<true, false, true> : k_kmer_chain<false, false, true>)
		: pk ? (qs ? k_kmer_chain<true, true, false> : k_kmer_chain<true, false, false>) : (qs ? k_kmer_chain<false, true, false> : k_kmer_chain<false, false, false>);
	*arena_out = nullptr; *ms = 0.0;
	off[0] = 0;
	if(ksz > 15) ksz = 15;
	if(m == 0) return BSA_OK;
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);
	if(rc != BSA_OK) return rc;
	size_t budget = bsa_ctx_workspace_limit_internal(ctx);
	if(budget == 0){
		size_t fr = 0, tot = 0;
		budget = (size_t)2 << 30;
		if(hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::min(budget, fr / 2);
	}
	budget = budget > 4096 ? budget - 4096 : 0;
	std::vector<uint64_t> arena;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	if(hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess){ if(ev0) (void)hipEventDestroy(ev0); return BSA_E_HIP; }
	std::vector<KcPair> meta;
	std::vector<uint8_t> pack;
	std::vector<uint32_t> h_off, h_st;
	rc = BSA_OK;
	size_t j0 = 0;
	while(j0 < m && rc == BSA_OK){
		// the chunk [j0, j1): as many pairs as the budget holds; a pair that does not fit alone is left to the caller
		size_t j1 = j0, bytes = 0, seqb = 0, slots = 0, acap = 0;
		meta.clear();
		while(j1 < m){
			const uint32_t k = idx[j1], ql = qlen[k], tl = tlen[k];
			const size_t need = kc_pair_bytes(ql, tl, au);
			if(need > budget){
				if(j1 > j0) break;                    // close the chunk in front of it
				fits[j1] = 0; off[j1 + 1] = off[j1]; if(st) st[j1] = 0;
				j0 = ++j1; continue;
			}
			if(bytes + need > budget || acap + std::min(ql, tl) > 0x7FFFFFF0ull || meta.size() >= 0x7FFFFFF0ull) break;
			fits[j1] = 1;
			KcPair P; P.slot = slots; P.qlen = ql; P.tlen = tl; P.cmin = kc_min_cover(ql, tl, ksz); P.rc = (qs && (qoff[k] & BSA_QOFF_REVCOMP)) ? 1u : 0u;
			if(pk){
				// the words [off / 32, (off + len + 31) / 32) of each read, the read at the same place inside its first word
				const uint64_t qo = qoff[k] & qmask, to = toff[k];
				P.qoff = (uint64_t)seqb * 4u + (qo & 31u); if(ql) seqb += (size_t)(((qo & 31u) + ql + 31u) >> 5) * 8u;
				P.toff = (uint64_t)seqb * 4u + (to & 31u); if(tl) seqb += (size_t)(((to & 31u) + tl + 31u) >> 5) * 8u;
			} else { P.qoff = seqb; P.toff = seqb + ql; seqb += (size_t)ql + tl; }
			meta.push_back(P);
			slots += 2u * kc_half_bytes(ql, tl) + (au ? kc_auto_bytes(ql, tl) : 0u); acap += std::min(ql, tl); bytes += need;
			j1 ++;
		}
		const size_t c = meta.size();
		if(c == 0) continue;
		// pack the chunk's sequences (the caller's blob may be far larger than what these pairs use)
		pack.resize(seqb);
		{
			const unsigned nth = seqb > ((size_t)4 << 20) ? 8u : 1u;
			auto body = [&](size_t a, size_t b){
				for(size_t j = a; j < b; j++){
					const uint32_t k = idx[j0 + j];
					const uint64_t qo = qoff[k] & qmask, to = toff[k];
					if(pk){
						if(meta[j].qlen) memcpy(pack.data() + (meta[j].qoff >> 5) * 8u, seqs + (qo >> 5) * 8u, (size_t)(((qo & 31u) + meta[j].qlen + 31u) >> 5) * 8u);
						if(meta[j].tlen) memcpy(pack.data() + (meta[j].toff >> 5) * 8u, seqs + (to >> 5) * 8u, (size_t)(((to & 31u) + meta[j].tlen + 31u) >> 5) * 8u);
						continue;
					}
					if(meta[j].qlen) memcpy(pack.data() + meta[j].qoff, seqs + qo, meta[j].qlen);
					if(meta[j].tlen) memcpy(pack.data() + meta[j].toff, seqs + toff[k], meta[j].tlen);
				}
			};
			if(nth == 1) body(0, c);
			else {
				std::vector<std::thread> pool;
				for(unsigned w = 0; w < nth; w++) pool.emplace_back(body, c * w / nth, c * (w + 1) / nth);
				for(auto &th : pool) th.join();
			}
		}
		// carve the scratch
		size_t o = 0;
		const size_t o_seq = o;  o += bsa_up256(seqb + 16);
		const size_t o_meta = o; o += bsa_up256(c * sizeof(KcPair));
		const size_t o_cnt = o;  o += bsa_up256(c * 4);
		const size_t o_off = o;  o += bsa_up256((c + 1) * 4);
		const size_t o_st = o;   o += bsa_up256(c * 4);
		const size_t o_res = o;  o += bsa_up256(c * 8);
		const size_t o_ar = o;   o += bsa_up256((acap + 1) * 8);
		const size_t o_ws = o;   o += bsa_up256(slots + 16);
		void *bufv = nullptr;
		if((rc = bsa_ctx_scratch_internal(ctx, 1, o, &bufv)) != BSA_OK) break;
		uint8_t *buf = (uint8_t*)bufv;
		auto hip_ok = [&](hipError_t e){ if(e != hipSuccess){ rc = BSA_E_HIP; return false; } return true; };
		if(seqb && !hip_ok(hipMemcpyAsync(buf + o_seq, pack.data(), seqb, hipMemcpyHostToDevice, stream))) break;
		if(!hip_ok(hipMemcpyAsync(buf + o_meta, meta.data(), c * sizeof(KcPair), hipMemcpyHostToDevice, stream))) break;
		if(!hip_ok(hipEventRecord(ev0, stream))) break;
		hipLaunchKernelGGL(kern, dim3((uint32_t)c), dim3(KC_THREADS), 0, stream, (const uint8_t*)(buf + o_seq), (const KcPair*)(buf + o_meta), buf + o_ws, ksz, literal,
			(uint32_t*)(buf + o_cnt), (uint64_t*)(buf + o_res), (uint32_t*)(buf + o_st));
		hipLaunchKernelGGL(k_kmer_scan, dim3(1), dim3(KC_THREADS), 0, stream, (const uint32_t*)(buf + o_cnt), (uint32_t*)(buf + o_off), (uint32_t)c);
		hipLaunchKernelGGL(k_kmer_gather, dim3((uint32_t)c), dim3(KC_THREADS), 0, stream, (const uint8_t*)(buf + o_ws), (const uint64_t*)(buf + o_res), (const uint32_t*)(buf + o_cnt),
			(const uint32_t*)(buf + o_off), (uint64_t*)(buf + o_ar), (uint64_t)acap);
		if(!hip_ok(hipGetLastError()) || !hip_ok(hipEventRecord(ev1, stream))) break;
		h_off.resize(c + 1); h_st.resize(c);
		if(!hip_ok(hipMemcpyAsync(h_off.data(), buf + o_off, (c + 1) * 4, hipMemcpyDeviceToHost, stream))) break;
		if(!hip_ok(hipMemcpyAsync(h_st.data(), buf + o_st, c * 4, hipMemcpyDeviceToHost, stream))) break;
		if(!hip_ok(hipStreamSynchronize(stream))) break;
		const size_t tot = h_off[c];
		if(tot > acap){ rc = BSA_E_HIP; break; }                 // (cannot happen: a pair has at most min(qlen, tlen) anchors)
		const size_t at = arena.size();
		arena.resize(at + tot);
		if(tot && !hip_ok(hipMemcpy(arena.data() + at, buf + o_ar, tot * 8, hipMemcpyDeviceToHost))) break;
		float t = 0;
		if(hip_ok(hipEventElapsedTime(&t, ev0, ev1))) *ms += t;
		for(size_t j = 0; j < c; j++){ off[j0 + j + 1] = at + h_off[j + 1]; if(st) st[j0 + j] = h_st[j]; }
		j0 = j1;
	}
	(void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
	if(rc != BSA_OK){ (void)hipGetLastError(); return rc; }
	uint64_t *a = (uint64_t*)malloc((arena.size() + 1) * sizeof(uint64_t));
	if(!a) return BSA_E_NOMEM;
	if(!arena.empty()) memcpy(a, arena.data(), arena.size() * sizeof(uint64_t));
	*arena_out = a;
	return BSA_OK;
}

// ---- the resident form: bsa_kmer_chain_plan_create / bsa_kmer_chain_run -------------------------------------------------------------------------
// The same k_kmer_chain kernels read the CALLER's device blob in place (KcPair.qoff / toff are the caller's offsets), the pair tables go up once when the
// plan is made, and a run is launches on the context stream and nothing else: per workspace chunk the chain kernel, k_kmer_scan_carry and
// k_kmer_gather_whole, which writes straight into the caller's arena.  Stream order is all that keeps chunk c + 1 from the slices chunk c still gathers from.

// (f) for a chunk of a plan: the exclusive scan of its counts in 64 bits, carried from chunk to chunk through the caller's array.  `off` points at the chunk's
// first entry: off[0] is what the chunk before wrote there as its total (the first chunk writes the 0 itself), off[i + 1] = off[0] + cnt[0] + .. + cnt[i].
// One workgroup; the counts of a chunk add up to less than 2^31 (the plan cuts its chunks that way), the totals across chunks do not have to.
__global__ __launch_bounds__(KC_THREADS) void k_kmer_scan_carry(const uint32_t *__restrict__ cnt, uint64_t *off, uint32_t n, uint32_t first){
	__shared__ uint32_t red[KC_THREADS / 64];
	const uint32_t tid = threadIdx.x, per = (n + KC_THREADS - 1u) / KC_THREADS;
	const uint32_t b0 = min(tid * per, n), e0 = min(b0 + per, n);
	const uint64_t base = first ? 0ull : off[0];              // (off[0] is read by every lane and written by none unless `first`, and then read by none)
	uint32_t c = 0, total;
	for(uint32_t i = b0; i < e0; i++) c += cnt[i];
	uint32_t w = kc_block_excl_scan(c, red, total);
	for(uint32_t i = b0; i < e0; i++){ w += cnt[i]; off[i + 1] = base + w; }
	if(first && tid == 0) off[0] = 0;
}
// ... and the gather into the CALLER's arena (off: the chunk's first entry, as above).  A pair is written whole or not at all: all of its words when its range
// ends inside the arena (off[pair + 1] <= arena_cap), none otherwise -- so nothing at or above arena_cap is touched, nor anything at or above the last
// offset, and with arena_cap == 0 `arena` is never dereferenced (it may be NULL: a count-only run).
__global__ __launch_bounds__(KC_THREADS) void k_kmer_gather_whole(const uint8_t *__restrict__ ws, const uint64_t *__restrict__ res_off, const uint32_t *__restrict__ cnt,
		const uint64_t *__restrict__ off, uint64_t *arena, uint64_t arena_cap){
	const uint32_t pair = blockIdx.x, c = cnt[pair];
	const uint64_t o = off[pair];
	if(c == 0 || o + c > arena_cap) return;
	const uint64_t *s = (const uint64_t*)(ws + res_off[pair]);
	for(uint32_t i = threadIdx.x; i < c; i += KC_THREADS) arena[o + i] = s[i];
}

// what one pair of a plan needs of the scratch: kc_pair_bytes without the packed sequence bytes and the staged arena (the kernels read the caller's blob and
// write the caller's arena)
static size_t kc_plan_pair_bytes(uint32_t qlen, uint32_t tlen, bool automatic){
	return 2u * kc_half_bytes(qlen, tlen) + 256u + sizeof(KcPair) + 32u + (automatic ? kc_auto_bytes(qlen, tlen) : 0u);
}

struct KcChunk { size_t j0, j1, slots; };                    // pairs [j0, j1) and the bytes of their slices
struct bsa_kmer_chain_plan {
	bsa_ctx_t *ctx = nullptr;
	size_t n = 0;
	uint32_t ksz = 0, flags = 0;
	KcPair *d_meta = nullptr;                                 // n entries, slot = the pair's offset inside its chunk's workspace
	std::vector<KcChunk> chunks;
	size_t scratch = 0;                                       // bytes of the context's scratch the largest chunk asks for
};
// a chunk's carve of the scratch: counts, result offsets, slices
static inline size_t kc_plan_o_res(size_t c){ return bsa_up256(c * 4); }
static inline size_t kc_plan_o_ws(size_t c){ return kc_plan_o_res(c) + bsa_up256(c * 8); }

extern "C" uint64_t bsa_kmer_chain_words_bound(const uint32_t *qlen, const uint32_t *tlen, size_t n){
	uint64_t w = 0;
	if(qlen && tlen) for(size_t k = 0; k < n; k++) w += std::min(qlen[k], tlen[k]);
	return w;
}
extern "C" void bsa_kmer_chain_plan_destroy(bsa_kmer_chain_plan_t *p){
	if(!p) return;
	if(p->d_meta) (void)hipFree(p->d_meta);
	delete p;
}
extern "C" uint32_t bsa_kmer_chain_plan_chunks(const bsa_kmer_chain_plan_t *p){ return p ? (uint32_t)p->chunks.size() : 0u; }

static int kc_plan_create(bsa_ctx_t *ctx, const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen, size_t n, uint32_t ksz, uint32_t flags,
		bsa_kmer_chain_plan_t **out){
	const bool qs = (flags & BSA_MODE_QSTRAND) != 0, au = (flags & BSA_KMER_STRAND_AUTO) != 0;
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);        // (also selects the context's device)
	if(rc != BSA_OK) return rc;
	size_t budget = bsa_ctx_workspace_limit_internal(ctx);
	if(budget == 0){
		size_t fr = 0, tot = 0;
		budget = (size_t)2 << 30;
		if(hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::min(budget, fr / 2);
	}
	budget = budget > 4096 ? budget - 4096 : 0;
	// no host route behind a run: every pair has to be one the kernels take
	const uint64_t lim = bsa_kmer_dev_max_internal();
	char msg[200];
	for(size_t k = 0; k < n; k++){
		const uint64_t sum = (uint64_t)qlen[k] + tlen[k];
		if(sum > lim){
			snprintf(msg, sizeof msg, "bsa_kmer_chain_plan_create: pair %zu has qlen + tlen = %llu, above %llu: chain it with bsa_kmer_chain_batch2", k, (unsigned long long)sum, (unsigned long long)lim);
			bsa_ctx_set_error_internal(ctx, msg);
			return BSA_E_UNSUPPORTED;
		}
		const size_t need = kc_plan_pair_bytes(qlen[k], tlen[k], au);
		if(need > budget){
			snprintf(msg, sizeof msg, "bsa_kmer_chain_plan_create: pair %zu alone needs %zu bytes of workspace, the limit leaves %zu: chain it with bsa_kmer_chain_batch2", k, need, budget);
			bsa_ctx_set_error_internal(ctx, msg);
			return BSA_E_UNSUPPORTED;
		}
	}
	std::unique_ptr<bsa_kmer_chain_plan, void(*)(bsa_kmer_chain_plan*)> p(new bsa_kmer_chain_plan(), bsa_kmer_chain_plan_destroy);
	p->ctx = ctx; p->n = n; p->ksz = ksz; p->flags = flags;
	std::vector<KcPair> meta(n);
	const uint64_t qmask = qs ? ~BSA_QOFF_REVCOMP : ~0ull;
	for(size_t j0 = 0; j0 < n; ){
		// the chunk [j0, j1): as many pairs as the budget holds
		size_t j1 = j0, bytes = 0, slots = 0, acap = 0;
		while(j1 < n){
			const uint32_t ql = qlen[j1], tl = tlen[j1];
			const size_t need = kc_plan_pair_bytes(ql, tl, au);
			if(j1 > j0 && (bytes + need > budget || acap + std::min(ql, tl) > 0x7FFFFFF0ull || j1 - j0 >= 0x7FFFFFF0ull)) break;
			KcPair &P = meta[j1];
			P.qoff = qoff[j1] & qmask; P.toff = toff[j1]; P.slot = slots; P.qlen = ql; P.tlen = tl;
			P.cmin = kc_min_cover(ql, tl, ksz); P.rc = (qs && (qoff[j1] & BSA_QOFF_REVCOMP)) ? 1u : 0u;
			slots += 2u * kc_half_bytes(ql, tl) + (au ? kc_auto_bytes(ql, tl) : 0u); acap += std::min(ql, tl); bytes += need;
			j1 ++;
		}
		p->chunks.push_back(KcChunk{ j0, j1, slots });
		p->scratch = std::max(p->scratch, kc_plan_o_ws(j1 - j0) + bsa_up256(slots + 16));
		j0 = j1;
	}
	if(n){
		if(hipMalloc((void**)&p->d_meta, n * sizeof(KcPair)) != hipSuccess){ p->d_meta = nullptr; (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_plan_create: no device memory for the pair table"); return BSA_E_NOMEM; }
		if(hipMemcpy(p->d_meta, meta.data(), n * sizeof(KcPair), hipMemcpyHostToDevice) != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_plan_create: upload of the pair table failed"); return BSA_E_HIP; }
	}
	*out = p.release();
	return BSA_OK;
}

extern "C" int bsa_kmer_chain_plan_create(bsa_ctx_t *ctx, const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen, size_t n,
		uint32_t ksz, uint32_t flags, bsa_kmer_chain_plan_t **out){
	if(!ctx || !out) return BSA_E_ARG;
	*out = nullptr;
	if(n && (!qoff || !qlen || !toff || !tlen)) return BSA_E_ARG;
	if(flags & ~(uint32_t)(BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND | BSA_KMER_STRAND_AUTO)){ bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_plan_create: unknown flag"); return BSA_E_ARG; }
	if((flags & BSA_MODE_QSTRAND) && (flags & BSA_KMER_STRAND_AUTO)){ bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_plan_create: BSA_KMER_STRAND_AUTO finds the strands, BSA_MODE_QSTRAND gives them"); return BSA_E_ARG; }
	if(n > 0xFFFFFFF0ull){ bsa_ctx_set_error_internal(ctx, "too many pairs"); return BSA_E_ARG; }
	try {
		return kc_plan_create(ctx, qoff, qlen, toff, tlen, n, ksz > 15 ? 15u : ksz, flags, out);
	} catch(...){
		return BSA_E_NOMEM;
	}
}

extern "C" int bsa_kmer_chain_run(bsa_kmer_chain_plan_t *p, const uint8_t *d_seqs, uint64_t *d_maps, size_t maps_cap, uint64_t *d_maps_off, uint32_t *d_status){
	if(!p || !d_maps_off || (p->n && !d_seqs) || (maps_cap && !d_maps)) return BSA_E_ARG;
	bsa_ctx_t *ctx = p->ctx;
	const bool pk = (p->flags & BSA_MODE_SEQ2BIT) != 0, qs = (p->flags & BSA_MODE_QSTRAND) != 0, au = (p->flags & BSA_KMER_STRAND_AUTO) != 0;
	if(au && !d_status){ bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_run: BSA_KMER_STRAND_AUTO reports the strands in d_status"); return BSA_E_ARG; }
	if(pk && ((uintptr_t)d_seqs & 7u)){ bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_run: a BSA_MODE_SEQ2BIT blob is 64-bit words, d_seqs has to be 8-byte aligned"); return BSA_E_ARG; }
	auto kern = au ? (pk ? k_kmer_chain<true, false, true> : k_kmer_chain<false, false, true>)
		: pk ? (qs ? k_kmer_chain<true, true, false> : k_kmer_chain<true, false, false>) : (qs ? k_kmer_chain<false, true, false> : k_kmer_chain<false, false, false>);
	// k-mer size 0: no anchors anywhere, the status as ever -- the kernel sees a k-mer no sequence is long enough for and leaves after its status word
	const uint32_t ksz = p->ksz ? p->ksz : 0xFFFFFFFFu;
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);
	if(rc != BSA_OK) return rc;
	hipEvent_t *ev = nullptr;
	if((rc = bsa_ctx_kmer_chain_events_internal(ctx, p->chunks.size(), (long)p->n, &ev)) != BSA_OK) return rc;
	if(p->chunks.empty()){                                    // n == 0: d_maps_off[0] = 0 is all there is to write
		hipLaunchKernelGGL(k_kmer_scan_carry, dim3(1), dim3(KC_THREADS), 0, stream, (const uint32_t*)nullptr, d_maps_off, 0u, 1u);
		if(hipGetLastError() != hipSuccess){ bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_run: launch failed"); return BSA_E_HIP; }
		return BSA_OK;
	}
	void *bufv = nullptr;
	if((rc = bsa_ctx_scratch_internal(ctx, 1, p->scratch, &bufv)) != BSA_OK) return rc;        // (waits for the stream only when it has to grow)
	uint8_t *buf = (uint8_t*)bufv;
	for(size_t ci = 0; ci < p->chunks.size(); ci++){
		const KcChunk &ch = p->chunks[ci];
		const uint32_t c = (uint32_t)(ch.j1 - ch.j0);
		uint32_t *cnt = (uint32_t*)buf;
		uint64_t *res = (uint64_t*)(buf + kc_plan_o_res(c));
		uint8_t *ws = buf + kc_plan_o_ws(c);
		if(hipEventRecord(ev[2 * ci], stream) != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_run: hipEventRecord failed"); return BSA_E_HIP; }
		hipLaunchKernelGGL(kern, dim3(c), dim3(KC_THREADS), 0, stream, d_seqs, (const KcPair*)(p->d_meta + ch.j0), ws, ksz, 0u, cnt, res, d_status ? d_status + ch.j0 : (uint32_t*)nullptr);
		hipLaunchKernelGGL(k_kmer_scan_carry, dim3(1), dim3(KC_THREADS), 0, stream, (const uint32_t*)cnt, d_maps_off + ch.j0, c, ci == 0 ? 1u : 0u);
		hipLaunchKernelGGL(k_kmer_gather_whole, dim3(c), dim3(KC_THREADS), 0, stream, (const uint8_t*)ws, (const uint64_t*)res, (const uint32_t*)cnt,
			(const uint64_t*)(d_maps_off + ch.j0), d_maps, (uint64_t)maps_cap);
		if(hipGetLastError() != hipSuccess || hipEventRecord(ev[2 * ci + 1], stream) != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_kmer_chain_run: launch failed"); return BSA_E_HIP; }
	}
	return BSA_OK;
}
