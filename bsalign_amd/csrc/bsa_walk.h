// bsa_walk.h -- the bookkeeping the traceback walkers share (bsa_align8.hip, bsa_align8_codes.hip, bsa_align8_sys.hip, bsa_edit.hip): the two CIGAR
// writers, the 8-byte base window, and for the walkers over code slots (bsa_align8_codes.hip) the view of a pair's slot, the start of the walk and
// its end.  The walks themselves -- tiles, rings, service points, ballots -- stay in the kernels.
#pragma once
#include "bsa_common.h"

// the zero record (score false: a bad walk over codes keeps the score it started from)
static __device__ __forceinline__ void bsa_result_zero(bsa_result_t &rs, bool score = true){
	if(score) rs.score = 0;
	rs.qb = rs.qe = rs.tb = rs.te = 0; rs.mat = rs.mis = rs.ins = rs.del = rs.aln = 0;
}
// ---- CIGAR words, a pair per lane: the reference's run-length merge (bsalign.h:409-417); word m goes to end - (m + 1), n counts them.  wr: whether this lane
// stores its words (k_align8_trace_sys<., WAVE> counts on all lanes and writes on one)
struct bsa_cig_lane_t {
	uint32_t *end; uint32_t n; bool wr;
	__device__ __forceinline__ bsa_cig_lane_t(uint32_t *cig_end, bool write = true) : end(cig_end), n(0), wr(write) {}
	__device__ __forceinline__ void push(uint32_t w){ n++; if(wr) *(end - n) = w; }
	__device__ __forceinline__ uint32_t add(uint32_t cg, uint32_t op, uint32_t sz){
		if(op == (cg & 0xf)) return cg + (sz << 4);
		if(cg) push(cg);
		return (sz << 4) | op;
	}
};

// ---- CIGAR words, a walk per wave.  The walker does not merge runs step by step (that logic was a third of the scalar instructions of a step): it
// records one TOKEN per gap event -- (matches / mismatches since the last event, op, length), one token per lane -- and a gap that simply goes on
// (no match in between, same op: the rows of a deletion run, consecutive insertions) extends its own token, so that neighbouring tokens never carry
// the same op.  Every 64 tokens (the last one stays: it may still grow) the lanes turn their tokens into words side by side: an M word when the run
// is not empty, then the gap's word, positions from two prefix popcounts (word m at end - (m + 1)).  The word sequence is the reference's run-length
// merge (bsalign.h:409-417) of the same op stream.
// tokN, tokB: the lane's token (run length; len << 2 | op, op 0: none) -- vector registers.  ntok, key: uniform -- tokens held, and the op of the last
// token << 28 | the match / mismatch columns since it, so that "same op, nothing in between" is one compare.  The key's low 28 bits must not
// overflow: fewer than 2^28 columns between two events (a walk over codes has fewer than 2^26 columns, bsa_api.hip sends longer queries to the
// literal kernels; 28 bits are also the length field of a CIGAR word, so a longer run has no word in the reference's format either).  The walkers
// add a run of match / mismatch columns to `key` themselves.
// (The members stand in this order on purpose: the compiler assigns the walk's registers in the order it meets them, and this order gives the
// instruction counts the walkers had with five separate variables -- profiles/walk_shared_isa_*.json; a comment does not change code, moving a line here does.)
struct bsa_cig_wave_t {
	static constexpr uint32_t KEYM = 0x0FFFFFFFu;
	uint32_t key, ntok, tokB, tokN, ncig, lane; uint32_t *end;
	__device__ __forceinline__ bsa_cig_wave_t(uint32_t *cig_end, uint32_t lane_) : key(0), ntok(0), tokB(0), tokN(0), ncig(0), lane(lane_), end(cig_end) {}
	__device__ __forceinline__ void flush(uint32_t cnt){
		const bool in = lane < cnt;
		tokN &= KEYM;
		const bool hasA = in && tokN != 0u, hasB = in && (tokB & 3u) != 0u;
		const uint64_t mA = __ballot(hasA), mB = __ballot(hasB);
		const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mA >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mA, 0u))
			+ __builtin_amdgcn_mbcnt_hi((uint32_t)(mB >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mB, 0u));
		uint32_t *wp = end - (ncig + below + 1u);
		if(hasA){ *wp = tokN << 4; wp--; }                // (tokN: already without the key's op field)
		if(hasB) *wp = ((tokB >> 2) << 4) | (tokB & 3u);
		ncig += (uint32_t)(__popcll(mA) + __popcll(mB));
	}
	__device__ __forceinline__ void emit(uint32_t op, uint32_t len){
		if(op == 0u){ key += len; return; }
		if(key == (op << 28)){ if(lane + 1u == ntok) tokB += len << 2; return; }
		if(ntok == 64u){
			flush(63u);
			tokN = (uint32_t)__builtin_amdgcn_readlane((int)tokN, 63); tokB = (uint32_t)__builtin_amdgcn_readlane((int)tokB, 63);
			ntok = 1u;
		}
		if(lane == ntok){ tokN = key; tokB = (len << 2) | op; }       // (the op field of the key is masked off when the token is written)
		ntok++; key = op << 28;
	}
	__device__ __forceinline__ void finish(){                        // the matches behind the last event, then everything out
		if(key & KEYM){
			if(ntok == 64u){ flush(64u); ntok = 0u; }
			if(lane == ntok){ tokN = key; tokB = 0u; }
			ntok++; key = 0u;
		}
		flush(ntok); ntok = 0u;
	}
};
// the sum of the lanes' values (uniform): the mismatches of a walk per wave are counted by the lanes
static __device__ __forceinline__ int bsa_wave_sum(uint32_t t){
	t += (uint32_t)__shfl_xor((int)t, 32); t += (uint32_t)__shfl_xor((int)t, 16); t += (uint32_t)__shfl_xor((int)t, 8);
	t += (uint32_t)__shfl_xor((int)t, 4); t += (uint32_t)__shfl_xor((int)t, 2); t += (uint32_t)__shfl_xor((int)t, 1);
	return __builtin_amdgcn_readfirstlane((int)t);
}

// ---- 8 bases of a sequence in a register window: a walk that moves down a sequence touches memory once per 8 steps (the staged sequences are padded)
struct bsa_base_win_t {
	const uint8_t *seq; uint64_t win; int wb;
	__device__ __forceinline__ bsa_base_win_t(const uint8_t *s) : seq(s), win(0), wb(-1000) {}
	__device__ __forceinline__ int at(int idx){
		if(idx < wb || idx >= wb + 8){ wb = max(idx - 7, 0); __builtin_memcpy(&win, seq + wb, 8); }
		return (int)((win >> (8 * (idx - wb))) & 0xffu);
	}
};

// ---- what is left at the top of a global / extend walk becomes a leading I / D (bsalign.h:3827-3842); sz 0: nothing is left
static __device__ __forceinline__ void bsa_walk_lead(bsa_result_t &rs, uint32_t &op, uint32_t &sz){
	op = 0; sz = 0;
	if(rs.qb >= 0){ op = 1; sz = (uint32_t)rs.qb + 1u; rs.ins += (int)sz; rs.qb = -1; }
	else if(rs.tb >= 0){ op = 2; sz = (uint32_t)rs.tb + 1u; rs.del += (int)sz; rs.tb = -1; }
}
// End of a walk, a pair per lane; cg: the run still open.  Overlap stops where the walk left the matrix (bsalign.h:3822-3826), global / extend add the
// leading gap.  A bad walk is flagged BSA_ST_TRACE and drops its words; the walkers over codes also zero its record (zero), the literal ones
// (bsa_align8.hip) leave score and end cell in it.  Lanes whose writer does not store (cig.wr) leave everything to the one that does.
static __device__ __forceinline__ void bsa_walk_end_lane(uint32_t *status, uint32_t pair, uint32_t ppos, int type, bool bad, uint32_t cg, bsa_cig_lane_t &cig,
		bsa_result_t &rs, bsa_result_t *out, uint32_t *cig_cnt, bool zero = true){
	if(!bad){
		if(type == BSA_MODE_OVERLAP){ if(cg) cig.push(cg); }
		else {
			uint32_t op, sz;
			bsa_walk_lead(rs, op, sz);
			rs.aln += (int)sz;
			cg = cig.add(cg, op, sz);
			if(cg) cig.push(cg);
		}
		rs.qb++; rs.tb++;
	}
	if(bad){
		if(cig.wr) atomicOr(&status[pair], BSA_ST_TRACE);
		if(zero) bsa_result_zero(rs, false);
		cig.n = 0;
	}
	if(cig.wr){ out[pair] = rs; cig_cnt[ppos] = cig.n; }
}

// ================================================================================================================================================
// Walkers over code slots (bsa_align8_codes.hip)
// ================================================================================================================================================

// end cell of the non-global modes from the forward pass's end record (bsa_common.h bsa_code_end_t): the best
// end-of-query candidate (strictly greater wins, in row order) against the maximum of the last row, whose tie rules are
// the reference's: per lane the first best 32-vector chunk, lanes reduced in its register order, then the first
// maximum inside the winning chunk (bsalign.h:3213-3329).
// ref_bw != 0 (a whole-query band run at a wider register-kernel width, bsa_api.hip): the row maximum is taken over the
// REFERENCE's band -- ref_bw columns, or roundup(qlen, 16) when ref_bw == 1 -- in the reference's striping of it (WR cells per
// lane), whose tie rules depend on that striping; the end record is in natural order, so only the lane boundaries move.
// `er`: the end record (the spare rows of a code slot, or the whole slot of a score-only pair: k_align8_score_finish)
template<int WK>
static __device__ void codes_end_cell(const bsa_code_end_t *er, uint32_t qlen, uint32_t tlen, uint32_t ref_bw, int &score, int &qe, int &te){
	const int8_t *us = (const int8_t*)(er + 1);           // natural band order: lane l, cell x at l * W + x
	const uint32_t W = ref_bw == 0u ? (uint32_t)WK : ref_bw == 1u ? (max(qlen, 1u) + 15u) / 16u : ref_bw / 16u;
	// H in front of band position p, from the kernel's own 16 block starts
	auto before = [&](uint32_t p) -> int { const uint32_t b = p / (uint32_t)WK; int h = er->ubegs[b]; for(uint32_t i = b * (uint32_t)WK; i < p; i++) h += us[i]; return h; };
	int best = BSA_SCORE_MIN, bte = 0;
	for(int l = 0; l < 16; l++){
		const int sc = er->cand_sc[l], t = er->cand_te[l];
		if(sc > best || (sc == best && sc != BSA_SCORE_MIN && t < bte)){ best = sc; bte = t; }
	}
	int lmax[16]; uint32_t lchunk[16];
	for(uint32_t l = 0; l < 16; l++){
		int base = (W == (uint32_t)WK) ? er->ubegs[l] : before(l * W);
		lmax[l] = BSA_SCORE_MIN; lchunk[l] = 0;
		for(uint32_t i = 0, c = 0; i < (uint32_t)W; i += 32, c++){
			const uint32_t n = (i + 32 < (uint32_t)W) ? 32 : (uint32_t)W - i;
			int run = 0, cmax = -32767;
			for(uint32_t x = 0; x < n; x++){
				run += us[l * W + i + x];
				run = min(max(run, -32768), 32767);
				cmax = max(cmax, run);
			}
			if(base + cmax > lmax[l]){ lmax[l] = base + cmax; lchunk[l] = c; }
			base += run;
		}
	}
	int ms, lane;
	{
		int mm[4], ii[4];
		for(int k = 0; k < 4; k++){
			int m01, i01, m23, i23;
			if(lmax[4 + k] > lmax[k]){ m01 = lmax[4 + k]; i01 = 4 + k; } else { m01 = lmax[k]; i01 = k; }
			if(lmax[12 + k] > lmax[8 + k]){ m23 = lmax[12 + k]; i23 = 12 + k; } else { m23 = lmax[8 + k]; i23 = 8 + k; }
			if(m23 > m01){ mm[k] = m23; ii[k] = i23; } else { mm[k] = m01; ii[k] = i01; }
		}
		ms = mm[0]; lane = ii[0];
		for(int k = 1; k < 4; k++) if(mm[k] > ms){ ms = mm[k]; lane = ii[k]; }
	}
	uint32_t x = lchunk[lane] * 32u, jj = x;
	const uint32_t y = min(x + 32u, (uint32_t)W);
	int umax = BSA_SCORE_MIN, uscr = 0;
	for(; x < y; x++){
		uscr += us[lane * W + x];
		if(uscr > umax){ jj = x; umax = uscr; }
	}
	if(ms > best){ score = ms; qe = er->rbeg_last + (int)((uint32_t)lane * W + jj); te = (int)tlen - 1; }
	else { score = best; qe = (int)qlen - 1; te = bte; }
}
template<int WK>
static __device__ void codes_end_cell(const uint8_t *rows, uint32_t RB, uint32_t qlen, uint32_t tlen, uint32_t ref_bw, int &score, int &qe, int &te){
	codes_end_cell<WK>((const bsa_code_end_t*)(rows + (size_t)bsa_code_rows(tlen) * RB), qlen, tlen, ref_bw, score, qe, te);
}

// code slot (bsa_common.h "COMPACT slot") of pair = a.order[ppos] at processing position ppos, RB bytes a code row: the band offsets, the code rows, the end of the
// CIGAR scratch behind the spare rows
struct bsa_code_slot_t {
	uint32_t pair, qlen, tlen;
	const uint8_t *qseq, *tseq;
	const int *begs; const uint8_t *rows; uint32_t *cig_end;
	__device__ __forceinline__ bsa_code_slot_t(const Align8Args &a, uint32_t ppos, uint32_t pair_, uint32_t RB){
		pair = pair_;
		qlen = a.qlen[pair]; tlen = a.tlen[pair];
		qseq = a.qst + a.qpoff[pair];
		tseq = a.tst + a.tpoff[pair];
		begs = (const int*)(a.rows + a.slot_off[ppos]);
		rows = (const uint8_t*)begs + bsa_begs_bytes(tlen);
		cig_end = (uint32_t*)(rows + ((size_t)bsa_code_rows(tlen) + BSA_CODE_SPARE_ROWS) * RB);
	}
};

// Start of a walk over codes: score and end cell by mode (type = a.mode & 3) into rs.score, rs.qe, rs.te -- global: the last cell, with 0x80000000 as the score where the
// band never reached the query end (bsalign.h:4034); overlap / extend: the best end cell (bsalign.h:4023-4046).  Returns `bad`: no score, or the end
// cell outside the stored band (lastbeg: the band offset of its row).
// Lane form: every lane its own pair; also steps rs.qb / rs.tb onto the end cell and rs.qe / rs.te behind it.
template<int W>
static __device__ __forceinline__ bool bsa_walk_start_lane(const Align8Args &a, const bsa_code_slot_t &s, uint32_t RB, int type, bsa_result_t &rs, int &lastbeg){
	bool bad = false;
	if(type == BSA_MODE_GLOBAL){
		rs.score = s.begs[s.tlen + 1];
		if(rs.score == (int)0x80000000u) bad = true;
		rs.qe = (int)s.qlen - 1; rs.te = (int)s.tlen - 1;
	} else codes_end_cell<W>(s.rows, RB, s.qlen, s.tlen, a.ref_bw, rs.score, rs.qe, rs.te);
	lastbeg = s.begs[rs.te + 1];
	if(rs.qe < lastbeg || rs.qe >= lastbeg + W * 16) bad = true;
	rs.qb = rs.qe; rs.qe++;
	rs.tb = rs.te; rs.te++;
	return bad;
}
// Wave form: the wave's one pair, results uniform.  LANE0 false: every lane works the end cell out and the first lane's values are taken
// (k_align8_trace_codes_wave); true: one lane does and broadcasts (k_align8_trace_codes2_wave).
template<int W, bool LANE0>
static __device__ __forceinline__ bool bsa_walk_start_wave(const Align8Args &a, const bsa_code_slot_t &s, uint32_t RB, int type, uint32_t lane, bsa_result_t &rs){
	bool bad = false;
	if(type == BSA_MODE_GLOBAL){
		rs.score = s.begs[s.tlen + 1];
		if(rs.score == (int)0x80000000u) bad = true;
		rs.qe = (int)s.qlen - 1; rs.te = (int)s.tlen - 1;
	} else if constexpr (LANE0){
		int sc = 0, qe = 0, te = 0;
		if(lane == 0) codes_end_cell<W>(s.rows, RB, s.qlen, s.tlen, a.ref_bw, sc, qe, te);
		rs.score = __shfl(sc, 0); rs.qe = __shfl(qe, 0); rs.te = __shfl(te, 0);
	} else codes_end_cell<W>(s.rows, RB, s.qlen, s.tlen, a.ref_bw, rs.score, rs.qe, rs.te);
	if constexpr (!LANE0){
		rs.score = __builtin_amdgcn_readfirstlane(rs.score); rs.qe = __builtin_amdgcn_readfirstlane(rs.qe); rs.te = __builtin_amdgcn_readfirstlane(rs.te);
	}
	const int lb = s.begs[rs.te + 1];
	if(rs.qe < lb || rs.qe >= lb + W * 16) bad = true;
	return bad;
}

// A deletion run that reached row -1.  With linear gaps that is an ordinary move while the column lies in row -1's band (qb < bw); with affine gaps
// only the e = -63 sentinel of row -1 leads there and the reference then compares real scores: the literal path (BSA_ST_TRACE, hand-over).  With
// two-piece gaps it is always the literal path (k_align8_trace_codes2, _codes2_wave).
static __device__ __forceinline__ bool bsa_drun_top_bad(bool lin, int qb, int bw){ return !lin || qb >= bw; }

// End of a walk per wave that stopped at (x, y) after starting at (x_start, y_start): rs.ins holds the inserted columns of the walk, the other totals
// follow from its two ends, the mismatches from the lanes' counts (vmis); then the leading gap, the words, and lane 0 stores.
static __device__ __forceinline__ void bsa_walk_end_wave(uint32_t *status, const bsa_code_slot_t &s, uint32_t ppos, int type, bool bad, int x, int y, int x_start, int y_start,
		uint32_t vmis, bsa_cig_wave_t &cig, bsa_result_t &rs, bsa_result_t *out, uint32_t *cig_cnt){
	if(!bad){
		rs.qb = x; rs.tb = y;
		const int mcols = (x_start - x) - rs.ins;
		rs.mis = bsa_wave_sum(vmis); rs.mat = mcols - rs.mis;
		rs.del = (y_start - y) - mcols;
		if(type != BSA_MODE_OVERLAP){
			uint32_t op, sz;
			bsa_walk_lead(rs, op, sz);
			if(sz) cig.emit(op, sz);
		}
		cig.finish();
		rs.qb++; rs.tb++;
		rs.aln = rs.mat + rs.mis + rs.ins + rs.del;
	} else {
		if(cig.lane == 0) atomicOr(&status[s.pair], BSA_ST_TRACE);
		bsa_result_zero(rs, false);
		cig.ncig = 0;
	}
	if(cig.lane == 0){ out[s.pair] = rs; cig_cnt[ppos] = cig.ncig; }
}
