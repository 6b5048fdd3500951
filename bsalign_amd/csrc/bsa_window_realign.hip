// bsa_window_realign.hip -- bsa_window_realign_run / _batch (include/bsalign_hip.h): every piece of a window aligned again, against the sequence
// bsa_window_stitch_run called for that window, and the result in the shape bsa_window_msa_run takes for a second round: piece records, guides whose
// first and last word are diagonal, and the called sequence as the per-window draft.
//
// A pass over public outputs: the piece records and codes of bsa_window_pieces_run (or bsa_window_select_run) and the sequence and = / X / I / D
// words of bsa_window_stitch_run.  It touches no plan and no other pass.  The steps on the context stream:
//   init : a thread a piece of piece_cap (k_window_realign_init): BSA_REALIGN_ST_NO_WINDOW, which the pieces no liftable window claims keep;
//   lift : a wave a window (k_window_realign_lift) goes over the window's words in tiles of 64 and tests "liftable"; then, a lane a piece, every
//          piece walks the words once more -- the loads are the same address in all lanes -- for s(a) and s(b) + k(b), tests the clauses of
//          "re-alignable" and leaves 16 bytes: where its span T begins in d_seq, u, m, the margin and the status;
//   dp   : a wave a piece, a lane a diagonal (k_window_realign_dp): the codes and T staged into LDS with 16-byte loads, the DP row by row -- the
//          target steps inside a row are a min-plus prefix scan over the lanes, six DPP steps -- with two direction bits a cell kept in LDS, a lane's
//          16 rows a dword; the traceback walks that dword a run of diagonal steps at a time, leaves the path as 2 bits a step in the context's
//          scratch, counts what is trimmed and the words, and writes the piece's record, status and cost.  The DP of a piece runs once a run;
//   scan : bsa_scan.hip's exclusive scan of the word counts of all piece_cap pieces: d_pcig2_off;
//   fill : a wave a piece, four a block (k_window_realign_fill), turns the kept steps into words by ballot and prefix count.
// Scratch: 16 bytes and one count a piece, the scan's temporaries, and a path slot of (2 max_len + 63) steps a piece (a re-alignable piece has n + m
// <= 2 n + 63 steps), all sized on the host from piece_cap and max_len.  Plain C++ with DPP moves; no kernel uses scratch memory.
#include "bsa_pass.h"
#include "bsa_dpp.h"

static_assert(sizeof(bsa_piece_t) == 32 && sizeof(bsa_realign_params_t) == 32, "the records' layouts");

#define WR_INF (1 << 28)           // an unreachable cell: above (2048 + 2111) * 255, and 64 * 255 can be added to it
#define WR_TPAD 64u                // bytes in front of T in LDS: lane 0 of row 1 reads T[dlo - 1], dlo >= -63

// what the lift leaves for the DP, and -- in the same 16 bytes -- what the DP leaves for the fill
struct wr_info_t { uint64_t toff; uint32_t um, sm; };        // T = seq[toff .. toff + m); u | m << 16; status | margin << 8
struct wr_path_t { uint32_t steps, lead, kept, cnt; };        // all steps of the path, the trimmed ones in front, the kept ones, their words
static_assert(sizeof(wr_info_t) == 16 && sizeof(wr_path_t) == 16, "16 bytes of scratch a piece");
enum { WR_LIFT = 1, WR_DP = 2, WR_SCAN = 4, WR_FILL = 8 };

static inline uint32_t wr_slot_dwords(uint32_t max_len){ return (2u * max_len + 63u + 15u) / 16u; }
// the DP kernel's LDS: the direction dwords of 16 rows by 64 lanes, T behind its pad and its shift, the codes behind their shift
static inline uint32_t wr_dir_bytes(uint32_t max_len){ return (max_len / 16u + 1u) * 256u; }
static inline uint32_t wr_t_bytes(uint32_t max_len){ return (WR_TPAD + 16u + max_len + 63u + 64u + 15u) & ~15u; }
static inline uint32_t wr_q_bytes(uint32_t max_len){ return (16u + max_len + 15u) & ~15u; }

__global__ void __launch_bounds__(256) k_window_realign_init(uint32_t piece_cap, wr_info_t *info){
	const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if(j < piece_cap){ const wr_info_t r = { 0ull, 0u, BSA_REALIGN_ST_NO_WINDOW }; info[j] = r; }
}

static __device__ __forceinline__ uint64_t wr_wave_sum(uint64_t v){
#pragma unroll
	for(int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// a wave a window, one a block: everything the block decides on is the same in all lanes
__global__ void __launch_bounds__(64) k_window_realign_lift(uint32_t nwin, const bsa_piece_t *piece, const uint64_t *piece_off, uint32_t piece_cap, uint64_t bases_cap,
		uint32_t window, const uint64_t *seq_off, uint64_t seq_cap, const uint32_t *cig, const uint64_t *cig_off, uint64_t cig_cap, bsa_realign_params_t par,
		wr_info_t *info, uint64_t *doff2, uint32_t *dlen2){
	const uint32_t lane = threadIdx.x;
	for(uint32_t g = blockIdx.x; g < nwin; g += gridDim.x){
		const uint64_t s0 = seq_off[g], s1 = seq_off[g + 1u], c0 = cig_off[g], c1 = cig_off[g + 1u];
		bool ok = s0 <= s1 && s1 <= seq_cap && s1 - s0 <= par.window2 && c0 <= c1 && c1 <= cig_cap;
		const uint64_t nw = ok ? c1 - c0 : 0ull;
		const uint32_t slen = ok ? (uint32_t)(s1 - s0) : 0u;
		uint64_t qs = 0, ts = 0;
		for(uint64_t w0 = 0; w0 < nw && ok; w0 += 64u){
			const bool has = w0 + lane < nw;
			const uint32_t word = has ? cig[c0 + w0 + lane] : 0u, op = word & 15u, len = word >> 4;
			const bool good = !has || ((op == BSA_CIGAR_I || op == BSA_CIGAR_D || op == BSA_CIGAR_EQ || op == BSA_CIGAR_X) && len != 0u);
			qs += wr_wave_sum(has && good && op != BSA_CIGAR_D ? len : 0u);
			ts += wr_wave_sum(has && good && op != BSA_CIGAR_I ? len : 0u);
			if(__ballot(!good) != 0ull || qs > slen || ts > window) ok = false;      // (the sums only grow: a window of very many words ends here)
		}
		ok = ok && qs == slen;
		const uint32_t Ld = (uint32_t)ts;
		if(lane == 0u){ doff2[g] = ok ? s0 : 0ull; dlen2[g] = ok ? slen : 0u; }
		const uint64_t x0 = piece_off[g], x1 = piece_off[g + 1u];
		if(!ok || !(x0 <= x1 && x1 <= piece_cap)) continue;
		for(uint64_t j0 = x0; j0 < x1; j0 += 64u){
			const uint64_t j = j0 + lane;
			const bool mine = j < x1;
			bsa_piece_t pc = { 0u, 0u, 0u, 0u, 0u, 0u, 0ull };
			if(mine) pc = piece[j];
			const uint32_t n = pc.len, a = pc.t_first % window;
			const uint64_t b = (uint64_t)a + (uint64_t)(pc.t_last - pc.t_first);
			uint32_t st = BSA_REALIGN_ST_OK;
			if(n == 0u) st = BSA_REALIGN_ST_BAD_PIECE;
			else if(n > par.max_len) st = BSA_REALIGN_ST_TOO_LONG;
			else if(pc.base_off > bases_cap || bases_cap - pc.base_off < n || pc.t_last < pc.t_first || b >= Ld) st = BSA_REALIGN_ST_BAD_PIECE;
			// s(a) and s(b) + k(b): one walk over the words, the same word in every lane
			uint32_t t = 0, s = 0, u = 0, e = 0;
			const bool look = mine && st == BSA_REALIGN_ST_OK;
			for(uint64_t w = 0; w < nw; w++){
				const uint32_t word = cig[c0 + w], op = word & 15u, len = word >> 4;
				if(op == BSA_CIGAR_I){ s += len; continue; }
				const uint32_t k = op == BSA_CIGAR_D ? 0u : 1u;
				if(look && a >= t && a - t < len) u = s + k * (a - t);
				if(look && (uint32_t)b >= t && (uint32_t)b - t < len) e = s + k * ((uint32_t)b - t + 1u);      // (e = v + 1)
				t += len; s += k * len;
			}
			if(!mine) continue;
			uint32_t m = 0, margin = 0;
			if(st == BSA_REALIGN_ST_OK){
				m = e - u;                                              // (s never decreases: e >= u)
				const uint32_t d = m > n ? m - n : n - m;
				margin = d <= 63u ? (63u - d) / 2u : 0u;
				if(m == 0u) st = BSA_REALIGN_ST_EMPTY_SPAN;
				else if(d > 63u || margin < par.min_margin) st = BSA_REALIGN_ST_OFF_BAND;
			}
			const wr_info_t r = { s0 + u, u | m << 16, st | margin << 8 };
			info[j] = r;
		}
	}
}

// n bytes into LDS where dst and src are congruent modulo 16: 16-byte vectors over the aligned middle, single bytes in front and behind, so that
// every vector lies inside the n bytes
static __device__ __forceinline__ void wr_stage(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane){
	uint32_t head = (uint32_t)((0u - (uintptr_t)src) & 15u);
	if(head > n) head = n;
	const uint32_t nv = (n - head) / 16u, tail = head + nv * 16u;
	if(lane < head) dst[lane] = src[lane];
	for(uint32_t i = lane; i < nv; i += 64u) ((uint4*)(dst + head))[i] = ((const uint4*)(src + head))[i];
	if(tail + lane < n) dst[tail + lane] = src[tail + lane];
}

// the inclusive prefix minimum over the 64 lanes: row shifts by 1, 2, 4, 8, then the two row broadcasts, the DPP operand folded into v_min_i32 (a
// lane without a source keeps its value).  A DPP read of a register the instruction in front wrote needs two wait states, and inline assembly is
// not seen by the compiler's hazard recogniser.
static __device__ __forceinline__ int wr_scan_min(int v){
	asm volatile(
		"s_nop 1\n\t"
		"v_min_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
		"s_nop 1\n\t"
		"v_min_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
		"s_nop 1\n\t"
		"v_min_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
		"s_nop 1\n\t"
		"v_min_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
		"s_nop 1\n\t"
		"v_min_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
		"s_nop 1\n\t"
		"v_min_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
		"s_nop 1"
		: "+v"(v));
	return v;
}
// lane l <- lane l + 1 (lane 63 keeps `fill`), and lane l <- lane l - 1 (lane 0 keeps `fill`): DPP wave shifts
static __device__ __forceinline__ int wr_from_above(int fill, int x){ return dpp_keep(__builtin_amdgcn_update_dpp(fill, x, 0x130, 0xf, 0xf, false)); }
static __device__ __forceinline__ int wr_from_below(int fill, int x){ return dpp_keep(__builtin_amdgcn_update_dpp(fill, x, 0x138, 0xf, 0xf, false)); }

// a wave a piece, one a block.  Lane l is diagonal dlo + l: in row i it holds cell jt = i + dlo + l.  The diagonal step comes from the lane's own
// value of the row above, the query step (I) from lane l + 1 of the row above, the target step (D) from lane l - 1 of the same row.  A cell's
// direction is the first that explains its value -- diagonal (0), then D (BSA_CIGAR_D), then I (BSA_CIGAR_I) -- and the directions of a lane's
// rows 16 k .. 16 k + 15 are the dword dirs[64 k + l], row i at bits 2 (i % 16).
__global__ void __launch_bounds__(64) k_window_realign_dp(uint32_t piece_cap, const bsa_piece_t *piece, const uint8_t *bases, const uint8_t *seq, bsa_realign_params_t par,
		wr_info_t *info, uint32_t *path, uint32_t slot, bsa_piece_t *piece2, uint32_t *pstatus, uint32_t *cost, uint32_t *cnt){
	extern __shared__ uint4 wr_lds[];
	const uint32_t lane = threadIdx.x;
	uint32_t *dirs = (uint32_t*)wr_lds;
	uint8_t *tbuf = (uint8_t*)wr_lds + (par.max_len / 16u + 1u) * 256u;
	uint8_t *qbuf = tbuf + ((WR_TPAD + 16u + par.max_len + 63u + 64u + 15u) & ~15u);
	const int gap = (int)par.g, mis = (int)par.x, lg = (int)lane * gap;
	for(uint32_t j = blockIdx.x; j < piece_cap; j += gridDim.x){
		const wr_info_t in = info[j];
		bsa_piece_t pc = piece[j];
		const uint32_t um = (uint32_t)__builtin_amdgcn_readfirstlane((int)in.um), sm = (uint32_t)__builtin_amdgcn_readfirstlane((int)in.sm);      // (the same in all lanes)
		uint32_t st = sm & 0xFFu;
		wr_path_t out = { 0u, 0u, 0u, 0u };
		uint32_t value = 0;
		if(st == BSA_REALIGN_ST_OK){
			const int n = __builtin_amdgcn_readfirstlane((int)pc.len), m = (int)(um >> 16), margin = (int)(sm >> 8);
			const uint32_t u = um & 0xFFFFu;
			const uint8_t *qsrc = bases + pc.base_off, *tsrc = seq + in.toff;
			uint8_t *ql = qbuf + ((uintptr_t)qsrc & 15u), *tl = tbuf + WR_TPAD + ((uintptr_t)tsrc & 15u);
			__syncthreads();                                         // (the walk of the piece in front is done with the LDS)
			wr_stage(ql, qsrc, (uint32_t)n, lane);
			wr_stage(tl, tsrc, (uint32_t)m, lane);
			__syncthreads();
			const int dlo = (m < n ? m - n : 0) - margin;
			int jt = dlo + (int)lane;
			int H = (jt >= 0 && jt <= m) ? jt * gap : WR_INF;
			uint32_t acc = jt > 0 ? (uint32_t)BSA_CIGAR_D : (uint32_t)BSA_CIGAR_I;      // row 0: target steps only; the origin ends every run of diagonal steps
			const uint8_t *tp = tl + dlo + (int)lane - 1;            // T[jt - 1] of row i is tp[i]
			uint32_t tc = tp[1];
			for(int i = 1; i <= n; i++){
				jt++;
				const uint32_t qc = ql[i - 1], tnext = tp[i + 1];
				const bool valid = (uint32_t)jt <= (uint32_t)m;
				const int dg = H + (((qc ^ tc) & 3u) ? mis : 0);
				const int up = wr_from_above(WR_INF, H) + gap;
				int c = dg < up ? dg : up;
				c = valid ? c : WR_INF;
				int Hn = wr_scan_min(c - lg) + lg;
				Hn = valid ? Hn : WR_INF;
				const int left = wr_from_below(WR_INF, Hn) + gap;
				const uint32_t dir = dg == Hn ? 0u : left == Hn ? (uint32_t)BSA_CIGAR_D : (uint32_t)BSA_CIGAR_I;
				if((i & 15) == 0){ dirs[(uint32_t)((i - 1) >> 4) * 64u + lane] = acc; acc = 0u; }
				acc |= dir << (2 * (i & 15));
				H = Hn; tc = tnext;
			}
			dirs[(uint32_t)(n >> 4) * 64u + lane] = acc;
			value = (uint32_t)__builtin_amdgcn_readlane(H, m - n - dlo);
			__syncthreads();
			// the walk from (n, m) to (0, 0): every value is the same in all lanes
			uint32_t *mine = path + (size_t)j * slot;
			int i = n, l = m - n - dlo;
			uint32_t pos = 0, pw = 0, tI = 0, tD = 0, lI = 0, lD = 0, runs = 0, runs_at_diag = 0, prev = 0;
			bool seen = false, edge = false;
			while(true){
				edge = edge || l == 0 || l == 63;
				if((i == 0 && i + dlo + l == 0) || pos >= (uint32_t)(n + m)) break;      // (a path has at most n + m steps: the slot is never left)
				const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)dirs[(uint32_t)(i >> 4) * 64u + (uint32_t)l]);
				const uint32_t r = (uint32_t)i & 15u, top = d << (2u * (15u - r));      // row i at bits 31:30, the rows below it in this dword behind it
				uint32_t k = top ? (uint32_t)__clz((int)top) / 2u : 16u;               // the diagonal steps in front of the first other step
				if(k > r + 1u) k = r + 1u;
				if(k > (uint32_t)(n + m) - pos) k = (uint32_t)(n + m) - pos;
				if(k){
					if(!seen){ seen = true; runs = 1u; } else if(prev != 0u) runs++;
					prev = 0u; runs_at_diag = runs; lI = 0u; lD = 0u;
					i -= (int)k;
					while(k){                                       // k steps of 00
						const uint32_t room = 16u - (pos & 15u), take = k < room ? k : room;
						pos += take; k -= take;
						if((pos & 15u) == 0u){ if(lane == 0u) mine[(pos >> 4) - 1u] = pw; pw = 0u; }
					}
					continue;
				}
				const uint32_t op = top >> 30;
				if(!seen){ if(op == BSA_CIGAR_I) tI++; else tD++; }
				else { if(prev != op) runs++; prev = op; if(op == BSA_CIGAR_I) lI++; else lD++; }
				if(op == BSA_CIGAR_I){ i--; l++; } else l--;
				pw |= op << (2u * (pos & 15u));
				pos++;
				if((pos & 15u) == 0u){ if(lane == 0u) mine[(pos >> 4) - 1u] = pw; pw = 0u; }
			}
			if((pos & 15u) != 0u && lane == 0u) mine[pos >> 4] = pw;
			if(seen){
				st = edge ? BSA_REALIGN_ST_EDGE : BSA_REALIGN_ST_OK;
				out.steps = pos; out.lead = lI + lD; out.kept = pos - lI - lD - tI - tD; out.cnt = runs_at_diag;
				pc.q_first += lI; pc.base_off += lI; pc.len -= lI + tI;
				pc.t_first = u + lD; pc.t_last = u + (uint32_t)m - 1u - tD; pc.reserved = 0u;
			} else st = BSA_REALIGN_ST_NO_DIAG;
		}
		if((st & 0xFFu) != BSA_REALIGN_ST_OK) pc.len = 0u;
		if(lane == 0u){
			piece2[j] = pc; pstatus[j] = st; cnt[j] = out.cnt;
			if(cost) cost[j] = value;
			*(wr_path_t*)(info + j) = out;
		}
	}
}

// a wave a piece, four a block: the kept steps of the path, 64 a trip, to maximal runs.  Forward step f is the path's step steps - 1 - f (the walk
// wrote them from the end).  A piece is written whole or not at all: when its range ends inside the arena.
__global__ void __launch_bounds__(256) k_window_realign_fill(uint32_t piece_cap, const wr_info_t *info, const uint32_t *path, uint32_t slot, const uint64_t *off, uint32_t *pcig,
		uint64_t cap){
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t lt = (1ull << lane) - 1ull;
	for(uint64_t j = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); j < piece_cap; j += (uint64_t)gridDim.x * 4u){
		const wr_path_t p = *(const wr_path_t*)(info + j);
		const uint64_t o0 = off[j], o1 = off[j + 1u];
		if(p.cnt == 0u || o1 > cap || o1 - o0 != (uint64_t)p.cnt) continue;      // (the offsets are this pass's own scan of the same counts)
		const uint32_t *mine = path + (size_t)j * slot;
		uint64_t cp = o0;                                              // where the next run's word goes
		uint32_t open = 0, open_len = 0;                               // the run the tiles in front left open: its kind (op + 1; 0: none) and steps
		for(uint32_t f0 = 0; f0 < p.kept; f0 += 64u){
			const uint32_t n = p.kept - f0 < 64u ? p.kept - f0 : 64u;
			uint32_t kind = 0;
			if(lane < n){ const uint32_t r = p.steps - 1u - (p.lead + f0 + lane); kind = ((mine[r >> 4] >> (2u * (r & 15u))) & 3u) + 1u; }
			const uint32_t below = (uint32_t)__shfl_up((int)kind, 1);
			const bool start = lane < n && kind != (lane ? below : open);
			const uint64_t S = __ballot(start);
			if(S){
				const uint32_t first = (uint32_t)__ffsll((long long)S) - 1u;          // the steps in front of the tile's first start end the open run
				if(open && lane == 0u && cp - 1u < o1) pcig[cp - 1u] = (open_len + first) << 4 | (open - 1u);
				const uint64_t above = S & ~((2ull << lane) - 1ull);
				const uint32_t next = above ? (uint32_t)__ffsll((long long)above) - 1u : n;
				const uint64_t at = cp + (uint32_t)__popcll(S & lt);
				if(start && above && at < o1) pcig[at] = (next - lane) << 4 | (kind - 1u);      // every start but the last ends at the next start
				const int last = 63 - __clzll((long long)S);
				open = (uint32_t)__shfl((int)kind, last);
				open_len = n - (uint32_t)last;
				cp += (uint32_t)__popcll(S);
			} else open_len += n;
		}
		if(open && lane == 0u && cp - 1u < o1) pcig[cp - 1u] = open_len << 4 | (open - 1u);
	}
}

// the argument errors of both calls
static int wr_check(bsa_ctx_t *ctx, const void *piece, const void *piece_off, size_t nwin, size_t piece_cap, const void *bases, size_t bases_cap, uint32_t window, const void *seq,
		size_t seq_cap, const void *seq_off, const void *cig, size_t cig_cap, const void *cig_off, const bsa_realign_params_t *par, const void *piece2, const void *pcig2,
		size_t pcig2_cap, const void *pcig2_off, const void *pstatus, const void *doff2, const void *dlen2){
	const char *msg = nullptr;
	int rc = BSA_E_ARG;
	if(!par || !pcig2_off || (nwin && (!piece_off || !seq_off || !cig_off || !doff2 || !dlen2)) || (piece_cap && (!piece || !piece2 || !pstatus))
			|| (bases_cap && !bases) || (seq_cap && !seq) || (cig_cap && !cig) || (pcig2_cap && !pcig2)) msg = "bsa_window_realign: null argument";
	else if(window == 0u || par->window2 == 0u || par->max_len == 0u || par->x == 0u || par->g == 0u || par->x > 255u || par->g > 255u || par->min_margin > 31u
			|| par->reserved[0] || par->reserved[1] || par->reserved[2]) msg = "bsa_window_realign: window, window2, max_len, x, g in 1 .. and x, g <= 255, min_margin <= 31, reserved 0";
	else if(nwin > 0xFFFFFFF0ull || piece_cap > 0xFFFFFFF0ull || pcig2_cap > 0xFFFFFFF0ull) msg = "bsa_window_realign: too many windows, pieces or words";
	else if(par->window2 > 4096u || par->max_len > 2048u){ msg = "bsa_window_realign: window2 above 4096 or max_len above 2048"; rc = BSA_E_UNSUPPORTED; }
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return rc; }
	return BSA_OK;
}

struct wr_args_t {
	const bsa_piece_t *piece; const uint64_t *piece_off; size_t nwin, piece_cap; const uint8_t *bases; size_t bases_cap; uint32_t window;
	const uint8_t *seq; size_t seq_cap; const uint64_t *seq_off; const uint32_t *cig; size_t cig_cap; const uint64_t *cig_off; bsa_realign_params_t par;
	bsa_piece_t *piece2; uint32_t *pcig2; size_t pcig2_cap; uint64_t *pcig2_off; uint32_t *pstatus, *cost; uint64_t *doff2; uint32_t *dlen2;
};

// the steps of `steps`, in order (one alone only for tools/bench_window_realign.py and for _batch's fill, on the scratch a whole run left)
static int wr_run(bsa_ctx_t *ctx, hipStream_t st, int steps, const wr_args_t &a){
	const size_t P = a.piece_cap;
	const uint32_t slot = wr_slot_dwords(a.par.max_len);
	const size_t o_info = 0, o_cnt = o_info + bsa_up256(P * sizeof(wr_info_t)), o_tmp = o_cnt + bsa_up256(P * 4u), o_path = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)P)),
		total = o_path + bsa_up256(P * (size_t)slot * 4u);
	void *bufv = nullptr;
	int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);              // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	wr_info_t *info = (wr_info_t*)(b + o_info);
	uint32_t *cnt = (uint32_t*)(b + o_cnt), *path = (uint32_t*)(b + o_path);
	uint64_t *tmp = (uint64_t*)(b + o_tmp);
	hipError_t e = hipSuccess;
	const size_t cus = (size_t)bsa_cus();
	if((steps & WR_LIFT) && P){
		hipLaunchKernelGGL(k_window_realign_init, dim3((uint32_t)((P + 255u) / 256u)), dim3(256), 0, st, (uint32_t)P, info);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & WR_LIFT) && a.nwin){                      // (without pieces too: the windows' drafts)
		hipLaunchKernelGGL(k_window_realign_lift, dim3((uint32_t)std::min<size_t>(a.nwin, cus * 64u)), dim3(64), 0, st, (uint32_t)a.nwin, a.piece, a.piece_off, (uint32_t)P,
			(uint64_t)a.bases_cap, a.window, a.seq_off, (uint64_t)a.seq_cap, a.cig, a.cig_off, (uint64_t)a.cig_cap, a.par, info, a.doff2, a.dlen2);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & WR_DP) && P){
		// a block is a wave with its own LDS: the waves a CU holds are what the LDS leaves (160 KB) up to 32
		const uint32_t lds = wr_dir_bytes(a.par.max_len) + wr_t_bytes(a.par.max_len) + wr_q_bytes(a.par.max_len);
		const size_t per_cu = std::min<size_t>(32u, std::max<size_t>(1u, ((size_t)160u << 10) / lds));
		hipLaunchKernelGGL(k_window_realign_dp, dim3((uint32_t)std::min<size_t>(P, cus * per_cu * 4u)), dim3(64), lds, st, (uint32_t)P, a.piece, a.bases, a.seq, a.par, info, path,
			slot, a.piece2, a.pstatus, a.cost, cnt);
		e = hipGetLastError();
	}
	if(e == hipSuccess && (steps & WR_SCAN)) e = bsa_launch_excl_scan(st, (const uint32_t*)cnt, a.pcig2_off, (uint32_t)P, nullptr, tmp);
	if(e == hipSuccess && (steps & WR_FILL) && P && a.pcig2_cap){
		const size_t want = (P + 3u) / 4u, most = cus * 16u;
		hipLaunchKernelGGL(k_window_realign_fill, dim3((uint32_t)(want < most ? want : most)), dim3(256), 0, st, (uint32_t)P, (const wr_info_t*)info, (const uint32_t*)path, slot,
			(const uint64_t*)a.pcig2_off, a.pcig2, (uint64_t)a.pcig2_cap);
		e = hipGetLastError();
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_realign: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

static int wr_run_checked(bsa_ctx_t *ctx, int steps, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const uint8_t *d_bases, size_t bases_cap,
		uint32_t window, const uint8_t *d_seq, size_t seq_cap, const uint64_t *d_seq_off, const uint32_t *d_cig, size_t cig_cap, const uint64_t *d_cig_off,
		const bsa_realign_params_t *par, bsa_piece_t *d_piece2, uint32_t *d_pcig2, size_t pcig2_cap, uint64_t *d_pcig2_off, uint32_t *d_pstatus, uint32_t *d_cost, uint64_t *d_doff2,
		uint32_t *d_dlen2){
	if(!ctx) return BSA_E_ARG;
	int rc = wr_check(ctx, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, window, d_seq, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, par, d_piece2, d_pcig2, pcig2_cap,
		d_pcig2_off, d_pstatus, d_doff2, d_dlen2);
	if(rc != BSA_OK) return rc;
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	const wr_args_t a = { d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, window, d_seq, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, *par, d_piece2, d_pcig2, pcig2_cap,
		d_pcig2_off, d_pstatus, d_cost, d_doff2, d_dlen2 };
	return wr_run(ctx, stream, steps, a);
}

extern "C" int bsa_window_realign_run(bsa_ctx_t *ctx, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const uint8_t *d_bases, size_t bases_cap,
		uint32_t window, const uint8_t *d_seq, size_t seq_cap, const uint64_t *d_seq_off, const uint32_t *d_cig, size_t cig_cap, const uint64_t *d_cig_off,
		const bsa_realign_params_t *par, bsa_piece_t *d_piece2, uint32_t *d_pcig2, size_t pcig2_cap, uint64_t *d_pcig2_off, uint32_t *d_pstatus, uint32_t *d_cost, uint64_t *d_doff2,
		uint32_t *d_dlen2){
	return wr_run_checked(ctx, WR_LIFT | WR_DP | WR_SCAN | WR_FILL, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, window, d_seq, seq_cap, d_seq_off, d_cig, cig_cap,
		d_cig_off, par, d_piece2, d_pcig2, pcig2_cap, d_pcig2_off, d_pstatus, d_cost, d_doff2, d_dlen2);
}

// for tools/bench_window_realign.py: one step alone (step: 0 the lift, 1 the DP, 2 the scan, 3 the fill), once more, with the arguments of the
// context's last bsa_window_realign_run and on the scratch it left: nothing else may have used the context in between, and the steps in order
// (the DP reads what the lift left and leaves what the fill reads in its place)
extern "C" int bsa_window_realign_step_internal(bsa_ctx_t *ctx, int step, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap,
		const uint8_t *d_bases, size_t bases_cap, uint32_t window, const uint8_t *d_seq, size_t seq_cap, const uint64_t *d_seq_off, const uint32_t *d_cig, size_t cig_cap,
		const uint64_t *d_cig_off, const bsa_realign_params_t *par, bsa_piece_t *d_piece2, uint32_t *d_pcig2, size_t pcig2_cap, uint64_t *d_pcig2_off, uint32_t *d_pstatus,
		uint32_t *d_cost, uint64_t *d_doff2, uint32_t *d_dlen2){
	if(step < 0 || step > 3) return BSA_E_ARG;
	return wr_run_checked(ctx, 1 << step, d_piece, d_piece_off, nwin, piece_cap, d_bases, bases_cap, window, d_seq, seq_cap, d_seq_off, d_cig, cig_cap, d_cig_off, par, d_piece2,
		d_pcig2, pcig2_cap, d_pcig2_off, d_pstatus, d_cost, d_doff2, d_dlen2);
}

extern "C" int bsa_window_realign_batch(bsa_ctx_t *ctx, const bsa_piece_t *piece, const uint64_t *piece_off, size_t nwin, size_t piece_cap, const uint8_t *bases, size_t bases_cap,
		uint32_t window, const uint8_t *seq, size_t seq_cap, const uint64_t *seq_off, const uint32_t *cig, size_t cig_cap, const uint64_t *cig_off, const bsa_realign_params_t *par,
		bsa_piece_t *piece2, uint32_t *pcig2, size_t pcig2_cap, uint64_t *pcig2_off, uint32_t *pstatus, uint32_t *cost, uint64_t *doff2, uint32_t *dlen2){
	if(!ctx) return BSA_E_ARG;
	int rc = wr_check(ctx, piece, piece_off, nwin, piece_cap, bases, bases_cap, window, seq, seq_cap, seq_off, cig, cig_cap, cig_off, par, piece2, pcig2, pcig2_cap, pcig2_off, pstatus,
		doff2, dlen2);
	if(rc != BSA_OK) return rc;
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	const size_t P = piece_cap;
	bsa_stage_t in(ctx, stream), res(ctx, stream);
	const size_t o_piece = in.part(P * sizeof(bsa_piece_t)), o_poff = in.part((nwin + 1u) * 8u), o_bases = in.part(bases_cap), o_seq = in.part(seq_cap), o_soff = in.part((nwin + 1u) * 8u),
		o_cig = in.part(cig_cap * 4u), o_coff = in.part((nwin + 1u) * 8u), o_p2 = in.part(P * sizeof(bsa_piece_t)), o_off2 = in.part((P + 1u) * 8u), o_st = in.part(P * 4u),
		o_cost = in.part(P * 4u), o_doff = in.part(nwin * 8u), o_dlen = in.part(nwin * 4u);
	if((rc = in.alloc("bsa_window_realign_batch: no device memory for the pieces, the sequences and the records")) != BSA_OK) return rc;
	if(!in.up(o_piece, piece, P * sizeof(bsa_piece_t)) || (nwin && (!in.up(o_poff, piece_off, (nwin + 1u) * 8u) || !in.up(o_soff, seq_off, (nwin + 1u) * 8u)
			|| !in.up(o_coff, cig_off, (nwin + 1u) * 8u))) || !in.up(o_bases, bases, bases_cap) || !in.up(o_seq, seq, seq_cap) || !in.up(o_cig, cig, cig_cap * 4u))
		return in.fail("bsa_window_realign_batch: upload failed");
	wr_args_t a = { in.at<bsa_piece_t>(o_piece), in.at<uint64_t>(o_poff), nwin, P, in.at<uint8_t>(o_bases), bases_cap, window, in.at<uint8_t>(o_seq), seq_cap, in.at<uint64_t>(o_soff),
		in.at<uint32_t>(o_cig), cig_cap, in.at<uint64_t>(o_coff), *par, in.at<bsa_piece_t>(o_p2), nullptr, 0, in.at<uint64_t>(o_off2), in.at<uint32_t>(o_st), in.at<uint32_t>(o_cost),
		in.at<uint64_t>(o_doff), in.at<uint32_t>(o_dlen) };
	if((rc = wr_run(ctx, stream, WR_LIFT | WR_DP | WR_SCAN, a)) != BSA_OK) return rc;
	if(!in.down(pcig2_off, o_off2, (P + 1u) * 8u) || !in.down(pstatus, o_st, P * 4u) || !in.down(piece2, o_p2, P * sizeof(bsa_piece_t)) || (cost && !in.down(cost, o_cost, P * 4u))
			|| !in.down(doff2, o_doff, nwin * 8u) || !in.down(dlen2, o_dlen, nwin * 4u) || !in.sync())
		return in.fail("bsa_window_realign_batch: download of the offsets and records failed");
	const uint64_t need = pcig2_off[P];                              // (the offsets are down before the capacity is judged)
	if(need > pcig2_cap) return in.fail("bsa_window_realign_batch: pcig2_cap too small, pcig2_off[piece_cap] holds the words needed", BSA_E_CIGAR_CAP);
	if(need == 0) return BSA_OK;
	const size_t o_words = res.part((size_t)need * 4u);
	if((rc = res.alloc("bsa_window_realign_batch: no device memory for the words")) != BSA_OK) return rc;
	a.pcig2 = res.at<uint32_t>(o_words); a.pcig2_cap = (size_t)need;
	if((rc = wr_run(ctx, stream, WR_FILL, a)) != BSA_OK) return rc;      // (on the scratch the first three steps left)
	if(!res.down(pcig2, o_words, (size_t)need * 4u) || !res.sync()) return res.fail("bsa_window_realign_batch: download of the words failed");
	return BSA_OK;
}
