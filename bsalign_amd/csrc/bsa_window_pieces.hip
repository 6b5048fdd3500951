// bsa_window_pieces.hip -- bsa_window_pieces_run / _batch (include/bsalign_hip.h): the turn from pair-major window records (what
// bsa_cigar_windows_run leaves: for every read, the windows it crosses) to window-major read pieces (for every window of the draft, the pieces
// of the reads that cross it, as 1 B/base codes in the strand that was aligned).
//
// A pass over public outputs and the resident blob: it knows no plan and no aligner.  Seven steps on the context stream:
//   clear  : the per-window counters in the context's scratch (hipMemsetAsync: a run leaves nothing behind that a later run reads);
//   count  : one wave a pair over its records (k_window_pieces_count): a record that is a piece adds 1 to cnt[g] and its length to bsum[g] with
//            vector atomics.  Integer sums do not depend on the order of the adds, so the offsets are a function of the inputs alone;
//   scan   : cnt -> d_piece_off and bsum (64-bit values) -> d_base_off, both with the 64-bit exclusive scan of bsa_scan.hip (its tile kernels
//            take either value type; 64-bit values always go to tiles);
//   place  : the count kernel's loop again (k_window_pieces_place): a piece of a window that FITS (both of its ranges end inside the caps) takes a
//            slot from the window's cursor and leaves (record index, pair, length) in ent[piece_off[g] + slot], in scratch.  The slot order is
//            whatever the atomics made it;
//   order  : one wave a window that fits (k_window_pieces_order): every entry counts the entries of its window with a smaller record index
//            -- its rank -- and sums their lengths -- its bases' offset -- against tiles of 64 entries held a lane each and read by shuffle, so a
//            window of any depth takes the same path (d entries cost d * ceil(d / 64) shuffle trips: 5000 pieces are a few milliseconds of one
//            wave, 40 are nothing).  The entry then writes its finished record to piece[piece_off[g] + rank]: every field, once.  Ranks are a
//            function of the record indices, so what the atomics did to the slots does not show.  The windows that fit are a prefix of the
//            windows (both offset arrays ascend); the wave of the last one leaves the number of records written for the gather;
//   gather : 16 lanes a piece, four pieces a wave, over the records just written (k_window_pieces_gather<PACKED, STRANDS>): the bytes in front
//            of the first 16-byte border of the destination one a lane, then 16 codes a lane and trip -- the staging kernels' reader (bsa_seq.h,
//            bsa_seq16: two unaligned 8-byte loads, byte-reversed and ^ 3 for a marked read, or two bits a base from packed words) -- into one aligned 16-byte
//            store, then the bytes behind the last border one a lane.  Every load lies inside the piece, so inside the read.
// No LDS in this file's kernels, plain C++ with vector loads, stores and atomics only.
#include "bsa_pass.h"
#include <vector>

static_assert(sizeof(bsa_piece_t) == 32, "bsa_piece_t is 32 bytes");

struct wp_ent_t { uint64_t i; uint32_t k, len; };          // a placed piece: its record, its pair, its bases

// the definition's "which records are pieces": *g gets the window.  gb >= nwin first, so that gb + t_first / w cannot wrap
static __device__ __forceinline__ bool wp_is_piece(const bsa_window_t &r, uint32_t ql, uint64_t gb, uint32_t w, uint32_t nwin, uint32_t *g){
	if(r.t_first == BSA_WINDOW_NONE || r.t_first > r.t_last || r.q_first > r.q_last || r.q_last >= ql || gb >= nwin) return false;
	const uint64_t x = gb + r.t_first / w;
	*g = (uint32_t)x;
	return x < nwin;
}

__global__ void __launch_bounds__(256) k_window_pieces_count(const bsa_window_t *win, const uint64_t *woff, const uint32_t *qlen, const uint64_t *gbase,
		uint32_t n, uint32_t w, uint32_t nwin, uint32_t *cnt, unsigned long long *bsum){
	const uint32_t k = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
	if(k >= n) return;
	const uint64_t a = woff[k], b = woff[k + 1u];
	const uint32_t ql = qlen[k];
	const uint64_t gb = gbase[k];
	for(uint64_t i = a + lane; i < b; i += 64u){
		const bsa_window_t r = win[i];
		uint32_t g;
		if(!wp_is_piece(r, ql, gb, w, nwin, &g)) continue;
		atomicAdd(&cnt[g], 1u);
		atomicAdd(&bsum[g], (unsigned long long)(r.q_last - r.q_first + 1u));
	}
}

// pcap, bcap: window g fits when poff[g + 1] <= pcap and boff[g + 1] <= bcap; ent has pcap places
__global__ void __launch_bounds__(256) k_window_pieces_place(const bsa_window_t *win, const uint64_t *woff, const uint32_t *qlen, const uint64_t *gbase,
		uint32_t n, uint32_t w, uint32_t nwin, const uint64_t *poff, const uint64_t *boff, uint64_t pcap, uint64_t bcap, uint32_t *cur, wp_ent_t *ent){
	const uint32_t k = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
	if(k >= n) return;
	const uint64_t a = woff[k], b = woff[k + 1u];
	const uint32_t ql = qlen[k];
	const uint64_t gb = gbase[k];
	for(uint64_t i = a + lane; i < b; i += 64u){
		const bsa_window_t r = win[i];
		uint32_t g;
		if(!wp_is_piece(r, ql, gb, w, nwin, &g)) continue;
		const uint64_t p1 = poff[g + 1u];
		if(p1 > pcap || boff[g + 1u] > bcap) continue;
		const uint64_t at = poff[g] + atomicAdd(&cur[g], 1u);
		if(at < p1){ wp_ent_t e; e.i = i; e.k = k; e.len = r.q_last - r.q_first + 1u; ent[at] = e; }          // (at < p1: the counts are this loop's own)
	}
}

// one wave a window
__global__ void __launch_bounds__(256) k_window_pieces_order(const bsa_window_t *win, const wp_ent_t *ent, const uint64_t *poff, const uint64_t *boff,
		uint32_t nwin, uint64_t pcap, uint64_t bcap, bsa_piece_t *piece, uint64_t *written){
	const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
	if(g >= nwin) return;
	const uint64_t p0 = poff[g], p1 = poff[g + 1u], b0 = boff[g];
	if(p1 > pcap || boff[g + 1u] > bcap) return;
	if(lane == 0u && (g + 1u == nwin || poff[g + 2u] > pcap || boff[g + 2u] > bcap)) *written = p1;          // the last window that fits
	if(p1 <= p0) return;
	const uint64_t d = p1 - p0;
	const wp_ent_t none = { ~0ull, 0u, 0u };
	for(uint64_t e0 = 0; e0 < d; e0 += 64u){
		const bool have = e0 + lane < d;
		const wp_ent_t mine = have ? ent[p0 + e0 + lane] : none;
		uint64_t rank = 0, bo = 0;
		for(uint64_t t0 = 0; t0 < d; t0 += 64u){
			const wp_ent_t o = t0 + lane < d ? ent[p0 + t0 + lane] : none;
			const int m = d - t0 < 64u ? (int)(d - t0) : 64;
			for(int j = 0; j < m; j++){
				const uint64_t oi = __shfl(o.i, j);
				const uint32_t ol = __shfl(o.len, j);
				if(oi < mine.i){ rank++; bo += ol; }
			}
		}
		if(have && rank < d){
			const bsa_window_t r = win[mine.i];
			bsa_piece_t x;
			x.pair = mine.k; x.q_first = r.q_first; x.len = mine.len; x.t_first = r.t_first; x.t_last = r.t_last; x.reserved = 0u; x.base_off = b0 + bo;
			piece[p0 + rank] = x;
		}
	}
}

// PK: BSA_MODE_SEQ2BIT words; QS: BSA_MODE_QSTRAND, bit 63 of qoff[k] asks for the reverse complement
template<bool PK, bool QS>
__global__ void __launch_bounds__(256) k_window_pieces_gather(const uint8_t *seqs, const uint64_t *qoff, const uint32_t *qlen, const bsa_piece_t *piece,
		const uint64_t *written, uint8_t *bases, uint64_t bcap){
	const uint32_t gl = threadIdx.x & 15u;
	const uint64_t P = *written, ngrp = (uint64_t)gridDim.x * 16u;
	const uint64_t *words = (const uint64_t*)seqs;
	for(uint64_t j = blockIdx.x * 16u + (threadIdx.x >> 4); j < P; j += ngrp){
		const bsa_piece_t pc = piece[j];
		const uint64_t qo = qoff[pc.pair];
		const uint32_t ql = qlen[pc.pair], len = pc.len, qf = pc.q_first;
		const bool rev = QS && (qo & BSA_QOFF_REVCOMP) != 0;
		const uint64_t off = QS ? qo & ~BSA_QOFF_REVCOMP : qo;
		if((uint64_t)qf + len > ql || pc.base_off + len > bcap) continue;          // (holds for every record the order kernel wrote)
		uint8_t *dst = bases + pc.base_off;
		// q'[x], one base
		auto code = [&](uint32_t x) -> uint8_t {
			const uint64_t pos = off + (rev ? ql - 1u - x : x);
			uint32_t c = PK ? (uint32_t)(words[pos >> 5] >> (62u - 2u * (uint32_t)(pos & 31u))) : seqs[pos];
			if(rev) c ^= 3u;
			return (uint8_t)(c & 3u);
		};
		const uint32_t head = min(len, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
		if(gl < head) dst[gl] = code(qf + gl);
		const uint32_t body = (len - head) >> 4;
		for(uint32_t c = gl; c < body; c += 16u){
			const uint32_t x = qf + head + 16u * c;                              // q'[x, x + 16): a whole piece of the read (x + 16 <= qf + len <= ql)
			// The reader (bsa_seq16) is given the read's own bounds, the loads are the piece's: with sixteen bases or more between them the second-word
			// conditions of bsa_bits16 (pos, end) and bsa_bits16_rc (beg, end) look at pos + 15 and at end - 16 alone, whatever `end` and `beg` are.
			// "A whole piece", said in the terms the reader tests, so that its end-piece paths are not compiled in (each holds: x + 16 <= ql, off < 2^63):
			__builtin_assume(x + 16u <= ql);
			if(PK){
				__builtin_assume(off + x < off + ql); __builtin_assume((off + ql) - (off + x) >= 16u);          // bsa_bits16(w, off + x, off + ql)
				__builtin_assume(off + ql - x > off); __builtin_assume((off + ql - x) - off >= 16u);            // bsa_bits16_rc(w, off, off + ql - x)
			}
			uint64_t v0, v1;
			uint32_t bad = 0;                                                    // (codes are taken & 3; nobody is told)
			bsa_seq16<PK, QS>(seqs, off, ql, x, rev, (uint8_t)0, v0, v1, bad);
			bsa_store16(dst + head + 16u * c, v0, v1);
		}
		const uint32_t tb = head + 16u * body;
		if(gl < len - tb) dst[tb + gl] = code(qf + tb + gl);
	}
}

// the pass's part of the context's scratch: cnt | bsum (cleared by the offsets) | cur | written (cleared by the fill) | the scans' tiles | ent
struct wp_scratch_t { uint32_t *cnt; unsigned long long *bsum; uint32_t *cur; uint64_t *written, *tmp32, *tmp64; wp_ent_t *ent; };
static int wp_scratch(bsa_ctx_t *ctx, size_t nwin, size_t ent_cap, wp_scratch_t *s){
	const size_t tmp = bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)nwin));
	const size_t o_cnt = 0, o_bsum = o_cnt + bsa_up256(nwin * 4u), o_cur = o_bsum + bsa_up256(nwin * 8u), o_wr = o_cur + bsa_up256(nwin * 4u), o_t32 = o_wr + 256u,
		o_t64 = o_t32 + tmp, o_ent = o_t64 + tmp;
	if(ent_cap > (((size_t)1 << 62) - o_ent) / sizeof(wp_ent_t)){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces: piece_cap too large for the scratch it needs"); return BSA_E_NOMEM; }
	void *bufv = nullptr;
	const int rc = bsa_ctx_scratch_internal(ctx, 1, o_ent + ent_cap * sizeof(wp_ent_t), &bufv);      // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	s->cnt = (uint32_t*)(b + o_cnt); s->bsum = (unsigned long long*)(b + o_bsum); s->cur = (uint32_t*)(b + o_cur); s->written = (uint64_t*)(b + o_wr);
	s->tmp32 = (uint64_t*)(b + o_t32); s->tmp64 = (uint64_t*)(b + o_t64); s->ent = (wp_ent_t*)(b + o_ent);
	return BSA_OK;
}

struct wp_in_t { const uint8_t *seqs; const uint64_t *qoff; const uint32_t *qlen; const bsa_window_t *win; const uint64_t *woff; const uint64_t *gbase; uint32_t n, window, nwin, flags; };

// clear, count, scan: d_piece_off[0 .. nwin], d_base_off[0 .. nwin]
static int wp_offsets(bsa_ctx_t *ctx, hipStream_t st, const wp_in_t &a, const wp_scratch_t &s, uint64_t *d_piece_off, uint64_t *d_base_off){
	hipError_t e = hipSuccess;
	if(a.nwin) e = hipMemsetAsync(s.cnt, 0, (size_t)((uint8_t*)s.cur - (uint8_t*)s.cnt), st);
	if(e == hipSuccess && a.n && a.nwin){
		hipLaunchKernelGGL(k_window_pieces_count, dim3((a.n + 3u) / 4u), dim3(256), 0, st, a.win, a.woff, a.qlen, a.gbase, a.n, a.window, a.nwin, s.cnt, s.bsum);
		e = hipGetLastError();
	}
	if(e == hipSuccess) e = bsa_launch_excl_scan(st, s.cnt, d_piece_off, a.nwin, nullptr, s.tmp32);
	if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint64_t*)s.bsum, d_base_off, a.nwin, nullptr, s.tmp64);
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_pieces: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}
// the gather launch of wp_fill; s.written: the records the order kernel left
static hipError_t wp_launch_gather(hipStream_t st, const wp_in_t &a, const wp_scratch_t &s, const bsa_piece_t *d_piece, size_t piece_cap, uint8_t *d_bases, size_t bases_cap){
	const dim3 grid = bsa_grid16(piece_cap), block(256);
	const bool pk = (a.flags & BSA_MODE_SEQ2BIT) != 0, qs = (a.flags & BSA_MODE_QSTRAND) != 0;
#define WP_GATHER(PK, QS) hipLaunchKernelGGL((k_window_pieces_gather<PK, QS>), grid, block, 0, st, a.seqs, a.qoff, a.qlen, d_piece, (const uint64_t*)s.written, d_bases, (uint64_t)bases_cap)
	if(pk){ if(qs) WP_GATHER(true, true); else WP_GATHER(true, false); }
	else { if(qs) WP_GATHER(false, true); else WP_GATHER(false, false); }
#undef WP_GATHER
	return hipGetLastError();
}

// place, order, gather: the windows that fit
static int wp_fill(bsa_ctx_t *ctx, hipStream_t st, const wp_in_t &a, const wp_scratch_t &s, const uint64_t *d_piece_off, const uint64_t *d_base_off,
		bsa_piece_t *d_piece, size_t piece_cap, uint8_t *d_bases, size_t bases_cap){
	if(a.n == 0 || a.nwin == 0 || piece_cap == 0 || bases_cap == 0) return BSA_OK;          // (a piece has a record and at least one base: nothing fits)
	hipError_t e = hipMemsetAsync(s.cur, 0, (size_t)((uint8_t*)s.tmp32 - (uint8_t*)s.cur), st);
	if(e == hipSuccess){
		hipLaunchKernelGGL(k_window_pieces_place, dim3((a.n + 3u) / 4u), dim3(256), 0, st, a.win, a.woff, a.qlen, a.gbase, a.n, a.window, a.nwin,
			d_piece_off, d_base_off, (uint64_t)piece_cap, (uint64_t)bases_cap, s.cur, s.ent);
		hipLaunchKernelGGL(k_window_pieces_order, dim3((a.nwin + 3u) / 4u), dim3(256), 0, st, a.win, (const wp_ent_t*)s.ent, d_piece_off, d_base_off,
			a.nwin, (uint64_t)piece_cap, (uint64_t)bases_cap, d_piece, s.written);
		e = wp_launch_gather(st, a, s, d_piece, piece_cap, d_bases, bases_cap);
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_pieces: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

// the argument errors of both calls
static int wp_check(bsa_ctx_t *ctx, const void *seqs, const void *qoff, const void *qlen, const void *woff, const void *gbase, size_t n, uint32_t window, size_t nwin,
		uint32_t flags, const void *piece, size_t piece_cap, const void *piece_off, const void *bases, size_t bases_cap, const void *base_off){
	const char *msg = nullptr;
	if(window == 0) msg = "bsa_window_pieces: window == 0";
	else if(flags & ~(uint32_t)(BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND)) msg = "bsa_window_pieces: flags other than BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND";
	else if(!piece_off || !base_off || (n && (!seqs || !qoff || !qlen || !woff || !gbase)) || (piece_cap && !piece) || (bases_cap && !bases)) msg = "bsa_window_pieces: null argument";
	else if(n > 0xFFFFFFF0ull) msg = "too many pairs";
	else if(nwin > 0xFFFFFFF0ull) msg = "too many windows";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	return BSA_OK;
}

extern "C" int bsa_window_pieces_run(bsa_ctx_t *ctx, const uint8_t *d_seqs, const uint64_t *d_qoff, const uint32_t *d_qlen,
		const bsa_window_t *d_win, const uint64_t *d_win_off, size_t n, uint32_t window, const uint64_t *d_gbase, size_t nwin, uint32_t flags,
		bsa_piece_t *d_piece, size_t piece_cap, uint64_t *d_piece_off, uint8_t *d_bases, size_t bases_cap, uint64_t *d_base_off){
	if(!ctx) return BSA_E_ARG;
	int rc = wp_check(ctx, d_seqs, d_qoff, d_qlen, d_win_off, d_gbase, n, window, nwin, flags, d_piece, piece_cap, d_piece_off, d_bases, bases_cap, d_base_off);
	if(rc != BSA_OK) return rc;
	if(n && !d_win){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_run: null argument"); return BSA_E_ARG; }
	if((flags & BSA_MODE_SEQ2BIT) && ((uintptr_t)d_seqs & 7u)){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_run: BSA_MODE_SEQ2BIT needs an 8-byte aligned d_seqs"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	const bool fill = n && nwin && piece_cap && bases_cap;
	wp_scratch_t s;
	if((rc = wp_scratch(ctx, nwin, fill ? piece_cap : 0u, &s)) != BSA_OK) return rc;
	const wp_in_t a = { d_seqs, d_qoff, d_qlen, d_win, d_win_off, d_gbase, (uint32_t)n, window, (uint32_t)nwin, flags };
	if((rc = wp_offsets(ctx, stream, a, s, d_piece_off, d_base_off)) != BSA_OK) return rc;
	return wp_fill(ctx, stream, a, s, d_piece_off, d_base_off, d_piece, piece_cap, d_bases, bases_cap);
}

// for tools/bench_window_pieces.py: the gather launch alone, once more, over the records the context's last bsa_window_pieces_run wrote (same arguments, same
// scratch: nothing else may have used the context in between)
extern "C" int bsa_window_pieces_gather_internal(bsa_ctx_t *ctx, const uint8_t *d_seqs, const uint64_t *d_qoff, const uint32_t *d_qlen, size_t nwin, uint32_t flags,
		const bsa_piece_t *d_piece, size_t piece_cap, uint8_t *d_bases, size_t bases_cap){
	if(!ctx || !d_seqs || !d_qoff || !d_qlen || !d_piece || !d_bases || !piece_cap || !bases_cap || nwin > 0xFFFFFFF0ull || (flags & ~(uint32_t)(BSA_MODE_SEQ2BIT | BSA_MODE_QSTRAND))) return BSA_E_ARG;
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);
	if(rc != BSA_OK) return rc;
	wp_scratch_t s;
	if((rc = wp_scratch(ctx, nwin, piece_cap, &s)) != BSA_OK) return rc;
	const wp_in_t a = { d_seqs, d_qoff, d_qlen, nullptr, nullptr, nullptr, 0u, 1u, (uint32_t)nwin, flags };
	if(wp_launch_gather(stream, a, s, d_piece, piece_cap, d_bases, bases_cap) != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_pieces: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

extern "C" int bsa_window_pieces_batch(bsa_ctx_t *ctx, const uint8_t *seqs, size_t seqs_bytes, const uint64_t *qoff, const uint32_t *qlen,
		const bsa_window_t *win, const uint64_t *win_off, size_t n, uint32_t window, const uint64_t *gbase, size_t nwin, uint32_t flags,
		bsa_piece_t *piece, size_t piece_cap, uint64_t *piece_off, uint8_t *bases, size_t bases_cap, uint64_t *base_off){
	if(!ctx) return BSA_E_ARG;
	int rc = wp_check(ctx, seqs, qoff, qlen, win_off, gbase, n, window, nwin, flags, piece, piece_cap, piece_off, bases, bases_cap, base_off);
	if(rc != BSA_OK) return rc;
	const bool pk = (flags & BSA_MODE_SEQ2BIT) != 0;
	if(pk && (seqs_bytes & 7u)){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_batch: BSA_MODE_SEQ2BIT needs seqs_bytes to be a multiple of 8"); return BSA_E_ARG; }
	if(n == 0 || nwin == 0){
		for(size_t g = 0; g <= nwin; g++) piece_off[g] = base_off[g] = 0;
		return BSA_OK;
	}
	const uint64_t mask = (flags & BSA_MODE_QSTRAND) ? ~BSA_QOFF_REVCOMP : ~0ull;
	const uint64_t have = pk ? (seqs_bytes > (~0ull >> 2) ? ~0ull : (uint64_t)seqs_bytes * 4u) : (uint64_t)seqs_bytes;
	for(size_t k = 0; k < n; k++){
		const uint64_t o = qoff[k] & mask;
		if(o > have || qlen[k] > have - o){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_batch: a read lies outside the blob"); return BSA_E_ARG; }
	}
	std::vector<uint64_t> woff;
	if((rc = bsa_rebase_offsets(ctx, win_off, n, woff, "bsa_window_pieces_batch: win_off decreases")) != BSA_OK) return rc;
	const uint64_t r0 = win_off[0], recs = woff[n];                       // only the records the offsets speak of go up
	if(recs && !win){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_batch: null argument"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	bsa_stage_t in(ctx, stream), res(ctx, stream);
	const size_t o_seq = in.part(seqs_bytes + 8u), o_qoff = in.part(n * 8u), o_qlen = in.part(n * 4u), o_woff = in.part((n + 1u) * 8u), o_gb = in.part(n * 8u),
		o_poff = in.part((nwin + 1u) * 8u), o_boff = in.part((nwin + 1u) * 8u), o_win = in.part(recs * sizeof(bsa_window_t) + 16u);
	if((rc = in.alloc("bsa_window_pieces_batch: no device memory for the blob and the records")) != BSA_OK) return rc;
	if(!in.up(o_seq, seqs, seqs_bytes) || !in.up(o_qoff, qoff, n * 8u) || !in.up(o_qlen, qlen, n * 4u) || !in.up(o_woff, woff.data(), (n + 1u) * 8u) || !in.up(o_gb, gbase, n * 8u)
			|| !in.up(o_win, recs ? win + r0 : nullptr, recs * sizeof(bsa_window_t))) return in.fail("bsa_window_pieces_batch: upload failed");
	const wp_in_t a = { in.at<uint8_t>(o_seq), in.at<uint64_t>(o_qoff), in.at<uint32_t>(o_qlen), in.at<bsa_window_t>(o_win), in.at<uint64_t>(o_woff), in.at<uint64_t>(o_gb),
		(uint32_t)n, window, (uint32_t)nwin, flags };
	uint64_t *d_poff = in.at<uint64_t>(o_poff), *d_boff = in.at<uint64_t>(o_boff);
	wp_scratch_t s;
	if((rc = wp_scratch(ctx, nwin, 0u, &s)) != BSA_OK) return rc;
	if((rc = wp_offsets(ctx, stream, a, s, d_poff, d_boff)) != BSA_OK) return rc;
	if(!in.down(piece_off, o_poff, (nwin + 1u) * 8u) || !in.down(base_off, o_boff, (nwin + 1u) * 8u) || !in.sync()) return in.fail("bsa_window_pieces_batch: download of the offsets failed");
	const uint64_t np = piece_off[nwin], nb = base_off[nwin];             // (the offsets are down before the capacities are judged)
	if(np > piece_cap || nb > bases_cap)
		return in.fail("bsa_window_pieces_batch: piece_cap or bases_cap too small, piece_off[nwin] and base_off[nwin] hold what is needed", BSA_E_CIGAR_CAP);
	if(np == 0) return BSA_OK;
	const size_t o_p = res.part(np * sizeof(bsa_piece_t)), o_b = res.part(nb);
	if((rc = res.alloc("bsa_window_pieces_batch: no device memory for the pieces")) != BSA_OK) return rc;
	if((rc = wp_scratch(ctx, nwin, np, &s)) != BSA_OK) return rc;
	if((rc = wp_fill(ctx, stream, a, s, d_poff, d_boff, res.at<bsa_piece_t>(o_p), np, res.at<uint8_t>(o_b), nb)) != BSA_OK) return rc;
	if(!res.down(piece, o_p, np * sizeof(bsa_piece_t)) || !res.down(bases, o_b, nb) || !res.sync()) return res.fail("bsa_window_pieces_batch: download of the pieces failed");
	return BSA_OK;
}
