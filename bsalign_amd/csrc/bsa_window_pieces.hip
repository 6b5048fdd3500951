// bsa_window_pieces.hip -- bsa_window_pieces_run / _batch (include/bsalign_hip.h): the turn from pair-major window records (what
// bsa_cigar_windows_run leaves: for every read, the windows it crosses) to window-major read pieces (for every window of the draft, the pieces
// of the reads that cross it, as 1 B/base codes in the strand that was aligned).
//
// A pass over public outputs and the resident blob: it knows no plan and no aligner.  Seven steps on the context stream:
//   clear  : the per-window counters in the context's scratch (hipMemsetAsync: a run leaves nothing behind that a later run reads);
//   count  : one wave a pair over its records (k_window_pieces_count): a record that is a piece adds 1 to cnt[g] and its length to bsum[g] with
//            vector atomics.  Integer sums do not depend on the order of the adds, so the offsets are a function of the inputs alone;
//   scan   : cnt -> d_piece_off with the 64-bit exclusive scan of bsa_api.hip, bsum (64-bit values) -> d_base_off with the same scan in tiles
//            for 64-bit input (k_wp_scan_*);
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
//            of the first 16-byte border of the destination one a lane, then 16 codes a lane and trip -- two unaligned 8-byte loads (byte-reversed
//            and ^ 3 for a marked read, as k_stage<.., true> does) or bsa_bits16 / bsa_bits16_rc from packed words -- into one aligned 16-byte
//            store, then the bytes behind the last border one a lane.  Every load lies inside the piece, so inside the read.
// No LDS, plain C++ with vector loads, stores and atomics only.
#include "bsa_common.h"
#include <vector>

extern "C" int bsa_ctx_get_stream_internal(bsa_ctx_t *ctx, hipStream_t *st);
extern "C" int bsa_ctx_scratch_internal(bsa_ctx_t *ctx, int slot, size_t bytes, void **out);
extern "C" void bsa_ctx_set_error_internal(bsa_ctx_t *ctx, const char *msg);
hipError_t bsa_launch_excl_scan(hipStream_t st, const uint32_t *cnt, uint64_t *off, uint32_t n, uint64_t *tmp);      // bsa_api.hip; tmp: bsa_excl_scan_tmp_bytes(n)
size_t bsa_excl_scan_tmp_bytes(uint32_t n);

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

static __device__ __forceinline__ uint64_t wp_load8(const uint8_t *p){ uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

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
			const uint32_t x = qf + head + 16u * c;                              // q'[x, x + 16)
			uint64_t v0, v1;
			if(PK){
				const uint32_t bits = rev ? bsa_bits16_rc(words, off + (ql - x - 16u), off + (ql - x)) : bsa_bits16(words, off + x, off + x + 16u);
				v0 = bsa_spread8(bits); v1 = bsa_spread8(bits >> 16);
			} else {
				if(rev){
					const uint8_t *s = seqs + off + (ql - x - 16u);              // the 16 stored bytes that end at ql - x, read backwards
					v1 = __builtin_bswap64(wp_load8(s)); v0 = __builtin_bswap64(wp_load8(s + 8));
					v0 ^= 0x0303030303030303ull; v1 ^= 0x0303030303030303ull;
				} else { v0 = wp_load8(seqs + off + x); v1 = wp_load8(seqs + off + x + 8u); }
				v0 &= 0x0303030303030303ull; v1 &= 0x0303030303030303ull;
			}
			uint4 o; o.x = (uint32_t)v0; o.y = (uint32_t)(v0 >> 32); o.z = (uint32_t)v1; o.w = (uint32_t)(v1 >> 32);
			*(uint4*)(dst + head + 16u * c) = o;
		}
		const uint32_t tb = head + 16u * body;
		if(gl < len - tb) dst[tb + gl] = code(qf + tb + gl);
	}
}

// the exclusive scan of bsa_api.hip for 64-bit values: sums of tiles, a scan of the sums by one block, every tile scanned with its base.
// tmp: tiles + 1 words, tiles = max(1, ceil(n / WP_SCAN_TILE)); off[n] = the total
#define WP_SCAN_TILE 4096u
__global__ void __launch_bounds__(256) k_wp_scan_sums(const uint64_t *v, uint32_t n, uint64_t *tmp){
	__shared__ uint64_t red[4];
	const uint32_t t = threadIdx.x;
	uint64_t s = 0;
	for(uint32_t i = t; i < WP_SCAN_TILE; i += 256u){ const uint64_t idx = (uint64_t)blockIdx.x * WP_SCAN_TILE + i; s += idx < n ? v[idx] : 0ull; }
	for(int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
	if((t & 63u) == 0u) red[t >> 6] = s;
	__syncthreads();
	if(t == 0) tmp[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(1024) k_wp_scan_bases(uint64_t *tmp, uint32_t tiles){
	__shared__ uint64_t part[1024];
	__shared__ uint64_t base;
	const uint32_t t = threadIdx.x;
	if(t == 0) base = 0ull;
	__syncthreads();
	for(uint32_t s = 0; s < tiles; s += 1024u){
		const uint64_t v = (s + t < tiles) ? tmp[s + t] : 0ull;
		part[t] = v;
		__syncthreads();
		for(uint32_t d = 1; d < 1024; d <<= 1){
			const uint64_t u = (t >= d) ? part[t - d] : 0ull;
			__syncthreads();
			part[t] += u;
			__syncthreads();
		}
		if(s + t < tiles) tmp[s + t] = part[t] - v + base;
		__syncthreads();
		if(t == 1023) base += part[1023];
		__syncthreads();
	}
	if(t == 0) tmp[tiles] = base;
}
__global__ void __launch_bounds__(256) k_wp_scan_apply(const uint64_t *v, uint64_t *off, uint32_t n, const uint64_t *tmp, uint32_t tiles){
	__shared__ uint64_t wsum[4];
	const uint32_t b = blockIdx.x, t = threadIdx.x;
	const uint64_t i0 = (uint64_t)b * WP_SCAN_TILE + t * 16u;          // 16 consecutive values per thread
	uint64_t loc[16], s = 0;
	for(int k = 0; k < 16; k++){ loc[k] = s; s += (i0 + k < n) ? v[i0 + k] : 0ull; }
	uint64_t inc = s;
	for(int d = 1; d < 64; d <<= 1){ const uint64_t u = __shfl_up(inc, d); if((t & 63u) >= (uint32_t)d) inc += u; }
	if((t & 63u) == 63u) wsum[t >> 6] = inc;
	__syncthreads();
	uint64_t wb = 0;
	for(uint32_t x = 0; x < (t >> 6); x++) wb += wsum[x];
	const uint64_t excl = tmp[b] + wb + inc - s;
	for(int k = 0; k < 16; k++) if(i0 + k < n) off[i0 + k] = excl + loc[k];
	if(b == tiles - 1u && t == 0) off[n] = tmp[tiles];
}
static uint32_t wp_scan_tiles(uint32_t n){ const uint32_t t = (uint32_t)(((uint64_t)n + WP_SCAN_TILE - 1u) / WP_SCAN_TILE); return t ? t : 1u; }
static hipError_t wp_launch_scan64(hipStream_t st, const uint64_t *v, uint64_t *off, uint32_t n, uint64_t *tmp){
	const uint32_t tiles = wp_scan_tiles(n);
	hipLaunchKernelGGL(k_wp_scan_sums, dim3(tiles), dim3(256), 0, st, v, n, tmp);
	hipLaunchKernelGGL(k_wp_scan_bases, dim3(1), dim3(1024), 0, st, tmp, tiles);
	hipLaunchKernelGGL(k_wp_scan_apply, dim3(tiles), dim3(256), 0, st, v, off, n, (const uint64_t*)tmp, tiles);
	return hipGetLastError();
}

// the pass's part of the context's scratch: cnt | bsum (cleared by the offsets) | cur | written (cleared by the fill) | the scans' tiles | ent
struct wp_scratch_t { uint32_t *cnt; unsigned long long *bsum; uint32_t *cur; uint64_t *written, *tmp32, *tmp64; wp_ent_t *ent; };
static int wp_scratch(bsa_ctx_t *ctx, size_t nwin, size_t ent_cap, wp_scratch_t *s){
	auto up = [](size_t b){ return (b + 255u) & ~(size_t)255u; };
	const size_t o_cnt = 0, o_bsum = o_cnt + up(nwin * 4u), o_cur = o_bsum + up(nwin * 8u), o_wr = o_cur + up(nwin * 4u), o_t32 = o_wr + 256u,
		o_t64 = o_t32 + up(bsa_excl_scan_tmp_bytes((uint32_t)nwin)), o_ent = o_t64 + up(((size_t)wp_scan_tiles((uint32_t)nwin) + 1u) * 8u);
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
	if(e == hipSuccess) e = bsa_launch_excl_scan(st, s.cnt, d_piece_off, a.nwin, s.tmp32);
	if(e == hipSuccess) e = wp_launch_scan64(st, (const uint64_t*)s.bsum, d_base_off, a.nwin, s.tmp64);
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_pieces: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}
// the gather launch of wp_fill; s.written: the records the order kernel left
static hipError_t wp_launch_gather(hipStream_t st, const wp_in_t &a, const wp_scratch_t &s, const bsa_piece_t *d_piece, size_t piece_cap, uint8_t *d_bases, size_t bases_cap){
	const size_t want = (piece_cap + 15u) / 16u, most = (size_t)bsa_cus() * 16u;          // 16 pieces a block and trip
	const dim3 grid((uint32_t)(want < most ? want : most)), block(256);
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
		if(win_off[k + 1] < win_off[k]){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_batch: win_off decreases"); return BSA_E_ARG; }
	}
	const uint64_t r0 = win_off[0], recs = win_off[n] - r0;          // only the records the offsets speak of go up
	if(recs && !win){ bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_batch: null argument"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	auto up = [](size_t b){ return (b + 255u) & ~(size_t)255u; };
	const size_t o_seq = 0, o_qoff = o_seq + up(seqs_bytes + 8u), o_qlen = o_qoff + up(n * 8u), o_woff = o_qlen + up(n * 4u), o_gb = o_woff + up((n + 1u) * 8u),
		o_poff = o_gb + up(n * 8u), o_boff = o_poff + up((nwin + 1u) * 8u), o_win = o_boff + up((nwin + 1u) * 8u), total = o_win + up(recs * sizeof(bsa_window_t) + 16u);
	uint8_t *buf = nullptr, *d_out = nullptr;
	auto fail = [&](const char *what, int code){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, what); rc = code; };
	std::vector<uint64_t> woff;
	try { woff.resize(n + 1); } catch(...){ return BSA_E_NOMEM; }
	for(size_t k = 0; k <= n; k++) woff[k] = win_off[k] - r0;
	do {
		if(hipMalloc((void**)&buf, total) != hipSuccess){ buf = nullptr; fail("bsa_window_pieces_batch: no device memory for the blob and the records", BSA_E_NOMEM); break; }
		if((seqs_bytes && hipMemcpyAsync(buf + o_seq, seqs, seqs_bytes, hipMemcpyHostToDevice, stream) != hipSuccess)
				|| hipMemcpyAsync(buf + o_qoff, qoff, n * 8u, hipMemcpyHostToDevice, stream) != hipSuccess
				|| hipMemcpyAsync(buf + o_qlen, qlen, n * 4u, hipMemcpyHostToDevice, stream) != hipSuccess
				|| hipMemcpyAsync(buf + o_woff, woff.data(), (n + 1u) * 8u, hipMemcpyHostToDevice, stream) != hipSuccess
				|| hipMemcpyAsync(buf + o_gb, gbase, n * 8u, hipMemcpyHostToDevice, stream) != hipSuccess
				|| (recs && hipMemcpyAsync(buf + o_win, win + r0, recs * sizeof(bsa_window_t), hipMemcpyHostToDevice, stream) != hipSuccess)){ fail("bsa_window_pieces_batch: upload failed", BSA_E_HIP); break; }
		const wp_in_t a = { buf + o_seq, (const uint64_t*)(buf + o_qoff), (const uint32_t*)(buf + o_qlen), (const bsa_window_t*)(buf + o_win), (const uint64_t*)(buf + o_woff),
			(const uint64_t*)(buf + o_gb), (uint32_t)n, window, (uint32_t)nwin, flags };
		uint64_t *d_poff = (uint64_t*)(buf + o_poff), *d_boff = (uint64_t*)(buf + o_boff);
		wp_scratch_t s;
		if((rc = wp_scratch(ctx, nwin, 0u, &s)) != BSA_OK) break;
		if((rc = wp_offsets(ctx, stream, a, s, d_poff, d_boff)) != BSA_OK) break;
		if(hipMemcpyAsync(piece_off, d_poff, (nwin + 1u) * 8u, hipMemcpyDeviceToHost, stream) != hipSuccess
				|| hipMemcpyAsync(base_off, d_boff, (nwin + 1u) * 8u, hipMemcpyDeviceToHost, stream) != hipSuccess
				|| hipStreamSynchronize(stream) != hipSuccess){ fail("bsa_window_pieces_batch: download of the offsets failed", BSA_E_HIP); break; }
		const uint64_t np = piece_off[nwin], nb = base_off[nwin];
		if(np > piece_cap || nb > bases_cap){
			bsa_ctx_set_error_internal(ctx, "bsa_window_pieces_batch: piece_cap or bases_cap too small, piece_off[nwin] and base_off[nwin] hold what is needed"); rc = BSA_E_CIGAR_CAP; break;
		}
		if(np == 0) break;
		const size_t o_b = up(np * sizeof(bsa_piece_t));
		if(hipMalloc((void**)&d_out, o_b + up(nb)) != hipSuccess){ d_out = nullptr; fail("bsa_window_pieces_batch: no device memory for the pieces", BSA_E_NOMEM); break; }
		if((rc = wp_scratch(ctx, nwin, np, &s)) != BSA_OK) break;
		if((rc = wp_fill(ctx, stream, a, s, d_poff, d_boff, (bsa_piece_t*)d_out, np, d_out + o_b, nb)) != BSA_OK) break;
		if(hipMemcpyAsync(piece, d_out, np * sizeof(bsa_piece_t), hipMemcpyDeviceToHost, stream) != hipSuccess
				|| hipMemcpyAsync(bases, d_out + o_b, nb, hipMemcpyDeviceToHost, stream) != hipSuccess
				|| hipStreamSynchronize(stream) != hipSuccess){ fail("bsa_window_pieces_batch: download of the pieces failed", BSA_E_HIP); break; }
	} while(0);
	if(rc != BSA_OK && rc != BSA_E_CIGAR_CAP) (void)hipStreamSynchronize(stream);      // nothing of the call is in flight when its buffers go
	if(d_out) (void)hipFree(d_out);
	if(buf) (void)hipFree(buf);
	return rc;
}
