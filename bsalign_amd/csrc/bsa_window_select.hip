// bsa_window_select.hip -- bsa_window_select_run / _batch (include/bsalign_hip.h): which of a window's pieces take part in its MSA.  Pieces whose
// span or whose pair's identity is too small are dropped, and of the candidates that remain at most max_depth are kept: the widest, ties decided by a
// hash of the pair and then by the index.  The selected records leave verbatim, in their order, window-major like the input.
//
// A pass over public outputs: the piece records and offsets as bsa_window_pieces_run wrote them and, for the identity test, the aligner's records.
// Three steps on the context stream:
//   count : a wave a window (k_window_select_count) goes over the window's records once, counts the candidates and, where the cap binds, finds the key T
//           of the max_depth-th best by radix selection: eight digits of eight bits from the top, every digit a histogram of the keys under the prefix
//           found so far, in 1 KB of the wave's LDS -- 8 x ceil(depth / 64) trips, not the depth x ceil(depth / 64) of a rank by comparison.  A window
//           of up to WSEL_HELD records keeps its keys in LDS (a lane reads back only what it wrote); a deeper one forms them from the records again,
//           with the same function, so that the result does not depend on the side a window falls.  It leaves T, the quota of keys equal to T and the
//           selected count in the context's scratch;
//   scan  : bsa_scan.hip's exclusive scan of the counts into d_sel_off;
//   fill  : a wave a window that fits (k_window_select_fill) goes over the records once more in the same order: a candidate is kept if its key is
//           above T, or equals T while the quota lasts.  A ballot and a prefix count give every kept record its place; 32 bytes move as two 16-byte
//           vectors where both arrays allow it.
// wsel_key is the one copy of the candidate test and the key; both kernels call it.  Plain C++; no kernel uses scratch memory.
#include "bsa_pass.h"

static_assert(sizeof(bsa_piece_t) == 32 && sizeof(bsa_select_params_t) == 32 && sizeof(bsa_result_t) == 40, "the records' layouts");

// the records a window may have to keep its keys in LDS: 4 KB a wave, with the histogram 20 KB a workgroup
#define WSEL_HELD 512u

struct wsel_par_t { const bsa_result_t *out; uint32_t n, max_depth, min_span, ident_num, ident_den, seed; };          // out: NULL without the identity test
enum { WSEL_COUNT = 1, WSEL_FILL = 2 };

static __device__ __forceinline__ uint32_t wsel_mix32(uint32_t x){
	x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
	return x;
}

// The rules of the header, once: is the piece a candidate, and its key -- the larger the better.
static __device__ __forceinline__ bool wsel_key(const wsel_par_t &p, uint32_t pair, uint32_t len, uint32_t t_first, uint32_t t_last, uint64_t *key){
	if(t_first > t_last || len == 0u) return false;
	const uint32_t sp = t_last - t_first;
	if(p.min_span > 1u && sp < p.min_span - 1u) return false;
	if(p.out){
		if(pair >= p.n) return false;
		const int32_t mat = p.out[pair].mat, aln = p.out[pair].aln;
		if(aln <= 0 || mat < 0) return false;
		if((uint64_t)(uint32_t)mat * p.ident_den < (uint64_t)p.ident_num * (uint64_t)(uint32_t)aln) return false;          // (below 2^63 both: nothing wraps)
	}
	*key = (uint64_t)sp << 32 | (uint32_t)~wsel_mix32(pair ^ p.seed);
	return true;
}

// the one door to the records: the window's first record and its depth, 0 for a window without pieces
static __device__ __forceinline__ uint32_t wsel_depth(const uint64_t *poff, uint32_t g, uint64_t pcap, uint64_t *p0){
	const uint64_t a = poff[g], b = poff[g + 1u];
	*p0 = a;
	return (b > pcap || b < a) ? 0u : (uint32_t)(b - a);             // (pcap <= 0xFFFFFFF0)
}

// what one lane wrote to the wave's LDS is there for the others, and the other way round (LDS operations of a wave complete in order)
static __device__ __forceinline__ void wsel_wave_sync(){
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave a window, four a workgroup
__global__ void __launch_bounds__(256) k_window_select_count(const bsa_piece_t *piece, const uint64_t *poff, uint32_t nwin, uint64_t pcap, wsel_par_t par,
		uint64_t *thr, uint32_t *quota, uint32_t *cnt, uint32_t *ncand){
	__shared__ uint64_t keys_all[4][WSEL_HELD];
	__shared__ uint4 hist_all[4][64];
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, g = blockIdx.x * 4u + wave;
	if(g >= nwin) return;
	uint64_t *keys = keys_all[wave];
	uint32_t *hist = (uint32_t*)hist_all[wave];
	uint64_t p0;
	const uint32_t d = wsel_depth(poff, g, pcap, &p0);
	const bool held = d <= WSEL_HELD;
	uint32_t C = 0, mine = 0;                                         // mine, bit t: record lane + 64 t is a candidate (held windows)
	for(uint64_t i0 = 0; i0 < d; i0 += 64u){
		uint64_t key = 0;
		bool c = false;
		if(i0 + lane < d){
			const bsa_piece_t *r = piece + p0 + i0 + lane;
			c = wsel_key(par, r->pair, r->len, r->t_first, r->t_last, &key);
		}
		if(held){ keys[i0 + lane] = key; mine |= (c ? 1u : 0u) << (uint32_t)(i0 >> 6); }
		C += (uint32_t)__popcll(__ballot(c));
	}
	uint64_t T = 0;
	uint32_t q = ~0u, sel = C;                                        // the cap does not bind: every candidate's key is T or above, and the quota never ends
	if(par.max_depth && C > par.max_depth){
		uint32_t k = par.max_depth;                                    // T is the k-th best of the keys under the prefix
		for(int shift = 56; shift >= 0; shift -= 8){
			const uint64_t above = shift == 56 ? 0ull : ~0ull << (shift + 8);
			hist_all[wave][lane] = make_uint4(0u, 0u, 0u, 0u);
			wsel_wave_sync();
			for(uint64_t i0 = 0; i0 < d; i0 += 64u){
				uint64_t key = 0;
				bool c = false;
				if(held){ key = keys[i0 + lane]; c = (mine >> (uint32_t)(i0 >> 6) & 1u) != 0u; }
				else if(i0 + lane < d){
					const bsa_piece_t *r = piece + p0 + i0 + lane;
					c = wsel_key(par, r->pair, r->len, r->t_first, r->t_last, &key);
				}
				if(c && (key & above) == T) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
			}
			wsel_wave_sync();
			// lane l has the digits 4 l .. 4 l + 3; the digit of the k-th best from the top
			const uint4 h = hist_all[wave][lane];
			const uint32_t s = h.x + h.y + h.z + h.w, incl = bsa_wave_iscan(s, lane);
			const uint32_t over = (uint32_t)__shfl((int)incl, 63) - incl;          // the keys in the digits of the lanes above
			const uint64_t has = __ballot(over < k && k - over <= s);              // (one lane: the keys under the prefix are k or more)
			const int src = has ? __ffsll((long long)has) - 1 : 0;
			uint32_t acc = over, dig = 3u;
			if(k - acc > h.w){ acc += h.w; dig = 2u; if(k - acc > h.z){ acc += h.z; dig = 1u; if(k - acc > h.y){ acc += h.y; dig = 0u; } } }
			dig = (uint32_t)__shfl((int)(4u * lane + dig), src);
			acc = (uint32_t)__shfl((int)acc, src);
			T |= (uint64_t)dig << shift;
			k -= acc;                                                 // acc keys under the old prefix have a larger digit: they are above T
			wsel_wave_sync();
		}
		q = k; sel = par.max_depth;
	}
	if(lane == 0u){
		thr[g] = T; quota[g] = q; cnt[g] = sel;
		if(ncand) ncand[g] = C;
	}
}

// a wave a window, four a workgroup.  V16: piece and sel are 16-byte aligned
template<bool V16>
__global__ void __launch_bounds__(256) k_window_select_fill(const bsa_piece_t *piece, const uint64_t *poff, uint32_t nwin, uint64_t pcap, wsel_par_t par,
		const uint64_t *thr, const uint32_t *quota, const uint64_t *soff, uint64_t scap, bsa_piece_t *sel, uint32_t *sel_src){
	const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6);
	if(g >= nwin) return;
	const uint64_t s0 = soff[g], s1 = soff[g + 1u];
	if(s1 > scap || s1 <= s0) return;
	uint64_t p0;
	const uint32_t d = wsel_depth(poff, g, pcap, &p0);
	const uint64_t T = thr[g], lt = (1ull << lane) - 1ull;
	const uint32_t q = quota[g];
	uint64_t at = s0;                                                 // where the next kept record goes
	uint32_t eqs = 0;                                                 // the candidates with key T in front of this trip
	for(uint64_t i0 = 0; i0 < d; i0 += 64u){
		const uint64_t i = p0 + i0 + lane;
		uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;                    // the record: pair, q_first, len, t_first | t_last, reserved, base_off
		uint64_t key = 0;
		bool c = false;
		if(i0 + lane < d){
			if(V16){ a = ((const uint4*)(piece + i))[0]; b = ((const uint4*)(piece + i))[1]; }
			else {
				const uint2 *v = (const uint2*)(piece + i);
				const uint2 v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
				a = make_uint4(v0.x, v0.y, v1.x, v1.y); b = make_uint4(v2.x, v2.y, v3.x, v3.y);
			}
			c = wsel_key(par, a.x, a.z, a.w, b.x, &key);
		}
		const bool e = c && key == T;
		const uint64_t E = __ballot(e);
		const bool keep = c && (key > T || (e && eqs + (uint32_t)__popcll(E & lt) < q));          // (no more than 0xFFFFFFF0 records: the sum does not wrap)
		const uint64_t K = __ballot(keep);
		const uint64_t p = at + (uint32_t)__popcll(K & lt);
		if(keep && p < s1){
			if(V16){ ((uint4*)(sel + p))[0] = a; ((uint4*)(sel + p))[1] = b; }
			else {
				uint2 *v = (uint2*)(sel + p);
				v[0] = make_uint2(a.x, a.y); v[1] = make_uint2(a.z, a.w); v[2] = make_uint2(b.x, b.y); v[3] = make_uint2(b.z, b.w);
			}
			if(sel_src) sel_src[p] = (uint32_t)i;
		}
		at += (uint32_t)__popcll(K);
		eqs += (uint32_t)__popcll(E);
	}
}

struct wsel_io_t { const bsa_piece_t *piece; const uint64_t *poff; size_t nwin, piece_cap; bsa_piece_t *sel; size_t sel_cap; uint64_t *soff; uint32_t *src, *ncand; };

// the argument errors of both calls; *kp: what the kernels take of the parameters
static int wsel_check(bsa_ctx_t *ctx, const wsel_io_t &a, const bsa_result_t *out, size_t n, const bsa_select_params_t *par, wsel_par_t *kp){
	const char *msg = nullptr;
	if(!par || !a.soff || (a.nwin && !a.poff) || (a.piece_cap && !a.piece) || (a.sel_cap && !a.sel)) msg = "bsa_window_select: null argument";
	else if(a.src && !a.sel) msg = "bsa_window_select: d_sel_src without d_sel";
	else if(par->reserved[0] || par->reserved[1] || par->reserved[2]) msg = "bsa_window_select: reserved parameters are not 0";
	else if(par->ident_den && !out) msg = "bsa_window_select: an identity test without d_out";
	else if(n > 0xFFFFFFF0ull) msg = "too many pairs";
	else if(a.nwin > 0xFFFFFFF0ull) msg = "too many windows";
	else if(a.piece_cap > 0xFFFFFFF0ull || a.sel_cap > 0xFFFFFFF0ull) msg = "bsa_window_select: piece_cap or sel_cap above 0xFFFFFFF0";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	const wsel_par_t k = { par->ident_den ? out : nullptr, (uint32_t)n, par->max_depth, par->min_span, par->ident_num, par->ident_den, par->seed };
	*kp = k;
	return BSA_OK;
}

// the steps of `steps`, in order (one alone only for tools/bench_window_select.py, on the scratch a whole run left); nwin > 0
static int wsel_run(bsa_ctx_t *ctx, hipStream_t st, int steps, const wsel_io_t &a, const wsel_par_t &kp){
	// scratch: T, the quota and the count of every window -- 16 bytes -- and the scan's temporaries
	const size_t o_thr = 0, o_quota = o_thr + bsa_up256(a.nwin * 8u), o_cnt = o_quota + bsa_up256(a.nwin * 4u), o_tmp = o_cnt + bsa_up256(a.nwin * 4u),
		total = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)a.nwin));
	void *bufv = nullptr;
	const int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);        // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	uint64_t *thr = (uint64_t*)(b + o_thr), *tmp = (uint64_t*)(b + o_tmp);
	uint32_t *quota = (uint32_t*)(b + o_quota), *cnt = (uint32_t*)(b + o_cnt);
	const dim3 grid((uint32_t)(((uint64_t)a.nwin + 3u) / 4u)), block(256);
	hipError_t e = hipSuccess;
	if(steps & WSEL_COUNT){
		hipLaunchKernelGGL(k_window_select_count, grid, block, 0, st, a.piece, a.poff, (uint32_t)a.nwin, (uint64_t)a.piece_cap, kp, thr, quota, cnt, a.ncand);
		e = hipGetLastError();
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)cnt, a.soff, (uint32_t)a.nwin, nullptr, tmp);
	}
	if(e == hipSuccess && (steps & WSEL_FILL) && a.sel_cap){
		if((((uintptr_t)a.piece | (uintptr_t)a.sel) & 15u) == 0u)
			hipLaunchKernelGGL((k_window_select_fill<true>), grid, block, 0, st, a.piece, a.poff, (uint32_t)a.nwin, (uint64_t)a.piece_cap, kp, (const uint64_t*)thr,
				(const uint32_t*)quota, (const uint64_t*)a.soff, (uint64_t)a.sel_cap, a.sel, a.src);
		else
			hipLaunchKernelGGL((k_window_select_fill<false>), grid, block, 0, st, a.piece, a.poff, (uint32_t)a.nwin, (uint64_t)a.piece_cap, kp, (const uint64_t*)thr,
				(const uint32_t*)quota, (const uint64_t*)a.soff, (uint64_t)a.sel_cap, a.sel, a.src);
		e = hipGetLastError();
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_select: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

static int wsel_run_checked(bsa_ctx_t *ctx, int steps, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const bsa_result_t *d_out, size_t n,
		const bsa_select_params_t *par, bsa_piece_t *d_sel, size_t sel_cap, uint64_t *d_sel_off, uint32_t *d_sel_src, uint32_t *d_ncand){
	if(!ctx) return BSA_E_ARG;
	const wsel_io_t a = { d_piece, d_piece_off, nwin, piece_cap, d_sel, sel_cap, d_sel_off, d_sel_src, d_ncand };
	wsel_par_t kp;
	int rc = wsel_check(ctx, a, d_out, n, par, &kp);
	if(rc != BSA_OK) return rc;
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	if(nwin == 0){
		if(bsa_launch_excl_scan(stream, (const uint32_t*)nullptr, d_sel_off, 0u, nullptr, nullptr) != hipSuccess){          // d_sel_off[0] = 0
			(void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_select: launch failed"); return BSA_E_HIP;
		}
		return BSA_OK;
	}
	return wsel_run(ctx, stream, steps, a, kp);
}

extern "C" int bsa_window_select_run(bsa_ctx_t *ctx, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap, const bsa_result_t *d_out, size_t n,
		const bsa_select_params_t *par, bsa_piece_t *d_sel, size_t sel_cap, uint64_t *d_sel_off, uint32_t *d_sel_src, uint32_t *d_ncand){
	return wsel_run_checked(ctx, WSEL_COUNT | WSEL_FILL, d_piece, d_piece_off, nwin, piece_cap, d_out, n, par, d_sel, sel_cap, d_sel_off, d_sel_src, d_ncand);
}

// for tools/bench_window_select.py: one step alone (step: 0 the count with its scan, 1 the fill), once more, with the arguments of the context's last
// bsa_window_select_run and on the scratch it left: nothing else may have used the context in between
extern "C" int bsa_window_select_step_internal(bsa_ctx_t *ctx, int step, const bsa_piece_t *d_piece, const uint64_t *d_piece_off, size_t nwin, size_t piece_cap,
		const bsa_result_t *d_out, size_t n, const bsa_select_params_t *par, bsa_piece_t *d_sel, size_t sel_cap, uint64_t *d_sel_off, uint32_t *d_sel_src, uint32_t *d_ncand){
	if(step < 0 || step > 1) return BSA_E_ARG;
	return wsel_run_checked(ctx, 1 << step, d_piece, d_piece_off, nwin, piece_cap, d_out, n, par, d_sel, sel_cap, d_sel_off, d_sel_src, d_ncand);
}

extern "C" int bsa_window_select_batch(bsa_ctx_t *ctx, const bsa_piece_t *piece, const uint64_t *piece_off, size_t nwin, size_t piece_cap, const bsa_result_t *out, size_t n,
		const bsa_select_params_t *par, bsa_piece_t *sel, size_t sel_cap, uint64_t *sel_off, uint32_t *sel_src, uint32_t *ncand){
	if(!ctx) return BSA_E_ARG;
	wsel_io_t a = { piece, piece_off, nwin, piece_cap, sel, sel_cap, sel_off, sel_src, ncand };
	wsel_par_t kp;
	int rc = wsel_check(ctx, a, out, n, par, &kp);
	if(rc != BSA_OK) return rc;
	if(nwin == 0){ sel_off[0] = 0; return BSA_OK; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	// the offsets go up as they are (a window whose offsets make no sense has no pieces), with all piece_cap records and, for the identity test, the n records
	bsa_stage_t in(ctx, stream), res(ctx, stream);
	const size_t o_piece = in.part(piece_cap * sizeof(bsa_piece_t)), o_poff = in.part((nwin + 1u) * 8u), o_out = in.part(kp.out ? n * sizeof(bsa_result_t) : 0u),
		o_soff = in.part((nwin + 1u) * 8u), o_nc = in.part(nwin * 4u);
	if((rc = in.alloc("bsa_window_select_batch: no device memory for the records")) != BSA_OK) return rc;
	if(!in.up(o_piece, piece, piece_cap * sizeof(bsa_piece_t)) || !in.up(o_poff, piece_off, (nwin + 1u) * 8u) || (kp.out && !in.up(o_out, out, n * sizeof(bsa_result_t))))
		return in.fail("bsa_window_select_batch: upload failed");
	if(kp.out) kp.out = in.at<bsa_result_t>(o_out);
	a.piece = in.at<bsa_piece_t>(o_piece); a.poff = in.at<uint64_t>(o_poff); a.soff = in.at<uint64_t>(o_soff); a.ncand = ncand ? in.at<uint32_t>(o_nc) : nullptr;
	a.sel = nullptr; a.sel_cap = 0; a.src = nullptr;
	if((rc = wsel_run(ctx, stream, WSEL_COUNT, a, kp)) != BSA_OK) return rc;
	if(!in.down(sel_off, o_soff, (nwin + 1u) * 8u) || (ncand && !in.down(ncand, o_nc, nwin * 4u)) || !in.sync()) return in.fail("bsa_window_select_batch: download of the offsets failed");
	const uint64_t need = sel_off[nwin];                                 // (the offsets are down before the capacity is judged)
	if(need > sel_cap) return in.fail("bsa_window_select_batch: sel_cap too small, sel_off[nwin] holds what is needed", BSA_E_CIGAR_CAP);
	if(need == 0) return BSA_OK;
	const size_t o_sel = res.part((size_t)need * sizeof(bsa_piece_t)), o_src = res.part(sel_src ? (size_t)need * 4u : 0u);
	if((rc = res.alloc("bsa_window_select_batch: no device memory for the selected records")) != BSA_OK) return rc;
	a.sel = res.at<bsa_piece_t>(o_sel); a.sel_cap = (size_t)need; a.src = sel_src ? res.at<uint32_t>(o_src) : nullptr;
	if((rc = wsel_run(ctx, stream, WSEL_FILL, a, kp)) != BSA_OK) return rc;
	if(!res.down(sel, o_sel, (size_t)need * sizeof(bsa_piece_t)) || (sel_src && !res.down(sel_src, o_src, (size_t)need * 4u)) || !res.sync())
		return res.fail("bsa_window_select_batch: download of the selected records failed");
	return BSA_OK;
}
