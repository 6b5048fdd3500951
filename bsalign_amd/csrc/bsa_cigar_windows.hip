// bsa_cigar_windows.hip -- bsa_cigar_windows_run / _batch (include/bsalign_hip.h): every alignment cut at the borders of windows of `w` target
// bases, a record of the first and the last aligned column for every window it crosses.
//
// A pass over the PUBLIC outputs of a run -- the records, the CIGAR arena and its offsets -- and nothing else: it knows no plan, no slot and
// no walker, so it serves both aligners, plain and = / X words, stranded pairs and every kernel route.  Three steps on the context stream:
//   count : one thread a pair reads the record and its two offsets, cnt[k] = the pair's windows (k_cigar_windows_count);
//   scan  : the 64-bit exclusive scan of bsa_scan.hip into the caller's d_win_off;
//   fill  : one wave a pair (k_cigar_windows_fill).  Words in tiles of 64, a lane a word, wave prefix sums give every lane the target and
//           query position at its word (bsa_pass.h, as in bsa_cigar_eqx.hip and bsa_band_margin.hip).  `pe`, the last diagonal column seen so far, is
//           carried from tile to tile; inside a tile a diagonal word finds its predecessor's last column with one ballot and two lane-indexed
//           shuffles.  A diagonal word that starts in a later window than its predecessor ends writes `last` of that window, NONE into
//           the windows in between and `first` of its own; the pair's first diagonal word writes NONE into the windows in front of it;
//           then the word loops over the borders inside itself (last = (m w - 1, ..), first = (m w, ..): two identical 10 kbp reads at
//           w = 500 are one lane's loop of 19 trips).  After the last tile the wave writes `last` of pe's window and NONE behind it.
//           So every field of every record of the pair is written exactly once: no atomics, no pre-fill a later store is ordered against.
// Target positions are summed in 64 bits (64 words of 2^28 bases overflow 32), query positions wrap in 32: they are never compared.
//
// No LDS in the count and fill kernels, no scratch; plain C++ with vector loads and stores only.
#include "bsa_pass.h"
#include <algorithm>
#include <vector>

#define CW_T_LIMIT 0x80000000ull     // a record's target positions are int32: a column at or above 2^31 belongs to no window

// the windows of one pair (the definition's "window count"); c: its words
static __device__ __forceinline__ uint32_t cw_count(int32_t tb, int32_t te, uint64_t c, uint32_t w){
	if(tb < 0 || te <= tb || c == 0u) return 0u;
	return ((uint32_t)te - 1u) / w - (uint32_t)tb / w + 1u;
}

__global__ void __launch_bounds__(256) k_cigar_windows_count(const bsa_result_t *out, const uint64_t *coff, uint32_t n, uint32_t w, uint32_t *cnt){
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if(k >= n) return;
	const uint64_t a = coff[k], b = coff[k + 1u];
	cnt[k] = cw_count(out[k].tb, out[k].te, b > a ? b - a : 0ull, w);
}

// record r of a pair that has nw of them at rec: the three kinds of store.  r < nw holds by construction (see the kernel); the comparison
// stays so that no arithmetic slip can ever write outside the pair's own records.
static __device__ __forceinline__ void cw_first(bsa_window_t *rec, uint32_t nw, uint32_t r, uint32_t t, uint32_t q){
	if(r < nw){ rec[r].t_first = t; rec[r].q_first = q; }
}
static __device__ __forceinline__ void cw_last(bsa_window_t *rec, uint32_t nw, uint32_t r, uint32_t t, uint32_t q){
	if(r < nw){ rec[r].t_last = t; rec[r].q_last = q; }
}
static __device__ __forceinline__ void cw_none(bsa_window_t *rec, uint32_t nw, uint32_t r){
	if(r < nw){ bsa_window_t x; x.t_first = x.q_first = x.t_last = x.q_last = BSA_WINDOW_NONE; rec[r] = x; }
}

// one wave a pair.  A pair is written whole or not at all: when its range ends inside the arena (woff[k + 1] <= cap), so with cap == 0
// `win` is never dereferenced (it may be NULL: a count-only run).
__global__ void __launch_bounds__(256) k_cigar_windows_fill(const bsa_result_t *out, const uint32_t *cigar, const uint64_t *coff, uint32_t n, uint32_t w,
		bsa_window_t *win, uint64_t cap, const uint64_t *woff){
	const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
	if(g >= n) return;
	const uint64_t base = woff[g], end = woff[g + 1u];
	if(end <= base || end > cap) return;
	const int32_t tbs = out[g].tb, tes = out[g].te;
	const uint64_t c0 = coff[g], c1 = coff[g + 1u];
	const uint64_t c = c1 > c0 ? c1 - c0 : 0ull;
	const uint32_t nw = cw_count(tbs, tes, c, w);
	if((uint64_t)nw != end - base) return;                     // (the offsets are this pass's own scan of the same counts)
	const uint32_t tb = (uint32_t)tbs, m0 = tb / w, m1 = ((uint32_t)tes - 1u) / w;
	// columns count up to the end of window m1 (the words are the caller's own: they may run on behind the record's te)
	const uint64_t lim = min(((uint64_t)m1 + 1u) * w, (uint64_t)CW_T_LIMIT);
	bsa_window_t *rec = win + base;
	const uint32_t *src = cigar + c0;
	uint64_t tp = tb; uint32_t qp = (uint32_t)out[g].qb;       // the positions in front of the tile
	bool have = false; uint32_t pt = 0, pq = 0;                // pe: the last diagonal column so far (the same in every lane)
	for(uint64_t w0 = 0; w0 < c && tp < lim; w0 += 64u){
		const uint64_t idx = w0 + lane;
		const uint32_t word = idx < c ? src[idx] : 0u;
		const uint32_t op = word & 15u, len = word >> 4;
		const bool dg = bsa_cig_diag(op);
		const uint32_t qa = bsa_cig_qadd(op, len);
		const uint64_t ta = bsa_cig_tadd<uint64_t>(op, len);
		const uint32_t qi = bsa_wave_iscan(qa, lane);
		const uint64_t ti = bsa_wave_iscan(ta, lane);
		const uint64_t ts64 = tp + ti - ta;                    // where this lane's word starts
		const uint32_t qs = qp + qi - qa;
		const bool act = dg && len != 0u && ts64 < lim;        // a word with a column that counts
		const uint32_t ts = (uint32_t)ts64;
		const uint32_t el = act ? (uint32_t)min((uint64_t)len, lim - ts64) : 1u;      // its columns that count
		const uint32_t lt = ts + el - 1u, lq = qs + el - 1u;   // its last column
		const uint64_t mask = __ballot(act);
		const uint64_t lower = mask & ((1ull << lane) - 1ull);
		const int P = lower ? 63 - __clzll((long long)lower) : 0;      // the diagonal word in front of this one, if the tile has one
		const uint32_t st = __shfl(lt, P), sq = __shfl(lq, P);
		const bool hp = lower != 0ull || have;
		const uint32_t ppt = lower ? st : pt, ppq = lower ? sq : pq;
		if(act){
			const uint32_t mf = ts / w, ml = lt / w;
			if(!hp){
				for(uint32_t m = m0; m < mf; m++) cw_none(rec, nw, m - m0);
				cw_first(rec, nw, mf - m0, ts, qs);
			} else {
				const uint32_t mp = ppt / w;
				if(mf > mp){
					cw_last(rec, nw, mp - m0, ppt, ppq);
					for(uint32_t m = mp + 1u; m < mf; m++) cw_none(rec, nw, m - m0);
					cw_first(rec, nw, mf - m0, ts, qs);
				}
			}
			for(uint32_t m = mf + 1u; m <= ml; m++){           // the borders inside the word
				const uint32_t b = m * w;                      // (<= lt < 2^31)
				cw_last(rec, nw, m - 1u - m0, b - 1u, qs + (b - 1u - ts));
				cw_first(rec, nw, m - m0, b, qs + (b - ts));
			}
		}
		if(mask){
			const int H = 63 - __clzll((long long)mask);
			pt = __shfl(lt, H); pq = __shfl(lq, H); have = true;
		}
		tp += __shfl(ti, 63); qp += __shfl(qi, 63);
	}
	// `last` of pe's window, NONE behind it (a lane a window)
	uint32_t mn = m0;
	if(have){
		const uint32_t mp = pt / w;
		if(lane == 0) cw_last(rec, nw, mp - m0, pt, pq);
		mn = mp + 1u;
	}
	for(uint64_t m = (uint64_t)mn + lane; m <= m1; m += 64u) cw_none(rec, nw, (uint32_t)m - m0);
}

extern "C" uint64_t bsa_cigar_windows_bound(const uint32_t *tlen, size_t n, uint32_t window){
	uint64_t s = 0;
	if(tlen && window) for(size_t k = 0; k < n; k++) s += ((uint64_t)tlen[k] + window - 1u) / window;
	return s;
}

// count and scan: d_win_off[0 .. n] on the stream; *cnt_out: the counts in the context's scratch
static int cw_offsets(bsa_ctx_t *ctx, hipStream_t stream, const bsa_result_t *d_out, const uint64_t *d_cigar_off, size_t n, uint32_t window, uint64_t *d_win_off){
	const size_t o_tmp = bsa_up256(n * 4u);
	void *bufv = nullptr;
	int rc = bsa_ctx_scratch_internal(ctx, 1, o_tmp + bsa_excl_scan_tmp_bytes((uint32_t)n), &bufv);      // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint32_t *cnt = (uint32_t*)bufv;
	if(n) hipLaunchKernelGGL(k_cigar_windows_count, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, d_out, d_cigar_off, (uint32_t)n, window, cnt);
	if(hipGetLastError() != hipSuccess || bsa_launch_excl_scan(stream, cnt, d_win_off, (uint32_t)n, nullptr, (uint64_t*)((uint8_t*)bufv + o_tmp)) != hipSuccess){
		(void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows: launch failed"); return BSA_E_HIP;
	}
	return BSA_OK;
}
static int cw_fill(bsa_ctx_t *ctx, hipStream_t stream, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off, size_t n, uint32_t window,
		bsa_window_t *d_win, size_t win_cap, const uint64_t *d_win_off){
	if(n == 0 || win_cap == 0) return BSA_OK;
	hipLaunchKernelGGL(k_cigar_windows_fill, dim3((uint32_t)((n + 3u) / 4u)), dim3(256), 0, stream, d_out, d_cigar, d_cigar_off, (uint32_t)n, window, d_win, (uint64_t)win_cap, d_win_off);
	if(hipGetLastError() != hipSuccess){ bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

extern "C" int bsa_cigar_windows_run(bsa_ctx_t *ctx, const bsa_result_t *d_out, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
		size_t n, uint32_t window, bsa_window_t *d_win, size_t win_cap, uint64_t *d_win_off){
	if(!ctx) return BSA_E_ARG;
	if(window == 0){ bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows_run: window == 0"); return BSA_E_ARG; }
	if(!d_win_off || (n && (!d_out || !d_cigar || !d_cigar_off)) || (win_cap && !d_win)){ bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows_run: null argument"); return BSA_E_ARG; }
	if(n > 0xFFFFFFF0ull){ bsa_ctx_set_error_internal(ctx, "too many pairs"); return BSA_E_ARG; }
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);        // (also selects the context's device)
	if(rc != BSA_OK) return rc;
	if((rc = cw_offsets(ctx, stream, d_out, d_cigar_off, n, window, d_win_off)) != BSA_OK) return rc;
	return cw_fill(ctx, stream, d_out, d_cigar, d_cigar_off, n, window, d_win, win_cap, d_win_off);
}

extern "C" int bsa_cigar_windows_batch(bsa_ctx_t *ctx, const bsa_result_t *out, const uint32_t *cigar, const uint64_t *cigar_off,
		size_t n, uint32_t window, bsa_window_t *win, size_t win_cap, uint64_t *win_off){
	if(!ctx) return BSA_E_ARG;
	if(window == 0){ bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows_batch: window == 0"); return BSA_E_ARG; }
	if(!win_off || (n && (!out || !cigar_off)) || (win_cap && !win)){ bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows_batch: null argument"); return BSA_E_ARG; }
	if(n > 0xFFFFFFF0ull){ bsa_ctx_set_error_internal(ctx, "too many pairs"); return BSA_E_ARG; }
	if(n == 0){ win_off[0] = 0; return BSA_OK; }
	std::vector<uint64_t> coff;
	int rc = bsa_rebase_offsets(ctx, cigar_off, n, coff, "bsa_cigar_windows_batch: cigar_off decreases");
	if(rc != BSA_OK) return rc;
	const uint64_t w0 = cigar_off[0], words = coff[n];                    // only the words the offsets speak of go up
	if(words && !cigar){ bsa_ctx_set_error_internal(ctx, "bsa_cigar_windows_batch: null argument"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	bsa_stage_t in(ctx, stream), res(ctx, stream);
	const size_t o_out = in.part(n * sizeof(bsa_result_t)), o_coff = in.part((n + 1) * 8), o_woff = in.part((n + 1) * 8), o_cig = in.part(words * 4 + 4);
	if((rc = in.alloc("bsa_cigar_windows_batch: no device memory for the records and words")) != BSA_OK) return rc;
	if(!in.up(o_out, out, n * sizeof(bsa_result_t)) || !in.up(o_coff, coff.data(), (n + 1) * 8) || !in.up(o_cig, words ? cigar + w0 : nullptr, words * 4)) return in.fail("bsa_cigar_windows_batch: upload failed");
	const bsa_result_t *d_out = in.at<bsa_result_t>(o_out);
	const uint64_t *d_coff = in.at<uint64_t>(o_coff);
	uint64_t *d_woff = in.at<uint64_t>(o_woff);
	if((rc = cw_offsets(ctx, stream, d_out, d_coff, n, window, d_woff)) != BSA_OK) return rc;
	if(!in.down(win_off, o_woff, (n + 1) * 8) || !in.sync()) return in.fail("bsa_cigar_windows_batch: download of the offsets failed");
	const uint64_t need = win_off[n];                                     // (the offsets are down before the capacity is judged)
	if(need > win_cap) return in.fail("bsa_cigar_windows_batch: win_cap too small, win_off[n] holds the records needed", BSA_E_CIGAR_CAP);
	if(need == 0) return BSA_OK;
	const size_t o_win = res.part(need * sizeof(bsa_window_t));
	if((rc = res.alloc("bsa_cigar_windows_batch: no device memory for the windows")) != BSA_OK) return rc;
	if((rc = cw_fill(ctx, stream, d_out, in.at<uint32_t>(o_cig), d_coff, n, window, res.at<bsa_window_t>(o_win), need, d_woff)) != BSA_OK) return rc;
	if(!res.down(win, o_win, need * sizeof(bsa_window_t)) || !res.sync()) return res.fail("bsa_cigar_windows_batch: download of the windows failed");
	return BSA_OK;
}
