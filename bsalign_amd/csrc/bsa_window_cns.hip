// bsa_window_cns.hip -- bsa_cns_model_create / _destroy, bsa_window_cns_run / _batch (include/bsalign_hip.h): the consensus of every window's MSA
// where bsa_window_msa_run left it, and the windows' called bases packed into contiguous polished sequence.
//
// A pass over public outputs: the columns and the bsa_cns_window_t records of bsa_window_msa_run.  The automaton is bsa_cns_dev.hip's (k_cns_dp and
// k_cns_finish through bsa_cns_launch_internal, unchanged); this file decides on the device which windows it may touch and where their workspace
// lies.  The steps on the context stream:
//   prepare : a thread a window (k_window_cns_prepare) tests the clauses of the live predicate that need no sum, copies the record into the
//             context's scratch -- nothing reads the caller's record a second time -- and leaves mlen, or 0, for the scan;
//   scan    : bsa_scan.hip's exclusive scan of those values: t, the workspace cursor;
//   records : a thread a window (k_window_cns_records) finishes the predicate with t[g + 1], writes d_status and the automaton's record.  A dead
//             window's record has mlen 0 and no rows: k_cns_dp writes the start slot of its one workspace column and k_cns_finish clen 0, score 0;
//   dp, finish : bsa_cns_launch_internal;
//   pack    : the exclusive scan of d_clen into d_seq_off, then a wave a window (k_window_cns_pack) copies the window's called bases and both
//             quality strings to their place in the compact arrays.
// Workspace column of window g: min(t[g], W) + g, W = min(out_cap, cols_cap / 4) -- a live window has t[g + 1] <= W and owns the mlen + 1 columns
// from t[g] + g on; a dead one owns one column that lies in no live window's range (header: the live window).
// Plain C++; no kernel uses scratch memory.
#include "bsa_pass.h"
#include "bsa_cns_dev.h"

static_assert(sizeof(bsa_cns_window_t) == 40 && sizeof(CnsWinDev) == 56, "the records' layouts");

struct bsa_cns_model { bsa_ctx_t *ctx; uint8_t *buf; const CnsModelDev *d_model; const double *d_lf; };

struct wc_in_t { const bsa_cns_window_t *cwin; uint64_t cols_cap, out_cap, wcols, mass_base, org_base; uint32_t nwin, max_rows; };

// the clauses of the live predicate that need no sum, in the header's order -> the first that fails
static __device__ __forceinline__ uint32_t wc_clauses(const bsa_cns_window_t &w, const wc_in_t &in){
	if(w.idxs_off != ~0ull || w.nseq > w.nall || w.nmax > w.nall || w.mlen >= 0x80000000u) return BSA_CNS_ST_BAD_RECORD;
	const uint64_t stride = (uint64_t)w.nall + 3u, bytes = (uint64_t)w.mlen * stride;      // (below 2^31 (2^32 + 2): the product does not wrap)
	if(w.cols_off > ~0ull - bytes || w.out_off > ~0ull - (uint64_t)w.mlen) return BSA_CNS_ST_BAD_RECORD;
	if(w.nseq > in.max_rows) return BSA_CNS_ST_TOO_DEEP;
	if(w.cols_off + bytes > in.cols_cap || w.out_off + w.mlen > in.out_cap) return BSA_CNS_ST_NO_ROOM;
	return BSA_CNS_ST_OK;
}

__global__ void __launch_bounds__(256) k_window_cns_prepare(const wc_in_t in, CnsWinDev *wd, uint32_t *stv, uint32_t *mlenv){
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if(g >= in.nwin) return;
	const bsa_cns_window_t w = in.cwin[g];
	const uint32_t st = wc_clauses(w, in);
	CnsWinDev d;
	d.cols_off = w.cols_off; d.idxs_off = ~0ull; d.out_off = w.out_off; d.mass_off = 0; d.org_off = 0;
	d.nall = w.nall; d.nseq = w.nseq; d.nmax = w.nmax; d.mlen = w.mlen;
	wd[g] = d; stv[g] = st; mlenv[g] = st == BSA_CNS_ST_OK ? w.mlen : 0u;
}

__global__ void __launch_bounds__(256) k_window_cns_records(const wc_in_t in, const uint64_t *t, CnsWinDev *wd, uint32_t *stv, uint32_t *status){
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if(g >= in.nwin) return;
	uint32_t st = stv[g];
	const uint64_t t0 = t[g], t1 = t[g + 1u];
	if(st == BSA_CNS_ST_OK && t1 > in.wcols) st = BSA_CNS_ST_NO_ROOM;
	const uint64_t col = (t0 < in.wcols ? t0 : in.wcols) + g;             // (a live window: t0 <= t1 <= wcols, its columns end at t1 + g + 1 <= wcols + nwin)
	CnsWinDev d = wd[g];
	if(st != BSA_CNS_ST_OK){ d.cols_off = 0; d.out_off = 0; d.nall = 0; d.nseq = 0; d.nmax = 0; d.mlen = 0; }
	d.mass_off = in.mass_base + col * 40u; d.org_off = in.org_base + col * 2u;
	wd[g] = d; stv[g] = st;
	if(status) status[g] = st;
}

// n bytes in units of V where dst and src are both aligned to V, single bytes in front and behind: coalesced over the wave either way
template<typename V>
static __device__ __forceinline__ void wc_copy_as(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane){
	uint32_t head = (uint32_t)((0u - (uintptr_t)dst) & (sizeof(V) - 1u));
	if(head > n) head = n;
	const uint32_t nv = (n - head) / (uint32_t)sizeof(V), tail = head + nv * (uint32_t)sizeof(V);
	for(uint32_t i = lane; i < head; i += 64u) dst[i] = src[i];
	for(uint32_t i = lane; i < nv; i += 64u) ((V*)(dst + head))[i] = ((const V*)(src + head))[i];
	for(uint32_t i = tail + lane; i < n; i += 64u) dst[i] = src[i];
}
// the widest unit the two addresses share: 16 bytes where they are congruent modulo 16, 4 modulo 4, else bytes
static __device__ __forceinline__ void wc_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane){
	const uint32_t rel = (uint32_t)(((uintptr_t)dst ^ (uintptr_t)src) & 15u);
	if(rel == 0u) wc_copy_as<uint4>(dst, src, n, lane);
	else if((rel & 3u) == 0u) wc_copy_as<uint32_t>(dst, src, n, lane);
	else for(uint32_t i = lane; i < n; i += 64u) dst[i] = src[i];
}

// a wave a window, four a workgroup.  The source range comes from the scratch record (tested by the predicate), the length from the pass's own offsets.
__global__ void __launch_bounds__(256) k_window_cns_pack(uint32_t nwin, const CnsWinDev *wd, const uint64_t *seq_off, uint64_t seq_cap, const uint8_t *cns, const uint8_t *qlt,
		const uint8_t *alt, uint8_t *seq, uint8_t *seq_qlt, uint8_t *seq_alt){
	const uint32_t lane = threadIdx.x & 63u;
	for(uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); g < nwin; g += (uint64_t)gridDim.x * 4u){
		const uint64_t s0 = seq_off[g], s1 = seq_off[g + 1u];
		if(s1 > seq_cap || s1 <= s0 || s1 - s0 > wd[g].mlen) continue;     // (clen <= mlen: k_cns_finish counts the window's own columns)
		const uint32_t n = (uint32_t)(s1 - s0);
		const uint64_t o = wd[g].out_off;
		wc_copy(seq + s0, cns + o, n, lane);
		if(seq_qlt) wc_copy(seq_qlt + s0, qlt + o, n, lane);
		if(seq_alt) wc_copy(seq_alt + s0, alt + o, n, lane);
	}
}

extern "C" int bsa_cns_model_create(bsa_ctx_t *ctx, const bsa_cns_params_t *par, bsa_cns_model_t **out){
	if(out) *out = nullptr;
	if(!ctx) return BSA_E_ARG;
	if(!par || !out){ bsa_ctx_set_error_internal(ctx, "bsa_cns_model_create: null argument"); return BSA_E_ARG; }
	hipStream_t stream;
	int rc = bsa_ctx_get_stream_internal(ctx, &stream);                  // (also selects the context's device)
	if(rc != BSA_OK) return rc;
	CnsModelDev mod; std::vector<double> lf;
	try { lf.resize(BSA_CNS_LF_FULL); } catch(...){ return BSA_E_NOMEM; }
	bsa_cns_model_fill_internal(par, &mod, lf.data(), BSA_CNS_LF_FULL);   // (lf[k] is a running sum from 0: it does not depend on the table's length)
	bsa_cns_model *m = new (std::nothrow) bsa_cns_model();
	if(!m) return BSA_E_NOMEM;
	const size_t o_lf = bsa_up256(sizeof(CnsModelDev));
	if(hipMalloc((void**)&m->buf, o_lf + BSA_CNS_LF_FULL * sizeof(double)) != hipSuccess){
		(void)hipGetLastError(); delete m; bsa_ctx_set_error_internal(ctx, "bsa_cns_model_create: no device memory"); return BSA_E_NOMEM;
	}
	if(hipMemcpy(m->buf, &mod, sizeof(CnsModelDev), hipMemcpyHostToDevice) != hipSuccess
			|| hipMemcpy(m->buf + o_lf, lf.data(), BSA_CNS_LF_FULL * sizeof(double), hipMemcpyHostToDevice) != hipSuccess){
		(void)hipGetLastError(); (void)hipFree(m->buf); delete m; bsa_ctx_set_error_internal(ctx, "bsa_cns_model_create: upload failed"); return BSA_E_HIP;
	}
	m->ctx = ctx; m->d_model = (const CnsModelDev*)m->buf; m->d_lf = (const double*)(m->buf + o_lf);
	*out = m;
	return BSA_OK;
}

extern "C" void bsa_cns_model_destroy(bsa_cns_model_t *m){
	if(!m) return;
	if(m->buf) (void)hipFree(m->buf);
	delete m;
}

// the argument errors of both calls (model: the run's model or the batch's parameters)
static int wc_check(bsa_ctx_t *ctx, const void *model, const void *cols, size_t cols_cap, const void *cwin, size_t nwin, const void *cns, const void *qlt, const void *alt,
		size_t out_cap, const void *clen, const void *seq, const void *seq_qlt, const void *seq_alt, size_t seq_cap, const void *seq_off){
	const char *msg = nullptr;
	if(!model || (nwin && (!cwin || !clen || !cns || !qlt || !alt)) || (cols_cap && !cols) || (out_cap && (!cns || !qlt || !alt)) || (seq_cap && !seq))
		msg = "bsa_window_cns: null argument";
	else if(!seq_off && (seq || seq_qlt || seq_alt || seq_cap)) msg = "bsa_window_cns: compact arrays or seq_cap without seq_off";
	else if(nwin > 0xFFFFFFF0ull) msg = "too many windows";
	if(msg){ bsa_ctx_set_error_internal(ctx, msg); return BSA_E_ARG; }
	return BSA_OK;
}

enum { WC_PREPARE = 1, WC_DP = 2, WC_FINISH = 4, WC_PACK = 8 };
// the steps of `steps`, in order (one alone only for tools/bench_window_cns.py, on the scratch a whole run left)
static int wc_run(bsa_ctx_t *ctx, hipStream_t st, int steps, const CnsModelDev *d_model, const double *d_lf, uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
		uint32_t max_rows, uint8_t *d_cns, uint8_t *d_qlt, uint8_t *d_alt, size_t out_cap, uint32_t *d_clen, double *d_score, uint32_t *d_status,
		uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off){
	if(bsa_cns_lds_bytes(max_rows, nullptr) > BSA_CNS_LDS_MAX){ bsa_ctx_set_error_internal(ctx, "bsa_window_cns: max_rows needs more than 160 KB of LDS"); return BSA_E_UNSUPPORTED; }
	hipError_t e = hipSuccess;
	if(nwin == 0){
		if(d_seq_off && (steps & WC_PACK)) e = bsa_launch_excl_scan(st, (const uint32_t*)nullptr, d_seq_off, 0u, nullptr, nullptr);      // d_seq_off[0] = 0
		if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_cns: launch failed"); return BSA_E_HIP; }
		return BSA_OK;
	}
	// scratch: the records, statuses, scan values and sums, a score array for a caller without one; then 40 + 2 bytes a workspace column
	const uint64_t wcols = std::min<uint64_t>(out_cap, cols_cap / 4u);
	if(wcols > ((uint64_t)1 << 40)){ bsa_ctx_set_error_internal(ctx, "bsa_window_cns: no scratch for caps this large"); return BSA_E_NOMEM; }
	const size_t ncol = (size_t)wcols + nwin;
	const size_t o_wd = 0, o_st = o_wd + bsa_up256(nwin * sizeof(CnsWinDev)), o_mlen = o_st + bsa_up256(nwin * 4u), o_t = o_mlen + bsa_up256(nwin * 4u),
		o_tmp = o_t + bsa_up256((nwin + 1u) * 8u), o_score = o_tmp + bsa_up256(bsa_excl_scan_tmp_bytes((uint32_t)nwin)), o_mass = o_score + bsa_up256(nwin * 8u),
		o_org = o_mass + bsa_up256(ncol * 40u), total = o_org + bsa_up256(ncol * 2u);
	void *bufv = nullptr;
	int rc = bsa_ctx_scratch_internal(ctx, 1, total, &bufv);              // (waits for the stream only when it has to grow)
	if(rc != BSA_OK) return rc;
	uint8_t *b = (uint8_t*)bufv;
	CnsWinDev *wd = (CnsWinDev*)(b + o_wd);
	uint32_t *stv = (uint32_t*)(b + o_st), *mlenv = (uint32_t*)(b + o_mlen);
	uint64_t *t = (uint64_t*)(b + o_t), *tmp = (uint64_t*)(b + o_tmp);
	const wc_in_t in = { d_cwin, (uint64_t)cols_cap, (uint64_t)out_cap, wcols, (uint64_t)o_mass, (uint64_t)o_org, (uint32_t)nwin, max_rows };
	const dim3 grid((uint32_t)(((uint64_t)nwin + 255u) / 256u));
	if(steps & WC_PREPARE){
		hipLaunchKernelGGL(k_window_cns_prepare, grid, dim3(256), 0, st, in, wd, stv, mlenv);
		e = hipGetLastError();
		if(e == hipSuccess) e = bsa_launch_excl_scan(st, (const uint32_t*)mlenv, t, (uint32_t)nwin, nullptr, tmp);
		if(e == hipSuccess){
			hipLaunchKernelGGL(k_window_cns_records, grid, dim3(256), 0, st, in, (const uint64_t*)t, wd, stv, d_status);
			e = hipGetLastError();
		}
	}
	if(e == hipSuccess && (steps & (WC_DP | WC_FINISH))){
		rc = bsa_cns_launch_internal(st, d_cols, nullptr, wd, nwin, d_model, d_lf, b, max_rows, d_cns, d_qlt, d_alt, d_clen, d_score ? d_score : (double*)(b + o_score),
			((steps & WC_DP) ? 1 : 0) | ((steps & WC_FINISH) ? 2 : 0));
		if(rc != BSA_OK){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_cns: launch of the automaton failed"); return rc; }
	}
	if(e == hipSuccess && (steps & WC_PACK) && d_seq_off){
		e = bsa_launch_excl_scan(st, (const uint32_t*)d_clen, d_seq_off, (uint32_t)nwin, nullptr, tmp);
		if(e == hipSuccess && seq_cap){
			const size_t want = (nwin + 3u) / 4u, most = (size_t)bsa_cus() * 16u;
			hipLaunchKernelGGL(k_window_cns_pack, dim3((uint32_t)(want < most ? want : most)), dim3(256), 0, st, (uint32_t)nwin, (const CnsWinDev*)wd, (const uint64_t*)d_seq_off,
				(uint64_t)seq_cap, (const uint8_t*)d_cns, (const uint8_t*)d_qlt, (const uint8_t*)d_alt, d_seq, d_seq_qlt, d_seq_alt);
			e = hipGetLastError();
		}
	}
	if(e != hipSuccess){ (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, "bsa_window_cns: launch failed"); return BSA_E_HIP; }
	return BSA_OK;
}

static int wc_run_checked(bsa_ctx_t *ctx, int steps, const bsa_cns_model_t *model, uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin, uint32_t max_rows,
		uint8_t *d_cns, uint8_t *d_qlt, uint8_t *d_alt, size_t out_cap, uint32_t *d_clen, double *d_score, uint32_t *d_status,
		uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off){
	if(!ctx) return BSA_E_ARG;
	int rc = wc_check(ctx, model, d_cols, cols_cap, d_cwin, nwin, d_cns, d_qlt, d_alt, out_cap, d_clen, d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off);
	if(rc != BSA_OK) return rc;
	if(model->ctx != ctx){ bsa_ctx_set_error_internal(ctx, "bsa_window_cns_run: the model belongs to another context"); return BSA_E_ARG; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;          // (also selects the context's device)
	return wc_run(ctx, stream, steps, model->d_model, model->d_lf, d_cols, cols_cap, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, d_score, d_status,
		d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off);
}

extern "C" int bsa_window_cns_run(bsa_ctx_t *ctx, const bsa_cns_model_t *model, uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin, uint32_t max_rows,
		uint8_t *d_cns, uint8_t *d_qlt, uint8_t *d_alt, size_t out_cap, uint32_t *d_clen, double *d_score, uint32_t *d_status,
		uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off){
	return wc_run_checked(ctx, WC_PREPARE | WC_DP | WC_FINISH | WC_PACK, model, d_cols, cols_cap, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, d_score, d_status,
		d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off);
}

// for tools/bench_window_cns.py: one step alone (step: 0 prepare with its scan and the records, 1 k_cns_dp, 2 k_cns_finish, 3 the pack with its scan), once
// more, with the arguments of the context's last bsa_window_cns_run and on the scratch it left: nothing else may have used the context in between
extern "C" int bsa_window_cns_step_internal(bsa_ctx_t *ctx, int step, const bsa_cns_model_t *model, uint8_t *d_cols, size_t cols_cap, const bsa_cns_window_t *d_cwin, size_t nwin,
		uint32_t max_rows, uint8_t *d_cns, uint8_t *d_qlt, uint8_t *d_alt, size_t out_cap, uint32_t *d_clen, double *d_score, uint32_t *d_status,
		uint8_t *d_seq, uint8_t *d_seq_qlt, uint8_t *d_seq_alt, size_t seq_cap, uint64_t *d_seq_off){
	if(step < 0 || step > 3) return BSA_E_ARG;
	return wc_run_checked(ctx, 1 << step, model, d_cols, cols_cap, d_cwin, nwin, max_rows, d_cns, d_qlt, d_alt, out_cap, d_clen, d_score, d_status,
		d_seq, d_seq_qlt, d_seq_alt, seq_cap, d_seq_off);
}

// the batch's model goes when everything declared behind it has gone (the stages wait for the stream before they free)
struct wc_model_guard { bsa_cns_model_t *m = nullptr; ~wc_model_guard(){ bsa_cns_model_destroy(m); } };

extern "C" int bsa_window_cns_batch(bsa_ctx_t *ctx, const bsa_cns_params_t *par, uint8_t *cols, size_t cols_cap, const bsa_cns_window_t *cwin, size_t nwin, uint32_t max_rows,
		uint8_t *cns, uint8_t *qlt, uint8_t *alt, size_t out_cap, uint32_t *clen, double *score, uint32_t *status,
		uint8_t *seq, uint8_t *seq_qlt, uint8_t *seq_alt, size_t seq_cap, uint64_t *seq_off){
	if(!ctx) return BSA_E_ARG;
	int rc = wc_check(ctx, par, cols, cols_cap, cwin, nwin, cns, qlt, alt, out_cap, clen, seq, seq_qlt, seq_alt, seq_cap, seq_off);
	if(rc != BSA_OK) return rc;
	if(bsa_cns_lds_bytes(max_rows, nullptr) > BSA_CNS_LDS_MAX){ bsa_ctx_set_error_internal(ctx, "bsa_window_cns: max_rows needs more than 160 KB of LDS"); return BSA_E_UNSUPPORTED; }
	if(nwin == 0){ if(seq_off) seq_off[0] = 0; return BSA_OK; }
	hipStream_t stream;
	if((rc = bsa_ctx_get_stream_internal(ctx, &stream)) != BSA_OK) return rc;
	wc_model_guard mg;
	if((rc = bsa_cns_model_create(ctx, par, &mg.m)) != BSA_OK) return rc;
	// the output arrays go up as they are: a range no window owns comes down as it went up
	bsa_stage_t in(ctx, stream);
	const size_t o_cols = in.part(cols_cap), o_cwin = in.part(nwin * sizeof(bsa_cns_window_t)), o_cns = in.part(out_cap), o_qlt = in.part(out_cap), o_alt = in.part(out_cap),
		o_clen = in.part(nwin * 4u), o_score = in.part(nwin * 8u), o_status = in.part(nwin * 4u), o_soff = in.part((nwin + 1u) * 8u),
		o_seq = in.part(seq_cap), o_sq = in.part(seq_qlt ? seq_cap : 0u), o_sa = in.part(seq_alt ? seq_cap : 0u);
	if((rc = in.alloc("bsa_window_cns_batch: no device memory for the columns, the records and the outputs")) != BSA_OK) return rc;
	if(!in.up(o_cols, cols, cols_cap) || !in.up(o_cwin, cwin, nwin * sizeof(bsa_cns_window_t)) || !in.up(o_cns, cns, out_cap) || !in.up(o_qlt, qlt, out_cap) || !in.up(o_alt, alt, out_cap))
		return in.fail("bsa_window_cns_batch: upload failed");
	rc = wc_run(ctx, stream, WC_PREPARE | WC_DP | WC_FINISH | WC_PACK, mg.m->d_model, mg.m->d_lf, cols_cap ? in.at<uint8_t>(o_cols) : nullptr, cols_cap, in.at<bsa_cns_window_t>(o_cwin), nwin,
		max_rows, in.at<uint8_t>(o_cns), in.at<uint8_t>(o_qlt), in.at<uint8_t>(o_alt), out_cap, in.at<uint32_t>(o_clen), in.at<double>(o_score), in.at<uint32_t>(o_status),
		seq_cap ? in.at<uint8_t>(o_seq) : nullptr, (seq_cap && seq_qlt) ? in.at<uint8_t>(o_sq) : nullptr, (seq_cap && seq_alt) ? in.at<uint8_t>(o_sa) : nullptr, seq_cap,
		seq_off ? in.at<uint64_t>(o_soff) : nullptr);
	if(rc != BSA_OK) return rc;
	if(!in.down(clen, o_clen, nwin * 4u) || (score && !in.down(score, o_score, nwin * 8u)) || (status && !in.down(status, o_status, nwin * 4u))
			|| (seq_off && !in.down(seq_off, o_soff, (nwin + 1u) * 8u)) || !in.sync())
		return in.fail("bsa_window_cns_batch: download of the lengths and offsets failed");
	const uint64_t need = seq_off ? seq_off[nwin] : 0ull;              // (the offsets are down before the capacity is judged)
	if(need > seq_cap) return in.fail("bsa_window_cns_batch: seq_cap too small, seq_off[nwin] holds the bytes needed", BSA_E_CIGAR_CAP);
	if(!in.down(cols, o_cols, cols_cap) || !in.down(cns, o_cns, out_cap) || !in.down(qlt, o_qlt, out_cap) || !in.down(alt, o_alt, out_cap)
			|| !in.down(seq, o_seq, (size_t)need) || (seq_qlt && !in.down(seq_qlt, o_sq, (size_t)need)) || (seq_alt && !in.down(seq_alt, o_sa, (size_t)need)) || !in.sync())
		return in.fail("bsa_window_cns_batch: download of the results failed");
	return BSA_OK;
}
