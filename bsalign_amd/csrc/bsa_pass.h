// bsa_pass.h -- what the passes over an aligner's outputs share (bsa_cigar_eqx.hip, bsa_band_margin.hip, bsa_cigar_windows.hip, bsa_window_pieces.hip,
// bsa_window_select.hip, bsa_piece_cigars.hip, bsa_window_msa.hip, bsa_window_cns.hip, bsa_window_stitch.hip): the context's internal entry points and the exclusive scan, declared once (bsa_api.hip and bsa_scan.hip include this header
// too, so the compiler checks declaration against definition), wave prefix sums, the rules of a CIGAR word, and the host arithmetic of their launchers.
#pragma once
#include "bsa_common.h"
#include <vector>

// bsa_api.hip
extern "C" int bsa_ctx_get_stream_internal(bsa_ctx_t *ctx, hipStream_t *st);                              // (also selects the context's device)
extern "C" int bsa_ctx_scratch_internal(bsa_ctx_t *ctx, int slot, size_t bytes, void **out);               // (waits for the stream only when it has to grow)
extern "C" void bsa_ctx_set_error_internal(bsa_ctx_t *ctx, const char *msg);
extern "C" size_t bsa_ctx_workspace_limit_internal(bsa_ctx_t *ctx);
extern "C" int bsa_ctx_kmer_chain_events_internal(bsa_ctx_t *ctx, size_t chunks, long on_device, hipEvent_t **ev);

// bsa_scan.hip: off[0 .. n] = the exclusive prefix sums of v[0 .. n) in 64 bits, off[n] the total; *carry (optional) is a running base that the total
// is added to.  tmp: bsa_excl_scan_tmp_bytes(n) bytes.  32-bit counts go to one block up to 16 384 of them (or without a tmp), to tiles above;
// 64-bit values always go to tiles and need the tmp.
hipError_t bsa_launch_excl_scan(hipStream_t st, const uint32_t *v, uint64_t *off, uint32_t n, uint64_t *carry, uint64_t *tmp);
hipError_t bsa_launch_excl_scan(hipStream_t st, const uint64_t *v, uint64_t *off, uint32_t n, uint64_t *carry, uint64_t *tmp);
size_t bsa_excl_scan_tmp_bytes(uint32_t n);

// inclusive prefix sums over the wave (T: uint32_t or uint64_t)
template<typename T>
static __device__ __forceinline__ T bsa_wave_iscan(T v, uint32_t lane){
#pragma unroll
	for(uint32_t d = 1; d < 64u; d <<= 1){ const T u = __shfl_up(v, d); if(lane >= d) v += u; }
	return v;
}

// a CIGAR word's op: does it walk the diagonal, does it take a step at all, and the bases a word of `len` adds to q and to t (T: the type the caller
// sums t in -- q wraps in 32 bits everywhere)
static __device__ __forceinline__ bool bsa_cig_diag(uint32_t op){ return op == BSA_CIGAR_M || op == BSA_CIGAR_EQ || op == BSA_CIGAR_X; }
static __device__ __forceinline__ bool bsa_cig_steps(uint32_t op){ return bsa_cig_diag(op) || op == BSA_CIGAR_I || op == BSA_CIGAR_D; }
static __device__ __forceinline__ uint32_t bsa_cig_qadd(uint32_t op, uint32_t len){ return (bsa_cig_diag(op) || op == BSA_CIGAR_I) ? len : 0u; }
template<typename T = uint32_t>
static __device__ __forceinline__ T bsa_cig_tadd(uint32_t op, uint32_t len){ return (bsa_cig_diag(op) || op == BSA_CIGAR_D) ? len : 0u; }

// the parts of one device buffer start at multiples of 256 bytes
static inline size_t bsa_up256(size_t b){ return (b + 255u) & ~(size_t)255u; }

// The staging of a _batch form: one device allocation carved into parts that start at multiples of 256 bytes.  Reserve the parts, alloc(), then move
// them on the context's stream.  The destructor waits for the stream before it frees: nothing of the call is in flight when its buffers go, however
// the call ends (declare the host arrays that go up in front of it).  fail() sets the context's error and returns the code.
struct bsa_stage_t {
	bsa_ctx_t *ctx; hipStream_t st; uint8_t *buf = nullptr; size_t total = 0;
	bsa_stage_t(bsa_ctx_t *c, hipStream_t s) : ctx(c), st(s) {}
	bsa_stage_t(const bsa_stage_t&) = delete;
	~bsa_stage_t(){ if(buf){ (void)hipStreamSynchronize(st); (void)hipFree(buf); } }
	int fail(const char *what, int code = BSA_E_HIP) const { (void)hipGetLastError(); bsa_ctx_set_error_internal(ctx, what); return code; }
	size_t part(size_t bytes){ const size_t o = total; total += bsa_up256(bytes); return o; }
	int alloc(const char *nomem){ if(hipMalloc((void**)&buf, total) == hipSuccess) return BSA_OK; buf = nullptr; return fail(nomem, BSA_E_NOMEM); }
	template<typename T> T *at(size_t o) const { return (T*)(buf + o); }
	bool up(size_t o, const void *src, size_t bytes) const { return bytes == 0 || hipMemcpyAsync(buf + o, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess; }
	bool down(void *dst, size_t o, size_t bytes) const { return bytes == 0 || hipMemcpyAsync(dst, buf + o, bytes, hipMemcpyDeviceToHost, st) == hipSuccess; }
	bool sync() const { return hipStreamSynchronize(st) == hipSuccess; }
};
// off[0 .. n] must not decrease (`what` is the context's error when it does); reb gets n + 1 offsets that start at 0 ({0} for n == 0)
static inline int bsa_rebase_offsets(bsa_ctx_t *ctx, const uint64_t *off, size_t n, std::vector<uint64_t> &reb, const char *what){
	for(size_t k = 0; k < n; k++) if(off[k + 1] < off[k]){ bsa_ctx_set_error_internal(ctx, what); return BSA_E_ARG; }
	try { reb.assign(n + 1, 0); } catch(...){ return BSA_E_NOMEM; }
	for(size_t k = 1; k <= n; k++) reb[k] = off[k] - off[0];
	return BSA_OK;
}

// the grid of a kernel that gives 16 lanes to an item (16 items a block of 256 and trip) and strides over `items` with at most 16 blocks a CU
static inline dim3 bsa_grid16(size_t items){
	const size_t want = (items + 15u) / 16u, most = (size_t)bsa_cus() * 16u;
	return dim3((uint32_t)(want < most ? want : most));
}
