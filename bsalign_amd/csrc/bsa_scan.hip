// bsa_scan.hip -- the exclusive scan in 64 bits (bsa_pass.h: bsa_launch_excl_scan) that turns counts into offsets: the align plan's CIGAR offsets and
// the offsets of the window passes.  One block for few counts, tiles for many and for 64-bit values.  Every sum is kept in 64 bits from the first add on.
#include "bsa_pass.h"

// single-block exclusive scan of cnt[0..n) into off[0..n], off[n] = total; *carry (optional) is a running base
__global__ void __launch_bounds__(1024) k_excl_scan(const uint32_t *cnt, uint64_t *off, uint32_t n, uint64_t *carry){
	__shared__ uint64_t part[1024];
	__shared__ uint64_t base;
	const uint32_t t = threadIdx.x;
	if(t == 0) base = carry ? *carry : 0ull;
	__syncthreads();
	for(uint32_t s = 0; s < n; s += 1024u * 8u){
		uint64_t loc[8]; uint64_t sum = 0;
		for(int k = 0; k < 8; k++){
			uint32_t idx = s + t * 8u + k;
			loc[k] = sum;
			sum += (idx < n) ? cnt[idx] : 0u;
		}
		part[t] = sum;
		__syncthreads();
		for(uint32_t d = 1; d < 1024; d <<= 1){   // Hillis-Steele inclusive scan of the per-thread sums
			uint64_t v = (t >= d) ? part[t - d] : 0ull;
			__syncthreads();
			part[t] += v;
			__syncthreads();
		}
		const uint64_t excl = part[t] - sum + base;
		for(int k = 0; k < 8; k++){
			uint32_t idx = s + t * 8u + k;
			if(idx < n) off[idx] = excl + loc[k];
		}
		__syncthreads();
		if(t == 1023) base += part[1023];
		__syncthreads();
	}
	if(t == 0){ off[n] = base; if(carry) *carry = base; }
}

// The same scan over many blocks for batches of millions of pairs (one block reads 4 bytes per pair at the speed of one CU: 2 ms
// for 2 M pairs, twice per step): sums of tiles of SCAN_TILE values, a scan of the sums by one block, then every tile scanned with
// its base.  T: uint32_t or uint64_t values.  tmp: (tiles + 1) uint64, tiles = max(1, ceil(n / SCAN_TILE)).
#define SCAN_TILE 4096u
template<typename T>
__global__ void __launch_bounds__(256) k_scan_tile_sums(const T *v, uint32_t n, uint64_t *tmp){
	__shared__ uint64_t red[4];
	const uint32_t b = blockIdx.x, t = threadIdx.x;
	uint64_t s = 0;
	for(uint32_t i = t; i < SCAN_TILE; i += 256u){ const uint64_t idx = (uint64_t)b * SCAN_TILE + i; s += (idx < n) ? v[idx] : 0u; }
	for(int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
	if((t & 63u) == 0u) red[t >> 6] = s;
	__syncthreads();
	if(t == 0) tmp[b] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(1024) k_scan_tile_bases(uint64_t *tmp, uint32_t tiles, uint64_t *carry){
	__shared__ uint64_t part[1024];
	__shared__ uint64_t base;
	const uint32_t t = threadIdx.x;
	if(t == 0) base = carry ? *carry : 0ull;
	__syncthreads();
	for(uint32_t s = 0; s < tiles; s += 1024u){
		const uint64_t v = (s + t < tiles) ? tmp[s + t] : 0ull;
		part[t] = v;
		__syncthreads();
		for(uint32_t d = 1; d < 1024; d <<= 1){
			const uint64_t w = (t >= d) ? part[t - d] : 0ull;
			__syncthreads();
			part[t] += w;
			__syncthreads();
		}
		if(s + t < tiles) tmp[s + t] = part[t] - v + base;
		__syncthreads();
		if(t == 1023) base += part[1023];
		__syncthreads();
	}
	if(t == 0){ tmp[tiles] = base; if(carry) *carry = base; }
}
template<typename T>
__global__ void __launch_bounds__(256) k_scan_tile_apply(const T *v, uint64_t *off, uint32_t n, const uint64_t *tmp, uint32_t tiles){
	__shared__ uint64_t wsum[4];
	const uint32_t b = blockIdx.x, t = threadIdx.x;
	const uint64_t i0 = (uint64_t)b * SCAN_TILE + t * 16u;  // 16 consecutive values per thread
	uint64_t loc[16], s = 0;                                // (the local prefixes too: three counts of 2^31 - 1 do not fit 32 bits)
	for(int k = 0; k < 16; k++){ loc[k] = s; s += (i0 + k < n) ? v[i0 + k] : 0u; }
	uint64_t inc = s;                                       // inclusive scan of the thread sums inside the wave, then across the four waves
	for(int d = 1; d < 64; d <<= 1){ const uint64_t u = __shfl_up(inc, d); if((t & 63u) >= (uint32_t)d) inc += u; }
	if((t & 63u) == 63u) wsum[t >> 6] = inc;
	__syncthreads();
	uint64_t wb = 0;
	for(uint32_t w = 0; w < (t >> 6); w++) wb += wsum[w];
	const uint64_t excl = tmp[b] + wb + inc - s;
	for(int k = 0; k < 16; k++) if(i0 + k < n) off[i0 + k] = excl + loc[k];
	if(b == tiles - 1u && t == 0) off[n] = tmp[tiles];
}

template<typename T>
static hipError_t scan_tiled(hipStream_t st, const T *v, uint64_t *off, uint32_t n, uint64_t *carry, uint64_t *tmp){
	const uint32_t tiles = n ? (uint32_t)(((uint64_t)n + SCAN_TILE - 1u) / SCAN_TILE) : 1u;
	hipLaunchKernelGGL(k_scan_tile_sums<T>, dim3(tiles), dim3(256), 0, st, v, n, tmp);
	hipLaunchKernelGGL(k_scan_tile_bases, dim3(1), dim3(1024), 0, st, tmp, tiles, carry);
	hipLaunchKernelGGL(k_scan_tile_apply<T>, dim3(tiles), dim3(256), 0, st, v, off, n, (const uint64_t*)tmp, tiles);
	return hipGetLastError();
}

size_t bsa_excl_scan_tmp_bytes(uint32_t n){ return ((size_t)n / SCAN_TILE + 2u) * 8u; }
hipError_t bsa_launch_excl_scan(hipStream_t st, const uint32_t *v, uint64_t *off, uint32_t n, uint64_t *carry, uint64_t *tmp){
	// (one block takes 111 us for the 100 000 counts of C2, twice a step; in tiles 3 x 5 us)
	if(n <= 16384u || !tmp){ hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(1024), 0, st, v, off, n, carry); return hipGetLastError(); }
	return scan_tiled(st, v, off, n, carry, tmp);
}
hipError_t bsa_launch_excl_scan(hipStream_t st, const uint64_t *v, uint64_t *off, uint32_t n, uint64_t *carry, uint64_t *tmp){
	return tmp ? scan_tiled(st, v, off, n, carry, tmp) : hipErrorInvalidValue;
}
