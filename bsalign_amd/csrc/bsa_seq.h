// bsa_seq.h -- how a caller's sequence blob is read: 1 B/base codes or BSA_MODE_SEQ2BIT words, forwards or (BSA_MODE_QSTRAND) as the reverse
// complement, sixteen codes at a time.  Everything that knows the two layouts and the strand rule is here, once, for host and device: the staging
// kernels (bsa_stage.hip), the window pass's gather (bsa_window_pieces.hip) and the CPU test of the staged codes (bsa_seq16_internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// BSA_MODE_SEQ2BIT blobs (include/bsalign_hip.h): base i at bits 62 - 2 (i % 32) of word i / 32.  The 16 bases [pos, pos + 16) as a
// 32-bit value LSB first (base pos + j at bits 2j, 2j + 1), bases at or past `end` zero.  Loads the word of `pos` and, only when a base
// before `end` lies in it, the next one -- never a word behind the one that holds base end - 1 (a caller's array may end there).
__host__ __device__ __forceinline__ uint32_t bsa_bits16(const uint64_t *w, uint64_t pos, uint64_t end){
	if(pos >= end) return 0u;
	const uint64_t idx = pos >> 5, rem = end - pos;
	const uint32_t r = (uint32_t)(pos & 31u);
	uint64_t hi = w[idx] << (2u * r);                               // MSB first: base pos at bits 63:62
	if(r > 16u && ((pos + (rem < 16u ? rem : 16u) - 1u) >> 5) != idx) hi |= w[idx + 1] >> (64u - 2u * r);      // (funnel shift across the word boundary)
	uint32_t x = __builtin_bitreverse32((uint32_t)(hi >> 32));      // base pos + j at bits 2j (its low bit) and 2j + 1 swapped ...
	x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);         // ... and swapped back
	if(rem < 16u) x &= (1u << (2u * (uint32_t)rem)) - 1u;
	return x;
}
// BSA_MODE_QSTRAND: the reverse twin -- the 16 bases [end - 16, end) read backwards and complemented (3 - c), LSB first: base end - 1 - j at
// bits 2j, 2j + 1, bases before `beg` zero.  Inside a word the MSB-first order IS the wanted order read from the other end (base p + 1 sits
// two bits below base p), so there is no bit reversal: a funnel shift, a NOT and a mask.  Loads the word of base end - 1 and, only when a
// base at or after `beg` lies in it, the one in front -- never a word in front of the one that holds base `beg`.
__host__ __device__ __forceinline__ uint32_t bsa_bits16_rc(const uint64_t *w, uint64_t beg, uint64_t end){
	if(end <= beg) return 0u;
	const uint64_t last = end - 1u, idx = last >> 5, rem = end - beg;
	const uint32_t r = (uint32_t)(last & 31u);
	uint32_t x = (uint32_t)(w[idx] >> (62u - 2u * r));              // base end - 1 at bits 1:0, the r bases in front of it above
	if(r < 15u && ((end - (rem < 16u ? rem : 16u)) >> 5) != idx) x |= (uint32_t)w[idx - 1] << (2u * r + 2u);      // (funnel shift across the word boundary)
	x = ~x;
	if(rem < 16u) x &= (1u << (2u * (uint32_t)rem)) - 1u;
	return x;
}
// 8 codes (2 bits each, LSB first) -> 8 bytes
__host__ __device__ __forceinline__ uint64_t bsa_spread8(uint32_t x){
	uint64_t v = x & 0xFFFFu;
	v = (v | (v << 24)) & 0x000000FF000000FFull;
	v = (v | (v << 12)) & 0x000F000F000F000Full;
	return (v | (v << 6)) & 0x0303030303030303ull;
}
// the even bits of x, packed (bit 2j -> bit j)
__host__ __device__ __forceinline__ uint32_t bsa_even16(uint32_t x){
	x &= 0x55555555u;
	x = (x | (x >> 1)) & 0x33333333u;
	x = (x | (x >> 2)) & 0x0F0F0F0Fu;
	x = (x | (x >> 4)) & 0x00FF00FFu;
	return (x | (x >> 8)) & 0x0000FFFFu;
}
// bytes [rem, 8) of v replaced by `pad` (rem may be <= 0 or >= 8)
__host__ __device__ __forceinline__ uint64_t bsa_pad_bytes(uint64_t v, int64_t rem, uint8_t pad){
	if(rem >= 8) return v;
	const uint64_t keep = rem <= 0 ? 0ull : (1ull << (8u * (uint32_t)rem)) - 1ull;
	return (v & keep) | ((uint64_t)pad * 0x0101010101010101ull & ~keep);
}

// THE READER.  s = the sequence of `len` bases at `off` of the blob (a byte offset; a base offset when PK), or, when QS and `rev`, its reverse
// complement.  v0 / v1 get the staged codes of s[i, i + 8) / s[i + 8, i + 16), a byte each, LSB first: s's own code below `len`, `padcode` at
// or past it.  Returns (PK) the same sixteen codes as two bits each, zero past `len` -- the bit planes come cheaper from them -- and 0 otherwise.
// 1 B/base: a whole piece (i + 16 <= len) is two 8-byte loads of any alignment, on the reverse strand the 16 stored bytes that end at len - i,
// byte-swapped and ^ 3; the piece that holds the end goes byte by byte and reads nothing at or past off + len (a caller's array may end
// there).  A code above 3 that lies below `len` sets `bad` and is taken & 3.  Packed: bsa_bits16 / bsa_bits16_rc, whose rules say which words
// are loaded; `bad` is never touched.
template<bool PK, bool QS>
__host__ __device__ __forceinline__ uint32_t bsa_seq16(const void *seqs, uint64_t off, uint32_t len, uint32_t i, bool rev, uint8_t padcode,
		uint64_t &v0, uint64_t &v1, uint32_t &bad){
	if constexpr (PK){
		const uint64_t *w = (const uint64_t*)seqs;
		const uint32_t x = (QS && rev) ? (i < len ? bsa_bits16_rc(w, off, off + len - i) : 0u) : bsa_bits16(w, off + i, off + len);
		v0 = bsa_spread8(x); v1 = bsa_spread8(x >> 16);
		if(padcode != 0 && i + 16u > len){ v0 = bsa_pad_bytes(v0, (int64_t)len - i, padcode); v1 = bsa_pad_bytes(v1, (int64_t)len - i - 8, padcode); }
		return x;
	} else {
		const uint8_t *src = (const uint8_t*)seqs + off;
		if(i + 16u <= len){
			if(QS && rev){
				const uint8_t *s = src + (len - i - 16u);
				__builtin_memcpy(&v1, s, 8); __builtin_memcpy(&v0, s + 8, 8);
				v0 = __builtin_bswap64(v0); v1 = __builtin_bswap64(v1);
			} else { __builtin_memcpy(&v0, src + i, 8); __builtin_memcpy(&v1, src + i + 8, 8); }
			if((v0 | v1) & 0xFCFCFCFCFCFCFCFCull) bad = 1;
			v0 &= 0x0303030303030303ull; v1 &= 0x0303030303030303ull;
			if(QS && rev){ v0 ^= 0x0303030303030303ull; v1 ^= 0x0303030303030303ull; }
		} else {
			v0 = v1 = 0;
#pragma unroll
			for(uint32_t b = 0; b < 16u; b++){
				uint8_t c = (i + b < len) ? ((QS && rev) ? src[len - 1u - i - b] : src[i + b]) : padcode;
				if(c > 3 && (padcode <= 3 || i + b < len)){ bad = 1; c &= 3; }          // (a pad code is no base)
				if(QS && rev && i + b < len) c ^= 3;
				if(b < 8u) v0 |= (uint64_t)c << (8u * b); else v1 |= (uint64_t)c << (8u * (b - 8u));
			}
		}
		return 0u;
	}
}

// sixteen staged codes to 16-byte aligned memory, one store
__device__ __forceinline__ void bsa_store16(uint8_t *dst, uint64_t v0, uint64_t v1){
	uint4 o; o.x = (uint32_t)v0; o.y = (uint32_t)(v0 >> 32); o.z = (uint32_t)v1; o.w = (uint32_t)(v1 >> 32);
	*(uint4*)dst = o;
}
