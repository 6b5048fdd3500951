// bsa_stage.hip -- from the caller's sequence blob to what the aligners read: the staging kernels of the align and the edit plans, their one
// launcher, and bsa_seq_pack2bit.  The blob's layouts and the strand rule are bsa_seq.h's (bsa_seq16); what is here is the walk over a pair.
//
// One pair per TPP threads -- a wave for short pairs (a block per pair spent most of its time being launched; the k-mer path stages 1.5 M pieces
// of ~26 bp), the whole block for long ones.  16 bases per thread and trip, one 16-byte store (the staged regions are 16-byte aligned and a
// whole number of 16-byte pieces; the source is not aligned and ends with the sequence).
//   align form: query codes padded with BSA_QPAD_CODE over qpad bytes, target codes padded with 0 over tpad bytes;
//   edit form (PLANES): both padded with 0 over 16 bytes, and the query also as two bit planes of qwords[k] words each (bit p of plane b = bit b
//     of base p; zero beyond qlen): 16 bits a trip -- from the packed value directly, or bit 0 / bit 1 of eight bytes gathered by a multiplication.
// QS (plans with BSA_MODE_QSTRAND): bit 63 of qoff[k] asks for the query's reverse complement; bytes and planes are then those of the reverse
// complement.  status[k]: BSA_ST_BAD_BASE (1 B/base blobs: a code above 3; packed words hold none), BSA_ST_EMPTY.
// No LDS; plain C++ with vector loads and stores only.
#include "bsa_pass.h"

template<int TPP, bool PK, bool QS, bool PLANES>
static __device__ __forceinline__ void stage_pair(const void *seqs, const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen,
		const uint64_t *qpoff, const uint64_t *tpoff, const uint64_t *qboff, const uint32_t *qwords, uint8_t *qst, uint8_t *tst, uint64_t *qbits,
		uint8_t qpadcode, uint32_t qpad, uint32_t tpad, uint32_t *status, uint32_t n){
	const uint32_t k = (TPP == 64) ? blockIdx.x * 4u + (threadIdx.x >> 6) : blockIdx.x, lane = threadIdx.x & (uint32_t)(TPP - 1);
	if(k >= n) return;
	const uint32_t ql = qlen[k], tl = tlen[k];
	const uint64_t qraw = qoff[k], to = toff[k];
	const bool qrev = QS && (qraw & BSA_QOFF_REVCOMP) != 0;
	const uint64_t qo = QS ? qraw & ~BSA_QOFF_REVCOMP : qraw;
	uint8_t *dq = qst + qpoff[k], *dt = tst + tpoff[k];
	uint32_t bad = 0;
	const uint32_t qbytes = (ql + qpad + 15u) & ~15u, tbytes = (tl + tpad + 15u) & ~15u;
	uint32_t qplane = 0;
	uint64_t *p0 = nullptr, *p1 = nullptr;
	if constexpr (PLANES){ const uint32_t nw = qwords[k]; p0 = qbits + qboff[k]; p1 = p0 + nw; qplane = nw * 64u; }
	for(uint32_t i = lane * 16u; i < max(qbytes, qplane); i += (uint32_t)TPP * 16u){
		uint64_t v0, v1;
		const uint32_t x = bsa_seq16<PK, QS>(seqs, qo, ql, i, qrev, qpadcode, v0, v1, bad);
		if(!PLANES || i < qbytes) bsa_store16(dq + i, v0, v1);
		if constexpr (PLANES){
			if(i < qplane){
				if constexpr (PK){
					((uint16_t*)p0)[i >> 4] = (uint16_t)bsa_even16(x);
					((uint16_t*)p1)[i >> 4] = (uint16_t)bsa_even16(x >> 1);
				} else {
					auto gather = [](uint64_t v) -> uint32_t { return (uint32_t)(((v & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56); };   // bit 0 of byte j -> bit j
					((uint16_t*)p0)[i >> 4] = (uint16_t)(gather(v0) | (gather(v1) << 8));
					((uint16_t*)p1)[i >> 4] = (uint16_t)(gather(v0 >> 1) | (gather(v1 >> 1) << 8));
				}
			}
		}
	}
	for(uint32_t i = lane * 16u; i < tbytes; i += (uint32_t)TPP * 16u){
		uint64_t v0, v1;
		bsa_seq16<PK, false>(seqs, to, tl, i, false, (uint8_t)0, v0, v1, bad);
		bsa_store16(dt + i, v0, v1);
	}
	uint32_t st = 0;
	if constexpr (!PK){ if((TPP == 64) ? __any((int)bad) : __syncthreads_or((int)bad)) st |= BSA_ST_BAD_BASE; }
	if(ql == 0 || tl == 0) st |= BSA_ST_EMPTY;
	if(lane == 0) status[k] = st;
}

// the four kernels: 1 B/base or BSA_MODE_SEQ2BIT words (2b), for the align plan or (edit) with the planes
#define STAGE_IN const uint64_t *qoff, const uint32_t *qlen, const uint64_t *toff, const uint32_t *tlen, const uint64_t *qpoff, const uint64_t *tpoff
template<int TPP, bool QS = false>
__global__ void __launch_bounds__(256) k_stage(const uint8_t *seqs, STAGE_IN, uint8_t *qst, uint8_t *tst, uint32_t qpad, uint32_t tpad, uint32_t *status, uint32_t n){
	stage_pair<TPP, false, QS, false>(seqs, qoff, qlen, toff, tlen, qpoff, tpoff, nullptr, nullptr, qst, tst, nullptr, (uint8_t)BSA_QPAD_CODE, qpad, tpad, status, n);
}
template<int TPP, bool QS = false>
__global__ void __launch_bounds__(256) k_stage2b(const uint64_t *seqs, STAGE_IN, uint8_t *qst, uint8_t *tst, uint32_t qpad, uint32_t tpad, uint32_t *status, uint32_t n){
	stage_pair<TPP, true, QS, false>(seqs, qoff, qlen, toff, tlen, qpoff, tpoff, nullptr, nullptr, qst, tst, nullptr, (uint8_t)BSA_QPAD_CODE, qpad, tpad, status, n);
}
template<int TPP, bool QS = false>
__global__ void __launch_bounds__(256) k_edit_stage(const uint8_t *seqs, STAGE_IN, const uint64_t *qboff, const uint32_t *qwords, uint8_t *qst, uint8_t *tst,
		uint64_t *qbits, uint32_t *status, uint32_t n){
	stage_pair<TPP, false, QS, true>(seqs, qoff, qlen, toff, tlen, qpoff, tpoff, qboff, qwords, qst, tst, qbits, (uint8_t)0, 16u, 16u, status, n);
}
template<int TPP, bool QS = false>
__global__ void __launch_bounds__(256) k_edit_stage2b(const uint64_t *seqs, STAGE_IN, const uint64_t *qboff, const uint32_t *qwords, uint8_t *qst, uint8_t *tst,
		uint64_t *qbits, uint32_t *status, uint32_t n){
	stage_pair<TPP, true, QS, true>(seqs, qoff, qlen, toff, tlen, qpoff, tpoff, qboff, qwords, qst, tst, qbits, (uint8_t)0, 16u, 16u, status, n);
}
#undef STAGE_IN

// The launch: one row of a switch over a packed key, one row macro per kernel wrapper (a key written twice does not compile; a key without a row
// launches nothing and is hipErrorInvalidValue).  The caller chooses the threads per pair; the QS instantiations are only for plans with BSA_MODE_QSTRAND.
constexpr uint32_t stage_key(bool seq2bit, bool planes, uint32_t tpp, bool qs){ return (uint32_t)seq2bit | (uint32_t)planes << 1 | (uint32_t)qs << 2 | tpp << 3; }
#define STAGE_IN a.qoff, a.qlen, a.toff, a.tlen, a.qpoff, a.tpoff
#define STAGE_ALIGN a.qst, a.tst, a.qpad, a.tpad, a.status, a.n
#define STAGE_EDIT a.qboff, a.qwords, a.qst, a.tst, a.qbits, a.status, a.n
#define STAGE_K(TPP, QS) case stage_key(false, false, TPP, QS): hipLaunchKernelGGL((k_stage<TPP, QS>), grid, dim3(256), 0, st, a.seqs, STAGE_IN, STAGE_ALIGN); break;
#define STAGE2B_K(TPP, QS) case stage_key(true, false, TPP, QS): hipLaunchKernelGGL((k_stage2b<TPP, QS>), grid, dim3(256), 0, st, (const uint64_t*)a.seqs, STAGE_IN, STAGE_ALIGN); break;
#define E_STAGE_K(TPP, QS) case stage_key(false, true, TPP, QS): hipLaunchKernelGGL((k_edit_stage<TPP, QS>), grid, dim3(256), 0, st, a.seqs, STAGE_IN, STAGE_EDIT); break;
#define E_STAGE2B_K(TPP, QS) case stage_key(true, true, TPP, QS): hipLaunchKernelGGL((k_edit_stage2b<TPP, QS>), grid, dim3(256), 0, st, (const uint64_t*)a.seqs, STAGE_IN, STAGE_EDIT); break;
hipError_t bsa_launch_stage(const StageArgs &a, bool seq2bit, uint32_t tpp, bool qstrand, hipStream_t st){
	if(a.n == 0) return hipSuccess;
	const dim3 grid(tpp == 64u ? (a.n + 3u) / 4u : a.n);
	switch(stage_key(seq2bit, a.qbits != nullptr, tpp, qstrand)){
		STAGE_K(64, false) STAGE_K(256, false) STAGE_K(64, true) STAGE_K(256, true)
		STAGE2B_K(64, false) STAGE2B_K(256, false) STAGE2B_K(64, true) STAGE2B_K(256, true)
		E_STAGE_K(64, false) E_STAGE_K(256, false) E_STAGE_K(64, true) E_STAGE_K(256, true)
		E_STAGE2B_K(64, false) E_STAGE2B_K(256, false) E_STAGE2B_K(64, true) E_STAGE2B_K(256, true)
		default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

// bsa_seq_pack2bit: 32 codes a thread into one word of the BSA_MODE_SEQ2BIT layout (c & 3; a code above 3 sets *bad)
__global__ void __launch_bounds__(256) k_pack2bit(const uint8_t *codes, uint64_t nbases, uint64_t *bits, uint32_t *bad){
	const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x, b0 = w * 32u;
	if(b0 >= nbases) return;
	uint64_t v = 0, hi = 0;
	if(b0 + 32u <= nbases){
#pragma unroll
		for(uint32_t j = 0; j < 4u; j++){
			uint64_t c;
			__builtin_memcpy(&c, codes + b0 + 8u * j, 8);
			hi |= c;
#pragma unroll
			for(uint32_t b = 0; b < 8u; b++) v |= ((c >> (8u * b)) & 3ull) << (62u - 2u * (8u * j + b));
		}
		hi &= 0xFCFCFCFCFCFCFCFCull;
	} else {
		for(uint32_t j = 0; b0 + j < nbases; j++){
			const uint8_t c = codes[b0 + j];
			hi |= c & 0xFCu;
			v |= (uint64_t)(c & 3u) << (62u - 2u * j);
		}
	}
	bits[w] = v;
	if(bad && hi) *bad = 1u;
}

extern "C" int bsa_seq_pack2bit(bsa_ctx_t *c, const uint8_t *d_codes, uint64_t nbases, uint64_t *d_bits, uint32_t *d_bad){
	if(!c || (nbases && (!d_codes || !d_bits))) return BSA_E_ARG;
	if(nbases == 0) return BSA_OK;
	hipStream_t st;
	const int rc = bsa_ctx_get_stream_internal(c, &st);          // (also selects the context's device)
	if(rc != BSA_OK) return rc;
	const uint64_t words = (nbases + 31u) / 32u, blocks = (words + 255u) / 256u;
	if(blocks > 0x7FFFFFFFull){ bsa_ctx_set_error_internal(c, "bsa_seq_pack2bit: too many bases"); return BSA_E_ARG; }
	hipLaunchKernelGGL(k_pack2bit, dim3((uint32_t)blocks), dim3(256), 0, st, d_codes, nbases, d_bits, d_bad);
	const hipError_t e = hipGetLastError();
	if(e != hipSuccess){ bsa_ctx_set_error_internal(c, hipGetErrorString(e)); return BSA_E_HIP; }
	return BSA_OK;
}

// the host side of bsa_seq16, for tests (no device): out = the sixteen staged codes of piece i, *bad = whether it set `bad`.  packed: the blob is
// BSA_MODE_SEQ2BIT words and `off` a base offset.  rev: 0 forwards, 1 the reverse complement, 2 forwards through the QS instantiation (a plan with
// BSA_MODE_QSTRAND reading an unmarked query)
extern "C" int bsa_seq16_internal(const void *seqs, uint64_t off, uint32_t len, uint32_t i, int packed, int rev, int padcode, uint8_t out[16], uint32_t *bad){
	if(!out || !bad || (len && !seqs) || rev < 0 || rev > 2 || padcode < 0 || padcode > 255) return BSA_E_ARG;
	uint64_t v[2];
	uint32_t b = 0;
	const uint8_t pc = (uint8_t)padcode;
	if(packed){ if(rev) bsa_seq16<true, true>(seqs, off, len, i, rev == 1, pc, v[0], v[1], b); else bsa_seq16<true, false>(seqs, off, len, i, false, pc, v[0], v[1], b); }
	else { if(rev) bsa_seq16<false, true>(seqs, off, len, i, rev == 1, pc, v[0], v[1], b); else bsa_seq16<false, false>(seqs, off, len, i, false, pc, v[0], v[1], b); }
	__builtin_memcpy(out, v, 16);
	*bad = b;
	return BSA_OK;
}
