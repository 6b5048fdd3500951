// bsa_align8_x.hip -- forward pass of the compact (4-bit code) path of the 8-bit banded DP in EXACT arithmetic.
//
// Same results as k_align8_fwd_pk<W, 1, true> (bsa_align8_pk.hip): the same code rows, band offsets and final score,
// bit for bit -- the traceback kernels (bsa_align8_codes.hip) do not know which forward kernel ran.  It is only
// dispatched inside a guard (bsa_align8_x_supported) under which none of the reference's int8-saturating operations
// can clamp (bsalign.h:2885-2960 row_cal, :2639-2652 F-penetration, :2618-2636 tail, :2244-2392 row_movx), so the
// recurrence may be restated freely.  What changed against the packed kernel, and why (tools/valu_rate_probe.hip:
// every packed / VOP3 / DPP instruction occupies its SIMD for 4 cycles and the old kernel issued 631 of them per row
// of 8 pairs, at 100 % of that rate):
//   * ONE pair per 8 lanes, both 16-bit halves of a register belong to the SAME pair: lane l owns the reference's
//     running blocks l (low half) and l + 8 (high half).  Per-pair scalars (band offset, steering, ubegs[0]) are
//     computed once, not once per half.
//   * frame shifted by the gap extension: with H~(x, y) = H(x, y) - gape * (x + y) extending a gap is free, which
//     removes the "+ gape" of e' and f' (U = u - gape, NE = gape - e, S~ = S - 2 gape, h~ = h - 2 gape, f~ = f - 2 gape):
//         ee = U - NE          m = max(ee, S~)          mg = m + gapo
//         pass 1:  f = max(f, mg) - U                                  (2 dependent ops per cell)
//         pass 2:  h = max(m, f)   fm = max(f, mg)   f = fm - U   n = h - ee   NE' = min(n, -gapo)   U' = h - v   v = h - U
//     and the four flags of a cell are differences the recurrence has anyway: M: h - S~ == 0, D: n == 0,
//     R: fm - mg == 0, Od: NE' == -gapo, each one packed min / saturating subtract + one v_pk_mad_u16.
//   * F-penetration as a prefix maximum: in the shifted frame an F value travels along the row unchanged, so with
//     X[b] = H~ at the end of block b (relative, int16) the value entering block b is max_{i<b}(fout[i] + X[i]) - X[b-1]:
//     a 3-step max scan over the 8 lanes plus one step from the low halves to the high ones, instead of the max-plus scan.
//   * the band slide is speculated: 96 % of the rows move the band by one cell, so pass 2 writes cell k of the new row
//     into slot k - 1 and the first cell of every block travels to the previous block's last slot with one DPP move.
//     Rows that do not move (or move by more) are corrected afterwards, under a wave-level branch.
//   * ubegs are kept as PN[b] = ubegs[b+1] - ubegs[0] - (b+1) W gape in packed int16 plus ubegs[0] in an int32.
// Values are value << 8 in each int16 half (as in the packed kernel), so S~ comes out of v_perm_b32 byte lookups.
// Two row bodies: x_forward holds the row as int8 differences (above; every shape), x_forward_abs as int16 scores (its own comment; one-piece and linear gaps with
// sixteen cells a half, where it is 11 % faster).  The pair preamble, the LDS carving, the target-base window, the band steering, the code-row store, the band
// offsets / end record and the hand-over between row segments are written in both, statement for statement: a fix to one of them goes into both.  (Moving any of
// them into a force-inlined helper changes this compiler's output for the file's kernels, measurably so for some: HISTORY.md 11b.)
// Two of these differ between the row bodies on purpose (HISTORY.md 19): x_forward_abs forms the row target of global steering in integers (x_rt_*, the double expression
// where a row's product divides evenly) and shifts the slots of a row that does not move by one two to an instruction (x_slots_up / x_slots_down), and it forms
// rbase behind a wave-level test of its two readers; x_forward keeps the double expression on every renewal, one v_cndmask_b32 a slot and rbase on every live row.
// A third since HISTORY.md 20: in its biased frame x_forward_abs forms the noise sum of band steering with v_sad_u16 on the unsigned H^ patterns; x_forward's signed
// differences keep the packed absolute values and the per-half sum.
#include "bsa_common.h"
#include "bsa_dpp.h"
#include <algorithm>
#include <cstdio>
typedef short xv2s __attribute__((ext_vector_type(2)));
typedef unsigned short xv2u __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ uint32_t x_add(uint32_t a, uint32_t b){ return __builtin_bit_cast(uint32_t, (xv2u)(__builtin_bit_cast(xv2u, a) + __builtin_bit_cast(xv2u, b))); }
static __device__ __forceinline__ uint32_t x_sub(uint32_t a, uint32_t b){ return __builtin_bit_cast(uint32_t, (xv2u)(__builtin_bit_cast(xv2u, a) - __builtin_bit_cast(xv2u, b))); }
static __device__ __forceinline__ uint32_t x_max(uint32_t a, uint32_t b){ return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(xv2s, a), __builtin_bit_cast(xv2s, b))); }
// max(a, b, c) per half in ONE instruction (v_pk_maximum3_f16; there is no three-operand packed integer maximum): the halves are read as f16, whose order is that
// of int16 for the patterns 0x0400 .. 0x7BFF (positive, finite, normal: no sign, no NaN, nothing a denormal mode could flush), and the result is one of the
// operands, bit for bit.  The caller keeps every operand in that range (x_forward_abs, "biased frame").
typedef _Float16 xv2h __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ uint32_t x_max3(uint32_t a, uint32_t b, uint32_t c){
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(xv2h, a), __builtin_bit_cast(xv2h, b)), __builtin_bit_cast(xv2h, c)));
}
static __device__ __forceinline__ uint32_t x_minu(uint32_t a, uint32_t b){ return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(xv2u, a), __builtin_bit_cast(xv2u, b))); }
static __device__ __forceinline__ uint32_t x_satsubu(uint32_t a, uint32_t b){ return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(xv2u, a), __builtin_bit_cast(xv2u, b))); }
// acc * 2 + flag per half: one v_pk_mad_u16 as long as the compiler cannot see that `two` is the constant 0x00020002 (it
// would turn the product into a shift and need a second instruction).  No inline asm in the row loop: on gfx950 the
// hazard recognizer puts a wait state behind every asm statement whose result a VALU instruction reads.
static __device__ __forceinline__ uint32_t x_acc(uint32_t acc, uint32_t flag, uint32_t two){
	return __builtin_bit_cast(uint32_t, (xv2u)(__builtin_bit_cast(xv2u, acc) * __builtin_bit_cast(xv2u, two) + __builtin_bit_cast(xv2u, flag)));
}
// One-bit flag "a == b" of a cell of x_forward_abs, put into its accumulator from n = b - a per half, where 0 <= a - b <= 256 (bsa_align8_flag_span has the
// bound): such an n is 0 or has bits 8 .. 15 all set, so any one of those bits is the flag inverted, and `bit` (one bit of 8 .. 15 in both halves, a constant of
// the cell that the compiler keeps in an SGPR) picks the place: acc = (bit & ~n) | (acc & ~bit), ONE v_bitop3_b32 (table 0x4E; of the operands a, b, c the table is
// the same expression of 0xF0, 0xCC, 0xAA).  By the builtin: from the plain expression the compiler, which knows the other bits of acc, makes a v_and_b32 per cell
// and a tree of three-operand exclusive-ors, half an instruction a cell more.  Nothing but the cell's own bit changes, so a cell outside the bound spoils its
// own flag only.  x_ins0 is the first cell of an accumulator, bit & ~n (table 0x0A): no zero to read.
static __device__ __forceinline__ uint32_t x_ins(uint32_t acc, uint32_t n, uint32_t bit){ return __builtin_amdgcn_bitop3_b32(n, acc, bit, 0x4E); }
static __device__ __forceinline__ uint32_t x_ins0(uint32_t n, uint32_t bit){ return __builtin_amdgcn_bitop3_b32(n, n, bit, 0x0A); }
static __device__ __forceinline__ uint32_t x_shl15(uint32_t a){ return __builtin_bit_cast(uint32_t, (xv2u)(__builtin_bit_cast(xv2u, a) << 15)); }
static __device__ __forceinline__ uint32_t x_ashr8(uint32_t a){ return __builtin_bit_cast(uint32_t, (xv2s)(__builtin_bit_cast(xv2s, a) >> 8)); }
static __device__ __forceinline__ uint32_t x_shl8(uint32_t a){ return __builtin_bit_cast(uint32_t, (xv2u)(__builtin_bit_cast(xv2u, a) << 8)); }
// x = take ? y : x, in place (the band corrections: a plain C select makes the register allocator copy the whole band)
static __device__ __forceinline__ void x_sel(uint32_t &x, uint32_t y, uint64_t take){ asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(x) : "v"(y), "s"(take)); }
// Shift of a row's W slots by one slot in the lanes that execute it (the caller's divergent if sets the execution mask), two slots an instruction: slots 2j and 2j + 1
// are handed over as one 64-bit operand, and v_pk_mov_b32 d, a, b op_sel:[x, y] writes d.lo = a[x], d.hi = b[y].
//   x_slots_up:    X[k] <- X[k - 1], X[0] <- in        pair j = {high of pair j - 1, its own low}, from the top down
//   x_slots_down:  X[k] <- X[k + 1], X[W - 1] <- in    pair j = {its own high, low of pair j + 1}, from the bottom up
// The entering value is the low dword of a 64-bit operand of its own (written into the pair behind the shift instead, it made the register allocator rotate the
// whole array by two registers and back).  The arrays stay uint32_t[W] in the source; the register coalescer keeps each in W / 2 aligned pairs.
typedef uint32_t xv2w __attribute__((ext_vector_type(2)));
template<int W> static __device__ __forceinline__ void x_slots_up(uint32_t *X, uint32_t in){
	xv2w P[W / 2];
#pragma unroll
	for(int j = 0; j < W / 2; j++){ P[j].x = X[2 * j]; P[j].y = X[2 * j + 1]; }
#pragma unroll
	for(int j = W / 2 - 1; j >= 1; j--) asm("v_pk_mov_b32 %0, %1, %0 op_sel:[1,0]" : "+v"(P[j]) : "v"(P[j - 1]));
	xv2w I;          // (the high dword is not selected by op_sel and stays unwritten: writing it costs a v_mov_b32 a shift)
	I.x = in;
	asm("v_pk_mov_b32 %0, %1, %0 op_sel:[0,0]" : "+v"(P[0]) : "v"(I));
#pragma unroll
	for(int j = 0; j < W / 2; j++){ X[2 * j] = P[j].x; X[2 * j + 1] = P[j].y; }
}
template<int W> static __device__ __forceinline__ void x_slots_down(uint32_t *X, uint32_t in){
	xv2w P[W / 2];
#pragma unroll
	for(int j = 0; j < W / 2; j++){ P[j].x = X[2 * j]; P[j].y = X[2 * j + 1]; }
#pragma unroll
	for(int j = 0; j + 1 < W / 2; j++) asm("v_pk_mov_b32 %0, %0, %1 op_sel:[1,0]" : "+v"(P[j]) : "v"(P[j + 1]));
	xv2w I;
	I.x = in;
	asm("v_pk_mov_b32 %0, %0, %1 op_sel:[1,0]" : "+v"(P[W / 2 - 1]) : "v"(I));
#pragma unroll
	for(int j = 0; j < W / 2; j++){ X[2 * j] = P[j].x; X[2 * j + 1] = P[j].y; }
}
// ROW TARGET of global steering (bsalign.h:4009) in integers, for x_forward_abs.  The reference's expression for row a of a pair (a < t = tlen, q = qlen):
static __host__ __device__ inline int x_rt_double(uint32_t a, uint32_t t, uint32_t q){ return (int)((1.0 * (double)a / (double)t) * (double)q); }
// Let v = a q / t exactly and a q = k t + r, 0 <= r < t.  The expression is y = fl(fl(a / t) q): two roundings, each within 2^-53 of its value, and a / t < 1, so
// |y - v| < q 2^-52.  Where r != 0, v lies at least 1 / t from an integer, so trunc(y) = k whenever q 2^-52 < 1 / t, i.e. q t < 2^52.  Where r = 0, v = k is an
// integer that y may miss from below, so those rows ask the expression itself (x_rt_set).
// The state {k, r} of row a steps to row a + n by adding {dk, dr} of n q = dk t + dr with one carry (x_rt_step): integers throughout, a q < 2^52, r + dr < 2^32.
// THE BOUND IS PER PAIR (x_rt_wide): the compact path bounds qlen (below 2^26), not tlen, so a pair with q t >= 2^52, or a length of 2^31 and more (r + dr could wrap),
// is outside the proof and takes the double expression on EVERY renewal, as the kernels did before: whatever its state holds is never read.
struct XRowTgt { uint32_t k, r; };
static __host__ __device__ inline bool x_rt_wide(uint32_t t, uint32_t q){ return (uint64_t)t * q >= (1ull << 52) || ((t | q) >> 31) != 0u; }
// {k, r} of a q by one division: the quotient of two exact doubles (a q < 2^52 when a < t and the pair is inside the bound) is within half an ulp of v, so its
// truncation is k, or k + 1 where v rounded up to an integer: one correction.  t = 0 (a dead pair) has no target; rows past a short target (a >= t) and pairs
// outside the bound get values nothing reads, and nothing here can fault.
static __host__ __device__ inline XRowTgt x_rt_at(uint32_t a, uint32_t t, uint32_t q){
	XRowTgt s = {0u, 0u};
	if(t == 0u) return s;
	const uint64_t p = (uint64_t)a * q;
	const double y = (double)p / (double)t;
	uint32_t k = y < 4294967295.0 ? (uint32_t)y : 0u;
	int64_t r = (int64_t)(p - (uint64_t)k * t);
	if(r < 0){ k--; r += t; }
	s.k = k; s.r = (uint32_t)r;
	return s;
}
static __host__ __device__ inline void x_rt_step(XRowTgt &s, const XRowTgt &d, uint32_t t){
	s.k += d.k; s.r += d.r;
	if(s.r >= t){ s.r -= t; s.k++; }
}
// one step back (k may wrap below zero in front of row 0: the step forward undoes it)
static __host__ __device__ inline void x_rt_back(XRowTgt &s, const XRowTgt &d, uint32_t t){
	s.k -= d.k;
	if(s.r < d.r){ s.r += t; s.k--; }
	s.r -= d.r;
}
// the row's target becomes y (the double expression's k or k - 1 where r = 0; k itself elsewhere): r takes up the difference, a q = y t + r still holds with r <= t,
// and the next step's one carry brings r below t again because dr < t
static __host__ __device__ inline void x_rt_set(XRowTgt &s, uint32_t y, uint32_t t){
	s.r += (s.k - y) * t;
	s.k = y;
}
static __device__ __forceinline__ uint32_t x_q8(int v){ return (((uint32_t)v & 0xffu) << 8) * 0x00010001u; }        // value << 8 in both halves
static __device__ __forceinline__ uint32_t x_i16(int v){ return ((uint32_t)v & 0xffffu) * 0x00010001u; }            // plain int16 in both halves
static __device__ __forceinline__ int x_lo8(uint32_t x){ return __builtin_amdgcn_sbfe((int)x, 8, 8); }              // value of the low half (value << 8 form)
static __device__ __forceinline__ int x_hi8(uint32_t x){ return (int)x >> 24; }
static __device__ __forceinline__ int x_lo16(uint32_t x){ return __builtin_amdgcn_sbfe((int)x, 0, 16); }
static __device__ __forceinline__ int x_hi16(uint32_t x){ return (int)x >> 16; }

// (no dpp_keep here: every consumer of these moves is a packed, a three-operand or a select instruction, none of which can
// absorb a DPP operand, so the v_subrev_u32_dpp fold that bsa_dpp.h guards against cannot happen)
#define XDPP(old, x, ctrl, bank) ((uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(x), (ctrl), 0xf, (bank), false))
// lanes without a source read 0 (bound_ctrl): the same values as XDPP(0, ...), but the compiler need not put a zero into the destination first -- with
// old = 0 every one of these moves was preceded by a v_mov_b32 v, 0 (ten a row on the headline shape)
#define XDPPZ(x, ctrl, bank) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), (ctrl), 0xf, (bank), true))
#define XQP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
#define XROW_SHL(n) (0x100 + (n))
#define XROW_SHR(n) (0x110 + (n))
#define XHALF_MIRROR 0x141

// A pair owns a group of L = 8 or 4 consecutive lanes (two or four groups per 16-lane DPP row).
// value of the first / last lane of every group, in all its lanes
template<int L> static __device__ __forceinline__ uint32_t x_bcast_first(uint32_t x){
	const uint32_t s = XDPPZ(x, XQP(0, 0, 0, 0), 0xf);
	if constexpr (L == 4) return s;
	else return XDPP(s, s, XROW_SHR(4), 0xA);          // lanes 4..7 <- lanes 0..3
}
template<int L> static __device__ __forceinline__ uint32_t x_bcast_last(uint32_t x){
	const uint32_t s = XDPPZ(x, XQP(3, 3, 3, 3), 0xf);
	if constexpr (L == 4) return s;
	else return XDPP(s, s, XROW_SHL(4), 0x5);          // lanes 0..3 <- lanes 4..7
}
// block b receives the value of block b - 1 (low half: block l, high half: block l + L); block 0 receives fill_lo
template<int L> static __device__ __forceinline__ uint32_t x_shift_down(uint32_t x, uint32_t fill_lo, bool first){
	if constexpr (L == 4){
		// a pair is one DPP quad: ONE rotation brings every lane its neighbour and lane 0 the last lane's value, ONE byte permute (the
		// selector is a loop invariant of the lane) puts that value's low half above the fill in lane 0 and leaves the others as they are
		const uint32_t r = XDPPZ(x, XQP(3, 0, 1, 2), 0xf);
		return __builtin_amdgcn_perm(r, fill_lo, first ? 0x05040100u : 0x07060504u);
	}
	const uint32_t s = XDPPZ(x, XROW_SHR(1), 0xf);
	const uint32_t w = XDPPZ(x, XROW_SHL(L - 1), 0xf);  // first lane <- last lane
	const uint32_t fix = (w << 16) | (fill_lo & 0xffffu);
	return first ? fix : s;
}
// block b receives the value of block b + 1; block 2L - 1 receives fill (given in both halves)
template<int L> static __device__ __forceinline__ uint32_t x_shift_up(uint32_t x, uint32_t fill, bool last){
	if constexpr (L == 4){
		const uint32_t r = XDPPZ(x, XQP(1, 2, 3, 0), 0xf);             // (lane 3 receives lane 0's value: its high half goes below the fill)
		return __builtin_amdgcn_perm(fill, r, last ? 0x05040302u : 0x03020100u);
	}
	const uint32_t s = XDPPZ(x, XROW_SHL(1), 0xf);
	const uint32_t w = XDPPZ(x, XROW_SHR(L - 1), 0xf);  // last lane <- first lane
	const uint32_t fix = __builtin_amdgcn_alignbit(fill, w, 16);        // {fill.lo, w.hi}
	return last ? fix : s;
}
// inclusive prefix maximum over the lanes of a group, per half (Sklansky: nothing crosses a group)
template<int L> static __device__ __forceinline__ uint32_t x_scan_max(uint32_t x){
	// (both quad permutes give every lane a source: the bound_ctrl form has the same values and no `old` operand, which cost a v_mov_b32 a step)
	uint32_t y = XDPPZ(x, XQP(0, 0, 2, 2), 0xf); x = x_max(x, y);
	y = XDPPZ(x, XQP(0, 1, 1, 1), 0xf); x = x_max(x, y);
	if constexpr (L == 8){
		const uint32_t z = XDPP(x, x, XQP(3, 3, 3, 3), 0xf);
		y = XDPP(x, z, XROW_SHR(4), 0xA); x = x_max(x, y);
	}
	return x;
}
// sum over the lanes of a group, per half, in every lane
template<int L> static __device__ __forceinline__ uint32_t x_sum(uint32_t x){
	x = x_add(x, XDPPZ(x, XQP(1, 0, 3, 2), 0xf));
	x = x_add(x, XDPPZ(x, XQP(2, 3, 0, 1), 0xf));
	if constexpr (L == 8) x = x_add(x, XDPPZ(x, XHALF_MIRROR, 0xf));
	return x;
}
// the same sum of one 32-bit number a lane: a plain add takes the DPP operand itself (v_add_u32_dpp), a packed one cannot
template<int L> static __device__ __forceinline__ uint32_t x_sum32(uint32_t x){
	x += XDPPZ(x, XQP(1, 0, 3, 2), 0xf);
	x += XDPPZ(x, XQP(2, 3, 0, 1), 0xf);
	if constexpr (L == 8) x += XDPPZ(x, XHALF_MIRROR, 0xf);
	return x;
}
// |a.lo - b.lo| + |a.hi - b.hi| + c, the halves read as UNSIGNED 16-bit numbers, the sum one 32-bit number (v_sad_u16)
static __device__ __forceinline__ uint32_t x_sad(uint32_t a, uint32_t b, uint32_t c){ return __builtin_amdgcn_sad_u16(a, b, c); }

template<int W>
static __device__ __forceinline__ void x_load_qcodes(const uint8_t *p, uint32_t *w){
	if constexpr (W >= 4) __builtin_memcpy(w, p, W);
	else if constexpr (W == 2){ uint16_t v; __builtin_memcpy(&v, p, 2); w[0] = v | 0x04040000u; }
	else w[0] = p[0] | 0x04040400u;
}


// W cells per lane and half, L lanes per pair: 2 L blocks of W cells; the reference's 16 running blocks have WR = 2 L W / 16
// cells, so a block here holds CR = 8 / L of them
// PW = 2: two-piece gaps.  The frame is shifted by the extension of piece 1, so piece 2 keeps a real step dP = gape2 - gape1 > 0:
//   qq = U - NQ      m = max(ee, qq, S~)      g = max(g, max(m, f) + gapo2) + dP - U      NQ' = min(h - qq, -gapo2) - dP
// and a cell has nine facts (bsa_common.h "COMPACT slot", 8 bits): M, D, D2, which chain equals h (I1, I2), R1, R2, Od1, Od2.
// STATIC: every pair of the launch has a band that covers its whole query (Align8Args::static_band): the band never moves, so
// the row is kept in place -- no speculative slide, no corrections of it, no band steering.
// Row segments (k_align8_fwd_xq): the rows [row0, row1) of the pairs (row0, row1 multiples of 8, so that no group of four code rows
// and no group of L band offsets is open at a cut); `st` = the wave's state block (XS_WORDS(W, PW) x 64 dwords, dword r of lane l at
// st[64 r + l]): loaded when row0 != 0, stored when a pair has rows left behind row1.  tid_base + threadIdx.x = the lane's index among
// the launch's lanes (L consecutive ones share a pair).  The plain kernels pass row0 = 0, row1 = 0xFFFFFFF8, st = nullptr.
#define XS_WORDS(W, PW) ((((PW) == 2) ? 3 : 2) * (W) + 11)
// NWV: waves per workgroup.  The code dwords of a group of four rows wait in LDS (a lane's own sixteen dwords, no synchronisation) until
// the group is complete and leaves as 16-byte pieces: kept in registers they were twelve of the 168 a wave may have at three per SIMD.
// (Stored row by row as four-byte pieces the same launch takes 40 % longer.)
// DO2 (one-piece gaps with 1 <= -gapo <= 3, bandwidth 128; Align8Args::code_fmt == 1): D and Od of a cell leave as ONE two-bit field,
// the new e-difference min(h - ee, -gapo) itself (0: D, -gapo: Od) -- one multiply-add a cell where the two planes take four
// instructions.  A reference block's dword is then M | R << 8 | field of cell c at bits 31 - 2c, 30 - 2c (bsa_common.h).
// EXT: the two LDS areas come from the caller (k_align8_fwd_x_mix runs two shapes of this function in one launch and a block only ever one of
// them: they share the areas instead of each instantiation carrying its own).
// SCORE (BSA_MODE_SCORE_ONLY, one-piece gaps): the recurrence and the band steering only -- no flags, no code rows, no band offsets.  The pair's slot
// is a record of fixed size (bsa_score_rec_bytes): the final score (global) or the end record bsa_code_end_t and the last row's u bytes (overlap /
// extend), read by k_align8_score_finish (bsa_align8_codes.hip).
template<int W, int L, int PW = 1, bool STATIC = false, int NWV = 4, bool DO2 = false, bool EXT = false, bool SCORE = false>
static __device__ __forceinline__ void x_forward(const Align8Args &a, const uint32_t first_pos, const uint32_t count, const uint32_t tid_base,
		const uint32_t row0 = 0u, const uint32_t row1 = 0xFFFFFFF8u, uint32_t *st = nullptr, uint32_t *ext_stage = nullptr, uint32_t *ext_qwin = nullptr){
	constexpr int BW = 2 * L * W;
	constexpr int WR = BW / 16, CR = 8 / L;
	static_assert((L == 8 || L == 4) && W * L / 8 == WR && (CR == 1 || (CR == 2 && (W == 16 || W == 8))), "supported shapes");
	constexpr int NQ = (W + 3) / 4;
	constexpr int NACC = (W + 7) / 8;                     // flag accumulators per plane (8 cells each)
	constexpr int TOPBIT = 8 + ((W < 8) ? W : 8) - 1;     // accumulator bit of the first cell it holds
	static_assert(PW == 0 || PW == 1 || (PW == 2 && ((W == 8 && (L == 8 || L == 4)) || (W == 16 && (L == 8 || L == 4)))), "two-piece gaps: bandwidth 128 (eight lanes per pair), 64 (four), 256 (eight, sixteen cells a half)");
	static_assert(!DO2 || (PW == 1 && WR == 8), "two-bit D / Od fields: one-piece gaps, bandwidth 128");
	static_assert(!SCORE || (PW <= 1 && !DO2 && !EXT), "score-only: one-piece gaps, plain code format, own LDS");
	constexpr int NDO = DO2 ? W / 4 : 1;                  // accumulators of the two-bit fields (four cells each, in the high byte of a half)
	constexpr int CWD = (PW == 2) ? WR / 4 : (WR >= 8) ? WR / 8 : 1;          // code dwords per reference block and row (two-piece gaps: eight bits a cell)
	constexpr int ND = (PW == 2) ? 2 * W / 4 : (WR == 8) ? 2 * NACC : (WR == 16) ? 4 : (W == 8) ? 4 : 2;      // code dwords per lane and row
	const int lt = threadIdx.x;
	const int jl = lt & (L - 1);
	const bool first = jl == 0, last = jl == L - 1;
	const uint32_t g = (tid_base + (uint32_t)lt) / (uint32_t)L;
	const bool live = g < count;
	const uint32_t ppos = first_pos + (live ? g : 0u);
	const uint32_t pair = a.order[ppos];
	const uint32_t qlen = a.qlen[pair];
	uint32_t tlen = a.tlen[pair];
	const uint8_t *qp = a.qst + a.qpoff[pair], *tp = a.tst + a.tpoff[pair];
	int *begs = (int*)(a.rows + a.slot_off[ppos]);          // (SCORE: the pair's record)
	uint8_t *rowp = (uint8_t*)begs + bsa_begs_bytes(tlen);
	if(!live || a.status[pair] != 0u) tlen = 0;

	const int mode = a.mode & 3;
	const int gapo1 = a.gapo1, gape1 = a.gape1;
	const int GE = gape1, GO = gapo1;                      // GO <= 0, GE <= 0 (bsa_align8_x_supported)
	const uint32_t GOQ = x_q8(GO);                         // gapo, value << 8
	const uint32_t NGOQ = x_q8(-GO), NGOQ1 = x_q8(-GO - 1);
	const uint32_t ONE = 0x01000100u;
	uint32_t TWO = 0x00020002u;
	asm volatile("" : "+s"(TWO));                          // opaque multiplier of x_acc
	// DO2: cell j of an accumulator's four goes to bits 15 - 2j, 14 - 2j of the half: multipliers 64, 16, 4 (and 1: an addition)
	uint32_t KDO0 = 0x00400040u, KDO1 = 0x00100010u, KDO2 = 0x00040004u;
	asm volatile("" : "+s"(KDO0), "+s"(KDO1), "+s"(KDO2));
	const uint32_t DOSP = (GO == -1) ? 2u : 1u;            // a field value that is neither 0 (D) nor -gapo (Od)
	const uint32_t MINF = x_q8(BSA_EPI8_MIN - 2 * GE);     // the -63 sentinel of f in the shifted frame
	const uint32_t NGEQ = x_q8(-GE);                       // a cell with u = 0
	const int gapo2 = a.gapo2, gape2 = a.gape2;
	const int DP = (PW == 2) ? gape2 - gape1 : 0;          // > 0
	const int gopen = (PW == 2) ? gapo2 + gape2 : gapo1 + gape1;
	const int cfirst = min(a.smin, gopen) - 1 - a.smax + gopen;                        // bsalign.h:2362
	const int dsw = (PW == 2) ? (gapo1 - gapo2) / (gape2 - gape1) : 0x7FFFFFFF;         // new cells beyond this distance extend with piece 2 (bsalign.h:2369-2389)
	// cells entering at the band end (bsalign.h:2357-2389): u = cfirst for the first one, gape1 (gape2) after it, e = q = 0
	const uint32_t NEWU0 = x_q8(cfirst - GE), NEWNE = (PW == 0) ? 0u : x_q8(GE);
	const uint32_t GQQ = x_q8(gapo2), NGQQ = x_q8(-gapo2), NGQQ1 = x_q8(-gapo2 - 1), DPQ = x_q8(DP);
	const uint32_t GE16 = x_i16(GE), WGE16 = x_i16(W * GE);
	const uint32_t PADS = (uint32_t)((BSA_EPI8_MIN - 2 * GE) & 0xff) * 0x01010101u;    // S~ beyond the query end
	// S~ rows per target base: four dwords in LDS, read by the lanes with their row's base as the index (every wave of the block writes the same values)
	__shared__ uint32_t x_mtab[4];
	if((lt & 63) < 4){
		const int t = lt & 3;
		uint32_t w = 0;
#pragma unroll
		for(int q = 0; q < 4; q++) w |= (uint32_t)(((int)a.matrix[q * 4 + t] - 2 * GE) & 0xff) << (8 * q);
		x_mtab[t] = w;
	}
	__builtin_amdgcn_wave_barrier();

	uint32_t U[W], NE[W], NQ2[(PW == 2) ? W : 1];     // NQ2: gape1 - q of piece 2
	uint32_t PN;                  // packed int16: ubegs[b+1] - ubegs[0] - (b+1) W gape for b = jl (low) and jl + L (high)
	uint32_t PM = 0;              // CR == 2: the same for the middle of the block (the end of its first reference block)
	int HB;                       // ubegs[0]
	uint32_t svU = 0, svNE = 0, svNQ = 0; // first cell of the row before the speculative slide (lane 0, low half: band position 0)
	uint32_t rbeg = 0, mov = 0, i = row0;
	int cand_sc = BSA_SCORE_MIN, cand_te = 0;       // overlap / extend: best end-of-query score this lane has seen, and its row
	// ---- row -1 (bsalign.h:2094-2140)
	if(row0 == 0u){
		const int first_u = (int)(int8_t)(gapo1 + gape1 + a.smin - a.smax);
		const int xp = (PW == 2) ? (gapo2 - gapo1) / (gape1 - gape2) : 0x7FFFFFFF;      // row -1 extends with piece 2 from here on (bsalign.h:2115-2125)
		auto u_init = [&](int p) -> int { return (mode == BSA_MODE_OVERLAP) ? 0 : (p == 0) ? first_u : (p < xp) ? gape1 : gape2; };
#pragma unroll
		for(int k = 0; k < W; k++){
			const int vlo = u_init(jl * W + k), vhi = u_init((jl + L) * W + k);
			U[k] = (((uint32_t)(vlo - GE) & 0xffu) << 8) | (((uint32_t)(vhi - GE) & 0xffu) << 24);
			NE[k] = (PW == 0) ? 0u : x_q8(GE - BSA_EPI8_MIN);      // linear gaps: e is the constant gape1 (bsalign.h:2779), NE stays 0
			if constexpr (PW == 2) NQ2[k] = x_q8(GE - BSA_EPI8_MIN);
		}
		if(mode == BSA_MODE_OVERLAP){
			PN = ((uint32_t)(-(jl + 1) * W * GE) & 0xffffu) | ((uint32_t)(-(jl + L + 1) * W * GE) << 16);
			PM = x_add(PN, x_i16((W / 2) * GE));
			HB = 0;
		} else {
			// sum of (u - gape1) over the cells in front of the block's end
			auto pn_at = [&](int cells) -> int { return (first_u - GE) + DP * max(0, cells - max(xp, 1)); };
			auto pn_init = [&](int b) -> int { return pn_at((b + 1) * W); };
			PN = ((uint32_t)pn_init(jl) & 0xffffu) | ((uint32_t)pn_init(jl + L) << 16);
			PM = ((uint32_t)pn_at(jl * W + W / 2) & 0xffffu) | ((uint32_t)pn_at((jl + L) * W + W / 2) << 16);       // (the same number with one piece; with two, piece 2's cells in the block's second half do not count yet)
			HB = a.smax - a.smin;
		}
	}
	// bring row -1 into the loop's form: slid by one cell, ubegs[0] not advanced
	if constexpr (!STATIC) if(row0 == 0u){
		const uint32_t t0u = U[0], t0e = NE[0];
#pragma unroll
		for(int k = 0; k + 1 < W; k++){ U[k] = U[k + 1]; NE[k] = NE[k + 1]; }
		const uint32_t inu = x_shift_up<L>(t0u, NEWU0, last), inne = x_shift_up<L>(t0e, NEWNE, last);
		U[W - 1] = inu; NE[W - 1] = inne;
		if constexpr (PW == 2){
			svNQ = NQ2[0];
#pragma unroll
			for(int k = 0; k + 1 < W; k++) NQ2[k] = NQ2[k + 1];
			NQ2[W - 1] = x_shift_up<L>(svNQ, NEWNE, last);
		}
		PN = x_add(x_add(PN, x_ashr8(inu)), GE16);
		if constexpr (CR == 2) PM = x_add(x_add(PM, x_ashr8(U[W / 2 - 1])), GE16);
		svU = t0u; svNE = t0e;
	}
	if(row0 != 0u){
		// the state the previous segment left (plain loads behind the acquire of k_align8_fwd_xq)
		const uint32_t *sp = st + (lt & 63);
		int r = 0;
#pragma unroll
		for(int k = 0; k < W; k++) U[k] = sp[64 * r++];
#pragma unroll
		for(int k = 0; k < W; k++) NE[k] = sp[64 * r++];
		if constexpr (PW == 2){
#pragma unroll
			for(int k = 0; k < W; k++) NQ2[k] = sp[64 * r++];
		}
		PN = sp[64 * r++]; PM = sp[64 * r++]; HB = (int)sp[64 * r++]; svU = sp[64 * r++]; svNE = sp[64 * r++]; svNQ = sp[64 * r++];
		rbeg = sp[64 * r++]; mov = sp[64 * r++]; cand_sc = (int)sp[64 * r++]; cand_te = (int)sp[64 * r++];
	}
	constexpr bool OWNSTG = !EXT && !SCORE;
	__shared__ uint32_t x_stage[OWNSTG ? NWV : 1][OWNSTG ? 4 * ND : 1][64];       // [wave][4 q + row of the group (CWD == 1) | ND row + dword (CWD >= 2)][lane]
	uint32_t *const stg = EXT ? ext_stage + (size_t)(lt >> 6) * (4 * ND * 64) + (lt & 63) : &x_stage[(OWNSTG && NWV > 1) ? (lt >> 6) : 0][0][lt & 63];
	// QUERY WINDOW.  A lane needs S~ of the W cells of each of its two blocks on every row, at a band offset that moves by about one base a
	// row: loaded from memory row by row that is one full round trip the wave waits for per row -- and `vmcnt` also holds the row's wait back behind the
	// code-row stores in flight (a second such round trip per row, added as an experiment, cost 5.4 ms of the 61: 9 %).  Instead the lane keeps, in LDS
	// slots of its own (no synchronisation, like the staging above), one dword per band column of its block pair, starting at the band offset of the last
	// refill: the byte-permute SELECTOR {0x0C, code of the low block's column, 0x0C, code of the high block's column}.  v_perm_b32(PADS, mr, selector) is then
	// the cell register's S~ {0, S~ low, 0, S~ high} in one instruction (0x0C selects a zero byte, code 4 the PADS byte): a row reads the W selectors at
	// the dword its offset has reached -- no shifting into place, no lookup of packed codes, no spreading of the looked-up bytes.  The selectors depend on
	// the query alone; they are built when the window is loaded, every 2 KD - W columns of band movement (about 15 rows), for all the live pairs of the wave at
	// once (below).  The staged query is padded far enough behind its end (plan: bandwidth + BSA_QPAD_TAIL bytes).
	constexpr bool QWIN = !STATIC && PW != 2 && W == 16;      // (measured: two-piece gaps at 251 registers lose 3 % with it, eight cells a half gain nothing)
	constexpr int KD = NQ + 12;   // the window is 2 KD dwords a lane
	constexpr int NSEL = 2 * KD;                          // selectors (band columns) in the window
	constexpr uint32_t QOFFMAX = (uint32_t)(NSEL - W);    // the last offset at which selectors off .. off + W - 1 are all inside
	static_assert(!QWIN || (NSEL % 4 == 0 && NSEL - W <= BSA_QPAD_TAIL), "a refill reads NSEL - W bytes behind the band's last block: the staged query's padding (bsa_api.hip: qpad = bandwidth + BSA_QPAD_TAIL) must cover it");
	__shared__ uint32_t x_qwin[(QWIN && !EXT) ? NWV : 1][(QWIN && !EXT) ? 2 * KD : 1][64];
	uint32_t *const qwp = EXT ? ext_qwin + (size_t)(lt >> 6) * (2 * KD * 64) + (lt & 63) : &x_qwin[(QWIN && !EXT && NWV > 1) ? (lt >> 6) : 0][0][lt & 63];
	uint32_t wbase = 0x40000000u;                          // band offset the window starts at (this value: no window yet)
	int begq = 0;
	if(!SCORE && tlen != 0u && first && row0 == 0u) begs[0] = 0;
	uint64_t twin = 0;
	if(row0 < tlen){ __builtin_memcpy(&twin, tp + row0, 8); twin <<= 2; }
	// STATIC: the band never moves, so a lane's query codes are the same on every row -- loaded once
	uint32_t sqlo[STATIC ? NQ : 1], sqhi[STATIC ? NQ : 1];
	if constexpr (STATIC){
#pragma unroll
		for(int n = 0; n < NQ; n++){ sqlo[n] = 0x04040404u; sqhi[n] = 0x04040404u; }
		if(tlen){ x_load_qcodes<W>(qp + jl * W, sqlo); x_load_qcodes<W>(qp + (jl + L) * W, sqhi); }
	}
	const int rbz = 2 * max((int)(tlen / max(qlen, 1u)), 1);          // bsalign.h:4008
	const bool rush32 = (unsigned long long)(uint32_t)rbz * tlen + qlen + (uint32_t)BW + (uint32_t)rbz < 0xFFFFFFFFull;
	// rbz * (rows left after this one), kept by subtraction: a 32-bit multiplication is a quarter-rate instruction and this one sat in every row
	uint32_t rzl = rush32 ? (uint32_t)rbz * (tlen - min(row0, tlen) - 1u) : 0u;
	int rby_tab = 0;
	const int rby_lane = (lt & (64 - L)) << 2;                   // byte address of lane 0 of this group for ds_bpermute
	const uint32_t kd1 = last ? 0x01000000u : 0u;          // band cell bw - 1 after a slide by one: x == bw, no deletion there (bsalign.h:3672-3678)

	// Wave-level tests: ONE vector compare into a scalar mask, the pair's liveness ANDed in on the scalar unit.  (`__any(act && x)` is the library's
	// __ockl_wfany_i32 on an `and` of two conditions: the backend materialises the predicate as 0 / 1 in a register and compares it again -- two to three
	// vector instructions a test, six tests a row.)
	uint64_t actm = 0;
	while(i < row1 && (actm = __builtin_amdgcn_ballot_w64(i < tlen)) != 0ull){
		const bool act = i < tlen;
		if(!STATIC && mode == BSA_MODE_GLOBAL && (i & (uint32_t)(L - 1)) == 0u)
			rby_tab = (int)((1.0 * (double)(i + (uint32_t)jl) / (double)tlen) * (double)qlen);      // bsalign.h:4009, row i + jl (measured: even a three-instruction f32 stand-in for the fifteen f64 instructions would give 0.1 - 0.3 ms of 57)
		// ---- band offset of this row (bsalign.h:3932-3946)
		if constexpr (!STATIC){
			// mov = (mov != 0 && rbeg + BW < qlen) ? min(mov, qlen - (rbeg + BW)) : 0 -- the room as a saturating difference makes it one minimum
			mov = min(mov, __builtin_elementwise_sub_sat(qlen, rbeg + (uint32_t)BW));
			rbeg += mov;
		}
		int rhj = 0;          // a band that jumps past everything it held: H at the last cell of the previous row (set in that branch, read for the first cell below)
		// ---- row_movx (bsalign.h:2244-2392): the row is held slid by one cell; correct what did not move that way
		if(!STATIC && __builtin_expect((__builtin_amdgcn_ballot_w64(mov != 1u) & actm) != 0ull, 0)){
			if(__any(act && mov >= (uint32_t)BW)){
				// the band jumped past everything it held: zero rows, every ubegs = SCORE_MIN (bsalign.h:2253-2259);
				const bool z = act && mov >= (uint32_t)BW;
				const uint32_t bc = x_bcast_last<L>(PN);
				const int rhz = HB + (x_hi16(bc) - cfirst) + BW * GE;
				if(z){
					rhj = rhz;
#pragma unroll
					for(int k = 0; k < W; k++){ U[k] = NGEQ; NE[k] = NEWNE; if constexpr (PW == 2) NQ2[k] = NEWNE; }
					HB = BSA_SCORE_MIN;
					PN = ((uint32_t)(-(jl + 1) * W * GE) & 0xffffu) | ((uint32_t)(-(jl + L + 1) * W * GE) << 16);
					PM = x_add(PN, x_i16((W / 2) * GE));
				}
			}
			if(__any(act && mov == 0u)){
				// undo the slide
				const bool d = act && mov == 0u;
				const uint64_t dm = __ballot(d);
				const uint32_t outu = U[W - 1];
				const uint32_t pu = x_shift_down<L>(outu, svU, first), pe = x_shift_down<L>(NE[W - 1], svNE, first);
				const uint32_t npn = x_sub(x_sub(PN, x_ashr8(outu)), GE16);
				PN = d ? npn : PN;
				if constexpr (CR == 2){ const uint32_t npm = x_sub(x_sub(PM, x_ashr8(U[W / 2 - 1])), GE16); PM = d ? npm : PM; }
#pragma unroll
				for(int k = W - 1; k >= 1; k--){ x_sel(U[k], U[k - 1], dm); x_sel(NE[k], NE[k - 1], dm); }
				x_sel(U[0], pu, dm); x_sel(NE[0], pe, dm);
				if constexpr (PW == 2){
					const uint32_t pq = x_shift_down<L>(NQ2[W - 1], svNQ, first);
#pragma unroll
					for(int k = W - 1; k >= 1; k--) x_sel(NQ2[k], NQ2[k - 1], dm);
					x_sel(NQ2[0], pq, dm);
				}
			}
			// one more cell at a time for steps of two and more (the first new cell went in with the speculative slide)
			for(uint32_t s = 1; __any(act && mov < (uint32_t)BW && s < mov); s++){
				const bool d = act && mov < (uint32_t)BW && s < mov;
				const uint64_t dm = __ballot(d);
				const uint32_t bc = x_bcast_first<L>(U[0]);
				const uint32_t D0 = __builtin_amdgcn_perm(bc, bc, 0x01000100u);
				const uint32_t NEWU1 = ((int)s >= dsw) ? DPQ : 0u;          // u = gape1, or gape2 beyond the switch distance
				const uint32_t inu = x_shift_up<L>(U[0], NEWU1, last), inne = x_shift_up<L>(NE[0], NEWNE, last);
				const uint32_t npn = x_add(PN, x_ashr8(x_sub(inu, D0)));
				PN = d ? npn : PN;
				if constexpr (CR == 2){ const uint32_t npm = x_add(PM, x_ashr8(x_sub(U[W / 2], D0))); PM = d ? npm : PM; }
				HB += d ? (x_lo8(bc) + GE) : 0;
#pragma unroll
				for(int k = 0; k + 1 < W; k++){ x_sel(U[k], U[k + 1], dm); x_sel(NE[k], NE[k + 1], dm); }
				x_sel(U[W - 1], inu, dm); x_sel(NE[W - 1], inne, dm);
				if constexpr (PW == 2){
					const uint32_t innq = x_shift_up<L>(NQ2[0], NEWNE, last);
#pragma unroll
					for(int k = 0; k + 1 < W; k++) x_sel(NQ2[k], NQ2[k + 1], dm);
					x_sel(NQ2[W - 1], innq, dm);
				}
			}
		}
		// ---- sequences, S~(x, y)
		uint32_t S[W];
		{
			// the target base of this row (i is uniform: the half of the eight-base window is picked on the scalar side), as the byte offset of its S~ row
			// (the window holds the bases times four: a base is 0 .. 3, so nothing crosses a byte)
			const uint32_t tw32 = (i & 4u) ? (uint32_t)(twin >> 32) : (uint32_t)twin;
			const uint32_t tb4 = __builtin_amdgcn_ubfe(tw32, 8u * (i & 3u), 4u);
			if constexpr (QWIN){
				uint32_t off = rbeg - wbase;
				if(__builtin_expect((__builtin_amdgcn_ballot_w64(off > QOFFMAX) & actm) != 0ull, 0)){
					// refill: the selectors of the NSEL columns from the band offset of this row on, for EVERY live pair of the wave, not only the one that has
					// run out: the sixteen pairs move at about the same rate, so their windows stay in step and this branch runs once in about 13 rows (refilled
					// each on its own, three in four rows would find some pair at its window's end and run the branch for one active pair)
					if(act){
						const uint8_t *pl = qp + rbeg + jl * W, *ph = qp + rbeg + (jl + L) * W;
						uint32_t bl[NSEL / 4], bh[NSEL / 4];
						__builtin_memcpy(bl, pl, NSEL); __builtin_memcpy(bh, ph, NSEL);
						// (the two selectors below have to be in vector registers -- the 0x0C dword takes the instruction's one scalar operand: made here, opaque,
						// so that they are not kept as invariants across the row loop, which has no register to spare)
						uint32_t PA = 0x02040004u, PB = 0x03040104u;
						asm volatile("" : "+v"(PA), "+v"(PB));
#pragma unroll
						for(int n = 0; n < NSEL / 4; n++){
							// {lo0, lo1, hi0, hi1} and {lo2, lo3, hi2, hi3} of the four columns, then each column's two codes between the 0x0C bytes
							const uint32_t y0 = __builtin_amdgcn_perm(bh[n], bl[n], 0x05040100u), y1 = __builtin_amdgcn_perm(bh[n], bl[n], 0x07060302u);
							qwp[64 * (4 * n)] = __builtin_amdgcn_perm(0x0C0C0C0Cu, y0, PA);
							qwp[64 * (4 * n + 1)] = __builtin_amdgcn_perm(0x0C0C0C0Cu, y0, PB);
							qwp[64 * (4 * n + 2)] = __builtin_amdgcn_perm(0x0C0C0C0Cu, y1, PA);
							qwp[64 * (4 * n + 3)] = __builtin_amdgcn_perm(0x0C0C0C0Cu, y1, PB);
						}
						wbase = rbeg; off = 0u;
					}
				}
				// (a lane whose pair has no row left computes on whatever its window holds: nothing of it is stored)
				const uint32_t *wl = qwp + 64u * (act ? off : 0u);
				const uint32_t mr = *(const uint32_t*)((const uint8_t*)x_mtab + tb4);
#pragma unroll
				for(int k = 0; k < W; k++) S[k] = __builtin_amdgcn_perm(PADS, mr, wl[64 * k]);
			} else {
			uint32_t qlo[NQ], qhi[NQ];
			if constexpr (STATIC){
#pragma unroll
				for(int n = 0; n < NQ; n++){ qlo[n] = act ? sqlo[n] : 0x04040404u; qhi[n] = act ? sqhi[n] : 0x04040404u; }
			} else if(act){ x_load_qcodes<W>(qp + rbeg + jl * W, qlo); x_load_qcodes<W>(qp + rbeg + (jl + L) * W, qhi); }
			else {
#pragma unroll
				for(int n = 0; n < NQ; n++){ qlo[n] = 0x04040404u; qhi[n] = 0x04040404u; }
			}
			// (a four-way select among uniform values compiles to three nested exec-mask regions with v_readlane hazards: one LDS read instead)
			const uint32_t mr = *(const uint32_t*)((const uint8_t*)x_mtab + tb4);
			uint32_t slo[NQ], shi[NQ];
#pragma unroll
			for(int n = 0; n < NQ; n++){ slo[n] = __builtin_amdgcn_perm(PADS, mr, qlo[n]); shi[n] = __builtin_amdgcn_perm(PADS, mr, qhi[n]); }
#pragma unroll
			for(int k = 0; k < W; k++){
				const uint32_t sel = 0x000C000Cu | ((uint32_t)(k & 3) << 8) | ((uint32_t)(4 + (k & 3)) << 24);   // {0, lo.byte[k], 0, hi.byte[k]}
				S[k] = __builtin_amdgcn_perm(shi[k >> 2], slo[k >> 2], sel);
			}
			}
		}
		// ---- first cell of the band (bsalign.h:2899-2907): h0 = rh - ubegs[0] + S, kept if >= u + e, else -63.  After a
		// slide inside the band rh == ubegs[0] and the rule changes neither h nor any flag, so only rows that stayed
		// (or jumped past the whole band: ubegs[0] = SCORE_MIN) need it.
		uint32_t hc0 = S[0];
		uint32_t q0m = 0, q0d = 0, q0d2 = 0;          // rows starting at query column 0: what h is compared with for M and D (bsalign.h:3763-3767)
		if(__builtin_expect((__builtin_amdgcn_ballot_w64(mov - 1u >= (uint32_t)BW - 1u) & actm) != 0ull, 0)){          // mov == 0 or mov >= BW
			// rh = H of the previous row left of the band's first cell: of its last cell after a jump, the row's own start value where the band has not moved
			// (a slide inside the band -- getscore(mov - 1) = ubegs[0] -- needs none: nothing below is used for such a pair)
			int rh;
			if(!STATIC && mov >= (uint32_t)BW) rh = rhj;
			else if(rbeg) rh = BSA_SCORE_MIN;
			else if(mode == BSA_MODE_OVERLAP || i == 0) rh = 0;
			else if(PW < 2) rh = gapo1 + gape1 * (int)i;
			else rh = max(gapo1 + gape1 * (int)i, gapo2 + gape2 * (int)i);
			const int s0 = x_lo8(S[0]) + 2 * GE, u0 = x_lo8(U[0]) + GE, e0 = GE - x_lo8(NE[0]);
			const int qq0 = (PW == 2) ? GE - x_lo8(NQ2[0]) : e0;
			const int t0 = u0 + max(e0, qq0);
			int hh = (rh - HB) + s0;
			hh = (hh >= t0) ? min(hh, BSA_EPI8_MAX) : BSA_EPI8_MIN;
			if(first && (mov == 0u || mov >= (uint32_t)BW)) hc0 = (hc0 & 0xffff0000u) | (((uint32_t)(hh - 2 * GE) & 0xffu) << 8);
			// compare values of the quirk, in the shifted frame; out of int8 range = never equal
			const int cm = rh - HB + s0 - 2 * GE, cd = u0 + e0 + rh - HB - 2 * GE, cd2 = u0 + qq0 + rh - HB - 2 * GE;
			q0m = (cm >= -128 && cm <= 127) ? (((uint32_t)cm & 0xffu) << 8) : 0x00ffu;
			q0d = (cd >= -128 && cd <= 127) ? (((uint32_t)cd & 0xffu) << 8) : 0x00ffu;
			q0d2 = (cd2 >= -128 && cd2 <= 127) ? (((uint32_t)cd2 & 0xffu) << 8) : 0x00ffu;
		}
		// ---- row_cal, pass 1 (bsalign.h:2911-2930): F leaving every block when nothing but the sentinel enters it
		uint32_t ee[W], m[W], mg[W], qq[(PW == 2) ? W : 1], Ud[(PW == 2) ? W : 1];
		uint32_t f = MINF, g2 = MINF;
#pragma unroll
		for(int k = 0; k < W; k++){
			ee[k] = x_sub(U[k], NE[k]);
			if constexpr (PW == 2){
				qq[k] = x_sub(U[k], NQ2[k]);
				Ud[k] = x_sub(U[k], DPQ);
				m[k] = x_max(x_max(ee[k], qq[k]), (k == 0) ? hc0 : S[k]);
				const uint32_t t = x_add(x_max(m[k], f), GQQ);
				g2 = x_sub(x_max(g2, t), Ud[k]);
			} else m[k] = x_max(ee[k], (k == 0) ? hc0 : S[k]);
			mg[k] = x_add(m[k], GOQ);
			f = x_sub(x_max(f, mg[k]), U[k]);
		}
		// ---- F-penetration (bsalign.h:2639-2652) as a prefix maximum over the blocks
		{
			const uint32_t Fa = x_add(x_ashr8(f), PN);
			const uint32_t P = x_scan_max<L>(Fa);
			const uint32_t bc = x_bcast_last<L>(P);
			const uint32_t Thi = (bc << 16) | 0x8000u;              // {-32768, max over blocks 0..7}
			const uint32_t G = x_sub(x_max(P, Thi), PN);
			f = x_shl8(x_shift_down<L>(G, x_i16(BSA_EPI8_MIN - 2 * GE), first));
			if constexpr (PW == 2){
				// the chain of piece 2 gains dP per cell on its way: the same scan on X - (b + 1) W dP
				const uint32_t PN2 = x_sub(PN, ((uint32_t)((jl + 1) * W * DP) & 0xffffu) | ((uint32_t)((jl + L + 1) * W * DP) << 16));
				const uint32_t Fb = x_add(x_ashr8(g2), PN2);
				const uint32_t P2 = x_scan_max<L>(Fb);
				const uint32_t bc2 = x_bcast_last<L>(P2);
				const uint32_t G2 = x_sub(x_max(P2, (bc2 << 16) | 0x8000u), PN2);
				g2 = x_shl8(x_shift_down<L>(G2, x_i16(BSA_EPI8_MIN - 2 * GE), first));
			}
		}
		// ---- pass 2 (bsalign.h:2932-2957), flags, new row written one slot to the left
		uint32_t accM[NACC], accD[NACC], accR[NACC], accO[NACC], accDO[NDO];
#pragma unroll
		for(int n = 0; n < NDO; n++) accDO[n] = 0;
		uint32_t accD2[NACC], accI1[NACC], accI2[NACC], accR2[NACC], accO2[NACC];          // PW == 2
#pragma unroll
		for(int n = 0; n < NACC; n++){ accD2[n] = 0; accI1[n] = 0; accI2[n] = 0; accR2[n] = 0; accO2[n] = 0; }
#pragma unroll
		for(int n = 0; n < NACC; n++){ accM[n] = 0; accD[n] = 0; accR[n] = 0; accO[n] = 0; }
		uint32_t tmpU0 = 0, tmpNE0 = 0, tmpNQ0 = 0, hfirst = 0;
		uint32_t v = 0, vmid = 0;
#pragma unroll
		for(int k = 0; k < W; k++){
			const uint32_t uk = U[k];
			uint32_t h = x_max(m[k], f);
			uint32_t nq = 0;
			if constexpr (PW == 2){
				const uint32_t t = x_add(h, GQQ);                  // max(m, f) + gapo2
				h = x_max(h, g2);
				accI1[k >> 3] = x_acc(accI1[k >> 3], x_minu(x_sub(h, f), ONE), TWO);
				accI2[k >> 3] = x_acc(accI2[k >> 3], x_minu(x_sub(h, g2), ONE), TWO);
				const uint32_t gm = x_max(g2, t);
				g2 = x_sub(gm, Ud[k]);
				accR2[k >> 3] = x_acc(accR2[k >> 3], x_minu(x_sub(gm, t), ONE), TWO);
				const uint32_t n2 = x_sub(h, qq[k]);
				accD2[k >> 3] = x_acc(accD2[k >> 3], x_minu(n2, ONE), TWO);
				const uint32_t nqd = x_minu(n2, NGQQ);
				accO2[k >> 3] = x_acc(accO2[k >> 3], x_satsubu(nqd, NGQQ1), TWO);
				nq = x_sub(nqd, DPQ);
			}
			const uint32_t fm = x_max(f, mg[k]);
			f = x_sub(fm, uk);
			if constexpr (PW != 0 && !SCORE) accR[k >> 3] = x_acc(accR[k >> 3], x_minu(x_sub(fm, mg[k]), ONE), TWO);
			const uint32_t n = x_sub(h, ee[k]);
			const uint32_t ne = (PW == 0) ? 0u : x_minu(n, NGOQ);
			if constexpr (SCORE){}
			else if constexpr (DO2){
				const uint32_t kk = ((k & 3) == 0) ? KDO0 : ((k & 3) == 1) ? KDO1 : KDO2;
				if((k & 3) == 3) accDO[k >> 2] = x_add(accDO[k >> 2], ne);
				else accDO[k >> 2] = x_acc(ne, accDO[k >> 2], kk);                 // ne * K + acc
			} else {
				accD[k >> 3] = x_acc(accD[k >> 3], x_minu(n, ONE), TWO);
				if constexpr (PW != 0) accO[k >> 3] = x_acc(accO[k >> 3], x_satsubu(ne, NGOQ1), TWO);
			}
			if constexpr (!SCORE) accM[k >> 3] = x_acc(accM[k >> 3], x_minu(x_sub(h, S[k]), ONE), TWO);
			const uint32_t un = x_sub(h, v);
			v = x_sub(h, uk);
			if(CR == 2 && k == W / 2 - 1) vmid = v;
			if(k == 0){ tmpU0 = un; tmpNE0 = ne; tmpNQ0 = nq; hfirst = h; }
			else if constexpr (STATIC){ U[k] = un; NE[k] = ne; if constexpr (PW == 2) NQ2[k] = nq; }       // in place (U[k] was read above)
			else { U[k - 1] = un; NE[k - 1] = ne; if constexpr (PW == 2) NQ2[k - 1] = nq; }
		}
		// ---- tail (bsalign.h:2618-2636): u of every block's first cell, ubegs of the new row, ubegs[0] re-based on cell 0
		const uint32_t vlast = v;
		tmpU0 = x_sub(tmpU0, x_shift_down<L>(vlast, NGEQ, first));
		const uint32_t bc0 = x_bcast_first<L>(tmpU0);
		{
			const uint32_t D0 = __builtin_amdgcn_perm(bc0, bc0, 0x01000100u);
			HB += x_lo8(bc0) + GE;
			PN = x_add(PN, x_ashr8(x_sub(vlast, D0)));
			if constexpr (CR == 2) PM = x_add(PM, x_ashr8(x_sub(vmid, D0)));
		}
		if(first) tmpU0 = (tmpU0 & 0xffff0000u) | (NGEQ & 0xffffu);
		const uint32_t Psh = x_shift_down<L>(PN, 0u, first);           // ubegs[b] - ubegs[0] - b W gape of the block's own start
		// ---- flags of special cells, then the code row (bsa_common.h "COMPACT slot"); M, D, R were accumulated inverted
		if constexpr (!SCORE){
		if(__builtin_expect((__builtin_amdgcn_ballot_w64(rbeg == 0u) & actm) != 0ull, 0)){
			if(first && rbeg == 0u){
				const uint32_t hl = hfirst & 0xffffu;
				const uint32_t b0 = 1u << TOPBIT;
				accM[0] = (accM[0] & ~b0) | ((hl == q0m) ? 0u : b0);
				if constexpr (DO2){
					// band position 0 of a row whose band starts at query column 0: D follows the quirk's comparison and need not agree with the
					// field, so this one cell carries D and Od literally (bit 14: D, bit 15: Od); the traceback knows it by x == 0 == band offset
					const uint32_t fld = (accDO[0] >> 14) & 3u;
					accDO[0] = (accDO[0] & ~0xC000u) | ((hl == q0d) ? 0x4000u : 0u) | ((fld == (uint32_t)(-GO)) ? 0x8000u : 0u);
				} else
				accD[0] = (accD[0] & ~b0) | ((hl == q0d) ? 0u : b0);
				if constexpr (PW == 2) accD2[0] = (accD2[0] & ~b0) | ((hl == q0d2) ? 0u : b0);
			}
		}
		if(__builtin_expect((__builtin_amdgcn_ballot_w64(mov > 1u) & actm) != 0ull, 0)){          // (the general form covers mov == 1 of the other pairs of the wave)
			// cells at / beyond the end of the previous row's band: x == bw decides M or I only, x > bw is always I
#pragma unroll
			for(int hf = 0; hf < 2; hf++){
				const int lim = BW - (int)mov - (jl + L * hf) * W;                 // cells k < lim have x < bw
				const int nd = min(max(lim, 0), W), nm = min(max(lim + 1, 0), W);
#pragma unroll
				for(int n = 0; n < NACC; n++){
					constexpr int CN = (W < 8) ? W : 8;
					// accumulator n holds cells 8n .. 8n + CN - 1, cell c at bit 8 + CN - 1 - (c - 8n)
					const int cd = min(max(nd - 8 * n, 0), CN), cm = min(max(nm - 8 * n, 0), CN);
					const uint32_t md = (((1u << (CN - cd)) - 1u) << 8) << (16 * hf), mm = (((1u << (CN - cm)) - 1u) << 8) << (16 * hf);
					if(mov != 0u){ if constexpr (!DO2) accD[n] |= md; accM[n] |= mm; if constexpr (PW == 2) accD2[n] |= md; }
				}
				if constexpr (DO2){
					// "no deletion here" = a zero field becomes the spare value: cells nd .. W - 1 of the half
#pragma unroll
					for(int n = 0; n < NDO; n++){
						const int c0 = min(max(nd - 4 * n, 0), 4);                    // the accumulator's cells c0 .. 3 (bits 15 - 2c, 14 - 2c)
						const uint32_t cm = (0x5500u & ((1u << (16 - 2 * c0)) - 1u)) << (16 * hf);
						const uint32_t z = ~(accDO[n] | (accDO[n] >> 1)) & cm;       // low bit of every zero field among them
						if(mov != 0u) accDO[n] |= z * DOSP;
					}
				}
			}
		} else if constexpr (DO2){
			const uint32_t t = accDO[NDO - 1];
			if(mov == 1u && last && (t & 0x03000000u) == 0u) accDO[NDO - 1] = t | (DOSP << 24);
		} else { accD[NACC - 1] |= (mov == 1u) ? kd1 : 0u; if constexpr (PW == 2) accD2[NACC - 1] |= (mov == 1u) ? kd1 : 0u; }
		if constexpr (PW == 0){
			// linear gaps: every gap is opened at length 1 (R and Od always set); accR is kept inverted, accO is not
#pragma unroll
			for(int n = 0; n < NACC; n++){ accR[n] = 0u; accO[n] = (W >= 8) ? 0xFF00FF00u : (((1u << W) - 1u) << 8) * 0x00010001u; }
		}
		// The code dwords of this row: ND per lane.  Rows are stored in groups of four (bsa_common.h): the lane keeps the
		// dwords of the group's rows in registers and stores whole 16-byte pieces when the group (or the pair) ends.
		{
			uint32_t cur[ND];
			if constexpr (PW == 2){
				// eight facts a cell (bsa_common.h): planes A, D, D2, B | R1, R2, Od1, Od2 of a reference block, W_R bits each.
				// M, D, D2, I1, I2, R1, R2 were accumulated inverted; the decision facts fold into A = M or (no D, no D2, I1 and I2),
				// B = not M and I1 (bit-wise on the planes, after the special cells were set above)
				const uint32_t F8 = 0xFF00FF00u;
				uint32_t pl[8][NACC];                 // the eight planes as they are stored (not inverted), cells in bits 15 .. 8 of each half
#pragma unroll
				for(int n = 0; n < NACC; n++){
					const uint32_t nA = accM[n] & (accI1[n] | accI2[n] | (~(accD[n] & accD2[n]) & F8));
					const uint32_t nB = (~accM[n] & F8) | accI1[n];
					pl[0][n] = ~nA & F8; pl[1][n] = ~accD[n] & F8; pl[2][n] = ~accD2[n] & F8; pl[3][n] = ~nB & F8;
					pl[4][n] = ~accR[n] & F8; pl[5][n] = ~accR2[n] & F8; pl[6][n] = accO[n] & F8; pl[7][n] = accO2[n] & F8;
				}
				if constexpr (WR == 8){
					// two dwords per reference block: A | D << 8 | D2 << 16 | B << 24 and R1 | R2 << 8 | Od1 << 16 | Od2 << 24; a half holds NACC blocks
#pragma unroll
					for(int n = 0; n < NACC; n++){
						const uint32_t t1 = __builtin_amdgcn_perm(pl[1][n], pl[0][n], 0x07030501u);        // {A.lo, D.lo, A.hi, D.hi}
						const uint32_t t2 = __builtin_amdgcn_perm(pl[3][n], pl[2][n], 0x07030501u);        // {D2.lo, B.lo, D2.hi, B.hi}
						const uint32_t t3 = __builtin_amdgcn_perm(pl[5][n], pl[4][n], 0x07030501u);
						const uint32_t t4 = __builtin_amdgcn_perm(pl[7][n], pl[6][n], 0x07030501u);
						cur[2 * n] = __builtin_amdgcn_perm(t2, t1, 0x05040100u); cur[2 * n + 1] = __builtin_amdgcn_perm(t4, t3, 0x05040100u);                         // block NACC jl + n
						cur[2 * (NACC + n)] = __builtin_amdgcn_perm(t2, t1, 0x07060302u); cur[2 * (NACC + n) + 1] = __builtin_amdgcn_perm(t4, t3, 0x07060302u);     // block NACC (jl + L) + n
					}
				} else if constexpr (WR == 4){
					// bandwidth 64: a half holds two reference blocks of four cells (bits 15 .. 12 and 11 .. 8); one dword a block, plane j at bits 4 j
					uint32_t pa = 0, pb = 0;              // per half 16 bits: planes 0 .. 3 of block a / b; then planes 4 .. 7
					uint32_t qa = 0, qb = 0;
#pragma unroll
					for(int j = 0; j < 4; j++){
						pa |= ((pl[j][0] >> 12) & 0x000F000Fu) << (4 * j); pb |= ((pl[j][0] >> 8) & 0x000F000Fu) << (4 * j);
						qa |= ((pl[4 + j][0] >> 12) & 0x000F000Fu) << (4 * j); qb |= ((pl[4 + j][0] >> 8) & 0x000F000Fu) << (4 * j);
					}
					cur[0] = (pa & 0xFFFFu) | (qa << 16); cur[1] = (pb & 0xFFFFu) | (qb << 16);                 // blocks 2 jl, 2 jl + 1
					cur[2] = (pa >> 16) | (qa & 0xFFFF0000u); cur[3] = (pb >> 16) | (qb & 0xFFFF0000u);       // blocks 2 (jl + L), 2 (jl + L) + 1
				} else {
					// bandwidth 256: a half is one reference block of sixteen cells; four dwords a block, plane j in the halfword j of them
					uint32_t x16[8];
#pragma unroll
					for(int j = 0; j < 8; j++) x16[j] = __builtin_amdgcn_perm(pl[j][0], pl[j][NACC - 1], 0x07030501u);      // {plane of the low block, plane of the high block}
#pragma unroll
					for(int d = 0; d < 4; d++){
						cur[d] = __builtin_amdgcn_perm(x16[2 * d + 1], x16[2 * d], 0x05040100u);         // block jl
						cur[4 + d] = __builtin_amdgcn_perm(x16[2 * d + 1], x16[2 * d], 0x07060302u);     // block jl + L
					}
				}
			} else if constexpr (DO2){
				// one dword per reference block: M | R << 8 | two-bit fields << 16 (cell c at bits 15 - 2c, 14 - 2c of those)
#pragma unroll
				for(int n = 0; n < NACC; n++){
					const uint32_t t1 = __builtin_amdgcn_perm(accR[n], accM[n], 0x07030501u);               // {M.lo, R.lo, M.hi, R.hi}
					const uint32_t t2 = __builtin_amdgcn_perm(accDO[2 * n], accDO[2 * n + 1], 0x07030501u);  // {cells 4-7 .lo, cells 0-3 .lo, 4-7 .hi, 0-3 .hi}
					cur[n] = __builtin_amdgcn_perm(t2, t1, 0x05040100u) ^ 0x0000FFFFu;            // block NACC jl + n
					cur[NACC + n] = __builtin_amdgcn_perm(t2, t1, 0x07060302u) ^ 0x0000FFFFu;     // block NACC (jl + L) + n
				}
			} else if constexpr (WR == 8){
				// one dword per reference block: M | D << 8 | R << 16 | Od << 24, cell k at bit 7 - k
#pragma unroll
				for(int n = 0; n < NACC; n++){
					const uint32_t t1 = __builtin_amdgcn_perm(accD[n], accM[n], 0x07030501u);   // {M.lo, D.lo, M.hi, D.hi}
					const uint32_t t2 = __builtin_amdgcn_perm(accO[n], accR[n], 0x07030501u);
					cur[n] = __builtin_amdgcn_perm(t2, t1, 0x05040100u) ^ 0x00FFFFFFu;            // block NACC jl + n
					cur[NACC + n] = __builtin_amdgcn_perm(t2, t1, 0x07060302u) ^ 0x00FFFFFFu;     // block NACC (jl + L) + n
				}
			} else if constexpr (WR == 4 && W == 8){
				// four lanes per pair at bandwidth 64: a half holds two reference blocks of four cells, the first in bits 15..12 of the
				// accumulators, the second in bits 11..8; one dword per reference block: M | D << 4 | R << 8 | Od << 12
				const uint32_t pa = (((accM[0] >> 12) & 0x000F000Fu) | ((accD[0] >> 8) & 0x00F000F0u) | ((accR[0] >> 4) & 0x0F000F00u) | (accO[0] & 0xF000F000u)) ^ 0x0FFF0FFFu;
				const uint32_t pb = (((accM[0] >> 8) & 0x000F000Fu) | ((accD[0] >> 4) & 0x00F000F0u) | (accR[0] & 0x0F000F00u) | ((accO[0] << 4) & 0xF000F000u)) ^ 0x0FFF0FFFu;
				cur[0] = pa & 0xFFFFu; cur[1] = pb & 0xFFFFu; cur[2] = pa >> 16; cur[3] = pb >> 16;      // blocks 2 jl, 2 jl + 1, 2 (jl + L), 2 (jl + L) + 1
			} else if constexpr (WR == 4){
				const uint32_t pk = ((accM[0] >> 8) | (accD[0] >> 4) | accR[0] | (accO[0] << 4)) ^ 0x0FFF0FFFu;
				cur[0] = pk & 0xFFFFu; cur[1] = pk >> 16;
			} else {
				static_assert(WR == 16 || WR == 8 || WR == 4, "code row layouts");
				// 16 cells per block: dword 0 = M | D << 16, dword 1 = R | Od << 16, cell k at bit 15 - k
				const uint32_t xm = __builtin_amdgcn_perm(accM[0], accM[NACC - 1], 0x07030501u) ^ 0xFFFFFFFFu;   // {M16 of the low block, M16 of the high block}
				const uint32_t xd = __builtin_amdgcn_perm(accD[0], accD[NACC - 1], 0x07030501u) ^ 0xFFFFFFFFu;
				const uint32_t xr = __builtin_amdgcn_perm(accR[0], accR[NACC - 1], 0x07030501u) ^ 0xFFFFFFFFu;
				const uint32_t xo = __builtin_amdgcn_perm(accO[0], accO[NACC - 1], 0x07030501u);
				cur[0] = __builtin_amdgcn_perm(xd, xm, 0x05040100u); cur[1] = __builtin_amdgcn_perm(xo, xr, 0x05040100u);     // block jl
				cur[2] = __builtin_amdgcn_perm(xd, xm, 0x07060302u); cur[3] = __builtin_amdgcn_perm(xo, xr, 0x07060302u);     // block jl + L
			}
			const uint32_t ri = i & 3u;                       // (uniform over the wave: all pairs are at row i)
			if constexpr (CWD == 1){
				uint32_t *const sr = stg + 64u * ri;
#pragma unroll
				for(int q = 0; q < ND; q++) sr[256 * q] = cur[q];
			} else {
				uint32_t *const sr = stg + (64u * ND) * ri;
#pragma unroll
				for(int q = 0; q < ND; q++) sr[64 * q] = cur[q];
			}
			if(act && (ri == 3u || i + 1u == tlen)){
				uint32_t *gp = (uint32_t*)rowp + bsa_code_off(i & ~3u, 0u, CWD);       // block y of this group: gp[4 CWD y], rows then dwords
				if constexpr (CWD == 1){
#pragma unroll
					for(int q = 0; q < ND; q++){
						constexpr int RBH = (WR == 8) ? NACC : (WR == 4 && W == 8) ? 2 : 0;      // reference blocks (= code dwords) per half, where a half holds whole ones
						const uint32_t blk = RBH ? (uint32_t)(RBH * (jl + L * (q / RBH)) + q % RBH) : (uint32_t)(jl + L * q);
						uint4 t; t.x = stg[256 * q]; t.y = stg[256 * q + 64]; t.z = stg[256 * q + 128]; t.w = stg[256 * q + 192];
						*(uint4*)(gp + 4u * blk) = t;
					}
				} else {
					// a block's four rows of CWD dwords are contiguous (row r at dword r CWD): 16-byte pieces of two rows (CWD == 2) or one (CWD == 4);
					// a half holds RBH whole reference blocks, the lane's dwords of block (hf, n) are cur[CWD (RBH hf + n) ..]
					constexpr int RBH = (WR == 8) ? NACC : 1;
#pragma unroll
					for(int hb = 0; hb < 2 * RBH; hb++){
						const int hf = hb / RBH, n = hb % RBH;
						const uint32_t blk = (uint32_t)(RBH * (jl + L * hf) + n);
						uint32_t *bp = gp + (4u * CWD) * blk;
#pragma unroll
						for(int pc = 0; pc < CWD; pc++){           // piece pc: dwords 4 pc .. 4 pc + 3 of the block's 4 CWD
							uint4 t;
							uint32_t *tw = (uint32_t*)&t;
#pragma unroll
							for(int e = 0; e < 4; e++){
								const int lin = 4 * pc + e, row = lin / CWD, d = lin % CWD;
								tw[e] = stg[64 * (ND * row + CWD * hb + d)];
							}
							*(uint4*)(bp + 4 * pc) = t;
						}
					}
				}
			}
		}
		}          // (!SCORE)
		if(act){
			// band offsets: lane (i mod L) keeps the offset of row i, the group stores them together
			constexpr uint32_t LM = (uint32_t)(L - 1);
			const bool lastrow = i + 1u == tlen;
			// (four rows of offsets are 16 bytes at an odd dword, partial lines in memory; sixteen rows -- one 64-byte line -- leaving at a time through LDS were measured
			// at C2: WRITE_SIZE 80.0 -> 69.7 GB, forward 59.6 -> 60.2 ms: the partial lines cost traffic, not time)
			if constexpr (!SCORE){
			if((i & LM) == (uint32_t)jl) begq = (int)rbeg;
			if(((i & LM) == LM || lastrow) && (uint32_t)jl <= (i & LM)) begs[(i & ~LM) + 1u + (uint32_t)jl] = begq;
			}
			// H at band position pos of the new row: ubegs of its block + the block's u up to it (getscore, bsalign.h:3187-3197);
			// meaningful in the lane that owns the block
			auto score_at = [&](uint32_t pos) -> int {
				const uint32_t b = pos / W, kk = pos % W;
				const bool hi = b >= (uint32_t)L;
				int sc = HB + (hi ? x_hi16(Psh) : x_lo16(Psh)) + (int)b * W * GE;
#pragma unroll
				for(int k = 0; k < W; k++){
					const uint32_t uu = (k == 0) ? tmpU0 : U[STATIC ? k : k - 1];
					sc += ((uint32_t)k <= kk) ? ((hi ? x_hi8(uu) : x_lo8(uu)) + GE) : 0;
				}
				return sc;
			};
			if(mode != BSA_MODE_GLOBAL && rbeg + BW >= qlen){
				// overlap / extend: while the band touches the query end, H at query column qlen - 1 is a candidate end
				// (bsalign.h:4023-4032); the lane that owns that cell keeps the best one it has seen (strictly greater wins)
				const uint32_t pos = qlen - 1u - rbeg;
				if(((pos / W) & (uint32_t)(L - 1)) == (uint32_t)jl){
					const int sc = score_at(pos);
					if(sc > cand_sc){ cand_sc = sc; cand_te = (int)i; }
				}
			}
			if(lastrow && mode == BSA_MODE_GLOBAL){
				// global score = H at query column qlen - 1 of the last row (bsalign.h:4034-4037), kept in begs[tlen + 1]
				const uint32_t pos = qlen - 1u - rbeg;
				int *const gs = SCORE ? begs : begs + tlen + 1u;          // (SCORE: the record is the score)
				if(pos >= (uint32_t)BW){ if(first) *gs = (int)0x80000000u; }        // band never reached the query end
				else if(((pos / W) & (uint32_t)(L - 1)) == (uint32_t)jl) *gs = score_at(pos);
			} else if(lastrow){
				// end record (bsa_common.h bsa_code_end_t): the candidates and the last row itself, per reference block, in natural
				// band order (row_max is taken by the traceback kernel)
				bsa_code_end_t *er = SCORE ? (bsa_code_end_t*)begs : (bsa_code_end_t*)(rowp + (size_t)bsa_code_rows(tlen) * (64u * CWD));
#pragma unroll
				for(int q = 0; q < 16 / L; q++){ er->cand_sc[jl + L * q] = q ? BSA_SCORE_MIN : cand_sc; er->cand_te[jl + L * q] = q ? 0 : cand_te; }
				int8_t *ub = (int8_t*)(er + 1);
#pragma unroll
				for(int hf = 0; hf < 2; hf++){
					const int b = jl + L * hf;
					er->ubegs[b * CR] = HB + (hf ? x_hi16(Psh) : x_lo16(Psh)) + b * W * GE;
					if constexpr (CR == 2) er->ubegs[b * CR + 1] = HB + (hf ? x_hi16(PM) : x_lo16(PM)) + (b * W + W / 2) * GE;
#pragma unroll
					for(int k = 0; k < W; k++){
						const uint32_t uu = (k == 0) ? tmpU0 : U[STATIC ? k : k - 1];
						ub[b * W + k] = (int8_t)((hf ? x_hi8(uu) : x_lo8(uu)) + GE);
					}
				}
				if(last){ er->ubegs[16] = HB + x_hi16(PN) + BW * GE; er->rbeg_last = (int)rbeg; }
			}
		}
		// ---- adaptive band (bsalign.h:3331-3349) + global steering (bsalign.h:4006-4021)
		if constexpr (!STATIC){
			uint32_t x;
			{
				if constexpr (CR == 1){
					const uint32_t dl = x_add(x_sub(PN, Psh), WGE16);         // ubegs[b+1] - ubegs[b]
					x = x_max(dl, x_sub(0u, dl));
				} else {
					const uint32_t HGE16 = x_i16((W / 2) * GE);
					const uint32_t da = x_add(x_sub(PM, Psh), HGE16), db = x_add(x_sub(PN, PM), HGE16);     // the two reference blocks of this block
					x = x_add(x_max(da, x_sub(0u, da)), x_max(db, x_sub(0u, db)));
				}
				x = x_sum<L>(x);
			}
			const int nzsum = (int)((x & 0xffffu) + (x >> 16));
			const int d16 = x_hi16(x_bcast_last<L>(PN)) + BW * GE;             // ubegs[16] - ubegs[0]
			uint32_t nz = (uint32_t)(nzsum / 16);
			nz = nz / (uint32_t)WR * 16u / 2u;
			const int noisy = (int)((16u > nz) ? 16u : nz);
			int rbx;
			if(i <= (uint32_t)BW / 4u) rbx = 0;
			else if(rbeg + BW >= qlen) rbx = 0;
			else if(noisy < d16) rbx = 2;
			else if(d16 < -noisy) rbx = 0;
			else rbx = 1;
			if(mode == BSA_MODE_GLOBAL){
				const int rby = __builtin_amdgcn_ds_bpermute(rby_lane + (int)((i & (uint32_t)(L - 1)) << 2), rby_tab);
				const uint32_t left = tlen - i - 1u;
				bool rush;
				if(rush32) rush = act && rbeg + rzl + (uint32_t)BW <= qlen + (uint32_t)rbz - 1u;
				else {
					const unsigned long long lhs = (unsigned long long)rbeg + (unsigned long long)(uint32_t)rbz * left + (unsigned long long)BW;
					rush = act && lhs <= (unsigned long long)(uint32_t)(qlen + (uint32_t)rbz - 1u);
				}
				if((int)rbeg < rby - BW) mov = (uint32_t)(rbx + 1);
				else if((int)rbeg > rby) mov = (uint32_t)max(0, rbx - 1);
				else mov = (uint32_t)rbx;
				if(rush) mov = 1u + (uint32_t)(qlen - (rbeg + BW)) / max(left, 1u);
			} else mov = (uint32_t)rbx;
		}
		if constexpr (STATIC){ U[0] = tmpU0; NE[0] = tmpNE0; if constexpr (PW == 2) NQ2[0] = tmpNQ0; }
		// ---- speculative slide by one cell: the first cell of every block becomes the last cell of the block before it
		else {
			uint32_t inu;
			if constexpr (L == 4) inu = x_shift_up<L>(tmpU0, NEWU0, last);
			else {
				const uint32_t nxt = XDPPZ(tmpU0, XROW_SHL(1), 0xf);          // (a DPP move must not sit in an arm of ?: -- only one arm runs)
				inu = last ? __builtin_amdgcn_alignbit(NEWU0, bc0, 16) : nxt;
			}
			const uint32_t inne = x_shift_up<L>(tmpNE0, NEWNE, last);
			U[W - 1] = inu; NE[W - 1] = inne;
			if constexpr (PW == 2){ NQ2[W - 1] = x_shift_up<L>(tmpNQ0, NEWNE, last); svNQ = tmpNQ0; }
			PN = x_add(x_add(PN, x_ashr8(inu)), GE16);
			if constexpr (CR == 2) PM = x_add(x_add(PM, x_ashr8(U[W / 2 - 1])), GE16);
			svU = tmpU0; svNE = tmpNE0;
		}
		i++;
		rzl -= (uint32_t)rbz;          // (meaningless once the pair has no row left: only read under `act`)
		// (the next eight target bases.  The compiler waits for them at the top of the next row, with `s_waitcnt vmcnt(0)` on every row; forcing the wait
		// into this branch instead -- once per eight rows, fully exposed -- was measured slower: 60.0 against 59.8 ms, two-piece gaps 129.8 against 127.1)
		if((i & 7u) == 0u && i < tlen){ __builtin_memcpy(&twin, tp + i, 8); twin <<= 2; }
	}
	if(st != nullptr && row1 < tlen){
		// write-through stores (sc1): the next segment usually runs on another CU, often on another XCD, and a release fence here
		// would write back every dirty line of this XCD's L2 -- the half-filled lines of the code rows of 400 waves -- once per item
		uint32_t *sp = st + (lt & 63);
		int r = 0;
		auto put = [&](uint32_t v){ __hip_atomic_store(sp + 64 * r, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); r++; };
#pragma unroll
		for(int k = 0; k < W; k++) put(U[k]);
#pragma unroll
		for(int k = 0; k < W; k++) put(NE[k]);
		if constexpr (PW == 2){
#pragma unroll
			for(int k = 0; k < W; k++) put(NQ2[k]);
		}
		put(PN); put(PM); put((uint32_t)HB); put(svU); put(svNE); put(svNQ);
		put(rbeg); put(mov); put((uint32_t)cand_sc); put((uint32_t)cand_te);
	}
}

// ABSOLUTE-SCORE form of the row body (one-piece gaps, sixteen cells a half, four lanes per pair, moving band, two-bit D / Od fields: the
// headline shape).  Same code rows, band offsets, scores and end records as x_forward, bit for bit.
// The row is kept as scores, not as differences: H^(x, y) = H(x, y) - gape (x + y) - base, x the query column, y the target row, base an int32
// of the pair.  In this frame extending a gap costs nothing in either direction, a cell's value does not depend on where the band stands, and the
// recurrence needs no re-basing from cell to cell:
//     pass 1:  d = Hp + S~     m = max(E, d)     mg = m + gapo     f = max(f, mg)
//     pass 2:  h = max(m, f)   fm = max(f, mg)   f = fm            En = max(E, h + gapo)
// with Hp[k] = H^ of the new cell k's diagonal predecessor and E[k] = its E^ (the upper neighbour's H^ + e - gape); both are plain int16 in the
// two halves.  Every comparison is x_forward's with the diagonal predecessor's score added on both sides, so the four facts of a cell are the same
// bits: M: h == d, D / Od field: h - En = min(h - E, -gapo), R: fm == mg.
// The row is held slid by one cell as in x_forward: cell k writes h into Hp[k] (its own slot: the new cell k's diagonal predecessor is the old
// cell k) and En into E[k - 1]; cell 0's En travels to the previous block's E[W - 1].  Nothing of Hp crosses a lane on a row that moves by one.
//   * the cell entering at the band end has H^ = (last cell) + cfirst - gape, E^ = that - gape (e = 0); the cells behind it (moves of two and
//     more) repeat both values (u = gape1);
//   * the virtual column left of the band's first cell (ubegs[0], re-based on cell 0 with u = 0 by the reference's tail) is (cell 0) + gape;
//   * the -63 sentinels (f entering every block in pass 1 and block 0 in pass 2, e of row -1, the first-cell rule) keep their exact values,
//     added to the score they were relative to; a band that jumps past all it held starts again from a row of SCORE_MIN;
//   * real scores are read where they are needed: H at band position p of row i = base + H^ + gape (rbeg + p + i).
// F values are absolute, so the F-penetration is the bare prefix maximum over the pair's lanes.
// S~ comes sign-extended out of ONE byte permute: the row's table entry is two dwords {PADS, S~(q0), 0, S~(q1)}, {0, S~(q2), 0, S~(q3)} and the
// window's selector of a column is {byte of its code, sign of that byte} per half (selectors 8 .. 11 replicate the top bit of bytes 1, 3, 5, 7);
// code 4 (beyond the query end) selects the PADS byte and the constant 0xFF: a fifth entry at no cost, queries shorter than the band included.
// REBASE: every (rmask + 1) rows the H^ of lane 0's first slot is subtracted from Hp and E and added to base (bsa_align8_abs_rows has the bound).
// FLAGS.  M, R (and D, Od of the four planes) are one bit a cell, accumulated as they are stored (not inverted), eight cells to an accumulator per half: cell k & 7 == 0
// in bit 15, so they fill the HIGH byte of a half in the code row's byte order.  A flag is "two scores are equal" where the difference a - b is known to lie in 0 .. 256
// (bsa_align8_flag_span derives it for every scoring of the guard), so of n = b - a bits 8 .. 15 are all clear (equal) or all set: two instructions a cell, the packed
// difference and one v_bitop3_b32 that puts the cell's bit of ~n into the accumulator (x_ins; the saturating form it replaces took three, the last a v_pk_mad_u16):
//     M: n = d - h     R: n = hg - fm     D: n = E - h     Od: n = hg - en   (= (h - en) + gapo: zero exactly where the field h - en equals -gapo)
// Cell 0 alone keeps the saturating comparison for M, in the waves that take the first-cell rule (the fix-up behind pass 2 says why).  The two-bit D / Od fields are a Horner multiply-add (x_acc) and fill the low byte.
// PW: 1 one-piece gaps, 0 linear gaps (gapo = 0: E^ of a cell is its upper neighbour's H^, R and Od are always set).  DO2: the two-bit D / Od fields (four lanes, one piece);
// otherwise the four planes, with D (h == E) and Od (field == -gapo) accumulated as they are stored too.  L = 8: bandwidth 256, a half is one reference block of sixteen cells.
// EXT: the staging area and the window come from the caller (k_align8_fwd_x_mix).
// M3: THREE-OPERAND MAXIMA in a BIASED FRAME.  m and mg are never formed:
//     pass 1:  d = Hp + S~     t = max3(t, E, d)                      (t enters as fini - gapo, F leaving the block is t + gapo:
//                                                                      max(fini, max_k (max(E_k, d_k) + gapo)) with the addition taken out of the maximum)
//     pass 2:  h = max3(E, d, f)   hg = h + gapo   fm = max(f, hg)   En = max(E, hg)
// fm is what it was: max(f, hg) = max(f, m + gapo, f + gapo) = max(f, mg) because gapo <= 0.  R is fm == hg: where f <= m that is the same comparison (h = m), and where
// f > m both are false for gapo < 0 (hg = f + gapo < f = fm, and mg < f = fm), which one-piece gaps always have (bsa_align8_x_supported).  Linear gaps: fm = En = h.
// max3 is the f16 instruction (x_max3), so every operand of it -- Hp / d, E, f, the sentinels -- must be an int16 in 0x0400 .. 0x7BFF.  The frame therefore sits at B = 0x4000
// instead of 0: a rebase makes lane 0's first slot B, not 0, and whatever writes absolute H^ / E^ values (row -1, the row a jumping band starts from) adds B, with -B folded
// into base, so that H = base + H^ + gape (x + y) holds wherever it is read.  Everything else is relative to a value of the row and needs nothing.  bsa_align8_abs_rows
// has the bound that keeps the values inside B +- 15359.  Only the maxima are f16: every addition and subtraction stays packed integer, and so do the F scan (its
// 0x8000 filler is no score; what leaves the scan is one) and the maxima of fm and En.  Lanes of dead pairs (tlen = 0) and of rows past a short target carry arbitrary
// patterns, NaNs included, through the maxima: nothing they compute is stored, and nothing crosses from one pair's lanes into another's.
// M3 = false keeps the integer recurrence above in the frame at 0, for the scorings whose bound does not fit the biased frame (bandwidth 256 only: bsa_align8_abs_rows).
// ROWS THAT DO NOT MOVE BY ONE CELL are paid for by the whole wave, so their fix-ups have a constant form for the common cases (a move of two: one mask per flag in
// the pair's last lane; a row that stays at rbeg > 0: the first cell's predecessor is fini's low half) and keep the general code for the wave that needs it.
// Their slot shifts run in the lanes that need them, two slots an instruction (x_slots_up, x_slots_down).
// ROW TARGET: {k, r} of (i + jl) qlen = k tlen + r, stepped every L rows (x_rt_double has the proof that k is what the reference's double expression gives where r != 0).
template<int L, int NWV, int PW = 1, bool DO2 = true, bool EXT = false, bool M3 = true>
static __device__ __forceinline__ void x_forward_abs(const Align8Args &a, const uint32_t first_pos, const uint32_t count, const uint32_t tid_base, const uint32_t rmask,
		const uint32_t row0 = 0u, const uint32_t row1 = 0xFFFFFFF8u, uint32_t *st = nullptr, uint32_t *ext_stage = nullptr, uint32_t *ext_qwin = nullptr){
	constexpr int W = 16, BW = 2 * L * W, WR = BW / 16, CR = 8 / L;
	static_assert((L == 4 || L == 8) && (PW == 0 || PW == 1) && (!DO2 || (PW == 1 && L == 4)), "bandwidth 128 (four lanes per pair) or 256 (eight), one-piece or linear gaps");
	constexpr int NACC = 2, NDO = DO2 ? 4 : 1, ND = 4, CWD = WR / 8;
	const int lt = threadIdx.x;
	const int jl = lt & (L - 1);
	const bool first = jl == 0, last = jl == L - 1;
	const uint32_t g = (tid_base + (uint32_t)lt) / (uint32_t)L;
	const bool live = g < count;
	const uint32_t ppos = first_pos + (live ? g : 0u);
	const uint32_t pair = a.order[ppos];
	const uint32_t qlen = a.qlen[pair];
	uint32_t tlen = a.tlen[pair];
	const uint8_t *qp = a.qst + a.qpoff[pair], *tp = a.tst + a.tpoff[pair];
	int *begs = (int*)(a.rows + a.slot_off[ppos]);
	uint8_t *rowp = (uint8_t*)begs + bsa_begs_bytes(tlen);
	if(!live || a.status[pair] != 0u) tlen = 0;

	const int mode = a.mode & 3;
	const int gapo1 = a.gapo1, gape1 = a.gape1;
	const int GE = gape1, GO = gapo1;
	const uint32_t GO16 = x_i16(GO), GE16 = x_i16(GE);
	const uint32_t ONE1 = 0x00010001u;
	uint32_t FOUR = 0x00040004u;
	asm volatile("" : "+s"(FOUR));                         // opaque multiplier of x_acc (the two-bit fields)
	const uint32_t DOSP = (GO == -1) ? 2u : 1u;
	const uint32_t MINF16 = x_i16(BSA_EPI8_MIN - 2 * GE);
	const int gopen = gapo1 + gape1;
	const int cfirst = min(a.smin, gopen) - 1 - a.smax + gopen;
	const uint32_t ENT16 = x_i16(cfirst - GE);             // the entering cell's H^ above the last cell's
	const int NEWNE = (PW == 0) ? 0 : GE;                  // gape - e of an entering cell (e = 0; linear gaps: e is the constant gape)
	const int NE0 = (PW == 0) ? 0 : GE - BSA_EPI8_MIN;     // ... of row -1 (e = -63)
	static_assert(M3 || L == 8, "no scoring inside bsa_align8_x_supported leaves the biased frame at bandwidth 128 (bsa_align8_abs_rows)");
	constexpr int FB = M3 ? 0x4000 : 0;                    // where the frame sits: H^ of lane 0's first slot after a rebase
	__shared__ __attribute__((aligned(8))) uint32_t xa_mtab[8];
	if((lt & 63) < 4){
		const int t = lt & 3;
		auto sb = [&](int q) -> uint32_t { return (uint32_t)(((int)a.matrix[q * 4 + t] - 2 * GE) & 0xff); };
		xa_mtab[2 * t] = (uint32_t)((BSA_EPI8_MIN - 2 * GE) & 0xff) | (sb(0) << 8) | (sb(1) << 24);
		xa_mtab[2 * t + 1] = (sb(2) << 8) | (sb(3) << 24);
	}
	__builtin_amdgcn_wave_barrier();

	uint32_t Hp[W], E[W];
	int base = 0;
	uint32_t svH = 0, svE = 0;        // lane 0, low half: H^ of the virtual column left of the row's first cell and E^ of that cell, for a row that does not move
	uint32_t rbeg = 0, mov = 0, i = row0;
	int cand_sc = BSA_SCORE_MIN, cand_te = 0;
	// this lane's band positions times -gape, per half
	const uint32_t NGP = ((uint32_t)(-GE * jl * W) & 0xffffu) | ((uint32_t)(-GE * (jl + L) * W) << 16);
	if(row0 == 0u){
		// row -1 (bsalign.h:2094-2140), slid by one cell: Hp[k] = H^ at band position p, E[k] = E^ at p + 1 (e = -63)
		const int first_u = (int)(int8_t)(gapo1 + gape1 + a.smin - a.smax);
		const bool ov = mode == BSA_MODE_OVERLAP;
		base = (ov ? 0 : gapo1 + 2 * gape1) - FB;
#pragma unroll
		for(int k = 0; k < W; k++){
			// global / extend: H(p, -1) = gapo + (p + 1) gape: H^ = 0; overlap: H = 0: H^ = -gape (p - 1); both above FB
			Hp[k] = ov ? x_add(NGP, x_i16(FB + GE - GE * k)) : x_i16(FB);
			E[k] = ov ? x_add(NGP, x_i16(FB - GE * k - NE0)) : x_i16(FB - NE0);
		}
		// the entering cell behind the row's last one
		if(last){
			const uint32_t hl = (Hp[W - 1] >> 16) + (uint32_t)(cfirst - GE - NEWNE);
			E[W - 1] = (E[W - 1] & 0xffffu) | (hl << 16);
		}
		svH = ov ? x_i16(FB + 2 * GE) : x_i16(FB + GE - first_u);
		svE = ov ? x_i16(FB + GE - NE0) : x_i16(FB - NE0);
	}
	if(row0 != 0u){
		const uint32_t *sp = st + (lt & 63);
		int r = 0;
#pragma unroll
		for(int k = 0; k < W; k++) Hp[k] = sp[64 * r++];
#pragma unroll
		for(int k = 0; k < W; k++) E[k] = sp[64 * r++];
		base = (int)sp[64 * r++]; svH = sp[64 * r++]; svE = sp[64 * r++];
		rbeg = sp[64 * r++]; mov = sp[64 * r++]; cand_sc = (int)sp[64 * r++]; cand_te = (int)sp[64 * r++];
	}
	__shared__ uint32_t xa_stage[EXT ? 1 : NWV][EXT ? 1 : 4 * ND][64];
	uint32_t *const stg = EXT ? ext_stage + (size_t)(lt >> 6) * (4 * ND * 64) + (lt & 63) : &xa_stage[(!EXT && NWV > 1) ? (lt >> 6) : 0][0][lt & 63];
	constexpr int KD = 4 + 12, NSEL = 2 * KD;
	constexpr uint32_t QOFFMAX = (uint32_t)(NSEL - W);
	static_assert(NSEL % 4 == 0 && NSEL - W <= BSA_QPAD_TAIL, "a refill reads NSEL - W bytes behind the band's last block");
	__shared__ uint32_t xa_qwin[EXT ? 1 : NWV][EXT ? 1 : 2 * KD][64];
	uint32_t *const qwp = EXT ? ext_qwin + (size_t)(lt >> 6) * (2 * KD * 64) + (lt & 63) : &xa_qwin[(!EXT && NWV > 1) ? (lt >> 6) : 0][0][lt & 63];
	uint32_t wbase = 0x40000000u;
	int begq = 0;
	if(tlen != 0u && first && row0 == 0u) begs[0] = 0;
	uint64_t twin = 0;          // eight target bases times eight: the byte offsets of their table entries
	if(row0 < tlen){ __builtin_memcpy(&twin, tp + row0, 8); twin <<= 3; }
	const int rbz = 2 * max((int)(tlen / max(qlen, 1u)), 1);
	const bool rush32 = (unsigned long long)(uint32_t)rbz * tlen + qlen + (uint32_t)BW + (uint32_t)rbz < 0xFFFFFFFFull;
	uint32_t rzl = rush32 ? (uint32_t)rbz * (tlen - min(row0, tlen) - 1u) : 0u;
	// the row target of row i + jl, renewed every L rows: held one step behind the segment's first row, the loop steps before it reads (row0 is a multiple of L)
	XRowTgt rt = {0u, 0u}, rtd = {0u, 0u};
	if(mode == BSA_MODE_GLOBAL){
		rt = x_rt_at(row0 + (uint32_t)jl, tlen, qlen);
		rtd = x_rt_at((uint32_t)L, tlen, qlen);
		x_rt_back(rt, rtd, tlen);
	}
	const uint64_t rtwide = __builtin_amdgcn_ballot_w64(x_rt_wide(tlen, qlen));          // lanes of the pairs outside the proof's bound: the double expression on every renewal
	const int rby_lane = (lt & (64 - L)) << 2;

	uint64_t actm = 0;
	while(i < row1 && (actm = __builtin_amdgcn_ballot_w64(i < tlen)) != 0ull){
		const bool act = i < tlen;
		if(mode == BSA_MODE_GLOBAL && (i & (uint32_t)(L - 1)) == 0u){
			// the row target of row i + jl in integers (x_rt_double has the proof); a wave with a live row whose product divides evenly, or with a live pair outside the
			// proof's bound, asks the double expression
			x_rt_step(rt, rtd, tlen);
			// (one compare a ballot, joined on the scalar unit: the ballot of a conjunction is made 0 / 1 in a register and compared again)
			if(__builtin_expect(((__builtin_amdgcn_ballot_w64(rt.r == 0u) & __builtin_amdgcn_ballot_w64(i + (uint32_t)jl < tlen)) | (rtwide & actm)) != 0ull, 0)){
				const uint32_t y = (uint32_t)x_rt_double(i + (uint32_t)jl, tlen, qlen);
				x_rt_set(rt, y, tlen);
			}
		}
		// ---- rebase (i is uniform)
		if((i & rmask) == 0u){
			const uint32_t bc = x_bcast_first<L>(Hp[0]);
			const uint32_t dl = x_sub(__builtin_amdgcn_perm(bc, bc, 0x01000100u), x_i16(FB));          // the slot becomes FB
#pragma unroll
			for(int k = 0; k < W; k++){ Hp[k] = x_sub(Hp[k], dl); E[k] = x_sub(E[k], dl); }
			svH = x_sub(svH, dl); svE = x_sub(svE, dl);
			base += x_lo16(bc) - FB;
		}
		mov = min(mov, __builtin_elementwise_sub_sat(qlen, rbeg + (uint32_t)BW));
		rbeg += mov;
		int rhj = 0;
		// ---- row_movx: correct what did not move by one
		if(__builtin_expect((__builtin_amdgcn_ballot_w64(mov != 1u) & actm) != 0ull, 0)){
			if(__any(act && mov >= (uint32_t)BW)){
				const bool z = act && mov >= (uint32_t)BW;
				const uint32_t bc = x_bcast_last<L>(Hp[W - 1]);
				// H at the last cell of the previous row (band offset rbeg - mov, row i - 1)
				const int rhz = base + x_hi16(bc) + GE * ((int)(rbeg - mov) + BW - 1 + (int)i - 1);
				if(z){
					rhj = rhz;
					// a row of SCORE_MIN with e = 0: base such that the diagonal predecessor of band position 0 has H^ = FB
					base = BSA_SCORE_MIN - GE * ((int)rbeg + (int)i - 2) - FB;
#pragma unroll
					for(int k = 0; k < W; k++){ Hp[k] = x_add(NGP, x_i16(FB - GE * k)); E[k] = x_add(NGP, x_i16(FB - GE * (k + 1) - NEWNE)); }
				}
			}
			if(__any(act && mov == 0u)){
				const bool d = act && mov == 0u;
				const uint32_t pu = x_shift_down<L>(Hp[W - 1], svH, first), pe = x_shift_down<L>(E[W - 1], svE, first);
				if(d){ x_slots_up<W>(Hp, pu); x_slots_up<W>(E, pe); }
			}
			for(uint32_t s = 1; __any(act && mov < (uint32_t)BW && s < mov); s++){
				const bool d = act && mov < (uint32_t)BW && s < mov;
				// the cells behind the band end: the first has H^ = last + cfirst - gape, the others repeat it; E^ of all of them is what the slide put in
				uint32_t hfill = __builtin_amdgcn_perm(Hp[W - 1], Hp[W - 1], 0x03020302u);
				if(s == 1u) hfill = x_add(hfill, ENT16);
				const uint32_t efill = __builtin_amdgcn_perm(E[W - 1], E[W - 1], 0x03020302u);
				const uint32_t inh = x_shift_up<L>(Hp[0], hfill, last), ine = x_shift_up<L>(E[0], efill, last);
				if(d){ x_slots_down<W>(Hp, inh); x_slots_down<W>(E, ine); }
			}
		}
		// ---- S~(x, y), sign-extended
		uint32_t S[W];
		{
			const uint32_t tw32 = (i & 4u) ? (uint32_t)(twin >> 32) : (uint32_t)twin;
			const uint32_t tb8 = __builtin_amdgcn_ubfe(tw32, 8u * (i & 3u), 5u);
			uint32_t off = rbeg - wbase;
			if(__builtin_expect((__builtin_amdgcn_ballot_w64(off > QOFFMAX) & actm) != 0ull, 0)){
				// refill for every live pair of the wave (x_forward, "refill"); a column's selector is {value byte, sign selector} of its two codes:
				// code c < 4: bytes 2c + 1 and 8 + c, code 4: byte 0 (PADS) and 0x0D (0xFF)
				if(act){
					const uint8_t *pl = qp + rbeg + jl * W, *ph = qp + rbeg + (jl + L) * W;
					uint32_t bl[NSEL / 4], bh[NSEL / 4];
					__builtin_memcpy(bl, pl, NSEL); __builtin_memcpy(bh, ph, NSEL);
					uint32_t TV = 0x07050301u, TS = 0x0B0A0908u;
					asm volatile("" : "+v"(TV), "+v"(TS));
#pragma unroll
					for(int n = 0; n < NSEL / 4; n++){
						const uint32_t lv = __builtin_amdgcn_perm(0x00000000u, TV, bl[n]), ls = __builtin_amdgcn_perm(0x0000000Du, TS, bl[n]);
						const uint32_t hv = __builtin_amdgcn_perm(0x00000000u, TV, bh[n]), hs = __builtin_amdgcn_perm(0x0000000Du, TS, bh[n]);
						const uint32_t l01 = __builtin_amdgcn_perm(ls, lv, 0x05010400u), l23 = __builtin_amdgcn_perm(ls, lv, 0x07030602u);
						const uint32_t h01 = __builtin_amdgcn_perm(hs, hv, 0x05010400u), h23 = __builtin_amdgcn_perm(hs, hv, 0x07030602u);
						qwp[64 * (4 * n)] = __builtin_amdgcn_perm(h01, l01, 0x05040100u);
						qwp[64 * (4 * n + 1)] = __builtin_amdgcn_perm(h01, l01, 0x07060302u);
						qwp[64 * (4 * n + 2)] = __builtin_amdgcn_perm(h23, l23, 0x05040100u);
						qwp[64 * (4 * n + 3)] = __builtin_amdgcn_perm(h23, l23, 0x07060302u);
					}
					wbase = rbeg; off = 0u;
				}
			}
			const uint32_t *wl = qwp + 64u * (act ? off : 0u);
			const uint2 mr = *(const uint2*)((const uint8_t*)xa_mtab + tb8);
#pragma unroll
			for(int k = 0; k < W; k++) S[k] = __builtin_amdgcn_perm(mr.y, mr.x, wl[64 * k]);
		}
		// ---- first cell of the band (bsalign.h:2899-2907), x_forward's rule with the scores made real: ubegs[0] = base + Hp[0] + gape (rbeg + i - 2)
		const uint32_t d0s = x_add(Hp[0], S[0]);
		uint32_t d0h = d0s;
		// q0m and q0d are read by the fix-up of rbeg = 0 alone (behind pass 2), and every live row at rbeg = 0 sets them below: they start without a value, at no instruction
		// (q0s likewise: d0s of a row that takes the first-cell rule, read by the fix-up of cell 0's M flag behind pass 2)
		uint32_t q0m, q0d, q0s;
		asm volatile("" : "=v"(q0m), "=v"(q0d), "=v"(q0s));
		const uint32_t fini = x_add(Hp[0], MINF16);
		// (a row that stays, mov = 0, or whose band jumped; rbeg = 0 implies mov = 0 on that row, rbeg being the sum of the moves, so every live row at rbeg = 0 comes here)
		// (the live lanes of such rows, kept as a scalar mask: the only rows on which d0h can differ from d0s, which the fix-ups behind pass 2 ask again)
		const uint64_t fcm = __builtin_amdgcn_ballot_w64(mov - 1u >= (uint32_t)BW - 1u) & actm;
		if(__builtin_expect(fcm != 0ull, 0)){
			q0s = d0s;
			const int hp0 = x_lo16(Hp[0]);
			const int HBr = base + hp0 + GE * ((int)rbeg + (int)i - 2);
			// A ROW THAT STAYS AT rbeg > 0 has rh = SCORE_MIN, and then hh = (SCORE_MIN - HBr) + s0 with s0 <= 127 (a matrix entry or the pad score) while
			// t0 = lo16(E[0]) - lo16(Hp[0]) + 2 gape > -2^17 (two int16 and |gape| <= 127).  So HBr > SCORE_MIN + 2^17 proves hh < t0 for the lane: hh becomes EPI8_MIN and
			// the low half of d0h is Hp[0] + (EPI8_MIN - 2 gape), which is fini's.  The test is per lane and is the proof: a band that jumped has rebuilt base from
			// SCORE_MIN, HBr is then near SCORE_MIN, the comparison can go either way, and such a lane takes the rule below as it stands.  A wave takes the rule whenever
			// one of its live rows needs it: a jump, a row at rbeg = 0, a row that fails the test.
			const bool near = mov == 0u && rbeg != 0u && HBr > BSA_SCORE_MIN + (1 << 17);
			if((__builtin_amdgcn_ballot_w64(mov - 1u >= (uint32_t)BW - 1u && !near) & actm) == 0ull){
				if(first && mov == 0u) d0h = (d0s & 0xffff0000u) | (fini & 0xffffu);
			} else {
				int rh;
				if(mov >= (uint32_t)BW) rh = rhj;
				else if(rbeg) rh = BSA_SCORE_MIN;
				else if(mode == BSA_MODE_OVERLAP || i == 0) rh = 0;
				else rh = gapo1 + gape1 * (int)i;
				const int s0 = x_lo16(S[0]) + 2 * GE;
				const int t0 = x_lo16(E[0]) - hp0 + 2 * GE;          // u + e
				int hh = (rh - HBr) + s0;
				hh = (hh >= t0) ? min(hh, BSA_EPI8_MAX) : BSA_EPI8_MIN;
				if(first && (mov == 0u || mov >= (uint32_t)BW)) d0h = (d0s & 0xffff0000u) | ((uint32_t)(hp0 + hh - 2 * GE) & 0xffffu);
				// a wave whose rows all stay at rbeg > 0 does not form q0m and q0d
				if((__builtin_amdgcn_ballot_w64(rbeg == 0u) & actm) != 0ull){
					const int cm = rh - HBr + s0 - 2 * GE, cd = t0 + rh - HBr - 2 * GE;
					q0m = (cm >= -128 && cm <= 127) ? ((uint32_t)(hp0 + cm) & 0xffffu) : 0x10000u;          // (0x10000: never equal to a half)
					q0d = (cd >= -128 && cd <= 127) ? ((uint32_t)(hp0 + cd) & 0xffffu) : 0x10000u;
				}
			}
		}
		// ---- pass 1: F leaving every block when nothing but the sentinel enters it
		uint32_t d[W], m[M3 ? 1 : W], mg[M3 ? 1 : W];
		uint32_t f = fini;
		if constexpr (M3){
			// (the opening is added once, behind the sixteen maxima)
			if constexpr (PW != 0) f = x_sub(f, GO16);
#pragma unroll
			for(int k = 0; k < W; k++){
				d[k] = (k == 0) ? d0s : x_add(Hp[k], S[k]);
				f = x_max3(f, E[k], (k == 0) ? d0h : d[k]);
			}
			if constexpr (PW != 0) f = x_add(f, GO16);
		} else {
#pragma unroll
		for(int k = 0; k < W; k++){
			d[k] = (k == 0) ? d0s : x_add(Hp[k], S[k]);
			m[k] = x_max(E[k], (k == 0) ? d0h : d[k]);
			mg[k] = (PW == 0) ? m[k] : x_add(m[k], GO16);
			f = x_max(f, mg[k]);
		}
		}
		// ---- F-penetration: prefix maximum over the blocks
		{
			const uint32_t P = x_scan_max<L>(f);
			const uint32_t bc = x_bcast_last<L>(P);
			const uint32_t Gm = x_max(P, (bc << 16) | 0x8000u);
			f = x_shift_down<L>(Gm, fini, first);
		}
		// ---- pass 2, flags
		uint32_t accM[NACC], accR[NACC], accD[NACC], accO[NACC], accDO[NDO];
#pragma unroll
		for(int n = 0; n < NDO; n++) accDO[n] = 0;
#pragma unroll
		for(int n = 0; n < NACC; n++){ accM[n] = 0; accR[n] = 0; accD[n] = 0; accO[n] = 0; }
		uint32_t tmpE0 = 0, hfirst = 0;
#pragma unroll
		for(int k = 0; k < W; k++){
			const uint32_t BIT = 0x80008000u >> (k & 7);
			auto ins = [&](uint32_t acc, uint32_t n) -> uint32_t { return (k & 7) == 0 ? x_ins0(n, BIT) : x_ins(acc, n, BIT); };
			uint32_t h, en, hg = 0;
			if constexpr (M3){
				h = x_max3(E[k], (k == 0) ? d0h : d[k], f);
				if constexpr (PW != 0){
					hg = x_add(h, GO16);
					const uint32_t fm = x_max(f, hg);
					accR[k >> 3] = ins(accR[k >> 3], x_sub(hg, fm));
					f = fm;
					en = x_max(E[k], hg);
				} else { f = h; en = h; }
			} else {
			h = x_max(m[k], f);
			const uint32_t fm = x_max(f, mg[k]);
			f = fm;
			if constexpr (PW != 0){
				// R as fm == hg here too (the comment above: max(f, mg) = max(f, hg), and the two comparisons agree); fm - mg has no bound where f > m
				hg = x_add(h, GO16);
				accR[k >> 3] = ins(accR[k >> 3], x_sub(hg, fm));
				en = x_max(E[k], hg);
			} else en = h;          // (gapo = 0: h >= E)
			}
			if constexpr (DO2){
				const uint32_t fld = x_sub(h, en);
				// four fields a byte, the first on top: fld0 * 64 + fld1 * 16 + fld2 * 4 + fld3 by Horner, three multiply-adds by construction
				if((k & 3) == 0) accDO[k >> 2] = fld;
				else accDO[k >> 2] = x_acc(accDO[k >> 2], fld, FOUR);
			} else {
				accD[k >> 3] = ins(accD[k >> 3], x_sub(E[k], h));
				// field == -gapo: hg - en = (h - en) + gapo, in gapo .. 0 because hg <= en <= h
				if constexpr (PW != 0) accO[k >> 3] = ins(accO[k >> 3], x_sub(hg, en));
			}
			// (cell 0's flag is right wherever d0h is d0s, i.e. in every wave that did not take the first-cell rule: the fix-up behind the loop has the others)
			accM[k >> 3] = ins(accM[k >> 3], x_sub(d[k], h));
			Hp[k] = h;
			if(k == 0){ tmpE0 = en; hfirst = h; }
			else E[k - 1] = en;
		}
		// ---- flags of special cells (x_forward's, on accumulators that are not inverted; the one-bit flags sit in the HIGH byte of a half, cell 0 of eight in
		// bit 15, the two-bit fields in the low byte)
		// A WAVE THAT TOOK THE FIRST-CELL RULE (fcm, the scalar mask of that test; every live row at rbeg = 0 is among its rows) forms cell 0's M flag again, by the
		// saturating comparison: there lane 0's h comes from d0h while M compares with d0s (kept in q0s), and where d0h < d0s the difference h - d0s can be negative,
		// which saturates to "no match" and would read as a match from the bits of d0s - h that the two-instruction insert looks at.  In every other wave d0h is d0s
		// in every lane, h >= d[0] as in the other cells, and the insert's bit stands: two instructions for cell 0 on those rows, where the saturating form took three.
		if(__builtin_expect(fcm != 0ull, 0)){
			accM[0] = (accM[0] & 0x7FFF7FFFu) | x_shl15(x_satsubu(ONE1, x_sub(hfirst, q0s)));
			if((__builtin_amdgcn_ballot_w64(rbeg == 0u) & actm) != 0ull){
				if(first && rbeg == 0u){
					const uint32_t hl = hfirst & 0xffffu;
					accM[0] = (accM[0] & ~0x8000u) | ((hl == q0m) ? 0x8000u : 0u);
					if constexpr (DO2){
						const uint32_t fld = (accDO[0] >> 6) & 3u;
						accDO[0] = (accDO[0] & ~0xC0u) | ((hl == q0d) ? 0x40u : 0u) | ((fld == (uint32_t)(-GO)) ? 0x80u : 0u);
					} else accD[0] = (accD[0] & ~0x8000u) | ((hl == q0d) ? 0x8000u : 0u);
				}
			}
		}
		// Moves of two and more: the cells whose upper neighbour (D / Od) or diagonal predecessor (M) is an entering cell lose those flags.  GENERAL FORM, per lane,
		// half hf and accumulator: block b = jl + L hf keeps D of its first nd = clamp(lim, 0, 16) cells and M of its first nm = clamp(lim + 1, 0, 16), with
		// lim = BW - mov - 16 b.  BW = 32 L, so a block b <= 2 L - 2 has lim >= 32 - mov and the last block (jl = L - 1, hf = 1) has lim = 16 - mov.  For mov <= 2
		// every block but the last keeps all (nd = nm = 16), and the last has
		//     mov = 0: nd = 16, nm = 16: nothing;     mov = 1: nd = 15, nm = 16;     mov = 2: nd = 14, nm = 15
		// which touches its second accumulator of eight alone (cd = nd - 8, cm = nm - 8; the first has cd = cm = 8: empty masks), in the high half:
		//     md = ((1 << (8 - cd)) - 1) << 24 = 0x01000000 (mov = 1), 0x03000000 (mov = 2);     mm = ((1 << (8 - cm)) - 1) << 24 = 0 (mov = 1), 0x01000000 (mov = 2)
		// and of the two-bit fields the fourth accumulator of four alone (c0 = nd - 12 = 3, 2; the others have c0 = 4: 0x55 & 0 = 0):
		//     (0x55 & ((1 << (8 - 2 c0)) - 1)) << 16 = 0x00010000 (mov = 1), 0x00050000 (mov = 2)
		// for L = 4 and L = 8 alike.  mov = 1 is what the branch below for rows without a move of two does.  So while no live pair of the wave moved by more than
		// two, the CONSTANT FORM does the general form's work with one mask per flag, chosen by mov in the pair's last lane; a wave with a live move of three and
		// more takes the general form for all its pairs.  (Rows past a short target may carry any mov into either form: nothing of theirs is stored.)
		if(__builtin_expect((__builtin_amdgcn_ballot_w64(mov > 1u) & actm) != 0ull, 0)){
			if((__builtin_amdgcn_ballot_w64(mov > 2u) & actm) == 0ull){
				const bool l1 = last && mov == 1u, l2 = last && mov == 2u;
				accM[NACC - 1] &= ~(l2 ? 0x01000000u : 0u);
				if constexpr (DO2){
					const uint32_t t = accDO[NDO - 1];
					const uint32_t z = ~(t | (t >> 1)) & (l2 ? 0x00050000u : l1 ? 0x00010000u : 0u);
					accDO[NDO - 1] = t | (z << (DOSP - 1u));          // z * DOSP, DOSP being 1 or 2
				} else accD[NACC - 1] &= ~(l2 ? 0x03000000u : l1 ? 0x01000000u : 0u);
			} else {
#pragma unroll
			for(int hf = 0; hf < 2; hf++){
				const int lim = BW - (int)mov - (jl + L * hf) * W;
				const int nd = min(max(lim, 0), W), nm = min(max(lim + 1, 0), W);
#pragma unroll
				for(int n = 0; n < NACC; n++){
					const int cd = min(max(nd - 8 * n, 0), 8), cm = min(max(nm - 8 * n, 0), 8);
					const uint32_t md = ((1u << (8 - cd)) - 1u) << (16 * hf + 8), mm = ((1u << (8 - cm)) - 1u) << (16 * hf + 8);
					if(mov != 0u){ if constexpr (!DO2) accD[n] &= ~md; accM[n] &= ~mm; }
				}
				if constexpr (DO2){
#pragma unroll
				for(int n = 0; n < NDO; n++){
					const int c0 = min(max(nd - 4 * n, 0), 4);
					const uint32_t cm = (0x55u & ((1u << (8 - 2 * c0)) - 1u)) << (16 * hf);
					const uint32_t z = ~(accDO[n] | (accDO[n] >> 1)) & cm;
					if(mov != 0u) accDO[n] |= z * DOSP;
				}
				}
			}
			}
		} else if constexpr (DO2){
			const uint32_t t = accDO[NDO - 1];
			if(mov == 1u && last && (t & 0x00030000u) == 0u) accDO[NDO - 1] = t | (DOSP << 16);
		} else accD[NACC - 1] &= ~((mov == 1u && last) ? 0x01000000u : 0u);          // band cell bw - 1 after a slide by one: no deletion there
		if constexpr (PW == 0){
#pragma unroll
			for(int n = 0; n < NACC; n++){ accR[n] = 0xFF00FF00u; accO[n] = 0xFF00FF00u; }          // linear gaps: every gap is opened at length 1
		}
		// ---- the code row (bsa_common.h "COMPACT slot"), the layouts of x_forward
		{
			uint32_t cur[ND];
			// (one-bit flags are bytes 1 and 3 of their accumulators, two-bit fields bytes 0 and 2)
			if constexpr (DO2){
				// M | R << 8 | two-bit fields << 16 per reference block
#pragma unroll
				for(int n = 0; n < NACC; n++){
					const uint32_t t1 = __builtin_amdgcn_perm(accR[n], accM[n], 0x07030501u);
					const uint32_t t2 = __builtin_amdgcn_perm(accDO[2 * n], accDO[2 * n + 1], 0x06020400u);
					cur[n] = __builtin_amdgcn_perm(t2, t1, 0x05040100u);
					cur[NACC + n] = __builtin_amdgcn_perm(t2, t1, 0x07060302u);
				}
			} else if constexpr (WR == 8){
				// M | D << 8 | R << 16 | Od << 24 per reference block
#pragma unroll
				for(int n = 0; n < NACC; n++){
					const uint32_t t1 = __builtin_amdgcn_perm(accD[n], accM[n], 0x07030501u);
					const uint32_t t2 = __builtin_amdgcn_perm(accO[n], accR[n], 0x07030501u);
					cur[n] = __builtin_amdgcn_perm(t2, t1, 0x05040100u);
					cur[NACC + n] = __builtin_amdgcn_perm(t2, t1, 0x07060302u);
				}
			} else {
				// sixteen cells a block: dword 0 = M | D << 16, dword 1 = R | Od << 16
				const uint32_t xm = __builtin_amdgcn_perm(accM[0], accM[1], 0x07030501u), xd = __builtin_amdgcn_perm(accD[0], accD[1], 0x07030501u);
				const uint32_t xr = __builtin_amdgcn_perm(accR[0], accR[1], 0x07030501u), xo = __builtin_amdgcn_perm(accO[0], accO[1], 0x07030501u);
				cur[0] = __builtin_amdgcn_perm(xd, xm, 0x05040100u); cur[1] = __builtin_amdgcn_perm(xo, xr, 0x05040100u);
				cur[2] = __builtin_amdgcn_perm(xd, xm, 0x07060302u); cur[3] = __builtin_amdgcn_perm(xo, xr, 0x07060302u);
			}
			const uint32_t ri = i & 3u;
			if constexpr (CWD == 1){
				uint32_t *const sr = stg + 64u * ri;
#pragma unroll
				for(int q = 0; q < ND; q++) sr[256 * q] = cur[q];
			} else {
				uint32_t *const sr = stg + (64u * ND) * ri;
#pragma unroll
				for(int q = 0; q < ND; q++) sr[64 * q] = cur[q];
			}
			if(act && (ri == 3u || i + 1u == tlen)){
				uint32_t *gp = (uint32_t*)rowp + bsa_code_off(i & ~3u, 0u, CWD);
				if constexpr (CWD == 1){
#pragma unroll
					for(int q = 0; q < ND; q++){
						const uint32_t blk = (uint32_t)(NACC * (jl + L * (q / NACC)) + q % NACC);
						uint4 t; t.x = stg[256 * q]; t.y = stg[256 * q + 64]; t.z = stg[256 * q + 128]; t.w = stg[256 * q + 192];
						*(uint4*)(gp + 4u * blk) = t;
					}
				} else {
					// a block's four rows of two dwords are contiguous: two 16-byte pieces of two rows each
#pragma unroll
					for(int hb = 0; hb < 2; hb++){
						uint32_t *bp = gp + (4u * CWD) * (uint32_t)(jl + L * hb);
#pragma unroll
						for(int pc = 0; pc < CWD; pc++){
							uint4 t;
							uint32_t *tw = (uint32_t*)&t;
#pragma unroll
							for(int e = 0; e < 4; e++){
								const int lin = 4 * pc + e, row = lin / CWD, d = lin % CWD;
								tw[e] = stg[64 * (ND * row + CWD * hb + d)];
							}
							*(uint4*)(bp + 4 * pc) = t;
						}
					}
				}
			}
		}
		// ---- tail: H^ left of every block (block 0: the virtual column, cell 0 + gape) and at the two ends of the row
		const uint32_t hv = x_add(Hp[0], GE16);
		const uint32_t Hsh = x_shift_down<L>(Hp[W - 1], hv, first);
		const uint32_t bcl = x_bcast_last<L>(Hp[W - 1]);
		if(act){
			constexpr uint32_t LM = (uint32_t)(L - 1);
			const bool lastrow = i + 1u == tlen;
			if((i & LM) == (uint32_t)jl) begq = (int)rbeg;
			if(((i & LM) == LM || lastrow) && (uint32_t)jl <= (i & LM)) begs[(i & ~LM) + 1u + (uint32_t)jl] = begq;
			// rbase and qlen - 1 - rbeg are read by the end-of-query candidate (non-global modes) and by the last row alone: formed behind one wave-level test
			if(__builtin_expect(__builtin_amdgcn_ballot_w64(lastrow || (mode != BSA_MODE_GLOBAL && rbeg + BW >= qlen)) != 0ull, 0)){
				const int rbase = base + GE * ((int)rbeg + (int)i);          // H at band position p = rbase + H^ + gape p
				auto score_at = [&](uint32_t pos) -> int {
					const uint32_t b = pos / W, kk = pos % W;
					const bool hi = b >= (uint32_t)L;
					uint32_t hh = Hp[0];
#pragma unroll
					for(int k = 1; k < W; k++) x_sel(hh, Hp[k], __ballot((uint32_t)k == kk));          // (a plain select chain is turned into an indexed load of the row from scratch)
					return rbase + (hi ? x_hi16(hh) : x_lo16(hh)) + GE * (int)pos;
				};
				if(mode != BSA_MODE_GLOBAL && rbeg + BW >= qlen){
					const uint32_t pos = qlen - 1u - rbeg;
					if(((pos / W) & (uint32_t)(L - 1)) == (uint32_t)jl){
						const int sc = score_at(pos);
						if(sc > cand_sc){ cand_sc = sc; cand_te = (int)i; }
					}
				}
				if(lastrow && mode == BSA_MODE_GLOBAL){
					const uint32_t pos = qlen - 1u - rbeg;
					int *const gs = begs + tlen + 1u;
					if(pos >= (uint32_t)BW){ if(first) *gs = (int)0x80000000u; }
					else if(((pos / W) & (uint32_t)(L - 1)) == (uint32_t)jl) *gs = score_at(pos);
				} else if(lastrow){
					bsa_code_end_t *er = (bsa_code_end_t*)(rowp + (size_t)bsa_code_rows(tlen) * (64u * CWD));
#pragma unroll
					for(int q = 0; q < 16 / L; q++){ er->cand_sc[jl + L * q] = q ? BSA_SCORE_MIN : cand_sc; er->cand_te[jl + L * q] = q ? 0 : cand_te; }
					int8_t *ub = (int8_t*)(er + 1);
#pragma unroll
					for(int hf = 0; hf < 2; hf++){
						const int b = jl + L * hf;
						auto half = [&](uint32_t x) -> int { return hf ? x_hi16(x) : x_lo16(x); };
						er->ubegs[b * CR] = rbase + half(Hsh) + GE * (b * W - 1);
						if constexpr (CR == 2) er->ubegs[b * CR + 1] = rbase + half(Hp[W / 2 - 1]) + GE * (b * W + W / 2 - 1);
#pragma unroll
						for(int k = 0; k < W; k++) ub[b * W + k] = (int8_t)(half(Hp[k]) - half((k == 0) ? Hsh : Hp[k - 1]) + GE);
					}
					if(last){ er->ubegs[16] = rbase + x_hi16(Hp[W - 1]) + GE * (BW - 1); er->rbeg_last = (int)rbeg; }
				}
			}
		}
		// ---- adaptive band + global steering (x_forward's, the block differences read from H^)
		{
			uint32_t nzsum;
			if constexpr (M3){
				// ubegs[b + 1] - ubegs[b] = H^(end of block b) - H^(left of it) + c gape over a block of c = 16 / CR cells.  In the biased frame every H^ of a live row is
				// a pattern in 0x0401 .. 0x7BFF (bsa_align8_abs_rows), and so is the virtual column of Hsh up to one gape below (>= 0x0401 - 127), so the halves are their own
				// values as UNSIGNED numbers and v_sad_u16 adds |a - b| of both halves into one 32-bit sum.  The constant goes UPWARD, onto the value left of the block (- c gape >= 0):
				// at most 0x7BFF + 16 * 127 = 0x83EF, inside 16 bits for every gape of the guard (|gape| <= 127), at either block size; added to the block's last cell it would
				// go below zero at sixteen cells a block (0x0401 - 16 * 127).  A pair's sum is 2 L CR <= 16 terms below 2^16 each: no carry is lost in 32 bits, where the packed
				// sum kept two 16-bit halves.  (Lanes of dead pairs and of rows past a short target sum arbitrary patterns: nothing reads their mov.)
				const uint32_t NC16 = x_i16(-(W / CR) * GE);
				uint32_t n;
				if constexpr (CR == 1) n = x_sad(Hp[W - 1], x_add(Hsh, NC16), 0u);
				else {
					n = x_sad(Hp[W / 2 - 1], x_add(Hsh, NC16), 0u);
					n = x_sad(Hp[W - 1], x_add(Hp[W / 2 - 1], NC16), n);
				}
				nzsum = x_sum32<L>(n);
			} else {
				// (the frame at 0: scores can be negative as int16, which v_sad_u16 would misread)
				uint32_t x;
				if constexpr (CR == 1){
					const uint32_t dl = x_add(x_sub(Hp[W - 1], Hsh), x_i16(W * GE));          // ubegs[b + 1] - ubegs[b]
					x = x_max(dl, x_sub(0u, dl));
				} else {
					const uint32_t HGE16 = x_i16((W / 2) * GE);
					const uint32_t da = x_add(x_sub(Hp[W / 2 - 1], Hsh), HGE16), db = x_add(x_sub(Hp[W - 1], Hp[W / 2 - 1]), HGE16);
					x = x_add(x_max(da, x_sub(0u, da)), x_max(db, x_sub(0u, db)));
				}
				x = x_sum<L>(x);
				nzsum = (x & 0xffffu) + (x >> 16);
			}
			const uint32_t bcf = x_bcast_first<L>(Hp[0]);
			const int d16 = x_hi16(bcl) - x_lo16(bcf) + (BW - 1) * GE;          // ubegs[16] - ubegs[0]
			uint32_t nz = nzsum / 16u;
			nz = nz / (uint32_t)WR * 16u / 2u;
			const int noisy = (int)((16u > nz) ? 16u : nz);
			int rbx;
			if(i <= (uint32_t)BW / 4u) rbx = 0;
			else if(rbeg + BW >= qlen) rbx = 0;
			else if(noisy < d16) rbx = 2;
			else if(d16 < -noisy) rbx = 0;
			else rbx = 1;
			if(mode == BSA_MODE_GLOBAL){
				const int rby = __builtin_amdgcn_ds_bpermute(rby_lane + (int)((i & (uint32_t)(L - 1)) << 2), (int)rt.k);
				const uint32_t left = tlen - i - 1u;
				bool rush;
				if(rush32) rush = act && rbeg + rzl + (uint32_t)BW <= qlen + (uint32_t)rbz - 1u;
				else {
					const unsigned long long lhs = (unsigned long long)rbeg + (unsigned long long)(uint32_t)rbz * left + (unsigned long long)BW;
					rush = act && lhs <= (unsigned long long)(uint32_t)(qlen + (uint32_t)rbz - 1u);
				}
				if((int)rbeg < rby - BW) mov = (uint32_t)(rbx + 1);
				else if((int)rbeg > rby) mov = (uint32_t)max(0, rbx - 1);
				else mov = (uint32_t)rbx;
				if(rush) mov = 1u + (uint32_t)(qlen - (rbeg + BW)) / max(left, 1u);
			} else mov = (uint32_t)rbx;
		}
		// ---- speculative slide by one cell: E of every block's first cell goes to the block before it, the entering cell's behind the last
		{
			const uint32_t efill = x_add(__builtin_amdgcn_perm(Hp[W - 1], Hp[W - 1], 0x03020302u), x_i16(cfirst - GE - NEWNE));
			E[W - 1] = x_shift_up<L>(tmpE0, efill, last);
			svH = hv; svE = tmpE0;
		}
		i++;
		rzl -= (uint32_t)rbz;
		if((i & 7u) == 0u && i < tlen){ __builtin_memcpy(&twin, tp + i, 8); twin <<= 3; }
	}
	if(st != nullptr && row1 < tlen){
		uint32_t *sp = st + (lt & 63);
		int r = 0;
		auto put = [&](uint32_t v){ __hip_atomic_store(sp + 64 * r, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); r++; };
#pragma unroll
		for(int k = 0; k < W; k++) put(Hp[k]);
#pragma unroll
		for(int k = 0; k < W; k++) put(E[k]);
		put((uint32_t)base); put(svH); put(svE);
		put(rbeg); put(mov); put((uint32_t)cand_sc); put((uint32_t)cand_te);
	}
}
// whole pairs in the absolute-score form (M3: x_forward_abs's three-operand maxima in the biased frame)
template<int L, int PW, bool DO2, bool M3 = true>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_align8_fwd_x_abs(const Align8Args a, const uint32_t rmask){
	x_forward_abs<L, 4, PW, DO2, false, M3>(a, a.first, a.count, blockIdx.x * 256u, rmask);
}

template<int W, int L, bool DO2 = false, bool SCORE = false>
__global__ void __launch_bounds__(256) k_align8_fwd_x(const Align8Args a){
	x_forward<W, L, 1, false, 4, DO2, false, SCORE>(a, a.first, a.count, blockIdx.x * 256u);
}
// linear gaps (piecewise 0)
template<int W, int L, bool SCORE = false>
__global__ void __launch_bounds__(256) k_align8_fwd_x0(const Align8Args a){
	x_forward<W, L, 0, false, 4, false, false, SCORE>(a, a.first, a.count, blockIdx.x * 256u);
}
// two-piece gaps (bandwidth 128): 8 bits per band cell
__global__ void __launch_bounds__(256) k_align8_fwd_x2(const Align8Args a){
	x_forward<8, 8, 2>(a, a.first, a.count, blockIdx.x * 256u);
}
// ... at bandwidth 64 (four lanes per pair) and 256 (sixteen cells a half: 256 registers, two waves per SIMD)
template<int W, int L>
__global__ void __launch_bounds__(256) k_align8_fwd_x2w(const Align8Args a){
	x_forward<W, L, 2>(a, a.first, a.count, blockIdx.x * 256u);
}
// bands that cover their whole queries (Align8Args::static_band): the row stays in place, no steering
template<int W, int L, int PW, bool DO2 = false, bool SCORE = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_align8_fwd_x_static(const Align8Args a){
	x_forward<W, L, PW, true, 4, DO2, false, SCORE>(a, a.first, a.count, blockIdx.x * 256u);
}

// Bandwidth 128, a batch that is not a whole number of four-lane rounds: the first nb8 blocks take the last n8 pairs
// eight lanes per pair, the others the first a.count - n8 pairs four lanes per pair.  One launch: the short blocks start
// first and the dispatcher hands the long ones to whichever CU has room, so pairs of one length no longer finish in
// lock-step rounds with a nearly empty last one.
// ABS: the four-lane blocks run the absolute-score form (rmask = its rebase period - 1)
template<bool ABS = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_align8_fwd_x_mix(const Align8Args a, const uint32_t nb8, const uint32_t n8, const uint32_t rmask = 0u){
	// one staging area and one query window for both shapes (four waves; <16, 4> is the larger: 16 code dwords and 2 x 16 window dwords a lane)
	__shared__ uint32_t mix_stage[4 * 16 * 64], mix_qwin[4 * 32 * 64];
	if(blockIdx.x < nb8) x_forward<8, 8, 1, false, 4, false, true>(a, a.first + (a.count - n8), n8, blockIdx.x * 256u, 0u, 0xFFFFFFF8u, nullptr, mix_stage, mix_qwin);
	else if constexpr (ABS) x_forward_abs<4, 4, 1, false, true>(a, a.first, a.count - n8, (blockIdx.x - nb8) * 256u, rmask, 0u, 0xFFFFFFF8u, nullptr, mix_stage, mix_qwin);
	else x_forward<16, 4, 1, false, 4, false, true>(a, a.first, a.count - n8, (blockIdx.x - nb8) * 256u, 0u, 0xFFFFFFF8u, nullptr, mix_stage, mix_qwin);
}

// PERSISTENT form for batches of more than one generation of resident waves.  A pair's rows are serial and pairs of one length finish
// together, so a launch of whole pairs ends with a generation that is mostly empty (100 000 pairs = 6250 waves of 16 pairs on 3072
// wave slots: two full generations and 106 waves alone on the chip for a third).  Here the work item is a SEGMENT of rows of the 16
// pairs of a wave: every wave of the launch takes ONE item (segment s of group g, all groups' segment s before any segment s + 1) off a
// counter, takes the band state the previous segment left in memory (XS_WORDS dwords a lane: the two row planes, the block offsets,
// the band position and its pending move), runs the rows and hands the state on.  The launch then ends within one segment of the
// ideal.  ctl[0] = next item, ctl[16 + g] = segments of group g that are done (release / acquire at agent scope: the next segment
// usually runs on another CU).  An item only ever waits for an item that was handed out before it, i.e. one that is running.
struct XQArgs { uint32_t *ctl; uint32_t *state; uint32_t ngroups, nseg, seg_rows, spin_cap, rmask; };          // ctl[0]: next ticket, ctl[1]: some wave gave up waiting, ctl[16 + g]: segments of group g done
// ABS: the absolute-score form of the row body (x_forward_abs; q.rmask = its rebase period - 1), M3: with its three-operand maxima in the biased frame
template<int W, int L, int PW, bool DO2 = false, int WPS = 3, bool SCORE = false, bool ABS = false, bool M3 = ABS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPS))) k_align8_fwd_xq(const Align8Args a, const XQArgs q){
	// one item per wave (a block is a wave: the dispatcher refills a wave slot the moment it is free); the ticket, not the block
	// index, names the item, so that an item's predecessor is always one that has started
	uint32_t id = 0;
	if(threadIdx.x == 0u) id = atomicAdd(q.ctl, 1u);
	id = (uint32_t)__builtin_amdgcn_readfirstlane((int)id);
	const uint32_t s = id / q.ngroups, g = id - s * q.ngroups;
	uint32_t *done = q.ctl + 16u + g;
	if(s != 0u){
		// BOUNDED wait (an item's predecessor was handed out earlier, i.e. is running: in a healthy launch this loop hardly ever turns).  Should the
		// predecessor never arrive -- a fault in its wave, a future change of the ticket order -- the wave gives up after about two seconds
		// (2^22 turns of s_sleep 16 = 1024 cycles), raises q.ctl[1] and flags its pairs BSA_ST_DEVICE instead of hanging the device: flagged pairs
		// are skipped by every later segment and by the traceback (zeroed result).  bsa_align_batch scans the status words and returns BSA_E_HIP;
		// a caller of the device-pointer form (bsa_align_run is asynchronous) finds the flag in its status array (include/bsalign_hip.h).
		// A wave waits for ITS predecessor only: another group's give-up does not end the wait of a healthy one.
		uint32_t gaveup = 0;
		if(threadIdx.x == 0u){
			uint32_t turns = 0;
			while(__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < s){
				__builtin_amdgcn_s_sleep(16);
				if(++turns >= q.spin_cap){ gaveup = 1; break; }
			}
		}
		gaveup = (uint32_t)__builtin_amdgcn_readfirstlane((int)gaveup);
		if(gaveup){
			const uint32_t pg = (g * 64u + threadIdx.x) / (uint32_t)L;
			if((threadIdx.x & (uint32_t)(L - 1)) == 0u && pg < a.count) atomicOr(&a.status[a.order[a.first + pg]], BSA_ST_DEVICE);
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");          // the flags are visible before the successor (which acquires after its wait) is let go
			if(threadIdx.x == 0u){
				atomicOr(q.ctl + 1, 1u);
				__hip_atomic_fetch_max(done, s + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);          // successors go on (and skip the flagged pairs)
			}
			return;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	}
	if constexpr (ABS){
		static_assert(W == 16 && PW <= 1 && !SCORE, "absolute-score form");
		x_forward_abs<L, 1, PW, DO2, false, M3>(a, a.first, a.count, g * 64u, q.rmask, s * q.seg_rows, (s + 1u) * q.seg_rows, q.state + (size_t)g * (XS_WORDS(W, PW) * 64u));
	} else
	x_forward<W, L, PW, false, 1, DO2, false, SCORE>(a, a.first, a.count, g * 64u, s * q.seg_rows, (s + 1u) * q.seg_rows, q.state + (size_t)g * (XS_WORDS(W, PW) * 64u));
	if(s + 1u < q.nseg){
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the state's write-through stores have arrived
		if(threadIdx.x == 0u) __hip_atomic_fetch_max(done, s + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (max: a successor that gave up may have written s + 2)
	}
}
// THE SHAPE RULE: cells per lane and half W and lanes per pair L of the kernels of a bandwidth and a gap model (2 W L = bw); false: there are none.  One-piece and
// linear gaps: 64 <8, 4>, 128 <16, 4>, 256 <16, 8>; two-piece gaps keep eight cells a half at 128: <8, 8>.  x_choose leaves it in two places, both behind a knob or
// a check of their own: BSA_ALIGN8_X_LANES=8 runs <4, 8> at 64 (whole pairs only), and two-piece row segments at 128 run <16, 4> (unless BSA_ALIGN8_X2_LANES=8).
static bool x_shape(uint32_t bw, int pw, uint32_t &W, uint32_t &L){
	if(pw < 0 || pw > 2 || !(bw == 64u || bw == 128u || bw == 256u)) return false;
	L = (bw == 256u || (pw == 2 && bw == 128u)) ? 8u : 4u;
	W = bw / (2u * L);
	return true;
}
// bytes of a.xq the persistent form needs for `count` pairs at the rule's shape (0: there are no such kernels): 64 dwords of control block and one a group, rounded
// up by a whole 256 where x_segments rounds to one, so its check passes at this shape for every count.  The <16, 4, 2> first try at bandwidth 128 is not sized for:
// it takes 59 state words a lane at sixteen pairs a wave where <8, 8, 2> takes 35 at eight, 15104 bytes a group of sixteen pairs against 2 x 8960, so it fits
// whenever count mod 16 is 0 or above 8, or count > 48; for 1..8, 17..24 and 33..40 pairs in a buffer of exactly this size it does not, and x_choose falls back to
// the <8, 8, 2> segments, which do.  (The context's buffer only grows: after a larger batch the first try fits there as well.)
size_t bsa_align8_xq_bytes(uint32_t bw, int pw, uint32_t count){
	uint32_t W, L;
	if(!x_shape(bw, pw, W, L)) return 0;
	const size_t groups = ((size_t)count * L + 63u) / 64u;
	return (16u + groups) * 4u + 256u + groups * (size_t)(XS_WORDS(W, pw) * 64u * 4u);
}
// name of a launch in the absolute-score form: the family's description, the rebase period and the form of the maxima that bsa_align8_abs_rows chose (tests read it)
static const char *x_abs_name(const char *what, uint32_t rebase_rows, bool m3){
	static thread_local char buf[320];
	snprintf(buf, sizeof buf, "%s [rebase every %u rows] [%s]", what, rebase_rows, m3 ? "three-operand maxima, biased frame" : "integer maxima");
	return buf;
}

// Exact arithmetic is the reference's arithmetic only while nothing saturates: the guard of the compact path
// (bsa_align8_codes_supported) plus room for the frame shift by 2 |gape| and for the int16 block offsets.
bool bsa_align8_x_supported(const Align8Args &a, int pw){
	const uint32_t W = a.bw / 16;
	const int ge = -(int)(int8_t)a.gape1, go = -(int)(int8_t)a.gapo1, m = a.smax, n = -a.smin;
	if(ge < 0 || go < 0 || m < 0 || n < 0 || (go == 0) != (pw == 0)) return false;
	int g = go + ge;
	if(pw == 2){
		// two pieces: bandwidth 64, 128, 256 (all three modes: the end record of overlap / extend is the one-piece kernels'); piece 2 opens
		// dearer and extends cheaper (bsalign.h:2084-2092 guarantees it), the bound is taken with the dearer opening
		if(!(W == 4 || W == 8 || W == 16)) return false;
		const int ge2 = -(int)(int8_t)a.gape2, go2 = -(int)(int8_t)a.gapo2;
		if(ge2 < 0 || go2 <= go || ge2 >= ge) return false;
		g = std::max(g, go2 + ge2);
		if(m + 3 * g > 64 || n + m + g > 100) return false;      // the compact path's own bound (bsa_align8_codes_supported)
	} else {
		if(pw > 1 || !bsa_align8_codes_supported(a, pw)) return false;
		if(!(W == 4 || W == 8 || W == 16)) return false;
	}
	const int cfirst = std::min(a.smin, -g) - 1 - a.smax - g;
	if(cfirst < -100) return false;
	return m + 3 * g + 2 * ge <= 100 && n + m + g + 2 * ge <= 110 && 63 + 2 * ge + n + m + 2 * g <= 125;
}

// Rebase period of the absolute-score form (x_forward_abs) in rows, a power of two; 0 = this launch keeps the difference form.
// The form exists for one-piece and linear gaps at bandwidth 128 and 256 (sixteen cells a half).  Bound, with m = smax, go = -gapo, ge = -gape, g = go + ge, in the frame
// H^ = H - gape (x + y) - base:
//   * step along a computed row, u^ = H^(x, y) - H^(x - 1, y): at least -go, because F^(x) >= H^(x - 1) + gapo; at most m + go + 2 ge, by induction over the rows: if h comes from F,
//     u^ <= 0; from the diagonal, H^(x - 1, y) >= E^ >= H^(x - 1, y - 1) + gapo gives u^ <= S~ - gapo <= m + 2 ge + go; from E, both columns took the same gap from a row y' and
//     u^(y) <= u^(y').  Cells behind the band end enter flat (u^ = 0) behind one step of cfirst - gape < 0, which only ever lowers the upper bound's induction.  So a row of bw cells
//     spans at most s bw with s = max(go, m + go + 2 ge).
//   * drift from row to row: every cell is at least its upper neighbour's H^ + gapo and at most the previous row's maximum + max(S~) = m + 2 ge: at most s a row, either way.
//   * what is not a computed cell lies within K = 512 of one: E^ and F^ (within go), mg = m + gapo, the -63 - 2 ge sentinels of F and of the first-cell rule, the virtual column
//     (+ gape), the entering cells (cfirst - gape - gape >= -100 - 2 ge inside the guard), the pads beyond the query end.  A band that jumps past all it held starts from a row that
//     is -gape p by construction: the SCORE_MIN of its real scores is carried by the int32 base, not by the int16 row.
// A rebase puts the row's first slot at the frame's origin; R rows later every value lies within D(R) = s (bw + R) + K of it.
//   * Three-operand maxima (x_forward_abs, M3; *m3 = true): the origin is B = 0x4000 and every operand of a maximum must be an int16 whose pattern an f16 maximum orders as an
//     integer one does, 0x0400 .. 0x7BFF.  That is [B - 15360, B + 15359]: D(R) <= 15359, the smaller side.  K = 512 already covers what enters those maxima beside cells:
//     E^, F^, the sentinels and fini - gapo (within 63 + 2 ge + go of a cell), the entering cells, the pads.
//   * Integer maxima (*m3 = false): the origin is 0 and an int16 holds D(R) <= 32767.
// R is the largest power of two up to 64 that meets the first bound; a scoring that leaves no R >= 8 there takes the largest that meets the second, and one that leaves none
// there either keeps the difference form.  (The benchmark's scoring: s = 9, 9 (128 + 64) + 512 = 2240.)  The guard gives s <= m + 3 g + 2 ge <= 100, and at bandwidth 128
// s (128 + 8) + 512 <= 15359 holds up to s = 109: the integer maxima are only ever chosen at bandwidth 256 (s >= 57), and the launchers build them for that width alone.
// A shorter period with three-operand maxima is still the cheaper row: a rebase is 37 instructions every R rows, the maxima save 30 a row.
// BSA_ALIGN8_ABS=0 keeps the difference form.  BSA_ALIGN8_ABS_R=<rows> (test hook) shortens the period: the largest power of two that is at most <rows>, at least 8 and at most
// the derived R; anything that is not a number of at least 8 gives 8.
uint32_t bsa_align8_abs_rows(const Align8Args &a, int pw, bool *m3){
	if(m3) *m3 = false;
	const char *e = bsa_env("BSA_ALIGN8_ABS");
	if((e && e[0] == '0') || pw > 1 || !(a.bw == 128u || a.bw == 256u) || !bsa_align8_x_supported(a, pw)) return 0u;
	const int go = -(int)(int8_t)a.gapo1, ge = -(int)(int8_t)a.gape1, m = a.smax;
	const int s = std::max(go, m + go + 2 * ge);
	uint32_t r = 64u;
	while(r >= 8u && s * (int)(a.bw + r) + 512 > 15359) r >>= 1;
	if(r >= 8u){ if(m3) *m3 = true; }
	else {
		r = 64u;
		while(r >= 8u && s * (int)(a.bw + r) + 512 > 32767) r >>= 1;
		if(r < 8u || a.bw != 256u) return 0u;
	}
	if(const char *re = bsa_env("BSA_ALIGN8_ABS_R")){
		const long want = std::max(atol(re), 8L);
		uint32_t f = 8u;
		while(f * 2u <= r && (long)(f * 2u) <= want) f *= 2u;
		r = f;
	}
	return r;
}

// Largest difference that a one-bit flag insert of x_forward_abs (x_ins) sees in a STORED cell of a live pair; the insert is exact for 0 .. 256.  terms (may be
// null) receives the BSA_FLAG_SPAN_TERMS terms the maximum is taken over.  0: the scoring does not run the absolute-score form.
// With m = smax, n = -smin, go, ge, g as in bsa_align8_abs_rows, P = 63 (-BSA_EPI8_MIN = BSA_EPI8_MAX) and, of a cell (x, y), A = Hp = H^(x - 1, y - 1) its diagonal
// predecessor, U = H^(x, y - 1) its upper and Lf = H^(x - 1, y) its left neighbour:
//   * S~ = S - 2 gape lies in [-max(n, P) + 2 ge, m + 2 ge]: the low end is a mismatch or the pad code beyond the query's end (-P - 2 gape), whichever is lower.
//   * s1 = m + go + 2 ge bounds a step between computed neighbours from above, along a row (U - A, bsa_align8_abs_rows) and, by the same induction with rows and
//     columns exchanged, down a column (Lf - A); both are at least -go (H >= F, H >= E of the next row).  The induction down a column starts at the band's first
//     cell: after a slide its neighbours are computed cells; on a row that does not move or that jumps, the first-cell rule clamps it to at most BSA_EPI8_MAX above
//     the virtual column, which is gape below the cell's upper neighbour: c0 = P + ge.  So Lf - A <= V = max(s1, c0).
//   * E^ lies in [U - go, U] and f = F^ in [Lf - go, Lf] (or is the low -P - 2 gape sentinel), h = max(E, d, f) with d = A + S~.
//   M  (h - d = max(0, E - d, f - d)):  E - d <= (U - A) - S~ <= s1 + max(n, P) - 2 ge  and  f - d <= (Lf - A) - S~ <= V + max(n, P) - 2 ge             [term 0: the latter]
//   D  (h - E = max(0, d - E, f - E)):  d - E <= (A - U) + S~ + go <= m + 2 ge + 2 go [1];  f - E <= (Lf - A) + (A - U) + go <= V + 2 go [2];  in row -1 E^ is
//      the -P sentinel, P - ge below A (global; P - 2 ge in overlap mode): d - E <= m + 2 ge + P - ge [3], f - E <= V + P - ge [4]
//   R, Od  (fm - hg, en - hg with hg = h + gapo <= fm, en <= h):  go [5]
//   * the row a jumping band starts from (Hp = -gape p, E^ = Hp + 2 ge one cell on) has steps of ge, and its first cell obeys the same clamp: E - d <= 2 ge - S~, d - E <= m,
//     f - E <= max(P, m): all below the terms above.  The cell entering behind the band end (H^ = last + cfirst - gape, E^ = that - gape) is far BELOW its
//     neighbours: as E of the new last cell it makes E - d negative, and M there has computed cells for A and Lf.
//   * not covered, because a fix-up overwrites the flag and an insert touches its own bit only: M and D of lane 0's cell 0 at rbeg = 0 (and M of cell 0 keeps the
//     saturating form everywhere: x_forward_abs), D of the cells whose upper neighbour is an entering cell and M of those whose diagonal predecessor is one (the
//     `mov == 1 && last` bit and the md / mm masks of moves of two and more).
// Inside bsa_align8_x_supported every term is at most 126: the third inequality (63 + 2 ge + n + m + 2 g <= 125) gives n <= 62 and m + go + ge + 63 <= 125, the first
// m + 3 go + 2 ge <= 100; so there is one form of the inserts and the launcher has nothing to choose (tests/test_align8_flag_span_cpu.py walks a grid).
uint32_t bsa_align8_flag_span(const Align8Args &a, int pw, uint32_t terms[BSA_FLAG_SPAN_TERMS]){
	if(bsa_align8_abs_rows(a, pw) == 0u) return 0u;
	const int go = -(int)(int8_t)a.gapo1, ge = -(int)(int8_t)a.gape1, m = a.smax, n = -a.smin, P = -BSA_EPI8_MIN;
	static_assert(BSA_EPI8_MAX == -BSA_EPI8_MIN, "the first-cell rule's clamp and the sentinels are one figure here");
	const int s1 = m + go + 2 * ge, V = std::max(s1, P + ge), lowS = std::max(n, P) - 2 * ge, hiS = m + 2 * ge;
	const int t[BSA_FLAG_SPAN_TERMS] = {V + lowS, hiS + 2 * go, V + 2 * go, hiS + P - ge, V + P - ge, go};
	if(terms) for(int k = 0; k < BSA_FLAG_SPAN_TERMS; k++) terms[k] = (uint32_t)std::max(t[k], 0);
	return (uint32_t)std::max(*std::max_element(t, t + BSA_FLAG_SPAN_TERMS), 0);
}

// The launcher's BSA_ALIGN8_* knobs, each read here and nowhere else (BSA_ALIGN8_ABS and _ABS_R: bsa_align8_abs_rows); x_choose takes them anew at every launch.
struct XKnobs {
	char xq = 0, lanes = 0;          // first character of _XQ (0: never row segments, 1: wherever there is a form and room) and of _X_LANES (4 / 8: one shape for all pairs)
	bool lanes_set, n8_set, x2_lanes8, no_static, do2_off;
	long xq_seg = 0, spin_cap = 0, n8 = -1;          // _XQ_SEG rows a segment, _XQ_SPIN_CAP (test hook: a cap of a few turns makes hand-over waits give up), _X_N8 (tuning: pairs that go eight lanes per pair)
	XKnobs(){
		const char *e;
		if((e = bsa_env("BSA_ALIGN8_XQ"))) xq = e[0];
		if((e = bsa_env("BSA_ALIGN8_XQ_SEG"))) xq_seg = atol(e);
		if((e = bsa_env("BSA_ALIGN8_XQ_SPIN_CAP"))) spin_cap = atol(e);
		if((lanes_set = (e = bsa_env("BSA_ALIGN8_X_LANES")) != nullptr)) lanes = e[0];
		if((n8_set = (e = bsa_env("BSA_ALIGN8_X_N8")) != nullptr)) n8 = atol(e);
		x2_lanes8 = (e = bsa_env("BSA_ALIGN8_X2_LANES")) && e[0] == '8';
		no_static = bsa_env("BSA_ALIGN8_NO_STATIC") != nullptr;
		do2_off = (e = bsa_env("BSA_ALIGN8_DO2")) && e[0] == '0';
	}
};

// the code rows with two-bit D / Od fields (Align8Args::code_fmt 1): what the forward kernels need; the traceback side is asked in bsa_api.hip
bool bsa_align8_do2_supported(const Align8Args &a, int pw){
	const int go = -(int)(int8_t)a.gapo1;
	const XKnobs k;
	return pw == 1 && a.bw == 128u && go >= 1 && go <= 3 && !k.do2_off && !k.lanes_set && !k.n8_set && bsa_align8_x_supported(a, pw);
}

// ONE LAUNCH of the forward DP, as x_choose decides it and x_run makes it
enum XForm : uint32_t { X_NONE, X_STATIC, X_SEG, X_WHOLE, X_MIX };          // no such launch; band in place; row segments; whole pairs; whole pairs, four and eight lanes per pair in one launch
struct XLaunch {
	XForm form; uint32_t W, L; int pw;          // the kernel's shape and gap model (X_MIX: the four-lane share's <16, 4>; its eight-lane blocks are <8, 8>)
	bool do2, score, abs, m3;                   // code format 1; score only; absolute-score form (X_MIX: in the four-lane blocks), with three-operand maxima
	uint32_t wps, rebase_rows;                  // X_SEG: waves per SIMD the kernel is built for; abs: the rebase period
	uint32_t grid;                              // blocks: of one wave for X_SEG, of four otherwise
	XQArgs q; size_t ctl_bytes;                 // X_SEG: the kernel's arguments but for the two pointers, and the bytes of the control block in front of the states
	uint32_t n8, nb8;                           // X_MIX: pairs and blocks at eight lanes per pair (the batch's last n8 pairs, the launch's first nb8 blocks)
	const char *name;                           // for bsa_last_fwd_kernel; nullptr: none, bsa_align_run's default for the path shows
};
// The name of a launch.  Kept as they were when every launch site set (or did not set) its own, so some misdescribe their kernel: the in-place kernels without
// code format 1 or score-only and the difference-form mix report nothing (the default names k_align8_fwd_x / k_align8_fwd_x2, whole pairs), the two-piece row
// segments at bandwidth 64 report 4-bit codes (HISTORY §14 has the list).
static const char *x_name(const XLaunch &l){
	switch(l.form){
		case X_STATIC:
			return l.do2 ? "k_align8_fwd_x_static (exact-arithmetic forward DP, band in place, traceback codes with two-bit D/Od fields)"
				: l.score ? "k_align8_fwd_x_static score-only (exact-arithmetic forward DP, band in place, no traceback codes)" : nullptr;
		case X_SEG:
			if(l.score) return "k_align8_fwd_xq score-only (exact-arithmetic forward DP in row segments, no traceback codes)";
			if(l.do2) return l.abs ? x_abs_name("k_align8_fwd_xq (exact-arithmetic forward DP in row segments, absolute scores, traceback codes with two-bit D/Od fields)", l.rebase_rows, l.m3)
				: "k_align8_fwd_xq (exact-arithmetic forward DP in row segments, traceback codes with two-bit D/Od fields)";
			if(l.abs) return x_abs_name("k_align8_fwd_xq (exact-arithmetic forward DP in row segments, absolute scores, 4-bit traceback codes)", l.rebase_rows, l.m3);
			if(l.pw == 2 && l.W == 16u) return "k_align8_fwd_xq (exact-arithmetic forward DP in row segments, two-piece gaps, four lanes per pair, 8-bit traceback codes)";
			if(l.pw == 2 && l.L == 8u) return "k_align8_fwd_xq (exact-arithmetic forward DP in row segments, two-piece gaps, 8-bit traceback codes)";
			return "k_align8_fwd_xq (exact-arithmetic forward DP in row segments, 4-bit traceback codes)";
		case X_WHOLE:
			if(l.score) return "k_align8_fwd_x score-only (exact-arithmetic forward DP, no traceback codes)";
			if(l.do2) return l.abs ? x_abs_name("k_align8_fwd_x (exact-arithmetic forward DP, absolute scores, traceback codes with two-bit D/Od fields)", l.rebase_rows, l.m3)
				: "k_align8_fwd_x (exact-arithmetic forward DP, traceback codes with two-bit D/Od fields)";
			if(l.abs) return x_abs_name("k_align8_fwd_x (exact-arithmetic forward DP, absolute scores, 4-bit traceback codes)", l.rebase_rows, l.m3);
			return l.pw == 2 && l.W * l.L != 64u ? "k_align8_fwd_x2 (exact-arithmetic forward DP, two-piece gaps, 8-bit traceback codes)" : nullptr;
		case X_MIX:
			return l.abs ? x_abs_name("k_align8_fwd_x_mix (exact-arithmetic forward DP, absolute scores in the four-lane blocks, 4-bit traceback codes)", l.rebase_rows, l.m3) : nullptr;
		default: return nullptr;
	}
}
// Row segments at l's shape: where the batch is more than one generation of resident waves (or BSA_ALIGN8_XQ=1) and a.xq holds its control block and states
static bool x_segments(XLaunch &l, const Align8Args &a, const XKnobs &k, int cus){
	const uint32_t groups = (uint32_t)(((size_t)a.count * l.L + 63u) / 64u);
	const uint32_t workers = (uint32_t)cus * 4u * l.wps;          // waves per SIMD x SIMDs
	if(k.xq != '1' && groups <= workers) return false;       // one generation: whole pairs
	const size_t ctl_bytes = ((16u + (size_t)groups) * 4u + 255u) & ~(size_t)255u;
	if(ctl_bytes + (size_t)groups * (XS_WORDS(l.W, l.pw) * 64u * 4u) > a.xq_bytes) return false;
	// segments: the last item of the launch should be a few percent of a wave slot's share
	uint32_t nseg = (uint32_t)std::min<uint64_t>(64u, (48ull * workers + groups - 1u) / groups);
	uint32_t seg_rows = ((a.max_tlen + nseg - 1u) / std::max(nseg, 1u) + 7u) & ~7u;
	if(k.xq_seg >= 8) seg_rows = ((uint32_t)k.xq_seg + 7u) & ~7u;
	seg_rows = std::max(seg_rows, 64u);
	nseg = std::max(1u, (a.max_tlen + seg_rows - 1u) / seg_rows);
	l.form = X_SEG; l.grid = groups * nseg; l.ctl_bytes = ctl_bytes;
	l.q = XQArgs{nullptr, nullptr, groups, nseg, seg_rows, k.spin_cap >= 1 ? (uint32_t)k.spin_cap : 1u << 22, l.abs ? l.rebase_rows - 1u : 0u};
	return true;
}
// What to launch for a chunk of a.count > 0 pairs on a device of `cus` CUs (form X_NONE: nothing, the arguments name no kernel).  No HIP call.  In order: the shape;
// band in place; absolute scores or differences; row segments; else whole pairs, at bandwidth 128 with one-piece gaps and plain codes split between lane counts.
static XLaunch x_choose(const Align8Args &a, int pw, bool score, int cus){
	const XKnobs k;
	XLaunch l{};
	l.pw = pw; l.score = score; l.do2 = a.code_fmt == 1u; l.wps = 3u;
	// score only: one-piece and linear gaps, no codes; two-bit D / Od fields (bsa_align8_do2_supported): bandwidth 128, one-piece gaps, four lanes per pair
	if(!x_shape(a.bw, pw, l.W, l.L) || (score && (pw > 1 || a.code_fmt != 0u)) || (l.do2 && (pw != 1 || a.bw != 128u))) return l;
	auto done = [&a](XLaunch &r){ if(r.form != X_SEG && r.form != X_MIX) r.grid = (uint32_t)(((uint64_t)a.count * r.L + 255u) / 256u); r.name = x_name(r); return r; };
	// bands that cover their whole queries stay in place (two-piece gaps: a kernel at 128 alone)
	if(a.static_band && !k.no_static && !(pw == 2 && a.bw != 128u)){ l.form = X_STATIC; return done(l); }
	// absolute-score form (bandwidth 128, 256; never score only); integer maxima at bandwidth 256 alone
	if(!score && (l.rebase_rows = bsa_align8_abs_rows(a, pw, &l.m3)) != 0u) l.abs = true;
	const bool mixable = !score && !l.do2 && pw == 1 && a.bw == 128u;
	if(!score && pw <= 1 && a.bw == 64u && k.lanes == '8'){ l.W = 4u; l.L = 8u; }          // BSA_ALIGN8_X_LANES=8 at 64: eight lanes per pair, whole pairs only
	if(a.xq && k.xq != '0' && l.W != 4u && !(mixable && (k.lanes_set || k.n8_set))){
		if(pw == 2 && a.bw == 128u && !k.x2_lanes8){
			// four lanes per pair at two waves per SIMD (sixteen pairs a wave share the per-row work: 126 ms against 137 for the eight-lane shape
			// at three waves, C2's shape); bsa_align8_xq_bytes does not size for it: where it does not fit, the rule's own shape below
			XLaunch f = l; f.W = 16u; f.L = 4u; f.wps = 2u;
			if(x_segments(f, a, k, cus)) return done(f);
		}
		if(!(pw == 2 && a.bw == 256u) && x_segments(l, a, k, cus)) return done(l);
	}
	l.form = X_WHOLE;
	if(mixable){
		// Four lanes per pair (16 pairs per wave) cost 620 instructions per row of a wave, eight lanes per pair 387.  Pairs of one length finish together, so what
		// counts is the largest number of waves any SIMD gets: whole rounds of one four-lane wave per SIMD, and a remainder of at most half a round as eight-lane
		// waves (0.62 of a round instead of a whole one).  BSA_ALIGN8_X_LANES=4 / 8 forces one shape.
		const uint32_t round4 = (uint32_t)cus * 4u * 16u;
		uint32_t n4 = a.count / round4 * round4;
		if(a.count - n4 > round4 / 2u) n4 = a.count;
		if(k.lanes == '8') n4 = 0;
		if(k.lanes == '4') n4 = a.count;
		if(k.n8 >= 0 && (uint32_t)k.n8 <= a.count) n4 = a.count - (uint32_t)k.n8;
		// (the four-lane shape runs the absolute-score form where it applies; the eight-lane one, eight cells a half, has none)
		if(n4 == 0){ l.W = l.L = 8u; l.abs = l.m3 = false; l.rebase_rows = 0u; }
		else if(n4 != a.count){ l.form = X_MIX; l.n8 = a.count - n4; l.nb8 = (l.n8 + 31u) / 32u; l.grid = l.nb8 + (n4 + 63u) / 64u; }
	}
	return done(l);
}

// x_choose as plain numbers, for tests of its contract (bsa_align8_x_choice_internal; no device): false = no such launch
bool bsa_align8_x_choice(const Align8Args &a, int pw, bool score, int cus, uint64_t out[BSA_X_CHOICE_WORDS], const char **name){
	const XLaunch l = x_choose(a, pw, score, cus);
	const uint64_t v[BSA_X_CHOICE_WORDS] = {l.form, l.W, l.L, (uint64_t)l.pw, l.do2, l.score, l.abs, l.m3, l.wps, l.rebase_rows, l.grid, l.q.ngroups, l.q.nseg, l.q.seg_rows,
		l.q.spin_cap, l.q.rmask, l.ctl_bytes, l.form == X_SEG ? (uint64_t)l.q.ngroups * (XS_WORDS(l.W, l.pw) * 64u * 4u) : 0u, l.n8, l.nb8};
	std::copy(v, v + BSA_X_CHOICE_WORDS, out);
	*name = l.name;
	return l.form != X_NONE;
}

// The one place that launches: every instance of the forward kernels is one row of the table in x_run, keyed by the description that runs it (a key twice does not
// compile).  The row macros stay defined to the end of the file: x_run and the two launchers.
constexpr uint32_t x_key(uint32_t form, uint32_t W, uint32_t L, int pw, bool do2, bool score, bool abs, bool m3, uint32_t wps){
	return form | W << 3 | L << 8 | (uint32_t)pw << 12 | (uint32_t)do2 << 14 | (uint32_t)score << 15 | (uint32_t)abs << 16 | (uint32_t)m3 << 17 | wps << 18;
}
#define X_STATIC_K(W, L, PW, DO2, SCORE) case x_key(X_STATIC, W, L, PW, DO2, SCORE, false, false, 3): hipLaunchKernelGGL((k_align8_fwd_x_static<W, L, PW, DO2, SCORE>), grid, dim3(256), 0, st, a); break;
#define X_SEG_K(W, L, PW, DO2, WPS, SCORE, ABS, M3) case x_key(X_SEG, W, L, PW, DO2, SCORE, ABS, M3, WPS): hipLaunchKernelGGL((k_align8_fwd_xq<W, L, PW, DO2, WPS, SCORE, ABS, M3>), grid, dim3(64), 0, st, a, q); break;
#define X_ABS_K(L, PW, DO2, M3) case x_key(X_WHOLE, 16, L, PW, DO2, false, true, M3, 3): hipLaunchKernelGGL((k_align8_fwd_x_abs<L, PW, DO2, M3>), grid, dim3(256), 0, st, a, rmask); break;
#define X_K1(W, L, DO2, SCORE) case x_key(X_WHOLE, W, L, 1, DO2, SCORE, false, false, 3): hipLaunchKernelGGL((k_align8_fwd_x<W, L, DO2, SCORE>), grid, dim3(256), 0, st, a); break;
#define X_K0(W, L, SCORE) case x_key(X_WHOLE, W, L, 0, false, SCORE, false, false, 3): hipLaunchKernelGGL((k_align8_fwd_x0<W, L, SCORE>), grid, dim3(256), 0, st, a); break;
#define X_K2W(W, L) case x_key(X_WHOLE, W, L, 2, false, false, false, false, 3): hipLaunchKernelGGL((k_align8_fwd_x2w<W, L>), grid, dim3(256), 0, st, a); break;
#define X_MIX_K(ABS) case x_key(X_MIX, 16, 4, 1, false, false, ABS, ABS, 3): hipLaunchKernelGGL(k_align8_fwd_x_mix<ABS>, grid, dim3(256), 0, st, a, l.nb8, l.n8, ABS ? rmask : 0u); break;
static hipError_t x_run(const XLaunch &l, const Align8Args &a, hipStream_t st){
	XQArgs q = l.q;
	if(l.form == X_SEG){
		q.ctl = a.xq; q.state = (uint32_t*)((uint8_t*)a.xq + l.ctl_bytes);
		const hipError_t err = hipMemsetAsync(a.xq, 0, l.ctl_bytes, st);
		if(err != hipSuccess) return err;
	}
	const dim3 grid(l.grid);
	const uint32_t rmask = l.rebase_rows - 1u;          // (read by the absolute-score forms alone)
	switch(x_key(l.form, l.W, l.L, l.pw, l.do2, l.score, l.abs, l.m3, l.wps)){
		// band in place: linear, one-piece (plain codes, code format 1, score only), two-piece gaps
		X_STATIC_K(8, 4, 0, false, false) X_STATIC_K(16, 4, 0, false, false) X_STATIC_K(16, 8, 0, false, false)
		X_STATIC_K(8, 4, 0, false, true) X_STATIC_K(16, 4, 0, false, true) X_STATIC_K(16, 8, 0, false, true)
		X_STATIC_K(8, 4, 1, false, false) X_STATIC_K(16, 4, 1, false, false) X_STATIC_K(16, 8, 1, false, false)
		X_STATIC_K(8, 4, 1, false, true) X_STATIC_K(16, 4, 1, false, true) X_STATIC_K(16, 8, 1, false, true)
		X_STATIC_K(16, 4, 1, true, false) X_STATIC_K(8, 8, 2, false, false)
		// row segments: the difference form, score only, absolute scores (integer maxima at <16, 8> alone), code format 1, two-piece gaps
		X_SEG_K(8, 4, 0, false, 3, false, false, false) X_SEG_K(16, 4, 0, false, 3, false, false, false) X_SEG_K(16, 8, 0, false, 3, false, false, false)
		X_SEG_K(8, 4, 1, false, 3, false, false, false) X_SEG_K(16, 4, 1, false, 3, false, false, false) X_SEG_K(16, 8, 1, false, 3, false, false, false)
		X_SEG_K(8, 4, 0, false, 3, true, false, false) X_SEG_K(16, 4, 0, false, 3, true, false, false) X_SEG_K(16, 8, 0, false, 3, true, false, false)
		X_SEG_K(8, 4, 1, false, 3, true, false, false) X_SEG_K(16, 4, 1, false, 3, true, false, false) X_SEG_K(16, 8, 1, false, 3, true, false, false)
		X_SEG_K(16, 4, 0, false, 3, false, true, true) X_SEG_K(16, 8, 0, false, 3, false, true, true) X_SEG_K(16, 8, 0, false, 3, false, true, false)
		X_SEG_K(16, 4, 1, false, 3, false, true, true) X_SEG_K(16, 8, 1, false, 3, false, true, true) X_SEG_K(16, 8, 1, false, 3, false, true, false)
		X_SEG_K(16, 4, 1, true, 3, false, false, false) X_SEG_K(16, 4, 1, true, 3, false, true, true)
		X_SEG_K(8, 4, 2, false, 3, false, false, false) X_SEG_K(8, 8, 2, false, 3, false, false, false) X_SEG_K(16, 4, 2, false, 2, false, false, false)
		// whole pairs in absolute scores
		X_ABS_K(4, 0, false, true) X_ABS_K(8, 0, false, true) X_ABS_K(8, 0, false, false)
		X_ABS_K(4, 1, false, true) X_ABS_K(8, 1, false, true) X_ABS_K(8, 1, false, false) X_ABS_K(4, 1, true, true)
		// whole pairs in differences: one-piece gaps (plain codes, code format 1, score only), linear gaps, two-piece gaps
		X_K1(4, 8, false, false) X_K1(8, 4, false, false) X_K1(8, 8, false, false) X_K1(16, 4, false, false) X_K1(16, 8, false, false)
		X_K1(16, 4, true, false) X_K1(8, 4, false, true) X_K1(16, 4, false, true) X_K1(16, 8, false, true)
		X_K0(4, 8, false) X_K0(8, 4, false) X_K0(16, 4, false) X_K0(16, 8, false) X_K0(8, 4, true) X_K0(16, 4, true) X_K0(16, 8, true)
		X_K2W(8, 4) X_K2W(16, 8) case x_key(X_WHOLE, 8, 8, 2, false, false, false, false, 3): hipLaunchKernelGGL(k_align8_fwd_x2, grid, dim3(256), 0, st, a); break;
		// four and eight lanes per pair in one launch
		X_MIX_K(false) X_MIX_K(true)
		default: return hipErrorInvalidValue;          // (a description x_choose does not make: no instance is built for it)
	}
	if(l.name) bsa_last_fwd_kernel = l.name;
	return hipGetLastError();
}
static hipError_t x_launch(const Align8Args &a, int pw, bool score, hipStream_t st){
	if(a.count == 0) return hipSuccess;
	const XLaunch l = x_choose(a, pw, score, bsa_cus());
	return l.form == X_NONE ? hipErrorInvalidValue : x_run(l, a, st);
}
// Called once per chunk; chunks of one run may choose differently, and bsa_last_fwd_kernel is left by the last one that names its launch
hipError_t bsa_launch_align8_fwd_x(const Align8Args &a, int pw, hipStream_t st){ return x_launch(a, pw, false, st); }
// BSA_MODE_SCORE_ONLY (bsa_api.hip): the SCORE forms of the one-piece and linear kernels at bandwidth 64, 128 and 256, each pair leaving its record (bsa_score_rec_bytes)
hipError_t bsa_launch_align8_fwd_x_score(const Align8Args &a, int pw, hipStream_t st){ return x_launch(a, pw, true, st); }

// The row target that x_forward_abs uses for rows a[n] of pairs (tlen[n], qlen[n]), a[n] < tlen[n], for tests of x_rt_double's proof; needs no device.  The state is
// taken by division at row a - stride * min(steps, a / stride) and stepped from there to row a (steps = 0: the division alone; the kernels step by L = 4 or 8 rows).
// value[n]: the target; fallback[n]: 1 where the row asks the double expression (a qlen mod tlen = 0, or a pair outside the bound of the proof: x_rt_wide).
// Returns 0, or -1 for an argument outside that.
extern "C" int bsa_align8_row_target_internal(const uint32_t *a, const uint32_t *tlen, const uint32_t *qlen, size_t n, uint32_t stride, uint32_t steps, int32_t *value, uint8_t *fallback){
	if(!a || !tlen || !qlen || !value || !fallback || (steps != 0u && stride == 0u)) return -1;
	for(size_t j = 0; j < n; j++){
		const uint32_t t = tlen[j], q = qlen[j];
		if(t == 0u || a[j] >= t) return -1;
		if(x_rt_wide(t, q)){ fallback[j] = 1; value[j] = x_rt_double(a[j], t, q); continue; }          // (every renewal: the state is never read)
		const uint32_t back = steps ? std::min(steps, a[j] / stride) : 0u;
		XRowTgt s = x_rt_at(a[j] - back * stride, t, q);
		if(back){
			const XRowTgt d = x_rt_at(stride, t, q);
			x_rt_back(s, d, t);          // as the kernel starts: one step behind
			for(uint32_t m = 0; m <= back; m++){
				x_rt_step(s, d, t);
				// a row on the way that divides evenly hands its state on through the double expression, as in the kernel
				if(s.r == 0u && m < back) x_rt_set(s, (uint32_t)x_rt_double(a[j] - (back - m) * stride, t, q), t);
			}
		}
		fallback[j] = s.r == 0u;
		value[j] = s.r == 0u ? x_rt_double(a[j], t, q) : (int32_t)s.k;
	}
	return 0;
}
