// chaindp_twin.hip -- the chain DP kernel for ordinary long-read units: TWO units per wave64, one per 32-lane half.
//
// Why (measured on MI355X, tools/issue_calib.hip -> profiles/r02_issue_calib.json): the one-unit-per-wave kernel
// (chaindp_kernels.hip) spends ~29 scalar and ~31 vector instructions per anchor.  The scalar unit is shared by the
// CU's four SIMDs and issues ONE instruction per cycle per CU, so 29 of them cost each SIMD ~125 of its 140 cycles per
// anchor; vector instructions that read an SGPR, have three register sources or use DPP issue at half rate (4.2
// cycles instead of 2.4).  And the scan of an ava-ont anchor ends (max_skip + 1 marked predecessors, chain.c:277-279)
// within 32 predecessors 99.99 % of the time (map-ont: 71 %, within 48: 99.9 %), so half of a 64-lane pass is wasted.
// Hence: chunks of 32 predecessors, two independent units side by side in one wave, and everything that is uniform
// per unit kept in VECTOR registers (replicated over the half's lanes) and updated by plain two-operand VALU
// instructions; the scalar unit only combines 64-bit lane masks (both halves at once) and branches.
//
// What it computes is exactly run_unit_fast of chaindp_kernels.hip (reference chain.c:246-284 for reads with one
// segment, not cDNA, bw <= 511, every q_span > 0), with the same four derivations on 32-lane chunks.  Units it
// does not take -- general-variant reads, and any unit whose scan needs a predecessor older than its LDS ring (64
// anchors) -- are appended to a leftover list and run by k_chain_units afterwards, from scratch.
//
// Round 3: a half's anchors enter and leave in tiles of 64, and the per-tile service (next tile in, finished tile's f/p/v out,
// unit switch) is done by ALL 64 lanes of the wave for one half at a time -- it was 32 anchors by the half's own 32 lanes with the
// other half idle, a third of every wave's time and 30 % of its vector instructions.  Scores are kept minus one inside the kernel
// (the PF ring holds f - 1, the current anchor's floor is q_span - 1; chain.c:251,274 compare the same way when both sides are
// shifted), so that a pass needs q_span - 1 only; reads with a zero q_span go to k_chain_units.
//
// LDS per wave (dynamic segment, starts at byte 0; h = half).  Two layouts (TwLayout): one cost table per wave, for batches whose
// units all have one table key, and one per half, for the others:
//   XY  [128 slots][2 halves] 8 B   x.lo+1, qpos+1 of anchor (slot = i & 127), written a whole tile at a time; with one table a pass
//                                   reads its own anchor from here too (the current tile is in the ring)
//   PF  [ 64 slots][2 halves] 8 B   4*p (unit-relative, -4 = none), f - 1 of anchor (slot = i & 63)
//   V   [ 64 slots][2 halves] 4 B   v | "emitted at its own step" << 31
//   XQ  [2 halves][64] 8 B          two tables only: the current tile's anchors as a pass wants them, x.lo, qpos
//   LUT [1 or 2][512] int8          the table of 1 - cost (reads whose costs do not fit a byte go to k_chain_units)
//   ST  [2 halves] 56 B             the half's cold state (TwinCold) and what a scan carries into its second chunk
//   MK  [2 halves][65] 4 B          marks by distance: word d-1 holds the scan tag of the anchor d behind; word 64 = sink
//   SP  128 B                       q_span - 1 of the current tile's anchors: one table, byte 2 (i & 63) + h (its XY address / 8);
//                                   two tables, [h][entry] (its XQ address / 8 + const)
//   KEY [2 halves] 4 B              which read's table the LUT holds (reads with the same avg_qspan share it; one word per table)
// 4864 bytes with one table, 6400 with two.  LDS is handed out in pieces of 1280 bytes on this chip (tools/lds_occupancy_probe.hip
// measures how many workgroups a CU holds; the occupancy API does not know): 5120 bytes leave 32 workgroups per CU (eight waves per
// SIMD), 6400 bytes 25 (the two-table layout runs 24: six waves per SIMD, whose registers keep a tile prefetch).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "chaindp_kernels.h"
#include "chaindp_wave.h"
#include "chaindp_lanes.h"

namespace chaindp {

#define TW_XY 0u
#define TW_PF 2048u                     // (tw_st64_pf_lanes has it as the DS offset: static_assert there)
#define TW_V 3072u
#define TW_LUT_BYTES 512u                // one table (bw + 1 <= 512 entries)
#define TW_ST_HALF 56u
#define TW_MK_HALF 260u
// XY, PF and V first (XY and PF at offsets 0 and 2048: the bank pattern of a pass' two ring reads), then:
//   one table per wave:  LUT [512], ST, MK, SP [64 slots][2 halves], KEY                     4864 bytes
//   one table per half:  XQ [2][64] 8 B, LUT [2][512], ST, MK, SP [2][64], KEY                6400 bytes (the layout before the one-table
//                        one existed: the pass reads its anchor from XQ, x.lo and qpos as they are)
template <bool ONE_LUT> struct TwLayout {
	static constexpr bool HAS_XQ = !ONE_LUT;
	static constexpr uint32_t XQ = 3584u, XQ_HALF = 512u;                    // (two tables only)
	static constexpr uint32_t LUT = ONE_LUT ? 3584u : XQ + 2u * XQ_HALF;
	static constexpr uint32_t LUT_HALF = ONE_LUT ? 0u : TW_LUT_BYTES;        // the second half's table
	static constexpr uint32_t ST = LUT + (ONE_LUT ? 1u : 2u) * TW_LUT_BYTES;
	static constexpr uint32_t MK = ST + 2u * TW_ST_HALF;
	static constexpr uint32_t SP = MK + 2u * TW_MK_HALF;
	static constexpr uint32_t SP_HALF = ONE_LUT ? 0u : 64u;                 // one table: byte 2 (i & 63) + h; two: [h][entry of XQ]
	static constexpr uint32_t SP_OF_XQ = SP - XQ / 8u;                        // (two tables) SP address = (XQ address >> 3) + this
	static constexpr uint32_t KEY = SP + 128u;                                // [2] 4 B: key of the cost table (UnitAux::lutkey); one table: word 0
	static constexpr uint32_t KEY_HALF = ONE_LUT ? 0u : 4u;
	static constexpr uint32_t BYTES = KEY + 8u;
	static_assert(ST % 8u == 0u && MK % 4u == 0u && KEY % 4u == 0u, "cold state is read as 64-bit words, marks and keys as 32-bit");
};
static_assert(TwLayout<true>::BYTES == 4864u && TwLayout<true>::BYTES <= 5120u, "one table: 32 workgroups per CU");
static_assert(TwLayout<false>::BYTES == 6400u, "two tables: 24 workgroups per CU");
// waves per SIMD each instantiation is compiled for (VGPRs <= 512 / waves, no scratch: tests/test_twin_resources.py).  One table:
// the LDS allows 32 workgroups per CU, and the registers eight waves per SIMD (seven for max_dist_y < max_dist_x, which carries one more
// per-lane constant, c_dqoff).  Two tables: the LDS allows 24 workgroups per CU, six waves per SIMD, and the registers at six waves keep
// the tile prefetch (PF in the kernel).
template <bool SAMEGAP, bool ONE_LUT> struct TwWaves { static constexpr int N = !ONE_LUT ? 6 : SAMEGAP ? 8 : 7; };
#define TW_TILE 64                      // anchors a half takes in / flushes at a time
#define TW_RING 64                      // predecessors a scan can reach in this kernel (two chunks of 32)
#define TW_QCH 8                        // units a half takes from the queue at a time

// exclusive prefix max over the 32 lanes of each half, floor 0 (scores are >= 0 where they matter): inclusive scan
// inside the 16-lane rows (4 DPP steps), one-lane shift inside the rows, and for the upper row of each half the lower
// row's total (row_bcast:15 into rows 1 and 3; harmless for the lanes that already hold a larger prefix)
__device__ __forceinline__ int tw_excl_max32(int v)
{
	v = max(v, __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(1), 0xf, 0xf, true));
	v = max(v, __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(2), 0xf, 0xf, true));
	v = max(v, __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(4), 0xf, 0xf, true));
	v = max(v, __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(8), 0xf, 0xf, true));
	int e = __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(1), 0xf, 0xf, true);
#if defined(__HIP_DEVICE_COMPILE__)
	// rows 1 and 3: e = max(e, lane 15 of the row below); rows 0 and 2 keep e (one DPP instruction; the two s_nop cover the
	// VALU-write -> DPP-read hazard on v and e whatever the scheduler puts in front)
	asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(e) : "v"(v));
#endif
	return e;
}
// inclusive prefix min over the 32 lanes of each half (general walk)
__device__ __forceinline__ int tw_incl_min32(int v)
{
	v = min(v, dpp_or_old<DPP_ROW_SHR(1), 0xf>(INT_MAX, v));
	v = min(v, dpp_or_old<DPP_ROW_SHR(2), 0xf>(INT_MAX, v));
	v = min(v, dpp_or_old<DPP_ROW_SHR(4), 0xf>(INT_MAX, v));
	v = min(v, dpp_or_old<DPP_ROW_SHR(8), 0xf>(INT_MAX, v));
	v = min(v, dpp_or_old<DPP_ROW_BCAST15, 0xa>(INT_MAX, v));
	return v;
}

// bits of the 64-bit lane mask m below this lane, counted inside the lane's own half
__device__ __forceinline__ int tw_below_in_half(uint64_t m, bool hi_half)
{
	const int lo = (int)__builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u);
	const int hi = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), 0u);
	return hi_half ? hi : lo;
}

// per half: mask of all 32 lanes if any bit of m is set in that half (four scalar instructions; written out because the
// compiler turns the C form into 64-bit vector compares)
__device__ __forceinline__ uint64_t tw_smear_halves(uint64_t m)
{
	uint32_t lo = 0, hi = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("s_cmp_lg_u32 %2, 0\n\ts_cselect_b32 %0, -1, 0\n\ts_cmp_lg_u32 %3, 0\n\ts_cselect_b32 %1, -1, 0"
	    : "=&s"(lo), "=&s"(hi) : "s"(TW_UNI((uint32_t)m)), "s"(TW_UNI((uint32_t)(m >> 32))) : "scc");
#endif
	return (uint64_t)hi << 32 | lo;
}

// per half: the highest set bit of m alone, or the half's lane 0 if m has none there (s_flbit gives -1 for 0, and a
// shift only uses the low five bits of its count: 0x80000000 >> 31 = lane 0)
__device__ __forceinline__ uint64_t tw_last_or_lane0(uint64_t m)
{
	uint32_t lo = 0, hi = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("s_flbit_i32_b32 %0, %2\n\ts_flbit_i32_b32 %1, %3\n\ts_lshr_b32 %0, 0x80000000, %0\n\ts_lshr_b32 %1, 0x80000000, %1"
	    : "=&s"(lo), "=&s"(hi) : "s"(TW_UNI((uint32_t)m)), "s"(TW_UNI((uint32_t)(m >> 32))));
#endif
	return (uint64_t)hi << 32 | lo;
}

// nonzero iff m has a set bit in BOTH halves (three scalar instructions with the compare the caller adds)
__device__ __forceinline__ uint32_t tw_both_halves(uint64_t m)
{
	uint32_t t = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("s_cmp_lg_u32 %1, 0\n\ts_cselect_b32 %0, %2, 0" : "=s"(t) : "s"(TW_UNI((uint32_t)m)), "s"(TW_UNI((uint32_t)(m >> 32))) : "scc");
#endif
	return t;
}

// per half: bits of m below the half's lowest set bit of b (all of m where b has none: (b - 1) & ~b is all ones for b = 0).  The
// halves as scalar words of their own: from "b's high word is not zero" the compiler makes a 64-bit vector compare.
__device__ __forceinline__ uint64_t tw_below_first(uint64_t m, uint64_t b)
{
	const uint32_t blo = TW_UNI((uint32_t)b), bhi = TW_UNI((uint32_t)(b >> 32));
	const uint32_t klo = (blo - 1u) & ~blo, khi = (bhi - 1u) & ~bhi;
	return m & ((uint64_t)khi << 32 | klo);
}

// a lane's byte offset for TW_AT, pinned to the block that uses it: instruction selection works a block at a time and takes the
// scalar base + 32-bit vector offset form only where it sees the offset's zero-extension, which the compiler otherwise hoists
__device__ __forceinline__ uint32_t tw_here(uint32_t x) { TW_VREG(x); return x; }
#define TW_HI31 0x8000000080000000ull

// per half: the bits of a above the lowest set bit of b, for disjoint a and b (b's lowest bit and all above it are set in -b; none
// where b has no bit)
__device__ __forceinline__ uint64_t tw_above_first(uint64_t a, uint64_t b)
{
	uint32_t lo = 0, hi = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("s_sub_i32 %0, 0, %2\n\ts_sub_i32 %1, 0, %3" : "=&s"(lo), "=&s"(hi) : "s"(TW_UNI((uint32_t)b)), "s"(TW_UNI((uint32_t)(b >> 32))) : "scc");
#endif
	return a & ((uint64_t)hi << 32 | lo);
}

// The one exit test of the fast loop: k, or 0 where a half has an A lane above its lowest B lane (interleaved).  The s_and_b64 of
// tw_above_first sets SCC, and the s_cselect reads it at once; `ia` keeps the interleave mask for the block behind the exit.
__device__ __forceinline__ uint32_t tw_exit_key(uint64_t a, uint64_t b, uint32_t k, uint64_t &ia)
{
#if defined(__HIP_DEVICE_COMPILE__)
	uint32_t lo, hi;
	asm("s_sub_i32 %0, 0, %2\n\ts_sub_i32 %1, 0, %3" : "=&s"(lo), "=&s"(hi) : "s"(TW_UNI((uint32_t)b)), "s"(TW_UNI((uint32_t)(b >> 32))) : "scc");
	asm("s_and_b64 %1, %2, %3\n\ts_cselect_b32 %0, 0, %0" : "+s"(k), "=&s"(ia) : "s"(a), "s"((uint64_t)hi << 32 | lo) : "scc");
#else
	ia = tw_above_first(a, b); k = ia ? 0u : k;
#endif
	return k;
}

// ds_write_b64 of (x, y) to the PF ring (byte a + TW_PF) by the lanes of m alone, exec set by hand: as a branch on m it would be the one
// divergent branch of the fast loop, and the compiler's structurizer would then merge the loop's uniform exits into flag registers
__device__ __forceinline__ void tw_st64_pf_lanes(uint64_t m, uint32_t a, uint32_t x, uint32_t y)
{
#if defined(__HIP_DEVICE_COMPILE__)
	tw_u32x2 t; t.x = x; t.y = y;
	uint64_t saved;
	asm volatile("s_and_saveexec_b64 %0, %1\n\tds_write_b64 %2, %3 offset:2048\n\ts_mov_b64 exec, %0"
	             : "=&s"(saved) : "s"(m), "v"(a), "v"(t) : "memory", "scc");
#endif
}
static_assert(TW_PF == 2048u, "tw_st64_pf_lanes writes the PF ring at DS offset 2048");


struct TwinArgs {
	Params par;
	const int64_t *off;
	const ulonglong2 *a;
	const unsigned long long *sumq;
	const uint16_t *lut;
	int lut_stride;
	const Unit *units;
	const UnitAux *aux;               // beside units[]: rel0, table key, "general" flag
	const unsigned long long *counters;
	int32_t *f, *p, *v;
	int32_t *first_child;
	uint8_t *flags;
	Unit *left;                       // leftover list for k_chain_units
	unsigned int *left_cnt;
	unsigned int *queue;              // eight grab counters, 64 words apart (the halves' first grabs are dealt statically: they start behind them)
	const unsigned int *key_range;    // [0] min, [1] max of the units' table keys (prepass)
	unsigned int *route;              // 2: the one-table layout took the batch; 3: the two-table layout did (1: retired, nothing writes it)
	int two_tables;                   // test switch: 1 keeps a one-key batch on the two-table layout
	int force_left;                   // test switch: 1 hand every unit over untouched, 2 hand every unit over after its first tile (resumed there)
	int64_t total;                    // anchors of the batch
	unsigned long long *stamp;        // diagnostic run (CHAINDP_TWIN_STAMP): per block 8 counters; nullptr otherwise
};

// the state of a half that only the service path needs lives in LDS (ST + 56 h), so that the pass loop carries
// nothing but what a pass reads
struct TwinCold {                     // 40 bytes at ST + 56 h (8-byte aligned: read and written as 64-bit words)
	int64_t next;                     // next unit of this half (grid-stride over pairs)
	int64_t base;                     // global index of the unit's first anchor
	uint32_t params_ok, spare;        // the launch's parameters are this kernel's (written once, when the kernel starts)
	int32_t rel0, room, read, tile0;  // unit start relative to its read; anchors the unit may have; its read; current tile's first anchor
};

// what a pass reads and writes, per half, replicated over the half's lanes
struct TwinHot {
	uint32_t S;                       // 16 * jtop + 8h, jtop = i - 1 - 32c: ring offset of lane 0's predecessor
	uint32_t m4;                      // 4 * (i - 1) + mark base: mark distance base and the scan's tag
	uint32_t pc;                      // (two tables) XQ entry of the current anchor
	uint32_t pend;                    // one table: m4 of the tile's last anchor, exhausted once m4 >= pend (0: no tile);
	                                  // two tables: end of the tile's XQ entries, exhausted once pc >= pend
};
// What a scan carries into its second chunk (one scan in thirty) is not worth registers: it sits behind the half's cold state
// (ST + 56 h + 40): 4 * max_j (-4: none), the running max of the scan (chain.c:274) minus one, n_skip, and the second chunks
// the unit has needed so far.
#define TW_CARRY 40u

// in-kernel stamps (where a wave's time goes): compiled in only with -DCHAINDP_TWIN_STAMPS, because even switched off they cost
// registers the kernel does not have to spare (make -C csrc stamps; then run with CHAINDP_TWIN_STAMP=1)
#ifdef CHAINDP_TWIN_STAMPS
#define TW_STAMP(...) __VA_ARGS__
#else
#define TW_STAMP(...)
#endif
// two sets of stamps inside service(), one per build (-DCHAINDP_TWIN_STAMPS=1: flush and unit switch; =2: the rest): both do not fit
#if defined(CHAINDP_TWIN_STAMPS) && CHAINDP_TWIN_STAMPS == 2
#define TW_STAMP_A(...)
#define TW_STAMP_B(...) __VA_ARGS__
#elif defined(CHAINDP_TWIN_STAMPS) && CHAINDP_TWIN_STAMPS == 1
#define TW_STAMP_A(...) __VA_ARGS__
#define TW_STAMP_B(...)
#else
#define TW_STAMP_A(...)
#define TW_STAMP_B(...)
#endif
// build 3: inside the unit switch (head: until the unit's record is there; take: until its first tile is there; tail: table, ring
// initialisation and the tile taken; n_unit counts the first tiles that were requested ahead)
#if defined(CHAINDP_TWIN_STAMPS) && CHAINDP_TWIN_STAMPS == 3
#define TW_STAMP_C(...) __VA_ARGS__
#else
#define TW_STAMP_C(...)
#endif
#define TW_NOW() __builtin_amdgcn_s_memtime()

// ONE_LUT: the layout with one cost table per wave (TwLayout<true>), for batches whose units all have the same table key; the other
// instantiation keeps one table per half.  Both are launched; the first that finds the batch to be its own takes it (g.route).
template <bool SAMEGAP, bool ONE_LUT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TwWaves<SAMEGAP, ONE_LUT>::N, TwWaves<SAMEGAP, ONE_LUT>::N))) void k_chain_twin(TwinArgs g)
{
	using L = TwLayout<ONE_LUT>;
	const int lane = threadIdx.x;
	const bool hi_half = lane >= 32;
	const int h = lane >> 5, hl = lane & 31;

	// ---- per-lane constants (vector registers on purpose, see TW_VREG)
	uint32_t L16 = ((uint32_t)hl + 1u) << 4;                        // 16 (k + 1): lane k's predecessor is anchor i - 1 - k
	const uint32_t mkbase = L::MK + TW_MK_HALF * (uint32_t)h;      // this half's mark words
	const uint32_t curbase = L::XQ + L::XQ_HALF * (uint32_t)h;     // (two tables) this half's XQ entries
	uint32_t c_mkbase = mkbase;
	uint32_t c_far = mkbase + 256u;                                // its sink word
	uint32_t c_own = mkbase + ((uint32_t)hl << 2);                 // lane's own mark word in chunk 0
	uint32_t c_lut = ONE_LUT ? 0u : L::LUT + L::LUT_HALF * (uint32_t)h;   // the half's table base (one table: in the DS offset, LUT_OFF)
	uint32_t c_8h = (uint32_t)h << 3;
	uint32_t c_M = (uint32_t)g.par.max_dist_x;
	uint32_t c_bw = (uint32_t)g.par.bw;
	uint32_t c_cbw = c_M - 1u > c_bw ? c_M - 1u - c_bw : 0u;
	const uint32_t mdq = (uint32_t)(g.par.max_dist_x < g.par.max_dist_y ? g.par.max_dist_x : g.par.max_dist_y);
	uint32_t c_dqoff = c_M - mdq;
	int c_ms = g.par.max_skip;
	int c_min = INT_MIN;
	int c_Mout = hl == 31 ? g.par.max_dist_x : INT_MAX;            // (two tables) window test that only the half's last lane can fail
	uint32_t c_bwl = c_bw + c_lut;                                 // table address of the last entry (- LUT_OFF)
	uint32_t c_cbwl = c_cbw - c_lut;                               // (dd + c_lut) + this = dd + c_cbw
	constexpr uint32_t LUT_OFF = ONE_LUT ? L::LUT : 0u;
	// (one table: c_M and c_ms stay scalar -- only compares read them -- for the registers of the eighth wave, and there is no c_Mout:
	// the fast pass' window test is off its common path, where a compare with c_M masked to lane 31 does)
	TW_VREG(L16); TW_VREG(c_far); TW_VREG(c_own);
	if (!ONE_LUT) { TW_VREG(c_M); TW_VREG(c_ms); TW_VREG(c_Mout); }
	if (!ONE_LUT) TW_VREG(c_lut);
	if (!SAMEGAP) TW_VREG(c_dqoff);
	TW_VREG(c_min); TW_VREG(c_bwl); TW_VREG(c_cbwl);

	// (uniform) which layout takes the batch: the one-table layout takes batches whose units share one table key and writes 2, which
	// the two-table layout, launched behind it, then finds.  (route == 1u: a retired value, written by the kernel with four units per
	// wave that was launched in front of this one; nothing writes it any more.  The compare stays until a change that measures takes
	// it out: this kernel sits at its register edge.)
	const uint32_t route = *g.route;
	if (ONE_LUT ? route == 1u || g.key_range[0] != g.key_range[1] || g.two_tables : route == 1u || route == 2u) return;
	const uint32_t n_units = (uint32_t)g.counters[0];                // (32 bits: one scalar register through the pass loops)
	// Units of a few thousand anchors (map-ont shape) are few and each is a long serial chain: two of them side by side gain
	// nothing and their scans need the second chunk for one anchor in three.  Such batches go to k_chain_units as a whole.
	const int64_t n_single = (int64_t)(g.counters[0] >> 32);
	const bool short_units = (g.total - n_single) <= 512 * (int64_t)n_units;
	if (!short_units) {                                            // (uniform: every block leaves; one of them says so)
		if (blockIdx.x == 0 && lane == 0) *g.left_cnt = 0xffffffffu;
		return;
	}
	if (blockIdx.x == 0 && lane == 0) *g.route = ONE_LUT ? 2u : 3u;
	// the parameters are this kernel's (else every unit is handed over).  The kernel's 32-bit differences (and the signed window
	// test) are exact while 129 * (max_dist_x + 1) < 2^31.  Decided here, once, from the kernel arguments, and kept in the halves'
	// cold state: service() finds it there where it picks a unit up.
	const bool params_ok = g.lut != nullptr && !g.par.is_cdna && g.par.max_dist_x >= 1 && g.par.max_dist_y >= 0 && g.par.n_segs <= 1 &&
	                       ((uint64_t)(int64_t)g.par.max_dist_x + 1) * 129ull < (1ull << 31) && g.par.bw + 1 <= (int)TW_LUT_BYTES && g.force_left != 1;

	TwinHot u;
	u.S = 0; u.m4 = 0; u.pc = L::HAS_XQ ? curbase : 0u; u.pend = u.pc;
	uint64_t live_m = ~0ull;                                       // halves that still have (or may get) work
	uint64_t contm = 0;                                            // halves that are in their second (= last) chunk
	const uint32_t st_addr = L::ST + TW_ST_HALF * (uint32_t)h;
#define TW_COLD (*TW_LDS(TwinCold, st_addr))
	// The unit queue.  Eight counters, a cache line apart (one same-address atomic takes ~7.5 ns: 133 M a second for the whole chip
	// on ONE counter), workgroup b on counter b mod 8.  A half's p-th grab of its counter k is the chunk of TW_QCH units number
	// 8 p + k while the list's long front lasts (units [0, U1)), and ONE unit -- number 8 (p - G1k) + k of [U1, n_units) -- for the
	// last sixteen units per half: the list is longest first, every half works on units of the same length at any time, and the
	// halves run out of work within one grab of each other -- eight units of 140 anchors were 0.4 ms, 0.2 ms of idle tail on average
	// behind a 3 ms kernel.  (Smaller grabs all along cost more than they save: same-address atomics.)
#ifndef TW_END_UNITS
#define TW_END_UNITS 16u                // units per half that are dealt in small pieces at the end of the list
#define TW_PIECE 1u                     // ... this many at a time (measured on the 76 M-anchor shard: 16 / 1: 2.86 ms, 16 / 2: 2.88, 24 / 1: 2.88, 32 / 2: 2.90, 8 / 2: 2.95; one counter, 8 at a time all along: 3.04)
#endif
	// (the queue's geometry stays worked out here, three scalar registers kept for the grabs: worked out at each grab instead, the
	// register allocation of every instantiation tips into VGPR spills)
	const uint32_t xcd = blockIdx.x & 7u;
	const uint64_t end_units = (uint64_t)TW_END_UNITS * 2u * gridDim.x;      // TW_END_UNITS per half
	const uint32_t U1 = (end_units >> 32) == 0 && n_units > (uint32_t)end_units ? (n_units - (uint32_t)end_units) & ~(8u * TW_QCH - 1u) : 0u;
	const uint32_t G1k = U1 / (8u * TW_QCH);                             // grabs of whole chunks per counter
	auto grab = [&](uint32_t p, uint32_t &nx, uint32_t &ne) {
		if (p < G1k) { nx = (8u * p + xcd) * TW_QCH; ne = nx + TW_QCH; }
		else { nx = U1 + TW_PIECE * (8u * (p - G1k) + xcd); ne = nx + TW_PIECE; }
	};
	if (hl == 0) {
		uint32_t nx, ne;
		grab(((blockIdx.x >> 3) << 1) | (uint32_t)h, nx, ne);                            // the half's first grab: dealt statically
		tw_st64(st_addr, nx, ne); tw_st64(st_addr + 8u, 0u, 0u);                         // TwinCold: next (low word: next unit, high word: end of the chunk), base
		tw_st64(st_addr + 16u, params_ok ? 1u : 0u, 0u); tw_st64(st_addr + 24u, 0u, 0u);   // params_ok, rel0, room
		tw_st64(st_addr + 32u, 0u, (uint32_t)-TW_TILE);                                 // read, tile0
		tw_st64(st_addr + TW_CARRY, 0xfffffffcu, 0u); tw_st64(st_addr + TW_CARRY + 8u, 0u, 0u);   // carry, second chunks so far
		tw_st32(L::KEY + 4u * (uint32_t)h, -1);                                         // no table yet (an avg_qspan is never a NaN)
	}
	wave_mem_fence();

	// The two-table layout runs at six waves per SIMD (its LDS allows 24 workgroups per CU), which leaves the registers for a tile
	// prefetch: each half's NEXT tile is requested a tile ahead into registers.  The one-table layout gives those eight registers up
	// for the seventh and eighth wave and loads a tile when it takes it.
	constexpr bool PF = !ONE_LUT;
	uint64_t nx0_x = 0, nx0_y = 0, nx1_x = 0, nx1_y = 0;           // (PF) each half's next tile, one anchor per lane; zeros where the unit has none
	int32_t pfu0 = -1, pfu1 = -1;                                  // (PF) ... or, when the unit ends with the current tile, the first tile of the half's
	                                                               // next unit: its first anchor's global index (wave-uniform), -1 = no such tile

	TW_STAMP(unsigned long long st_t0 = 0; unsigned int st_service = 0, st_n_service = 0, st_n_fast = 0, st_flush = 0, st_unit = 0, st_n_unit = 0, st_head = 0, st_take = 0, st_tail = 0, st_rounds = 0, st_n_flush = 0;)   // (32-bit sums: a wave's ticks fit, and the build has no registers to spare)

	// One service round for the halves in `svc`, whose tile is exhausted (or which have no unit yet).  One half at a time, by ALL 64
	// lanes of the wave (a tile is 64 anchors, one per lane): everything that is per half (the cold state, the unit being picked,
	// loop conditions) is wave-uniform and lives in scalar registers, loads by scalar address go through the scalar cache, and the
	// loops are scalar branches; what goes back into the half's hot state is selected into its 32 lanes (TW_SEL by `hm`).  Order:
	// the unit's next tile is loaded and taken first -- before the finished tile's f/p/v are stored, so that nothing waits for those
	// stores --, then the finished tile is flushed; a half whose unit is over picks its next unit and loads that one's first tile.
	// Once per 64 anchors and half.  Where the layout prefetches (PF), the next tile and a successor unit's first tile are already in
	// registers, requested a tile of passes ago.
	auto service = [&](uint64_t svc) {
		const auto kp = TW_KARGS(g);                                     // the arguments, read where they are used (chaindp_lanes.h)
		// the lane number, and what the service derives from it (ring and table addresses, byte offsets into a tile of the global
		// arrays: 4, 16 and 1 bytes an anchor), from a value the compiler cannot trace: it would work them out once and keep them in
		// vector registers through the pass loops, which have none to spare
		uint32_t ln = (uint32_t)threadIdx.x;
		TW_VREG(ln);
		const int lane = (int)ln;                                        // (hides the kernel's `lane`)
#if defined(__HIP_DEVICE_COMPILE__)
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // (whatever is outstanding was issued a tile of passes ago: no wait in practice)
#endif
		wave_mem_fence();
		uint64_t retired = 0;
		for (int hs = 0; hs < 2; ++hs) {
			if (((svc >> (32 * hs)) & 1ull) == 0) continue;
			TW_STAMP_B(const unsigned long long th0 = g.stamp ? TW_NOW() : 0;)
			const uint64_t hm = hs ? 0xffffffff00000000ull : 0x00000000ffffffffull;   // the lanes that carry this half's hot state
			const uint32_t sa = L::ST + TW_ST_HALF * (uint32_t)hs, keya = L::KEY + L::KEY_HALF * (uint32_t)hs;
			const uint32_t mkb = L::MK + TW_MK_HALF * (uint32_t)hs, lutb = L::LUT + L::LUT_HALF * (uint32_t)hs;
			const uint32_t curb = L::XQ + L::XQ_HALF * (uint32_t)hs, spb = L::SP + L::SP_HALF * (uint32_t)hs;
			const tw_u32x2 cw0 = tw_ld64(sa), cw1 = tw_ld64(sa + 8u), cw2 = tw_ld64(sa + 16u), cw3 = tw_ld64(sa + 24u), cw4 = tw_ld64(sa + 32u);
			int64_t c_next = (int64_t)((uint64_t)TW_UNI(cw0.y) << 32 | TW_UNI(cw0.x));
			int64_t c_base = (int64_t)((uint64_t)TW_UNI(cw1.y) << 32 | TW_UNI(cw1.x));
			const bool params_ok = TW_UNI(cw2.x) != 0;                        // (decided when the kernel started)
			int c_rel0 = (int)TW_UNI(cw3.x), c_room = (int)TW_UNI(cw3.y), c_read = (int)TW_UNI(cw4.x), c_tile0 = (int)TW_UNI(cw4.y);
			// anchors of the tile a half holds (the one just scored, or the one taken in this call)
			auto tile_cnt = [&]() -> int {
				const uint32_t pe = TW_UNI(__builtin_amdgcn_readlane((int)u.pend, 32 * hs));
				if constexpr (L::HAS_XQ) return (int)((pe - curb) >> 3);
				else return pe < mkb ? 0 : (int)((pe - mkb) >> 2) + 1 - c_tile0;
			};
			const int cnt_prev = tile_cnt();
			const int slow_h = (int)TW_UNI((uint32_t)tw_ld32(sa + TW_CARRY + 12u));
			const uint32_t cur_key = TW_UNI((uint32_t)tw_ld32(keya));
			const int tile_prev = c_tile0, rel0_prev = c_rel0;
			const int64_t base_prev = c_base;
			bool live = true;
			// The half's next unit (PF: and the one after it), in case this call needs them -- the unit ends here, or (PF) with the tile
			// taken now, and its successor's first tile is then requested a tile ahead: records and UnitAux through the scalar cache,
			// issued before the work below and read after it.
			const uint32_t nx0 = (uint32_t)c_next, ne0 = (uint32_t)((uint64_t)c_next >> 32);
			tw_u32x4 rec0 = {0u, 0u, 0u, 0u}, aux0 = {0u, 0u, 0u, 0u}, rec1 = {0u, 0u, 0u, 0u};
			const bool rec0_ok = nx0 < ne0 && nx0 < n_units;       // (whenever they are known: a unit can end before its bound says so)
			const bool rec1_ok = PF && rec0_ok && nx0 + 1u < ne0 && nx0 + 1u < n_units;     // (rec0_ok: nx0 + 1 <= n_units, no wrap)
			if (rec0_ok) { rec0 = *TW_CONST(tw_u32x4, kp->units + nx0); aux0 = *TW_CONST(tw_u32x4, kp->aux + nx0); }
			if (rec1_ok) rec1 = *TW_CONST(tw_u32x4, kp->units + nx0 + 1u);

			// takes a tile's anchors (one per lane, raw mm128_t) into the half's LDS: XY ring (the anchors as predecessors and as the
			// current anchor), SP.  The unit's length is exact (k_emit_units: the first gap > max_dist_x behind its start, chain.c:252,
			// or its read's end), so no gap is tested here.  Returns the anchors the tile holds (0: there are none left).
			auto take_tile = [&](const uint64_t an_x, const uint64_t an_y) -> int {
				const int i_lane = c_tile0 + lane;
				const int cnt = c_room - c_tile0 < TW_TILE ? c_room - c_tile0 : TW_TILE;
				if constexpr (L::HAS_XQ) { u.pc = TW_SEL(hm, curb, u.pc); u.pend = TW_SEL(hm, curb + ((uint32_t)cnt << 3), u.pend); }
				else u.pend = TW_SEL(hm, mkb + ((uint32_t)(c_tile0 + cnt - 1) << 2), u.pend);
				if (cnt == 0) return 0;
				wave_mem_fence();
				if (lane < cnt) {
					const int sp = span_of_hi((uint32_t)(an_y >> 32));
					tw_st64((((uint32_t)i_lane & 127u) << 4 | (uint32_t)hs << 3) + TW_XY, (uint32_t)an_x + 1u, (uint32_t)an_y + 1u);
					if constexpr (L::HAS_XQ) {
						tw_st64(curb + ((uint32_t)lane << 3), (uint32_t)an_x, (uint32_t)an_y);
						tw_st8(spb + (uint32_t)lane, sp - 1);
					} else tw_st8((((uint32_t)i_lane & 63u) << 1 | (uint32_t)hs) + L::SP, sp - 1);
					// first_child[] starts at "none" for every anchor the kernel takes in: stored here, a whole tile of passes before the
					// tile's flush (or any later one) lowers it with atomics -- and service() waits for the wave's outstanding memory
					// operations when it starts, so those atomics come after this store in memory as well.  No batch-wide memset.
					TW_AT(int32_t, kp->first_child + (c_base + c_tile0), tw_here(ln << 2)) = NO_CHILD;
				}
				wave_mem_fence();
				if constexpr (PF) {
					// the tile after this one: the load is issued now and read at the half's next service, 64 anchors of work later
					if (cnt == TW_TILE && c_tile0 + TW_TILE < c_room) {        // (else: the unit ends with this tile; the registers are for its successor)
						uint64_t rx = 0, ry = 0;
						if (i_lane + TW_TILE < c_room) { const ulonglong2 t = TW_AT(const ulonglong2, kp->a + (c_base + c_tile0 + TW_TILE), tw_here(ln << 4)); rx = t.x; ry = t.y; }
						if (hs) { nx1_x = rx; nx1_y = ry; pfu1 = -1; } else { nx0_x = rx; nx0_y = ry; pfu0 = -1; }
					}
				}
				return cnt;
			};

			// ---- the unit goes on?
			bool goes_on = cnt_prev == TW_TILE && c_tile0 + TW_TILE < c_room;
			if (goes_on && (slow_h * 8 > c_tile0 + TW_TILE || kp->force_left == 2)) {
				// a unit that keeps needing second chunks (more than one anchor in eight) is cheaper in k_chain_units: hand the rest of
				// it over.  The tiles up to the one flushed below are done: k_chain_units goes on behind them (the count rides in the
				// high word of the start; force_left == 2 is the tests' way to send every unit down this road)
				if (lane == 0) {
					Unit un; un.start = (int64_t)((uint64_t)c_base | (uint64_t)(uint32_t)(c_tile0 + TW_TILE) << 32); un.read = c_read; un.len = c_room;
					kp->left[atomicAdd(kp->left_cnt, 1u)] = un;
				}
				goes_on = false;
			}
			// the unit's next tile: in registers since the last service (PF), else loaded now
			if (goes_on) {
				c_tile0 += TW_TILE;
				uint64_t nt_x = 0, nt_y = 0;
				if constexpr (PF) { nt_x = hs ? nx1_x : nx0_x; nt_y = hs ? nx1_y : nx0_y; }
				else if (c_tile0 + lane < c_room) { const ulonglong2 t = TW_AT(const ulonglong2, kp->a + (c_base + c_tile0), tw_here(ln << 4)); nt_x = t.x; nt_y = t.y; }
				// (never 0: the test above has seen the anchors.  The test stays: without it the compiler reshapes the loop below so
				// that its flags merge where an `if (lane == 0)` joins, takes them for per-lane values and moves the service's masks
				// into vector registers -- 64 VGPRs and scratch in every instantiation)
				if (take_tile(nt_x, nt_y) == 0) goes_on = false;
			}
			TW_STAMP_B(if (g.stamp) st_take += (unsigned int)(TW_NOW() - th0);)
			// ---- flush the finished tile
			TW_STAMP_A(const unsigned long long tf0 = g.stamp ? TW_NOW() : 0;)
			if (cnt_prev > 0) {
				const int i_lane = tile_prev + lane;                         // this lane's anchor of the finished tile
				const bool have = lane < cnt_prev;
				// the tile's place in the five output arrays: a scalar base each (64-bit scalar arithmetic) and one lane offset, 4 * lane
				// (flags: lane) -- relative to the tile, so that it fits 32 bits whatever the batch holds
				const int64_t g0 = base_prev + tile_prev;
				int32_t *const f0 = kp->f + g0, *const p0 = kp->p + g0, *const v0 = kp->v + g0;
				uint8_t *const fl0 = kp->flags + g0;
				// a predecessor is at most TW_RING anchors behind its anchor: first_child from TW_RING anchors before the tile
				int32_t *const fc0 = kp->first_child + (g0 - TW_RING);
				const int min_sc = kp->par.min_sc;
				int fi = 0, p4 = -4;
				if (have) {
					const tw_u32x2 pf = tw_ld64((((uint32_t)i_lane & 63u) << 4 | (uint32_t)hs << 3) + TW_PF);
					p4 = (int)pf.x; fi = (int)pf.y + 1;                      // (the ring holds f - 1)
				}
				const int pi = p4 >> 2;                                      // unit-relative predecessor, -1 = none
				int val = fi, ptr = have ? pi : -1;
				const bool ext = ptr >= 0 && ptr < tile_prev;                // predecessor in an earlier tile: its v is final, in the V ring
				int vext = 0;
				if (ext) {
					vext = tw_ld32((((uint32_t)ptr & 63u) << 3 | (uint32_t)hs << 2) + TW_V);
					val = max(val, vext & 0x7fffffff);
					ptr = -1;
				}
				const bool ext_self = ext && vext < 0;                       // (bit 31 of a V entry: the anchor was emitted at its own step)
				// v[i] = max(f[i], v[p[i]]) (chain.c:284) by pointer doubling over the tile: after r rounds val is the maximum of f over the
				// lane and its first 2^r - 1 in-tile ancestors (and the final v of an ancestor in an earlier tile), ptr the ancestor after those.
				// Lanes whose pointer has left the tile read themselves, so pv = val and pp = ptr there.  Two ways out.  No pointer is
				// inside the tile any more: at most six rounds.  And a round that would raise no lane's value: then val[ptr] <= val
				// wherever ptr is inside the tile, and v = val follows lane by lane in tile order (p[i] < i: v[ptr] = val[ptr] by
				// induction, so v = max(val, v[ptr]) = val).  Chains run up through a tile and f mostly grows along them, so this is
				// the first round in nearly every tile (profiles/r08_*): one ds_bpermute where there were twelve.
				if (__builtin_amdgcn_ballot_w64(ptr >= tile_prev) != 0) {
					int r = 0;
					do {
						TW_STAMP_A(if (g.stamp) ++st_rounds;)
						const int src = (ptr >= tile_prev ? ptr - tile_prev : lane) << 2;
						const int pv = __builtin_amdgcn_ds_bpermute(src, val);
						if (__builtin_amdgcn_ballot_w64(pv > val) == 0) break;
						ptr = __builtin_amdgcn_ds_bpermute(src, ptr);
						val = max(val, pv);
					} while (++r < 6 && __builtin_amdgcn_ballot_w64(ptr >= tile_prev) != 0);
				}
				TW_STAMP_A(if (g.stamp) ++st_n_flush;)
				const bool self = val >= min_sc || pi >= 0;            // emitted at its own step (chain.c:304)
				// is the predecessor emitted at its own step?  in-tile predecessors: ask their lane
				const int srcp = (pi >= tile_prev ? pi - tile_prev : lane) << 2;
				const int pself_in = __builtin_amdgcn_ds_bpermute(srcp, self ? 1 : 0);
				const bool pred_self = ext ? ext_self : pself_in != 0;
				wave_mem_fence();
				if (have) tw_st32((((uint32_t)i_lane & 63u) << 3 | (uint32_t)hs << 2) + TW_V, val | (self ? INT_MIN : 0));
				wave_mem_fence();
				// (first_child[] of the tile's anchors is NO_CHILD since the tile was taken in)
				if (have) {
					const uint32_t l4 = tw_here(ln << 2);
					TW_AT(int32_t, f0, l4) = fi;
					TW_AT(int32_t, p0, l4) = pi < 0 ? -1 : pi + rel0_prev;
					TW_AT(int32_t, v0, l4) = val;
					int maybe_first = 0;
					if (pi >= 0 && !pred_self) {
						tw_atomic_min(&TW_AT(int32_t, fc0, tw_here((uint32_t)(pi - tile_prev + TW_RING) << 2)), rel0_prev + i_lane);
						maybe_first = 4;
					}
					TW_AT(uint8_t, fl0, tw_here(ln)) = (uint8_t)((self ? 2 : 0) | maybe_first | (val >= min_sc ? 8 : 0) | (fi < val ? 16 : 0));
				}
			}
			TW_STAMP_A(if (g.stamp) st_flush += (unsigned int)(TW_NOW() - tf0);)
			TW_STAMP_A(const unsigned long long tu0 = g.stamp ? TW_NOW() : 0;)
			TW_STAMP_A(if (g.stamp && !goes_on) ++st_n_unit;)
			// ---- the unit is over: the half's next unit (units that are not for this kernel are handed over), its LDS, its first tile
			bool have_rec = rec0_ok;                                       // rec0 / aux0 are the records of unit c_next
			const bool rec0_used = !goes_on;                               // the loop below takes unit nx0 (or hands it over)
			uint32_t cur_key_now = cur_key;
			while (!goes_on && live) {
				uint32_t nx = (uint32_t)c_next, ne = (uint32_t)((uint64_t)c_next >> 32);
				if (nx >= ne) {
					// the chunk is used up: the counter's next grab (the list is longest first, so the two halves of a wave, and all
					// waves, work on units of similar length at any time and run out of work together)
					uint32_t q0 = 0;
					if (lane == 0) q0 = atomicAdd(kp->queue + 64u * xcd, 1u);
					grab(TW_UNI(q0), nx, ne);
					have_rec = false;
				}
				if (nx >= n_units) {
					c_next = (int64_t)((uint64_t)ne << 32 | nx); live = false;
					if constexpr (L::HAS_XQ) { u.pc = TW_SEL(hm, curb, u.pc); u.pend = TW_SEL(hm, curb, u.pend); }
					else u.pend = TW_SEL(hm, 0u, u.pend);
					break;
				}
				TW_STAMP_C(const unsigned long long tc0 = g.stamp ? TW_NOW() : 0;)
				if (!have_rec) { rec0 = *TW_CONST(tw_u32x4, kp->units + nx); aux0 = *TW_CONST(tw_u32x4, kp->aux + nx); }
				have_rec = false;
				TW_STAMP_C(if (g.stamp) { asm volatile("" :: "s"(rec0.x), "s"(aux0.x)); st_head += (unsigned int)(TW_NOW() - tc0); })
				c_next = (int64_t)((uint64_t)ne << 32 | (nx + 1u));
				Unit un;
				un.start = (int64_t)((uint64_t)rec0.y << 32 | rec0.x); un.read = (int32_t)rec0.z; un.len = (int32_t)rec0.w;
				if (!params_ok || (aux0.z & 1u) || (ONE_LUT && cur_key_now != 0xffffffffu && aux0.y != cur_key_now)) {
					// not for this kernel: hand the unit over (the key test, one table per wave, cannot fail: key_range)
					if (lane == 0) kp->left[atomicAdd(kp->left_cnt, 1u)] = un;
					continue;
				}
				c_base = un.start; c_rel0 = (int)aux0.x; c_room = un.len; c_read = un.read; c_tile0 = 0;
				// the unit's first tile: (PF) requested a tile ago if the unit before it ended as foreseen, else loaded now
				uint64_t tl_x = 0, tl_y = 0;
				TW_STAMP_C(const unsigned long long tc1 = g.stamp ? TW_NOW() : 0;)
				TW_STAMP_C(if (g.stamp && PF && (hs ? pfu1 : pfu0) == (int32_t)c_base) ++st_n_unit;)
				if (PF && (hs ? pfu1 : pfu0) == (int32_t)c_base) { tl_x = hs ? nx1_x : nx0_x; tl_y = hs ? nx1_y : nx0_y; }
				else if (lane < c_room) { const ulonglong2 t = TW_AT(const ulonglong2, kp->a + c_base, tw_here(ln << 4)); tl_x = t.x; tl_y = t.y; }
				if constexpr (PF) { if (hs) pfu1 = -1; else pfu0 = -1; }
				TW_STAMP_C(if (g.stamp) { asm volatile("" :: "v"(tl_x), "v"(tl_y)); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); st_take += (unsigned int)(TW_NOW() - tc1); })
				TW_STAMP_C(const unsigned long long tc2 = g.stamp ? TW_NOW() : 0;)
				// LDS of the half for a new unit: marks never match, every XY slot fails the window test, the read's table (as bytes) unless
				// the table in place is that of a read with the same avg_qspan
				wave_mem_fence();
				if (aux0.y != cur_key_now) {
					const uint2 *src = (const uint2*)(kp->lut + (int64_t)c_read * kp->lut_stride);
					for (int k = lane; k * 4 <= kp->par.bw; k += 64) {           // lut_stride is a multiple of 8 entries: whole uint2 loads
						const uint2 t = src[k];
						const uint32_t w = (t.x & 0xffu) | (t.x >> 8 & 0xff00u) | (t.y << 16 & 0xff0000u) | (t.y << 8 & 0xff000000u);
						tw_st32(lutb + ((uint32_t)k << 2), (int)w);
					}
					cur_key_now = aux0.y;
					if (lane == 0) tw_st32(keya, (int)cur_key_now);
				}
				const uint32_t x_none = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)tl_x, 0) - (uint32_t)kp->par.max_dist_x - 1u;   // "no anchor here" (x+1 encoding)
				for (int k = lane; k < 128; k += 64) tw_st64(((uint32_t)k << 4 | (uint32_t)hs << 3) + TW_XY, x_none, 0u);
				for (int k = lane; k < 65; k += 64) tw_st32(mkb + ((uint32_t)k << 2), -1);
				wave_mem_fence();
				if (lane == 0) tw_st32(sa + TW_CARRY + 12u, 0);
				if (take_tile(tl_x, tl_y) > 0) goes_on = true;                 // (a unit has at least two anchors: always)
				TW_STAMP_C(if (g.stamp) { st_tail += (unsigned int)(TW_NOW() - tc2); ++st_unit; })
			}
			// ---- (PF) the unit ends with the tile just taken: request its successor's first tile now, if the successor is known
			if (PF && live) {
				const int cnt_now = tile_cnt();
				const uint32_t nxn = (uint32_t)c_next, nen = (uint32_t)((uint64_t)c_next >> 32);
				if (!(cnt_now == TW_TILE && c_tile0 + TW_TILE < c_room) && (hs ? pfu1 : pfu0) < 0 && nxn < nen && nxn < n_units &&
				    ((nxn == nx0 && rec0_ok && !rec0_used) || (nxn == nx0 + 1u && rec1_ok))) {
					const tw_u32x4 rn = nxn == nx0 ? rec0 : rec1;            // (nxn == nx0: the loop above did not run, rec0 is untouched)
					const int32_t st = (int32_t)rn.x, len = (int32_t)rn.w;
					uint64_t rx = 0, ry = 0;
					if (lane < len) { const ulonglong2 t = TW_AT(const ulonglong2, kp->a + (int64_t)st, tw_here(ln << 4)); rx = t.x; ry = t.y; }
					if (hs) { nx1_x = rx; nx1_y = ry; pfu1 = st; } else { nx0_x = rx; nx0_y = ry; pfu0 = st; }
				}
			}
			TW_STAMP_A(if (g.stamp) st_unit += (unsigned int)(TW_NOW() - tu0);)
			// ---- the tile's first anchor becomes current
			if (live) {
				const uint32_t i = (uint32_t)c_tile0;
				u.S = TW_SEL(hm, (i - 1u) << 4 | (uint32_t)hs << 3, u.S); u.m4 = TW_SEL(hm, ((i - 1u) << 2) + mkb, u.m4);
			} else retired |= hm;
			if (lane == 0) {
				tw_st64(sa, (uint32_t)c_next, (uint32_t)((uint64_t)c_next >> 32)); tw_st64(sa + 8u, (uint32_t)c_base, (uint32_t)((uint64_t)c_base >> 32));
				tw_st64(sa + 24u, (uint32_t)c_rel0, (uint32_t)c_room);
				tw_st64(sa + 32u, (uint32_t)c_read, (uint32_t)c_tile0);
			}
		}
		wave_mem_fence();
		live_m &= ~retired;
		contm &= ~svc;
	};

	// The tail of a pass in which not both halves finish their scan in their first chunk (or a half is idle): per half either
	// the next anchor becomes current, or the second chunk follows, or -- still undecided after the second chunk -- the unit is
	// handed over.  Returns the halves to service.
	auto slow_tail = [&](uint64_t D, uint32_t a_cur, int nskip_after) -> uint64_t {
		// There are two chunks.  Lane 31 of the second (j = i - 64) is not evaluated (its PF slot is anchor i's own), so a half
		// that is still undecided after it is handed over to k_chain_units.
		const uint64_t giveup = ~D & contm;
		const int vlast = __builtin_amdgcn_ds_bpermute(((h << 5) + 31) << 2, nskip_after);
		wave_mem_fence();
		const tw_u32x2 cur = tw_ld64(a_cur);                                 // the running max just written
		if (__builtin_amdgcn_inverse_ballot_w64(D)) {
			u.m4 += 4u;
			u.S = ((u.m4 - c_mkbase) << 2) | c_8h;
			if constexpr (L::HAS_XQ) u.pc += 8u;
		} else {
			if (hl == 0) {                                                   // what the second chunk starts from
				tw_st64(st_addr + TW_CARRY, cur.x, cur.y);
				tw_st32(st_addr + TW_CARRY + 8u, vlast);
				tw_st32(st_addr + TW_CARRY + 12u, tw_ld32(st_addr + TW_CARRY + 12u) + 1);
			}
			u.S -= 512u;
		}
		contm = ~D & ~giveup & live_m;
		if (__builtin_expect(giveup != 0, 0)) {
			const auto kp = TW_KARGS(g);
			if (__builtin_amdgcn_inverse_ballot_w64(giveup)) {
				wave_mem_fence();
				if (hl == 0) {
					const TwinCold c = TW_COLD;
					Unit un; un.start = (int64_t)((uint64_t)c.base | (uint64_t)(uint32_t)c.tile0 << 32); un.read = c.read; un.len = c.room;
					kp->left[atomicAdd(kp->left_cnt, 1u)] = un;                  // k_chain_units goes on from the tile this scan is in (the tiles
					                                                         // before it are flushed).  The unit is over for this kernel: an empty tile ...
				}
				u.pc = curbase; u.pend = L::HAS_XQ ? curbase : 0u;            // ... has nothing to flush and cannot go on: service() picks the half's next unit
			}
			return giveup;
		}
		return 0;
	};

	TW_STAMP(if (g.stamp) st_t0 = TW_NOW();)
	service(~0ull);
	bool force_general = false;
	// ======================================================================================== main loop: one chunk pass per trip
	while (live_m != 0) {
		wave_mem_fence();                                                    // PF[i-1] of the previous pass, rings written by service()
		uint64_t svc = 0;
		if (__builtin_expect(contm == 0 && live_m == ~0ull && !force_general, 1)) {
			// ------------------------------------------------------------ both halves in their first chunk (n_skip = 0, max_j = none).
			// A loop of its own: while both halves finish every scan in the first chunk nothing but the pass below runs, and its
			// state is updated in place.
			if constexpr (ONE_LUT) {
				// Inside this loop u.S runs one anchor ahead (16 i + 8h: the S1 of the pass), so that it is updated in place; every exit
				// puts it back.  Both halves advance one anchor per pass, so the tile test is a scalar count of the passes until either
				// half's tile ends (at least one: the test behind every pass left both halves with anchors).
				//
				// One exit, so that the compiler has no exits to merge into flag registers: a pass goes on iff it is not interleaved and
				// min(#(B | E) lo, #(B | E) hi, passes left + ms0) > ms0, one scalar compare at the bottom of the inner loop.  Behind it, the
				// rare block finds out why the inner loop stopped: interleaved (general pass), a half that does not break (lane-31 window
				// test: if both halves' scans are complete the outer loop goes on), or the end of the stretch of passes (the tile's, or E's).
				// u.S and u.m4 move on at the end of every pass and are taken back where the anchor is not done.
				uint64_t B, D = 0, I, E = 0;
				uint32_t drx;                                                    // dr - 1 of the pass the inner loop stopped at
				bool tile_end = false;                                           // (or E's stretch: service() then finds no tile exhausted)
				int npass = 1;
				if constexpr (L::HAS_XQ) {
					const int n0 = (int)(TW_UNI(__builtin_amdgcn_readlane((int)u.pend, 0)) - TW_UNI(__builtin_amdgcn_readlane((int)u.pc, 0))) >> 3;
					const int n1 = (int)(TW_UNI(__builtin_amdgcn_readlane((int)u.pend, 32)) - TW_UNI(__builtin_amdgcn_readlane((int)u.pc, 32))) >> 3;
					npass = max(min(n0, n1), 1);
				} else if constexpr (!SAMEGAP) {
					// (the seven-wave instantiation keeps the scalar form of the block below: with the vector form its register
					// allocation spills four more scalar registers in the service)
					const uint32_t m0 = TW_UNI(__builtin_amdgcn_readlane((int)u.m4, 0)), m1 = TW_UNI(__builtin_amdgcn_readlane((int)u.m4, 32));
					const int n0 = (int)(TW_UNI(__builtin_amdgcn_readlane((int)u.pend, 0)) - m0) >> 2;
					const int n1 = (int)(TW_UNI(__builtin_amdgcn_readlane((int)u.pend, 32)) - m1) >> 2;
					npass = max(min(n0, n1), 1);
					const int e0 = 31 - ((int)(m0 - L::MK) >> 2), e1 = 31 - ((int)(m1 - L::MK - TW_MK_HALF) >> 2);   // 32 - i (m4 = 4 (i - 1) + mark base)
					if (e0 > 0) { E |= 0x00000000ffffffffull; npass = min(npass, e0); }
					if (e1 > 0) { E |= 0xffffffff00000000ull; npass = min(npass, e1); }
				} else {
					// Passes until either half's tile ends (at least one), worked out per half in its own lanes (plain two-operand VALU) and
					// read from one lane of each: as scalar code on four v_readlane it was 27 scalar instructions at every entry of this
					// loop, and the loop is entered at every tile and twice more per unit.
					// A half whose anchor is one of its unit's first 32 (i <= 31) has its lane 31 on a slot from before the unit, which
					// fails the window test: its scan is complete whether it breaks or not.  Such a half counts as having 32 B lanes (E)
					// for the passes until its i reaches 32, and the stretch of passes ends there (the outer loop sets E again).
					const uint32_t tm1 = (uint32_t)max(((int)(u.pend - u.m4) >> 2) - 1, 0);         // passes left in the tile, minus one
					const uint32_t em1 = 30u - (uint32_t)((int)(u.m4 - c_mkbase) >> 2);              // 32 - i - 1 (m4 = 4 (i - 1) + mark base): above 31 for i >= 32
					const uint32_t nm1 = min(tm1, em1);
					E = TW_ULT(em1, 32u);
					npass = (int)min(TW_UNI(__builtin_amdgcn_readlane((int)nm1, 0)), TW_UNI(__builtin_amdgcn_readlane((int)nm1, 32))) + 1;
				}
				const uint32_t ms0 = (uint32_t)max(g.par.max_skip, 0);           // a half's scan breaks in this chunk iff it has more B lanes
				uint32_t P = (uint32_t)npass + ms0;                              // passes left + ms0 (npass <= 64: no wrap)
				u.S += 16u;
				for (;;) {
					uint32_t key;
					do {
						const uint32_t S1 = u.S;                                     // 16 i + 8h
						const uint32_t t0 = S1 - L16;                                // lane k <-> predecessor j = i - 1 - k of its half's anchor
						const tw_u32x2 xy = tw_ld64((t0 & 0x7f8u) + TW_XY);
						// the anchor itself: one table, from its XY slot (x + 1, q + 1); two tables, from XQ (x, q)
						const tw_u32x2 cur = tw_ld64(L::HAS_XQ ? u.pc : (S1 & 0x7f8u) + TW_XY);
	#if defined(__HIP_DEVICE_COMPILE__)
						__builtin_amdgcn_sched_barrier(0);                           // the differences wait for these two reads only, not for PF's
	#endif
						const tw_u32x2 pf = tw_ld64((t0 & 0x3f8u) + TW_PF);
						uint32_t a_cur = S1 & 0x3f8u;                                // PF slot of anchor i; one table: its SP byte is this / 8 (a shift:
						TW_OPAQUE(a_cur);                                            // the compiler would make it a three-operand v_bfe from S1)
						const int spm1 = tw_ld_u8(L::HAS_XQ ? (u.pc >> 3) + L::SP_OF_XQ : (a_cur >> 3) + L::SP);   // ... and q_span - 1
	#ifdef TW_EXP_PAD
						// experiment: TW_EXP_PAD dependence-free half-rate VALU instructions (three sources; the result is dropped)
						for (int k = 0; k < TW_EXP_PAD; ++k) { uint32_t pad; asm volatile("v_max3_u32 %0, %1, %1, %1" : "=v"(pad) : "v"(c_far)); }
	#endif
						// differences minus one (the ring holds x + 1, q + 1)
						const uint32_t drm1 = L::HAS_XQ ? cur.x - xy.x : tw_sub_m1(cur.x, xy.x), dqm1 = L::HAS_XQ ? cur.y - xy.y : tw_sub_m1(cur.y, xy.y);
						drx = drm1;
						const uint32_t ddl = ONE_LUT ? tw_absdiff(drm1, dqm1) : tw_sad(drm1, dqm1, c_lut);   // |dr - dq| + the half's table base
						const uint32_t dqs = SAMEGAP ? dqm1 : __builtin_elementwise_add_sat(dqm1, c_dqoff);
						const uint32_t m3 = max(max(drm1, dqs), ddl + c_cbwl);
						const uint64_t okm = TW_ULT(m3, c_M);                        // chain.c:252-260 as one compare
						// the mark round trip (chain.c:281: store by distance, the others to the sink; then the lane's own word) and the table
						// lookup are issued back to back, before anything waits for either
						const uint32_t dst = TW_SEL(okm, min(u.m4 - pf.x, c_far), c_far);
						tw_st32(dst, (int)u.m4);
						wave_mem_fence();
						const int tj = tw_ld32(c_own);
						const int lutv = tw_ld_i8(min(ddl, c_bwl) + LUT_OFF);
	#if defined(__HIP_DEVICE_COMPILE__)
						__builtin_amdgcn_sched_barrier(0);
	#endif
						const int sc0 = min(min((int)dqm1, (int)drm1), spm1);        // chain.c:262-263, minus one
						const int sc = TW_SEL(okm, sc0 + (int)pf.y + lutv, c_min);   // chain.c:272-273 via the table, minus one (the ring holds f - 1)
						const int excl = max(tw_excl_max32(sc), spm1);               // (q_span - 1 >= 0: the scan's zero fill stays below it)
						const uint64_t A = TW_SGT(sc, excl);                         // new running max (chain.c:274); masked lanes hold INT_MIN
						B = TW_EQ(tj, u.m4) & okm & ~A;                              // marked and not better (chain.c:277)
						// n_skip walk (chain.c:276,278) from n_skip = 0.  When every A lane of a half precedes every B lane of it, n_skip at a
						// B lane is the number of B lanes up to it: the break is the (max_skip + 1)-th of them.  An A lane above a B lane
						// (interleaved, rare) sends the anchor to the general pass, which redoes it.  Both tests are on the scalar side, in the
						// exit test below: interleaved iff a half has an A lane above its lowest B lane, and a half breaks iff it has more than
						// max_skip B lanes.
						//
						// The running max goes to PF[i]: the half's last A lane writes its own score and predecessor, or (none) the half's
						// lane 0 writes "no predecessor, q_span" (minus one).  f is max(excl, sc) either way: sc > excl at an A lane, and at lane 0
						// of a half without one, sc <= excl = q_span - 1.  An interleaved pass writes it too: the general pass that redoes the
						// anchor writes PF[i] of both halves before anything reads it.
						{
							const uint32_t wp = TW_SEL(A, u.m4 - c_own, 0xfffffffcu);      // 4 j of the lane's predecessor: 4 (i - 1 - k)
							const int wf = max(excl, sc);
							tw_st64_pf_lanes(tw_last_or_lane0(A), a_cur, wp, (uint32_t)wf);
						}
#ifdef TW_EXP_SPAD
						// experiment: TW_EXP_SPAD dependence-free scalar ALU instructions (a scratch SGPR; no memory, no VALU)
						for (int k = 0; k < TW_EXP_SPAD; ++k) { uint32_t pad; asm volatile("s_xor_b32 %0, %0, %0" : "=s"(pad) :: "scc"); }
#endif
						u.m4 += 4u; u.S += 16u;
						--P;
						const uint64_t BE = B | E;
						uint32_t nmin = min((uint32_t)__builtin_popcount((uint32_t)BE), (uint32_t)__builtin_popcount((uint32_t)(BE >> 32)));
	#if defined(__HIP_DEVICE_COMPILE__)
						asm("" : "+s"(nmin));                                        // (else the two mins become a v_min3 and a v_readfirstlane)
	#endif
						key = tw_exit_key(A, B, min(nmin, P), I);
						TW_STAMP(if (g.stamp && key > ms0) ++st_n_fast;)
						wave_mem_fence();
					} while (__builtin_expect(key > ms0, 1));
					// why the pass stopped.  Interleaved: the general pass redoes the anchor
					if (I != 0) { force_general = true; break; }
					// scan complete: break taken, or the half's last lane is outside the window (x is sorted: nothing older can matter).
					// The window test only matters for a half that does not break.
					const uint32_t nlo = (uint32_t)__builtin_popcount((uint32_t)B), nhi = (uint32_t)__builtin_popcount((uint32_t)(B >> 32));
					if (min(nlo, nhi) <= ms0) {
						const uint64_t OUT = TW_SGE(drx, c_M) & TW_HI31;         // the half's last lane is outside the window (or no anchor there yet)
						D = tw_smear_halves(OUT | (nlo > ms0 ? 0x00000000ffffffffull : 0ull) | (nhi > ms0 ? 0xffffffff00000000ull : 0ull));
						if (tw_both_halves(D) == 0) break;
					}
					// both halves' scans are complete: the next anchor, unless the tile ends
					TW_STAMP(if (g.stamp) ++st_n_fast;)
					if (P <= ms0) { tile_end = true; break; }
					wave_mem_fence();
				}
				TW_OPAQUE(u.S); TW_OPAQUE(u.m4);                                 // (else the compiler keeps the pass' S1 and m4 live out of the loop)
				if (!tile_end) { u.m4 -= 4u; u.S -= 16u; }                        // the anchor the loop stopped at is not done
				const uint32_t a_cur = u.S & 0x3f8u;                             // its PF slot (no tile end)
				u.S -= 16u;
				if (!force_general && !tile_end) {
					// a half wants its second chunk.  n_skip after the first: #B, as no A lane follows a B lane
					svc = slow_tail(D, a_cur + TW_PF, tw_below_in_half(B, hi_half) + (int)__builtin_amdgcn_inverse_ballot_w64(B));
				}
			} else {
				// The two-table layout keeps the pass as it was before the one-table diet: at six waves per SIMD with its tile prefetch, the
				// diet's scalar instructions cost it more than its vector ones save (mixed-key job, chain DP +2 %).
				uint64_t B, X, tile;
				int cB;
				uint32_t a_cur;
				for (;;) {
					const uint32_t S1 = u.S + 16u;                               // 16 i + 8h
					const uint32_t t0 = S1 - L16;                                // lane k <-> predecessor j = jtop - k of its half's anchor
					const tw_u32x2 xy = tw_ld64((t0 & 0x7f8u) + TW_XY);
					const tw_u32x2 cur = tw_ld64(u.pc);
	#if defined(__HIP_DEVICE_COMPILE__)
					__builtin_amdgcn_sched_barrier(0);                           // the differences wait for these two reads only, not for PF's
	#endif
					const tw_u32x2 pf = tw_ld64((t0 & 0x3f8u) + TW_PF);
					const int spm1 = tw_ld_u8((u.pc >> 3) + L::SP_OF_XQ);        // ... and q_span - 1
					const uint32_t drm1 = cur.x - xy.x, dqm1 = cur.y - xy.y;
					const uint32_t ddl = tw_sad(drm1, dqm1, c_lut);
					const uint32_t dqs = SAMEGAP ? dqm1 : __builtin_elementwise_add_sat(dqm1, c_dqoff);
					const uint32_t m3 = max(max(drm1, dqs), ddl + c_cbwl);
					const uint64_t okm = TW_ULT(m3, c_M);
					const uint32_t dst = TW_SEL(okm, min(u.m4 - pf.x, c_far), c_far);
					tw_st32(dst, (int)u.m4);
					wave_mem_fence();
					const int tj = tw_ld32(c_own);
					const int lutv = tw_ld_i8(min(ddl, c_bwl) + LUT_OFF);
	#if defined(__HIP_DEVICE_COMPILE__)
					__builtin_amdgcn_sched_barrier(0);
	#endif
					const int sc0 = min(min((int)dqm1, (int)drm1), spm1);
					const int sc = TW_SEL(okm, sc0 + (int)pf.y + lutv, c_min);
					const int excl = max(tw_excl_max32(sc), spm1);
					const uint64_t A = TW_SGT(sc, excl);
					B = TW_EQ(tj, u.m4) & okm & ~A;
					const uint64_t OUT = TW_SGE(drm1, c_Mout);
					cB = tw_below_in_half(B, hi_half);
					tile = 0; X = 0; a_cur = 0;
					if (__builtin_expect((TW_SGT(cB, 0) & A) != 0, 0)) { force_general = true; break; }
					a_cur = S1 & 0x3f8u;
					{
						const uint32_t wp = TW_SEL(A, u.m4 - c_own, 0xfffffffcu);
						const int wf = TW_SEL(A, sc, spm1);
						if (__builtin_amdgcn_inverse_ballot_w64(tw_last_or_lane0(A))) tw_st64(a_cur + TW_PF, wp, (uint32_t)wf);
					}
					X = (TW_SGE(cB, c_ms) & B) | OUT;
					if (__builtin_expect(tw_both_halves(X) == 0, 0)) break;
					u.m4 += 4u; u.S = S1;
					u.pc += 8u; tile = TW_SGE(u.pc, u.pend);
					TW_STAMP(if (g.stamp) ++st_n_fast;)
					if (__builtin_expect(tile != 0, 0)) break;
					wave_mem_fence();
				}
				if (!force_general && tile == 0) {
					// a half wants its second chunk.  n_skip after the first: #B, as no A lane follows a B lane
					svc = slow_tail(tw_smear_halves(X), a_cur + TW_PF, cB + (int)__builtin_amdgcn_inverse_ballot_w64(B));
				}
			}
		} else {
			// ------------------------------------------------------------ general pass: second chunks, idle halves, interleaved walks
			force_general = false;
			const uint32_t t0 = u.S + 16u - L16;                                  // (L16 is 16 (k + 1))
			const uint32_t xcur = ((((u.m4 - c_mkbase) + 4u) << 2) & 0x7f8u) | c_8h;   // XY slot of anchor i (m4 = 4 (i - 1) + mark base)
			const tw_u32x2 xy = tw_ld64((t0 & 0x7f8u) + TW_XY);
			const tw_u32x2 pf = tw_ld64((t0 & 0x3f8u) + TW_PF);
			const tw_u32x2 cur = tw_ld64(L::HAS_XQ ? u.pc : xcur + TW_XY);
			const int spm1 = tw_ld_u8(L::HAS_XQ ? (u.pc >> 3) + L::SP_OF_XQ : ((xcur >> 3) & 0x7fu) + L::SP);
			const uint64_t first = ~contm;                                       // halves in their first chunk: running max = q_span, nothing carried
			const tw_u32x2 carry = tw_ld64(st_addr + TW_CARRY);
			const int maxf = TW_SEL(first, spm1, (int)carry.y);
			const uint32_t maxj4 = TW_SEL(first, 0xfffffffcu, carry.x);
			const int nskip0 = TW_SEL(first, 0, tw_ld32(st_addr + TW_CARRY + 8u));
			const uint32_t kb4 = TW_SEL(first, 0u, 128u);                        // 128 * c
			const uint32_t drm1 = L::HAS_XQ ? cur.x - xy.x : tw_sub_m1(cur.x, xy.x), dqm1 = L::HAS_XQ ? cur.y - xy.y : tw_sub_m1(cur.y, xy.y);
			const uint32_t ddl = ONE_LUT ? tw_absdiff(drm1, dqm1) : tw_sad(drm1, dqm1, c_lut);
			const uint32_t dqs = SAMEGAP ? dqm1 : __builtin_elementwise_add_sat(dqm1, c_dqoff);
			const uint32_t m3 = max(max(drm1, dqs), ddl + c_cbwl);
			// not evaluated: lane 31 of a second chunk (j = i - 64 shares its PF slot with anchor i itself) and idle halves
			const uint64_t okm = TW_ULT(m3, c_M) & ~(contm & TW_HI31) & live_m;
			const int sc0 = min(min((int)dqm1, (int)drm1), spm1);
			const int lutv = tw_ld_i8(min(ddl, c_bwl) + LUT_OFF);
			const uint32_t dst = TW_SEL(okm, min(u.m4 - pf.x, c_far), c_far);
			tw_st32(dst, (int)u.m4);
			wave_mem_fence();
			const int tj = tw_ld32(c_own + kb4);
			const int sc = TW_SEL(okm, sc0 + (int)pf.y + lutv, c_min);
			const int excl = max(tw_excl_max32(sc), maxf);
			const uint64_t A = TW_SGT(sc, excl);
			const uint64_t B = TW_EQ(tj, u.m4) & okm & ~A;
			const uint64_t OUT = TW_SGE(drm1, c_M);
			const int cB = tw_below_in_half(B, hi_half), cA = tw_below_in_half(A, hi_half);
			const int isA = (int)__builtin_amdgcn_inverse_ballot_w64(A), isB = (int)__builtin_amdgcn_inverse_ballot_w64(B);
			const uint64_t inter = TW_SGT(cB, 0) & A;
			uint64_t brk, Ap;
			int nskip_after;
			if (inter == 0) {
				// at a B lane all A lanes of the half are below it: n_skip = max(n0 - #A, 0) + #B up to and including it
				nskip_after = max(nskip0 - cA - isA, 0) + cB + isB;
				brk = TW_SGT(nskip_after, c_ms) & B;
				Ap = A;
			} else {
				const int Sk = nskip0 + cB + isB - cA - isA;
				nskip_after = Sk - min(tw_incl_min32(Sk), 0);
				brk = TW_SGT(nskip_after, c_ms) & B;
				Ap = tw_below_first(A, brk);
			}
			const uint32_t a_cur = (xcur & 0x3f8u) + TW_PF;                      // PF slot of anchor i
			{
				const uint32_t wp = TW_SEL(Ap, u.m4 - c_own - kb4, maxj4);          // 4 j = 4 (i - 1 - 32 c - k)
				const int wf = TW_SEL(Ap, sc, maxf);
				if (__builtin_amdgcn_inverse_ballot_w64(tw_last_or_lane0(Ap))) tw_st64(a_cur, wp, (uint32_t)wf);
			}
			const uint64_t D = tw_smear_halves(brk | (OUT & TW_HI31) | ~live_m);   // idle halves count as done
			svc = slow_tail(D, a_cur, nskip_after);
		}
		// ---------------------------------------------------------------- tile exhausted (or unit handed over): flush, next tile / unit
		svc |= tw_smear_halves((L::HAS_XQ ? TW_SGE(u.pc, u.pend) : TW_SGE(u.m4, u.pend)) & live_m & ~contm);
		if (__builtin_expect(svc != 0, 0)) {
			TW_STAMP(const unsigned long long ts = g.stamp ? TW_NOW() : 0;)
			service(svc & live_m);
			TW_STAMP(if (g.stamp) { st_service += (unsigned int)(TW_NOW() - ts); ++st_n_service; })
		}
	}
	TW_STAMP(if (g.stamp && lane == 0) {
		unsigned long long *o = g.stamp + 12 * (size_t)blockIdx.x;
		o[0] = TW_NOW() - st_t0; o[1] = st_service; o[2] = st_flush; o[3] = st_unit; o[4] = st_n_service; o[5] = st_n_fast; o[6] = st_n_unit; o[7] = 1; o[8] = st_head; o[9] = st_take; o[10] = st_tail; o[11] = (unsigned long long)st_n_flush << 32 | st_rounds;
	})
#undef TW_COLD
}

size_t twin_lds_bytes(bool one_table) { return one_table ? TwLayout<true>::BYTES : TwLayout<false>::BYTES; }

// workgroups per CU a launch asks for at most: what the LDS allows (32 with one table, 24 with two) and the registers (TwWaves)
int twin_max_wg_per_cu(bool samegap, bool one_table)
{
	const int lds_wg = one_table ? 32 : 24;                          // 5120 / 6400 bytes of LDS allocated per workgroup (4864 / 6400 used)
	const int waves = one_table ? (samegap ? TwWaves<true, true>::N : TwWaves<false, true>::N)
	                            : (samegap ? TwWaves<true, false>::N : TwWaves<false, false>::N);
	return 4 * waves < lds_wg ? 4 * waves : lds_wg;
}

// the grid of a launch: persistent waves, as many as the chip holds at the layout's occupancy (LDS, and TwWaves per SIMD for the
// registers; wg_per_cu, CHAINDP_TWIN_WG_PER_CU, lowers it), each half taking units from a queue
static int64_t twin_blocks(int64_t max_units, int cus, int max_wg, int wg_per_cu)
{
	int64_t blocks = (max_units + 2 * TW_QCH - 1) / (2 * TW_QCH);
	const int64_t cap = (int64_t)cus * (wg_per_cu >= 1 && wg_per_cu <= max_wg ? wg_per_cu : max_wg);
	if (blocks > cap) blocks = cap;
	if (blocks < 1) blocks = 1;
	return (blocks + 7) & ~(int64_t)7;                             // eight grab counters, workgroup b on counter b mod 8: the same number of halves on each
}

// DpDevice::twin_stamp: 12 words per workgroup of the largest grid on a device of `cus` CUs
size_t twin_stamp_bytes(int cus) { return (size_t)twin_blocks(INT64_MAX / 2, cus, 32, 0) * 96; }

// one launch of the layout ONE_LUT (the kernel returns at once when the batch is not for it)
template <bool ONE_LUT>
static hipError_t launch_twin_layout(const DpDevice &dev, hipStream_t st, TwinArgs g, int64_t max_units)
{
	const bool samegap = g.par.max_dist_y >= g.par.max_dist_x;
	const int64_t blocks = twin_blocks(max_units, dev.cus, twin_max_wg_per_cu(samegap, ONE_LUT), dev.twin_wg_per_cu);
	{
		const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)g.queue, (int)(2 * blocks / 8), 8 * 64, st);   // every counter starts behind its halves' first grabs
		if (e != hipSuccess) return e;
	}
	// diagnostic: CHAINDP_TWIN_STAMP=1 makes the kernel stamp where its waves' time goes (s_memtime: shader-clock ticks) and this
	// function print the averages -- it synchronises, so never set it in a timed run
	g.stamp = dev.twin_stamp;
	if (g.stamp) (void)hipMemsetAsync(g.stamp, 0, (size_t)blocks * 96, st);
	if (samegap) hipLaunchKernelGGL((k_chain_twin<true, ONE_LUT>), dim3((unsigned)blocks), dim3(64), TwLayout<ONE_LUT>::BYTES, st, g);
	else hipLaunchKernelGGL((k_chain_twin<false, ONE_LUT>), dim3((unsigned)blocks), dim3(64), TwLayout<ONE_LUT>::BYTES, st, g);
	if (g.stamp) {
		std::vector<unsigned long long> hb((size_t)blocks * 12);
		if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(hb.data(), g.stamp, hb.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
			double tot = 0, svc = 0, flush = 0, unit = 0, nsvc = 0, nfast = 0, nunit = 0, nb = 0, head = 0, take = 0, tail = 0, rounds = 0, nflush = 0;
			for (int64_t b = 0; b < blocks; ++b) if (hb[(size_t)b * 12 + 7]) {
				const unsigned long long *o = &hb[(size_t)b * 12];
				tot += o[0]; svc += o[1]; flush += o[2]; unit += o[3]; nsvc += o[4]; nfast += o[5]; nunit += o[6]; head += o[8]; take += o[9]; tail += o[10]; rounds += (double)(o[11] & 0xffffffffull); nflush += (double)(o[11] >> 32); ++nb;
			}
			if (nb > 0) fprintf(stderr, "[twin stamp raw] sums over waves: head %.0f take %.0f tail %.0f unit %.0f n_unit %.0f (build 3: ticks until the record / the first tile / the rest of a unit switch; switches; first tiles requested ahead)\n", head, take, tail, unit, nunit);
			if (nflush > 0) fprintf(stderr, "[twin stamp flush] %.0f tiles flushed, %.0f rounds of the v[] loop: %.3f a tile (build 1)\n", nflush, rounds, rounds / nflush);
			if (nb > 0) fprintf(stderr, "[twin stamp] %.0f waves, %.0f ticks each: service %.1f%% (%.0f calls, %.0f ticks each: cold state and decisions %.0f, next tile %.0f, flush %.0f, "
			                "unit switch %.0f (%.0f switches, %.0f ticks each), first anchor and cold state back %.0f), passes %.0f (%.0f ticks each, everything else included)\n",
			        nb, tot / nb, 100.0 * svc / tot, nsvc, svc / (nsvc > 0 ? nsvc : 1), head / (nsvc > 0 ? nsvc : 1), take / (nsvc > 0 ? nsvc : 1), flush / (nsvc > 0 ? nsvc : 1),
			        unit / (nsvc > 0 ? nsvc : 1), nunit, unit / (nunit > 0 ? nunit : 1), tail / (nsvc > 0 ? nsvc : 1), nfast, (tot - svc) / (nfast > 0 ? nfast : 1));
		}
	}
	return hipGetLastError();
}

hipError_t launch_chain_twin(const DpDevice &dev, const DpBatch &b)
{
	const int64_t max_units = b.total / 2;
	if (max_units <= 0) return hipSuccess;
	if (!b.aux || !b.key_range || !b.twin_queue) return hipErrorInvalidValue;
	TwinArgs g;
	g.par = b.par; g.off = b.off; g.a = (const ulonglong2*)b.a; g.sumq = b.sumq; g.lut = b.lut; g.lut_stride = b.lut_stride;
	if (b.n_segs) g.par.n_segs = 1;      // with per-read segment counts the units' UnitAux flags say which reads are multi-segment
	                                     // (the batch-wide count is not used then, as in k_chain_units)
	g.units = b.units; g.aux = b.aux; g.counters = b.counters; g.f = b.f; g.p = b.p; g.v = b.v; g.first_child = b.first_child; g.flags = b.flags;
	g.left = b.left; g.left_cnt = b.hw.left_count(); g.queue = b.twin_queue; g.key_range = b.key_range; g.route = b.hw.route(); g.two_tables = b.two_tables != 0;
	g.force_left = b.force_left; g.total = b.total; g.stamp = nullptr;
	// both layouts, one table first: the device decides which one takes the batch (g.route), the other returns at once
	hipError_t e = launch_twin_layout<true>(dev, b.st, g, max_units);
	if (e == hipSuccess) e = launch_twin_layout<false>(dev, b.st, g, max_units);
	return e;
}

// the instantiations of k_chain_twin (their LDS size is the layout's, fixed)
int twin_kernels(DpKernel *out)
{
	out[0] = {(const void*)k_chain_twin<true, true>, "k_chain_twin<samegap, one table>", TwLayout<true>::BYTES};
	out[1] = {(const void*)k_chain_twin<false, true>, "k_chain_twin<one table>", TwLayout<true>::BYTES};
	out[2] = {(const void*)k_chain_twin<true, false>, "k_chain_twin<samegap, two tables>", TwLayout<false>::BYTES};
	out[3] = {(const void*)k_chain_twin<false, false>, "k_chain_twin<two tables>", TwLayout<false>::BYTES};
	return 4;
}

} // namespace chaindp
