// chaindp_ksw.hip -- ksw_extd2_sse (reference ksw2_extd2_sse.c, the path without KSW_EZ_GENERIC_SC) for a batch of problems, bit for bit.
//
// One workgroup per problem: one wave, or KSW_WIDE_WAVES waves for the wide ones.  The diagonals r = 0 .. qlen + tlen - 2 are serial;
// on a diagonal thread l of NT owns the cells t = st + l (mod NT), NT at a time.  The state keeps the reference's memory layout: its nine byte arrays u v x y x2 y2 s sf qr are ONE block of
// 8 T + Q + 16 bytes (T, Q = tlen, qlen rounded up to 16), because the reference
//   - computes every cell of the 16-byte words the band [st0, en0] touches, from stale s[], and reads some of them back one
//     diagonal later (x8[st - 1] at :143, u[en0 + 1] / y[en0 + 1] when the band's upper edge moves), and
//   - lets its unaligned 16-byte score stores (:171) run from s into sf[0..14] and its loads (:160-161) from sf into qr and from qr
//     into the zero padding behind it.
// With the block laid out the same way all of that falls out of plain indexing.  A diagonal is done as the vector code does a word:
// every load of a step before any of its stores.  Cells are carried sign-extended in 32-bit registers and wrapped to int8 after every
// add and subtract (v_bfe_i32), so compares, max and min are the signed 8-bit ones of the reference.
// The block and H[] (int32 per t) live in LDS while 12 T + Q + 16 <= KSW_LDS_BUDGET, else in the workgroup's slice of global scratch;
// the path matrix p (a byte per cell, n_col_ * 16 per diagonal) is global, one slice per resident workgroup, and is walked back by
// lane 0 right after the last diagonal (ksw_backtrack with is_rot = 1; off[] / off_end[] are recomputed from r).
#include "chaindp_kernels.h"
#include "chaindp_wave.h"

namespace chaindp {

#define KSW_NEG_INF (-0x40000000)
#define KSW_F_SCORE_ONLY 0x01
#define KSW_F_RIGHT 0x02
#define KSW_F_APPROX_MAX 0x08
#define KSW_F_EXTZ_ONLY 0x40
#define KSW_F_REV_CIGAR 0x80

__device__ __forceinline__ int wrap8(int v) { return (int)(int8_t)v; }     // what _mm_add_epi8 / _mm_sub_epi8 leave of a sum

// store -> load hand-over between the threads of the workgroup
template <bool IN_LDS, int WAVES> __device__ __forceinline__ void ksw_fence()
{
	if (WAVES > 1) __syncthreads();
	else if (IN_LDS) wave_mem_fence();
	else wave_global_fence();
}
// between the loads of a step and its stores: one wave runs in lockstep, several have to meet
template <int WAVES> __device__ __forceinline__ void ksw_loads_done()
{
	if (WAVES > 1) __syncthreads(); else wave_mem_fence();
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the band of diagonal r (:124-139): st0, en0 as computed, st, en rounded out to 16-byte words; false where st0 > en0
__device__ __forceinline__ bool ksw_band(int r, int qlen, int tlen, int w, int &st0, int &en0, int &st, int &en)
{
	st0 = 0; en0 = tlen - 1;
	if (st0 < r - qlen + 1) st0 = r - qlen + 1;
	if (en0 > r) en0 = r;
	if (st0 < (r - w + 1) >> 1) st0 = (r - w + 1) >> 1;
	if (en0 > (r + w) >> 1) en0 = (r + w) >> 1;
	st = st0 / 16 * 16; en = (en0 + 16) / 16 * 16 - 1;
	return st0 <= en0;
}

// ksw_backtrack(is_rot = 1, min_intron_len = 0) from cell (i0, j0) with the run-length push; returns n_cigar.  One lane.
__device__ __forceinline__ int ksw_traceback(const uint8_t *p, int n_col, int qlen, int tlen, int w, int i0, int j0, uint32_t *cig)
{
	int n = 0, i = i0, j = j0, state = 0;
	uint32_t cur_op = 0, cur_len = 0;
	auto push = [&](uint32_t op, uint32_t len) {
		if (cur_len && op == cur_op) cur_len += len;
		else {
			if (cur_len) cig[n++] = cur_len << 4 | cur_op;
			cur_op = op; cur_len = len;
		}
	};
	while (i >= 0 && j >= 0) {
		const int r = i + j;
		int st0, en0, st, en, force = -1;
		ksw_band(r, qlen, tlen, w, st0, en0, st, en);
		if (i < st) force = 2;
		if (i > en) force = 1;
		const int tmp = force < 0 ? p[(int64_t)r * n_col + i - st] : 0;
		if (state == 0) state = tmp & 7;
		else if (!(tmp >> (state + 2) & 1)) state = 0;
		if (state == 0) state = tmp & 7;
		if (force >= 0) state = force;
		if (state == 0) { push(0, 1); --i; --j; }
		else if (state == 1 || state == 3) { push(2, 1); --i; }
		else { push(1, 1); --j; }
	}
	if (i >= 0) push(2, i + 1);
	if (j >= 0) push(1, j + 1);
	if (cur_len) cig[n++] = cur_len << 4 | cur_op;
	return n;
}

template <bool IN_LDS, int WAVES>
__device__ __forceinline__ void ksw_problem(long long *xch, int8_t *mem, int32_t *H, uint8_t *p, const uint8_t *query, const uint8_t *target, int qlen, int tlen,
                                            int w, int zdrop, int end_bonus, int flag, const KswScore sc, int route, int32_t *ez_out, uint32_t *cig)
{
	constexpr int NT = 64 * WAVES;
	const int lane = threadIdx.x;                      // the thread's number in the workgroup
	const int q = sc.q, e = sc.e, q2 = sc.q2, e2 = sc.e2, qe = sc.qe0;
	const bool with_cigar = !(flag & KSW_F_SCORE_ONLY), approx_max = flag & KSW_F_APPROX_MAX, right = flag & KSW_F_RIGHT;
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	const int T = (tlen + 15) / 16 * 16, Q = (qlen + 15) / 16 * 16;
	const int n_col = ksw_n_col(qlen, tlen, w);
	int long_thres = e != e2 ? (q2 - q) / (e - e2) - 1 : 0;
	if (q2 + e2 + long_thres * e2 > q + e + long_thres * e) ++long_thres;
	const int long_diff = long_thres * (e - e2) - (q2 - q) - e2;
	const int init1 = wrap8(-q - e), init2 = wrap8(-q2 - e2), q8 = wrap8(q), q28 = wrap8(q2), qe8 = wrap8(q + e), qe28 = wrap8(q2 + e2);
	const int sc_mch = wrap8(sc.a), sc_mis = wrap8(-sc.b), sc_n = wrap8(-e2);
	int8_t *u8 = mem, *v8 = mem + T, *x8 = mem + 2 * T, *y8 = mem + 3 * T, *x28 = mem + 4 * T, *y28 = mem + 5 * T, *s8 = mem + 6 * T;
	const uint8_t *sf = (const uint8_t*)mem + 7 * T, *qr = (const uint8_t*)mem + 8 * T;

	// the block as :99-108, :120-121 leave it, and H[]
	for (int i = lane; i < 8 * T + Q + 16; i += NT) {
		int val = i < 4 * T ? init1 : i < 6 * T ? init2 : 0;
		if (i >= 7 * T && i < 7 * T + tlen) val = target[i - 7 * T];
		else if (i >= 8 * T && i < 8 * T + qlen) val = query[qlen - 1 - (i - 8 * T)];
		mem[i] = (int8_t)val;
	}
	for (int i = lane; i < T; i += NT) H[i] = KSW_NEG_INF;
	ksw_fence<IN_LDS, WAVES>();

	// ksw_extz_t, wave-uniform
	int ez_max = 0, ez_zdropped = 0, ez_max_q = -1, ez_max_t = -1, ez_mqe = KSW_NEG_INF, ez_mqe_t = -1, ez_mte = KSW_NEG_INF, ez_mte_q = -1;
	int ez_score = KSW_NEG_INF, ez_reach_end = 0;
	int H0 = 0, last_H0_t = 0, last_st = -1, last_en = -1;
	const int n_diag = qlen + tlen - 1;

	for (int r = 0; r < n_diag; ++r) {
		int st0, en0, st, en;
		if (!ksw_band(r, qlen, tlen, w, st0, en0, st, en)) { ez_zdropped = 1; break; }
		// boundary conditions (:141-155)
		const int edge = r == 0 ? init1 : r < long_thres ? wrap8(-e) : r == long_thres ? wrap8(long_diff) : wrap8(-e2);
		int x1 = init1, x21 = init2, v1 = init1;
		if (st > 0) {
			if (st - 1 >= last_st && st - 1 <= last_en) { x1 = uniform(x8[st - 1]); x21 = uniform(x28[st - 1]); v1 = uniform(v8[st - 1]); }
		} else v1 = edge;
		if (en >= r && lane == 0) { y8[r] = (int8_t)init1; y28[r] = (int8_t)init2; u8[r] = (int8_t)edge; }
		// scores (:158-172): whole 16-byte words from st0; the loads of a step before its stores
		const uint8_t *qrr = qr + (qlen - 1 - r);
		const int n_sc = ((en0 - st0) / 16 + 1) * 16;
		for (int j0 = 0; j0 < n_sc; j0 += NT) {
			const int t = st0 + j0 + lane;
			const bool act = j0 + lane < n_sc;
			int val = 0;
			if (act) {
				const int sq = sf[t], sr = qrr[t];
				val = sq == sr ? sc_mch : sc_mis;
				if (sq == 4 || sr == 4) val = sc_n;
			}
			ksw_loads_done<WAVES>();
			if (act) s8[t] = (int8_t)val;
		}
		ksw_fence<IN_LDS, WAVES>();
		// the cells of [st, en], highest NT first: a step's left neighbours belong to a step that has not stored yet
		uint8_t *pr = p + (int64_t)r * n_col;
		for (int c = (en - st) / NT; c >= 0; --c) {
			const int t = st + c * NT + lane;
			const bool act = t <= en;
			int z = 0, ut = 0, xt1 = x1, vt1 = v1, x2t1 = x21, yt = 0, y2t = 0;
			if (act) {
				z = s8[t]; ut = u8[t]; yt = y8[t]; y2t = y28[t];
				if (t > st) { xt1 = x8[t - 1]; vt1 = v8[t - 1]; x2t1 = x28[t - 1]; }
			}
			ksw_loads_done<WAVES>();
			if (act) {
				int a = wrap8(xt1 + vt1), b = wrap8(yt + ut), a2 = wrap8(x2t1 + vt1), b2 = wrap8(y2t + ut), d;
				if (!right) {
					d = a > z ? 1 : 0; z = max(z, a);
					d = b > z ? 2 : d; z = max(z, b);
					d = a2 > z ? 3 : d; z = max(z, a2);
					d = b2 > z ? 4 : d; z = max(z, b2);
				} else {
					d = z > a ? 0 : 1; z = max(z, a);
					d = z > b ? d : 2; z = max(z, b);
					d = z > a2 ? d : 3; z = max(z, a2);
					d = z > b2 ? d : 4; z = max(z, b2);
				}
				z = min(z, sc_mch);
				u8[t] = (int8_t)(z - vt1);
				v8[t] = (int8_t)(z - ut);
				int tmp = wrap8(z - q8);
				a = wrap8(a - tmp); b = wrap8(b - tmp);
				tmp = wrap8(z - q28);
				a2 = wrap8(a2 - tmp); b2 = wrap8(b2 - tmp);
				x8[t] = (int8_t)(max(a, 0) - qe8);
				y8[t] = (int8_t)(max(b, 0) - qe8);
				x28[t] = (int8_t)(max(a2, 0) - qe28);
				y28[t] = (int8_t)(max(b2, 0) - qe28);
				if (with_cigar) {
					const int lim = right ? -1 : 0;               // left: continue where > 0; right: where >= 0
					d |= (a > lim ? 0x08 : 0) | (b > lim ? 0x10 : 0) | (a2 > lim ? 0x20 : 0) | (b2 > lim ? 0x40 : 0);
					pr[t - st] = (uint8_t)d;
				}
			}
		}
		ksw_fence<IN_LDS, WAVES>();
		if (!approx_max) {
			// H[], max_H and max_t (:315-350)
			int max_H, max_t, H_en0, H_st0;
			if (r > 0) {
				H_en0 = en0 > 0 ? uniform(H[en0 - 1]) + uniform(u8[en0]) : uniform(H[en0]) + uniform(v8[en0]);
				ksw_loads_done<WAVES>();
				// The reference keeps four running maxima over t = st0 + i (mod 4), t < en1, each its first strict one, all seeded with
				// H[en0]; merges them in lane order with a strict compare; then runs the last (en0 - st0) % 4 cells.  Among equal values
				// the winner is the first in that order: the seed, class 0 by t, class 1 by t, ..., the tail by t.
				const int en1 = st0 + (en0 - st0) / 4 * 4;
				long long best = (long long)H_en0 << 32 | 0xffffffffu;
				for (int t = st0 + lane; t < en0; t += NT) {
					const int h = H[t] + v8[t];
					H[t] = h;
					const uint32_t rank = (uint32_t)(t < en1 ? (t - st0) & 3 : 4) << 28 | (uint32_t)t;
					const long long key = (long long)h << 32 | (0x7fffffffu - rank);
					best = key > best ? key : best;
				}
				for (int m = 32; m; m >>= 1) {
					const long long o = __shfl_xor(best, m);
					best = o > best ? o : best;
				}
				if (WAVES > 1) {                        // the waves' maxima meet in LDS
					if ((lane & 63) == 0) xch[lane >> 6] = best;
					__syncthreads();
					for (int k = 0; k < WAVES; ++k) best = xch[k] > best ? xch[k] : best;
				}
				max_H = (int)(best >> 32);
				const uint32_t lo = (uint32_t)best;
				max_t = lo == 0xffffffffu ? en0 : (int)((0x7fffffffu - lo) & 0x0fffffffu);
				if (lane == 0) H[en0] = H_en0;
				ksw_fence<IN_LDS, WAVES>();
				H_st0 = st0 == en0 ? H_en0 : uniform(H[st0]);
			} else {
				H_en0 = H_st0 = max_H = uniform(v8[0]) - qe; max_t = 0;
				if (lane == 0) H[0] = H_en0;
				ksw_fence<IN_LDS, WAVES>();
			}
			if (en0 == tlen - 1 && H_en0 > ez_mte) { ez_mte = H_en0; ez_mte_q = r - en; }
			if (r - st0 == qlen - 1 && H_st0 > ez_mqe) { ez_mqe = H_st0; ez_mqe_t = st0; }
			// ksw_apply_zdrop
			if (max_H > ez_max) { ez_max = max_H; ez_max_t = max_t; ez_max_q = r - max_t; }
			else if (max_t >= ez_max_t && r - max_t >= ez_max_q) {
				const int tl = max_t - ez_max_t, ql = (r - max_t) - ez_max_q, l = tl > ql ? tl - ql : ql - tl;
				if (zdrop >= 0 && ez_max - max_H > zdrop + l * e2) { ez_zdropped = 1; break; }
			}
			if (r == n_diag - 1 && en0 == tlen - 1) ez_score = H_en0;
		} else {
			// one cell per diagonal (:359-375; KSW_EZ_APPROX_DROP is not taken)
			if (r > 0) {
				if (last_H0_t >= st0 && last_H0_t <= en0 && last_H0_t + 1 >= st0 && last_H0_t + 1 <= en0) {
					const int d0 = uniform(v8[last_H0_t]), d1 = uniform(u8[last_H0_t + 1]);
					if (d0 > d1) H0 += d0;
					else { H0 += d1; ++last_H0_t; }
				} else if (last_H0_t >= st0 && last_H0_t <= en0) H0 += uniform(v8[last_H0_t]);
				else { ++last_H0_t; H0 += uniform(u8[last_H0_t]); }
			} else { H0 = uniform(v8[0]) - qe; last_H0_t = 0; }
			if (r == n_diag - 1 && en0 == tlen - 1) ez_score = H0;
		}
		last_st = st; last_en = en;
	}

	// where the traceback starts (:381-390), the walk, the reversal
	int n_cigar = 0;
	if (with_cigar) {
		int i0 = -1, j0 = -1;
		if (!ez_zdropped && !(flag & KSW_F_EXTZ_ONLY)) { i0 = tlen - 1; j0 = qlen - 1; }
		else if (!ez_zdropped && (flag & KSW_F_EXTZ_ONLY) && ez_mqe + end_bonus > ez_max) { ez_reach_end = 1; i0 = ez_mqe_t; j0 = qlen - 1; }
		else if (ez_max_t >= 0 && ez_max_q >= 0) { i0 = ez_max_t; j0 = ez_max_q; }
		if (i0 >= 0) {
			ksw_fence<false, WAVES>();
			if (lane == 0) n_cigar = ksw_traceback(p, n_col, qlen, tlen, w, i0, j0, cig);
			if (WAVES > 1) {
				if (lane == 0) xch[WAVES] = n_cigar;
				__syncthreads();
				n_cigar = (int)xch[WAVES];
			} else n_cigar = __shfl(n_cigar, 0);
			if (!(flag & KSW_F_REV_CIGAR)) {
				ksw_fence<false, WAVES>();
				for (int i = lane; i < n_cigar >> 1; i += NT) {
					const uint32_t lo = cig[i], hi = cig[n_cigar - 1 - i];
					cig[i] = hi; cig[n_cigar - 1 - i] = lo;
				}
			}
		}
	}
	if (lane == 0) {
		ez_out[0] = ez_max; ez_out[1] = ez_zdropped; ez_out[2] = ez_max_q; ez_out[3] = ez_max_t; ez_out[4] = ez_mqe; ez_out[5] = ez_mqe_t;
		ez_out[6] = ez_mte; ez_out[7] = ez_mte_q; ez_out[8] = ez_score; ez_out[9] = ez_reach_end; ez_out[10] = n_cigar; ez_out[11] = route;
	}
}

static_assert((KSW_WIDE_WAVES + 2) * 8 <= KSW_XCH_BYTES, "the exchange words of a workgroup: one per wave and two more");

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_ksw_extd(int64_t n, const KswProb *__restrict__ prob, const int32_t *__restrict__ order,
                                                         const uint8_t *__restrict__ bases, const KswScore sc, uint8_t *state, size_t state_stride,
                                                         uint8_t *path, size_t path_stride, int32_t *ez, uint32_t *cig, unsigned int *counter)
{
	extern __shared__ __align__(16) uint8_t ksw_lds[];
	long long *xch = (long long*)ksw_lds;
	uint8_t *lds = ksw_lds + KSW_XCH_BYTES;
	const int lane = threadIdx.x;
	for (;;) {
		unsigned int k = 0;
		if (lane == 0) k = atomicAdd(counter, 1u);
		if (WAVES > 1) {
			if (lane == 0) xch[WAVES + 1] = k;
			__syncthreads();
			k = (unsigned int)xch[WAVES + 1];
		}
		k = (unsigned int)uniform((int)k);
		if ((int64_t)k >= n) break;
		const int i = order[k];
		const KswProb pb = prob[i];
		const int route = ksw_route(pb.qlen, pb.tlen, sc.skip);
		int32_t *ez_i = ez + (int64_t)i * KSW_EZ_WORDS;
		uint32_t *cig_i = cig + pb.cig_beg;
		uint8_t *p = path + (size_t)blockIdx.x * path_stride;
		const int64_t blk = ksw_state_bytes(pb.qlen, pb.tlen) - 4 * (((int64_t)pb.tlen + 15) / 16 * 16);      // the nine arrays; H[] behind them
		if (route == KSW_ROUTE_NONE) {
			if (lane < KSW_EZ_WORDS) {      // ksw_reset_extz
				// max, zdropped 0; max_q, max_t, mqe_t, mte_q -1; mqe, mte, score KSW_NEG_INF; reach_end, n_cigar, route 0
				const bool neg1 = lane == 2 || lane == 3 || lane == 5 || lane == 7, ninf = lane == 4 || lane == 6 || lane == 8;
				ez_i[lane] = neg1 ? -1 : ninf ? KSW_NEG_INF : 0;
			}
		} else if (route != KSW_ROUTE_GLOBAL) {
			ksw_problem<true, WAVES>(xch, (int8_t*)lds, (int32_t*)(lds + blk), p, bases + pb.q_beg, bases + pb.t_beg, pb.qlen, pb.tlen, pb.w, pb.zdrop,
			                         pb.end_bonus, pb.flag, sc, route, ez_i, cig_i);
		} else if (WAVES == 1) {
			uint8_t *g = state + (size_t)blockIdx.x * state_stride;
			ksw_problem<false, 1>(xch, (int8_t*)g, (int32_t*)(g + blk), p, bases + pb.q_beg, bases + pb.t_beg, pb.qlen, pb.tlen, pb.w, pb.zdrop,
			                      pb.end_bonus, pb.flag, sc, route, ez_i, cig_i);
		}
		ksw_fence<false, WAVES>();      // the next problem reuses the state, the path slice and the exchange words
	}
}

__global__ __launch_bounds__(64) void k_ksw_pack(int64_t n, const KswProb *__restrict__ prob, const int32_t *__restrict__ ez,
                                                 const int64_t *__restrict__ off, const uint32_t *__restrict__ cig, uint32_t *__restrict__ out)
{
	for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
		const int m = ez[i * KSW_EZ_WORDS + 10];
		const uint32_t *src = cig + prob[i].cig_beg;
		uint32_t *dst = out + off[i];
		for (int k = threadIdx.x; k < m; k += 64) dst[k] = src[k];
	}
}

hipError_t launch_ksw_extd(hipStream_t st, int waves, int grid, size_t lds_bytes, int64_t n, const KswProb *d_prob, const int32_t *d_order,
                           const uint8_t *d_bases, const KswScore &sc, uint8_t *d_state, size_t state_stride, uint8_t *d_path, size_t path_stride,
                           int32_t *d_ez, uint32_t *d_cig, unsigned int *d_counter)
{
	if (n <= 0) return hipSuccess;
	// the exchange words come on top of a state that may fill KSW_LDS_BUDGET: more dynamic LDS than a kernel gets unasked (set per
	// launch: the attribute belongs to the current device)
	hipError_t e = waves == 1 ? hipFuncSetAttribute((const void*)k_ksw_extd<1>, hipFuncAttributeMaxDynamicSharedMemorySize, KSW_LDS_BUDGET + KSW_XCH_BYTES)
	                          : hipFuncSetAttribute((const void*)k_ksw_extd<KSW_WIDE_WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, KSW_LDS_BUDGET + KSW_XCH_BYTES);
	if (e != hipSuccess) return e;
	e = hipMemsetAsync(d_counter, 0, sizeof(unsigned int), st);
	if (e != hipSuccess) return e;
	if (waves == 1)
		hipLaunchKernelGGL(k_ksw_extd<1>, dim3(grid), dim3(64), KSW_XCH_BYTES + lds_bytes, st, n, d_prob, d_order, d_bases, sc, d_state, state_stride,
		                   d_path, path_stride, d_ez, d_cig, d_counter);
	else
		hipLaunchKernelGGL(k_ksw_extd<KSW_WIDE_WAVES>, dim3(grid), dim3(64 * KSW_WIDE_WAVES), KSW_XCH_BYTES + lds_bytes, st, n, d_prob, d_order, d_bases, sc,
		                   d_state, state_stride, d_path, path_stride, d_ez, d_cig, d_counter);
	return hipGetLastError();
}

hipError_t launch_ksw_pack(hipStream_t st, int64_t n, const KswProb *d_prob, const int32_t *d_ez, const int64_t *d_off, const uint32_t *d_cig,
                           uint32_t *d_out)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_ksw_pack, dim3((unsigned)(n < 4096 ? n : 4096)), dim3(64), 0, st, n, d_prob, d_ez, d_off, d_cig, d_out);
	return hipGetLastError();
}

} // namespace chaindp
