// chaindp_post.hip -- what the reference does with a read's hits after mm_gen_regs when nothing is aligned (MM_F_CIGAR unset,
// one segment): chain_post (map.c:238-247: mm_set_parent, mm_select_sub, mm_join_long) and mm_set_mapq (hit.c:437-480), over the
// hits chaindp_gen_regs left in HBM.  mm_est_err sits between the two (map.c:872) and is k_regs_div of chaindp_regs.hip, run on
// this file's output and the anchors as chain_post left them.
//
//   k_post_read     one wave (and one workgroup) per read.  The hits' mutable fields are staged as one int array per field, in LDS
//                   for reads of up to POST_LDS_CAP hits and in a global scratch area (the same code through the same generic
//                   pointers) above.  mm_set_parent's outer loop is sequential; its scan of the primaries is spread over the lanes
//                   (the overlapping ones gathered in w order by ballot, the length of their union without a sort, the first one
//                   that passes the mask test by the lowest lane of a ballot).  mm_select_sub, the join walk of mm_join_long, its
//                   parent fix-up and mm_filter_regs are the reference's in-place loops, run by every lane in step (every lane
//                   computes and stores the same values, so no lane waits for another).  mm_squeeze_a, mm_sync_regs and the fuzzy
//                   lengths of a joined chain use the whole wave.  Output: the read's hits at the positions its input occupied
//                   (slot k at chains_off[r] + k), their count, and the read's anchors as chain_post leaves them.
//   (scan)          exclusive scan of the counts: the CSR offsets of the output (launch_scan_u64)
//   k_post_scatter  wave per read: packs the records
//   k_post_mapq     wave per read, lane per hit: mm_set_mapq with the r->p == NULL branch; sum_sc by a wave reduction.
//
// Types and order of operations follow the reference (float where it computes in float, the one double add of sc_thres, float
// division that rounds correctly -- hipcc's default).  logf of an integer is the host's (post_logf_int).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "chaindp_kernels.h"
#include "chaindp_wave.h"

namespace chaindp {

enum {
	PF_ID, PF_CNT, PF_RID, PF_SCORE, PF_QS, PF_QE, PF_RS, PF_RE, PF_PARENT, PF_SUBSC, PF_AS, PF_MLEN, PF_BLEN, PF_NSUB, PF_BITS,
	PF_ORIG,                                 // the hit's index in the read's mm_gen_regs output (score0, hash, div come from there)
	PF_NREC,                                 // fields that move with a record (mm_reg1_t assignment)
	PF_W = PF_NREC, PF_CP, PF_CS, PF_CE,     // per-slot work arrays: w[] of mm_set_parent / tmp[] of mm_sync_regs, the overlapping
	PF_NF                                    // primaries of one hit (index, clipped start, clipped end)
};
static_assert(PF_NF == POST_SCRATCH_INTS, "global scratch per hit");

#define BIT_REV (1u << 10)
#define BIT_INV (1u << 11)
#define BIT_SAM_PRI (1u << 12)
#define BIT_SEG_SPLIT (1u << 15)
#define POST_PARENT_UNSET (-1)
#define POST_PARENT_TMP_PRI (-2)
#define POST_SEED_LONG_JOIN (1ull << 40)   // mmpriv.h:16

struct PostFields {
	int *base;
	int stride;
	__device__ __forceinline__ int &operator()(int f, int i) const { return base[f * stride + i]; }
};

__device__ __forceinline__ int wave_sum_i(int v)
{
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

__device__ __forceinline__ int wave_max_i(int v)
{
	for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
	return v;
}

// r[k] = r[i] (every lane the same copy)
__device__ __forceinline__ void post_copy(const PostFields &F, int k, int i)
{
	if (k == i) return;
	for (int f = 0; f < PF_NREC; ++f) F(f, k) = F(f, i);
}

// mm_reg_set_coor + mm_cal_fuzzy_len (hit.c:8-38) of slot s over the read's anchors a[]; the anchors by the lanes
__device__ void post_set_coor(const PostFields &F, int s, int qlen, const ulonglong2 *a, int lane)
{
	const int k = F(PF_AS, s), cnt = F(PF_CNT, s);
	const ulonglong2 f = a[k], l = a[k + cnt - 1];
	const int q_span = (int)(f.y >> 32 & 0xff), rev = (int)(f.x >> 63);
	int mlen = 0, blen = 0;
	for (int i = k + 1 + lane; i < k + cnt; i += 64) {
		const ulonglong2 cur = a[i], prev = a[i - 1];
		const int span = (int)(cur.y >> 32 & 0xff);
		const int tl = (int)(int32_t)cur.x - (int)(int32_t)prev.x, ql = (int)(int32_t)cur.y - (int)(int32_t)prev.y;
		blen += tl > ql ? tl : ql;
		mlen += tl > span && ql > span ? span : tl < ql ? tl : ql;
	}
	mlen = wave_sum_i(mlen) + q_span; blen = wave_sum_i(blen) + q_span;
	F(PF_BITS, s) = (F(PF_BITS, s) & ~BIT_REV) | (uint32_t)rev << 10;
	F(PF_RID, s) = (int)(f.x << 1 >> 33);
	F(PF_RS, s) = (int32_t)f.x + 1 > q_span ? (int32_t)f.x + 1 - q_span : 0;
	F(PF_RE, s) = (int32_t)l.x + 1;
	if (!rev) { F(PF_QS, s) = (int32_t)f.y + 1 - q_span; F(PF_QE, s) = (int32_t)l.y + 1; }
	else { F(PF_QS, s) = qlen - ((int32_t)l.y + 1); F(PF_QE, s) = qlen - ((int32_t)f.y + 1 - q_span); }
	F(PF_MLEN, s) = mlen; F(PF_BLEN, s) = blen;
}

// mm_sync_regs + mm_set_sam_pri (hit.c:195-228) of slots [0, n)
__device__ void post_sync_regs(const PostFields &F, int n, int lane)
{
	if (n <= 0) return;
	int mx = -1;
	for (int i = lane; i < n; i += 64) mx = max(mx, F(PF_ID, i));
	mx = wave_max_i(mx);                                   // ids are slot numbers of mm_set_parent: below the read's hit count
	for (int i = lane; i <= mx; i += 64) F(PF_W, i) = -1;
	__syncthreads();
	for (int i = lane; i < n; i += 64) { const int id = F(PF_ID, i); if (id >= 0) F(PF_W, id) = i; }   // ids are distinct
	__syncthreads();
	int first_pri = INT_MAX;
	for (int i = lane; i < n; i += 64) {
		const int p = F(PF_PARENT, i);
		int np;
		if (p == POST_PARENT_TMP_PRI) np = i;
		else if (p >= 0 && p <= mx && F(PF_W, p) >= 0) np = F(PF_W, p);
		else np = POST_PARENT_UNSET;
		F(PF_ID, i) = i; F(PF_PARENT, i) = np;
		if (np == i) first_pri = min(first_pri, i);
	}
	for (int d = 32; d > 0; d >>= 1) first_pri = min(first_pri, __shfl_xor(first_pri, d));
	for (int i = lane; i < n; i += 64) F(PF_BITS, i) = (F(PF_BITS, i) & ~BIT_SAM_PRI) | (i == first_pri ? BIT_SAM_PRI : 0u);
	__syncthreads();
}

// mm_set_parent (hit.c:109-165) with r->p == NULL
__device__ void post_set_parent(const PostFields &F, int n, float mask_level, int lane)
{
	if (n <= 0) return;
	for (int i = lane; i < n; i += 64) F(PF_ID, i) = i;
	__syncthreads();
	F(PF_W, 0) = 0; F(PF_PARENT, 0) = 0;
	int k = 1;
	for (int i = 1; i < n; ++i) {
		const int si = F(PF_QS, i), ei = F(PF_QE, i);
		int n_cov = 0;                                     // the overlapping primaries, clipped, in w order
		for (int base = 0; base < k; base += 64) {
			const int j = base + lane;
			bool ov = false;
			int p = 0, sj = 0, ej = 0;
			if (j < k) { p = F(PF_W, j); sj = F(PF_QS, p); ej = F(PF_QE, p); ov = !(ej <= si || sj >= ei); }
			const uint64_t m = __ballot(ov);
			if (ov) {
				const int idx = n_cov + lanes_below(m);
				F(PF_CP, idx) = p; F(PF_CS, idx) = sj < si ? si : sj; F(PF_CE, idx) = ej > ei ? ei : ej;
			}
			n_cov += __popcll(m);
		}
		int found = -1;
		if (n_cov > 0) {
			__syncthreads();
			// |union of the clipped intervals|: an interval adds what lies beyond the largest end of the intervals before it in
			// (start, end, index) order -- those all start at or before its start, so the part they cover is one piece
			int cov = 0;
			for (int base = 0; base < n_cov; base += 64) {
				const int j = base + lane;
				if (j < n_cov) {
					const int s = F(PF_CS, j), e = F(PF_CE, j);
					int M = s;
					for (int l = 0; l < n_cov; ++l) {
						const int sl = F(PF_CS, l), el = F(PF_CE, l);
						if (sl < s || (sl == s && (el < e || (el == e && l < j)))) M = max(M, el);
					}
					if (e > M) cov += e - M;
				}
			}
			const int uncov_len = (ei - si) - wave_sum_i(cov);
			for (int base = 0; base < n_cov && found < 0; base += 64) {
				const int j = base + lane;
				bool pass = false;
				if (j < n_cov) {
					const int p = F(PF_CP, j), sj = F(PF_QS, p), ej = F(PF_QE, p);
					const int mn = ej - sj < ei - si ? ej - sj : ei - si;
					const int mx = ej - sj > ei - si ? ej - sj : ei - si;
					const int ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
					pass = (float)ol / mn - (float)uncov_len / mx > mask_level;
				}
				const uint64_t m = __ballot(pass);
				if (m) found = F(PF_CP, base + (int)__builtin_ctzll(m));
			}
			__syncthreads();
		}
		if (found >= 0) {
			const int rp = found;
			F(PF_PARENT, i) = F(PF_PARENT, rp);
			const int sc = F(PF_SCORE, i), ss = F(PF_SUBSC, rp);
			F(PF_SUBSC, rp) = ss > sc ? ss : sc;
			if (F(PF_CNT, i) >= F(PF_CNT, rp)) F(PF_NSUB, rp) = F(PF_NSUB, rp) + 1;
		} else {
			F(PF_W, k) = i; F(PF_PARENT, i) = i; F(PF_NSUB, i) = 0;
			++k;
		}
	}
	__syncthreads();
}

// mm_select_sub (hit.c:230-247).  Compacts in place while it reads r[p]: a kept hit may already sit in slot p -- as in the reference.
__device__ int post_select_sub(const PostFields &F, int n, float pri_ratio, int min_diff, int best_n, int lane)
{
	if (!(pri_ratio > 0.0f && n > 0)) return n;
	int k = 0, n_2nd = 0;
	for (int i = 0; i < n; ++i) {
		const int p = F(PF_PARENT, i);
		if (p == i || (F(PF_BITS, i) & BIT_INV)) { post_copy(F, k, i); ++k; continue; }
		if (p < 0 || p >= n) continue;                     // never: every hit has a parent after mm_set_parent
		const int si = F(PF_SCORE, i), sp = F(PF_SCORE, p);
		if (((float)si >= sp * pri_ratio || si + min_diff >= sp) && n_2nd < best_n) {
			if (!(F(PF_QS, i) == F(PF_QS, p) && F(PF_QE, i) == F(PF_QE, p) && F(PF_RID, i) == F(PF_RID, p) && F(PF_RS, i) == F(PF_RS, p) &&
			      F(PF_RE, i) == F(PF_RE, p))) {
				post_copy(F, k, i); ++k; ++n_2nd;
			}
		}
	}
	__syncthreads();
	if (k != n) post_sync_regs(F, k, lane);
	return k;
}

// mm_join_long (hit.c:290-346) with mm_squeeze_a (hit.c:269-288) and mm_filter_regs (hit.c:249-267, r->p == NULL).  b: the read's
// chain anchors as mm_gen_regs saw them; sq: where the read's anchors as chain_post leaves them go (already a copy of b when this
// returns without squeezing).
__device__ int post_join_long(const PostFields &F, int n, const PostOpt &o, int qlen, const ulonglong2 *b, ulonglong2 *sq, int n_b, int lane)
{
	if (n < 2) {
		for (int t = lane; t < n_b; t += 64) sq[t] = b[t];
		return n;
	}
	// mm_squeeze_a: slots in (as, slot) order, each chain's anchors moved down to the running sum of the counts before it.  Its
	// in-place memmove never reads what it has overwritten (sources lie at or above their destinations, in ascending order), so
	// copying from b gives the same array; above the squeezed total the old anchors stay.
	int tot = 0;
	for (int s = lane; s < n; s += 64) tot += F(PF_CNT, s);
	tot = wave_sum_i(tot);
	for (int s = lane; s < n; s += 64) {
		const int as = F(PF_AS, s);
		int nas = 0;
		for (int t = 0; t < n; ++t) { const int at = F(PF_AS, t); if (at < as || (at == as && t < s)) nas += F(PF_CNT, t); }
		F(PF_CS, s) = nas;
	}
	__syncthreads();
	for (int s = 0; s < n; ++s) {
		const int from = F(PF_AS, s), to = F(PF_CS, s), cnt = F(PF_CNT, s);
		for (int t = lane; t < cnt; t += 64) sq[to + t] = b[from + t];
	}
	for (int t = tot + lane; t < n_b; t += 64) sq[t] = b[t];
	__syncthreads();
	for (int s = lane; s < n; s += 64) F(PF_AS, s) = F(PF_CS, s);
	__syncthreads();                                                     // the ranks below read every slot's new `as`
	// the primaries (parent == i or unset) in (as, slot) order -> w[]
	int n_aux = 0;
	for (int s = lane; s < n; s += 64) {
		const int ps = F(PF_PARENT, s);
		if (!(ps == s || ps < 0)) continue;
		const int as = F(PF_AS, s);
		int rank = 0;
		for (int t = 0; t < n; ++t) {
			const int pt = F(PF_PARENT, t);
			if (!(pt == t || pt < 0)) continue;
			const int at = F(PF_AS, t);
			rank += at < as || (at == as && t < s);
		}
		F(PF_W, rank) = s;
		++n_aux;
	}
	n_aux = wave_sum_i(n_aux);
	__syncthreads();
	int n_drop = 0;
	for (int i = n_aux - 1; i >= 1; --i) {
		const int r0 = F(PF_W, i - 1), r1 = F(PF_W, i);
		const int as0 = F(PF_AS, r0), cnt0 = F(PF_CNT, r0), as1 = F(PF_AS, r1);
		if (as0 + cnt0 != as1) continue;
		if (F(PF_RID, r0) != F(PF_RID, r1) || ((F(PF_BITS, r0) ^ F(PF_BITS, r1)) & BIT_REV)) continue;
		const ulonglong2 a0e = sq[as0 + cnt0 - 1], a1s = sq[as1];
		if (a1s.x <= a0e.x || (int32_t)a1s.y <= (int32_t)a0e.y) continue;
		int max_gap, min_gap;
		max_gap = min_gap = (int32_t)a1s.y - (int32_t)a0e.y;
		const unsigned long long dx = a1s.x - a0e.x;                 // the reference compares these as uint64_t
		max_gap = (unsigned long long)(long long)max_gap > dx ? max_gap : (int)dx;
		min_gap = (unsigned long long)(long long)min_gap < dx ? min_gap : (int)dx;
		if (max_gap > o.max_join_long || min_gap > o.max_join_short) continue;
		const int sc_thres = (int)((double)((float)o.min_join_flank_sc / o.max_join_long * max_gap) + .499);
		if (F(PF_SCORE, r0) < sc_thres || F(PF_SCORE, r1) < sc_thres) continue;
		if (F(PF_RE, r0) - F(PF_RS, r0) < max_gap >> 1 || F(PF_QE, r0) - F(PF_QS, r0) < max_gap >> 1) continue;
		if (F(PF_RE, r1) - F(PF_RS, r1) < max_gap >> 1 || F(PF_QE, r1) - F(PF_QS, r1) < max_gap >> 1) continue;
		sq[as1].y = a1s.y | POST_SEED_LONG_JOIN;
		F(PF_CNT, r0) = cnt0 + F(PF_CNT, r1);
		F(PF_SCORE, r0) = F(PF_SCORE, r0) + F(PF_SCORE, r1);
		post_set_coor(F, r0, qlen, sq, lane);
		F(PF_CNT, r1) = 0;
		F(PF_PARENT, r1) = F(PF_ID, r0);
		++n_drop;
	}
	if (n_drop == 0) { __syncthreads(); return n; }
	for (int i = 0; i < n; ++i) {                                        // parent fix-up, in the reference's order
		const int p = F(PF_PARENT, i);
		if (p >= 0 && p < n && F(PF_ID, i) != p) {
			const int pp = F(PF_PARENT, p);
			if (pp >= 0 && pp != p) F(PF_PARENT, i) = pp;
		}
	}
	int k = 0;                                                           // mm_filter_regs
	for (int i = 0; i < n; ++i) {
		const uint32_t bits = (uint32_t)F(PF_BITS, i);
		const bool flt = !(bits & BIT_INV) && !(bits & BIT_SEG_SPLIT) && F(PF_CNT, i) < o.min_cnt;
		if (!flt) { post_copy(F, k, i); ++k; }
	}
	__syncthreads();
	post_sync_regs(F, k, lane);
	return k;
}

template <bool IN_LDS>
__device__ void post_read(int64_t r, const int64_t *__restrict__ chains_off, const int64_t *__restrict__ b_off, const ulonglong2 *__restrict__ b,
                          const int32_t *__restrict__ regs, const int32_t *__restrict__ qlen, PostOpt o, int32_t *__restrict__ scratch,
                          int32_t *__restrict__ stage, ulonglong2 *__restrict__ sq, unsigned long long *__restrict__ n_out, int *lds)
{
	const int lane = threadIdx.x & 63;
	const int64_t c0 = chains_off[r];
	const int n0 = (int)(chains_off[r + 1] - c0);
	const int64_t a0 = b_off[r];
	const int n_b = (int)(b_off[r + 1] - a0);
	PostFields F;
	if (IN_LDS) { F.base = lds; F.stride = POST_LDS_CAP; }
	else { F.base = scratch + c0 * PF_NF; F.stride = n0; }
	const int32_t *in = regs + c0 * 20;
	for (int s = lane; s < n0; s += 64) {
		const int32_t *g = in + s * 20;
		F(PF_ID, s) = g[0]; F(PF_CNT, s) = g[1]; F(PF_RID, s) = g[2]; F(PF_SCORE, s) = g[3]; F(PF_QS, s) = g[4]; F(PF_QE, s) = g[5];
		F(PF_RS, s) = g[6]; F(PF_RE, s) = g[7]; F(PF_PARENT, s) = g[8]; F(PF_SUBSC, s) = g[9]; F(PF_AS, s) = g[10]; F(PF_MLEN, s) = g[11];
		F(PF_BLEN, s) = g[12]; F(PF_NSUB, s) = g[13]; F(PF_BITS, s) = g[15]; F(PF_ORIG, s) = s;
	}
	__syncthreads();
	int n = n0;
	const ulonglong2 *ba = b + a0;
	ulonglong2 *sa = sq + a0;
	if (!(o.flag & POST_F_ALL_CHAINS)) {                                 // chain_post, map.c:238-247
		post_set_parent(F, n, o.mask_level, lane);
		n = post_select_sub(F, n, o.pri_ratio, o.min_diff, o.best_n, lane);
		if (!(o.flag & (POST_F_SPLICE | POST_F_SR | POST_F_NO_LJOIN))) n = post_join_long(F, n, o, qlen[r], ba, sa, n_b, lane);
		else for (int t = lane; t < n_b; t += 64) sa[t] = ba[t];
	} else {
		for (int t = lane; t < n_b; t += 64) sa[t] = ba[t];
	}
	for (int s = lane; s < n; s += 64) {
		const int32_t *g = in + F(PF_ORIG, s) * 20;
		int32_t *d = stage + (c0 + s) * 20;
		d[0] = F(PF_ID, s); d[1] = F(PF_CNT, s); d[2] = F(PF_RID, s); d[3] = F(PF_SCORE, s); d[4] = F(PF_QS, s); d[5] = F(PF_QE, s);
		d[6] = F(PF_RS, s); d[7] = F(PF_RE, s); d[8] = F(PF_PARENT, s); d[9] = F(PF_SUBSC, s); d[10] = F(PF_AS, s); d[11] = F(PF_MLEN, s);
		d[12] = F(PF_BLEN, s); d[13] = F(PF_NSUB, s); d[14] = g[14]; d[15] = F(PF_BITS, s); d[16] = g[16]; d[17] = g[17]; d[18] = g[18]; d[19] = g[19];
	}
	if (lane == 0) n_out[r] = (unsigned long long)n;
}

__global__ __launch_bounds__(64) void k_post_read(int64_t n_reads, const int64_t *__restrict__ chains_off, const int64_t *__restrict__ b_off,
                                                  const ulonglong2 *__restrict__ b, const int32_t *__restrict__ regs, const int32_t *__restrict__ qlen,
                                                  PostOpt o, int32_t *__restrict__ scratch, int32_t *__restrict__ stage, ulonglong2 *__restrict__ sq,
                                                  unsigned long long *__restrict__ n_out)
{
	__shared__ int lds[PF_NF * POST_LDS_CAP];
	const int64_t r = blockIdx.x;
	if (r >= n_reads) return;
	const int64_t n = chains_off[r + 1] - chains_off[r];
	if (n <= POST_LDS_CAP) post_read<true>(r, chains_off, b_off, b, regs, qlen, o, scratch, stage, sq, n_out, lds);
	else post_read<false>(r, chains_off, b_off, b, regs, qlen, o, scratch, stage, sq, n_out, lds);
}

__global__ __launch_bounds__(256) void k_post_scatter(int64_t n_reads, const int64_t *__restrict__ chains_off, const unsigned long long *__restrict__ out_off,
                                                      const int32_t *__restrict__ stage, int32_t *__restrict__ out)
{
	const int lane = threadIdx.x & 63;
	const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (r >= n_reads) return;
	const int64_t o0 = (int64_t)out_off[r], words = ((int64_t)out_off[r + 1] - o0) * 20;
	const int32_t *src = stage + chains_off[r] * 20;
	int32_t *dst = out + o0 * 20;
	for (int64_t t = lane; t < words; t += 64) dst[t] = src[t];
}

// logf of an integer as the host computes it: the correctly rounded (float)log((double)k) -- log(k) stays more than 5 double ulp away
// from every float rounding midpoint for k <= 2^24 -- except at the integers the host lists, where its logf rounds the other way
__device__ __forceinline__ float post_logf_int(int k, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch)
{
	const float c = (float)log((double)k);
	if (k < 1 || k > POST_LOGF_MAX) return c;
	int lo = 0, hi = n_patch - 1;
	while (lo <= hi) {
		const int mid = (lo + hi) >> 1;
		const uint32_t m = pk[mid];
		if (m == (uint32_t)k) return pv[mid];
		if (m < (uint32_t)k) lo = mid + 1; else hi = mid - 1;
	}
	return c;
}

// (int)f as the reference's x86-64 build converts it (cvttss2si): INT_MIN for NaN and for anything outside the int range
__device__ __forceinline__ int post_f2i(float f)
{
	if (!(f > -2147483904.0f && f < 2147483648.0f)) return INT_MIN;
	return (int)f;
}

// (int)(4.343f * logf(n_sub + 1) + .499f) of hit.c:474: a float add of .499f (for n_sub + 1 <= 2^24 a double add differs from it at 119
// integers, the first 141 265 -- beyond what a fixture reaches; chaindp_post_logf_selftest checks this term over the whole range)
__device__ __forceinline__ int post_nsub_term(int k, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch)
{
	return post_f2i(4.343f * post_logf_int(k, pk, pv, n_patch) + .499f);
}

// mm_set_mapq (hit.c:437-480) with r->p == NULL; mm_set_inv_mapq is a no-op here (no hit has its inv bit without alignment, and
// the inv branch is kept for completeness).  err: set when a logf argument lies beyond the patch list.
__global__ __launch_bounds__(256) void k_post_mapq(int64_t n_reads, const unsigned long long *__restrict__ out_off, const int32_t *__restrict__ rep_len,
                                                   int min_chain_sc, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch,
                                                   int32_t *__restrict__ out, int32_t *__restrict__ err)
{
	const int lane = threadIdx.x & 63;
	const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (r >= n_reads) return;
	const int64_t o0 = (int64_t)out_off[r];
	const int n = (int)((int64_t)out_off[r + 1] - o0);
	int32_t *regs = out + o0 * 20;
	long long sum_sc = 0;
	for (int i = lane; i < n; i += 64) if (regs[i * 20 + 8] == regs[i * 20]) sum_sc += regs[i * 20 + 3];
	for (int d = 32; d > 0; d >>= 1) sum_sc += __shfl_xor(sum_sc, d);
	const float uniq_ratio = (float)sum_sc / (float)(sum_sc + rep_len[r]);
	for (int i = lane; i < n; i += 64) {
		int32_t *g = regs + i * 20;
		const uint32_t bits = (uint32_t)g[15];
		int mapq_out;
		if (bits & BIT_INV) {
			mapq_out = 0;
		} else if (g[8] == g[0]) {
			const int score = g[3], cnt = g[1], n_sub = g[13];
			if (score > POST_LOGF_MAX || n_sub + 1 > POST_LOGF_MAX) *err = 1;
			const float pen_s1 = (score > 100 ? 1.0f : 0.01f * (float)score) * uniq_ratio;
			float pen_cm = cnt > 10 ? 1.0f : 0.1f * (float)cnt;
			pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
			const int subsc = g[9] > min_chain_sc ? g[9] : min_chain_sc;
			const float x = (float)subsc / (float)g[14];
			const float q = pen_cm * 40.0f * (1.0f - x) * post_logf_int(score, pk, pv, n_patch);
			int mapq = post_f2i(q);
			const int sub = post_nsub_term(n_sub + 1, pk, pv, n_patch);
			mapq = (int)((uint32_t)mapq - (uint32_t)sub);               // wraps as the reference's int subtraction does on x86
			mapq = mapq > 0 ? mapq : 0;
			mapq_out = mapq < 60 ? mapq : 60;
		} else {
			mapq_out = 0;
		}
		g[15] = (int32_t)((bits & ~0xffu) | ((uint32_t)mapq_out & 0xffu));
	}
}

// the device half of the logf self-test: out[k - 1] = post_logf_int(k), term[k - 1] = post_nsub_term(k) for k in [1, kmax]
__global__ __launch_bounds__(256) void k_post_logf_probe(int kmax, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch,
                                                         float *__restrict__ out, int32_t *__restrict__ term)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= kmax) return;
	out[g] = post_logf_int((int)g + 1, pk, pv, n_patch);
	term[g] = post_nsub_term((int)g + 1, pk, pv, n_patch);
}

hipError_t launch_post_read(hipStream_t st, int64_t n_reads, const int64_t *d_chains_off, const int64_t *d_b_off, const void *d_b, const void *d_regs,
                            const int32_t *d_qlen, const PostOpt &o, int32_t *d_scratch, void *d_stage, void *d_sq, unsigned long long *d_n_out)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_read, dim3((unsigned)n_reads), dim3(64), 0, st, n_reads, d_chains_off, d_b_off, (const ulonglong2*)d_b,
	                   (const int32_t*)d_regs, d_qlen, o, d_scratch, (int32_t*)d_stage, (ulonglong2*)d_sq, d_n_out);
	return hipGetLastError();
}

hipError_t launch_post_scatter(hipStream_t st, int64_t n_reads, const int64_t *d_chains_off, const unsigned long long *d_out_off, const void *d_stage,
                               void *d_out)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_scatter, dim3((unsigned)((n_reads * 64 + 255) / 256)), dim3(256), 0, st, n_reads, d_chains_off, d_out_off,
	                   (const int32_t*)d_stage, (int32_t*)d_out);
	return hipGetLastError();
}

hipError_t launch_post_mapq(hipStream_t st, int64_t n_reads, const unsigned long long *d_out_off, const int32_t *d_rep_len, int min_chain_sc,
                            const uint32_t *d_pk, const float *d_pv, int n_patch, void *d_out, int32_t *d_err)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_mapq, dim3((unsigned)((n_reads * 64 + 255) / 256)), dim3(256), 0, st, n_reads, d_out_off, d_rep_len, min_chain_sc,
	                   d_pk, d_pv, n_patch, (int32_t*)d_out, d_err);
	return hipGetLastError();
}

hipError_t launch_post_logf_probe(hipStream_t st, int kmax, const uint32_t *d_pk, const float *d_pv, int n_patch, float *d_out, int32_t *d_term)
{
	if (kmax <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_logf_probe, dim3((unsigned)((kmax + 255) / 256)), dim3(256), 0, st, kmax, d_pk, d_pv, n_patch, d_out, d_term);
	return hipGetLastError();
}

} // namespace chaindp
