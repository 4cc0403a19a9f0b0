// chaindp_post_dev.h -- the device functions of chain_post (map.c:238-247) over one read's hits, staged as one int array per field:
// mm_set_parent, mm_select_sub, mm_sync_regs, mm_join_long (with mm_squeeze_a and mm_filter_regs) and mm_reg_set_coor.  Shared by
// k_post_read (chaindp_post.hip: single-segment reads) and the fragment kernels (chaindp_frag.hip: reads of several segments).
// Every function is run by one whole wave; "every lane the same" steps compute and store the same values in every lane.
#ifndef CHAINDP_POST_DEV_H
#define CHAINDP_POST_DEV_H

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
// integers, the first 141 265 -- reached through r[0].n_sub, which mm_set_parent never resets: the nsub_term scene of the align-post
// edge tier sits on it; chaindp_post_logf_selftest checks this term over the whole range)
__device__ __forceinline__ int post_nsub_term(int k, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch)
{
	return post_f2i(4.343f * post_logf_int(k, pk, pv, n_patch) + .499f);
}

} // namespace chaindp
#endif
