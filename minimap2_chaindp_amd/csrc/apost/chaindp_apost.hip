// apost/chaindp_apost.hip -- what the reference does with a read's regions once they carry alignments: the tail of align_regs
// (map.c:253-257: mm_set_parent with r->p, mm_select_sub, mm_set_sam_pri) and mm_set_mapq with mm_set_inv_mapq (map.c:876,
// hit.c:411-480), over the regions chaindp_align_reads left in HBM or a caller handed in.
//
//   k_apost_read        one wave (and one workgroup) per read, all of the steps above in the one launch: nothing from outside the read
//                       sits between them.  The regions' mutable fields are staged as one int array per field (chaindp_post_dev.h's
//                       PostFields), in LDS for lists of up to lds_cap regions and in global scratch, through the same code, above.
//                       What r->p holds (has_p, dp_max, dp_max2) and score0 do not move with a record: they stay at the region's
//                       input place and are reached through PF_ORIG.  mm_set_parent's scan of the primaries is spread over the lanes
//                       as post_set_parent spreads it; mm_select_sub and mm_sync_regs are chaindp_post_dev.h's.  mm_set_mapq is a
//                       lane per region with sum_sc by a wave reduction; mm_set_inv_mapq ranks the primaries by (as, i) by counting
//                       and walks them in step.  Output: the survivors' records at the places the read's input occupied, their
//                       dp_max2, input index and the CIGAR words before them in the read; per read the count and the word total.
//   (scans)             exclusive scans of the counts and the words: out_off and the reads' first CIGAR word (launch_scan_u64)
//   k_apost_gather      a wave per read: records, extras, dp_max2 and cigar_off into final order
//   k_apost_gather_cig  a wave per final region: its CIGAR words; a dropped region leaves none behind and no hole
//
// Types and order of operations follow the reference (float where it computes in float, left to right, no fused operation, float
// division that rounds correctly).  logf of an integer is post_logf_int's; logf((float)dp_max / match_sc) is the correctly rounded
// (float)log((double)x) except at the dp_max the host lists for the call's match_sc (chaindp_apost_plan.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "../chaindp_kernels.h"
#include "../chaindp_wave.h"
#include "../chaindp_post_dev.h"
#include "../chaindp_apost_plan.h"

namespace chaindp {

enum { AF_HASP = PF_NF, AF_DPMAX, AF_DPMAX2, AF_SCORE0, AF_NF };     // indexed by the region's input place in its read (PF_ORIG)
static_assert(AF_NF == AP_NF, "ints per staged region");
static_assert(PF_ID == 0 && PF_NSUB == 13 && PF_BITS == 14, "a region's first fourteen words are the first fourteen fields");
static_assert(AP_LOGF_MAX == POST_LOGF_MAX, "one range for both patch lists");

// a value every lane holds the same, into scalar registers: what a read's lanes share (its offsets and counts) costs no vector register
__device__ __forceinline__ int ap_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t ap_uniform64(int64_t v)
{
	return (int64_t)((uint64_t)(uint32_t)ap_uniform((int)((uint64_t)v >> 32)) << 32 | (uint32_t)ap_uniform((int)(uint32_t)v));
}

// mm_set_parent (hit.c:109-165) with the r->p branch of hit.c:152-155.  Runs before anything moves a record: PF_ORIG(s) == s.
__device__ void apost_set_parent(const PostFields &F, int n, float mask_level, int sub_diff, int lane)
{
	if (n <= 0) return;
	for (int i = lane; i < n; i += 64) F(PF_ID, i) = i;
	__syncthreads();
	F(PF_W, 0) = 0; F(PF_PARENT, 0) = 0;                    // neither r[0].n_sub nor any subsc is reset, as in the reference
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
			// |union of the clipped intervals|, as post_set_parent counts it
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
		if (found >= 0) {                                  // every lane the same
			const int rp = found;
			F(PF_PARENT, i) = F(PF_PARENT, rp);
			const int sc = F(PF_SCORE, i), ss = F(PF_SUBSC, rp);
			F(PF_SUBSC, rp) = ss > sc ? ss : sc;
			bool cnt_sub = F(PF_CNT, i) >= F(PF_CNT, rp);
			if (F(AF_HASP, rp) && F(AF_HASP, i)) {
				const int sj = F(PF_QS, rp), ej = F(PF_QE, rp);
				const int mn = ej - sj < ei - si ? ej - sj : ei - si;
				const int ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
				if (F(PF_RID, rp) != F(PF_RID, i) || F(PF_RS, rp) != F(PF_RS, i) || F(PF_RE, rp) != F(PF_RE, i) || ol != mn) {   // not identical hits after DP
					const int di = F(AF_DPMAX, i), d2 = F(AF_DPMAX2, rp);
					F(AF_DPMAX2, rp) = d2 > di ? d2 : di;
					if ((int)((uint32_t)F(AF_DPMAX, rp) - (uint32_t)di) <= sub_diff) cnt_sub = true;
				}
			}
			if (cnt_sub) F(PF_NSUB, rp) = F(PF_NSUB, rp) + 1;
		} else {
			F(PF_W, k) = i; F(PF_PARENT, i) = i; F(PF_NSUB, i) = 0;
			++k;
		}
	}
	__syncthreads();
}

// mm_set_sam_pri (hit.c:195-204)
__device__ void apost_set_sam_pri(const PostFields &F, int n, int lane)
{
	int first_pri = INT_MAX;
	for (int i = lane; i < n; i += 64) if (F(PF_ID, i) == F(PF_PARENT, i)) first_pri = min(first_pri, i);
	for (int d = 32; d > 0; d >>= 1) first_pri = min(first_pri, __shfl_xor(first_pri, d));
	for (int i = lane; i < n; i += 64) F(PF_BITS, i) = (F(PF_BITS, i) & ~BIT_SAM_PRI) | (i == first_pri ? BIT_SAM_PRI : 0u);
	__syncthreads();
}

// logf(x) as the host computes it, for the float x that `key` stands for under the list (lk, lv): (float)key under post_logf_int's list
// (exact up to 2^24, so this is post_logf_int(key)), or (float)dp_max / match_sc under the list of the call's match_sc.  The correctly
// rounded (float)log((double)x) except at the listed keys.
__device__ __forceinline__ float apost_logf(float x, int key, const uint32_t *__restrict__ lk, const float *__restrict__ lv, int n_list)
{
	const float c = (float)log((double)x);
	if (key < 1 || key > AP_LOGF_MAX) return c;
	int lo = 0, hi = n_list - 1;
	while (lo <= hi) {
		const int mid = (lo + hi) >> 1;
		const uint32_t m = lk[mid];
		if (m == (uint32_t)key) return lv[mid];
		if (m < (uint32_t)key) lo = mid + 1; else hi = mid - 1;
	}
	return c;
}

// mm_set_mapq (hit.c:437-480) with both of its r->p branches, and mm_set_inv_mapq (hit.c:411-435)
__device__ void apost_set_mapq(const PostFields &F, int n, const PostOpt &o, int rep_len, const ApostDev &d, int lane)
{
	long long sum_sc = 0;
	for (int i = lane; i < n; i += 64) if (F(PF_PARENT, i) == F(PF_ID, i)) sum_sc += F(PF_SCORE, i);
	for (int s = 32; s > 0; s >>= 1) sum_sc += __shfl_xor(sum_sc, s);
	const float uniq_ratio = (float)sum_sc / (float)(sum_sc + rep_len);
	// The logarithms first, in a loop that keeps little else alive (the double logarithm is the costliest code of the kernel): the one of
	// the primary's branch (hit.c:460, 469, 471) into cs[], the n_sub term of hit.c:474 into ce[]
	for (int i = lane; i < n; i += 64) {
		if (((uint32_t)F(PF_BITS, i) & BIT_INV) || F(PF_PARENT, i) != F(PF_ID, i)) continue;
		const int at = F(PF_ORIG, i), n_sub = F(PF_NSUB, i);
		const bool has_p = F(AF_HASP, at) != 0;
		const int key = has_p ? F(AF_DPMAX, at) : F(PF_SCORE, i);
		if (n_sub + 1 > POST_LOGF_MAX || key > POST_LOGF_MAX) *d.err = 1;
		const float x = has_p ? (float)key / (float)o.match_sc : (float)key;
		F(PF_CS, i) = __float_as_int(apost_logf(x, key, has_p ? d.dp_k : d.logf_k, has_p ? d.dp_v : d.logf_v, has_p ? d.n_dp : d.n_logf));
		F(PF_CE, i) = post_nsub_term(n_sub + 1, d.logf_k, d.logf_v, d.n_logf);
	}
	bool inv = false;
	for (int i = lane; i < n; i += 64) {
		const uint32_t bits = (uint32_t)F(PF_BITS, i);
		int mapq_out = 0;
		if (bits & BIT_INV) {
			inv = true;
		} else if (F(PF_PARENT, i) == F(PF_ID, i)) {
			const int at = F(PF_ORIG, i);
			const int score = F(PF_SCORE, i), cnt = F(PF_CNT, i), score0 = F(AF_SCORE0, at);
			const int has_p = F(AF_HASP, at), dp_max = F(AF_DPMAX, at), dp_max2 = F(AF_DPMAX2, at);
			const float pen_s1 = (score > 100 ? 1.0f : 0.01f * (float)score) * uniq_ratio;
			float pen_cm = cnt > 10 ? 1.0f : 0.1f * (float)cnt;
			pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
			const int subsc = F(PF_SUBSC, i) > o.min_chain_score ? F(PF_SUBSC, i) : o.min_chain_score;
			int mapq;
			const float lg = __int_as_float(F(PF_CS, i));
			if (has_p && dp_max2 > 0 && dp_max > 0) {
				const float identity = (float)F(PF_MLEN, i) / (float)F(PF_BLEN, i);
				const float x = (float)dp_max2 * (float)subsc / (float)dp_max / (float)score0;
				mapq = post_f2i(identity * pen_cm * 40.0f * (1.0f - x * x) * lg);
				if (!o.is_sr) {
					const int mapq_alt = post_f2i(6.02f * identity * identity * (float)(dp_max - dp_max2) / (float)o.match_sc + .499f);
					mapq = mapq < mapq_alt ? mapq : mapq_alt;
				}
			} else {
				const float x = (float)subsc / (float)score0;
				if (has_p) {
					const float identity = (float)F(PF_MLEN, i) / (float)F(PF_BLEN, i);
					mapq = post_f2i(identity * pen_cm * 40.0f * (1.0f - x) * lg);
				} else {
					mapq = post_f2i(pen_cm * 40.0f * (1.0f - x) * lg);
				}
			}
			const int sub = F(PF_CE, i);
			mapq = (int)((uint32_t)mapq - (uint32_t)sub);               // wraps as the reference's int subtraction does on x86
			mapq = mapq > 0 ? mapq : 0;
			mapq_out = mapq < 60 ? mapq : 60;
			if (has_p && dp_max > dp_max2 && mapq_out == 0) mapq_out = 1;
		}
		F(PF_BITS, i) = (int)((bits & ~0xffu) | ((uint32_t)mapq_out & 0xffu));
	}
	__syncthreads();
	if (n < 3 || !__ballot(inv)) return;                     // mm_set_inv_mapq: wave-uniform
	// the primaries (parent == i or unset) in (as, i) order -> w[]
	int n_aux = 0;
	for (int s = lane; s < n; s += 64) {
		const int ps = F(PF_PARENT, s);
		if (!(ps == s || ps < 0)) continue;
		const uint32_t as = (uint32_t)F(PF_AS, s);
		int rank = 0;
		for (int t = 0; t < n; ++t) {
			const int pt = F(PF_PARENT, t);
			if (!(pt == t || pt < 0)) continue;
			const uint32_t at = (uint32_t)F(PF_AS, t);
			rank += at < as || (at == as && t < s);
		}
		F(PF_W, rank) = s;
		++n_aux;
	}
	n_aux = wave_sum_i(n_aux);
	__syncthreads();
	for (int i = 1; i < n_aux - 1; ++i) {                    // every lane the same; an inversion may neighbour one already set
		const int v = F(PF_W, i);
		const uint32_t bits = (uint32_t)F(PF_BITS, v);
		if (!(bits & BIT_INV)) continue;
		const uint32_t ml = (uint32_t)F(PF_BITS, F(PF_W, i - 1)) & 0xffu, mr = (uint32_t)F(PF_BITS, F(PF_W, i + 1)) & 0xffu;
		F(PF_BITS, v) = (int)((bits & ~0xffu) | (ml < mr ? ml : mr));
	}
	__syncthreads();
}

template <bool IN_LDS>
__device__ void apost_read(int64_t r, const PostOpt &o, const ApostDev &d, int *lds)
{
	const int lane = threadIdx.x & 63;
	const int64_t g0 = ap_uniform64(d.regs_off[r]);
	const int n0 = ap_uniform((int)(d.regs_off[r + 1] - g0));
	PostFields F;
	if (IN_LDS) { F.base = lds; F.stride = AP_LDS_CAP; }
	else { F.base = d.scratch + g0 * AF_NF; F.stride = n0; }
	const int32_t *in = d.regs + g0 * AP_REG_WORDS;
	const int32_t *ex = d.extra + g0 * AP_EXTRA_WORDS;
	// a region's words 0..13 are the fields PF_ID..PF_NSUB in their order; 14 is score0, 15 the bit-field word
	for (int t = lane; t < n0 * AP_REG_WORDS; t += 64) {
		const int s = t / AP_REG_WORDS, w = t - s * AP_REG_WORDS;
		const int32_t v = in[t];
		if (w < PF_BITS) F(w, s) = v;
		else if (w == 14) F(AF_SCORE0, s) = v;
		else if (w == 15) F(PF_BITS, s) = v;
	}
	for (int s = lane; s < n0; s += 64) {
		F(PF_ORIG, s) = s; F(AF_HASP, s) = ex[s * AP_EXTRA_WORDS]; F(AF_DPMAX, s) = ex[s * AP_EXTRA_WORDS + 2]; F(AF_DPMAX2, s) = 0;
	}
	__syncthreads();
	int n = n0;
	if (!(o.flag & POST_F_ALL_CHAINS)) {                                 // map.c:253-257
		apost_set_parent(F, n, o.mask_level, o.sub_diff, lane);
		n = post_select_sub(F, n, o.pri_ratio, o.min_diff, o.best_n, lane);
		apost_set_sam_pri(F, n, lane);
	}
	apost_set_mapq(F, n, o, ap_uniform(d.rep_len[r]), d, lane);                      // map.c:876
	long long words = 0;
	for (int s0 = 0; s0 < n; s0 += 64) {
		const int s = s0 + lane;
		int m = 0, at = 0;
		if (s < n) { at = F(PF_ORIG, s); m = max(ex[at * AP_EXTRA_WORDS + 4], 0); }
		int incl = m;
		for (int k = 1; k < 64; k <<= 1) { const int v = __shfl_up(incl, k); if (lane >= k) incl += v; }
		if (s < n) { d.st_dp2[g0 + s] = F(AF_DPMAX2, at); d.st_src[g0 + s] = at; d.st_wpre[g0 + s] = (int32_t)(words + incl - m); }
		words += __shfl(incl, 63);
	}
	int32_t *st = d.st_regs + g0 * AP_REG_WORDS;
	for (int t = lane; t < n * AP_REG_WORDS; t += 64) {
		const int s = t / AP_REG_WORDS, w = t - s * AP_REG_WORDS;
		st[t] = w < PF_BITS ? F(w, s) : w == 15 ? F(PF_BITS, s) : in[F(PF_ORIG, s) * AP_REG_WORDS + w];
	}
	if (lane == 0) { d.cnt[r] = (unsigned long long)n; d.words[r] = (unsigned long long)words; }
}

__global__ __launch_bounds__(64, 8) void k_apost_read(PostOpt o, ApostDev d, int lds_cap)
{
	__shared__ int lds[AF_NF * AP_LDS_CAP];
	const int64_t r = blockIdx.x;                                        // one read per workgroup: nothing is carried from read to read
	if (r >= d.n_reads) return;
	const int64_t n = ap_uniform64(d.regs_off[r + 1] - d.regs_off[r]);
	if (n <= lds_cap) apost_read<true>(r, o, d, lds);
	else apost_read<false>(r, o, d, lds);
}

__global__ __launch_bounds__(64) void k_apost_gather(ApostDev d)
{
	const int lane = threadIdx.x;
	const int64_t *out_off = (const int64_t*)d.cnt, *word_off = (const int64_t*)d.words;
	if (blockIdx.x == 0 && lane == 0) {
		const int64_t total = out_off[d.n_reads];
		d.need[0] = total; d.need[1] = word_off[d.n_reads];
		d.out_cigar_off[total] = word_off[d.n_reads];
	}
	for (int64_t r = blockIdx.x; r < d.n_reads; r += gridDim.x) {
		const int64_t g0 = d.regs_off[r], f0 = out_off[r], w0 = word_off[r];
		const int64_t n = out_off[r + 1] - f0;
		const int32_t *src = d.st_regs + g0 * AP_REG_WORDS;
		int32_t *dst = d.out_regs + f0 * AP_REG_WORDS;
		for (int64_t t = lane; t < n * AP_REG_WORDS; t += 64) dst[t] = src[t];
		for (int64_t t = lane; t < n * AP_EXTRA_WORDS; t += 64) {
			const int64_t s = t / AP_EXTRA_WORDS;
			const int w = (int)(t - s * AP_EXTRA_WORDS);
			d.out_extra[(f0 + s) * AP_EXTRA_WORDS + w] = d.extra[(g0 + d.st_src[g0 + s]) * AP_EXTRA_WORDS + w];
		}
		for (int64_t s = lane; s < n; s += 64) {
			d.out_dp2[f0 + s] = d.st_dp2[g0 + s];
			d.out_cigar_off[f0 + s] = w0 + d.st_wpre[g0 + s];
			d.fsrc[f0 + s] = g0 + d.st_src[g0 + s];
		}
	}
}

// a wave per final region: a CIGAR is a few words to a few hundred
__global__ __launch_bounds__(64) void k_apost_gather_cig(ApostDev d)
{
	const int64_t total = d.need[0];
	for (int64_t f = blockIdx.x; f < total; f += gridDim.x) {
		const int64_t m = d.out_cigar_off[f + 1] - d.out_cigar_off[f];
		const uint32_t *from = d.cig + d.cigar_off[d.fsrc[f]];
		uint32_t *to = d.out_cig + d.out_cigar_off[f];
		for (int64_t c = threadIdx.x; c < m; c += 64) to[c] = from[c];
	}
}

__global__ __launch_bounds__(256) void k_apost_logf_probe(int kmax, int match_sc, const uint32_t *__restrict__ dk, const float *__restrict__ dv, int n_dp,
                                                          float *__restrict__ out)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= kmax) return;
	out[g] = apost_logf((float)((int)g + 1) / (float)match_sc, (int)g + 1, dk, dv, n_dp);
}

static unsigned apost_grid(int64_t n) { return (unsigned)(n < 1 ? 1 : n < 65536 ? n : 65536); }

hipError_t launch_apost_read(hipStream_t st, const PostOpt &o, const ApostDev &d, int lds_cap)
{
	if (d.n_reads <= 0) return hipSuccess;
	if (d.n_reads > 0x7fffffff) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_apost_read, dim3((unsigned)d.n_reads), dim3(64), 0, st, o, d, lds_cap < AP_LDS_CAP ? lds_cap : AP_LDS_CAP);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	if ((e = launch_scan_u64(st, d.n_reads, d.cnt, d.tile, d.cnt + d.n_reads)) != hipSuccess) return e;
	return launch_scan_u64(st, d.n_reads, d.words, d.tile, d.words + d.n_reads);
}

hipError_t launch_apost_gather(hipStream_t st, const ApostDev &d)
{
	if (d.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_apost_gather, dim3(apost_grid(d.n_reads)), dim3(64), 0, st, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess || d.n_regs <= 0) return e;
	hipLaunchKernelGGL(k_apost_gather_cig, dim3(apost_grid(d.n_regs)), dim3(64), 0, st, d);
	return hipGetLastError();
}

hipError_t launch_apost_logf_probe(hipStream_t st, int kmax, int match_sc, const uint32_t *d_k, const float *d_v, int n, float *d_out)
{
	if (kmax <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_apost_logf_probe, dim3((unsigned)((kmax + 255) / 256)), dim3(256), 0, st, kmax, match_sc, d_k, d_v, n, d_out);
	return hipGetLastError();
}

} // namespace chaindp
