// chaindp_apost_plan.h -- what the host decides about a chaindp_align_post call (the tail of align_regs, map.c:253-257, and mm_set_mapq,
// map.c:876, over regions that carry alignments): the argument checks, where the pieces of the staged batch lie in their device
// buffers, and the list of the dp_max at which the host's logf((float)dp_max / match_sc) is not what the device computes by itself.
// No HIP in here, as chaindp_reads_plan.h: a stand-alone program runs it under the sanitizers.
#ifndef CHAINDP_APOST_PLAN_H
#define CHAINDP_APOST_PLAN_H
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

namespace chaindp {

#define AP_LDS_CAP 48                 // regions of a read k_apost_read stages in LDS (AP_NF ints each: 4.5 KB, so that LDS leaves room for eight
                                      // one-wave workgroups per SIMD); longer lists take the global route
#define AP_NF 24                      // ints per staged region: the 20 of chaindp_post_dev.h's PF_NF, then has_p, dp_max, dp_max2, score0
#define AP_LOGF_MAX (1 << 24)         // the patch list covers dp_max up to here
#define AP_F_SPLICE 0x080
#define AP_F_SR 0x1000
#define AP_REG_WORDS 20
#define AP_EXTRA_WORDS 5              // chaindp_align_extra_t: has_extra, dp_score, dp_max, n_ambi, n_cigar

struct ApostOpt {                     // chaindp_post_opt_t, word for word
	int32_t flag;
	float mask_level, pri_ratio;
	int32_t best_n, min_diff, sub_diff, max_join_long, max_join_short, min_join_flank_sc, min_cnt, min_chain_score, match_sc, is_sr;
};

// The call's own arguments.  0, or -1 with err.
inline int apost_check_call(const ApostOpt *o, int64_t n_reads, const int32_t *rep_len, int64_t regs_cap, int64_t cigar_cap, bool has_out_off_need,
                            bool has_reg_arrays, bool has_cigar, std::string &err)
{
	if (!o) { err = "NULL opt"; return -1; }
	if (o->flag & (AP_F_SR | AP_F_SPLICE)) { err = "MM_F_SR and MM_F_SPLICE are not supported"; return -1; }
	if (o->match_sc <= 0) { err = "match_sc must be positive"; return -1; }
	if (n_reads < 0) { err = "negative n_reads"; return -1; }
	if (n_reads > 0 && !rep_len) { err = "NULL rep_len"; return -1; }
	for (int64_t r = 0; r < n_reads; ++r)
		if (rep_len[r] < 0) { err = "negative rep_len of read " + std::to_string((long long)r); return -1; }
	if (!has_out_off_need) { err = "NULL out_off or need"; return -1; }
	if (regs_cap < 0 || cigar_cap < 0) { err = "negative capacity"; return -1; }
	if ((regs_cap > 0 && !has_reg_arrays) || (cigar_cap > 0 && !has_cigar)) { err = "a capacity without its arrays"; return -1; }
	return 0;
}

// The regions a caller hands in from the host (chaindp_align_post_regs): CSR over the reads, the extras, CSR of the CIGAR words.  0 with
// n_regs and n_words, or -1 with err.
inline int apost_check_regs(int64_t n_reads, const int64_t *regs_off, const int32_t *regs, const int32_t *extra, const int64_t *cigar_off, const uint32_t *cigar,
                            int64_t &n_regs, int64_t &n_words, std::string &err)
{
	n_regs = n_words = 0;
	if (n_reads == 0) return 0;
	if (!regs_off) { err = "NULL regs_off"; return -1; }
	if (regs_off[0] != 0) { err = "regs_off does not start at 0"; return -1; }
	for (int64_t r = 0; r < n_reads; ++r) {
		if (regs_off[r + 1] < regs_off[r]) { err = "regs_off falls at read " + std::to_string((long long)r); return -1; }
		// (the kernel indexes a read's staged ints with an int)
		if (regs_off[r + 1] - regs_off[r] > INT32_MAX / AP_NF) { err = "too many regions in read " + std::to_string((long long)r); return -1; }
	}
	const int64_t N = regs_off[n_reads];
	if (N == 0) return 0;
	if (!regs || !extra || !cigar_off) { err = "regions without regs, extra or cigar_off"; return -1; }
	if (cigar_off[0] != 0) { err = "cigar_off does not start at 0"; return -1; }
	for (int64_t g = 0; g < N; ++g) {
		const int32_t *x = extra + g * AP_EXTRA_WORDS;
		if (x[0] != 0 && x[0] != 1) { err = "has_extra of region " + std::to_string((long long)g) + " is neither 0 nor 1"; return -1; }
		if (cigar_off[g + 1] < cigar_off[g]) { err = "cigar_off falls at region " + std::to_string((long long)g); return -1; }
		if ((int64_t)x[4] != cigar_off[g + 1] - cigar_off[g]) { err = "n_cigar of region " + std::to_string((long long)g) + " disagrees with cigar_off"; return -1; }
	}
	if (cigar_off[N] > 0 && !cigar) { err = "CIGAR words without cigar"; return -1; }
	n_regs = N; n_words = cigar_off[N];
	return 0;
}

static inline size_t apost_take(size_t &at, size_t bytes) { const size_t o = at; at += (bytes + 15) / 16 * 16; return o; }

// Where the pieces lie, in bytes, for R reads, N regions in and W CIGAR words in.  `in`: what comes up from the host (the regions only
// for chaindp_align_post_regs).  `work`: the kernels' own.  `out`: the resident result.  Every piece starts on 16 bytes.
struct ApostLayout {
	size_t in_rep, in_regs_off, in_regs, in_extra, in_cigar_off, in_cigar, in_bytes;
	size_t w_cnt, w_words, w_tile, w_st_regs, w_st_dp2, w_st_src, w_st_wpre, w_fsrc, w_scratch, w_err, work_bytes;
	size_t o_need, o_regs, o_extra, o_dp2, o_cigar_off, out_bytes, out_cig_bytes;
	ApostLayout(size_t R, size_t N, size_t W, bool regs_from_host)
	{
		size_t at = 0;
		in_rep = apost_take(at, R * 4);
		in_regs_off = in_regs = in_extra = in_cigar_off = in_cigar = 0;
		if (regs_from_host) {
			in_regs_off = apost_take(at, (R + 1) * 8); in_regs = apost_take(at, N * AP_REG_WORDS * 4); in_extra = apost_take(at, N * AP_EXTRA_WORDS * 4);
			in_cigar_off = apost_take(at, (N + 1) * 8); in_cigar = apost_take(at, W * 4);
		}
		in_bytes = at + 16;
		at = 0;
		w_cnt = apost_take(at, (R + 1) * 8); w_words = apost_take(at, (R + 1) * 8); w_tile = apost_take(at, (R / 1024 + 2) * 8);
		w_st_regs = apost_take(at, N * AP_REG_WORDS * 4); w_st_dp2 = apost_take(at, N * 4); w_st_src = apost_take(at, N * 4); w_st_wpre = apost_take(at, N * 4);
		w_fsrc = apost_take(at, N * 8); w_scratch = apost_take(at, N * AP_NF * 4); w_err = apost_take(at, 4);
		work_bytes = at + 16;
		at = 0;
		o_need = apost_take(at, 16); o_regs = apost_take(at, N * AP_REG_WORDS * 4); o_extra = apost_take(at, N * AP_EXTRA_WORDS * 4); o_dp2 = apost_take(at, N * 4);
		o_cigar_off = apost_take(at, (N + 1) * 8);
		out_bytes = at + 16;
		out_cig_bytes = W * 4 + 16;
	}
};

// ---- logf((float)dp_max / match_sc) as the host computes it (hit.c:460, 469)
// The device takes the correctly rounded (float)log((double)x) of the float quotient x.  Its double log need not be the host's: the
// result is the same float as long as log(x) keeps AP_LOGF_MARGIN_ULP double ulps away from every midpoint between two floats.  The list
// holds, for one match_sc, every dp_max in [1, kmax] where the host's logf differs from that float or where the margin is not kept,
// with the host's value.  Through volatile pointers, so that the compiler neither folds nor substitutes the library calls.
#define AP_LOGF_MARGIN_ULP 8
inline float apost_libm_logf(float x) { static float (*volatile f)(float) = logf; return f(x); }
inline double apost_libm_log(double x) { static double (*volatile f)(double) = log; return f(x); }

inline float apost_host_logf(int32_t dp_max, int32_t match_sc) { return apost_libm_logf((float)dp_max / (float)match_sc); }

inline bool apost_logf_clear(double d, float f)
{
	if (!(d == d) || isinf(d)) return true;                                  // not reached for dp_max >= 1
	const double lo = (double)nextafterf(f, -INFINITY), hi = (double)nextafterf(f, INFINITY);
	const double m0 = ((double)f + lo) * 0.5, m1 = ((double)f + hi) * 0.5;
	const double ulp = nextafter(fabs(d), INFINITY) - fabs(d);
	const double margin = AP_LOGF_MARGIN_ULP * ulp;
	return fabs(d - m0) > margin && fabs(d - m1) > margin;
}

inline void apost_logf_build(int32_t match_sc, int32_t kmax, std::vector<uint32_t> &k_out, std::vector<float> &v_out)
{
	k_out.clear(); v_out.clear();
	const float m = (float)match_sc;
	for (int32_t k = 1; k <= kmax; ++k) {
		const float x = (float)k / m;
		const float h = apost_libm_logf(x);
		const double d = apost_libm_log((double)x);
		const float c = (float)d;
		if (memcmp(&h, &c, 4) != 0 || !apost_logf_clear(d, c)) { k_out.push_back((uint32_t)k); v_out.push_back(h); }
	}
}

} // namespace chaindp
#endif
