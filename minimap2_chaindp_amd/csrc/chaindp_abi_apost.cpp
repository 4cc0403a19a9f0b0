// chaindp_abi_apost.cpp -- aligned reads finished on the device (include/chaindp_align_post.h): the tail of align_regs and mm_set_mapq
// over regions that carry alignments.  The argument checks, the layout of the buffers and the logf list are chaindp_apost_plan.h's,
// the kernels apost/chaindp_apost.hip's; this file owns the stage's buffers, the copies and the order of the calls:
//   (regions up, for chaindp_align_post_regs) -> rep_len up -> k_apost_read -> scans -> gathers -> (need, error word down) -> the
//   result down, or later by fetch
// The three public calls share align_post_impl, which works on device-resident regions, extras and CIGAR words.
#include "chaindp_ctx.h"
#include "../../include/chaindp_align_post.h"
#include <string.h>
#include <map>
#include <mutex>

using namespace chaindp;

static_assert(sizeof(ApostOpt) == sizeof(chaindp_post_opt_t) && sizeof(ApostOpt) == sizeof(PostOpt), "one layout of the post options");
static_assert(sizeof(chaindp_reg_t) == AP_REG_WORDS * 4 && sizeof(chaindp_align_extra_t) == AP_EXTRA_WORDS * 4, "the words of a region and its extra");

// The logf list of a match_sc over the whole range, built once per process and match_sc.
struct ApostList { std::vector<uint32_t> k; std::vector<float> v; };
static std::mutex g_ap_mutex;
static std::map<int32_t, ApostList> g_ap_lists;

static const ApostList &apost_list(int32_t match_sc)
{
	std::lock_guard<std::mutex> lock(g_ap_mutex);
	auto it = g_ap_lists.find(match_sc);
	if (it == g_ap_lists.end()) {
		it = g_ap_lists.emplace(match_sc, ApostList()).first;
		apost_logf_build(match_sc, AP_LOGF_MAX, it->second.k, it->second.v);
	}
	return it->second;
}

// ... and on the device, one match_sc at a time per context
static int apost_list_upload(chaindp_ctx *ctx, int32_t match_sc, const char *who)
{
	if (ctx->ap_dp_sc == match_sc && ctx->ap_dp.p) return CHAINDP_OK;
	const ApostList &l = apost_list(match_sc);
	const size_t n = l.k.size();
	ctx->ap_dp_sc = 0;
	if (int rc = ksw_grow(ctx, ctx->ap_dp, n * 8 + 32, "the logf list", who)) return rc;
	char *d = (char*)ctx->ap_dp.p;
	if (n) {
		HIP_TRY(ctx, host_copy(d, l.k.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, host_copy(d + (n * 4 + 15) / 16 * 16, l.v.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	ctx->ap_dp_sc = match_sc; ctx->ap_n_dp = (int)n;
	return CHAINDP_OK;
}

extern "C" int64_t chaindp_apost_logf_patches(int32_t match_sc, uint32_t *k, float *v, int64_t cap)
{
	if (match_sc <= 0) return -1;
	const ApostList &l = apost_list(match_sc);
	const int64_t n = (int64_t)l.k.size();
	for (int64_t i = 0; i < n && i < cap; ++i) { if (k) k[i] = l.k[(size_t)i]; if (v) v[i] = l.v[(size_t)i]; }
	return n;
}

extern "C" int64_t chaindp_apost_logf_selftest(chaindp_ctx_t *ctx, int32_t match_sc, int32_t kmax)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (match_sc <= 0 || kmax < 1 || kmax > AP_LOGF_MAX) { ctx->err = "chaindp_apost_logf_selftest: match_sc must be positive and kmax lie in [1, 2^24]"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (int rc = apost_list_upload(ctx, match_sc, "chaindp_apost_logf_selftest")) return rc;
	float *d_out = nullptr;
	HIP_TRY(ctx, hipMalloc(&d_out, (size_t)kmax * 4));
	std::vector<float> dev((size_t)kmax);
	const char *d = (const char*)ctx->ap_dp.p;
	const size_t n = (size_t)ctx->ap_n_dp;
	hipError_t e = launch_apost_logf_probe(ctx->stream, kmax, match_sc, (const uint32_t*)d, (const float*)(d + (n * 4 + 15) / 16 * 16), (int)n, d_out);
	if (e == hipSuccess) e = hipMemcpyAsync(dev.data(), d_out, (size_t)kmax * 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	(void)hipFree(d_out);
	if (e != hipSuccess) { ctx->err = std::string("chaindp_apost_logf_selftest: ") + hipGetErrorString(e); return CHAINDP_ERR_HIP; }
	int64_t bad = 0;
	for (int32_t k = 1; k <= kmax; ++k) {
		const float h = apost_host_logf(k, match_sc);
		bad += memcmp(&h, &dev[(size_t)k - 1], 4) != 0;
	}
	return bad;
}

extern "C" int chaindp_align_post_debug_check(const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, const int64_t *regs_off, const chaindp_reg_t *regs,
                                              const chaindp_align_extra_t *extra, const int64_t *in_cigar_off, const uint32_t *in_cigar, int64_t regs_cap,
                                              int64_t cigar_cap, int64_t out[2])
{
	std::string err;
	int64_t N = 0, W = 0;
	if (apost_check_call((const ApostOpt*)opt, n_reads, rep_len, regs_cap, cigar_cap, true, true, true, err)) return CHAINDP_ERR_ARG;
	if (regs_off && apost_check_regs(n_reads, regs_off, (const int32_t*)regs, (const int32_t*)extra, in_cigar_off, in_cigar, N, W, err)) return CHAINDP_ERR_ARG;
	if (out) { out[0] = N; out[1] = W; }
	return CHAINDP_OK;
}

extern "C" int chaindp_align_post_debug_set_lds_cap(chaindp_ctx_t *ctx, int cap, int32_t *out_cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (cap < 0 || cap > AP_LDS_CAP) { ctx->err = "chaindp_align_post_debug_set_lds_cap: cap outside 0.." + std::to_string(AP_LDS_CAP); return CHAINDP_ERR_ARG; }
	ctx->ap_lds_cap = cap ? cap : AP_LDS_CAP;
	if (out_cap) *out_cap = AP_LDS_CAP;
	return CHAINDP_OK;
}

extern "C" int chaindp_align_post_debug_ms(chaindp_ctx_t *ctx, double ms[2])
{
	if (!ctx || !ms) return CHAINDP_ERR_ARG;
	ms[0] = ctx->ap_ms[0]; ms[1] = ctx->ap_ms[1];
	return CHAINDP_OK;
}

// the call's own arguments, for all four public calls (rep_len only where the call computes)
static int check_call(chaindp_ctx *ctx, const char *who, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, int64_t *out_off,
                      chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar,
                      int64_t cigar_cap, int64_t *need)
{
	std::string err;
	if (apost_check_call((const ApostOpt*)opt, n_reads, rep_len, regs_cap, cigar_cap, out_off && need, out_regs && out_extra && out_dp_max2 && cigar_off, cigar != nullptr, err)) {
		ctx->err = std::string(who) + ": " + err;
		return CHAINDP_ERR_ARG;
	}
	return CHAINDP_OK;
}

// the resident result into the caller's arrays
static int deliver(chaindp_ctx *ctx, const char *who, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2,
                   int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	need[0] = ctx->ap_need[0]; need[1] = ctx->ap_need[1];
	out_off[0] = 0;
	if (n_reads == 0) { if (cigar_off) cigar_off[0] = 0; return CHAINDP_OK; }
	hipStream_t st = ctx->stream;
	const char *d_out = (const char*)ctx->ap_out.p;
	HIP_TRY(ctx, host_copy(out_off, (const char*)ctx->ap_work.p + ctx->ap_at[0], (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
	const bool fits = need[0] <= regs_cap && need[1] <= cigar_cap;
	if (fits) {
		const size_t R = (size_t)need[0];
		if (R) HIP_TRY(ctx, host_copy(out_regs, d_out + ctx->ap_at[1], R * 80, hipMemcpyDeviceToHost, st));
		if (R) HIP_TRY(ctx, host_copy(out_extra, d_out + ctx->ap_at[2], R * 20, hipMemcpyDeviceToHost, st));
		if (R) HIP_TRY(ctx, host_copy(out_dp_max2, d_out + ctx->ap_at[3], R * 4, hipMemcpyDeviceToHost, st));
		if (cigar_off) HIP_TRY(ctx, host_copy(cigar_off, d_out + ctx->ap_at[4], (R + 1) * 8, hipMemcpyDeviceToHost, st));
		if (need[1]) HIP_TRY(ctx, host_copy(cigar, ctx->ap_out_cig.p, (size_t)need[1] * 4, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (fits) return CHAINDP_OK;
	ctx->err = std::string(who) + ": " + std::to_string((long long)need[0]) + " regions and " + std::to_string((long long)need[1]) + " CIGAR words, room for " +
	           std::to_string((long long)regs_cap) + " and " + std::to_string((long long)cigar_cap);
	return CHAINDP_ERR_CAPACITY;
}

// The stage over N regions with W CIGAR words of n_reads reads.  regs_off == nullptr: the regions are the resident result of
// chaindp_align_reads; else they come up from the host arrays, which apost_check_regs has accepted.  d_rep_len: rep_len is on the device
// already (chaindp_align_resident) and the host's is not read.
static int align_post_impl(chaindp_ctx *ctx, const char *who, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, int64_t N, int64_t W,
                           const int64_t *regs_off, const chaindp_reg_t *regs, const chaindp_align_extra_t *extra, const int64_t *in_cigar_off, const uint32_t *in_cigar,
                           const int32_t *d_rep_len = nullptr)
{
	ctx->ap_n_reads = -1;                                // whatever was resident is no longer
	ctx->ap_need[0] = ctx->ap_need[1] = 0;
	if (n_reads == 0) { ctx->ap_n_reads = 0; return CHAINDP_OK; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // a buffer that grows is freed: nothing of an earlier call may be in flight
	hipStream_t st = ctx->stream;
	int rc;
	if ((rc = post_logf_upload(ctx))) return rc;
	if ((rc = apost_list_upload(ctx, opt->match_sc, who))) return rc;
	const bool from_host = regs_off != nullptr;
	const size_t R = (size_t)n_reads;
	const ApostLayout L(R, (size_t)N, (size_t)W, from_host);
	if ((rc = ksw_grow(ctx, ctx->ap_in, L.in_bytes, "the regions", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ap_work, L.work_bytes, "the work arrays", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ap_out, L.out_bytes, "the result", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ap_out_cig, L.out_cig_bytes, "the result's CIGARs", who))) return rc;
	char *d_in = (char*)ctx->ap_in.p, *d_w = (char*)ctx->ap_work.p, *d_o = (char*)ctx->ap_out.p;
	if (!d_rep_len) HIP_TRY(ctx, host_copy(d_in + L.in_rep, rep_len, R * 4, hipMemcpyHostToDevice, st));
	ApostDev d = {};
	d.n_reads = n_reads; d.n_regs = N;
	if (from_host) {
		HIP_TRY(ctx, host_copy(d_in + L.in_regs_off, regs_off, (R + 1) * 8, hipMemcpyHostToDevice, st));
		if (N) {
			HIP_TRY(ctx, host_copy(d_in + L.in_regs, regs, (size_t)N * 80, hipMemcpyHostToDevice, st));
			HIP_TRY(ctx, host_copy(d_in + L.in_extra, extra, (size_t)N * 20, hipMemcpyHostToDevice, st));
			HIP_TRY(ctx, host_copy(d_in + L.in_cigar_off, in_cigar_off, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, st));
		}
		if (W) HIP_TRY(ctx, host_copy(d_in + L.in_cigar, in_cigar, (size_t)W * 4, hipMemcpyHostToDevice, st));
		d.regs_off = (const int64_t*)(d_in + L.in_regs_off); d.regs = (const int32_t*)(d_in + L.in_regs); d.extra = (const int32_t*)(d_in + L.in_extra);
		d.cigar_off = (const int64_t*)(d_in + L.in_cigar_off); d.cig = (const uint32_t*)(d_in + L.in_cigar);
	} else {
		const char *d_rd = (const char*)ctx->rd_out.p;
		d.regs_off = (const int64_t*)(d_rd + ctx->rd_out_at[0]); d.regs = (const int32_t*)(d_rd + ctx->rd_out_at[1]); d.extra = (const int32_t*)(d_rd + ctx->rd_out_at[2]);
		d.cigar_off = (const int64_t*)(d_rd + ctx->rd_out_at[3]); d.cig = (const uint32_t*)ctx->rd_out_cig.p;
	}
	d.rep_len = d_rep_len ? d_rep_len : (const int32_t*)(d_in + L.in_rep);
	d.logf_k = ctx->d_logf_k; d.logf_v = ctx->d_logf_v; d.n_logf = ctx->n_logf;
	d.dp_k = (const uint32_t*)ctx->ap_dp.p; d.dp_v = (const float*)((const char*)ctx->ap_dp.p + ((size_t)ctx->ap_n_dp * 4 + 15) / 16 * 16); d.n_dp = ctx->ap_n_dp;
	d.cnt = (unsigned long long*)(d_w + L.w_cnt); d.words = (unsigned long long*)(d_w + L.w_words); d.tile = (unsigned long long*)(d_w + L.w_tile);
	d.st_regs = (int32_t*)(d_w + L.w_st_regs); d.st_dp2 = (int32_t*)(d_w + L.w_st_dp2); d.st_src = (int32_t*)(d_w + L.w_st_src); d.st_wpre = (int32_t*)(d_w + L.w_st_wpre);
	d.fsrc = (int64_t*)(d_w + L.w_fsrc); d.scratch = (int32_t*)(d_w + L.w_scratch); d.err = (int32_t*)(d_w + L.w_err);
	d.need = (int64_t*)(d_o + L.o_need); d.out_regs = (int32_t*)(d_o + L.o_regs); d.out_extra = (int32_t*)(d_o + L.o_extra); d.out_dp2 = (int32_t*)(d_o + L.o_dp2);
	d.out_cigar_off = (int64_t*)(d_o + L.o_cigar_off); d.out_cig = (uint32_t*)ctx->ap_out_cig.p;
	HIP_TRY(ctx, hipMemsetAsync(d.err, 0, 4, st));
	StageEvents ev(ctx);
	HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_apost_read(st, to_post_opt(opt), d, ctx->ap_lds_cap));
	HIP_TRY(ctx, ev.mark(0));
	HIP_TRY(ctx, launch_apost_gather(st, d));
	HIP_TRY(ctx, ev.mark(1));
	int32_t err = 0;
	int64_t need[2] = {0, 0};
	HIP_TRY(ctx, host_copy(need, d.need, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(&err, d.err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (ctx->prof) {
		double ms[2] = {0, 0};
		if ((rc = ev.fold(ms, 2))) return rc;
		ctx->ap_ms[0] = ms[0]; ctx->ap_ms[1] = ms[1];
	}
	if (err) { ctx->err = std::string(who) + ": a dp_max, a score or n_sub + 1 above 2^24: beyond the logf patch lists"; return CHAINDP_ERR_CAPACITY; }
	ctx->ap_need[0] = need[0]; ctx->ap_need[1] = need[1];
	ctx->ap_at[0] = L.w_cnt; ctx->ap_at[1] = L.o_regs; ctx->ap_at[2] = L.o_extra; ctx->ap_at[3] = L.o_dp2; ctx->ap_at[4] = L.o_cigar_off;
	ctx->ap_n_reads = n_reads;
	return CHAINDP_OK;
}

int chaindp::align_post_resident(chaindp_ctx *ctx, const char *who, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, const int32_t *d_rep_len)
{
	return align_post_impl(ctx, who, opt, n_reads, rep_len, ctx->rd_need[0], ctx->rd_need[1], nullptr, nullptr, nullptr, nullptr, nullptr, d_rep_len);
}

int chaindp::align_post_deliver(chaindp_ctx *ctx, const char *who, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra,
                                int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	return deliver(ctx, who, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need);
}

extern "C" int chaindp_align_post_fetch(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra,
                                        int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	static const char *const who = "chaindp_align_post_fetch";
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!out_off || !need) { ctx->err = std::string(who) + ": NULL out_off or need"; return CHAINDP_ERR_ARG; }
	if (regs_cap < 0 || cigar_cap < 0) { ctx->err = std::string(who) + ": negative capacity"; return CHAINDP_ERR_ARG; }
	if ((regs_cap > 0 && (!out_regs || !out_extra || !out_dp_max2 || !cigar_off)) || (cigar_cap > 0 && !cigar)) { ctx->err = std::string(who) + ": a capacity without its arrays"; return CHAINDP_ERR_ARG; }
	if (ctx->ap_n_reads < 0 || n_reads != ctx->ap_n_reads) { ctx->err = std::string(who) + ": no result is resident, or not of n_reads reads"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	return deliver(ctx, who, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need);
}

extern "C" int chaindp_align_post(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, int64_t *out_off, chaindp_reg_t *out_regs,
                                  chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap,
                                  int64_t need[2])
{
	static const char *const who = "chaindp_align_post";
	if (!ctx) return CHAINDP_ERR_ARG;
	if (int rc = check_call(ctx, who, opt, n_reads, rep_len, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need)) return rc;
	if (ctx->rd_n_reads < 0 || n_reads != ctx->rd_n_reads) { ctx->err = std::string(who) + ": no result of chaindp_align_reads is resident, or not of n_reads reads"; return CHAINDP_ERR_ARG; }
	if (int rc = align_post_impl(ctx, who, opt, n_reads, rep_len, ctx->rd_need[0], ctx->rd_need[1], nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
	return deliver(ctx, who, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need);
}

extern "C" int chaindp_align_post_regs(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, const int64_t *regs_off,
                                       const chaindp_reg_t *regs, const chaindp_align_extra_t *extra, const int64_t *in_cigar_off, const uint32_t *in_cigar,
                                       int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap,
                                       int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	static const char *const who = "chaindp_align_post_regs";
	if (!ctx) return CHAINDP_ERR_ARG;
	if (int rc = check_call(ctx, who, opt, n_reads, rep_len, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need)) return rc;
	int64_t N = 0, W = 0;
	std::string err;
	if (apost_check_regs(n_reads, regs_off, (const int32_t*)regs, (const int32_t*)extra, in_cigar_off, in_cigar, N, W, err)) { ctx->err = std::string(who) + ": " + err; return CHAINDP_ERR_ARG; }
	if (int rc = align_post_impl(ctx, who, opt, n_reads, rep_len, N, W, regs_off, regs, extra, in_cigar_off, in_cigar)) return rc;
	return deliver(ctx, who, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need);
}

extern "C" int chaindp_align_reads_post(chaindp_ctx_t *ctx, const chaindp_align_opt_t *aopt, const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *seq_off,
                                        const char *seq, const int64_t *a_off, chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs,
                                        const int32_t *rep_len, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2,
                                        int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	static const char *const who = "chaindp_align_reads_post";
	if (!ctx) return CHAINDP_ERR_ARG;
	if (int rc = check_call(ctx, who, opt, n_reads, rep_len, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need)) return rc;
	if (int rc = align_reads_compute(ctx, aopt, n_reads, seq_off, seq, a_off, a, regs_off, regs, regs_cap, cigar_cap)) return rc;
	if (int rc = align_post_impl(ctx, who, opt, n_reads, rep_len, ctx->rd_need[0], ctx->rd_need[1], nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
	return deliver(ctx, who, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need);
}
