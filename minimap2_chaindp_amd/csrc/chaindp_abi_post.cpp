// chaindp_abi_post.cpp -- chain_post + mm_est_err + mm_set_mapq (chaindp_post.hip), and the map calls that end with them.
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

// The integers k in [1, 2^24] where the host's logf((float)k) is not the correctly rounded (float)log((double)k), with the host's value
// there: built once per process.  Through volatile pointers, so that the compiler neither folds nor substitutes the library calls.
static std::once_flag g_logf_once;
static std::vector<uint32_t> g_logf_k;
static std::vector<float> g_logf_v;
static float (*volatile g_host_logf)(float) = logf;
static double (*volatile g_host_log)(double) = log;

static void build_logf_patches()
{
	std::call_once(g_logf_once, [] {
		float (*lf)(float) = g_host_logf;
		double (*ld)(double) = g_host_log;
		for (uint32_t k = 1; k <= (uint32_t)POST_LOGF_MAX; ++k) {
			const float h = lf((float)k), c = (float)ld((double)k);
			if (memcmp(&h, &c, 4) != 0) { g_logf_k.push_back(k); g_logf_v.push_back(h); }
		}
	});
}

extern "C" int64_t chaindp_post_logf_patches(uint32_t *k, float *v, int64_t cap)
{
	build_logf_patches();
	const int64_t n = (int64_t)g_logf_k.size();
	for (int64_t i = 0; i < n && i < cap; ++i) { if (k) k[i] = g_logf_k[(size_t)i]; if (v) v[i] = g_logf_v[(size_t)i]; }
	return n;
}

int chaindp::post_logf_upload(chaindp_ctx *ctx)
{
	if (ctx->logf_ready) return CHAINDP_OK;
	build_logf_patches();
	const size_t n = g_logf_k.size(), m = ctx->pool.mark();
	hipError_t e = (hipError_t)ctx->pool.alloc_group({dev_buf(ctx->d_logf_k, (n ? n : 1) * 4), dev_buf(ctx->d_logf_v, (n ? n : 1) * 4)});
	if (e == hipSuccess && n) e = hipMemcpy(ctx->d_logf_k, g_logf_k.data(), n * 4, hipMemcpyHostToDevice);
	if (e == hipSuccess && n) e = hipMemcpy(ctx->d_logf_v, g_logf_v.data(), n * 4, hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		ctx->pool.rollback(m);
		ctx->err = std::string("logf patch tables: ") + hipGetErrorString(e);
		return CHAINDP_ERR_HIP;
	}
	ctx->n_logf = (int)n; ctx->logf_ready = true;
	return CHAINDP_OK;
}

// everything chaindp_chain_post and chaindp_frag_post share on the device, for a batch of n_c chains with n_b chain anchors
int chaindp::post_reserve(chaindp_ctx *ctx, int64_t n_c, int64_t n_b)
{
	ctx->post_n_reads = -1;                              // the caller is about to overwrite what a finished chaindp_chain_post left there
	int rc = regs_per_read_buffers(ctx);
	if (rc) return rc;
	if ((rc = post_logf_upload(ctx)) != CHAINDP_OK) return rc;
	const size_t RB = (size_t)ctx->cap_reads + 2;
	rc = first_use(ctx, ctx->post_ready, "chain_post", {dev_buf(ctx->d_post_off, RB * 8), dev_buf(ctx->d_post_tile, (RB / 1024 + 2) * 8),
	                                                    dev_buf(ctx->d_post_qlen, RB * 4), dev_buf(ctx->d_post_rep, RB * 4), dev_buf(ctx->d_post_err, 4)});
	if (rc) return rc;
	HIP_TRY(ctx, dev_grow(ctx, ctx->post_stage, (size_t)n_c * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->post_out, (size_t)n_c * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->post_sq, (size_t)(n_b > 0 ? n_b : 1) * 16));
	HIP_TRY(ctx, dev_grow(ctx, ctx->post_scratch, (size_t)n_c * POST_SCRATCH_INTS * 4));
	return CHAINDP_OK;
}

extern "C" int64_t chaindp_post_logf_selftest(chaindp_ctx_t *ctx, int32_t kmax)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (kmax < 1 || kmax > POST_LOGF_MAX) { ctx->err = "kmax must lie in [1, 2^24]"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = post_logf_upload(ctx);
	if (rc) return rc;
	float *d_out = nullptr;
	HIP_TRY(ctx, hipMalloc(&d_out, (size_t)kmax * 8));
	int32_t *d_term = (int32_t*)(d_out + kmax);
	std::vector<float> dev((size_t)kmax);
	std::vector<int32_t> term((size_t)kmax);
	hipError_t e = chaindp::launch_post_logf_probe(ctx->stream, kmax, ctx->d_logf_k, ctx->d_logf_v, ctx->n_logf, d_out, d_term);
	if (e == hipSuccess) e = hipMemcpyAsync(dev.data(), d_out, (size_t)kmax * 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(term.data(), d_term, (size_t)kmax * 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	(void)hipFree(d_out);
	if (e != hipSuccess) { ctx->err = std::string("logf self-test: ") + hipGetErrorString(e); return CHAINDP_ERR_HIP; }
	float (*lf)(float) = g_host_logf;
	int64_t bad = 0;
	for (int32_t k = 1; k <= kmax; ++k) {
		const float h = lf((float)k);
		const int t = (int)(4.343f * h + .499f);                     // hit.c:474 as the host evaluates it: float multiply, float add
		bad += memcmp(&h, &dev[(size_t)k - 1], 4) != 0 || t != term[(size_t)k - 1];
	}
	return bad;
}

chaindp::PostOpt chaindp::to_post_opt(const chaindp_post_opt_t *o)
{
	chaindp::PostOpt p;
	p.flag = o->flag; p.mask_level = o->mask_level; p.pri_ratio = o->pri_ratio; p.best_n = o->best_n; p.min_diff = o->min_diff;
	p.sub_diff = o->sub_diff; p.max_join_long = o->max_join_long; p.max_join_short = o->max_join_short;
	p.min_join_flank_sc = o->min_join_flank_sc; p.min_cnt = o->min_cnt; p.min_chain_score = o->min_chain_score; p.match_sc = o->match_sc;
	p.is_sr = o->is_sr;
	return p;
}

// What chaindp_chain_post and chaindp_frag_post open and end with.  post_require_hits: the hits of a chaindp_gen_regs on this batch are
// resident.  post_stage_rep_len: *d_rep = the caller's rep_len, uploaded, or what the seed collection left.  post_finish: the error word
// of k_post_mapq comes down behind the results, then the stream is drained.
int chaindp::post_require_hits(chaindp_ctx *ctx, const char *who)
{
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has || !ctx->regs_resident) {
		ctx->err = std::string(who) + " needs the hits of a chaindp_gen_regs on this batch (a chaindp_est_err since has replaced them)";
		return CHAINDP_ERR_ARG;
	}
	return CHAINDP_OK;
}

int chaindp::post_stage_rep_len(chaindp_ctx *ctx, const int32_t *rep_len, int64_t R, const int32_t **d_rep)
{
	hipStream_t st = ctx->stream;
	*d_rep = ctx->d_rep_len;
	if (rep_len) { HIP_TRY(ctx, hipMemcpyAsync(ctx->d_post_rep, rep_len, (size_t)R * 4, hipMemcpyHostToDevice, st)); *d_rep = ctx->d_post_rep; }
	return CHAINDP_OK;
}

int chaindp::post_finish(chaindp_ctx *ctx)
{
	hipStream_t st = ctx->stream;
	int32_t err = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&err, ctx->d_post_err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (err) { ctx->err = "a score or n_sub + 1 above 2^24: beyond the logf patch list"; return CHAINDP_ERR_CAPACITY; }
	return CHAINDP_OK;
}

extern "C" int chaindp_chain_post(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, const int32_t *qlen, const int32_t *rep_len,
                                  const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                                  int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *a_off, chaindp_anchor_t *a)
{
	return chain_post_impl(ctx, opt, qlen, rep_len, ref_len, n_ref, mini_pos_off, mini_pos, regs_off, regs, regs_cap, a_off, a, false);
}

// A call that runs to its end leaves the batch's final hits whole in HBM (post_out at d_post_off, the anchors in post_sq) and says so in
// ctx->post_n_reads, for chaindp_align_resident; any other way out leaves it at -1.
int chaindp::chain_post_impl(chaindp_ctx *ctx, const chaindp_post_opt_t *opt, const int32_t *qlen, const int32_t *rep_len, const int32_t *ref_len, int32_t n_ref,
                             const int64_t *mini_pos_off, const uint64_t *mini_pos, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *a_off,
                             chaindp_anchor_t *a, bool keep_only)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!opt || !regs_off || (!keep_only && (regs_cap < 0 || (regs_cap > 0 && !regs))) || n_ref < 0 || (n_ref > 0 && !ref_len) || (a && !a_off)) {
		ctx->err = "NULL argument"; return CHAINDP_ERR_ARG;
	}
	if (int rc = post_require_hits(ctx, "chaindp_chain_post")) return rc;
	ctx->post_n_reads = -1;
	auto whole = [&](int64_t n_reads, int64_t n_out) {
		ctx->post_n_out = n_out; ctx->post_cigar = (opt->flag & CHAINDP_F_CIGAR) != 0;
		ctx->post_ref_len.assign(ref_len, ref_len + n_ref);
		ctx->post_n_reads = n_reads;
	};
	const int64_t R = ctx->bot_n_reads, n_c = ctx->bot_n_chains, n_b = ctx->bot_n_b;
	const bool do_mapq = !(opt->flag & CHAINDP_F_CIGAR), do_err = !opt->is_sr;
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// single-segment reads only (mm_select_sub_multi, mm_seg_gen and mm_pair are not here)
	if (ctx->ran_par.n_segs > 1 && !ctx->has_n_segs) { ctx->err = "chaindp_chain_post takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	if (ctx->has_n_segs && R > 0) {
		std::vector<int32_t> ns((size_t)R);
		HIP_TRY(ctx, hipMemcpyAsync(ns.data(), ctx->d_n_segs, (size_t)R * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		for (int32_t v : ns) if (v > 1) { ctx->err = "chaindp_chain_post takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	}
	if (R == 0 || n_c == 0) {
		for (int64_t r = 0; r <= R; ++r) { regs_off[r] = 0; if (a_off) a_off[r] = 0; }
		whole(R, 0);
		return CHAINDP_OK;
	}
	int rc = do_err ? mini_pos_check(ctx, mini_pos_off, mini_pos) : CHAINDP_OK;
	if (rc) return rc;
	if (do_mapq && !rep_len && !ctx->mp_resident) { ctx->err = "no resident rep_len: pass it, or collect the seeds with chaindp_collect_seeds"; return CHAINDP_ERR_ARG; }
	if ((rc = post_reserve(ctx, n_c, n_b)) != CHAINDP_OK) return rc;
	const int32_t *d_qlen = ctx->d_rqlen;
	if (qlen) { HIP_TRY(ctx, hipMemcpyAsync(ctx->d_post_qlen, qlen, (size_t)R * 4, hipMemcpyHostToDevice, st)); d_qlen = ctx->d_post_qlen; }
	const int32_t *d_rep = nullptr;
	if ((rc = post_stage_rep_len(ctx, rep_len, R, &d_rep)) != CHAINDP_OK) return rc;
	HIP_TRY(ctx, hipMemsetAsync(ctx->d_post_err, 0, 4, st));
	const chaindp::PostOpt po = to_post_opt(opt);
	HIP_TRY(ctx, chaindp::launch_post_read(st, R, ctx->bot.chains_off, ctx->bot.b_off, ctx->bot.b_out, ctx->regs.p, d_qlen, po,
	                                       (int32_t*)ctx->post_scratch.p, ctx->post_stage.p, ctx->post_sq.p, ctx->d_post_off));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, R, ctx->d_post_off, ctx->d_post_tile, ctx->d_post_off + R));
	HIP_TRY(ctx, chaindp::launch_post_scatter(st, R, ctx->bot.chains_off, ctx->d_post_off, ctx->post_stage.p, ctx->post_out.p));
	HIP_TRY(ctx, hipMemcpyAsync(regs_off, ctx->d_post_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const int64_t n_out = regs_off[R];
	if (!keep_only && n_out > regs_cap) { ctx->err = "more hits than regs has room for (regs_off is valid)"; return CHAINDP_ERR_CAPACITY; }
	if (do_err && n_out > 0) {
		const int64_t *d_mpo = nullptr;
		const unsigned long long *d_mp = nullptr;
		if ((rc = stage_mini_pos(ctx, R, mini_pos_off, mini_pos, ref_len, n_ref, d_mpo, d_mp)) != CHAINDP_OK) return rc;
		// k_regs_div over the packed output, with the anchors as chain_post left them (mm_est_err at map.c:872)
		HIP_TRY(ctx, chaindp::launch_est_err(st, R, n_out, (const int64_t*)ctx->d_post_off, ctx->bot.b_off, ctx->post_sq.p, d_qlen,
		                                     (const int32_t*)ctx->ref_len.p, n_ref, d_mpo, d_mp, ctx->d_sum_k, ctx->post_out.p, nullptr));
	}
	if (do_mapq && n_out > 0)
		HIP_TRY(ctx, chaindp::launch_post_mapq(st, R, ctx->d_post_off, d_rep, opt->min_chain_score, ctx->d_logf_k, ctx->d_logf_v, ctx->n_logf,
		                                       ctx->post_out.p, ctx->d_post_err));
	if (n_out > 0 && !keep_only) HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->post_out.p, (size_t)n_out * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	if (a_off) HIP_TRY(ctx, hipMemcpyAsync(a_off, ctx->bot.b_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
	if (a && n_b > 0) HIP_TRY(ctx, hipMemcpyAsync(a, ctx->post_sq.p, (size_t)n_b * 16, hipMemcpyDeviceToHost, st));
	if ((rc = post_finish(ctx)) != CHAINDP_OK) return rc;
	whole(R, n_out);
	return CHAINDP_OK;
}

extern "C" int chaindp_map_reads(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                                 const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid,
                                 const int32_t *qlen, const uint32_t *hash, const int32_t *ref_len, int32_t n_ref, int64_t *regs_off, chaindp_reg_t *regs,
                                 int64_t regs_cap, int32_t *rep_len, int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
	if (!opt || !regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && !hash)) { ctx->err = "NULL output, hash or opt"; return CHAINDP_ERR_ARG; }
	if (par->n_segs > 1) { ctx->err = "chaindp_map_reads takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	// the stages of chaindp_map_batch, with the hits left in HBM, then chain_post on them
	rc = map_prefix(ctx, ix, flag, max_occ, par, min_cnt, n_reads, mini_off, mini, bid, qlen, nullptr, hash, rep_len, n_anchors, nullptr, nullptr, 0);
	if (rc) return rc;
	return chaindp_chain_post(ctx, opt, nullptr, nullptr, ref_len, n_ref, nullptr, nullptr, regs_off, regs, regs_cap, nullptr, nullptr);
}

extern "C" int chaindp_map_seqs(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int w, int k, int is_hpc, int flag, int max_occ, const chaindp_params_t *par,
                                int min_cnt, const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const uint32_t *bid,
                                const uint32_t *hash, const int32_t *ref_len, int32_t n_ref, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap,
                                int32_t *rep_len, int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
	if (!opt || !regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && (!hash || !bid))) { ctx->err = "NULL output, bid, hash or opt"; return CHAINDP_ERR_ARG; }
	if (!ix || ix->device != ctx->device) { ctx->err = "index image missing or on another device"; return CHAINDP_ERR_ARG; }
	std::vector<int64_t> mini_off((size_t)(n_reads > 0 ? n_reads + 1 : 1));
	if ((rc = chaindp_sketch(ctx, w, k, is_hpc, n_reads, seq_off, seq, nullptr, mini_off.data())) != CHAINDP_OK) return rc;
	return chaindp_map_reads(ctx, ix, flag, max_occ, par, min_cnt, opt, n_reads, nullptr, nullptr, bid, nullptr, hash, ref_len, n_ref, regs_off, regs,
	                         regs_cap, rep_len, n_anchors);
}
