// chaindp_abi_hits.cpp -- chains to hits: chaindp_backtrack, chaindp_gen_regs, chaindp_est_err and what they stage
// (kernels: chaindp_bottom.hip, chaindp_regs.hip).
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

extern "C" int chaindp_backtrack(chaindp_ctx_t *ctx, const chaindp_params_t *par, int min_cnt,
                                 int64_t *chains_off, uint64_t *u, int64_t *b_off, chaindp_anchor_t *b)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!ctx->ran || !ctx->d_seeds) { ctx->err = "chaindp_backtrack needs a completed run and compaction"; return CHAINDP_ERR_ARG; }
	if (!chains_off || !b_off) { ctx->err = "NULL output"; return CHAINDP_ERR_ARG; }
	ctx->regs_resident = false; ctx->post_n_reads = -1;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the record count of the last compaction (it may have been launched asynchronously by chaindp_run_full)
	unsigned long long n_seeds = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&n_seeds, ctx->cmp.n_seeds, 8, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const int64_t m = ctx->total > 0 && ctx->n_reads > 0 ? (int64_t)(uint32_t)n_seeds : 0;
	ctx->n_seeds = m;
	const size_t M = (size_t)ctx->cap_anchors, R = (size_t)ctx->cap_reads, NB = M / 1024 + 2, NS = (NB > R + 2 ? NB : R + 2) * 8;
	chaindp::BottomScratch &s = ctx->bot;
	rc = first_use(ctx, ctx->bot_ready, "backtrack", {
		dev_buf(s.has, M),
		dev_buf(s.owner, M * 4), dev_buf(s.end_rec, M * 4), dev_buf(s.ccnt, M * 4), dev_buf(s.kpos, M * 4), dev_buf(s.bpos, M * 4),
		dev_buf(s.c_src, M * 4), dev_buf(s.c_dst, M * 4),
		dev_buf(s.key, M * 8), dev_buf(s.skey, M * 8), dev_buf(s.cu, M * 8), dev_buf(s.u_tmp, M * 8), dev_buf(s.u_out, M * 8),
		dev_buf(s.b_tmp, M * 16), dev_buf(s.b_out, M * 16), dev_buf(s.w, M * 16),
		dev_buf(s.stacks, (M / 64 + 2 * R + 4) * 12),
		dev_buf(s.block_cnt, NS), dev_buf(s.tile_tmp, NS),
		dev_buf(s.read_tot, (R + 2) * 8), dev_buf(s.total, 8),
		dev_buf(s.ends_off, (R + 2) * 8), dev_buf(s.chains_off, (R + 2) * 8), dev_buf(s.b_off, (R + 2) * 8)});
	if (rc) return rc;
	EventSet es;
	HIP_TRY(ctx, prof_begin(ctx, es, 2, 3, ctx->stream));
	HIP_TRY(ctx, chaindp::launch_backtrack(ctx->stream, min_cnt, par->min_sc, ctx->n_reads, ctx->cap_anchors, ctx->d_seeds_off, ctx->d_seeds,
	                                       ctx->cmp.n_seeds, ctx->bot, m));
	HIP_TRY(ctx, prof_mark(ctx, es, 1, ctx->stream));
	const size_t ob = (size_t)(ctx->n_reads > 0 ? ctx->n_reads + 1 : 1) * 8;
	HIP_TRY(ctx, hipMemcpyAsync(chains_off, ctx->bot.chains_off, ob, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(b_off, ctx->bot.b_off, ob, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const int64_t n_c = ctx->n_reads > 0 ? chains_off[ctx->n_reads] : 0, n_b = ctx->n_reads > 0 ? b_off[ctx->n_reads] : 0;
	ctx->bot_n_reads = ctx->n_reads; ctx->bot_n_chains = n_c; ctx->bot_n_b = n_b;
	if (u && n_c > 0) HIP_TRY(ctx, hipMemcpyAsync(u, ctx->bot.u_out, (size_t)n_c * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (b && n_b > 0) HIP_TRY(ctx, hipMemcpyAsync(b, ctx->bot.b_out, (size_t)n_b * 16, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

// per-read arrays of the hit stages
int chaindp::regs_per_read_buffers(chaindp_ctx *ctx)
{
	const size_t R = (size_t)ctx->cap_reads + 2;
	return first_use(ctx, ctx->regs_ready, "hit", {dev_buf(ctx->d_rhash, R * 4), dev_buf(ctx->d_rqlen, R * 4), dev_buf(ctx->d_regs_off, R * 8),
	                                               dev_buf(ctx->d_mp_off_up, R * 8), dev_buf(ctx->d_sum_k, R * 8)});
}

// mini_pos[] of the batch for mm_est_err: the caller's arrays or, with both NULL, what chaindp_collect_seeds left resident.
// mini_pos_check is the argument check (no device work); stage_mini_pos uploads the caller's arrays and the targets' lengths,
// growing their buffers, and returns the offsets and positions the kernel reads.
int chaindp::mini_pos_check(chaindp_ctx *ctx, const int64_t *mini_pos_off, const uint64_t *mini_pos)
{
	const bool resident = mini_pos == nullptr && mini_pos_off == nullptr;
	if (resident && (!ctx->mp_resident || !ctx->d_mp_off)) { ctx->err = "no resident mini_pos: pass the arrays, or collect the seeds with chaindp_collect_seeds"; return CHAINDP_ERR_ARG; }
	if (!resident && !mini_pos_off) { ctx->err = "mini_pos without offsets"; return CHAINDP_ERR_ARG; }
	return CHAINDP_OK;
}

int chaindp::stage_mini_pos(chaindp_ctx *ctx, int64_t R, const int64_t *mini_pos_off, const uint64_t *mini_pos, const int32_t *ref_len, int32_t n_ref,
                          const int64_t *&d_mpo, const unsigned long long *&d_mp)
{
	hipStream_t st = ctx->stream;
	d_mpo = ctx->d_mp_off; d_mp = ctx->d_mini_pos;
	if (mini_pos || mini_pos_off) {
		const int64_t n_mp = mini_pos_off[R];
		if (n_mp < 0 || (n_mp > 0 && !mini_pos)) { ctx->err = "mini_pos announced but absent"; return CHAINDP_ERR_ARG; }
		HIP_TRY(ctx, dev_grow(ctx, ctx->mp_up, (size_t)(n_mp > 0 ? n_mp : 1) * 8));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mp_off_up, mini_pos_off, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, st));
		if (n_mp > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->mp_up.p, mini_pos, (size_t)n_mp * 8, hipMemcpyHostToDevice, st));
		d_mpo = ctx->d_mp_off_up; d_mp = (const unsigned long long*)ctx->mp_up.p;
	}
	HIP_TRY(ctx, dev_grow(ctx, ctx->ref_len, (size_t)(n_ref > 0 ? n_ref : 1) * 4));
	if (n_ref > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->ref_len.p, ref_len, (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
	return CHAINDP_OK;
}

// download = false: the hits stay in HBM only (chaindp_map_reads)
int chaindp::gen_regs_impl(chaindp_ctx *ctx, const uint32_t *hash, const int32_t *qlen, chaindp_reg_t *regs, bool download)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has) { ctx->err = "chaindp_gen_regs needs the chains of a chaindp_backtrack on this batch"; return CHAINDP_ERR_ARG; }
	const int64_t R = ctx->bot_n_reads, n_c = ctx->bot_n_chains;
	if (R > 0 && (!hash || !qlen)) { ctx->err = "NULL hash or qlen"; return CHAINDP_ERR_ARG; }
	if (download && n_c > 0 && !regs) { ctx->err = "NULL output"; return CHAINDP_ERR_ARG; }
	ctx->regs_resident = false; ctx->post_n_reads = -1;
	if (R == 0 || n_c == 0) { ctx->regs_resident = true; return CHAINDP_OK; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = regs_per_read_buffers(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, dev_grow(ctx, ctx->regs, (size_t)n_c * sizeof(chaindp_reg_t)));
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rhash, hash, (size_t)R * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rqlen, qlen, (size_t)R * 4, hipMemcpyHostToDevice, st));
	// sort keys go to the backtrack's 16-byte scratch (free once the chains are out), range stacks to its stack area
	HIP_TRY(ctx, chaindp::launch_gen_regs(st, R, ctx->bot.chains_off, ctx->bot.b_off, ctx->bot.u_out, ctx->bot.b_out, ctx->d_rhash, ctx->d_rqlen,
	                                      ctx->bot.w, ctx->bot.stacks, ctx->regs.p));
	if (download) HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->regs.p, (size_t)n_c * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	ctx->regs_resident = true;
	return CHAINDP_OK;
}

extern "C" int chaindp_gen_regs(chaindp_ctx_t *ctx, const uint32_t *hash, const int32_t *qlen, chaindp_reg_t *regs)
{
	return gen_regs_impl(ctx, hash, qlen, regs, true);
}

extern "C" int chaindp_est_err(chaindp_ctx_t *ctx, const int64_t *regs_off, chaindp_reg_t *regs, const int32_t *qlen,
                               const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                               int32_t *match_tot)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has) { ctx->err = "chaindp_est_err needs the chains of a chaindp_backtrack on this batch"; return CHAINDP_ERR_ARG; }
	const int64_t R = ctx->bot_n_reads;
	if (R == 0) return CHAINDP_OK;
	if (!regs_off || !qlen || (n_ref > 0 && !ref_len) || n_ref < 0) { ctx->err = "NULL argument"; return CHAINDP_ERR_ARG; }
	if (regs_off[0] != 0) { ctx->err = "regs_off must start at 0"; return CHAINDP_ERR_ARG; }
	for (int64_t r = 0; r < R; ++r) if (regs_off[r + 1] < regs_off[r]) { ctx->err = "regs_off must not decrease"; return CHAINDP_ERR_ARG; }
	const int64_t n_regs = regs_off[R];
	if (n_regs == 0) return CHAINDP_OK;
	if (!regs) { ctx->err = "NULL regs"; return CHAINDP_ERR_ARG; }
	int rc = mini_pos_check(ctx, mini_pos_off, mini_pos);
	if (rc) return rc;
	for (int64_t g = 0; g < n_regs; ++g) if (regs[g].cnt < 0 || regs[g].as < 0) { ctx->err = "hit with a negative count or offset"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if ((rc = regs_per_read_buffers(ctx)) != CHAINDP_OK) return rc;
	hipStream_t st = ctx->stream;
	ctx->regs_resident = false; ctx->post_n_reads = -1;          // the upload below replaces what chaindp_gen_regs left in d_regs / d_rqlen
	// every hit's anchors must lie inside its read's chain anchors: checked here, on the host's copy of the offsets
	{
		std::vector<int64_t> boff((size_t)R + 1);
		HIP_TRY(ctx, hipMemcpyAsync(boff.data(), ctx->bot.b_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		for (int64_t r = 0; r < R; ++r)
			for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g)
				if ((int64_t)regs[g].as + regs[g].cnt > boff[r + 1] - boff[r]) { ctx->err = "hit reaches beyond its read's chain anchors"; return CHAINDP_ERR_ARG; }
	}
	HIP_TRY(ctx, dev_grow(ctx, ctx->regs, (size_t)n_regs * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->reg_counts, (size_t)n_regs * 8));
	const int64_t *d_mpo = nullptr;
	const unsigned long long *d_mp = nullptr;
	if ((rc = stage_mini_pos(ctx, R, mini_pos_off, mini_pos, ref_len, n_ref, d_mpo, d_mp)) != CHAINDP_OK) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_regs_off, regs_off, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rqlen, qlen, (size_t)R * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->regs.p, regs, (size_t)n_regs * sizeof(chaindp_reg_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, chaindp::launch_est_err(st, R, n_regs, ctx->d_regs_off, ctx->bot.b_off, ctx->bot.b_out, ctx->d_rqlen, (const int32_t*)ctx->ref_len.p, n_ref,
	                                     d_mpo, d_mp, ctx->d_sum_k, ctx->regs.p, (int32_t*)ctx->reg_counts.p));
	HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->regs.p, (size_t)n_regs * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	if (match_tot) HIP_TRY(ctx, hipMemcpyAsync(match_tot, ctx->reg_counts.p, (size_t)n_regs * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	return CHAINDP_OK;
}
