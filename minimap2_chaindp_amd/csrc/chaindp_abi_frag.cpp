// chaindp_abi_frag.cpp -- reads of several segments (chaindp_frag.hip): chain_post with mm_select_sub_multi, mm_seg_gen, per-segment
// mm_set_parent and mm_set_mapq.
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

extern "C" int chaindp_debug_set_frag_lds_cap(chaindp_ctx_t *ctx, int cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (cap < 0 || cap > FRAG_LDS_CAP) { ctx->err = "the fragment kernels keep 0..FRAG_LDS_CAP hits in LDS"; return CHAINDP_ERR_ARG; }
	ctx->frag_lds_cap = cap;
	return CHAINDP_OK;
}

static int frag_post_impl(chaindp_ctx *ctx, const chaindp_post_opt_t *opt, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                          const int32_t *rep_len, const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                          int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *seg_a_off, chaindp_anchor_t *seg_a, int pe_ori,
                          const int32_t *host_qlen = nullptr)   // host_qlen: the caller has just uploaded n_segs_per_read and this qlen itself
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!opt || !seg_regs_off || n_seqs < 0 || regs_cap < 0 || (regs_cap > 0 && !regs) || n_ref < 0 || (n_ref > 0 && !ref_len) || (seg_a && !seg_a_off)) {
		ctx->err = "NULL argument"; return CHAINDP_ERR_ARG;
	}
	if (int rc = post_require_hits(ctx, "chaindp_frag_post")) return rc;
	const int64_t R = ctx->bot_n_reads, n_c = ctx->bot_n_chains, n_b = ctx->bot_n_b, S = n_seqs;
	const bool do_mapq = !(opt->flag & CHAINDP_F_CIGAR);
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the reads' segments: the caller's, checked against what the batch was chained with
	std::vector<int32_t> ns((size_t)R, ctx->ran_par.n_segs), read_seq0((size_t)R + 1, 0);
	if (host_qlen && n_segs_per_read) {
		ns.assign(n_segs_per_read, n_segs_per_read + R);
	} else if (ctx->has_n_segs && R > 0) {
		HIP_TRY(ctx, hipMemcpyAsync(ns.data(), ctx->d_n_segs, (size_t)R * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
	}
	bool any_single = false;
	int64_t n_sum = 0;
	for (int64_t r = 0; r < R; ++r) {
		if (n_segs_per_read && n_segs_per_read[r] != ns[(size_t)r]) { ctx->err = "n_segs_per_read differs from the segments the batch was chained with"; return CHAINDP_ERR_ARG; }
		if (ns[(size_t)r] < 1 || ns[(size_t)r] > 255) { ctx->err = "a read owns 1..255 segments (MM_MAX_SEG)"; return CHAINDP_ERR_ARG; }
		any_single |= ns[(size_t)r] == 1;
		n_sum += ns[(size_t)r];
		read_seq0[(size_t)r + 1] = (int32_t)(n_sum <= S ? n_sum : S);
	}
	if (n_sum != S) { ctx->err = "the reads' segments do not add up to n_seqs"; return CHAINDP_ERR_ARG; }
	if (!seg_len) {
		if (!ctx->sk_valid || (int64_t)ctx->sk_seq_len.size() != S) { ctx->err = "no seg_len and no chaindp_sketch of n_seqs sequences resident"; return CHAINDP_ERR_ARG; }
		seg_len = ctx->sk_seq_len.data();
	}
	for (int64_t q = 0; q < S; ++q) if (seg_len[q] < 0) { ctx->err = "negative seg_len"; return CHAINDP_ERR_ARG; }
	if (S == 0 || n_c == 0) {                                    // no hits anywhere: nothing resident to look at (chaindp_gen_regs uploaded nothing)
		for (int64_t q = 0; q <= S; ++q) { seg_regs_off[q] = 0; if (seg_a_off) seg_a_off[q] = 0; }
		return CHAINDP_OK;
	}
	{
		std::vector<int32_t> ql((size_t)R);
		if (host_qlen) {
			ql.assign(host_qlen, host_qlen + R);
		} else {
			HIP_TRY(ctx, hipMemcpyAsync(ql.data(), ctx->d_rqlen, (size_t)R * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(ctx, hipStreamSynchronize(st));
		}
		for (int64_t r = 0; r < R; ++r) {
			int64_t sum = 0;
			for (int32_t q = read_seq0[(size_t)r]; q < read_seq0[(size_t)r + 1]; ++q) sum += seg_len[q];
			if (sum != ql[(size_t)r]) { ctx->err = "seg_len does not add up to the qlen chaindp_gen_regs was given"; return CHAINDP_ERR_ARG; }
		}
	}
	const bool do_err = !opt->is_sr && any_single;               // mm_seg_gen rebuilds the records of the other reads: div = -1 there
	int rc = do_err ? mini_pos_check(ctx, mini_pos_off, mini_pos) : CHAINDP_OK;
	if (rc) return rc;
	if (do_mapq && !rep_len && !ctx->mp_resident) { ctx->err = "no resident rep_len: pass it, or collect the seeds with chaindp_collect_seeds"; return CHAINDP_ERR_ARG; }
	if ((rc = post_reserve(ctx, n_c, n_b)) != CHAINDP_OK) return rc;
	// per sequence: read_seq0[R + 1] | seq_len | seq_read | seq_rep | seq_hash; counts -> offsets: 3 x (S + 1), then the scans' scratch
	const size_t SB = (size_t)S + 2, tile_items = SB / 1024 + 2;
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_seq, ((size_t)R + 2 + 4 * SB) * 4));
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_cnt, (3 * SB + tile_items) * 8));
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_a, (size_t)(n_b > 0 ? n_b : 1) * 16));
	int32_t *d_read_seq0 = (int32_t*)ctx->frag_seq.p, *d_seq_len = d_read_seq0 + R + 2, *d_seq_read = d_seq_len + SB, *d_seq_rep = d_seq_read + SB;
	uint32_t *d_seq_hash = (uint32_t*)(d_seq_rep + SB);
	unsigned long long *d_g = (unsigned long long*)ctx->frag_cnt.p, *d_o = d_g + SB, *d_a = d_o + SB, *d_tile = d_a + SB;
	HIP_TRY(ctx, hipMemcpyAsync(d_read_seq0, read_seq0.data(), (size_t)(R + 1) * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_seq_len, seg_len, (size_t)S * 4, hipMemcpyHostToDevice, st));
	const int32_t *d_rep = nullptr;
	if ((rc = post_stage_rep_len(ctx, rep_len, R, &d_rep)) != CHAINDP_OK) return rc;
	HIP_TRY(ctx, hipMemsetAsync(ctx->d_post_err, 0, 4, st));
	const chaindp::PostOpt po = to_post_opt(opt);
	// mm_select_sub_multi's max_gap_ref (map.c:243) is the gap_ref the read was chained with: the run's own copy where it took per-read gaps
	const int2 *d_read_gaps = ctx->ran_gaps ? (const int2*)ctx->gaps_ran.p : nullptr;
	// chain_post per read and the first half of mm_seg_gen.  The global scratch of what exceeds the LDS cap is sized for the fragments'
	// hits at this point and grown below for the segments' hits, once their count is known.
	HIP_TRY(ctx, chaindp::launch_frag_read(st, R, ctx->bot.chains_off, ctx->bot.b_off, ctx->bot.b_out, ctx->regs.p, ctx->d_rqlen, d_read_seq0, d_seq_len, po,
	                                       ctx->ran_par.max_dist_x, ctx->frag_lds_cap, (int32_t*)ctx->post_scratch.p, ctx->post_stage.p, ctx->post_sq.p,
	                                       ctx->d_post_off, d_g, d_o, d_a, d_read_gaps));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, R, ctx->d_post_off, ctx->d_post_tile, ctx->d_post_off + R));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, S, d_g, d_tile, d_g + S));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, S, d_o, d_tile, d_o + S));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, S, d_a, d_tile, d_a + S));
	unsigned long long tot[4] = {0, 0, 0, 0};
	HIP_TRY(ctx, hipMemcpyAsync(&tot[0], ctx->d_post_off + R, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(&tot[1], d_g + S, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(&tot[2], d_a + S, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(seg_regs_off, d_o, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, st));
	if (seg_a_off) HIP_TRY(ctx, hipMemcpyAsync(seg_a_off, d_a, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const int64_t n_post = (int64_t)tot[0], n_g = (int64_t)tot[1], n_sa = (int64_t)tot[2], n_out = seg_regs_off[S];
	if (n_post > n_c || n_sa > n_b || n_g > n_out) { ctx->err = "chaindp_frag_post: inconsistent counts"; return CHAINDP_ERR_HIP; }
	if (n_out > regs_cap) { ctx->err = "more hits than regs has room for (seg_regs_off is valid)"; return CHAINDP_ERR_CAPACITY; }
	HIP_TRY(ctx, chaindp::launch_post_scatter(st, R, ctx->bot.chains_off, ctx->d_post_off, ctx->post_stage.p, ctx->post_out.p));
	if (do_err && n_post > 0) {
		const int64_t *d_mpo = nullptr;
		const unsigned long long *d_mp = nullptr;
		if ((rc = stage_mini_pos(ctx, R, mini_pos_off, mini_pos, ref_len, n_ref, d_mpo, d_mp)) != CHAINDP_OK) return rc;
		// mm_est_err (map.c:872) on the packed hits of every read; only the one-segment reads keep theirs
		HIP_TRY(ctx, chaindp::launch_est_err(st, R, n_post, (const int64_t*)ctx->d_post_off, ctx->bot.b_off, ctx->post_sq.p, ctx->d_rqlen,
		                                     (const int32_t*)ctx->ref_len.p, n_ref, d_mpo, d_mp, ctx->d_sum_k, ctx->post_out.p, nullptr));
	}
	const size_t ng1 = (size_t)(n_g > 0 ? n_g : 1);
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_u, ng1 * 8));
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_stage, ng1 * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_z, ng1 * 16));
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_stacks, (ng1 / 64 + 2 * (size_t)S + 4) * 12));
	HIP_TRY(ctx, dev_grow(ctx, ctx->frag_out, (size_t)(n_out > 0 ? n_out : 1) * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->post_scratch, ng1 * POST_SCRATCH_INTS * 4));
	HIP_TRY(ctx, chaindp::launch_frag_split(st, R, ctx->d_post_off, ctx->post_out.p, ctx->bot.b_off, ctx->post_sq.p, d_read_seq0, d_seq_len, ctx->d_rhash,
	                                        do_mapq ? d_rep : nullptr, d_g, d_o, d_a, (unsigned long long*)ctx->frag_u.p, ctx->frag_a.p, ctx->frag_out.p,
	                                        d_seq_hash, d_seq_rep, d_seq_read));
	// mm_gen_regs per (fragment, segment) (hit.c:393): a segment is a read of its own to k_regs_keys / k_regs_fill
	if (n_g > 0)
		HIP_TRY(ctx, chaindp::launch_gen_regs(st, S, (const int64_t*)d_g, (const int64_t*)d_a, (const unsigned long long*)ctx->frag_u.p, ctx->frag_a.p,
		                                      d_seq_hash, d_seq_len, ctx->frag_z.p, ctx->frag_stacks.p, ctx->frag_stage.p));
	HIP_TRY(ctx, chaindp::launch_frag_seg(st, S, d_read_seq0, d_seq_read, d_g, d_o, ctx->frag_stage.p, opt->mask_level, ctx->frag_lds_cap,
	                                      (int32_t*)ctx->post_scratch.p, ctx->frag_out.p));
	if (do_mapq && n_out > 0)
		HIP_TRY(ctx, chaindp::launch_post_mapq(st, S, d_o, d_seq_rep, opt->min_chain_score, ctx->d_logf_k, ctx->d_logf_v, ctx->n_logf, ctx->frag_out.p,
		                                       ctx->d_post_err));
	HIP_TRY(ctx, chaindp::launch_frag_flip(st, S, d_read_seq0, d_seq_read, d_seq_len, d_o, pe_ori, ctx->frag_out.p));
	if (n_out > 0) HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->frag_out.p, (size_t)n_out * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	if (seg_a && n_sa > 0) HIP_TRY(ctx, hipMemcpyAsync(seg_a, ctx->frag_a.p, (size_t)n_sa * 16, hipMemcpyDeviceToHost, st));
	return post_finish(ctx);
}

extern "C" int chaindp_frag_post(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                                 const int32_t *rep_len, const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                                 int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *seg_a_off, chaindp_anchor_t *seg_a)
{
	return frag_post_impl(ctx, opt, n_seqs, n_segs_per_read, seg_len, rep_len, ref_len, n_ref, mini_pos_off, mini_pos, seg_regs_off, regs, regs_cap,
	                      seg_a_off, seg_a, -1);
}

static int map_frags_impl(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                          const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid,
                          const int32_t *qlen, const uint32_t *hash, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                          const int32_t *ref_len, int32_t n_ref, int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len,
                          int64_t *n_anchors, int pe_ori)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
	if (!opt || !seg_regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && (!hash || !n_segs_per_read))) {
		ctx->err = "NULL output, hash, n_segs_per_read or opt"; return CHAINDP_ERR_ARG;
	}
	// the stages of chaindp_map_batch with the reads' segment counts, the hits left in HBM, then the fragment post steps on them
	rc = map_prefix(ctx, ix, flag, max_occ, par, min_cnt, n_reads, mini_off, mini, bid, qlen, n_segs_per_read, hash, rep_len, n_anchors, nullptr, nullptr, 0);
	if (rc) return rc;
	return frag_post_impl(ctx, opt, n_seqs, n_segs_per_read, seg_len, nullptr, ref_len, n_ref, nullptr, nullptr, seg_regs_off, regs, regs_cap, nullptr, nullptr,
	                      pe_ori, qlen);
}

extern "C" int chaindp_map_frags(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                                 const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid,
                                 const int32_t *qlen, const uint32_t *hash, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                                 const int32_t *ref_len, int32_t n_ref, int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len,
                                 int64_t *n_anchors)
{
	return map_frags_impl(ctx, ix, flag, max_occ, par, min_cnt, opt, n_reads, mini_off, mini, bid, qlen, hash, n_seqs, n_segs_per_read, seg_len, ref_len, n_ref,
	                      seg_regs_off, regs, regs_cap, rep_len, n_anchors, -1);
}

extern "C" int chaindp_map_frag_seqs(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int w, int k, int is_hpc, int flag, int max_occ,
                                     const chaindp_params_t *par, int min_cnt, const chaindp_post_opt_t *opt, int pe_ori, int64_t n_reads, int64_t n_seqs,
                                     const int32_t *n_segs_per_read, const int64_t *seq_off, const char *seq, const uint32_t *bid, const uint32_t *hash,
                                     const int32_t *ref_len, int32_t n_ref, int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len,
                                     int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
	if (!opt || !seg_regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && (!hash || !bid || !n_segs_per_read))) {
		ctx->err = "NULL output, bid, hash, n_segs_per_read or opt"; return CHAINDP_ERR_ARG;
	}
	if (pe_ori < -1 || pe_ori > 3) { ctx->err = "pe_ori must be -1 or 0..3"; return CHAINDP_ERR_ARG; }
	if (!ix || ix->device != ctx->device) { ctx->err = "index image missing or on another device"; return CHAINDP_ERR_ARG; }
	int64_t sum = 0;
	for (int64_t r = 0; r < n_reads; ++r) sum += n_segs_per_read[r] > 0 ? n_segs_per_read[r] : n_seqs + 1;
	if (sum != n_seqs) { ctx->err = "n_segs_per_read does not add up to n_seqs"; return CHAINDP_ERR_ARG; }
	std::vector<int64_t> mini_off((size_t)(n_reads > 0 ? n_reads + 1 : 1));
	if ((rc = sketch_impl(ctx, w, k, is_hpc, n_seqs, seq_off, seq, n_reads > 0 ? n_segs_per_read : nullptr, mini_off.data(), pe_ori)) != CHAINDP_OK) return rc;
	return map_frags_impl(ctx, ix, flag, max_occ, par, min_cnt, opt, n_reads, nullptr, nullptr, bid, nullptr, hash, n_seqs, n_segs_per_read, nullptr, ref_len, n_ref,
	                      seg_regs_off, regs, regs_cap, rep_len, n_anchors, pe_ori);
}
