// chaindp_abi_inv.cpp -- the inversion stage of the host ABI (include/chaindp_align_inv.h): mm_align1_inv for every pair of neighbouring regions.
// The checks, the early returns and the extension problems are chaindp_inv_plan.h's, the kernels inv/chaindp_inv.hip's, the DP, the
// stage events and the CIGARs out the alignment stages' scaffold (chaindp_ctx.h: ksw_plan_route, ksw_reserve, ksw_dispatch, ksw_view,
// StageEvents, cigar_pack_out); this file owns the stage's own buffers, the copies and the order of the launches:
//   candidates up -> local score -> (scores down, survivors and problems up) -> gather -> DP -> finish -> skip rule -> (counts down) -> pack
#include "chaindp_ctx.h"
#include "../../include/chaindp_align_inv.h"
#include <string.h>

using namespace chaindp;

static const char *const WHO = "chaindp_align1_inv";

extern "C" int chaindp_align_inv_debug_check(const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const int64_t *regs_off,
                                             const chaindp_reg_t *regs, int64_t n_t, const int64_t *t_off, int64_t out[2])
{
	InvPlan pl;
	if (inv_plan((const AlignOpt*)opt, n_reads, seq_off, regs_off, (const int32_t*)regs, n_t, t_off, pl)) return CHAINDP_ERR_ARG;
	if (out) { out[0] = pl.n_slots; out[1] = (int64_t)pl.cand.size(); }
	return CHAINDP_OK;
}

extern "C" int chaindp_align_inv_debug_ll(chaindp_ctx_t *ctx, int64_t n, int32_t *out3)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n != ctx->inv_n || (n > 0 && !out3)) { ctx->err = "chaindp_align_inv_debug_ll: not the candidate count of the last chaindp_align1_inv"; return CHAINDP_ERR_ARG; }
	if (n == 0) return CHAINDP_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, host_copy(out3, ctx->inv_ll.p, (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_align_inv_debug_ms(chaindp_ctx_t *ctx, double ms[4])
{
	if (!ctx || !ms) return CHAINDP_ERR_ARG;
	for (int k = 0; k < 4; ++k) ms[k] = ctx->inv_ms[k];
	return CHAINDP_OK;
}

extern "C" int chaindp_align1_inv(chaindp_ctx_t *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                                  const int64_t *regs_off, const chaindp_reg_t *regs, int32_t *made, chaindp_reg_t *r_inv,
                                  chaindp_align_extra_t *extra, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap)
{
	return align1_inv_impl(ctx, opt, n_reads, seq_off, seq, regs_off, regs, made, r_inv, extra, cigar_off, cigar, cigar_cap, nullptr);
}

int chaindp::align1_inv_impl(chaindp_ctx *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const int64_t *regs_off,
                             const chaindp_reg_t *regs, int32_t *made, chaindp_reg_t *r_inv, chaindp_align_extra_t *extra, int64_t *cigar_off, uint32_t *cigar,
                             int64_t cigar_cap, AlignResident *res)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!cigar_off) { ctx->err = "chaindp_align1_inv: NULL cigar_off"; return CHAINDP_ERR_ARG; }
	if (!res && (cigar_cap < 0 || (cigar_cap > 0 && !cigar))) { ctx->err = "chaindp_align1_inv: cigar_cap without a cigar array"; return CHAINDP_ERR_ARG; }
	InvPlan ip;
	const int64_t n_t = (int64_t)ctx->al_t_off.size() - 1;
	if (inv_plan((const AlignOpt*)opt, n_reads, seq_off, regs_off, (const int32_t*)regs, n_t < 0 ? 0 : n_t, n_t < 0 ? nullptr : ctx->al_t_off.data(), ip)) {
		ctx->err = ip.err;
		return CHAINDP_ERR_ARG;
	}
	const AlignOpt o = *(const AlignOpt*)opt;
	KswPlan kp;
	if (!ksw_plan_score(o.a, o.b, o.q, o.e, o.q2, o.e2, kp.sc)) { ctx->err = "chaindp_align1_inv: scoring"; return CHAINDP_ERR_ARG; }
	cigar_off[0] = 0;
	const int64_t G = ip.n_slots;
	const size_t C = ip.cand.size();
	if (G == 0) return CHAINDP_OK;
	if (!made || !r_inv || !extra) { ctx->err = "chaindp_align1_inv: NULL made, r_inv or extra"; return CHAINDP_ERR_ARG; }
	if (C > 0 && ip.n_bases > 0 && !seq && !res) { ctx->err = "chaindp_align1_inv: NULL sequence"; return CHAINDP_ERR_ARG; }
	memset(made, 0, (size_t)G * 4); memset(r_inv, 0, (size_t)G * 80); memset(extra, 0, (size_t)G * 20); memset(cigar_off, 0, (size_t)(G + 1) * 8);
	if (C == 0) { ctx->inv_n = 0; return CHAINDP_OK; }          // every pair returned early: nothing for the device
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // a buffer that grows is freed: nothing of an earlier call may be in flight
	hipStream_t st = ctx->stream;
	ctx->inv_n = -1;
	int rc;
	Carve in;
	// (the reads' own part is the caller's where the batch is resident)
	const size_t o_seq_off = in.take(res ? 0 : (size_t)(n_reads + 1) * 8), o_regs_off = in.take((size_t)(n_reads + 1) * 8), o_cand = in.take(C * sizeof(InvCand)),
	             o_slot_cand = in.take((size_t)G * 4), o_seq = in.take(res ? 0 : (size_t)ip.n_bases);
	if ((rc = ksw_grow(ctx, ctx->inv_in, in.at + 16, "the batch", WHO))) return rc;
	Carve rs;
	const size_t o_made = rs.take((size_t)G * 4), o_rinv = rs.take((size_t)G * 80), o_extra = rs.take((size_t)G * 20), o_coff = rs.take((size_t)(G + 1) * 8);
	if ((rc = ksw_grow(ctx, ctx->inv_res, rs.at + 16, "results", WHO))) return rc;
	Carve ll;                            // the local scores first: chaindp_align_inv_debug_ll reads them from the buffer's start
	const size_t o_out3 = ll.take(C * 12), o_surv = ll.take(C * sizeof(InvSurv)), o_prob = ll.take(C * sizeof(KswProb));
	if ((rc = ksw_grow(ctx, ctx->inv_ll, ll.at + 16, "local scores", WHO))) return rc;
	char *d_in = (char*)ctx->inv_in.p, *d_rs = (char*)ctx->inv_res.p, *d_ll = (char*)ctx->inv_ll.p;
	InvDev d = {};
	d.n_reads = n_reads; d.n_cand = (int)C;
	d.seq_off = (const int64_t*)(d_in + o_seq_off); d.regs_off = (const int64_t*)(d_in + o_regs_off); d.seq = d_in + o_seq;
	d.cand = (const InvCand*)(d_in + o_cand); d.slot_cand = (const int32_t*)(d_in + o_slot_cand);
	if (res) { d.seq_off = res->seq_off; d.seq = res->seq; }
	d.t_off = (const int64_t*)ctx->al_toff.p; d.tcodes = (const uint8_t*)ctx->al_tgt.p;
	d.made = (int32_t*)(d_rs + o_made); d.r_inv = (int32_t*)(d_rs + o_rinv); d.extra = (int32_t*)(d_rs + o_extra);
	d.surv = (const InvSurv*)(d_ll + o_surv); d.prob = (const KswProb*)(d_ll + o_prob);
	int64_t *d_coff = (int64_t*)(d_rs + o_coff);
	int32_t *d_out3 = (int32_t*)(d_ll + o_out3);
	auto up = [&](char *base, size_t off, const void *src, size_t bytes) { return bytes ? host_copy(base + off, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
	if (!res) HIP_TRY(ctx, up(d_in, o_seq_off, seq_off, (size_t)(n_reads + 1) * 8));
	HIP_TRY(ctx, up(d_in, o_regs_off, regs_off, (size_t)(n_reads + 1) * 8));
	HIP_TRY(ctx, up(d_in, o_cand, ip.cand.data(), C * sizeof(InvCand)));
	HIP_TRY(ctx, up(d_in, o_slot_cand, ip.slot_cand.data(), (size_t)G * 4));
	if (!res) HIP_TRY(ctx, up(d_in, o_seq, seq, (size_t)ip.n_bases));
	HIP_TRY(ctx, hipMemsetAsync(d_rs, 0, o_coff, st));
	StageEvents ev(ctx);
	HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_inv_ll(st, o, d, (int)inv_ll_rows(ip.max_ql), d_out3));
	HIP_TRY(ctx, ev.mark(0));
	std::vector<int32_t> out3(C * 3);
	HIP_TRY(ctx, host_copy(out3.data(), d_out3, C * 12, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	ctx->inv_n = (int64_t)C;
	// the extensions of the candidates that reached min_dp_max
	std::vector<InvSurv> surv;
	int64_t n_bases = 0;
	inv_problems(o, ip, out3, surv, kp.prob, n_bases);
	const size_t S = surv.size();
	d.n_surv = (int)S;
	if (S) {
		ksw_plan_route(kp, ctx->dp.cus, ctx->ksw_grid_cap);
		if ((rc = ksw_reserve(ctx, kp, n_bases, WHO))) return rc;
		const KswView v = ksw_view(ctx, S);
		HIP_TRY(ctx, up(d_ll, o_surv, surv.data(), S * sizeof(InvSurv)));
		HIP_TRY(ctx, up(d_ll, o_prob, kp.prob.data(), S * sizeof(KswProb)));
		HIP_TRY(ctx, ev.mark(-1));
		HIP_TRY(ctx, launch_inv_gather(st, d, (uint8_t*)ctx->ksw_bases.p));
		if ((rc = ksw_dispatch(ctx, kp, nullptr))) return rc;
		HIP_TRY(ctx, ev.mark(1));
		HIP_TRY(ctx, launch_inv_finish(st, o, d, v.ez, v.cig));
	} else HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_inv_skip(st, d));
	HIP_TRY(ctx, ev.mark(2));
	HIP_TRY(ctx, host_copy(made, d.made, (size_t)G * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(r_inv, d.r_inv, (size_t)G * 80, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(extra, d.extra, (size_t)G * 20, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (S) ctx->ksw_n = (int64_t)S;                      // chaindp_ksw_debug_route: the extensions' routes
	const int64_t total = cigar_prefix((const int32_t*)extra, 5, 4, G, cigar_off);
	const std::function<hipError_t(uint32_t*)> pack = [&](uint32_t *out) {
		hipError_t e;
		return (e = ev.mark(-1)) || (e = launch_inv_pack(st, d, d_coff, ksw_view(ctx, S).cig, out)) ? e : ev.mark(3);
	};
	if (res) { res->d_regs = d.r_inv; res->d_extra = d.extra; }
	const int ret = res ? cigar_pack_dev(ctx, cigar_off, G, total, d_coff, res->room, pack) : cigar_pack_out(ctx, WHO, cigar_off, G, total, cigar, cigar_cap, d_coff, pack);
	if (ret != CHAINDP_ERR_HIP && (rc = ev.fold(ctx->inv_ms, 4))) return rc;
	return ret;
}
