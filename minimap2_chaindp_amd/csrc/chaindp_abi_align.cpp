// chaindp_abi_align.cpp -- the region alignment stage of the host ABI (include/chaindp_align.h): mm_align1 for a batch of regions.
// The checks and the layout of the problems are chaindp_align_plan.h's, the kernels chaindp_align.hip's, the DP, the stage events and
// the CIGARs out the alignment stages' scaffold (chaindp_ctx.h: ksw_plan_route, ksw_reserve, ksw_dispatch, ksw_view, StageEvents,
// cigar_pack_out); this file owns the stage's own buffers, the copies and the order of the launches:
//   plan -> (lengths down, offsets up) -> gather -> DP -> zdrop -> (codes down) -> DP of the second pass -> stitch -> extra -> (counts down) -> pack
#include "chaindp_ctx.h"
#include "../../include/chaindp_align.h"
#include <string.h>

using namespace chaindp;

static_assert(sizeof(chaindp_align_opt_t) == sizeof(AlignOpt), "chaindp_align_opt_t is AlignOpt");
static_assert(sizeof(chaindp_reg_t) == AL_REG_WORDS * 4, "chaindp_reg_t in words");
static_assert(sizeof(chaindp_align_extra_t) == 20, "five words");
static const char *const WHO = "chaindp_align1";

extern "C" int chaindp_align_set_targets(chaindp_ctx_t *ctx, int64_t n_seqs, const int64_t *seq_off, const char *seq)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n_seqs < 0 || n_seqs > 0x7fffffff || !seq_off || seq_off[0] != 0) { ctx->err = "chaindp_align_set_targets: bad sequence offsets"; return CHAINDP_ERR_ARG; }
	for (int64_t i = 0; i < n_seqs; ++i)
		if (seq_off[i + 1] < seq_off[i] || seq_off[i + 1] - seq_off[i] >= 0x7fffffff) { ctx->err = "chaindp_align_set_targets: falling offsets or a sequence of 2^31 - 1 bases or more"; return CHAINDP_ERR_ARG; }
	const int64_t total = seq_off[n_seqs];
	if (total > 0 && !seq) { ctx->err = "chaindp_align_set_targets: NULL sequence"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->al_t_off.clear();
	int rc;
	// the characters are staged behind the codes and encoded in place of nothing: codes [0, total), characters [total, 2 total)
	if ((rc = ksw_grow(ctx, ctx->al_tgt, (size_t)total * 2 + 16, "targets", "chaindp_align_set_targets"))) return rc;
	if ((rc = ksw_grow(ctx, ctx->al_toff, (size_t)(n_seqs + 1) * sizeof(int64_t), "target offsets", "chaindp_align_set_targets"))) return rc;
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, host_copy(ctx->al_toff.p, seq_off, (size_t)(n_seqs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
	if (total) {
		HIP_TRY(ctx, host_copy((char*)ctx->al_tgt.p + total, seq, (size_t)total, hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, launch_align_encode(st, total, (const char*)ctx->al_tgt.p + total, (uint8_t*)ctx->al_tgt.p));
	}
	HIP_TRY(ctx, hipStreamSynchronize(st));
	ctx->al_t_off.assign(seq_off, seq_off + n_seqs + 1);
	return CHAINDP_OK;
}

extern "C" int chaindp_align_clear_targets(chaindp_ctx_t *ctx)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->pool.release(&ctx->al_tgt.p); ctx->al_tgt.cap = 0;
	ctx->pool.release(&ctx->al_toff.p); ctx->al_toff.cap = 0;
	ctx->al_t_off.clear();
	return CHAINDP_OK;
}

extern "C" int chaindp_align_debug_check(const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const int64_t *a_off,
                                         const chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, int64_t n_t, const int64_t *t_off,
                                         int64_t out[2])
{
	AlignPlan pl;
	if (align_plan((const AlignOpt*)opt, n_reads, seq_off, a_off, (const uint64_t*)a, regs_off, (const int32_t*)regs, n_t, t_off, pl)) return CHAINDP_ERR_ARG;
	if (out) { out[0] = pl.n_regs; out[1] = pl.n_slots; }
	return CHAINDP_OK;
}

extern "C" int chaindp_align_debug_ms(chaindp_ctx_t *ctx, double ms[5])
{
	if (!ctx || !ms) return CHAINDP_ERR_ARG;
	for (int k = 0; k < 5; ++k) ms[k] = ctx->al_ms[k];
	return CHAINDP_OK;
}

extern "C" int chaindp_align1(chaindp_ctx_t *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                              const int64_t *a_off, chaindp_anchor_t *a, const int64_t *regs_off, chaindp_reg_t *regs, chaindp_reg_t *regs2,
                              chaindp_align_extra_t *extra, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap)
{
	return align1_impl(ctx, opt, n_reads, seq_off, seq, a_off, a, regs_off, regs, regs2, extra, cigar_off, cigar, cigar_cap, nullptr);
}

int chaindp::align1_impl(chaindp_ctx *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const int64_t *a_off,
                         chaindp_anchor_t *a, const int64_t *regs_off, chaindp_reg_t *regs, chaindp_reg_t *regs2, chaindp_align_extra_t *extra,
                         int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, AlignResident *res)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!cigar_off) { ctx->err = "chaindp_align1: NULL cigar_off"; return CHAINDP_ERR_ARG; }
	if (!res && (cigar_cap < 0 || (cigar_cap > 0 && !cigar))) { ctx->err = "chaindp_align1: cigar_cap without a cigar array"; return CHAINDP_ERR_ARG; }
	AlignPlan planned;
	const int64_t n_t = (int64_t)ctx->al_t_off.size() - 1;
	if (!(res && res->plan) && align_plan((const AlignOpt*)opt, n_reads, seq_off, a_off, (const uint64_t*)a, regs_off, (const int32_t*)regs, n_t < 0 ? 0 : n_t,
	               n_t < 0 ? nullptr : ctx->al_t_off.data(), planned)) {
		ctx->err = planned.err;
		return CHAINDP_ERR_ARG;
	}
	const AlignPlan &ap = res && res->plan ? *res->plan : planned;
	const AlignOpt o = *(const AlignOpt*)opt;
	KswScore sc;
	if (!ksw_plan_score(o.a, o.b, o.q, o.e, o.q2, o.e2, sc)) { ctx->err = "chaindp_align1: scoring"; return CHAINDP_ERR_ARG; }
	cigar_off[0] = 0;
	const int64_t G = ap.n_regs;
	if (G == 0) return CHAINDP_OK;
	if (!regs2 || !extra) { ctx->err = "chaindp_align1: NULL regs2 or extra"; return CHAINDP_ERR_ARG; }
	if (ap.n_bases > 0 && !seq && !res) { ctx->err = "chaindp_align1: NULL sequence"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // a buffer that grows is freed: nothing of an earlier call may be in flight
	hipStream_t st = ctx->stream;
	int rc;
	// the batch: offsets, the regions' reads, anchors, regions, bases
	Carve in;
	// (the reads' own part is the caller's where the batch is resident)
	const size_t o_seq_off = in.take(res ? 0 : (size_t)(n_reads + 1) * 8), o_a_off = in.take(res ? 0 : (size_t)(n_reads + 1) * 8), o_slot_off = in.take((size_t)(G + 1) * 8),
	             o_first = in.take((size_t)(G + 1) * 8), o_reg_read = in.take((size_t)G * 4), o_a = in.take(res ? 0 : (size_t)ap.n_anchors * 16),
	             o_regs = in.take((size_t)G * 80), o_regs2 = in.take((size_t)G * 80), o_seq = in.take(res ? 0 : (size_t)ap.n_bases);
	if ((rc = ksw_grow(ctx, ctx->al_in, in.at + 16, "the batch", WHO))) return rc;
	Carve rg;
	const size_t o_areg = rg.take((size_t)G * sizeof(AlignReg)), o_stitch = rg.take((size_t)G * sizeof(AlignStitch)), o_extra = rg.take((size_t)G * 20),
	             o_coff = rg.take((size_t)(G + 1) * 8);
	if ((rc = ksw_grow(ctx, ctx->al_reg, rg.at + 16, "region records", WHO))) return rc;
	const size_t S = (size_t)ap.n_slots;
	if ((rc = ksw_grow(ctx, ctx->al_slot, S * sizeof(KswProb) + 16, "problem slots", WHO))) return rc;
	Carve sd;
	const size_t o_side = sd.take(S * sizeof(AlignSide)), o_kbuf = sd.take(S * 4);
	if ((rc = ksw_grow(ctx, ctx->al_side, sd.at + 16, "problem sides", WHO))) return rc;
	char *d_in = (char*)ctx->al_in.p, *d_rg = (char*)ctx->al_reg.p;
	AlignDev d = {};
	d.n_regs = (int)G;
	d.seq_off = (const int64_t*)(d_in + o_seq_off); d.a_off = (const int64_t*)(d_in + o_a_off); d.slot_off = (const int64_t*)(d_in + o_slot_off);
	d.first = (const int64_t*)(d_in + o_first); d.reg_read = (const int32_t*)(d_in + o_reg_read); d.a = d_in + o_a;
	d.regs = (int32_t*)(d_in + o_regs); d.regs2 = (int32_t*)(d_in + o_regs2); d.seq = d_in + o_seq;
	if (res) { d.seq_off = res->seq_off; d.a_off = res->a_off; d.a = res->a; d.seq = res->seq; }
	d.t_off = (const int64_t*)ctx->al_toff.p; d.tcodes = (const uint8_t*)ctx->al_tgt.p;
	d.slots = (KswProb*)ctx->al_slot.p; d.side = (AlignSide*)((char*)ctx->al_side.p + o_side); d.kbuf = (int32_t*)((char*)ctx->al_side.p + o_kbuf);
	d.areg = (AlignReg*)(d_rg + o_areg); d.stitch = (AlignStitch*)(d_rg + o_stitch); d.extra = (int32_t*)(d_rg + o_extra);
	int64_t *d_coff = (int64_t*)(d_rg + o_coff);
	auto up = [&](size_t off, const void *src, size_t bytes) { return bytes ? host_copy(d_in + off, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
	if (!res) {
		HIP_TRY(ctx, up(o_seq_off, seq_off, (size_t)(n_reads + 1) * 8));
		HIP_TRY(ctx, up(o_a_off, a_off, (size_t)(n_reads + 1) * 8));
		HIP_TRY(ctx, up(o_a, a, (size_t)ap.n_anchors * 16));
		HIP_TRY(ctx, up(o_seq, seq, (size_t)ap.n_bases));
	}
	HIP_TRY(ctx, up(o_slot_off, ap.slot_off.data(), (size_t)(G + 1) * 8));
	HIP_TRY(ctx, up(o_reg_read, ap.reg_read.data(), (size_t)G * 4));
	HIP_TRY(ctx, up(o_regs, regs, (size_t)G * 80));
	HIP_TRY(ctx, up(o_regs2, regs2, (size_t)G * 80));
	StageEvents ev(ctx);
	HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_align_plan(st, o, d));
	HIP_TRY(ctx, ev.mark(0));
	std::vector<AlignReg> areg((size_t)G);
	std::vector<KswProb> slots(S);
	HIP_TRY(ctx, host_copy(areg.data(), d.areg, (size_t)G * sizeof(AlignReg), hipMemcpyDeviceToHost, st));
	if (S) HIP_TRY(ctx, host_copy(slots.data(), d.slots, S * sizeof(KswProb), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	// the first pass: every extension and every fill of every region
	KswPlan p1;
	p1.sc = sc;
	std::vector<int32_t> src_slot;
	std::vector<int64_t> first;
	int64_t n_bases = 0;
	align_compact(ap, areg, slots, p1.prob, src_slot, first, n_bases);
	ksw_plan_route(p1, ctx->dp.cus, ctx->ksw_grid_cap);
	const size_t P = p1.prob.size();
	d.n_prob = (int64_t)P;
	if ((rc = ksw_reserve(ctx, p1, n_bases, WHO))) return rc;
	Carve pc;
	const size_t o_prob = pc.take(P * sizeof(KswProb)), o_src = pc.take(P * 4), o_code = pc.take(P * 4), o_sec = pc.take(P * 4);
	if ((rc = ksw_grow(ctx, ctx->al_code, pc.at + 16, "problem list", WHO))) return rc;
	if ((rc = ksw_grow(ctx, ctx->al_ez1, P * KSW_EZ_WORDS * 4 + 16, "first-pass results", WHO))) return rc;
	if ((rc = ksw_grow(ctx, ctx->al_cig1, (size_t)p1.cig_words * 4 + 16, "first-pass CIGARs", WHO))) return rc;
	if ((rc = ksw_grow(ctx, ctx->al_stage, (size_t)p1.cig_words * 4 + 16, "stitched CIGARs", WHO))) return rc;
	char *d_pc = (char*)ctx->al_code.p;
	d.prob = (const KswProb*)(d_pc + o_prob); d.src_slot = (const int32_t*)(d_pc + o_src); d.code = (int32_t*)(d_pc + o_code); d.sec = (const int32_t*)(d_pc + o_sec);
	d.ez1 = (const int32_t*)ctx->al_ez1.p; d.cig1 = (const uint32_t*)ctx->al_cig1.p; d.stage = (uint32_t*)ctx->al_stage.p;
	HIP_TRY(ctx, up(o_first, first.data(), (size_t)(G + 1) * 8));
	std::vector<int32_t> sec(P, -1);
	KswPlan p2;
	if (P) {
		HIP_TRY(ctx, host_copy(d_pc + o_prob, p1.prob.data(), P * sizeof(KswProb), hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, host_copy(d_pc + o_src, src_slot.data(), P * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, ev.mark(-1));
		HIP_TRY(ctx, launch_align_gather(st, d, (uint8_t*)ctx->ksw_bases.p));
		HIP_TRY(ctx, ev.mark(0));
		if ((rc = ksw_dispatch(ctx, p1, nullptr))) return rc;
		HIP_TRY(ctx, ev.mark(1));
		const KswView v1 = ksw_view(ctx, P);
		int max_t = 0;
		for (size_t c = 0; c < P; ++c) max_t = std::max(max_t, p1.prob[c].tlen);
		const int lds_t = std::max(std::min(max_t, o.max_gap - 1), 0) + 1;
		HIP_TRY(ctx, launch_align_zdrop(st, o, d, (const uint8_t*)ctx->ksw_bases.p, v1.ez, v1.cig, lds_t));
		HIP_TRY(ctx, ev.mark(2));
		// the first pass's answers out of the DP's buffers: the second pass writes there
		HIP_TRY(ctx, hipMemcpyAsync(ctx->al_ez1.p, v1.ez, P * KSW_EZ_WORDS * 4, hipMemcpyDeviceToDevice, st));
		if (p1.cig_words) HIP_TRY(ctx, hipMemcpyAsync(ctx->al_cig1.p, v1.cig, (size_t)p1.cig_words * 4, hipMemcpyDeviceToDevice, st));
		std::vector<int32_t> code(P);
		HIP_TRY(ctx, host_copy(code.data(), d.code, P * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		// the second pass: the fills whose code is not 0, without the approximate maximum, under the Z-drop the code names
		p2.sc = sc;
		for (size_t c = 0; c < P; ++c) {
			if (code[c] != 1 && code[c] != 2) continue;
			KswProb p = p1.prob[c];
			p.flag = 0; p.zdrop = code[c] == 2 ? o.zdrop_inv : o.zdrop;
			sec[c] = (int32_t)p2.prob.size();
			p2.prob.push_back(p);
		}
		HIP_TRY(ctx, host_copy(d_pc + o_sec, sec.data(), P * 4, hipMemcpyHostToDevice, st));
		if (!p2.prob.empty()) {
			ksw_plan_route(p2, ctx->dp.cus, ctx->ksw_grid_cap);
			if ((rc = ksw_reserve(ctx, p2, n_bases, WHO))) return rc;
			HIP_TRY(ctx, ev.mark(-1));
			if ((rc = ksw_dispatch(ctx, p2, nullptr))) return rc;
			HIP_TRY(ctx, ev.mark(1));
		}
	}
	const KswView v2 = ksw_view(ctx, p2.prob.size());
	HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_align_stitch(st, o, d, p1.cig_words, v2.prob, v2.ez, v2.cig));
	HIP_TRY(ctx, ev.mark(3));
	HIP_TRY(ctx, launch_align_extra(st, o, d));
	HIP_TRY(ctx, ev.mark(4));
	HIP_TRY(ctx, host_copy(extra, d.extra, (size_t)G * 20, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(regs, d.regs, (size_t)G * 80, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(regs2, d.regs2, (size_t)G * 80, hipMemcpyDeviceToHost, st));
	if (ap.n_anchors && !res) HIP_TRY(ctx, host_copy(a, d.a, (size_t)ap.n_anchors * 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const int64_t total = cigar_prefix((const int32_t*)extra, 5, 4, G, cigar_off);
	const std::function<hipError_t(uint32_t*)> pack = [&](uint32_t *out) {
		hipError_t e;
		return (e = ev.mark(-1)) || (e = launch_align_pack(st, d, d_coff, out)) ? e : ev.mark(4);
	};
	if (res) { res->d_regs = d.regs; res->d_extra = d.extra; }
	const int ret = res ? cigar_pack_dev(ctx, cigar_off, G, total, d_coff, res->room, pack) : cigar_pack_out(ctx, WHO, cigar_off, G, total, cigar, cigar_cap, d_coff, pack);
	if (ret != CHAINDP_ERR_HIP && (rc = ev.fold(ctx->al_ms, 5))) return rc;
	return ret;
}
