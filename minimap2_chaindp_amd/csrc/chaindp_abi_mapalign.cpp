// chaindp_abi_mapalign.cpp -- reads mapped with base alignment in one call (include/chaindp_map_align.h): chain_post's result handed to
// the alignment stages on the device.  The checks are chaindp_handoff_plan.h's, the kernels handoff/chaindp_handoff.hip's, the stages
// align_reads_compute (chaindp_abi_reads.cpp) and align_post_resident (chaindp_abi_apost.cpp); this file owns the hand-off's buffers,
// the copies and the order of the calls:
//   count -> scan -> move -> (regions' offsets, regions, a_off, squeezed anchors down, once: the stages plan on the host) ->
//   align_reads_compute on the resident bases and anchors -> align_post_resident on the resident rep_len -> the result down, or later
//   by chaindp_align_post_fetch; the anchors' marks down only if the caller wants a
#include "chaindp_ctx.h"
#include "../../include/chaindp_map_align.h"
#include <string.h>

using namespace chaindp;

static const char *const WHO = "chaindp_align_resident";

extern "C" int chaindp_map_align_debug_set_lds_cap(chaindp_ctx_t *ctx, int cap, int32_t *out_cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (cap < 0 || cap > HO_LDS_CAP) { ctx->err = "chaindp_map_align_debug_set_lds_cap: cap outside 0.." + std::to_string(HO_LDS_CAP); return CHAINDP_ERR_ARG; }
	ctx->ho_lds_cap = cap ? cap : HO_LDS_CAP;
	if (out_cap) *out_cap = HO_LDS_CAP;
	return CHAINDP_OK;
}

extern "C" int chaindp_map_align_debug_ms(chaindp_ctx_t *ctx, double ms[7])
{
	if (!ctx || !ms) return CHAINDP_ERR_ARG;
	ms[0] = ctx->ho_ms;
	for (int k = 0; k < 4; ++k) ms[1 + k] = ctx->rd_ms[k];
	ms[5] = ctx->ap_ms[0]; ms[6] = ctx->ap_ms[1];
	return CHAINDP_OK;
}

extern "C" int chaindp_map_align_debug_handoff(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *a_off)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->ho_n_reads < 0 || n_reads != ctx->ho_n_reads || !regs_off || !a_off || regs_cap < 0 || (regs_cap > 0 && !regs)) {
		ctx->err = "chaindp_map_align_debug_handoff: no hand-off of n_reads reads was made, or a NULL array";
		return CHAINDP_ERR_ARG;
	}
	memcpy(regs_off, ctx->ho_h_regs_off.data(), (size_t)(n_reads + 1) * 8);
	memcpy(a_off, ctx->ho_h_a_off.data(), (size_t)(n_reads + 1) * 8);
	const int64_t N = regs_off[n_reads];
	if (N > regs_cap) { ctx->err = "chaindp_map_align_debug_handoff: " + std::to_string((long long)N) + " regions, room for " + std::to_string((long long)regs_cap); return CHAINDP_ERR_CAPACITY; }
	if (N) memcpy(regs, ctx->ho_h_regs.data(), (size_t)N * 80);
	return CHAINDP_OK;
}

extern "C" int chaindp_align_resident_anchors(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *a_off, chaindp_anchor_t *a, int64_t a_cap)
{
	static const char *const who = "chaindp_align_resident_anchors";
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->ho_n_reads < 0 || n_reads != ctx->ho_n_reads || ctx->rd_n_reads != n_reads) { ctx->err = std::string(who) + ": no result of chaindp_align_resident of n_reads reads is resident"; return CHAINDP_ERR_ARG; }
	if (!a_off || a_cap < 0 || (a_cap > 0 && !a)) { ctx->err = std::string(who) + ": NULL a_off, or a_cap without a"; return CHAINDP_ERR_ARG; }
	memcpy(a_off, ctx->ho_h_a_off.data(), (size_t)(n_reads + 1) * 8);
	const int64_t n_a = a_off[n_reads];
	if (n_a > a_cap) { ctx->err = std::string(who) + ": " + std::to_string((long long)n_a) + " anchors, room for " + std::to_string((long long)a_cap); return CHAINDP_ERR_CAPACITY; }
	if (n_a == 0) return CHAINDP_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, host_copy(a, ctx->ho_a.p, (size_t)n_a * 16, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

// what the context holds, for handoff_check_resident
static HandoffResident resident_facts(const chaindp_ctx *ctx)
{
	HandoffResident h;
	h.post_n_reads = ctx->post_n_reads; h.post_cigar = ctx->post_cigar;
	h.hits_resident = ctx->regs_resident && ctx->bot_n_reads >= 0 && ctx->bot_n_reads == ctx->n_reads;
	h.rep_resident = ctx->mp_resident && ctx->d_rep_len != nullptr;
	h.from_sketch = ctx->from_sketch; h.sketch_valid = ctx->sk_valid;
	h.sketch_reads = ctx->sk_n_reads; h.sketch_seqs = (int64_t)ctx->sk_seq_len.size();
	h.n_t = (int64_t)ctx->al_t_off.size() - 1; h.t_off = ctx->al_t_off.data();
	h.n_ref = (int64_t)ctx->post_ref_len.size(); h.ref_len = ctx->post_ref_len.data();
	return h;
}

static int check_call(chaindp_ctx *ctx, const chaindp_align_opt_t *aopt, const chaindp_post_opt_t *popt, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs,
                      chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t *need,
                      int64_t *a_off, chaindp_anchor_t *a)
{
	std::string err;
	if (handoff_check_call((const ApostOpt*)popt, aopt != nullptr, n_reads, regs_cap, cigar_cap, out_off && need, out_regs && out_extra && out_dp_max2 && cigar_off,
	                       cigar != nullptr, a_off != nullptr, a != nullptr, err)) {
		ctx->err = std::string(WHO) + ": " + err;
		return CHAINDP_ERR_ARG;
	}
	// what the alignment stage refuses about its options, before anything is launched: its own check on a batch of no reads
	static const int64_t none[1] = {0};
	const int64_t n_t = (int64_t)ctx->al_t_off.size() - 1;
	AlignPlan ap;
	if (reads_check((const AlignOpt*)aopt, 0, none, none, nullptr, none, nullptr, n_t < 0 ? 0 : n_t, n_t < 0 ? nullptr : ctx->al_t_off.data(), regs_cap, cigar_cap, ap, err)) {
		ctx->err = std::string(WHO) + ": " + err;
		return CHAINDP_ERR_ARG;
	}
	return CHAINDP_OK;
}

// The hand-off on the device and its result on the host (ctx->ho_h_*): R reads, N regions at d_regs_off / d_regs, their anchors (n_b in
// all) at d_b_off / d_sq.  d comes back with the addresses of what it left resident.  Two trips down: the offsets, the regions and the
// kernel's error word first, then the squeezed anchors, whose number only the offsets tell (typically a third of n_b: what
// mm_select_sub dropped stays behind).
static int handoff_device(chaindp_ctx *ctx, const char *who, int64_t R, int64_t N, int64_t n_b, const unsigned long long *d_regs_off, const int32_t *d_regs,
                          const int64_t *d_b_off, const void *d_sq, HandoffDev &d)
{
	std::vector<int64_t> &h_regs_off = ctx->ho_h_regs_off, &h_a_off = ctx->ho_h_a_off;
	std::vector<int32_t> &h_regs = ctx->ho_h_regs;
	std::vector<uint64_t> &h_a = ctx->ho_h_a;
	h_regs_off.assign((size_t)R + 1, 0); h_a_off.assign((size_t)R + 1, 0); h_regs.assign((size_t)N * HO_REG_WORDS, 0); h_a.clear();
	hipStream_t st = ctx->stream;
	int rc;
	Carve of;
	const size_t o_aoff = of.take((size_t)(R + 2) * 8), o_tile = of.take((size_t)(R / 1024 + 2) * 8), o_err = of.take(4);
	if ((rc = ksw_grow(ctx, ctx->ho_off, of.at + 16, "the anchors' offsets", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ho_a, (size_t)n_b * 16 + 16, "the squeezed anchors", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ho_regs, (size_t)N * 80 + 16, "the regions", who))) return rc;
	char *d_of = (char*)ctx->ho_off.p;
	d = HandoffDev{};
	d.n_reads = R; d.a_off = (unsigned long long*)(d_of + o_aoff); d.a = ctx->ho_a.p; d.out_regs = (int32_t*)ctx->ho_regs.p; d.err = (int32_t*)(d_of + o_err);
	if (N == 0) {
		// a batch without regions: nothing to move, the stages still get addresses
		HIP_TRY(ctx, hipMemsetAsync(d.a_off, 0, (size_t)(R + 1) * 8, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		ctx->ho_ms = ctx->prof ? 0 : -1;
		return CHAINDP_OK;
	}
	d.regs_off = d_regs_off; d.regs = d_regs; d.b_off = d_b_off; d.sq = d_sq;
	HIP_TRY(ctx, hipMemsetAsync(d.err, 0, 4, st));
	StageEvents ev(ctx);
	HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_handoff(st, d, (unsigned long long*)(d_of + o_tile), ctx->ho_lds_cap));
	HIP_TRY(ctx, ev.mark(0));
	int32_t flagged = 0;
	HIP_TRY(ctx, host_copy(h_regs_off.data(), d_regs_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(h_a_off.data(), d.a_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(h_regs.data(), d.out_regs, (size_t)N * 80, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, host_copy(&flagged, d.err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	double ms[1] = {-1};
	if (ctx->prof && (rc = ev.fold(ms, 1))) return rc;
	ctx->ho_ms = ms[0];
	const int64_t n_a = h_a_off[(size_t)R];
	std::string err;
	if (flagged) err = "a region does not lie inside its read's chain anchors";
	if (flagged || h_regs_off[(size_t)R] != N || n_a < 0 || n_a > n_b || handoff_check_down(R, h_regs_off.data(), h_regs.data(), h_a_off.data(), err)) {
		ctx->err = std::string(who) + ": the hand-off left inconsistent regions: " + err;
		return CHAINDP_ERR_HIP;
	}
	h_a.assign((size_t)n_a * 2, 0);
	if (n_a) HIP_TRY(ctx, host_copy(h_a.data(), d.a, (size_t)n_a * 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	return CHAINDP_OK;
}

extern "C" int chaindp_map_align_debug_run_handoff(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *regs_off, const chaindp_reg_t *regs, const int64_t *b_off,
                                                   const chaindp_anchor_t *b, chaindp_reg_t *out_regs, int64_t *a_off, chaindp_anchor_t *a)
{
	static const char *const who = "chaindp_map_align_debug_run_handoff";
	if (!ctx) return CHAINDP_ERR_ARG;
	std::string err;
	if (handoff_check_up(n_reads, regs_off, (const int32_t*)regs, b_off, b != nullptr, out_regs != nullptr, a_off != nullptr, a != nullptr, err)) {
		ctx->err = std::string(who) + ": " + err;
		return CHAINDP_ERR_ARG;
	}
	ctx->ho_n_reads = -1;
	a_off[0] = 0;
	if (n_reads == 0) return CHAINDP_OK;
	const int64_t R = n_reads, N = regs_off[R], n_b = b_off[R];
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	hipStream_t st = ctx->stream;
	Carve in;
	const size_t o_roff = in.take((size_t)(R + 1) * 8), o_boff = in.take((size_t)(R + 1) * 8), o_regs = in.take((size_t)N * 80), o_b = in.take((size_t)n_b * 16);
	if (int rc = ksw_grow(ctx, ctx->ho_in, in.at + 16, "the regions and anchors", who)) return rc;
	char *d_in = (char*)ctx->ho_in.p;
	HIP_TRY(ctx, host_copy(d_in + o_roff, regs_off, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, host_copy(d_in + o_boff, b_off, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, st));
	if (N) HIP_TRY(ctx, host_copy(d_in + o_regs, regs, (size_t)N * 80, hipMemcpyHostToDevice, st));
	if (n_b) HIP_TRY(ctx, host_copy(d_in + o_b, b, (size_t)n_b * 16, hipMemcpyHostToDevice, st));
	HandoffDev d;
	if (int rc = handoff_device(ctx, who, R, N, n_b, (const unsigned long long*)(d_in + o_roff), (const int32_t*)(d_in + o_regs), (const int64_t*)(d_in + o_boff), d_in + o_b, d)) return rc;
	memcpy(a_off, ctx->ho_h_a_off.data(), (size_t)(R + 1) * 8);
	if (N) memcpy(out_regs, ctx->ho_h_regs.data(), (size_t)N * 80);
	if (!ctx->ho_h_a.empty()) memcpy(a, ctx->ho_h_a.data(), ctx->ho_h_a.size() * 8);
	return CHAINDP_OK;
}

// the call behind its argument checks
static int align_resident_impl(chaindp_ctx *ctx, const chaindp_align_opt_t *aopt, const chaindp_post_opt_t *popt, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs,
                               chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap,
                               int64_t need[2], int64_t *a_off, chaindp_anchor_t *a)
{
	std::string err;
	if (handoff_check_resident(resident_facts(ctx), n_reads, err)) { ctx->err = std::string(WHO) + ": " + err; return CHAINDP_ERR_ARG; }
	const int64_t R = n_reads, N = ctx->post_n_out, n_b = N ? ctx->bot_n_b : 0;
	ctx->ho_n_reads = -1;
	std::vector<int64_t> seq_off;
	handoff_seq_off(ctx->sk_seq_len, seq_off);
	AlignResident from;
	from.seq_off = ctx->sk.seq_off; from.seq = (const char*)ctx->sk.seq; from.a_off = nullptr; from.a = nullptr;
	ctx->ho_h_regs_off.assign(1, 0); ctx->ho_h_a_off.assign(1, 0); ctx->ho_h_regs.clear(); ctx->ho_h_a.clear();
	if (R > 0) {
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // a buffer that grows is freed: nothing of an earlier call may be in flight
		HandoffDev d;
		if (int rc = handoff_device(ctx, WHO, R, N, n_b, ctx->d_post_off, (const int32_t*)ctx->post_out.p, ctx->bot.b_off, ctx->post_sq.p, d)) return rc;
		from.a_off = (const int64_t*)d.a_off; from.a = d.a;
	}
	ctx->ho_n_reads = R;
	std::vector<int64_t> &h_regs_off = ctx->ho_h_regs_off, &h_a_off = ctx->ho_h_a_off;
	std::vector<uint64_t> &h_a = ctx->ho_h_a;
	// the stages, on what is resident; what they refuse is this call's refusal
	int rc = align_reads_compute(ctx, aopt, R, seq_off.data(), nullptr, h_a_off.data(), (chaindp_anchor_t*)h_a.data(), h_regs_off.data(), (const chaindp_reg_t*)ctx->ho_h_regs.data(),
	                             regs_cap, cigar_cap, &from, a != nullptr);
	if (rc) return rc;
	if ((rc = align_post_resident(ctx, WHO, popt, R, nullptr, ctx->d_rep_len))) return rc;
	if (a_off) memcpy(a_off, h_a_off.data(), (size_t)(R + 1) * 8);
	if (a && !h_a.empty()) memcpy(a, h_a.data(), h_a.size() * 8);
	return align_post_deliver(ctx, WHO, R, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need);
}

extern "C" int chaindp_align_resident(chaindp_ctx_t *ctx, const chaindp_align_opt_t *aopt, const chaindp_post_opt_t *popt, int64_t n_reads, int64_t *out_off,
                                      chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off,
                                      uint32_t *cigar, int64_t cigar_cap, int64_t need[2], int64_t *a_off, chaindp_anchor_t *a)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (int rc = check_call(ctx, aopt, popt, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need, a_off, a)) return rc;
	return align_resident_impl(ctx, aopt, popt, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need, a_off, a);
}

extern "C" int chaindp_map_align_seqs(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int w, int k, int is_hpc, int flag, int max_occ, const chaindp_params_t *par,
                                      int min_cnt, const chaindp_post_opt_t *popt, const chaindp_align_opt_t *aopt, int64_t n_reads, const int64_t *seq_off,
                                      const char *seq, const uint32_t *bid, const uint32_t *hash, const int32_t *ref_len, int32_t n_ref, int64_t *out_off,
                                      chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off,
                                      uint32_t *cigar, int64_t cigar_cap, int64_t need[2], int64_t *a_off, chaindp_anchor_t *a, int32_t *rep_len, int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	// everything either half would refuse about the call's own arguments, before anything is launched
	if (int rc = check_call(ctx, aopt, popt, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need, a_off, a)) return rc;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
	if (n_reads > 0 && (!hash || !bid)) { ctx->err = "chaindp_map_align_seqs: NULL bid or hash"; return CHAINDP_ERR_ARG; }
	if (n_ref < 0 || (n_ref > 0 && !ref_len)) { ctx->err = "chaindp_map_align_seqs: NULL ref_len"; return CHAINDP_ERR_ARG; }
	if (par->n_segs > 1) { ctx->err = "chaindp_map_align_seqs takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	if (!ix || ix->device != ctx->device) { ctx->err = "index image missing or on another device"; return CHAINDP_ERR_ARG; }
	{
		HandoffResident h;                               // the targets against the call's own ref_len: the rest becomes true below
		h.n_t = (int64_t)ctx->al_t_off.size() - 1; h.t_off = ctx->al_t_off.data(); h.n_ref = n_ref; h.ref_len = ref_len;
		h.post_n_reads = n_reads; h.post_cigar = h.hits_resident = h.rep_resident = h.from_sketch = h.sketch_valid = true; h.sketch_reads = h.sketch_seqs = n_reads;
		std::string err;
		if (handoff_check_resident(h, n_reads, err)) { ctx->err = "chaindp_map_align_seqs: " + err; return CHAINDP_ERR_ARG; }
	}
	// chaindp_map_seqs, the hits left in HBM
	std::vector<int64_t> off((size_t)(n_reads > 0 ? n_reads + 1 : 1));
	if ((rc = chaindp_sketch(ctx, w, k, is_hpc, n_reads, seq_off, seq, nullptr, off.data())) != CHAINDP_OK) return rc;
	const int32_t *qlen = nullptr;
	if ((rc = map_prefix(ctx, ix, flag, max_occ, par, min_cnt, n_reads, nullptr, nullptr, bid, qlen, nullptr, hash, rep_len, n_anchors, nullptr, nullptr, 0))) return rc;
	if ((rc = chain_post_impl(ctx, popt, nullptr, nullptr, ref_len, n_ref, nullptr, nullptr, off.data(), nullptr, 0, nullptr, nullptr, true))) return rc;
	return align_resident_impl(ctx, aopt, popt, n_reads, out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need, a_off, a);
}
