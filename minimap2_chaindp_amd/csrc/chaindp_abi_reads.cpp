// chaindp_abi_reads.cpp -- whole reads in one call (include/chaindp_align_reads.h): mm_align_skeleton's loop around the two alignment stages.
// Which regions a round aligns, where a record stands in its read's list and the place key are chaindp_reads_plan.h's, the stages
// are align1_impl and align1_inv_impl (chaindp_ctx.h) on a batch that is resident, the end of the loop reads/chaindp_reads.hip's; this
// file owns the loop's buffers, the two pools that outlive a round, the copies and the order of the calls:
//   bases, anchors up -> round 0, 1, ... (each: records into the pool, CIGARs packed into the pool, regs2 down) -> inversions over the
//   lists (the same) -> anchors down -> lists up -> finish -> gather -> (need, out_off down) -> the result down, or later by fetch
// align_reads_compute is everything up to the resident result (chaindp_align_reads_post runs the post stage on it before anything comes
// down); deliver brings a resident result into the caller's arrays.
#include "chaindp_ctx.h"
#include "../../include/chaindp_align_reads.h"
#include <string.h>

using namespace chaindp;

static const char *const WHO = "chaindp_align_reads";

// A pool that outlives the rounds: pair[cur] holds `used` bytes that must survive.  Room for need bytes: nothing while it fits; else
// the other buffer of the pair is grown (what it held is of no use), the used bytes copied over and the old buffer released.
static int pool_grow(chaindp_ctx *ctx, DevGrow pair[2], int &cur, size_t used, size_t need, const char *what)
{
	if (pair[cur].p && need <= pair[cur].cap) return CHAINDP_OK;
	DevGrow &to = pair[cur ^ 1], &from = pair[cur];
	if (int rc = ksw_grow(ctx, to, need + need / 2, what, WHO)) return rc;
	if (used && from.p) HIP_TRY(ctx, hipMemcpyAsync(to.p, from.p, used, hipMemcpyDeviceToDevice, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->pool.release(&from.p); from.cap = 0;
	cur ^= 1;
	return CHAINDP_OK;
}

extern "C" int chaindp_align_reads_debug_check(const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const int64_t *a_off,
                                               const chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, int64_t n_t, const int64_t *t_off,
                                               int64_t regs_cap, int64_t cigar_cap, int64_t out[2])
{
	std::string err;
	AlignPlan ap;
	if (reads_check((const AlignOpt*)opt, n_reads, seq_off, a_off, (const uint64_t*)a, regs_off, (const int32_t*)regs, n_t, t_off, regs_cap, cigar_cap, ap, err)) return CHAINDP_ERR_ARG;
	if (out) { out[0] = n_reads ? regs_off[n_reads] : 0; out[1] = n_reads; }
	return CHAINDP_OK;
}

extern "C" int chaindp_align_reads_debug_ms(chaindp_ctx_t *ctx, double ms[4])
{
	if (!ctx || !ms) return CHAINDP_ERR_ARG;
	for (int k = 0; k < 4; ++k) ms[k] = ctx->rd_ms[k];
	return CHAINDP_OK;
}

extern "C" int chaindp_align_reads_debug_set_lds_cap(chaindp_ctx_t *ctx, int cap, int32_t *out_cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (cap < 0 || cap > RD_LDS_CAP) { ctx->err = "chaindp_align_reads_debug_set_lds_cap: cap outside 0.." + std::to_string(RD_LDS_CAP); return CHAINDP_ERR_ARG; }
	ctx->rd_lds_cap = cap ? cap : RD_LDS_CAP;
	if (out_cap) *out_cap = RD_LDS_CAP;
	return CHAINDP_OK;
}

extern "C" int chaindp_align_reads_debug_rounds(chaindp_ctx_t *ctx, int64_t *out, int64_t cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->rd_n_reads < 0 || !out || cap < 1) { ctx->err = "chaindp_align_reads_debug_rounds: no result is resident, or no room"; return CHAINDP_ERR_ARG; }
	out[0] = (int64_t)ctx->rd_rounds.size();
	for (int64_t k = 0; k < out[0] && k + 1 < cap; ++k) out[1 + k] = ctx->rd_rounds[(size_t)k];
	return CHAINDP_OK;
}

extern "C" int chaindp_align_reads_debug_placed(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *placed_off, chaindp_reg_t *placed, int64_t placed_cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->rd_n_reads < 0 || n_reads != ctx->rd_n_reads || !placed_off) { ctx->err = "chaindp_align_reads_debug_placed: not the reads of a resident result"; return CHAINDP_ERR_ARG; }
	if (placed_cap < 0 || (placed_cap > 0 && !placed)) { ctx->err = "chaindp_align_reads_debug_placed: placed_cap without an array"; return CHAINDP_ERR_ARG; }
	placed_off[0] = 0;
	if (n_reads == 0) return CHAINDP_OK;
	memcpy(placed_off, ctx->rd_list_off.data(), (size_t)(n_reads + 1) * 8);
	const size_t L = ctx->rd_item.size();
	if ((int64_t)L > placed_cap) { ctx->err = "chaindp_align_reads_debug_placed: " + std::to_string(L) + " records, room for " + std::to_string((long long)placed_cap); return CHAINDP_ERR_CAPACITY; }
	if (L == 0) return CHAINDP_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	std::vector<int32_t> order(L);
	HIP_TRY(ctx, host_copy(order.data(), (char*)ctx->rd_list.p + ctx->rd_out_at[4], L * 4, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	// the pool in one copy, the records picked on the host
	std::vector<int32_t> rec((size_t)ctx->rd_n_rec * RD_REC_WORDS);
	HIP_TRY(ctx, host_copy(rec.data(), ctx->rd_rec[ctx->rd_rec_cur].p, rec.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	for (size_t k = 0; k < L; ++k) {
		const int32_t at = order[k];
		if (at < 0 || (size_t)at >= L) { ctx->err = "chaindp_align_reads_debug_placed: the placed order is no permutation"; return CHAINDP_ERR_HIP; }
		memcpy(placed + k, &rec[(size_t)ctx->rd_item[(size_t)at] * RD_REC_WORDS], 80);
	}
	return CHAINDP_OK;
}

// the resident result into the caller's arrays
static int deliver(chaindp_ctx *ctx, const char *who, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int64_t regs_cap,
                   int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	need[0] = ctx->rd_need[0]; need[1] = ctx->rd_need[1];
	out_off[0] = 0;
	if (n_reads == 0) { if (cigar_off) cigar_off[0] = 0; return CHAINDP_OK; }
	hipStream_t st = ctx->stream;
	const char *d_out = (const char*)ctx->rd_out.p;
	HIP_TRY(ctx, host_copy(out_off, d_out + ctx->rd_out_at[0], (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
	const bool fits = need[0] <= regs_cap && need[1] <= cigar_cap;
	if (fits) {
		const size_t R = (size_t)need[0];
		if (R) HIP_TRY(ctx, host_copy(out_regs, d_out + ctx->rd_out_at[1], R * 80, hipMemcpyDeviceToHost, st));
		if (R) HIP_TRY(ctx, host_copy(out_extra, d_out + ctx->rd_out_at[2], R * 20, hipMemcpyDeviceToHost, st));
		if (cigar_off) HIP_TRY(ctx, host_copy(cigar_off, d_out + ctx->rd_out_at[3], (R + 1) * 8, hipMemcpyDeviceToHost, st));
		if (need[1]) HIP_TRY(ctx, host_copy(cigar, ctx->rd_out_cig.p, (size_t)need[1] * 4, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (fits) return CHAINDP_OK;
	ctx->err = std::string(who) + ": " + std::to_string((long long)need[0]) + " regions and " + std::to_string((long long)need[1]) + " CIGAR words, room for " +
	           std::to_string((long long)regs_cap) + " and " + std::to_string((long long)cigar_cap);
	return CHAINDP_ERR_CAPACITY;
}

static int check_outputs(chaindp_ctx *ctx, const char *who, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int64_t regs_cap,
                         int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t *need)
{
	if (!out_off || !need) { ctx->err = std::string(who) + ": NULL out_off or need"; return CHAINDP_ERR_ARG; }
	if (regs_cap < 0 || cigar_cap < 0) { ctx->err = std::string(who) + ": negative capacity"; return CHAINDP_ERR_ARG; }
	if ((regs_cap > 0 && (!out_regs || !out_extra || !cigar_off)) || (cigar_cap > 0 && !cigar)) { ctx->err = std::string(who) + ": a capacity without its arrays"; return CHAINDP_ERR_ARG; }
	return CHAINDP_OK;
}

extern "C" int chaindp_align_reads_fetch(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra,
                                         int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (int rc = check_outputs(ctx, "chaindp_align_reads_fetch", out_off, out_regs, out_extra, regs_cap, cigar_off, cigar, cigar_cap, need)) return rc;
	if (ctx->rd_n_reads < 0 || n_reads != ctx->rd_n_reads) { ctx->err = "chaindp_align_reads_fetch: no result is resident, or not of n_reads reads"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	return deliver(ctx, "chaindp_align_reads_fetch", n_reads, out_off, out_regs, out_extra, regs_cap, cigar_off, cigar, cigar_cap, need);
}

extern "C" int chaindp_align_reads(chaindp_ctx_t *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                                   const int64_t *a_off, chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs,
                                   int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int64_t regs_cap,
                                   int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2])
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (int rc = check_outputs(ctx, WHO, out_off, out_regs, out_extra, regs_cap, cigar_off, cigar, cigar_cap, need)) return rc;
	if (int rc = align_reads_compute(ctx, opt, n_reads, seq_off, seq, a_off, a, regs_off, regs, regs_cap, cigar_cap)) return rc;
	return deliver(ctx, WHO, n_reads, out_off, out_regs, out_extra, regs_cap, cigar_off, cigar, cigar_cap, need);
}

int chaindp::align_reads_compute(chaindp_ctx *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const int64_t *a_off,
                                 chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, int64_t regs_cap, int64_t cigar_cap,
                                 const AlignResident *from, bool marks_down)
{
	const int64_t n_t = (int64_t)ctx->al_t_off.size() - 1;
	AlignPlan plan0;
	if (reads_check((const AlignOpt*)opt, n_reads, seq_off, a_off, (const uint64_t*)a, regs_off, (const int32_t*)regs, n_t < 0 ? 0 : n_t,
	                n_t < 0 ? nullptr : ctx->al_t_off.data(), regs_cap, cigar_cap, plan0, ctx->err)) return CHAINDP_ERR_ARG;
	const AlignOpt o = *(const AlignOpt*)opt;
	KswScore sc;
	if (!ksw_plan_score(o.a, o.b, o.q, o.e, o.q2, o.e2, sc)) { ctx->err = "chaindp_align_reads: scoring"; return CHAINDP_ERR_ARG; }
	ctx->rd_n_reads = -1;                                // whatever was resident is no longer
	ctx->rd_need[0] = ctx->rd_need[1] = 0;
	if (!from) ctx->ho_n_reads = -1;                     // ... nor is it a hand-off's
	ctx->rd_rounds.clear(); ctx->rd_list_off.clear(); ctx->rd_item.clear();
	if (n_reads == 0) {
		ctx->rd_n_reads = 0;
		return CHAINDP_OK;
	}
	const int64_t n_bases = seq_off[n_reads], n_a = a_off[n_reads];
	if (n_bases > 0 && !seq && !from) { ctx->err = "chaindp_align_reads: NULL sequence"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // a buffer that grows is freed: nothing of an earlier call may be in flight
	hipStream_t st = ctx->stream;
	int rc;
	// the reads, once for all rounds: up from the host, or where the caller says they are
	AlignResident res;
	if (from) {
		res.seq_off = from->seq_off; res.seq = from->seq; res.a_off = from->a_off; res.a = from->a;
	} else {
		Carve in;
		const size_t o_seq_off = in.take((size_t)(n_reads + 1) * 8), o_a_off = in.take((size_t)(n_reads + 1) * 8), o_a = in.take((size_t)n_a * 16), o_seq = in.take((size_t)n_bases);
		if ((rc = ksw_grow(ctx, ctx->rd_in, in.at + 16, "the reads", WHO))) return rc;
		char *d_in = (char*)ctx->rd_in.p;
		HIP_TRY(ctx, host_copy(d_in + o_seq_off, seq_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, host_copy(d_in + o_a_off, a_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
		if (n_a) HIP_TRY(ctx, host_copy(d_in + o_a, a, (size_t)n_a * 16, hipMemcpyHostToDevice, st));
		if (n_bases) HIP_TRY(ctx, host_copy(d_in + o_seq, seq, (size_t)n_bases, hipMemcpyHostToDevice, st));
		res.seq_off = (const int64_t*)(d_in + o_seq_off); res.seq = d_in + o_seq; res.a_off = (const int64_t*)(d_in + o_a_off); res.a = d_in + o_a;
	}
	ReadsPlan pl;
	reads_begin(pl, n_reads, regs_off);
	// a stage's CIGARs go behind the words the pool holds
	res.room = [&](int64_t total, uint32_t **out) -> int {
		const size_t used = (size_t)pl.cig_words * 4;
		if (int e = pool_grow(ctx, ctx->rd_cig, ctx->rd_cig_cur, used, used + (size_t)total * 4 + 16, "the pool of CIGAR words")) return e;
		*out = (uint32_t*)ctx->rd_cig[ctx->rd_cig_cur].p + pl.cig_words;
		return (int)CHAINDP_OK;
	};
	// a stage's records go behind the records the pool holds
	auto keep = [&](int64_t at, int64_t n) -> int {
		if (int e = pool_grow(ctx, ctx->rd_rec, ctx->rd_rec_cur, (size_t)at * RD_REC_WORDS * 4, (size_t)(at + n) * RD_REC_WORDS * 4 + 16, "the pool of records")) return e;
		HIP_TRY(ctx, launch_reads_keep(st, n, res.d_regs, res.d_extra, (int32_t*)ctx->rd_rec[ctx->rd_rec_cur].p + at * RD_REC_WORDS));
		return (int)CHAINDP_OK;
	};
	const bool prof = ctx->prof;
	double ms[4] = {0, 0, 0, 0};
	std::vector<int32_t> r_in((const int32_t*)regs, (const int32_t*)regs + regs_off[n_reads] * AL_REG_WORDS), r_next, r2, ex;
	std::vector<int64_t> coff;
	for (int round = 0; !pl.pend.empty(); ++round) {
		const size_t G = pl.pend.size();
		const int64_t at = pl.pend[0];                   // a round's records are consecutive in the pool, in the round's order
		r2.assign(G * AL_REG_WORDS, 0); ex.assign(G * 5, 0); coff.assign(G + 1, 0);
		res.d_regs = res.d_extra = nullptr;
		res.plan = round == 0 ? &plan0 : nullptr;        // round 0 runs on the caller's arguments, which reads_check has planned
		rc = align1_impl(ctx, opt, n_reads, seq_off, seq, a_off, a, pl.pend_off.data(), (chaindp_reg_t*)r_in.data(), (chaindp_reg_t*)r2.data(),
		                 (chaindp_align_extra_t*)ex.data(), coff.data(), nullptr, 0, &res);
		if (rc) { ctx->err = std::string(WHO) + ": round " + std::to_string(round) + ": " + ctx->err; return rc; }
		if (prof) for (int k = 0; k < 5; ++k) ms[0] += ctx->al_ms[k] > 0 ? ctx->al_ms[k] : 0;
		const int64_t cig_base = pl.cig_words;
		if (res.d_regs && (rc = keep(at, (int64_t)G))) return rc;
		reads_round(pl, r_in.data(), r2.data(), ex.data(), cig_base, r_next);
		r_in.swap(r_next);
	}
	// the anchors carry every round's marks now
	if (n_a && marks_down) HIP_TRY(ctx, host_copy(a, res.a, (size_t)n_a * 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	// one inversion call over the lists as the rounds leave them
	std::vector<int64_t> l_off;
	std::vector<int32_t> l_item;
	reads_lists(pl, l_off, l_item);
	const size_t GA = l_item.size();
	if (GA) {
		std::vector<int32_t> l_regs(GA * AL_REG_WORDS), made(GA, 0), r_inv(GA * AL_REG_WORDS, 0);
		for (size_t g = 0; g < GA; ++g) memcpy(&l_regs[g * AL_REG_WORDS], &pl.regs[(size_t)l_item[g] * AL_REG_WORDS], AL_REG_WORDS * 4);
		ex.assign(GA * 5, 0); coff.assign(GA + 1, 0);
		res.d_regs = res.d_extra = nullptr;
		rc = align1_inv_impl(ctx, opt, n_reads, seq_off, seq, l_off.data(), (const chaindp_reg_t*)l_regs.data(), made.data(), (chaindp_reg_t*)r_inv.data(),
		                     (chaindp_align_extra_t*)ex.data(), coff.data(), nullptr, 0, &res);
		if (rc) { ctx->err = std::string(WHO) + ": inversions: " + ctx->err; return rc; }
		if (prof && res.d_regs) for (int k = 0; k < 4; ++k) ms[1] += ctx->inv_ms[k] > 0 ? ctx->inv_ms[k] : 0;
		if (res.d_regs) {                                // else every pair returned early: nothing made, no record to keep
			const int64_t cig_base = pl.cig_words;
			if ((rc = keep(pl.n_regions, (int64_t)GA))) return rc;
			reads_inversions(pl, l_item, made.data(), r_inv.data(), ex.data(), cig_base);
		}
	}
	// the end of the loop on the device
	std::vector<uint64_t> key;
	std::vector<int64_t> cig_at;
	reads_items(pl, ctx->rd_list_off, ctx->rd_item, key, cig_at);
	const size_t L = ctx->rd_item.size(), R = (size_t)n_reads;
	Carve ls;
	const size_t o_loff = ls.take((R + 1) * 8), o_item = ls.take(L * 4), o_key = ls.take(L * 8), o_cat = ls.take(L * 8), o_placed = ls.take(L * 4), o_final = ls.take(L * 4),
	             o_skey = ls.take(L * 8), o_mark = ls.take(L * 4), o_cnt = ls.take(R * 4), o_words = ls.take(R * 8), o_woff = ls.take((R + 1) * 8), o_src = ls.take(L * 4),
	             o_tied = ls.take(R * 4), o_pairs = ls.take(L * 16), o_stack = ls.take((size_t)reads_tied_stack((int64_t)L, n_reads) * 12);
	if ((rc = ksw_grow(ctx, ctx->rd_list, ls.at + 16, "the lists", WHO))) return rc;
	Carve ot;
	const size_t o_ooff = ot.take((R + 1) * 8), o_need = ot.take(16), o_oregs = ot.take(L * 80), o_oextra = ot.take(L * 20), o_coff = ot.take((L + 1) * 8);
	if ((rc = ksw_grow(ctx, ctx->rd_out, ot.at + 16, "the result", WHO))) return rc;
	if ((rc = ksw_grow(ctx, ctx->rd_out_cig, (size_t)pl.cig_words * 4 + 16, "the result's CIGARs", WHO))) return rc;
	// (a batch without regions has made no pool yet: the kernels get addresses, not NULL)
	if ((rc = pool_grow(ctx, ctx->rd_rec, ctx->rd_rec_cur, 0, 16, "the pool of records"))) return rc;
	if ((rc = pool_grow(ctx, ctx->rd_cig, ctx->rd_cig_cur, 0, 16, "the pool of CIGAR words"))) return rc;
	char *d_ls = (char*)ctx->rd_list.p, *d_ot = (char*)ctx->rd_out.p;
	ReadsDev d = {};
	d.n_reads = n_reads; d.n_listed = (int64_t)L;
	d.seq_off = res.seq_off; d.list_off = (const int64_t*)(d_ls + o_loff); d.item = (const int32_t*)(d_ls + o_item);
	d.key = (const unsigned long long*)(d_ls + o_key); d.cig_at = (const int64_t*)(d_ls + o_cat);
	d.rec = (const int32_t*)ctx->rd_rec[ctx->rd_rec_cur].p; d.cig = (const uint32_t*)ctx->rd_cig[ctx->rd_cig_cur].p;
	d.placed = (int32_t*)(d_ls + o_placed); d.final_order = (int32_t*)(d_ls + o_final); d.sort_key = (unsigned long long*)(d_ls + o_skey);
	d.mark = (uint32_t*)(d_ls + o_mark); d.cnt = (int32_t*)(d_ls + o_cnt); d.words = (int64_t*)(d_ls + o_words); d.word_off = (int64_t*)(d_ls + o_woff);
	d.src = (int32_t*)(d_ls + o_src); d.tied = (int32_t*)(d_ls + o_tied); d.pairs = d_ls + o_pairs; d.stack = d_ls + o_stack;
	d.out_off = (int64_t*)(d_ot + o_ooff); d.need = (int64_t*)(d_ot + o_need); d.out_regs = (int32_t*)(d_ot + o_oregs); d.out_extra = (int32_t*)(d_ot + o_oextra);
	d.cigar_off = (int64_t*)(d_ot + o_coff); d.out_cig = (uint32_t*)ctx->rd_out_cig.p;
	HIP_TRY(ctx, host_copy(d_ls + o_loff, ctx->rd_list_off.data(), (R + 1) * 8, hipMemcpyHostToDevice, st));
	if (L) {
		HIP_TRY(ctx, host_copy(d_ls + o_item, ctx->rd_item.data(), L * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, host_copy(d_ls + o_key, key.data(), L * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, host_copy(d_ls + o_cat, cig_at.data(), L * 8, hipMemcpyHostToDevice, st));
	}
	StageEvents ev(ctx);
	HIP_TRY(ctx, ev.mark(-1));
	HIP_TRY(ctx, launch_reads_finish(st, o, d, ctx->rd_lds_cap));
	HIP_TRY(ctx, ev.mark(2));
	HIP_TRY(ctx, launch_reads_gather(st, d));
	HIP_TRY(ctx, ev.mark(3));
	HIP_TRY(ctx, host_copy(ctx->rd_need, d.need, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (prof) {
		double fin[4] = {0, 0, 0, 0};
		if ((rc = ev.fold(fin, 4))) return rc;
		ms[2] = fin[2]; ms[3] = fin[3];
		for (int k = 0; k < 4; ++k) ctx->rd_ms[k] = ms[k];
	}
	ctx->rd_out_at[0] = o_ooff; ctx->rd_out_at[1] = o_oregs; ctx->rd_out_at[2] = o_oextra; ctx->rd_out_at[3] = o_coff; ctx->rd_out_at[4] = o_placed;
	ctx->rd_rounds = pl.rounds;
	ctx->rd_n_rec = (int64_t)pl.rec.size();
	ctx->rd_n_reads = n_reads;
	return CHAINDP_OK;
}
