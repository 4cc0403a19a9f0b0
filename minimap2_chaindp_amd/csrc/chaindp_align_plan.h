// chaindp_align_plan.h -- what the host decides about a batch of chaindp_align1 before anything touches the device (the argument checks,
// the regions' reads and problem slots) and between its kernels (the compact problem list with its offsets, the second pass), and the
// records the kernels and the host share.  No HIP in here, as chaindp_ksw_plan.h: a stand-alone program runs it under the sanitizers.
#ifndef CHAINDP_ALIGN_PLAN_H
#define CHAINDP_ALIGN_PLAN_H
#include <initializer_list>
#include "chaindp_ksw_plan.h"

namespace chaindp {

#define AL_F_SPLICE 0x80
#define AL_F_SR 0x1000
#define AL_F_NO_INV_TEST (0x80 | 0x1000 | 0x100000 | 0x200000)     // MM_F_SPLICE | MM_F_SR | MM_F_FOR_ONLY | MM_F_REV_ONLY (align.c:71)
#define AL_MAX_GAP 20000              // the inversion test keeps 8 bytes of state per target base of a stretch below max_gap in LDS
#define AL_REG_WORDS 20               // chaindp_reg_t in 32-bit words
enum { AL_LEFT = 0, AL_FILL = 1, AL_RIGHT = 2 };

struct AlignOpt { int32_t a, b, q, e, q2, e2, bw, zdrop, zdrop_inv, end_bonus, min_cnt, min_chain_score, min_dp_max, min_ksw_len, max_gap, flag, k, is_hpc; };
// per region, by k_align_plan: the anchors chosen, the ends of the first and the last anchor taken, the bounds, its problems
struct AlignReg { int32_t as1, cnt1, rid, rev, rs, qs, re, qe, rs0, qs0, re0, qe0, n_prob, qlen, tlen, pad; };
// per problem, beside its KswProb: the region, AL_LEFT / AL_FILL / AL_RIGHT, the anchor it ends at (relative to as1), where it starts
// on the target and on the read's mapped strand (the left extension: where its reversed sequences end)
struct AlignSide { int32_t reg, kind, i, rs, qs, pad; };
// per region, by k_align_stitch
struct AlignStitch { int32_t n_cigar, dp_score, has_p, rs1, re1, qs1, qe1, pad; };

struct AlignPlan {
	std::vector<int32_t> reg_read;       // the read of every region
	std::vector<int64_t> slot_off;       // [n_regs + 1]: a region's problems lie in slots slot_off[r] .. + cnt + 1
	int64_t n_regs = 0, n_slots = 0, n_anchors = 0, n_bases = 0;
	std::string err;
};

// ---- the checks chaindp_align1 and chaindp_align1_inv share; who: the call's name and ": ", ahead of every message.  false with err.  The options, up to max_gap:
inline bool align_check_opt(const AlignOpt *o, int64_t n_reads, const std::string &who, std::string &err)
{
	if (!o) { err = who + "NULL options"; return false; }
	if (n_reads < 0 || n_reads > 0x7fffffff) { err = who + "read count outside 0..2^31 - 1"; return false; }
	if (o->flag & (AL_F_SR | AL_F_SPLICE)) { err = who + "MM_F_SR and MM_F_SPLICE are not built"; return false; }
	for (int v : {o->a, o->b, o->q, o->e, o->q2, o->e2})
		if (v < 0 || v > 127) { err = who + "a, b, q, e, q2, e2 must lie in 0..127"; return false; }
	if (o->q == o->q2 && o->e == o->e2) { err = who + "q == q2 and e == e2 (ksw_extz2_sse) is not built"; return false; }
	if (o->max_gap < 0 || o->max_gap > AL_MAX_GAP) { err = who + "max_gap outside 0.." + std::to_string(AL_MAX_GAP); return false; }
	return true;
}
// The per-read offset arrays of n_reads > 0 reads: none NULL, each from 0 and not falling; a read spans less than 2^31 - 1 entries of
// each of the first n_len of them.  targets_ok: the call's own rule about the targets, looked at between the NULLs and the values.
inline bool align_check_offsets(int64_t n_reads, std::initializer_list<const int64_t*> offs, size_t n_len, bool targets_ok, const std::string &who, std::string &err)
{
	for (const int64_t *off : offs) if (!off) { err = who + "NULL offsets"; return false; }
	if (!targets_ok) { err = who + "no targets"; return false; }
	for (const int64_t *off : offs) if (off[0] != 0) { err = who + "offsets must start at 0"; return false; }
	for (int64_t r = 0; r < n_reads; ++r) {
		for (const int64_t *off : offs) if (off[r + 1] < off[r]) { err = who + "falling offsets at read " + std::to_string(r); return false; }
		size_t k = 0;
		for (const int64_t *off : offs) if (k++ < n_len && off[r + 1] - off[r] >= 0x7fffffff) { err = who + "read " + std::to_string(r) + " is too long"; return false; }
	}
	return true;
}

// 0 and a filled plan, or -1 (CHAINDP_ERR_ARG) with plan.err.  a: x, y pairs; regs: AL_REG_WORDS words per region; t_off: the targets' offsets.
inline int align_plan(const AlignOpt *o, int64_t n_reads, const int64_t *seq_off, const int64_t *a_off, const uint64_t *a, const int64_t *regs_off,
                      const int32_t *regs, int64_t n_t, const int64_t *t_off, AlignPlan &pl)
{
	pl = AlignPlan();
	const std::string who = "chaindp_align1: ";
	if (!align_check_opt(o, n_reads, who, pl.err)) return -1;
	if (o->bw < 0 || o->bw > (1 << 26) || o->k < 0 || o->k > 255 || o->min_cnt < 0 || o->min_ksw_len < 0) { pl.err = who + "bw, k, min_cnt or min_ksw_len out of range"; return -1; }
	if (n_reads == 0) { pl.slot_off.assign(1, 0); return 0; }
	if (!align_check_offsets(n_reads, {seq_off, a_off, regs_off}, 2, n_t >= 0 && (n_t == 0 || t_off), who, pl.err)) return -1;
	pl.n_bases = seq_off[n_reads]; pl.n_anchors = a_off[n_reads]; pl.n_regs = regs_off[n_reads];
	if (pl.n_regs > 0x7fffffff) { pl.err = who + "more than 2^31 - 1 regions"; return -1; }
	if ((pl.n_anchors > 0 && !a) || (pl.n_regs > 0 && !regs)) { pl.err = who + "NULL anchors or regions"; return -1; }
	pl.reg_read.resize((size_t)pl.n_regs);
	pl.slot_off.assign((size_t)pl.n_regs + 1, 0);
	for (int64_t r = 0; r < n_reads; ++r) {
		const int64_t qlen = seq_off[r + 1] - seq_off[r], n_a = a_off[r + 1] - a_off[r];
		const uint64_t *ar = a + 2 * a_off[r];
		bool used = false;
		for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g) {
			const int32_t cnt = regs[g * AL_REG_WORDS + 1], as = regs[g * AL_REG_WORDS + 10];
			pl.reg_read[(size_t)g] = (int32_t)r;
			if (cnt < 0 || as < 0 || (int64_t)as + cnt > n_a) { pl.err = who + "region " + std::to_string(g) + " reaches outside its read's anchors"; return -1; }
			pl.slot_off[(size_t)g + 1] = pl.slot_off[(size_t)g] + (cnt ? cnt + 1 : 0);
			for (int32_t i = 1; i < cnt; ++i)
				if (ar[2 * (as + i)] >> 32 != ar[2 * as] >> 32) { pl.err = who + "region " + std::to_string(g) + " has anchors of several targets or strands"; return -1; }
			used = used || cnt > 0;
		}
		if (!used) continue;
		for (int64_t i = 0; i < n_a; ++i) {
			const uint64_t x = ar[2 * i], y = ar[2 * i + 1];
			const int64_t rid = (int64_t)(x << 1 >> 33);
			if (rid >= n_t) { pl.err = who + "anchor " + std::to_string(i) + " of read " + std::to_string(r) + " names no target"; return -1; }
			if ((int64_t)(uint32_t)x >= t_off[rid + 1] - t_off[rid] || (int64_t)(uint32_t)y >= qlen) {
				pl.err = who + "anchor " + std::to_string(i) + " of read " + std::to_string(r) + " lies outside its sequence"; return -1;
			}
		}
	}
	pl.n_slots = pl.slot_off[(size_t)pl.n_regs];
	if (pl.n_slots > 0x7fffffff) { pl.err = who + "more than 2^31 - 1 problems"; return -1; }
	return 0;
}

// The compact problem list of the first pass, from the slots k_align_plan filled (slot[s] holds lengths, band, zdrop, end bonus and flag):
// the problems of a region in order, q_beg / t_beg as running offsets into the base buffer.  first[r] = a region's first problem.
inline void align_compact(const AlignPlan &pl, const std::vector<AlignReg> &reg, const std::vector<KswProb> &slot, std::vector<KswProb> &prob,
                          std::vector<int32_t> &src_slot, std::vector<int64_t> &first, int64_t &n_bases)
{
	prob.clear(); src_slot.clear(); first.assign((size_t)pl.n_regs + 1, 0); n_bases = 0;
	for (int64_t r = 0; r < pl.n_regs; ++r) {
		first[(size_t)r] = (int64_t)prob.size();
		const int64_t room = pl.slot_off[(size_t)r + 1] - pl.slot_off[(size_t)r];
		const int64_t n = std::min<int64_t>(std::max<int64_t>(reg[(size_t)r].n_prob, 0), room);
		for (int64_t k = 0; k < n; ++k) {
			KswProb p = slot[(size_t)(pl.slot_off[(size_t)r] + k)];
			p.qlen = std::max(p.qlen, 0); p.tlen = std::max(p.tlen, 0);
			p.q_beg = n_bases; p.t_beg = n_bases + p.qlen;
			n_bases += (int64_t)p.qlen + p.tlen;
			prob.push_back(p); src_slot.push_back((int32_t)(pl.slot_off[(size_t)r] + k));
		}
	}
	first[(size_t)pl.n_regs] = (int64_t)prob.size();
}

} // namespace chaindp
#endif
