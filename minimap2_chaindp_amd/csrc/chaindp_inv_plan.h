// chaindp_inv_plan.h -- what the host decides about a batch of chaindp_align1_inv (mm_align1_inv, align.c:638-693): the argument checks,
// the early returns of every pair of neighbouring regions (the candidates that remain go to the device as a compact list), and, once
// the local scores are back, the extension problems of the candidates that pass min_dp_max.  No HIP in here, as chaindp_align_plan.h:
// a stand-alone program runs it under the sanitizers.
#ifndef CHAINDP_INV_PLAN_H
#define CHAINDP_INV_PLAN_H
#include "chaindp_align_plan.h"

namespace chaindp {

#define INV_PARENT_TMP_PRI (-2)
#define INV_BIT_SPLIT1 (1u << 8)      // split & 1: a region was split off behind this one
#define INV_BIT_SPLIT2 (1u << 9)      // split & 2: this region was split off
#define INV_BIT_REV (1u << 10)
#define INV_BIT_INV (1u << 11)
#define INV_BIT_SPLIT_INV (1u << 24)
enum { INV_NONE = 0, INV_MADE = 1, INV_LOW_SCORE = 2, INV_SKIPPED = 3, INV_NO_CIGAR = 4 };

// a pair (r1, r2) that passed the early returns.  The query stretch is ql bases of the strand opposite to r1 from qb on (qseq0[!rev1]
// in the reference's terms), the target stretch tl bases of target rid from ts = r1->re on.
struct InvCand { int32_t slot, read, rid, rev1, qb, ql, ts, tl, qlen, tlen, r2qs, r2qe; };
// a candidate whose local score reached min_dp_max: where its extension starts inside the two stretches (q_off may be -7 .. -1)
struct InvSurv { int32_t cand, q_off, t_off, pad; };

struct InvPlan {
	std::vector<InvCand> cand;           // in slot order
	std::vector<int32_t> slot_cand;      // [n_slots]: a slot's candidate, -1 where the pair returns early
	int64_t n_slots = 0, n_bases = 0, max_ql = 0;
	std::string err;
};

// the 16-bit state of k_inv_ll: H and E of the stripe's right edge per row of the padded query
inline int64_t inv_ll_rows(int64_t ql) { return (ql + 7) / 8 * 8; }

// 0 and a filled plan, or -1 (CHAINDP_ERR_ARG) with plan.err.  regs: AL_REG_WORDS words per region; t_off: the targets' offsets.
inline int inv_plan(const AlignOpt *o, int64_t n_reads, const int64_t *seq_off, const int64_t *regs_off, const int32_t *regs, int64_t n_t,
                    const int64_t *t_off, InvPlan &pl)
{
	pl = InvPlan();
	const std::string who = "chaindp_align1_inv: ";
	if (!align_check_opt(o, n_reads, who, pl.err)) return -1;
	if (o->bw < 0 || o->bw > (1 << 26)) { pl.err = who + "bw out of range"; return -1; }
	if (n_reads == 0) return 0;
	if (!align_check_offsets(n_reads, {seq_off, regs_off}, 1, n_t > 0 && t_off, who, pl.err)) return -1;
	pl.n_bases = seq_off[n_reads]; pl.n_slots = regs_off[n_reads];
	if (pl.n_slots > 0x7fffffff) { pl.err = who + "more than 2^31 - 1 regions"; return -1; }
	if (pl.n_slots > 0 && !regs) { pl.err = who + "NULL regions"; return -1; }
	pl.slot_cand.assign((size_t)pl.n_slots, -1);
	for (int64_t r = 0; r < n_reads; ++r)
		for (int64_t g = regs_off[r] + 1; g < regs_off[r + 1]; ++g) {
			const int32_t *r1 = regs + (g - 1) * AL_REG_WORDS, *r2 = regs + g * AL_REG_WORDS;
			const uint32_t b1 = (uint32_t)r1[15], b2 = (uint32_t)r2[15];
			if (!(b2 & INV_BIT_SPLIT_INV)) continue;                                        // align.c:748
			if (!(b1 & INV_BIT_SPLIT1) || !(b2 & INV_BIT_SPLIT2)) continue;                 // :646
			if (r1[0] != r1[8] && r1[8] != INV_PARENT_TMP_PRI) continue;                    // :647
			if (r2[0] != r2[8] && r2[8] != INV_PARENT_TMP_PRI) continue;                    // :648
			if (r1[2] != r2[2] || ((b1 ^ b2) & INV_BIT_REV)) continue;                      // :649
			const int rev1 = (int)(b1 >> 10 & 1);
			const int64_t ql = rev1 ? (int64_t)r1[4] - r2[5] : (int64_t)r2[4] - r1[5], tl = (int64_t)r2[6] - r1[7];
			if (ql < o->min_chain_score || ql > o->max_gap) continue;                       // :652
			if (tl < o->min_chain_score || tl > o->max_gap) continue;                       // :653
			const int64_t rid = r1[2];
			if (rid < 0 || rid >= n_t) { pl.err = who + "the pair at region " + std::to_string(g) + " names no target"; return -1; }
			const int64_t tlen = t_off[rid + 1] - t_off[rid], qlen = seq_off[r + 1] - seq_off[r];
			if (r1[7] < 0 || r2[6] > tlen || tl < 0) { pl.err = who + "the pair at region " + std::to_string(g) + " lies outside its target"; return -1; }
			const int64_t qb = rev1 ? (int64_t)r2[5] : qlen - r2[4];                          // :658
			if (qb < INT32_MIN / 2 || qb > INT32_MAX / 2) { pl.err = who + "the pair at region " + std::to_string(g) + " lies far outside its read"; return -1; }
			pl.slot_cand[(size_t)g] = (int32_t)pl.cand.size();
			pl.cand.push_back(InvCand{(int32_t)g, (int32_t)r, (int32_t)rid, rev1, (int32_t)qb, (int32_t)ql, r1[7], (int32_t)tl, (int32_t)qlen, (int32_t)tlen,
			                          r2[4], r2[5]});
			pl.max_ql = std::max(pl.max_ql, ql);
		}
	return 0;
}

// From the local scores (score, qe, te per candidate, of the reversed stretches): for every candidate at or above min_dp_max (the device
// has marked the others INV_LOW_SCORE) the survivor record and the DP's problem, q_beg / t_beg as running offsets into the base buffer
// (align.c:667-669).
inline void inv_problems(const AlignOpt &o, const InvPlan &pl, const std::vector<int32_t> &ll, std::vector<InvSurv> &surv,
                         std::vector<KswProb> &prob, int64_t &n_bases)
{
	surv.clear(); prob.clear(); n_bases = 0;
	for (size_t c = 0; c < pl.cand.size(); ++c) {
		const InvCand &C = pl.cand[c];
		const int score = ll[3 * c];
		if (C.ql <= 0 || C.tl <= 0 || score < o.min_dp_max) continue;
		const int qe = std::min<int64_t>(std::max(ll[3 * c + 1], 0), inv_ll_rows(C.ql) - 1), te = std::min(std::max(ll[3 * c + 2], 0), C.tl - 1);
		const int q_off = C.ql - (qe + 1), t_off = C.tl - (te + 1);
		KswProb p = {n_bases, 0, 0, C.ql - q_off, C.tl - t_off, (int)(o.bw * 1.5), o.zdrop, -1, 0x40};
		p.w = std::min(p.w, std::max(p.qlen, p.tlen));
		p.t_beg = n_bases + p.qlen;
		n_bases += (int64_t)p.qlen + p.tlen;
		surv.push_back(InvSurv{(int32_t)c, q_off, t_off, 0});
		prob.push_back(p);
	}
}

} // namespace chaindp
#endif
