// chaindp_reads_plan.h -- what the host decides about a chaindp_align_reads call (mm_align_skeleton, align.c:705-761): the argument
// checks, which regions each round of chaindp_align1 aligns (round 0 every region, round k what round k - 1 split off), the lists the
// one chaindp_align1_inv call sees, and where every record the rounds and that call made stands in its read's list.  No HIP in here,
// as chaindp_inv_plan.h: a stand-alone program runs it under the sanitizers.  The place key is the one definition host and kernel share.
#ifndef CHAINDP_READS_PLAN_H
#define CHAINDP_READS_PLAN_H
#include <algorithm>
#include "chaindp_inv_plan.h"

#ifdef __HIPCC__
#define RD_HD __host__ __device__
#else
#define RD_HD
#endif

namespace chaindp {

#define RD_LDS_CAP 1024               // records of a read k_reads_finish keeps in LDS (24 bytes each); longer lists take the global route
#define RD_BIT_INV (1u << 11)
#define RD_BIT_SEG_SPLIT (1u << 15)
#define RD_REC_WORDS 25               // a pool record: the region's AL_REG_WORDS words, then the five of chaindp_align_extra_t

// Where a record stands in its read's list as the loop leaves it for mm_filter_regs.  A region is aligned once, so it splits off at most
// one region, which mm_insert_reg puts right behind it: the regions that descend from input region `origin` stand together, in the order
// of the rounds that made them.  An inversion record stands right behind its right region.  Keys of one read are distinct.
RD_HD inline uint64_t reads_place_key(uint32_t origin, uint32_t born, uint32_t is_inv)
{
	return (uint64_t)origin << 32 | (uint64_t)born << 1 | (uint64_t)(is_inv & 1u);
}

// Pending ranges of radix_sort_128x (chaindp_rsort.h: n / 65 + 2 for a list of n) for every read of a batch at once: read r's lie at
// list_off[r] / 65 + 2 r.
RD_HD inline int64_t reads_tied_stack(int64_t n_listed, int64_t n_reads) { return n_listed / 65 + 2 * n_reads + 2; }

// a record of the pool, in pool order: round 0's regions, round 1's, ..., then one per slot of the inversion call
struct ReadsRec { int32_t read, origin, born, is_inv; };

struct ReadsPlan {
	int64_t n_reads = 0;
	std::vector<ReadsRec> rec;           // the pool's records
	std::vector<int32_t> regs;           // their region words as the stages returned them (AL_REG_WORDS each; the inversion slots': zero unless made)
	std::vector<int32_t> n_cig;          // their CIGAR words ...
	std::vector<int64_t> cig_at;         // ... and where those start in the pool of CIGAR words
	std::vector<int32_t> listed;         // 1: the record stands in its read's list (every region; an inversion slot only with made == 1)
	std::vector<int32_t> pend;           // the round's regions: pool indices, read by read
	std::vector<int64_t> pend_off;       // [n_reads + 1]
	std::vector<int64_t> rounds;         // regions of every round made so far
	int64_t n_regions = 0;               // pool records that are regions (the inversion slots lie behind them)
	int64_t cig_words = 0;               // CIGAR words in the pool
	std::string err;
};

// The arguments, as chaindp_align1 and chaindp_align1_inv would look at them, and the call's own.  0 with ap = round 0's plan (round 0
// is not planned a second time), or -1 with err.
inline int reads_check(const AlignOpt *o, int64_t n_reads, const int64_t *seq_off, const int64_t *a_off, const uint64_t *a, const int64_t *regs_off,
                       const int32_t *regs, int64_t n_t, const int64_t *t_off, int64_t regs_cap, int64_t cigar_cap, AlignPlan &ap, std::string &err)
{
	const std::string who = "chaindp_align_reads: ";
	if (align_plan(o, n_reads, seq_off, a_off, a, regs_off, regs, n_t, t_off, ap)) { err = who + ap.err; return -1; }
	InvPlan ip;
	if (inv_plan(o, n_reads, seq_off, regs_off, regs, n_t, t_off, ip)) { err = who + ip.err; return -1; }
	if (regs_cap < 0 || cigar_cap < 0) { err = who + "negative capacity"; return -1; }
	return 0;
}

// Round 0: every region of every read, origin = its place among its read's regions.
inline void reads_begin(ReadsPlan &pl, int64_t n_reads, const int64_t *regs_off)
{
	pl = ReadsPlan();
	pl.n_reads = n_reads;
	pl.pend_off.assign((size_t)n_reads + 1, 0);
	for (int64_t r = 0; r < n_reads; ++r) {
		for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g) {
			pl.pend.push_back((int32_t)pl.rec.size());
			pl.rec.push_back(ReadsRec{(int32_t)r, (int32_t)(g - regs_off[r]), 0, 0});
		}
		pl.pend_off[(size_t)r + 1] = (int64_t)pl.pend.size();
	}
}

// A round came back: regs, regs2 and extra of its pend.size() regions (words), its CIGARs at cig_base of the pool.  The records are
// filled in; pend becomes what the round split off (regs2.cnt > 0), next_regs those regions for the next round.  Returns their count.
inline int64_t reads_round(ReadsPlan &pl, const int32_t *regs, const int32_t *regs2, const int32_t *extra, int64_t cig_base, std::vector<int32_t> &next_regs)
{
	const size_t G = pl.pend.size();
	pl.rounds.push_back((int64_t)G);
	pl.regs.resize(pl.rec.size() * AL_REG_WORDS, 0);
	pl.n_cig.resize(pl.rec.size(), 0); pl.cig_at.resize(pl.rec.size(), 0); pl.listed.resize(pl.rec.size(), 1);
	std::vector<int32_t> nxt;
	std::vector<int64_t> nxt_off((size_t)pl.n_reads + 1, 0);
	next_regs.clear();
	int64_t at = cig_base;
	for (int64_t r = 0; r < pl.n_reads; ++r) {
		for (int64_t k = pl.pend_off[(size_t)r]; k < pl.pend_off[(size_t)r + 1]; ++k) {
			const size_t i = (size_t)pl.pend[(size_t)k];
			std::copy(regs + k * AL_REG_WORDS, regs + (k + 1) * AL_REG_WORDS, pl.regs.begin() + i * AL_REG_WORDS);
			pl.n_cig[i] = std::max(extra[k * 5 + 4], 0); pl.cig_at[i] = at;
			at += pl.n_cig[i];
			if (regs2[k * AL_REG_WORDS + 1] > 0) {                                // align.c:747
				nxt.push_back((int32_t)(pl.rec.size() + nxt.size()));
				next_regs.insert(next_regs.end(), regs2 + k * AL_REG_WORDS, regs2 + (k + 1) * AL_REG_WORDS);
			}
		}
		nxt_off[(size_t)r + 1] = (int64_t)nxt.size();
	}
	pl.cig_words = at;
	// the new records, in pend order as nxt names them: read and origin of their parents, one round later
	size_t j = 0;
	for (size_t k = 0; k < G; ++k)
		if (regs2[k * AL_REG_WORDS + 1] > 0) {
			const ReadsRec p = pl.rec[(size_t)pl.pend[k]];
			pl.rec.push_back(ReadsRec{p.read, p.origin, p.born + 1, 0});
			++j;
		}
	pl.pend.swap(nxt); pl.pend_off.swap(nxt_off);
	pl.n_regions = (int64_t)pl.rec.size();
	return (int64_t)j;
}

// After the last round: every read's regions in placed order (pool indices), for the inversion call and for the slots' records.
inline void reads_lists(const ReadsPlan &pl, std::vector<int64_t> &off, std::vector<int32_t> &item)
{
	std::vector<int64_t> cnt((size_t)pl.n_reads + 1, 0);
	for (int64_t i = 0; i < pl.n_regions; ++i) ++cnt[(size_t)pl.rec[(size_t)i].read + 1];
	off.assign((size_t)pl.n_reads + 1, 0);
	for (int64_t r = 0; r < pl.n_reads; ++r) off[(size_t)r + 1] = off[(size_t)r] + cnt[(size_t)r + 1];
	item.assign((size_t)pl.n_regions, 0);
	std::vector<int64_t> at(off.begin(), off.end() - 1);
	for (int64_t i = 0; i < pl.n_regions; ++i) item[(size_t)at[(size_t)pl.rec[(size_t)i].read]++] = (int32_t)i;
	for (int64_t r = 0; r < pl.n_reads; ++r)
		std::sort(item.begin() + off[(size_t)r], item.begin() + off[(size_t)r + 1], [&](int32_t x, int32_t y) {
			const ReadsRec &a = pl.rec[(size_t)x], &b = pl.rec[(size_t)y];
			return reads_place_key((uint32_t)a.origin, (uint32_t)a.born, 0) < reads_place_key((uint32_t)b.origin, (uint32_t)b.born, 0);
		});
}

// The inversion call came back over the lists of reads_lists (slot g = item[g]): one pool record per slot behind the regions', listed
// where made == 1, standing behind its right region; its CIGAR words at cig_base of the pool.
inline void reads_inversions(ReadsPlan &pl, const std::vector<int32_t> &item, const int32_t *made, const int32_t *r_inv, const int32_t *extra, int64_t cig_base)
{
	int64_t at = cig_base;
	for (size_t g = 0; g < item.size(); ++g) {
		const ReadsRec p = pl.rec[(size_t)item[g]];
		pl.rec.push_back(ReadsRec{p.read, p.origin, p.born, 1});
		pl.regs.insert(pl.regs.end(), r_inv + g * AL_REG_WORDS, r_inv + (g + 1) * AL_REG_WORDS);
		pl.n_cig.push_back(std::max(extra[g * 5 + 4], 0)); pl.cig_at.push_back(at);
		at += pl.n_cig.back();
		pl.listed.push_back(made[g] == INV_MADE);
	}
	pl.cig_words = at;
}

// What the finish kernel takes: per read the listed records in pool order (it ranks them by key itself), their keys and CIGAR places.
inline void reads_items(const ReadsPlan &pl, std::vector<int64_t> &off, std::vector<int32_t> &item, std::vector<uint64_t> &key, std::vector<int64_t> &cig_at)
{
	off.assign((size_t)pl.n_reads + 1, 0);
	for (size_t i = 0; i < pl.rec.size(); ++i) if (pl.listed[i]) ++off[(size_t)pl.rec[i].read + 1];
	for (int64_t r = 0; r < pl.n_reads; ++r) off[(size_t)r + 1] += off[(size_t)r];
	const size_t L = (size_t)off[(size_t)pl.n_reads];
	item.assign(L, 0); key.assign(L, 0); cig_at.assign(L, 0);
	std::vector<int64_t> at(off.begin(), off.end() - 1);
	for (size_t i = 0; i < pl.rec.size(); ++i) {
		if (!pl.listed[i]) continue;
		const ReadsRec &c = pl.rec[i];
		const size_t k = (size_t)at[(size_t)c.read]++;
		item[k] = (int32_t)i; key[k] = reads_place_key((uint32_t)c.origin, (uint32_t)c.born, (uint32_t)c.is_inv); cig_at[k] = pl.cig_at[i];
	}
}

} // namespace chaindp
#endif
