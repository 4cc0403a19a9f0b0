// The host planning of chaindp_align_reads on its own: every refusal, the empty calls, and seeded batches taken through several rounds
// with made-up stage results, whose pending lists, place keys, lists and items are checked against a loop written the plain way
// (a list per read, insertion behind the parent).  The arrays are heap blocks of exactly the stated lengths, so that a read past an
// end is a sanitizer report.
#include <assert.h>
#include <stdio.h>
#include <memory>
#include <random>
#include "../../minimap2_chaindp_amd/csrc/chaindp_reads_plan.h"

using namespace chaindp;

template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T> &v)
{
	std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
	for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
	return p;
}

struct Batch {
	AlignOpt o{2, 4, 4, 2, 24, 1, 500, 400, 200, -1, 3, 40, 80, 200, 200, 0, 15, 0};
	std::vector<int64_t> seq_off{0}, a_off{0}, regs_off{0}, t_off{0};
	std::vector<uint64_t> a;          // x, y pairs
	std::vector<int32_t> regs;        // AL_REG_WORDS per region
	int64_t regs_cap = 0, cigar_cap = 0;
	void target(int len) { t_off.push_back(t_off.back() + len); }
	void read(int qlen) { seq_off.push_back(seq_off.back() + qlen); a_off.push_back((int64_t)a.size() / 2); regs_off.push_back((int64_t)regs.size() / AL_REG_WORDS); }
	// a region of cnt anchors on target rid behind the read's anchors so far
	void region(int cnt, int rid = 0)
	{
		const int64_t n_a = (int64_t)a.size() / 2 - a_off[a_off.size() - 2];
		std::vector<int32_t> r(AL_REG_WORDS, 0);
		r[1] = cnt; r[2] = rid; r[10] = (int32_t)n_a;
		for (int i = 0; i < cnt; ++i) { a.push_back((uint64_t)rid << 32 | (uint64_t)(20 + 10 * (n_a + i))); a.push_back(15ull << 32 | (uint64_t)(15 + 10 * (n_a + i))); }
		regs.insert(regs.end(), r.begin(), r.end());
		a_off.back() = (int64_t)a.size() / 2; regs_off.back() = (int64_t)regs.size() / AL_REG_WORDS;
	}
	int check(std::string &err, bool null_a = false, bool null_t = false) const
	{
		auto so = exact(seq_off), ao = exact(a_off), ro = exact(regs_off), to = exact(t_off);
		auto av = exact(a);
		auto rv = exact(regs);
		AlignPlan ap;
		return reads_check(&o, (int64_t)seq_off.size() - 1, so.get(), ao.get(), a.empty() || null_a ? nullptr : av.get(), ro.get(), regs.empty() ? nullptr : rv.get(),
		                   (int64_t)t_off.size() - 1, null_t ? nullptr : to.get(), regs_cap, cigar_cap, ap, err);
	}
};

// The loop the plain way: a list of (pool index) per read; a split-off region goes behind its parent, an inversion behind its slot's region.
struct Plain {
	std::vector<std::vector<int32_t>> lists;
	void insert_behind(int read, int32_t parent, int32_t child)
	{
		std::vector<int32_t> &l = lists[(size_t)read];
		for (size_t i = 0; i < l.size(); ++i) if (l[i] == parent) { l.insert(l.begin() + (long)i + 1, child); return; }
		assert(!"the parent stands in its read's list");
	}
};

// One call's planning over reads with n_regs[r] regions each; split(round, k) says whether the k-th region of a round splits.
static void loop(const std::vector<int> &n_regs, std::mt19937 &rng, int max_rounds, int &n_rounds_seen)
{
	const int64_t R = (int64_t)n_regs.size();
	std::vector<int64_t> regs_off(1, 0);
	for (int n : n_regs) regs_off.push_back(regs_off.back() + n);
	auto ro = exact(regs_off);
	ReadsPlan pl;
	reads_begin(pl, R, ro.get());
	assert((int64_t)pl.pend.size() == regs_off.back() && (int64_t)pl.pend_off.size() == R + 1 && pl.pend_off[(size_t)R] == regs_off.back());
	Plain plain;
	plain.lists.resize((size_t)R);
	for (size_t i = 0; i < pl.rec.size(); ++i) plain.lists[(size_t)pl.rec[i].read].push_back((int32_t)i);
	std::vector<int32_t> next;
	int64_t cig = 0;
	int round = 0;
	while (!pl.pend.empty()) {
		const size_t G = pl.pend.size();
		for (size_t k = 0; k < G; ++k) assert(pl.pend[k] == pl.pend[0] + (int32_t)k);           // a round's records are consecutive in the pool
		std::vector<int32_t> regs(G * AL_REG_WORDS, 0), regs2(G * AL_REG_WORDS, 0), extra(G * 5, 0), parents;
		for (size_t k = 0; k < G; ++k) {
			regs[k * AL_REG_WORDS] = 1000 * round + (int32_t)k;                                  // a mark to find the record by
			extra[k * 5 + 4] = (int32_t)(rng() % 7);
			if (round + 1 < max_rounds && rng() % 3 == 0) { regs2[k * AL_REG_WORDS + 1] = 1 + (int32_t)(rng() % 5); parents.push_back(pl.pend[k]); }
		}
		auto rv = exact(regs), r2 = exact(regs2), ex = exact(extra);
		const std::vector<int32_t> pend = pl.pend;
		const int64_t n_before = (int64_t)pl.rec.size(), cig_before = cig;
		const int64_t n_next = reads_round(pl, rv.get(), r2.get(), ex.get(), cig, next);
		assert(n_next == (int64_t)parents.size() && (int64_t)pl.rec.size() == n_before + n_next && next.size() == (size_t)n_next * AL_REG_WORDS);
		assert((int64_t)pl.rounds.size() == round + 1 && pl.rounds.back() == (int64_t)G && pl.n_regions == (int64_t)pl.rec.size());
		int64_t at = cig_before;
		for (size_t k = 0; k < G; ++k) {
			const size_t i = (size_t)pend[k];
			assert(pl.regs[i * AL_REG_WORDS] == 1000 * round + (int32_t)k && pl.cig_at[i] == at && pl.n_cig[i] == extra[k * 5 + 4] && pl.listed[i] == 1);
			at += extra[k * 5 + 4];
		}
		cig = pl.cig_words;
		assert(cig == at);
		for (size_t j = 0; j < parents.size(); ++j) {
			const ReadsRec &p = pl.rec[(size_t)parents[j]], &c = pl.rec[(size_t)n_before + j];
			assert(pl.pend[j] == (int32_t)(n_before + (int64_t)j) && c.read == p.read && c.origin == p.origin && c.born == p.born + 1 && c.is_inv == 0);
			assert(next[j * AL_REG_WORDS + 1] == regs2[(size_t)(parents[j] - pend[0]) * AL_REG_WORDS + 1]);
			plain.insert_behind(p.read, parents[j], (int32_t)(n_before + (int64_t)j));
		}
		for (int64_t r = 0; r < R; ++r)
			for (int64_t k = pl.pend_off[(size_t)r]; k < pl.pend_off[(size_t)r + 1]; ++k) assert(pl.rec[(size_t)pl.pend[(size_t)k]].read == r);
		++round;
	}
	n_rounds_seen = std::max(n_rounds_seen, round);
	// the lists the inversion call sees are the plain loop's
	std::vector<int64_t> off;
	std::vector<int32_t> item;
	reads_lists(pl, off, item);
	for (int64_t r = 0; r < R; ++r) {
		assert(off[(size_t)r + 1] - off[(size_t)r] == (int64_t)plain.lists[(size_t)r].size());
		for (size_t i = 0; i < plain.lists[(size_t)r].size(); ++i) assert(item[(size_t)off[(size_t)r] + i] == plain.lists[(size_t)r][i]);
	}
	// inversions: some slots made, behind their regions
	const size_t GA = item.size();
	std::vector<int32_t> made(GA, 0), r_inv(GA * AL_REG_WORDS, 0), extra(GA * 5, 0);
	for (size_t g = 0; g < GA; ++g) { made[g] = (int32_t)(rng() % 5); extra[g * 5 + 4] = made[g] == INV_MADE ? 3 : 0; }
	auto mv = exact(made), iv = exact(r_inv), ev = exact(extra);
	const int64_t n_regions = pl.n_regions;
	reads_inversions(pl, item, mv.get(), iv.get(), ev.get(), cig);
	assert(pl.rec.size() == (size_t)n_regions + GA && pl.n_regions == n_regions);
	for (size_t g = 0; g < GA; ++g)
		if (made[g] == INV_MADE) plain.insert_behind(pl.rec[(size_t)item[g]].read, item[g], (int32_t)(n_regions + (int64_t)g));
	std::vector<int64_t> l_off, cig_at;
	std::vector<int32_t> l_item;
	std::vector<uint64_t> key;
	reads_items(pl, l_off, l_item, key, cig_at);
	for (int64_t r = 0; r < R; ++r) {
		const int64_t b = l_off[(size_t)r], n = l_off[(size_t)r + 1] - b;
		assert(n == (int64_t)plain.lists[(size_t)r].size());
		// ranked by key, the items are the plain loop's list; the keys of a read are distinct
		std::vector<int64_t> order((size_t)n);
		for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
		std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key[(size_t)(b + x)] < key[(size_t)(b + y)]; });
		for (int64_t i = 0; i < n; ++i) {
			assert(l_item[(size_t)(b + order[(size_t)i])] == plain.lists[(size_t)r][(size_t)i]);
			assert(i == 0 || key[(size_t)(b + order[(size_t)i - 1])] < key[(size_t)(b + order[(size_t)i])]);
			assert(cig_at[(size_t)(b + i)] == pl.cig_at[(size_t)l_item[(size_t)(b + i)]]);
		}
	}
}

int main()
{
	std::string err;
	int refused = 0, planned = 0;
	// keys: origin first, then the round, an inversion right behind its region
	assert(reads_place_key(0, 0, 0) < reads_place_key(0, 0, 1) && reads_place_key(0, 0, 1) < reads_place_key(0, 1, 0) && reads_place_key(0, 9, 1) < reads_place_key(1, 0, 0));
	assert(reads_place_key(0xffffffffu, 0x7fffffffu, 1) == ~0ull);
	{ Batch b; assert(b.check(err) == 0); ++planned; }                                                          // no reads
	Batch base;
	base.target(1000); base.target(500);
	base.read(300); base.region(4); base.region(3, 1);
	base.read(50);
	base.read(200); base.region(5);
	assert(base.check(err) == 0); ++planned;
	auto refuse = [&](void (*edit)(Batch &b), bool null_a = false, bool null_t = false) {
		Batch b = base;
		edit(b);
		err.clear();
		assert(b.check(err, null_a, null_t) == -1 && err.rfind("chaindp_align_reads: ", 0) == 0);
		++refused;
	};
	refuse([](Batch &b) { b.o.flag = AL_F_SR; });
	refuse([](Batch &b) { b.o.flag = AL_F_SPLICE; });
	refuse([](Batch &b) { b.o.q2 = b.o.q; b.o.e2 = b.o.e; });
	refuse([](Batch &b) { b.o.a = 128; });
	refuse([](Batch &b) { b.o.max_gap = AL_MAX_GAP + 1; });
	refuse([](Batch &b) { b.o.bw = -1; });
	refuse([](Batch &b) { b.o.min_cnt = -1; });
	refuse([](Batch &b) { b.t_off.resize(1); });                                   // no targets
	refuse([](Batch &) {}, false, true);                                            // targets without offsets
	refuse([](Batch &) {}, true);                                                   // NULL anchors
	refuse([](Batch &b) { b.seq_off[0] = 1; });
	refuse([](Batch &b) { b.a_off[2] = b.a_off[1] - 1; });
	refuse([](Batch &b) { b.regs[1] = 100; });                                     // a region past its read's anchors
	refuse([](Batch &b) { b.regs[10] = -1; });
	refuse([](Batch &b) { b.a[2 * 1] |= 1ull << 63; });                            // two strands in one region
	refuse([](Batch &b) { b.a[0] = 7ull << 32 | 20; });                            // an anchor of no target
	refuse([](Batch &b) { b.a[0] = 5000; });                                       // ... outside its target
	refuse([](Batch &b) { b.a[1] = 15ull << 32 | 5000; });                         // ... outside its read
	refuse([](Batch &b) { b.regs_cap = -1; });
	refuse([](Batch &b) { b.cigar_cap = -1; });
	// the inversion stage's own refusal: a pair that passes the early returns on a target that is none
	refuse([](Batch &b) {
		int32_t *r1 = b.regs.data(), *r2 = r1 + AL_REG_WORDS;
		r1[15] = (int32_t)INV_BIT_SPLIT1; r2[15] = (int32_t)(INV_BIT_SPLIT2 | INV_BIT_SPLIT_INV);
		r1[2] = r2[2] = 9; r1[5] = 100; r2[4] = 200; r1[7] = 100; r2[6] = 200;
		r1[1] = r2[1] = 0;                                                            // (no anchors: the first stage has nothing to say)
	});
	// loops: no reads, reads without regions first and last, one round, several
	std::mt19937 rng(7);
	int rounds = 0;
	loop({}, rng, 3, rounds); ++planned;
	loop({0, 0}, rng, 3, rounds); ++planned;
	loop({0, 3, 0}, rng, 1, rounds); ++planned;
	assert(rounds == 1);
	for (int t = 0; t < 40; ++t) {
		std::vector<int> n((size_t)(1 + rng() % 6));
		for (int &x : n) x = (int)(rng() % 70);
		loop(n, rng, 2 + (int)(rng() % 5), rounds); ++planned;
	}
	assert(rounds >= 4);
	printf("reads plan ok: %d batches planned, %d calls refused, up to %d rounds\n", planned, refused, rounds);
	return 0;
}
