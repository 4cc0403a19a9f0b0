// The host planning of chaindp_align1 on its own: every refusal, the empty calls, and seeded batches whose slots, compact problem list
// and DP plan are checked for what the kernels index.  The arrays are heap blocks of exactly the stated lengths, so that a read past
// an end is a sanitizer report.
#include <assert.h>
#include <stdio.h>
#include <memory>
#include <random>
#include "../../minimap2_chaindp_amd/csrc/chaindp_align_plan.h"

using namespace chaindp;

template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T> &v)
{
	std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
	for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
	return p;
}

struct Batch {
	AlignOpt o{2, 4, 4, 2, 24, 1, 500, 400, 200, -1, 3, 40, 80, 200, 5000, 0, 15, 0};
	std::vector<int64_t> seq_off{0}, a_off{0}, regs_off{0}, t_off{0};
	std::vector<uint64_t> a;          // x, y pairs
	std::vector<int32_t> regs;        // AL_REG_WORDS per region
	void target(int len) { t_off.push_back(t_off.back() + len); }
	void read(int qlen) { seq_off.push_back(seq_off.back() + qlen); a_off.push_back((int64_t)a.size() / 2); regs_off.push_back((int64_t)regs.size() / AL_REG_WORDS); }
	void anchor(int rev, int rid, uint32_t x, uint32_t y, int span = 15) { a.push_back((uint64_t)rev << 63 | (uint64_t)rid << 32 | x); a.push_back((uint64_t)span << 32 | y); a_off.back() = (int64_t)a.size() / 2; }
	void region(int as, int cnt) { std::vector<int32_t> r(AL_REG_WORDS, 0); r[1] = cnt; r[10] = as; regs.insert(regs.end(), r.begin(), r.end()); regs_off.back() = (int64_t)regs.size() / AL_REG_WORDS; }
	int plan(AlignPlan &pl) const
	{
		auto so = exact(seq_off), ao = exact(a_off), ro = exact(regs_off), to = exact(t_off);
		auto av = exact(a);
		auto rv = exact(regs);
		return align_plan(&o, (int64_t)seq_off.size() - 1, so.get(), ao.get(), a.empty() ? nullptr : av.get(), ro.get(), regs.empty() ? nullptr : rv.get(),
		                  (int64_t)t_off.size() - 1, to.get(), pl);
	}
};

static Batch simple()
{
	Batch b;
	b.target(1000); b.target(500);
	b.read(300);
	for (int i = 0; i < 6; ++i) b.anchor(0, 0, 100 + 40 * i, 20 + 40 * i);
	b.region(0, 3); b.region(3, 3);
	b.read(200);
	for (int i = 0; i < 4; ++i) b.anchor(1, 1, 50 + 30 * i, 30 + 30 * i);
	b.region(0, 4); b.region(0, 0);
	return b;
}

int main()
{
	AlignPlan pl;
	int refused = 0, planned = 0;
	{ Batch b; assert(b.plan(pl) == 0 && pl.n_regs == 0 && pl.n_slots == 0 && pl.slot_off.size() == 1); }            // no reads
	{ Batch b; b.target(10); b.read(50); b.read(0); assert(b.plan(pl) == 0 && pl.n_regs == 0 && pl.n_slots == 0); } // reads without regions
	Batch base = simple();
	assert(base.plan(pl) == 0 && pl.n_regs == 4 && pl.n_slots == 4 + 4 + 5 + 0 && pl.reg_read[2] == 1 && pl.slot_off[3] == pl.slot_off[4]);
	auto refuse = [&](Batch b) { assert(b.plan(pl) == -1 && !pl.err.empty()); ++refused; };
	{ Batch b = base; b.o.flag = AL_F_SR; refuse(b); }
	{ Batch b = base; b.o.flag = AL_F_SPLICE | 0x4; refuse(b); }
	{ Batch b = base; b.o.q2 = b.o.q; b.o.e2 = b.o.e; refuse(b); }
	{ Batch b = base; b.o.a = 128; refuse(b); }
	{ Batch b = base; b.o.e2 = -1; refuse(b); }
	{ Batch b = base; b.o.max_gap = AL_MAX_GAP + 1; refuse(b); }
	{ Batch b = base; b.a[2 * 1] ^= 1ull << 63; refuse(b); }                       // another strand inside a region
	{ Batch b = base; b.a[2 * 4] += 1ull << 32; refuse(b); }                       // another rid inside a region
	{ Batch b = base; b.a[2 * 7] += 5ull << 32; refuse(b); }                       // a rid that is no target (the whole region carries it: read 1's first)
	{ Batch b = base; for (int i = 6; i < 10; ++i) b.a[2 * i] += 1ull << 32; refuse(b); }   // ... all four anchors: no such target
	{ Batch b = base; b.a[2 * 5] = (b.a[2 * 5] & ~0xffffffffull) | 1000; refuse(b); }   // x at the target's length
	{ Batch b = base; b.a[2 * 2 + 1] = (b.a[2 * 2 + 1] & ~0xffffffffull) | 300; refuse(b); }   // y at the read's length
	{ Batch b = base; b.regs[1] = 7; refuse(b); }                                  // a region past its read's anchors
	{ Batch b = base; b.regs[10] = -1; refuse(b); }
	{ Batch b = base; b.regs[AL_REG_WORDS * 2 + 1] = -2; refuse(b); }
	{ Batch b = base; b.seq_off[1] = 500; b.seq_off[2] = 400; refuse(b); }
	{ Batch b = base; b.t_off.resize(1); refuse(b); }                              // no targets
	assert(align_plan(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pl) == -1); ++refused;
	{ Batch b = base; b.o.flag = 0x100000; assert(b.plan(pl) == 0); }              // MM_F_FOR_ONLY is allowed
	// the checks shared with chaindp_align1_inv (align_check_opt, align_check_offsets): every refusal's text, under this call's name
	auto says = [&](const Batch &b, const char *text) { assert(b.plan(pl) == -1 && pl.err == text); ++refused; };
	assert(pl.err.empty() && align_plan(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pl) == -1 && pl.err == "chaindp_align1: NULL options");
	for (int64_t n : {(int64_t)-1, (int64_t)1 << 31}) {
		assert(align_plan(&base.o, n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pl) == -1 && pl.err == "chaindp_align1: read count outside 0..2^31 - 1");
		++refused;
	}
	{ Batch b = base; b.o.flag = AL_F_SR; says(b, "chaindp_align1: MM_F_SR and MM_F_SPLICE are not built"); }
	{ Batch b = base; b.o.flag = AL_F_SPLICE; b.o.a = -1; says(b, "chaindp_align1: MM_F_SR and MM_F_SPLICE are not built"); }   // the flag before the scoring
	for (int k = 0; k < 6; ++k) for (int v : {-1, 128}) { Batch b = base; (&b.o.a)[k] = v; says(b, "chaindp_align1: a, b, q, e, q2, e2 must lie in 0..127"); }
	{ Batch b = base; b.o.q2 = b.o.q; b.o.e2 = b.o.e; b.o.max_gap = -1; says(b, "chaindp_align1: q == q2 and e == e2 (ksw_extz2_sse) is not built"); }
	for (int v : {-1, AL_MAX_GAP + 1}) { Batch b = base; b.o.max_gap = v; b.o.bw = -1; says(b, "chaindp_align1: max_gap outside 0..20000"); }
	{ Batch b = base; b.o.max_gap = AL_MAX_GAP; assert(b.plan(pl) == 0); }
	// ... what only this call checks of its options comes behind them, and before the offsets
	for (int f = 0; f < 6; ++f) {
		Batch b = base; b.t_off.resize(1);
		(f == 0 ? b.o.bw : f == 1 ? b.o.k : f == 2 ? b.o.min_cnt : f == 3 ? b.o.min_ksw_len : f == 4 ? b.o.bw : b.o.k) = f == 4 ? (1 << 26) + 1 : f == 5 ? 256 : -1;
		says(b, "chaindp_align1: bw, k, min_cnt or min_ksw_len out of range");
	}
	{
		const int64_t zero[3] = {0, 0, 0}, one[3] = {1, 1, 1}, fall[3] = {0, 5, 4}, big[3] = {0, 0x7fffffff, 0x7fffffff}, ok[3] = {0, 0x7ffffffe, 0x7ffffffe},
		              late[3] = {0, 0, 0x7fffffff};
		auto direct = [&](const int64_t *so, const int64_t *ao, const int64_t *ro, int64_t n_t, const int64_t *to, const char *text) {
			assert(align_plan(&base.o, 2, so, ao, nullptr, ro, nullptr, n_t, to, pl) == -1 && pl.err == text); ++refused;
		};
		direct(nullptr, zero, zero, 0, zero, "chaindp_align1: NULL offsets");
		direct(zero, nullptr, zero, 0, zero, "chaindp_align1: NULL offsets");
		direct(zero, zero, nullptr, -1, nullptr, "chaindp_align1: NULL offsets");      // ... before the targets are looked at
		direct(one, zero, zero, -1, zero, "chaindp_align1: no targets");              // ... and those before the offsets' values
		direct(zero, zero, zero, 1, nullptr, "chaindp_align1: no targets");
		direct(one, zero, zero, 0, nullptr, "chaindp_align1: offsets must start at 0");     // this call's rule: no target at all is none missing
		direct(zero, one, zero, 1, zero, "chaindp_align1: offsets must start at 0");
		direct(zero, zero, one, 1, zero, "chaindp_align1: offsets must start at 0");
		direct(fall, zero, zero, 1, zero, "chaindp_align1: falling offsets at read 1");
		direct(zero, fall, zero, 1, zero, "chaindp_align1: falling offsets at read 1");
		direct(late, zero, fall, 1, zero, "chaindp_align1: falling offsets at read 1");     // a read's fall before its length
		direct(big, zero, fall, 1, zero, "chaindp_align1: read 0 is too long");            // ... read by read
		direct(big, zero, zero, 1, zero, "chaindp_align1: read 0 is too long");
		direct(zero, big, zero, 1, zero, "chaindp_align1: read 0 is too long");
		direct(fall, big, zero, 1, zero, "chaindp_align1: read 0 is too long");
		direct(zero, zero, big, 1, zero, "chaindp_align1: NULL anchors or regions");   // regions are not counted per read: 2^31 - 1 of them pass the offsets
		direct(ok, ok, zero, 1, zero, "chaindp_align1: NULL anchors or regions");      // one below the limit passes them too
	}
	// seeded batches: slots, then the compact list and the DP plan from records a planning kernel could have left
	std::mt19937 rng(11);
	for (int t = 0; t < 30; ++t) {
		Batch b;
		const int n_t = 1 + rng() % 3;
		std::vector<int> tl;
		for (int i = 0; i < n_t; ++i) { tl.push_back(200 + rng() % 3000); b.target(tl.back()); }
		const int n_reads = rng() % 6;
		for (int r = 0; r < n_reads; ++r) {
			const int qlen = 100 + rng() % 1500, rid = rng() % n_t, rev = rng() % 2, n_a = rng() % 40;
			b.read(qlen);
			for (int i = 0; i < n_a; ++i) b.anchor(rev, rid, rng() % tl[rid], rng() % qlen);
			int as = 0;
			while (as < n_a && rng() % 4) { const int cnt = rng() % (n_a - as + 1); b.region(as, cnt); as += cnt; }
		}
		assert(b.plan(pl) == 0);
		assert((int64_t)pl.slot_off.size() == pl.n_regs + 1 && (int64_t)pl.reg_read.size() == pl.n_regs);
		std::vector<AlignReg> reg((size_t)pl.n_regs);
		std::vector<KswProb> slot((size_t)pl.n_slots);
		for (int64_t g = 0; g < pl.n_regs; ++g) {
			const int cnt = b.regs[(size_t)g * AL_REG_WORDS + 1];
			assert(pl.slot_off[(size_t)g + 1] - pl.slot_off[(size_t)g] == (cnt ? cnt + 1 : 0));
			reg[(size_t)g] = AlignReg{};
			reg[(size_t)g].n_prob = cnt ? (int)(rng() % (cnt + 3)) - 1 : 0;        // also below 0 and above the room: clamped
			for (int64_t s = pl.slot_off[(size_t)g]; s < pl.slot_off[(size_t)g + 1]; ++s)
				slot[(size_t)s] = KswProb{0, 0, 0, (int32_t)(rng() % 400) - 5, (int32_t)(rng() % 400) - 5, (int32_t)(rng() % 100), 400, -1, (int32_t)(rng() % 2 ? 0x08 : 0x40)};
		}
		KswPlan kp;
		std::vector<int32_t> src;
		std::vector<int64_t> first;
		int64_t n_bases = 0;
		align_compact(pl, reg, slot, kp.prob, src, first, n_bases);
		assert(first.size() == (size_t)pl.n_regs + 1 && first.back() == (int64_t)kp.prob.size() && src.size() == kp.prob.size());
		int64_t at = 0;
		for (size_t c = 0; c < kp.prob.size(); ++c) {
			const KswProb &p = kp.prob[c];
			assert(p.qlen >= 0 && p.tlen >= 0 && p.q_beg == at && p.t_beg == at + p.qlen && src[c] >= 0 && src[c] < pl.n_slots);
			at += p.qlen + p.tlen;
		}
		assert(at == n_bases);
		assert(ksw_plan_score(2, 4, 4, 2, 24, 1, kp.sc));
		ksw_plan_route(kp, 256);
		assert((int64_t)kp.order.size() == (int64_t)kp.prob.size() && kp.count[0] + kp.count[1] == (int64_t)kp.prob.size());
		int64_t words = 0;
		for (const KswProb &p : kp.prob) { assert(p.cig_beg == words); if (p.qlen > 0 && p.tlen > 0) words += p.qlen + p.tlen; }
		assert(words == kp.cig_words);
		++planned;
	}
	// more regions than the 65 536 workgroups a bookkeeping kernel gets: the plan and the compact list of 70 000 regions of two anchors
	// (three slots each), the records' n_prob running over -1 .. 3 with one region that fills its slots exactly and one whose record
	// claims more than its room, which is clamped to the room
	const int big = 70000;
	{
		Batch b;
		b.target(5000);
		for (int r = 0; r < big; ++r) {
			b.read(50);
			b.anchor(r & 1, 0, 100 + r % 4000, 14); b.anchor(r & 1, 0, 125 + r % 4000, 39);
			b.region(0, 2);
		}
		assert(b.plan(pl) == 0 && pl.n_regs == big && pl.n_slots == 3 * (int64_t)big && pl.n_anchors == 2 * (int64_t)big && pl.n_bases == 50 * (int64_t)big);
		std::vector<AlignReg> reg((size_t)big, AlignReg{});
		std::vector<KswProb> slot((size_t)pl.n_slots);
		for (int g = 0; g < big; ++g) {
			assert(pl.slot_off[(size_t)g] == 3 * (int64_t)g && pl.reg_read[(size_t)g] == g);
			reg[(size_t)g].n_prob = g % 5 - 1;
		}
		const int full = 100, over = 66000;
		reg[full].n_prob = 3; reg[over].n_prob = 3 + 4;
		for (size_t s = 0; s < slot.size(); ++s) slot[s] = KswProb{0, 0, 0, (int32_t)(s % 40), (int32_t)(s % 37), 61, 400, -1, 0x08};
		KswPlan kp;
		std::vector<int32_t> src;
		std::vector<int64_t> first;
		int64_t n_bases = 0, at = 0;
		align_compact(pl, reg, slot, kp.prob, src, first, n_bases);
		assert(first.size() == (size_t)big + 1 && first.back() == (int64_t)kp.prob.size() && src.size() == kp.prob.size());
		for (int g = 0; g < big; ++g) {
			const int want = g == full || g == over ? 3 : std::min(std::max(g % 5 - 1, 0), 3);
			assert(first[(size_t)g + 1] - first[(size_t)g] == want);
			for (int64_t c = first[(size_t)g]; c < first[(size_t)g + 1]; ++c) assert(src[(size_t)c] == 3 * g + (int)(c - first[(size_t)g]));
		}
		for (size_t c = 0; c < kp.prob.size(); ++c) {
			const KswProb &p = kp.prob[c];
			assert(p.q_beg == at && p.t_beg == at + p.qlen && p.qlen == src[c] % 40 && p.tlen == src[c] % 37);
			at += p.qlen + p.tlen;
		}
		assert(at == n_bases);
		assert(ksw_plan_score(2, 4, 4, 2, 24, 1, kp.sc));
		ksw_plan_route(kp, 256);
		assert(kp.order.size() == kp.prob.size() && kp.count[0] == (int64_t)kp.prob.size() && kp.count[1] == 0 && kp.grid[0] <= 256 * 32);
	}
	printf("align plan ok: %d batches planned, %d calls refused; %d regions compacted, full and overfull slots clamped\n", planned, refused, big);
	return 0;
}
