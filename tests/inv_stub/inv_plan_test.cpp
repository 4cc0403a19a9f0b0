// The host planning of chaindp_align1_inv on its own: every refusal, the empty calls, every early return, and seeded batches whose
// candidate list, extension problems and DP plan are checked for what the kernels index.  The arrays are heap blocks of exactly the
// stated lengths, so that a read past an end is a sanitizer report.
#include <assert.h>
#include <stdio.h>
#include <memory>
#include <random>
#include "../../minimap2_chaindp_amd/csrc/chaindp_inv_plan.h"

using namespace chaindp;

template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T> &v)
{
	std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
	for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
	return p;
}

struct Batch {
	AlignOpt o{2, 4, 4, 2, 24, 1, 500, 400, 200, -1, 3, 40, 80, 200, 200, 0, 15, 0};
	std::vector<int64_t> seq_off{0}, regs_off{0}, t_off{0};
	std::vector<int32_t> regs;        // AL_REG_WORDS per region
	void target(int len) { t_off.push_back(t_off.back() + len); }
	void read(int qlen) { seq_off.push_back(seq_off.back() + qlen); regs_off.push_back((int64_t)regs.size() / AL_REG_WORDS); }
	int32_t *region(int qs, int qe, int rs, int re, uint32_t bits, int id, int parent, int rid = 0)
	{
		std::vector<int32_t> r(AL_REG_WORDS, 0);
		r[0] = id; r[2] = rid; r[4] = qs; r[5] = qe; r[6] = rs; r[7] = re; r[8] = parent; r[15] = (int32_t)bits;
		regs.insert(regs.end(), r.begin(), r.end());
		regs_off.back() = (int64_t)regs.size() / AL_REG_WORDS;
		return regs.data() + regs.size() - AL_REG_WORDS;
	}
	// a forward pair with a stretch of ql query and tl target bases between a 30-base and a 30-base region
	void pair(int ql, int tl, int rid = 0)
	{
		read(60 + ql);
		region(0, 30, 100, 130, INV_BIT_SPLIT1, 0, 0, rid);
		region(30 + ql, 60 + ql, 130 + tl, 160 + tl, INV_BIT_SPLIT2 | INV_BIT_SPLIT_INV, -1, INV_PARENT_TMP_PRI, rid);
	}
	int plan(InvPlan &pl) const
	{
		auto so = exact(seq_off), ro = exact(regs_off), to = exact(t_off);
		auto rv = exact(regs);
		return inv_plan(&o, (int64_t)seq_off.size() - 1, so.get(), ro.get(), regs.empty() ? nullptr : rv.get(), (int64_t)t_off.size() - 1, to.get(), pl);
	}
};

int main()
{
	InvPlan pl;
	int refused = 0, planned = 0;
	{ Batch b; assert(b.plan(pl) == 0 && pl.n_slots == 0 && pl.cand.empty()); ++planned; }                                   // no reads
	{ Batch b; b.target(10); b.read(50); b.read(0); assert(b.plan(pl) == 0 && pl.n_slots == 0 && pl.cand.empty()); ++planned; }   // reads without regions
	Batch base;
	base.target(1000); base.target(400);
	base.pair(60, 70); base.pair(40, 200); base.pair(90, 50, 1);
	assert(base.plan(pl) == 0 && pl.n_slots == 6 && pl.cand.size() == 3 && pl.max_ql == 90); ++planned;
	assert(pl.slot_cand[0] == -1 && pl.slot_cand[1] == 0 && pl.slot_cand[3] == 1 && pl.slot_cand[5] == 2);
	assert(pl.cand[0].ql == 60 && pl.cand[0].tl == 70 && pl.cand[0].ts == 130 && pl.cand[0].qb == 30 && pl.cand[2].rid == 1 && pl.cand[2].read == 2);
	// every early return drops the candidate and refuses nothing
	auto drops = [&](void (*edit)(int32_t *r1, int32_t *r2, AlignOpt &o)) {
		Batch b = base;
		edit(b.regs.data(), b.regs.data() + AL_REG_WORDS, b.o);
		assert(b.plan(pl) == 0 && pl.cand.size() == 2 && pl.slot_cand[1] == -1 && pl.slot_cand[3] == 0);
		++planned;
	};
	drops([](int32_t *r1, int32_t *, AlignOpt &) { r1[15] &= ~(int32_t)INV_BIT_SPLIT1; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[15] &= ~(int32_t)INV_BIT_SPLIT2; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[15] &= ~(int32_t)INV_BIT_SPLIT_INV; });
	drops([](int32_t *r1, int32_t *, AlignOpt &) { r1[8] = 7; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[8] = -1; r2[0] = 3; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[2] = 1; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[15] |= (int32_t)INV_BIT_REV; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[4] = 30 + 39; });            // ql below min_chain_score
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[4] = 30 + 201; });           // ql above max_gap
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[6] = 130 + 39; });
	drops([](int32_t *, int32_t *r2, AlignOpt &) { r2[6] = 130 + 201; });
	// a pair on the reverse strand: ql from r1->qs - r2->qe, the stretch starts at r2->qe of the forward strand
	{
		Batch b; b.target(1000); b.read(150);
		b.region(120, 150, 100, 130, INV_BIT_SPLIT1 | INV_BIT_REV, 0, 0);
		b.region(0, 30, 220, 250, INV_BIT_SPLIT2 | INV_BIT_SPLIT_INV | INV_BIT_REV, 5, 5);
		assert(b.plan(pl) == 0 && pl.cand.size() == 1 && pl.cand[0].ql == 90 && pl.cand[0].tl == 90 && pl.cand[0].qb == 30 && pl.cand[0].rev1 == 1); ++planned;
	}
	auto refuse = [&](Batch b) { assert(b.plan(pl) == -1 && !pl.err.empty()); ++refused; };
	{ Batch b = base; b.o.flag = AL_F_SR; refuse(b); }
	{ Batch b = base; b.o.flag = AL_F_SPLICE; refuse(b); }
	{ Batch b = base; b.o.q2 = 4; b.o.e2 = 2; refuse(b); }
	{ Batch b = base; b.o.a = 128; refuse(b); }
	{ Batch b = base; b.o.e = -1; refuse(b); }
	{ Batch b = base; b.o.max_gap = AL_MAX_GAP + 1; refuse(b); }
	{ Batch b = base; b.o.bw = -1; refuse(b); }
	{ Batch b = base; b.t_off = {0}; refuse(b); }                                   // no targets
	{ Batch b = base; b.seq_off[0] = 1; refuse(b); }
	{ Batch b = base; b.regs_off[1] = 5; b.regs_off[2] = 4; refuse(b); }            // falling offsets
	{ Batch b = base; b.regs[2] = b.regs[AL_REG_WORDS + 2] = 2; refuse(b); }        // a candidate's rid is no target
	{ Batch b = base; b.regs[2] = b.regs[AL_REG_WORDS + 2] = -1; refuse(b); }
	{ Batch b = base; b.t_off = {0, 199, 599}; refuse(b); }                         // [r1->re, r2->rs) ends past its target
	{ Batch b = base; b.regs[7] = -5; b.regs[AL_REG_WORDS + 6] = 60; refuse(b); }   // ... starts before it
	{ Batch b = base; assert(inv_plan(nullptr, 3, nullptr, nullptr, nullptr, 0, nullptr, pl) == -1); ++refused; (void)b; }
	{ Batch b = base; auto so = exact(b.seq_off), ro = exact(b.regs_off), to = exact(b.t_off);
	  assert(inv_plan(&b.o, 3, so.get(), ro.get(), nullptr, 2, to.get(), pl) == -1); ++refused; }                  // NULL regions
	// the checks shared with chaindp_align1 (align_check_opt, align_check_offsets): every refusal's text, under this call's name
	auto says = [&](const Batch &b, const char *text) { assert(b.plan(pl) == -1 && pl.err == text); ++refused; };
	assert(inv_plan(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, pl) == -1 && pl.err == "chaindp_align1_inv: NULL options"); ++refused;
	for (int64_t n : {(int64_t)-1, (int64_t)1 << 31}) {
		assert(inv_plan(&base.o, n, nullptr, nullptr, nullptr, 0, nullptr, pl) == -1 && pl.err == "chaindp_align1_inv: read count outside 0..2^31 - 1");
		++refused;
	}
	{ Batch b = base; b.o.flag = AL_F_SR; says(b, "chaindp_align1_inv: MM_F_SR and MM_F_SPLICE are not built"); }
	{ Batch b = base; b.o.flag = AL_F_SPLICE; b.o.a = -1; says(b, "chaindp_align1_inv: MM_F_SR and MM_F_SPLICE are not built"); }   // the flag before the scoring
	for (int k = 0; k < 6; ++k) for (int v : {-1, 128}) { Batch b = base; (&b.o.a)[k] = v; says(b, "chaindp_align1_inv: a, b, q, e, q2, e2 must lie in 0..127"); }
	{ Batch b = base; b.o.q2 = b.o.q; b.o.e2 = b.o.e; b.o.max_gap = -1; says(b, "chaindp_align1_inv: q == q2 and e == e2 (ksw_extz2_sse) is not built"); }
	for (int v : {-1, AL_MAX_GAP + 1}) { Batch b = base; b.o.max_gap = v; b.o.bw = -1; says(b, "chaindp_align1_inv: max_gap outside 0..20000"); }
	// ... what only this call checks of its options comes behind them, and before the offsets; k, min_cnt and min_ksw_len are not its own
	for (int v : {-1, (1 << 26) + 1}) { Batch b = base; b.t_off = {0}; b.o.bw = v; says(b, "chaindp_align1_inv: bw out of range"); }
	{ Batch b = base; b.o.k = -1; b.o.min_cnt = -1; b.o.min_ksw_len = -1; assert(b.plan(pl) == 0 && pl.cand.size() == 3); ++planned; }
	{
		const int64_t zero[3] = {0, 0, 0}, one[3] = {1, 1, 1}, fall[3] = {0, 5, 4}, big[3] = {0, 0x7fffffff, 0x7fffffff}, ok[3] = {0, 0x7ffffffe, 0x7ffffffe},
		              late[3] = {0, 0, 0x7fffffff};
		auto direct = [&](const int64_t *so, const int64_t *ro, int64_t n_t, const int64_t *to, const char *text) {
			assert(inv_plan(&base.o, 2, so, ro, nullptr, n_t, to, pl) == -1 && pl.err == text); ++refused;
		};
		direct(nullptr, zero, 1, zero, "chaindp_align1_inv: NULL offsets");
		direct(zero, nullptr, 0, nullptr, "chaindp_align1_inv: NULL offsets");         // ... before the targets are looked at
		direct(one, zero, 0, zero, "chaindp_align1_inv: no targets");                 // this call's rule: it needs a target; before the offsets' values
		direct(one, zero, -1, zero, "chaindp_align1_inv: no targets");
		direct(zero, zero, 1, nullptr, "chaindp_align1_inv: no targets");
		direct(one, zero, 1, zero, "chaindp_align1_inv: offsets must start at 0");
		direct(zero, one, 1, zero, "chaindp_align1_inv: offsets must start at 0");
		direct(fall, zero, 1, zero, "chaindp_align1_inv: falling offsets at read 1");
		direct(late, fall, 1, zero, "chaindp_align1_inv: falling offsets at read 1");  // a read's fall before its length
		direct(big, fall, 1, zero, "chaindp_align1_inv: read 0 is too long");         // ... read by read
		direct(zero, fall, 1, zero, "chaindp_align1_inv: falling offsets at read 1");
		direct(zero, big, 1, zero, "chaindp_align1_inv: NULL regions");               // regions are not counted per read: 2^31 - 1 of them pass the offsets
		direct(ok, big, 1, zero, "chaindp_align1_inv: NULL regions");                 // a read one below the limit passes them too
	}
	// a refused pair that returns early is no refusal: its rid is never looked at
	{ Batch b = base; b.regs[2] = b.regs[AL_REG_WORDS + 2] = 9; b.regs[AL_REG_WORDS + 15] &= ~(int32_t)INV_BIT_SPLIT_INV; assert(b.plan(pl) == 0 && pl.cand.size() == 2); ++planned; }
	// seeded batches: the candidates in slot order, the problems of the survivors inside their stretches, the DP's plan over them
	std::mt19937 rng(7);
	for (int round = 0; round < 12; ++round) {
		Batch b; b.target(4000);
		const int n = 1 + (int)(rng() % 40);
		for (int i = 0; i < n; ++i) b.pair(30 + (int)(rng() % 180), 30 + (int)(rng() % 180));
		assert(b.plan(pl) == 0 && pl.n_slots == 2 * n);
		std::vector<int32_t> ll(3 * pl.cand.size());
		for (size_t c = 0; c < pl.cand.size(); ++c) {
			const InvCand &C = pl.cand[c];
			assert(pl.slot_cand[(size_t)C.slot] == (int32_t)c && C.ql >= 40 && C.ql <= 200 && C.tl >= 40 && C.tl <= 200 && (c == 0 || pl.cand[c - 1].slot < C.slot));
			ll[3 * c] = (int)(rng() % 160);
			ll[3 * c + 1] = (int)(rng() % (unsigned)inv_ll_rows(C.ql)) + (rng() % 8 == 0 ? 50 : 0);          // now and then out of range: clamped
			ll[3 * c + 2] = (int)(rng() % (unsigned)C.tl) - (rng() % 8 == 0 ? 300 : 0);
		}
		std::vector<InvSurv> surv;
		KswPlan kp;
		int64_t n_bases = 0;
		inv_problems(b.o, pl, ll, surv, kp.prob, n_bases);
		assert(surv.size() == kp.prob.size());
		int64_t at = 0;
		size_t s = 0;
		for (size_t c = 0; c < pl.cand.size(); ++c) {
			if (ll[3 * c] < b.o.min_dp_max) continue;
			assert(s < surv.size() && surv[s].cand == (int32_t)c);
			const KswProb &p = kp.prob[s];
			const InvCand &C = pl.cand[c];
			assert(surv[s].q_off >= -7 && surv[s].q_off < C.ql && surv[s].t_off >= 0 && surv[s].t_off < C.tl);
			assert(p.qlen == C.ql - surv[s].q_off && p.tlen == C.tl - surv[s].t_off && p.q_beg == at && p.t_beg == at + p.qlen && p.w <= 750 && p.flag == 0x40 && p.end_bonus == -1);
			at += p.qlen + p.tlen;
			++s;
		}
		assert(s == surv.size() && at == n_bases);
		if (!ksw_plan_score(b.o.a, b.o.b, b.o.q, b.o.e, b.o.q2, b.o.e2, kp.sc)) assert(0);
		ksw_plan_route(kp, 256);
		assert(kp.order.size() == kp.prob.size() && kp.count[0] + kp.count[1] == (int64_t)kp.prob.size());
		++planned;
	}
	printf("inv plan ok: %d batches planned, %d calls refused\n", planned, refused);
	return 0;
}
