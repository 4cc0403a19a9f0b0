// The plan of chaindp_ksw_extd on its own: every refusal, the empty call, and seeded batches whose sizes are checked against what the
// kernel will index -- the state block, H[], the path matrix and the CIGAR room of every problem, diagonal by diagonal.
// The arrays handed in are exactly as long as the call says, so a read past any of them is AddressSanitizer's to report.
#include <assert.h>
#include <limits.h>
#include <stdio.h>
#include <memory>
#include <random>
#include "../../minimap2_chaindp_amd/csrc/chaindp_ksw_plan.h"

using namespace chaindp;

struct Batch {
	std::vector<uint8_t> bases;
	std::vector<int64_t> q_beg, t_beg;
	std::vector<int32_t> q_len, t_len, w, zdrop, end_bonus, flag;
	int sc[6] = {2, 4, 4, 2, 24, 1};
	int plan(KswPlan &pl, int cus = 256, int cap = 0) const
	{
		// copies of exactly the stated sizes (an empty vector's data() may be anything: NULL is what a caller passes then)
		auto exact = [](const auto &v) { using T = typename std::decay<decltype(v[0])>::type; std::unique_ptr<T[]> p(new T[v.size()]); std::copy(v.begin(), v.end(), p.get()); return p; };
		auto b = exact(bases); auto qb = exact(q_beg); auto tb = exact(t_beg); auto ql = exact(q_len); auto tl = exact(t_len);
		auto w_ = exact(w); auto z = exact(zdrop); auto eb = exact(end_bonus); auto f = exact(flag);
		return ksw_plan((int64_t)q_len.size(), bases.empty() ? nullptr : b.get(), qb.get(), ql.get(), tb.get(), tl.get(), sc[0], sc[1], sc[2], sc[3], sc[4], sc[5],
		                w_.get(), z.get(), eb.get(), f.get(), cus, pl, cap);
	}
	void add(std::mt19937 &rng, int ql, int tl, int w_, int flag_)
	{
		q_beg.push_back((int64_t)bases.size()); q_len.push_back(ql);
		for (int k = 0; k < ql; ++k) bases.push_back((uint8_t)(rng() % 5));
		t_beg.push_back((int64_t)bases.size()); t_len.push_back(tl);
		for (int k = 0; k < tl; ++k) bases.push_back((uint8_t)(rng() % 5));
		w.push_back(w_); zdrop.push_back((int)(rng() % 500) - 1); end_bonus.push_back((int)(rng() % 12) - 1); flag.push_back(flag_);
	}
};

// what the kernel indexes for one problem, against the sizes the plan settled on
static void check_problem(const KswPlan &pl, const KswProb &p, int64_t cig_end)
{
	const int route = ksw_route(p.qlen, p.tlen, pl.sc.skip);
	if (route == KSW_ROUTE_NONE) return;
	const int64_t T = (p.tlen + 15) / 16 * 16, Q = (p.qlen + 15) / 16 * 16, block = 8 * T + Q + 16;
	assert(ksw_state_bytes(p.qlen, p.tlen) == block + 4 * T);
	if (route == KSW_ROUTE_GLOBAL) assert((size_t)(block + 4 * T) <= pl.state_stride);
	else assert((size_t)(block + 4 * T) <= pl.lds_bytes[route == KSW_ROUTE_WIDE] && block + 4 * T <= KSW_LDS_BUDGET);
	assert((route == KSW_ROUTE_LDS) == (block + 4 * T <= KSW_WIDE_BYTES));
	const int w = p.w < 0 ? std::max(p.qlen, p.tlen) : p.w;
	assert(w <= std::max(p.qlen, p.tlen));                         // no overflow in r + w
	const int64_t n_col = ksw_n_col(p.qlen, p.tlen, p.w), n_diag = (int64_t)p.qlen + p.tlen - 1;
	const bool cigar = !(p.flag & 1);
	if (cigar) {
		assert((size_t)(n_diag * n_col) <= pl.path_stride[route == KSW_ROUTE_WIDE]);
		assert(p.cig_beg + p.qlen + p.tlen <= cig_end);
	}
	for (int64_t r = 0; r < n_diag; ++r) {
		int64_t st0 = std::max<int64_t>(std::max<int64_t>(0, r - p.qlen + 1), (r - w + 1) >> 1), en0 = std::min<int64_t>(std::min<int64_t>(p.tlen - 1, r), (r + w) >> 1);
		if (st0 > en0) break;
		const int64_t st = st0 / 16 * 16, en = (en0 + 16) / 16 * 16 - 1, n_sc = ((en0 - st0) / 16 + 1) * 16;
		assert(en < T && en - st < n_col);                            // the cells and their row of the path matrix
		assert(6 * T + st0 + n_sc - 1 < block);                       // the score stores, from s into sf
		assert(7 * T + st0 + n_sc - 1 < block);                       // the target loads, from sf into qr
		assert(p.qlen - 1 - r + st0 >= 0 && 8 * T + (p.qlen - 1 - r) + st0 + n_sc - 1 < block);      // the query loads, into the padding
		if (en >= r) assert(r < T);                                   // y[r], y2[r], u[r]
	}
}

static void check_plan(const Batch &b, const KswPlan &pl, int cus, int cap = 0)
{
	const size_t n = b.q_len.size();
	assert(pl.prob.size() == n && pl.order.size() == n && (size_t)(pl.count[0] + pl.count[1]) == n);
	std::vector<int> seen(n, 0);
	for (size_t k = 0; k < n; ++k) {
		const int32_t i = pl.order[k];
		assert(i >= 0 && (size_t)i < n && !seen[(size_t)i]++);
		const bool wide = ksw_route(pl.prob[(size_t)i].qlen, pl.prob[(size_t)i].tlen, pl.sc.skip) == KSW_ROUTE_WIDE;
		assert(wide == ((int64_t)k >= pl.count[0]));                  // launch 0's problems first
	}
	int64_t ends = 0;
	for (size_t i = 0; i < n; ++i) {
		check_problem(pl, pl.prob[i], pl.cig_words);
		if (b.q_len[i]) ends = std::max(ends, b.q_beg[i] + b.q_len[i]);
		if (b.t_len[i]) ends = std::max(ends, b.t_beg[i] + b.t_len[i]);
	}
	assert(pl.n_bases == ends && (size_t)ends <= b.bases.size());
	for (int c = 0; c < 2; ++c) {
		assert((pl.grid[c] > 0) == (pl.count[c] > 0) && pl.grid[c] <= pl.count[c] && pl.grid[c] <= cus * 32);
		assert(pl.path_stride[c] % 256 == 0 && pl.lds_bytes[c] <= KSW_LDS_BUDGET);
		assert(pl.grid[c] <= 64 || (size_t)pl.grid[c] * pl.path_stride[c] <= KSW_PATH_TOTAL);
		if (cap > 0) assert(pl.grid[c] <= cap);                       // chaindp_ksw_debug_set_grid_cap
	}
	assert(pl.state_stride % 256 == 0);
}

int main()
{
	std::mt19937 rng(12345);
	KswPlan pl;
	int refused = 0, planned = 0, capped = 0;
	// the empty call
	{ Batch b; assert(b.plan(pl) == 0 && pl.prob.empty() && pl.grid[0] == 0 && pl.grid[1] == 0 && pl.cig_words == 0); }
	// refusals: each leaves a message and reads nothing it should not
	auto refuse = [&](Batch b) { assert(b.plan(pl) == -1 && !pl.err.empty()); ++refused; };
	Batch base; base.add(rng, 10, 12, -1, 0); base.add(rng, 7, 5, 3, 0x40);
	assert(base.plan(pl) == 0);
	for (int f : {0x04, 0x10, 0x20, 0x100, 0x200, 0x400, 0x800, -1, INT_MIN}) { Batch b = base; b.flag[1] = f; refuse(b); }
	for (int k = 0; k < 6; ++k) for (int v : {-1, 128, INT_MAX, INT_MIN}) { Batch b = base; b.sc[k] = v; refuse(b); }
	{ Batch b = base; b.q_len[0] = -1; refuse(b); }
	{ Batch b = base; b.t_len[1] = INT_MIN; refuse(b); }
	{ Batch b = base; b.q_beg[1] = -1; refuse(b); }
	{ Batch b = base; b.t_beg[0] = INT64_MIN; refuse(b); }
	{ Batch b = base; b.q_len[0] = KSW_MAX_SPAN; refuse(b); }                       // refused before a base of it is read
	{ Batch b = base; b.q_len[0] = INT_MAX; b.t_len[0] = INT_MAX; refuse(b); }
	{ Batch b = base; b.q_beg[0] = INT64_MAX; refuse(b); }
	{ Batch b = base; b.bases[3] = 5; refuse(b); }
	{ Batch b = base; b.bases.back() = 255; refuse(b); }
	{ Batch b = base; b.bases.clear(); b.q_beg = {0, 0}; b.t_beg = {0, 0}; refuse(b); }   // lengths but no bases at all
	{ Batch b; b.q_beg = {0}; b.t_beg = {0}; b.q_len = {0}; b.t_len = {0}; b.w = {0}; b.zdrop = {0}; b.end_bonus = {0}; b.flag = {0};
	  assert(b.plan(pl) == 0 && pl.n_bases == 0); }                                   // an empty problem needs no bases
	// seeded batches: sizes around every rounding and routing edge, w from none to INT_MAX, every accepted flag
	const int lens[] = {0, 1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 288, 304, 305, 656, 700, 2000, 2100, 5440, 5501};
	const int ws[] = {-1, INT_MIN, 0, 1, 2, 15, 16, 17, 100, 500, 751, INT_MAX};
	const int flags[] = {0, 0x01, 0x02, 0x08, 0x09, 0x40, 0x80, 0xc2, 0xcb};
	const int scorings[][6] = {{2, 4, 4, 2, 24, 1}, {1, 19, 39, 3, 81, 1}, {2, 4, 24, 1, 4, 2}, {1, 19, 4, 2, 24, 1}, {127, 127, 127, 127, 127, 127}, {0, 0, 0, 0, 0, 0}};
	for (int round = 0; round < 40; ++round) {
		Batch b;
		for (int k = 0; k < 6; ++k) b.sc[k] = scorings[round % 6][k];
		const int n = 1 + (int)(rng() % 40);
		for (int i = 0; i < n; ++i) {
			int ql = lens[rng() % 23], tl = lens[rng() % 23];
			if (ql > 1000 && tl > 1000 && round % 4) ql = 40;         // few of the largest: the check walks every diagonal
			b.add(rng, ql, tl, ws[rng() % 12], flags[rng() % 9]);
		}
		const int cus = round % 5 == 0 ? 1 : 256;
		assert(b.plan(pl, cus) == 0);
		assert(pl.sc.q + pl.sc.e <= pl.sc.q2 + pl.sc.e2 && pl.sc.qe0 == b.sc[2] + b.sc[3]);
		check_plan(b, pl, cus);
		++planned;
		// the grid cap: no launch above it, every size as before; cap 1 is one workgroup for the whole launch
		const int grid0[2] = {pl.grid[0], pl.grid[1]};
		for (int cap : {1, 3, 1 << 20}) {
			KswPlan pc;
			assert(b.plan(pc, cus, cap) == 0);
			check_plan(b, pc, cus, cap);
			for (int c = 0; c < 2; ++c) assert(pc.grid[c] == std::min(grid0[c], cap) && pc.path_stride[c] == pl.path_stride[c] && pc.lds_bytes[c] == pl.lds_bytes[c]);
			assert(pc.order == pl.order && pc.cig_words == pl.cig_words && pc.state_stride == pl.state_stride);
			++capped;
		}
	}
	// the shapes of the edge tier (tests/ksw_edge_shapes.py): one and two bases against the wide and global routes, the long queries
	{
		Batch b;
		const int shapes[][3] = {{1, 700, -1}, {2, 690, -1}, {7793, 17, -1}, {7793, 17, 5}, {1, 5500, -1}, {2, 5470, -1}, {3000, 5500, 100}, {5480, 5500, 20},
		                         {300, 5600, -1}, {64, 5470, 70}, {600, 610, 1}, {3000, 640, 8}, {100, 1500, 60}};
		for (const auto &s : shapes) for (int f : {0, 0x01, 0xc2}) b.add(rng, s[0], s[1], s[2], f);
		for (int cap : {0, 1, 2}) { assert(b.plan(pl, 256, cap) == 0); check_plan(b, pl, 256, cap); ++capped; }
	}
	// the halving of the grid: 65 to 400 one-wave problems, one of them global with a path matrix of 32 to 128 MiB -- that many slices
	// of that size pass KSW_PATH_TOTAL, so the grid comes out below min(count, cus * per_cu)
	int halved = 0;
	for (int n : {65, 66, 127, 128, 129, 200, 400}) {
		Batch b;
		int big;                                                        // 7 999 x 4 016 = 32 MiB .. 15 999 x 8 016 = 128 MiB
		do big = 4000 + (int)(rng() % 4001); while ((size_t)n * (size_t)(2 * big - 1) * (size_t)ksw_n_col(big, big, -1) <= KSW_PATH_TOTAL + ((size_t)n << 8));
		const int at = (int)(rng() % n);
		for (int i = 0; i < n; ++i) {
			if (i == at) b.add(rng, big, big, -1, 0x40);
			else b.add(rng, lens[1 + rng() % 13], lens[1 + rng() % 13], ws[rng() % 12], flags[rng() % 9]);
		}
		assert(b.plan(pl) == 0);
		check_plan(b, pl, 256);
		const size_t path = (size_t)(2 * big - 1) * (size_t)ksw_n_col(big, big, -1);
		assert(path >= ((size_t)32 << 20) - 4096 * 16 && path <= (size_t)128 << 20 && pl.path_stride[0] == (path + 255) / 256 * 256);
		assert(pl.count[0] == n && pl.count[1] == 0);
		assert((size_t)n * pl.path_stride[0] > KSW_PATH_TOTAL);            // ... so the loop had to run
		assert(pl.grid[0] < n && pl.grid[0] >= 32 && pl.grid[0] <= 64);      // n < cus * per_cu: the natural grid would have been n
		KswPlan pc;                                                     // the cap comes first: a capped grid of 64 or less is not halved
		assert(b.plan(pc, 256, 3) == 0 && pc.grid[0] == 3);
		check_plan(b, pc, 256, 3);
		++halved;
	}
	// what the alignment stages share of their host side.  The DP's buffers for N problems: the offsets and sizes as the stages spelled
	// them out before there was a description
	int layouts = 0;
	for (size_t N : {0, 1, 2, 63, 64, 65, 4160}) {
		const KswLayout lay(N);
		assert(lay.order == N * sizeof(KswProb) && lay.off == 2 * 8 && lay.ez == (2 + N + 1) * 8);
		assert(lay.prob_bytes == N * sizeof(KswProb) + N * 4 + 16);
		assert(lay.ez_bytes == N * KSW_EZ_WORDS * 4 + (N + 1) * 8 + 32);
		assert(lay.order + N * 4 <= lay.prob_bytes && lay.ez + N * KSW_EZ_WORDS * 4 <= lay.ez_bytes && lay.order % 8 == 0 && lay.ez % 8 == 0);
		// pieces of N-dependent sizes, one of them empty: 16-byte aligned, in order, none reaching into the next
		Carve c;
		const size_t bytes[] = {(N + 1) * 8, N * 4, 0, N * sizeof(KswProb), 1, N * 20, 17};
		size_t end = 0;
		for (size_t b : bytes) {
			const size_t o = c.take(b);
			assert(o % 16 == 0 && o >= end && o < end + 16 && c.at >= o + b && c.at % 16 == 0 && c.at < o + b + 16);
			end = o + b;
		}
		// the CIGAR offsets from the counts, as ez keeps them (word 10 of KSW_EZ_WORDS) and as chaindp_align_extra_t does (word 4 of 5)
		const size_t strides[2][2] = {{KSW_EZ_WORDS, 10}, {5, 4}};
		for (const auto &sa : strides) {
			std::unique_ptr<int32_t[]> cnt(new int32_t[N * sa[0] + 1]);
			std::unique_ptr<int64_t[]> off(new int64_t[N + 1]);
			for (size_t i = 0; i < N * sa[0] + 1; ++i) cnt[i] = -1000000;              // a word that is no count spoils the sum
			int64_t sum = 0;
			for (size_t i = 0; i < N; ++i) sum += cnt[i * sa[0] + sa[1]] = (int32_t)(rng() % 3 ? rng() % 5000 : 0);
			for (size_t i = 0; i <= N; ++i) off[i] = -1;
			assert(cigar_prefix(cnt.get(), sa[0], sa[1], (int64_t)N, off.get()) == sum && off[0] == 0 && off[N] == sum);
			for (size_t i = 0; i < N; ++i) assert(off[i + 1] - off[i] == cnt[i * sa[0] + sa[1]]);
			// room for exactly that many words is room enough; one word less is the refusal, in the words of each of the three calls
			std::string err = "untouched";
			assert(cigar_room("chaindp_ksw_extd", sum, sum, err) && cigar_room("chaindp_align1", sum, sum + 1, err) && err == "untouched");
			for (const char *who : {"chaindp_ksw_extd", "chaindp_align1", "chaindp_align1_inv"}) {
				assert(!cigar_room(who, sum + 1, sum, err));
				assert(err == std::string(who) + ": " + std::to_string((long long)(sum + 1)) + " CIGAR words, room for " + std::to_string((long long)sum));
				++refused;
			}
		}
		++layouts;
	}
	{
		std::string err;
		assert(!cigar_room("chaindp_ksw_extd", 13, 12, err) && err == "chaindp_ksw_extd: 13 CIGAR words, room for 12");
		assert(!cigar_room("chaindp_align1", 4097, 4096, err) && err == "chaindp_align1: 4097 CIGAR words, room for 4096");
		assert(!cigar_room("chaindp_align1_inv", 1, 0, err) && err == "chaindp_align1_inv: 1 CIGAR words, room for 0");
		assert(cigar_room("chaindp_align1_inv", 0, 0, err));
	}
	printf("ksw plan ok: %d batches planned, %d calls refused; %d plans under a grid cap, %d with a halved grid; %d buffer layouts\n", planned, refused, capped,
	       halved, layouts);
	return 0;
}
