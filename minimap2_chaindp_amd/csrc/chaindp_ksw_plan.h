// chaindp_ksw_plan.h -- what the host decides about a batch of chaindp_ksw_extd before anything touches the device: the argument checks,
// the per-problem records, the order they are taken in and the sizes of every buffer; and, at the end, what the alignment stages share of
// their host side (buffer layout, CIGAR offsets).  No HIP in here: the kernels' translation unit takes the constants and the record from
// it, the host ABI the plan, and a stand-alone program runs the plan under the sanitizers.
#ifndef CHAINDP_KSW_PLAN_H
#define CHAINDP_KSW_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define KSW_HD __host__ __device__
#else
#define KSW_HD
#endif

namespace chaindp {

#define KSW_LDS_BUDGET 65536         // bytes of LDS a problem may take (the most a workgroup gets without asking for more)
#define KSW_MAX_SPAN (1 << 27)       // q_len + t_len stays below this: a cell's order among equal maxima is packed beside its t
#define KSW_ROUTE_NONE 0             // the reference's early returns: nothing computed
#define KSW_ROUTE_LDS 1              // state in LDS, one wave
#define KSW_ROUTE_GLOBAL 2           // state in global scratch, one wave
#define KSW_ROUTE_WIDE 3             // state in LDS, KSW_WIDE_WAVES waves: a state above KSW_WIDE_BYTES
#define KSW_WIDE_BYTES 8192
#ifndef KSW_WIDE_WAVES
#define KSW_WIDE_WAVES 4             // (a build with 1 is the one-wave loop over the same problems: DESIGN.md 8 has the comparison)
#endif
#define KSW_XCH_BYTES 128            // ahead of the state in LDS: where a workgroup's waves exchange their maxima, n_cigar and the problem taken
#define KSW_EZ_WORDS 12              // per problem on the device: the ten fields of ez_out, n_cigar, the route taken
struct KswProb { int64_t q_beg, t_beg, cig_beg; int32_t qlen, tlen, w, zdrop, end_bonus, flag; };
struct KswScore { int a, b, q, e, q2, e2, qe0, skip; };   // q + e <= q2 + e2 already (ksw2_extd2_sse.c:70); qe0: the caller's q + e, from before that swap
                                                          // (:60; what H of the first cell is seeded with); skip: b > 2 (q + e), every problem returns early
KSW_HD inline int64_t ksw_state_bytes(int qlen, int tlen)
{
	const int64_t T = ((int64_t)tlen + 15) / 16 * 16, Q = ((int64_t)qlen + 15) / 16 * 16;
	return 12 * T + Q + 16;
}
KSW_HD inline int ksw_n_col(int qlen, int tlen, int w)      // n_col_ * 16 of ksw2_extd2_sse.c:82-86
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	int n = qlen < tlen ? qlen : tlen;
	if (w < n - 1) n = w + 1;
	return ((n + 15) / 16 + 1) * 16;
}
KSW_HD inline int ksw_route(int qlen, int tlen, bool skip)
{
	if (skip || qlen <= 0 || tlen <= 0) return KSW_ROUTE_NONE;
	const int64_t bytes = ksw_state_bytes(qlen, tlen);
	return bytes <= KSW_WIDE_BYTES ? KSW_ROUTE_LDS : bytes <= KSW_LDS_BUDGET ? KSW_ROUTE_WIDE : KSW_ROUTE_GLOBAL;
}

// ---- host only
struct KswPlan {
	std::vector<KswProb> prob;       // one per problem; w above max(qlen, tlen) is that maximum (the same band), cig_beg = words before it
	std::vector<int32_t> order;      // the problems of launch 0, then those of launch 1, each by falling work: diagonals x cells per diagonal
	KswScore sc{};
	int64_t n_bases = 0;             // bases to upload: the furthest end of a problem
	int64_t cig_words = 0;           // sum of qlen + tlen over the problems that make a CIGAR: no CIGAR has more words
	// launch 0: one wave per problem (KSW_ROUTE_NONE, _LDS, _GLOBAL); launch 1: KSW_WIDE_WAVES waves (KSW_ROUTE_WIDE)
	int64_t count[2] = {0, 0};       // problems
	size_t lds_bytes[2] = {0, 0};    // the largest state of an LDS problem of the launch
	int grid[2] = {0, 0};            // workgroups; launch 1's slices of path matrix lie behind launch 0's
	size_t state_stride = 0;         // the largest state on the global route, rounded up to 256
	size_t path_stride[2] = {0, 0};  // the largest path matrix of the launch, rounded up to 256
	std::string err;
};
#define KSW_PATH_TOTAL ((size_t)1 << 32)    // the path slices of a launch's workgroups together stay below this while there are 64 or more

// From the records in pl.prob (lengths, band, flag; pl.sc set): cig_beg of every problem, the order, the two launches' sizes.
// cus: compute units of the device; grid_cap > 0: no launch gets more workgroups than that (chaindp_ksw_debug_set_grid_cap).
// What chaindp_align1 calls on the records its planning kernel made.
inline void ksw_plan_route(KswPlan &pl, int cus, int grid_cap = 0)
{
	const int64_t n = (int64_t)pl.prob.size();
	std::vector<int64_t> work((size_t)n);
	pl.cig_words = 0;
	for (int c = 0; c < 2; ++c) { pl.count[c] = 0; pl.lds_bytes[c] = 0; pl.path_stride[c] = 0; }
	pl.state_stride = 0;
	for (int64_t i = 0; i < n; ++i) {
		KswProb &p = pl.prob[(size_t)i];
		p.cig_beg = pl.cig_words;
		const int route = ksw_route(p.qlen, p.tlen, pl.sc.skip);
		work[(size_t)i] = 0;
		if (route == KSW_ROUTE_NONE) continue;
		const int64_t n_diag = (int64_t)p.qlen + p.tlen - 1, n_col = ksw_n_col(p.qlen, p.tlen, p.w);
		work[(size_t)i] = n_diag * n_col;
		if (!(p.flag & 0x01)) {
			pl.cig_words += (int64_t)p.qlen + p.tlen;
			pl.path_stride[route == KSW_ROUTE_WIDE] = std::max(pl.path_stride[route == KSW_ROUTE_WIDE], (size_t)(n_diag * n_col));
		}
		const size_t state = (size_t)ksw_state_bytes(p.qlen, p.tlen);
		if (route == KSW_ROUTE_GLOBAL) pl.state_stride = std::max(pl.state_stride, state);
		else pl.lds_bytes[route == KSW_ROUTE_WIDE] = std::max(pl.lds_bytes[route == KSW_ROUTE_WIDE], state);
	}
	pl.state_stride = (pl.state_stride + 255) / 256 * 256;
	for (int c = 0; c < 2; ++c) pl.path_stride[c] = (pl.path_stride[c] + 255) / 256 * 256;
	auto wide = [&](int32_t i) { return ksw_route(pl.prob[(size_t)i].qlen, pl.prob[(size_t)i].tlen, pl.sc.skip) == KSW_ROUTE_WIDE; };
	pl.order.resize((size_t)n);
	for (int64_t i = 0; i < n; ++i) pl.order[(size_t)i] = (int32_t)i;
	std::stable_sort(pl.order.begin(), pl.order.end(), [&](int32_t x, int32_t y) { return wide(x) != wide(y) ? wide(y) : work[(size_t)x] > work[(size_t)y]; });
	for (int64_t i = 0; i < n; ++i) ++pl.count[wide((int32_t)i)];
	// as many workgroups as can be resident: the LDS each asks for decides, up to 32 waves per compute unit
	const size_t lds_cu = 160 * 1024;
	for (int c = 0; c < 2; ++c) {
		const int waves = c ? KSW_WIDE_WAVES : 1;
		const size_t lds = pl.lds_bytes[c] + KSW_XCH_BYTES;
		int per_cu = (int)std::min<size_t>(32 / waves, lds_cu / lds);
		if (per_cu < 1) per_cu = 1;
		pl.grid[c] = (int)std::min<int64_t>(pl.count[c], (int64_t)(cus > 0 ? cus : 1) * per_cu);
		if (grid_cap > 0) pl.grid[c] = std::min(pl.grid[c], grid_cap);
	}
	// ... fewer while the launch's path slices together would pass KSW_PATH_TOTAL
	for (int c = 0; c < 2; ++c)
		while (pl.grid[c] > 64 && (size_t)pl.grid[c] * pl.path_stride[c] > KSW_PATH_TOTAL) pl.grid[c] = (pl.grid[c] + 1) / 2;
}

// the scoring set as the kernel takes it; false where a value lies outside 0..127
inline bool ksw_plan_score(int a, int b, int q, int e, int q2, int e2, KswScore &sc)
{
	for (int v : {a, b, q, e, q2, e2})
		if (v < 0 || v > 127) return false;
	const int qe0 = q + e;
	if (q2 + e2 < q + e) { std::swap(q, q2); std::swap(e, e2); }        // ksw2_extd2_sse.c:70
	sc = KswScore{a, b, q, e, q2, e2, qe0, b > 2 * (q + e)};
	return true;
}

// 0 and a filled plan, or -1 (CHAINDP_ERR_ARG) with plan.err.  cus, grid_cap: as ksw_plan_route takes them.
inline int ksw_plan(int64_t n, const uint8_t *bases, const int64_t *q_beg, const int32_t *q_len, const int64_t *t_beg, const int32_t *t_len,
                    int a, int b, int q, int e, int q2, int e2, const int32_t *w, const int32_t *zdrop, const int32_t *end_bonus,
                    const int32_t *flag, int cus, KswPlan &pl, int grid_cap = 0)
{
	pl = KswPlan();
	if (n < 0) { pl.err = "chaindp_ksw_extd: negative problem count"; return -1; }
	if (n > 0x7fffffff) { pl.err = "chaindp_ksw_extd: more than 2^31 - 1 problems"; return -1; }
	if (!ksw_plan_score(a, b, q, e, q2, e2, pl.sc)) { pl.err = "chaindp_ksw_extd: a, b, q, e, q2, e2 must lie in 0..127"; return -1; }
	if (n > 0 && (!q_beg || !q_len || !t_beg || !t_len || !w || !zdrop || !end_bonus || !flag)) { pl.err = "chaindp_ksw_extd: NULL per-problem array"; return -1; }
	pl.prob.resize((size_t)n);
	for (int64_t i = 0; i < n; ++i) {
		if (flag[i] & ~0xcb) { pl.err = "chaindp_ksw_extd: flag bit outside SCORE_ONLY, RIGHT, APPROX_MAX, EXTZ_ONLY, REV_CIGAR in problem " + std::to_string(i); return -1; }
		if (q_len[i] < 0 || t_len[i] < 0 || q_beg[i] < 0 || t_beg[i] < 0) { pl.err = "chaindp_ksw_extd: negative start or length in problem " + std::to_string(i); return -1; }
		if ((int64_t)q_len[i] + t_len[i] >= KSW_MAX_SPAN) { pl.err = "chaindp_ksw_extd: q_len + t_len of 2^27 or more in problem " + std::to_string(i); return -1; }
		if (q_beg[i] > INT64_MAX - q_len[i] || t_beg[i] > INT64_MAX - t_len[i]) { pl.err = "chaindp_ksw_extd: range past int64 in problem " + std::to_string(i); return -1; }
		if ((q_len[i] > 0 || t_len[i] > 0) && !bases) { pl.err = "chaindp_ksw_extd: NULL bases"; return -1; }
		KswProb &p = pl.prob[(size_t)i];
		const int32_t wmax = std::max(q_len[i], t_len[i]);
		p = KswProb{q_beg[i], t_beg[i], 0, q_len[i], t_len[i], std::min(w[i], wmax), zdrop[i], end_bonus[i], flag[i]};
		if (q_len[i] > 0) pl.n_bases = std::max(pl.n_bases, q_beg[i] + q_len[i]);
		if (t_len[i] > 0) pl.n_bases = std::max(pl.n_bases, t_beg[i] + t_len[i]);
	}
	for (int64_t i = 0; i < n; ++i) {
		const KswProb &p = pl.prob[(size_t)i];
		for (int64_t k = 0; k < p.qlen; ++k) if (bases[p.q_beg + k] > 4) { pl.err = "chaindp_ksw_extd: base above 4 in the query of problem " + std::to_string(i); return -1; }
		for (int64_t k = 0; k < p.tlen; ++k) if (bases[p.t_beg + k] > 4) { pl.err = "chaindp_ksw_extd: base above 4 in the target of problem " + std::to_string(i); return -1; }
	}
	ksw_plan_route(pl, cus, grid_cap);
	return 0;
}

// ---- what the alignment stages (chaindp_ksw_extd, chaindp_align1, chaindp_align1_inv) share of their host side
struct Carve {                       // consecutive 16-byte aligned pieces of one buffer
	size_t at = 0;
	size_t take(size_t bytes) { const size_t o = at; at += (bytes + 15) / 16 * 16; return o; }
};

// The DP's two buffers for N problems, in bytes: ksw_reserve takes the sizes from here, every reader (ksw_view) the offsets.  ksw_prob: the N
// records, then the N order words.  ksw_ez: the two launches' counters (8 bytes each), the N + 1 CSR offsets, the N x KSW_EZ_WORDS result words.
struct KswLayout {
	size_t order, prob_bytes;        // ksw_prob: where the order words start (the records start the buffer), the buffer's size
	size_t off, ez, ez_bytes;        // ksw_ez: where the CSR offsets and the result words start (the counters start the buffer), its size
	explicit KswLayout(size_t N)
		: order(N * sizeof(KswProb)), prob_bytes(order + N * sizeof(int32_t) + 16), off(2 * sizeof(int64_t)),
		  ez(off + (N + 1) * sizeof(int64_t)), ez_bytes(ez + N * KSW_EZ_WORDS * sizeof(int32_t) + 16) {}
};

// The end of a call that returns CIGARs.  The counts are word `at` of every `stride` words of cnt (ez: word 10 at stride KSW_EZ_WORDS;
// chaindp_align_extra_t: word 4 at stride 5): cigar_off[0..n] becomes their running sum, the total is returned.
inline int64_t cigar_prefix(const int32_t *cnt, size_t stride, size_t at, int64_t n, int64_t *cigar_off)
{
	cigar_off[0] = 0;
	for (int64_t i = 0; i < n; ++i) cigar_off[i + 1] = cigar_off[i] + cnt[(size_t)i * stride + at];
	return cigar_off[n];
}
// ... and whether the caller's array holds them: false with the refusal's text in err (CHAINDP_ERR_CAPACITY)
inline bool cigar_room(const char *who, int64_t total, int64_t cap, std::string &err)
{
	if (total <= cap) return true;
	err = std::string(who) + ": " + std::to_string((long long)total) + " CIGAR words, room for " + std::to_string((long long)cap);
	return false;
}

} // namespace chaindp
#endif
