// chaindp_abi_ksw.cpp -- the alignment stage of the host ABI (include/chaindp_ksw.h): ksw_extd2_sse for a batch of problems.
// The plan (checks, records, order, sizes) is chaindp_ksw_plan.h's; this file owns the buffers, the copies and the two launches.
#include "chaindp_ctx.h"
#include <string.h>

using namespace chaindp;

// a buffer of the stage: grown new-then-free; a device without room is the batch's problem (CHAINDP_ERR_CAPACITY), not the context's
int chaindp::ksw_grow(chaindp_ctx *ctx, DevGrow &g, size_t need, const char *what, const char *who)
{
	const hipError_t e = dev_grow(ctx, g, need);
	if (e == hipSuccess) return CHAINDP_OK;
	(void)hipGetLastError();
	ctx->err = std::string(who) + ": " + what + " (" + std::to_string((unsigned long long)need) + " bytes): " + hipGetErrorString(e);
	return e == hipErrorOutOfMemory ? CHAINDP_ERR_CAPACITY : CHAINDP_ERR_HIP;
}

// every buffer a planned batch needs (the stream is idle: a buffer that grows is freed)
int chaindp::ksw_reserve(chaindp_ctx *ctx, const KswPlan &pl, int64_t n_bases, const char *who)
{
	const size_t N = pl.prob.size();
	int rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_bases, (size_t)n_bases + 16, "sequences", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_prob, N * sizeof(KswProb) + N * sizeof(int32_t) + 16, "problem records", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_ez, N * KSW_EZ_WORDS * sizeof(int32_t) + (N + 1) * sizeof(int64_t) + 32, "results", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_state, (size_t)pl.grid[0] * pl.state_stride + 16, "DP state", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_path, (size_t)pl.grid[0] * pl.path_stride[0] + (size_t)pl.grid[1] * pl.path_stride[1] + 16, "path matrices", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_cig, (size_t)pl.cig_words * sizeof(uint32_t) + 16, "CIGAR staging", who))) return rc;
	ctx->ksw_n = 0;
	for (int c = 0; c < 2; ++c) {                        // chaindp_ksw_debug_launch
		ctx->ksw_launch[c] = pl.count[c]; ctx->ksw_launch[2 + c] = pl.grid[c];
		ctx->ksw_launch[4 + c] = (int64_t)pl.lds_bytes[c]; ctx->ksw_launch[6 + c] = (int64_t)pl.path_stride[c];
	}
	return CHAINDP_OK;
}

// the records and their order up, the two launches; the bases are on the device already.  ev0 / ev1 (or null): recorded around the launches
int chaindp::ksw_dispatch(chaindp_ctx *ctx, const KswPlan &pl, hipEvent_t ev0, hipEvent_t ev1)
{
	const size_t N = pl.prob.size();
	hipStream_t st = ctx->stream;
	// ksw_prob: the records, then the order; ksw_ez: the two launches' counters (8 bytes each), the CSR offsets, the result words
	KswProb *d_prob = (KswProb*)ctx->ksw_prob.p;
	int32_t *d_order = (int32_t*)(d_prob + N);
	unsigned int *d_counter = (unsigned int*)ctx->ksw_ez.p;
	int32_t *d_ez = (int32_t*)((int64_t*)ctx->ksw_ez.p + 2 + N + 1);
	HIP_TRY(ctx, hipMemcpyAsync(d_prob, pl.prob.data(), N * sizeof(KswProb), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_order, pl.order.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, st));
	if (ev0) HIP_TRY(ctx, hipEventRecord(ev0, st));
	// the wide problems first: theirs are the long workgroups, the one-wave ones fill in behind them
	HIP_TRY(ctx, launch_ksw_extd(st, KSW_WIDE_WAVES, pl.grid[1], pl.lds_bytes[1], pl.count[1], d_prob, d_order + pl.count[0], (const uint8_t*)ctx->ksw_bases.p,
	                             pl.sc, nullptr, 0, (uint8_t*)ctx->ksw_path.p + (size_t)pl.grid[0] * pl.path_stride[0], pl.path_stride[1], d_ez,
	                             (uint32_t*)ctx->ksw_cig.p, d_counter + 2));
	HIP_TRY(ctx, launch_ksw_extd(st, 1, pl.grid[0], pl.lds_bytes[0], pl.count[0], d_prob, d_order, (const uint8_t*)ctx->ksw_bases.p, pl.sc,
	                             (uint8_t*)ctx->ksw_state.p, pl.state_stride, (uint8_t*)ctx->ksw_path.p, pl.path_stride[0], d_ez, (uint32_t*)ctx->ksw_cig.p,
	                             d_counter));
	if (ev1) HIP_TRY(ctx, hipEventRecord(ev1, st));
	return CHAINDP_OK;
}

extern "C" int chaindp_ksw_extd(chaindp_ctx_t *ctx, int64_t n, const uint8_t *bases, const int64_t *q_beg, const int32_t *q_len,
                                const int64_t *t_beg, const int32_t *t_len, int a, int b, int q, int e, int q2, int e2, const int32_t *w,
                                const int32_t *zdrop, const int32_t *end_bonus, const int32_t *flag, int32_t *ez_out, int64_t *cigar_off,
                                uint32_t *cigar, int64_t cigar_cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!cigar_off || (n > 0 && !ez_out)) { ctx->err = "chaindp_ksw_extd: NULL output array"; return CHAINDP_ERR_ARG; }
	if (cigar_cap < 0 || (cigar_cap > 0 && !cigar)) { ctx->err = "chaindp_ksw_extd: cigar_cap without a cigar array"; return CHAINDP_ERR_ARG; }
	KswPlan pl;
	if (ksw_plan(n, bases, q_beg, q_len, t_beg, t_len, a, b, q, e, q2, e2, w, zdrop, end_bonus, flag, ctx->dp.cus, pl, ctx->ksw_grid_cap)) {
		ctx->err = pl.err;
		return CHAINDP_ERR_ARG;
	}
	cigar_off[0] = 0;
	if (n == 0) return CHAINDP_OK;                       // nothing to do, nothing allocated
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // a buffer that grows is freed: nothing of an earlier call may be in flight
	const size_t N = (size_t)n;
	int rc;
	if ((rc = ksw_reserve(ctx, pl, pl.n_bases, "chaindp_ksw_extd"))) return rc;
	hipStream_t st = ctx->stream;
	KswProb *d_prob = (KswProb*)ctx->ksw_prob.p;
	int64_t *d_off = (int64_t*)ctx->ksw_ez.p + 2;
	int32_t *d_ez = (int32_t*)(d_off + N + 1);
	if (pl.n_bases) HIP_TRY(ctx, hipMemcpyAsync(ctx->ksw_bases.p, bases, (size_t)pl.n_bases, hipMemcpyHostToDevice, st));
	struct Events {                                       // while profiling is on: the DP kernels' own time, apart from the copies around them
		hipEvent_t e[2] = {nullptr, nullptr};
		~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
		hipEvent_t operator[](int k) const { return e[k]; }
	} ev;
	if (ctx->prof) {
		HIP_TRY(ctx, hipEventCreate(&ev.e[0]));
		HIP_TRY(ctx, hipEventCreate(&ev.e[1]));
	}
	if ((rc = ksw_dispatch(ctx, pl, ev[0], ev[1]))) return rc;
	std::vector<int32_t> ez(N * KSW_EZ_WORDS);
	HIP_TRY(ctx, hipMemcpyAsync(ez.data(), d_ez, ez.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (ev[0]) {
		float ms = 0;
		HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
		ctx->ksw_ms = ms;
	}
	ctx->ksw_n = n;
	for (size_t i = 0; i < N; ++i) {
		memcpy(ez_out + i * 10, ez.data() + i * KSW_EZ_WORDS, 10 * sizeof(int32_t));
		cigar_off[i + 1] = cigar_off[i] + ez[i * KSW_EZ_WORDS + 10];
	}
	const int64_t total = cigar_off[N];
	if (total > cigar_cap) {
		ctx->err = "chaindp_ksw_extd: " + std::to_string((long long)total) + " CIGAR words, room for " + std::to_string((long long)cigar_cap);
		return CHAINDP_ERR_CAPACITY;
	}
	if (total == 0) return CHAINDP_OK;
	if ((rc = ksw_grow(ctx, ctx->ksw_out, (size_t)total * sizeof(uint32_t), "CIGARs", "chaindp_ksw_extd"))) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(d_off, cigar_off, (N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, launch_ksw_pack(st, n, d_prob, d_ez, d_off, (const uint32_t*)ctx->ksw_cig.p, (uint32_t*)ctx->ksw_out.p));
	HIP_TRY(ctx, hipMemcpyAsync(cigar, ctx->ksw_out.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	return CHAINDP_OK;
}

// test hook (no GPU needed): what the device routes a problem by -- out = KSW_LDS_BUDGET, then the bytes of state per target base,
// per query base (both lengths rounded up to 16 first) and per problem: LDS while their sum fits the budget, global scratch beyond;
// out[4] = KSW_WIDE_BYTES (a sum above it gets out[5] = KSW_WIDE_WAVES waves).
extern "C" int chaindp_ksw_debug_routing(int64_t out[6])
{
	if (!out) return CHAINDP_ERR_ARG;
	out[0] = KSW_LDS_BUDGET;
	out[3] = ksw_state_bytes(0, 0);
	out[1] = (ksw_state_bytes(0, 16) - out[3]) / 16;
	out[2] = (ksw_state_bytes(16, 0) - out[3]) / 16;
	out[4] = KSW_WIDE_BYTES; out[5] = KSW_WIDE_WAVES;
	return CHAINDP_OK;
}

// tuning hook: device milliseconds of k_ksw_extd in the last chaindp_ksw_extd made while profiling was on (chaindp_set_profiling); -1 before
extern "C" double chaindp_ksw_debug_ms(chaindp_ctx_t *ctx) { return ctx ? ctx->ksw_ms : -1; }

// test hook: at most cap workgroups in either DP launch of every later plan (chaindp_ksw_extd, chaindp_align1, chaindp_align1_inv), so
// that a workgroup takes problem after problem; 0 leaves the plan alone.  Launches nothing.
extern "C" int chaindp_ksw_debug_set_grid_cap(chaindp_ctx_t *ctx, int cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (cap < 0) { ctx->err = "chaindp_ksw_debug_set_grid_cap: negative cap"; return CHAINDP_ERR_ARG; }
	ctx->ksw_grid_cap = cap;
	return CHAINDP_OK;
}

// test hook: the last plan the DP's buffers were sized for -- count[0..1], grid[0..1], lds_bytes[0..1], path_stride[0..1].  Launches nothing.
extern "C" int chaindp_ksw_debug_launch(chaindp_ctx_t *ctx, int64_t out[8])
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!out) { ctx->err = "chaindp_ksw_debug_launch: NULL out"; return CHAINDP_ERR_ARG; }
	memcpy(out, ctx->ksw_launch, sizeof ctx->ksw_launch);
	return CHAINDP_OK;
}

// test hook: the route every problem of the last chaindp_ksw_extd took, as the device reported it (0 early return, 1 LDS, 2 global, 3 LDS with several waves)
extern "C" int chaindp_ksw_debug_route(chaindp_ctx_t *ctx, int64_t n, int32_t *route)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n != ctx->ksw_n || (n > 0 && !route)) { ctx->err = "chaindp_ksw_debug_route: not the problem count of the last chaindp_ksw_extd"; return CHAINDP_ERR_ARG; }
	if (n == 0) return CHAINDP_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	std::vector<int32_t> ez((size_t)n * KSW_EZ_WORDS);
	const int32_t *d_ez = (const int32_t*)((const int64_t*)ctx->ksw_ez.p + 2 + n + 1);
	HIP_TRY(ctx, hipMemcpyAsync(ez.data(), d_ez, ez.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	for (int64_t i = 0; i < n; ++i) route[i] = ez[(size_t)i * KSW_EZ_WORDS + 11];
	return CHAINDP_OK;
}
