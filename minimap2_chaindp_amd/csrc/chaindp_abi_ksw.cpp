// chaindp_abi_ksw.cpp -- the alignment stage of the host ABI (include/chaindp_ksw.h): ksw_extd2_sse for a batch of problems, and the
// host scaffold it shares with chaindp_align1 and chaindp_align1_inv (declared in chaindp_ctx.h): the DP's buffers and their view, the
// two launches, the stage events, the CIGARs out.  The plan (checks, records, order, sizes, the buffers' layout) is chaindp_ksw_plan.h's.
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
	const KswLayout lay(pl.prob.size());
	int rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_bases, (size_t)n_bases + 16, "sequences", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_prob, lay.prob_bytes, "problem records", who))) return rc;
	if ((rc = ksw_grow(ctx, ctx->ksw_ez, lay.ez_bytes, "results", who))) return rc;
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

hipError_t chaindp::host_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
	for (size_t at = 0; at < bytes; at += KSW_COPY_PIECE)
		if (hipError_t e = hipMemcpyAsync((char*)dst + at, (const char*)src + at, std::min(KSW_COPY_PIECE, bytes - at), kind, st)) return e;
	return hipSuccess;
}

KswView chaindp::ksw_view(const chaindp_ctx *ctx, size_t N)
{
	const KswLayout lay(N);
	char *prob = (char*)ctx->ksw_prob.p, *ez = (char*)ctx->ksw_ez.p;
	return KswView{(KswProb*)prob, (int32_t*)(prob + lay.order), (unsigned int*)ez, (int64_t*)(ez + lay.off), (int32_t*)(ez + lay.ez), (uint32_t*)ctx->ksw_cig.p};
}

StageEvents::~StageEvents() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }

hipError_t StageEvents::mark(int stage_)
{
	if (!ctx->prof) return hipSuccess;
	hipEvent_t x;
	if (hipError_t err = hipEventCreate(&x)) return err;
	e.push_back(x); stage.push_back(stage_);
	return hipEventRecord(x, ctx->stream);
}

int StageEvents::fold(double *ms, int n)
{
	if (e.empty()) return CHAINDP_OK;
	for (int k = 0; k < n; ++k) ms[k] = 0;
	for (size_t k = 1; k < e.size(); ++k) {
		if (stage[k] < 0) continue;
		float t = 0;
		HIP_TRY(ctx, hipEventElapsedTime(&t, e[k - 1], e[k]));
		ms[stage[k]] += t;
	}
	return CHAINDP_OK;
}

int chaindp::ksw_dispatch(chaindp_ctx *ctx, const KswPlan &pl, StageEvents *ev)
{
	const size_t N = pl.prob.size();
	hipStream_t st = ctx->stream;
	const KswView v = ksw_view(ctx, N);
	HIP_TRY(ctx, host_copy(v.prob, pl.prob.data(), N * sizeof(KswProb), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, host_copy(v.order, pl.order.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, st));
	if (ev) HIP_TRY(ctx, ev->mark(-1));
	// the wide problems first: theirs are the long workgroups, the one-wave ones fill in behind them
	HIP_TRY(ctx, launch_ksw_extd(st, KSW_WIDE_WAVES, pl.grid[1], pl.lds_bytes[1], pl.count[1], v.prob, v.order + pl.count[0], (const uint8_t*)ctx->ksw_bases.p,
	                             pl.sc, nullptr, 0, (uint8_t*)ctx->ksw_path.p + (size_t)pl.grid[0] * pl.path_stride[0], pl.path_stride[1], v.ez,
	                             v.cig, v.counter + 2));
	HIP_TRY(ctx, launch_ksw_extd(st, 1, pl.grid[0], pl.lds_bytes[0], pl.count[0], v.prob, v.order, (const uint8_t*)ctx->ksw_bases.p, pl.sc,
	                             (uint8_t*)ctx->ksw_state.p, pl.state_stride, (uint8_t*)ctx->ksw_path.p, pl.path_stride[0], v.ez, v.cig, v.counter));
	if (ev) HIP_TRY(ctx, ev->mark(0));
	return CHAINDP_OK;
}

int chaindp::cigar_pack_out(chaindp_ctx *ctx, const char *who, const int64_t *cigar_off, int64_t n, int64_t total, uint32_t *cigar, int64_t cigar_cap,
                            int64_t *d_off, const std::function<hipError_t(uint32_t *out)> &launch)
{
	if (!cigar_room(who, total, cigar_cap, ctx->err)) return CHAINDP_ERR_CAPACITY;
	if (total == 0) return CHAINDP_OK;
	hipStream_t st = ctx->stream;
	if (int rc = ksw_grow(ctx, ctx->cigar_out, (size_t)total * sizeof(uint32_t) + 16, "CIGARs", who)) return rc;
	HIP_TRY(ctx, host_copy(d_off, cigar_off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, launch((uint32_t*)ctx->cigar_out.p));
	HIP_TRY(ctx, host_copy(cigar, ctx->cigar_out.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	return CHAINDP_OK;
}

int chaindp::cigar_pack_dev(chaindp_ctx *ctx, const int64_t *cigar_off, int64_t n, int64_t total, int64_t *d_off, const std::function<int(int64_t total, uint32_t **out)> &room,
                            const std::function<hipError_t(uint32_t *out)> &launch)
{
	if (total == 0) return CHAINDP_OK;
	uint32_t *out = nullptr;
	if (int rc = room(total, &out)) return rc;
	HIP_TRY(ctx, host_copy(d_off, cigar_off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, launch(out));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
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
	const KswView v = ksw_view(ctx, N);
	if (pl.n_bases) HIP_TRY(ctx, host_copy(ctx->ksw_bases.p, bases, (size_t)pl.n_bases, hipMemcpyHostToDevice, st));
	StageEvents ev(ctx);                                 // the DP kernels' own time, apart from the copies around them
	if ((rc = ksw_dispatch(ctx, pl, &ev))) return rc;
	std::vector<int32_t> ez(N * KSW_EZ_WORDS);
	HIP_TRY(ctx, host_copy(ez.data(), v.ez, ez.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if ((rc = ev.fold(&ctx->ksw_ms, 1))) return rc;
	ctx->ksw_n = n;
	for (size_t i = 0; i < N; ++i) memcpy(ez_out + i * 10, ez.data() + i * KSW_EZ_WORDS, 10 * sizeof(int32_t));
	const int64_t total = cigar_prefix(ez.data(), KSW_EZ_WORDS, 10, n, cigar_off);
	return cigar_pack_out(ctx, "chaindp_ksw_extd", cigar_off, n, total, cigar, cigar_cap, v.off, [&](uint32_t *out) {
		return launch_ksw_pack(st, n, v.prob, v.ez, v.off, v.cig, out);
	});
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
	HIP_TRY(ctx, host_copy(ez.data(), ksw_view(ctx, (size_t)n).ez, ez.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	for (int64_t i = 0; i < n; ++i) route[i] = ez[(size_t)i * KSW_EZ_WORDS + 11];
	return CHAINDP_OK;
}
