// chaindp_abi.cpp -- host side of the C ABI declared in include/chaindp.h.
// Owns the per-GPU context (stream, HBM buffers, scratch), stages batches and launches the kernels
// of chaindp_kernels.hip / chaindp_compact.hip.  No CPU implementation of the DP exists in this
// library: without a GPU every entry point fails with CHAINDP_ERR_NODEVICE.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/chaindp.h"
#include "chaindp_kernels.h"
#include "chaindp_devmem.h"

using chaindp::Params;
using chaindp::Unit;

static thread_local std::string g_create_error;

struct EventSet { hipEvent_t e[3]; int n; int slot0; };  // e[0..n): consecutive kernel boundaries; slot0 = first ms[] index

struct chaindp_ctx {
	int device = -1;
	// every device buffer below is an entry of this pool: allocated, grown and freed through it and nowhere else
	chaindp::DevPool pool{[](void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }, [](void *p) { return (int)hipFree(p); }};
	hipStream_t stream = nullptr;
	int64_t cap_anchors = 0, cap_reads = 0;
	int ring = 128;
	// resident batch
	int64_t n_reads = 0, total = 0, n_seeds = 0;
	bool has_n_segs = false, ran = false;
	bool singles_pending = false;    // the last run left f, p, v, flags[] of its singletons to k_fill_singles (chaindp_download runs it)
	chaindp_params_t ran_par{};      // the parameters of that run
	int64_t *d_off = nullptr;
	void *d_a = nullptr;
	int32_t *d_n_segs = nullptr;
	int32_t *d_f = nullptr, *d_p = nullptr, *d_v = nullptr;
	// scratch
	unsigned long long *d_tg = nullptr;   // deep-path marks, tagged with the run epoch (never re-initialised)
	uint32_t epoch = 0;
	unsigned long long *d_sumq = nullptr;
	Unit *d_units = nullptr;
	chaindp::UnitAux *d_unit_aux = nullptr;   // per unit, beside d_units: what k_chain_twin needs to pick it up without further loads
	Unit *d_left = nullptr;               // units the two-per-wave kernel hands over to k_chain_units
	unsigned long long *d_left_cnt = nullptr;   // [0] handed-over count | the twin / quad kernel's queue << 32; [1] count of d_deep; [2] k_chain_dense1's two queues;
	                                            // [3] route: 1 = k_chain_quad took the batch, 2 / 3 = k_chain_twin with one / two cost tables
	Unit *d_deep = nullptr;               // units k_chain_units hands over to its k_chain_dense (scans that keep reaching past the ring)
	int deep_route = 0;                   // test hook: 1 k_chain_dense, 2 k_chain_dense1 whatever the batch looks like
	int deep_eager = 0;                   // test hook: hand over any unit with a few deep scans, whatever its length
	bool deep_handover = true;            // CHAINDP_NO_DEEP_HANDOVER (diagnostic / A-B): every unit stays in the launch that took it
	bool use_quad = false;                // CHAINDP_QUAD=1 / chaindp_debug_set_quad (A/B, tests): one-table batches of ordinary units four per wave
	                                      // (k_chain_quad: correct, measured slower than k_chain_twin -- DESIGN.md section 6 -- so off by default)
	int twin_two_tables = 0;              // chaindp_debug_set_twin_tables (tests): 1 keeps one-key batches on k_chain_twin's two-table layout
	int twin_force_left = 0;              // CHAINDP_TWIN_FORCE_LEFT / chaindp_debug_set_twin_handover (tests): 1 k_chain_twin hands every unit
	                                      // over untouched, 2 after its first tile (k_chain_units resumes there); the variable is read once, at chaindp_create
	int variant = 0;                      // 0: k_chain_twin + k_chain_units for the rest; 1: k_chain_units, general variant; 2: k_chain_units only
	unsigned long long *d_counters = nullptr;
	chaindp::PrepassScratch pre = {nullptr, nullptr, nullptr, nullptr, nullptr};
	chaindp::CompactScratch cmp = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	chaindp::BottomScratch bot = {};
	// first-use groups of buffers: each flag is set once, after its group's allocations have all succeeded, and never reset
	bool compact_ready = false, bot_ready = false, seed_ready = false, regs_ready = false, post_ready = false, logf_ready = false;
	uint16_t *d_lut = nullptr;
	void **d_ptrs = nullptr;         // per-read host pointers for the gather / scatter kernels
	size_t ptr_bytes = 0;
	size_t lut_bytes = 0;
	bool use_lut = true;
	// compaction (allocated on first use)
	int32_t *d_first_child = nullptr;
	unsigned int *d_twin_queue = nullptr;   // k_chain_twin's eight grab counters, a cache line apart (2 KB)
	int64_t *d_seeds_off = nullptr;
	void *d_seeds = nullptr;
	// seed collection (allocated on first use, grown with the batch)
	chaindp::SeedScratch seed = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	void *d_mini = nullptr;
	int64_t *d_mini_off = nullptr, *d_mp_off = nullptr;
	uint32_t *d_bid = nullptr;
	int32_t *d_qlen = nullptr, *d_rep_len = nullptr;
	unsigned long long *d_mini_pos = nullptr;
	int64_t seed_cap_mini = 0, n_mini_pos = 0;
	int seed_max_n = -1, seed_max_n2 = -1; // largest reads the two configurations of the LDS sort take on this device
	int seed_lab_cap = 0;                  // digits k_seed_sort_huge keeps in LDS
	bool seed_route_valid = false;         // seed.totals[2..3] are the last collection's (chaindp_debug_seed_route): its sort was launched
	// chains to hits (allocated on first use, grown with the batch)
	void *d_regs = nullptr, *d_reg_counts = nullptr, *d_ref_len = nullptr, *d_mp_up = nullptr;
	size_t regs_cap = 0, reg_counts_cap = 0, ref_len_cap = 0, mp_up_cap = 0;
	uint32_t *d_rhash = nullptr;
	int32_t *d_rqlen = nullptr;
	int64_t *d_regs_off = nullptr, *d_mp_off_up = nullptr;
	unsigned long long *d_sum_k = nullptr;
	int64_t bot_n_reads = -1, bot_n_chains = 0, bot_n_b = 0;   // what the last chaindp_backtrack left resident (-1: nothing of this batch)
	bool mp_resident = false;                                  // this batch's mini_pos are on the device (it came from chaindp_collect_seeds)
	bool regs_resident = false;      // d_regs / d_rqlen hold what chaindp_gen_regs made of the resident chains (chaindp_est_err's upload clears it)
	// chain_post + mm_set_mapq (allocated on first use, grown with the batch)
	void *d_post_stage = nullptr, *d_post_out = nullptr, *d_post_sq = nullptr, *d_post_scratch = nullptr;
	size_t post_stage_cap = 0, post_out_cap = 0, post_sq_cap = 0, post_scratch_cap = 0;
	unsigned long long *d_post_off = nullptr, *d_post_tile = nullptr;
	int32_t *d_post_qlen = nullptr, *d_post_rep = nullptr, *d_post_err = nullptr;
	uint32_t *d_logf_k = nullptr;
	float *d_logf_v = nullptr;
	int n_logf = 0;
	// reads of several segments: chaindp_frag_post (allocated on first use, grown with the batch)
	void *d_frag_seq = nullptr, *d_frag_cnt = nullptr, *d_frag_u = nullptr, *d_frag_a = nullptr, *d_frag_stage = nullptr, *d_frag_z = nullptr;
	void *d_frag_stacks = nullptr, *d_frag_out = nullptr;
	size_t frag_seq_cap = 0, frag_cnt_cap = 0, frag_u_cap = 0, frag_a_cap = 0, frag_stage_cap = 0, frag_z_cap = 0, frag_stacks_cap = 0, frag_out_cap = 0;
	int frag_lds_cap = FRAG_LDS_CAP;           // chaindp_debug_set_frag_lds_cap (tests): fewer hits per fragment stay in LDS
	// sketch (allocated on first use, grown with the batch)
	chaindp::SketchArgs sk = {};
	int64_t sk_cap_bases = -1, sk_cap_chunks = -1, sk_cap_seqs = -1;
	int64_t sk_max_bases = 0x7fffff00;         // CHAINDP_SKETCH_MAX_BASES (test switch) lowers it; positions and ranks are 32-bit
	unsigned long long *d_sk_totals = nullptr;
	bool sk_valid = false;                     // d_mini / d_mini_off hold what the last chaindp_sketch made
	int64_t sk_n_reads = 0, sk_n_mini = 0;
	int ix_status = 0;                         // code of the last chaindp_index_build (chaindp_index_build_status)
	int64_t ix_chunk_bases = 0;                // chaindp_debug_index_chunk_bases (tests): bases per sketch sub-batch of an index build, 0 = sk_max_bases
	std::vector<int64_t> sk_mini_off;          // its mini_off and the reads' lengths, for the calls that say "the resident ones"
	std::vector<int32_t> sk_qlen;
	std::vector<int32_t> sk_seq_len;           // ... and the lengths of its sequences (the segments of chaindp_frag_post)
	hipEvent_t sk_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the two phases of a sketch while profiling is on (created once)
	double sk_ms = 0;
	int64_t sk_calls = 0;
	// profiling
	bool prof = false;
	std::vector<EventSet> pending;
	double ms[4] = {0, 0, 0, 0};
	int64_t launches[4] = {0, 0, 0, 0};
	int64_t stats[4] = {0, 0, 0, 0};
	std::string err;
};

// (ctx: a context or a pipe)
#define HIP_TRY(ctx, call)                                                                         \
	do {                                                                                           \
		hipError_t e_ = (call);                                                                    \
		if (e_ != hipSuccess) {                                                                    \
			(ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
			return CHAINDP_ERR_HIP;                                                                \
		}                                                                                          \
	} while (0)

using chaindp::dev_buf;

// A first-use group of buffers, all or nothing: an out-of-memory half way leaves the context as it was (what this attempt allocated
// is freed again and the next call tries anew) instead of half-initialised with kernels launched on null scratch pointers.
static int first_use(chaindp_ctx *ctx, bool &ready, const char *what, std::initializer_list<chaindp::DevBuf> bufs)
{
	if (ready) return CHAINDP_OK;
	const hipError_t e = (hipError_t)ctx->pool.alloc_group(bufs);
	if (e != hipSuccess) { ctx->err = std::string(what) + " buffers: " + hipGetErrorString(e); return CHAINDP_ERR_HIP; }
	ready = true;
	return CHAINDP_OK;
}

// grow-only device buffer with a quarter of slack; a failed growth leaves the old buffer and its capacity
static hipError_t dev_grow(chaindp_ctx *ctx, void *&p, size_t &cap, size_t need)
{
	return (hipError_t)ctx->pool.reserve(&p, cap, need, need + need / 4, false);
}

// A new batch is resident (or, with 0 reads, none): what the calls on the one before left is no longer of this batch.
static void begin_batch(chaindp_ctx *ctx, int64_t n_reads, int64_t total, bool mp_resident = false)
{
	ctx->n_reads = n_reads; ctx->total = total; ctx->ran = false; ctx->bot_n_reads = -1; ctx->mp_resident = mp_resident;
}

// the batch's per-read segment counts, if it has any, on the stream that carries its upload
static hipError_t stage_n_segs(chaindp_ctx *ctx, const int32_t *n_segs_per_read, int64_t n_reads, hipStream_t st)
{
	ctx->has_n_segs = n_segs_per_read != nullptr;
	if (!n_segs_per_read || !n_reads) return hipSuccess;
	return hipMemcpyAsync(ctx->d_n_segs, n_segs_per_read, (size_t)n_reads * 4, hipMemcpyHostToDevice, st);
}

// Profiling bracket around a launch: n events at consecutive kernel boundaries, their times added to ms[slot0...].  prof_begin
// records the first, prof_mark the k-th; the last one queues the set for chaindp_get_kernel_ms.  Nothing happens while profiling is off.
static hipError_t prof_begin(chaindp_ctx *ctx, EventSet &es, int n, int slot0, hipStream_t st)
{
	es.n = 0; es.slot0 = slot0;
	if (!ctx->prof) return hipSuccess;
	for (int k = 0; k < n; ++k) if (hipError_t e = hipEventCreate(&es.e[k])) return e;
	es.n = n;
	return hipEventRecord(es.e[0], st);
}

static hipError_t prof_mark(chaindp_ctx *ctx, EventSet &es, int k, hipStream_t st)
{
	if (!es.n) return hipSuccess;
	const hipError_t e = hipEventRecord(es.e[k], st);
	if (e == hipSuccess && k == es.n - 1) ctx->pending.push_back(es);
	return e;
}

static Params to_params(const chaindp_params_t *p)
{
	Params q;
	q.max_dist_x = p->max_dist_x; q.max_dist_y = p->max_dist_y; q.bw = p->bw; q.max_skip = p->max_skip;
	q.min_sc = p->min_sc; q.is_cdna = p->is_cdna; q.n_segs = p->n_segs;
	return q;
}

static int check_params(chaindp_ctx *ctx, const chaindp_params_t *par)
{
	if (!par) { ctx->err = "params is NULL"; return CHAINDP_ERR_ARG; }
	// the reference compares unsigned differences against these after an int -> u64 conversion
	// (chain.c:252); negative values would silently mean "unbounded", refuse them instead
	if (par->max_dist_x < 0 || par->max_dist_y < 0 || par->bw < 0) {
		ctx->err = "max_dist_x, max_dist_y and bw must be >= 0";
		return CHAINDP_ERR_ARG;
	}
	return CHAINDP_OK;
}

extern "C" int chaindp_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" const char *chaindp_last_error(const chaindp_ctx_t *ctx)
{
	return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" void chaindp_destroy(chaindp_ctx_t *ctx)
{
	if (!ctx) return;
	if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	for (auto &es : ctx->pending) for (int k = 0; k < es.n; ++k) (void)hipEventDestroy(es.e[k]);
	ctx->pool.release_all();
	for (hipEvent_t e : ctx->sk_ev) if (e) (void)hipEventDestroy(e);
	if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;
}

extern "C" chaindp_ctx_t *chaindp_create(int device, int64_t max_anchors, int64_t max_reads)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { g_create_error = "no HIP device visible"; return nullptr; }
	if (device < 0 || device >= n_dev || max_anchors < 0 || max_reads < 0 || max_anchors > 0x7fffffff || max_reads > 0x7fffffff) {
		g_create_error = "bad device index or capacity (at most 2^31-1 anchors and reads per batch)";
		return nullptr;
	}
	chaindp_ctx *ctx = new chaindp_ctx();
	ctx->device = device;
	ctx->cap_anchors = max_anchors > 0 ? max_anchors : 1;
	ctx->cap_reads = max_reads > 0 ? max_reads : 1;
	const size_t na = (size_t)ctx->cap_anchors, nr = (size_t)ctx->cap_reads;
	size_t flags_bytes = 0, cblocks_bytes = 0, mask_bytes = 0, blocks_bytes = 0;
	chaindp::compact_scratch_bytes(ctx->cap_anchors, &flags_bytes, &cblocks_bytes);
	chaindp::prepass_scratch_bytes(ctx->cap_anchors, &mask_bytes, &blocks_bytes);
	hipError_t e = hipSetDevice(device);
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
	if (e == hipSuccess) e = (hipError_t)ctx->pool.alloc_group({
		dev_buf(ctx->d_off, (nr + 1) * 8),
		dev_buf(ctx->d_a, na * 16),
		dev_buf(ctx->d_n_segs, nr * 4),
		dev_buf(ctx->d_f, na * 4),
		dev_buf(ctx->d_twin_queue, 8 * 64 * sizeof(unsigned int)),
		dev_buf(ctx->d_p, na * 4),
		dev_buf(ctx->d_v, na * 4),
		dev_buf(ctx->d_tg, na * 8),
		dev_buf(ctx->d_sumq, nr * 8),
		dev_buf(ctx->d_units, (na / 2 + 1) * sizeof(Unit)),
		dev_buf(ctx->d_unit_aux, (na / 2 + 1) * sizeof(chaindp::UnitAux)),
		dev_buf(ctx->d_counters, 2 * sizeof(unsigned long long)),
		dev_buf(ctx->d_left, (na / 2 + 1) * sizeof(Unit)),
		dev_buf(ctx->d_left_cnt, 4 * sizeof(unsigned long long)),
		dev_buf(ctx->d_deep, (na / 64 + 2) * sizeof(Unit)),    // a unit is handed over after its first 64-anchor tile at the earliest (test mode), with anchors to go
		dev_buf(ctx->d_first_child, na * 4),
		dev_buf(ctx->cmp.flags, flags_bytes),
		dev_buf(ctx->pre.start_mask, mask_bytes),
		dev_buf(ctx->pre.single_mask, mask_bytes),
		dev_buf(ctx->pre.emit_mask, mask_bytes),
		dev_buf(ctx->pre.block_cnt, blocks_bytes),
		dev_buf(ctx->pre.tile_tmp, blocks_bytes),
		dev_buf(ctx->pre.units_tmp, (na / 2 + 1) * sizeof(Unit)),
		dev_buf(ctx->pre.hist, (2 * 128 + 2) * sizeof(unsigned int)),
		dev_buf(ctx->pre.block_reads, blocks_bytes)});         // 8 B per block, like the counters
	if (e == hipSuccess) e = hipMemset(ctx->d_tg, 0, na * 8);
	if (e == hipSuccess) {                                     // aliases into the allocations above
		ctx->cmp.single_mask = ctx->pre.single_mask; ctx->cmp.emit_mask = ctx->pre.emit_mask; ctx->cmp.block_reads = ctx->pre.block_reads;
		ctx->pre.key_range = ctx->pre.hist + 2 * 128;
	}
	ctx->use_quad = getenv("CHAINDP_QUAD") != nullptr;
	ctx->deep_handover = getenv("CHAINDP_NO_DEEP_HANDOVER") == nullptr;      // diagnostic switches are read here, once per context:
	if (const char *v = getenv("CHAINDP_TWIN_FORCE_LEFT")) ctx->twin_force_left = atoi(v) == 2 ? 2 : 1;   // never on the launch path (contexts run from several host threads)
	if (const char *v = getenv("CHAINDP_SKETCH_MAX_BASES")) { const long long m = atoll(v); if (m >= 0 && m < ctx->sk_max_bases) ctx->sk_max_bases = m; }
	if (e != hipSuccess) {
		g_create_error = std::string("chaindp_create: ") + hipGetErrorString(e);
		chaindp_destroy(ctx);
		return nullptr;
	}
	return ctx;
}

extern "C" int chaindp_set_ring(chaindp_ctx_t *ctx, int ring)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ring != 128 && ring != 256 && ring != 512) { ctx->err = "ring must be 128, 256 or 512"; return CHAINDP_ERR_ARG; }
	ctx->ring = ring;
	return CHAINDP_OK;
}

extern "C" int chaindp_set_variant(chaindp_ctx_t *ctx, int force_general)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (force_general < 0 || force_general > 2) { ctx->err = "variant must be 0 (two units per wave + the rest), 1 (general) or 2 (one unit per wave)"; return CHAINDP_ERR_ARG; }
	ctx->use_lut = force_general != 1;
	ctx->variant = force_general;
	return CHAINDP_OK;
}

extern "C" int chaindp_set_profiling(chaindp_ctx_t *ctx, int on)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	ctx->prof = on != 0;
	return CHAINDP_OK;
}

// Launch prepass + chain DP on `st` for a batch described by device pointers, using ctx's scratch.
static int run_on_stream(chaindp_ctx *ctx, const chaindp_params_t *par, int64_t n_reads, int64_t total,
                         const int64_t *d_off, const void *d_a, const int32_t *d_n_segs,
                         int32_t *d_f, int32_t *d_p, int32_t *d_v, hipStream_t st)
{
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (n_reads < 0 || total < 0) { ctx->err = "negative batch size"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) {
		ctx->err = "batch exceeds the capacity the context was created with";
		return CHAINDP_ERR_CAPACITY;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const Params q = to_params(par);
	EventSet es;
	HIP_TRY(ctx, prof_begin(ctx, es, 3, 0, st));
	HIP_TRY(ctx, chaindp::launch_prepass(st, q, n_reads, total, d_off, d_a, ctx->d_sumq, ctx->d_units, ctx->d_counters, ctx->pre, ctx->d_unit_aux, d_n_segs, ctx->d_left_cnt));
	HIP_TRY(ctx, prof_mark(ctx, es, 1, st));
	// per-read gap-cost table for the fast variant (skipped when the table would not apply)
	uint16_t *lut = nullptr;
	int lut_stride = 0;
	if (ctx->use_lut && !q.is_cdna && q.bw <= CHAINDP_LUT_MAX_BW && n_reads > 0) {
		lut_stride = (q.bw + 1 + 7) & ~7;
		const size_t need = (size_t)n_reads * lut_stride * sizeof(uint16_t);
		if (need > ctx->lut_bytes) {
			HIP_TRY(ctx, hipStreamSynchronize(st));
			HIP_TRY(ctx, (hipError_t)ctx->pool.reserve((void**)&ctx->d_lut, ctx->lut_bytes, need, need, true));
		}
		lut = ctx->d_lut;
		HIP_TRY(ctx, chaindp::launch_lut(st, q, n_reads, d_off, ctx->d_sumq, lut_stride, lut));
	}
	if (++ctx->epoch == 0) {                                       // 2^32 runs: start the mark epochs over
		HIP_TRY(ctx, hipMemsetAsync(ctx->d_tg, 0, (size_t)ctx->cap_anchors * 8, st));
		ctx->epoch = 1;
	}
	// (d_left_cnt -- hand-over counts and the twin kernel's queue word -- was zeroed by the prepass' first kernel)
	Unit *const deep = ctx->deep_handover ? ctx->d_deep : nullptr;
	unsigned int *const deep_cnt = (unsigned int*)(ctx->d_left_cnt + 1);
	if (ctx->variant == 0 && lut) {
		// ordinary units two per wave; what that kernel hands over (and nothing else) goes through k_chain_units
		// (first_child[] is initialised by the DP kernels themselves, per tile: no batch-wide memset)
		// four units per wave where the whole batch has one cost table, else two per wave: both are launched, the device decides
		unsigned int *const route = (unsigned int*)(ctx->d_left_cnt + 3);
		Params qt = q;                          // with per-read segment counts the units' UnitAux flags say which reads are multi-segment
		if (d_n_segs) qt.n_segs = 1;            // (the batch-wide count is not used then, as in k_chain_units)
		if (ctx->use_quad)
			HIP_TRY(ctx, chaindp::launch_chain_quad(st, qt, total / 2, d_a, lut, lut_stride, ctx->d_units, ctx->d_unit_aux, ctx->d_counters, ctx->pre.key_range,
			                                        d_f, d_p, d_v, ctx->d_first_child, ctx->cmp.flags, ctx->d_left, (unsigned int*)ctx->d_left_cnt,
			                                        (unsigned int*)ctx->d_left_cnt + 1, route, ctx->twin_force_left, total));
		HIP_TRY(ctx, chaindp::launch_chain_twin(st, qt, total / 2, d_off, d_a, ctx->d_sumq, lut, lut_stride, ctx->d_units, ctx->d_counters,
		                                        d_f, d_p, d_v, ctx->d_first_child, ctx->cmp.flags, ctx->d_left, (unsigned int*)ctx->d_left_cnt,
		                                        ctx->twin_force_left, total, ctx->d_unit_aux, ctx->pre.key_range, route, ctx->d_twin_queue,
		                                        ctx->twin_two_tables));
		const int64_t left_grid = total / 2 < 32768 ? total / 2 : 32768;
		HIP_TRY(ctx, chaindp::launch_chain(st, ctx->ring, q, left_grid, d_off, d_a, d_n_segs, ctx->d_sumq, lut, lut_stride, ctx->d_left,
		                                   ctx->d_left_cnt, d_f, d_p, d_v, ctx->d_tg, ctx->epoch, ctx->d_first_child, ctx->cmp.flags,
		                                   ctx->d_units, ctx->d_counters, deep, deep_cnt, ctx->pre.hist + CHAINDP_LONG_UNIT_CLASS, ctx->deep_eager, ctx->deep_route));
	} else
		HIP_TRY(ctx, chaindp::launch_chain(st, ctx->ring, q, total / 2, d_off, d_a, d_n_segs, ctx->d_sumq, lut, lut_stride, ctx->d_units,
		                                   ctx->d_counters, d_f, d_p, d_v, ctx->d_tg, ctx->epoch, ctx->d_first_child, ctx->cmp.flags,
		                                   nullptr, nullptr, deep, deep_cnt, ctx->pre.hist + CHAINDP_LONG_UNIT_CLASS, ctx->deep_eager, ctx->deep_route));
	// units whose scans kept reaching past the ring (dense repeats): redone by k_chain_dense
	if (deep && lut) {
		HIP_TRY(ctx, chaindp::launch_chain_dense(st, q, total / 64 + 1, d_off, d_a, lut, lut_stride, ctx->d_deep, ctx->d_left_cnt + 1,
		                                         d_f, d_p, d_v, ctx->d_first_child, ctx->cmp.flags, ctx->pre.hist + CHAINDP_LONG_UNIT_CLASS, ctx->deep_route,
		                                           (unsigned int*)(ctx->d_left_cnt + 3) + 1));   // (the word behind the route flag: zeroed with it)
		HIP_TRY(ctx, chaindp::launch_chain_dense16(st, q, total / 64 + 1, d_off, d_a, lut, lut_stride, ctx->d_deep, ctx->d_left_cnt + 1,
		                                           d_f, d_p, d_v, ctx->d_first_child, ctx->cmp.flags, ctx->pre.hist + CHAINDP_LONG_UNIT_CLASS, ctx->deep_route,
		                                           (unsigned int*)(ctx->d_left_cnt + 3) + 1));   // (the word behind the route flag: zeroed with it)
		HIP_TRY(ctx, chaindp::launch_chain_dense1(st, q, total / 64 + 1, d_off, d_a, lut, lut_stride, ctx->d_deep, ctx->d_left_cnt + 1,
		                                          ctx->pre.hist + CHAINDP_LONG_UNIT_CLASS, ctx->deep_route, (unsigned int*)(ctx->d_left_cnt + 2), d_f, d_p, d_v, ctx->d_first_child, ctx->cmp.flags));
	}
	HIP_TRY(ctx, prof_mark(ctx, es, 2, st));
	ctx->stats[2] = total; ctx->stats[3] = n_reads;
	return CHAINDP_OK;
}

extern "C" int chaindp_upload(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *off, const chaindp_anchor_t *a,
                              const int32_t *n_segs_per_read)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n_reads < 0 || !off || (n_reads > 0 && off[0] != 0)) { ctx->err = "bad offsets"; return CHAINDP_ERR_ARG; }
	const int64_t total = n_reads > 0 ? off[n_reads] : 0;
	if (total < 0 || (total > 0 && !a)) { ctx->err = "bad anchors"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) {
		ctx->err = "batch exceeds the capacity the context was created with";
		return CHAINDP_ERR_CAPACITY;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
	if (total) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_a, a, (size_t)total * 16, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, stage_n_segs(ctx, n_segs_per_read, n_reads, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	begin_batch(ctx, n_reads, total);
	return CHAINDP_OK;
}

extern "C" int chaindp_run(chaindp_ctx_t *ctx, const chaindp_params_t *par)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = run_on_stream(ctx, par, ctx->n_reads, ctx->total, ctx->d_off, ctx->d_a, ctx->has_n_segs ? ctx->d_n_segs : nullptr,
	                       ctx->d_f, ctx->d_p, ctx->d_v, ctx->stream);
	if (rc == CHAINDP_OK) { ctx->ran = true; ctx->singles_pending = true; ctx->ran_par = *par; }
	return rc;
}

extern "C" int chaindp_run_device(chaindp_ctx_t *ctx, const chaindp_params_t *par, int64_t n_reads, int64_t total_anchors,
                                  const void *d_off, const void *d_a, const void *d_n_segs,
                                  void *d_f, void *d_p, void *d_v, void *stream)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!d_off || (total_anchors > 0 && (!d_a || !d_f || !d_p || !d_v))) { ctx->err = "NULL device pointer"; return CHAINDP_ERR_ARG; }
	hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
	const int rc = run_on_stream(ctx, par, n_reads, total_anchors, (const int64_t*)d_off, d_a, (const int32_t*)d_n_segs,
	                             (int32_t*)d_f, (int32_t*)d_p, (int32_t*)d_v, st);
	if (rc != CHAINDP_OK) return rc;
	// the caller reads its own arrays: the singletons' entries are written right away
	HIP_TRY(ctx, chaindp::launch_fill_singles(st, to_params(par), total_anchors, d_a, ctx->pre, (int32_t*)d_f, (int32_t*)d_p, (int32_t*)d_v, ctx->cmp.flags));
	return CHAINDP_OK;
}

extern "C" int chaindp_sync(chaindp_ctx_t *ctx)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_download(chaindp_ctx_t *ctx, int32_t *f, int32_t *p, int32_t *v)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!ctx->ran) { ctx->err = "chaindp_download before chaindp_run"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t bytes = (size_t)ctx->total * 4;
	if (ctx->singles_pending) {          // (the compaction works from the prepass' masks: only this call looks at the singletons' f, p, v)
		HIP_TRY(ctx, chaindp::launch_fill_singles(ctx->stream, to_params(&ctx->ran_par), ctx->total, ctx->d_a, ctx->pre, ctx->d_f, ctx->d_p, ctx->d_v, ctx->cmp.flags));
		ctx->singles_pending = false;
	}
	if (bytes) {
		if (f) HIP_TRY(ctx, hipMemcpyAsync(f, ctx->d_f, bytes, hipMemcpyDeviceToHost, ctx->stream));
		if (p) HIP_TRY(ctx, hipMemcpyAsync(p, ctx->d_p, bytes, hipMemcpyDeviceToHost, ctx->stream));
		if (v) HIP_TRY(ctx, hipMemcpyAsync(v, ctx->d_v, bytes, hipMemcpyDeviceToHost, ctx->stream));
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_chain_batch(chaindp_ctx_t *ctx, const chaindp_params_t *par, int64_t n_reads, const int64_t *off,
                                   const chaindp_anchor_t *a, const int32_t *n_segs_per_read,
                                   int32_t *f, int32_t *p, int32_t *v)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if ((rc = chaindp_upload(ctx, n_reads, off, a, n_segs_per_read)) != CHAINDP_OK) return rc;
	if ((rc = chaindp_run(ctx, par)) != CHAINDP_OK) return rc;
	return chaindp_download(ctx, f, p, v);
}

// launches the compaction kernels on the context's stream (asynchronous)
static int compact_launch(chaindp_ctx *ctx, const chaindp_params_t *par)
{
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!ctx->ran) { ctx->err = "compaction before chaindp_run"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t na = (size_t)ctx->cap_anchors, nr = (size_t)ctx->cap_reads;
	size_t flags_bytes = 0, blocks_bytes = 0;
	chaindp::compact_scratch_bytes(ctx->cap_anchors, &flags_bytes, &blocks_bytes);
	// d_seeds is the only slot of any group that may be filled before its group's first use (collect_seeds_impl makes it when it runs
	// first): alloc_group keeps a filled slot, and a rollback frees only what this attempt allocated.  Every other slot is null here.
	rc = first_use(ctx, ctx->compact_ready, "compaction", {
		dev_buf(ctx->d_seeds_off, (nr + 1) * 8), dev_buf(ctx->d_seeds, na * sizeof(chaindp_seed_t) + 16),
		dev_buf(ctx->cmp.block_cnt, blocks_bytes), dev_buf(ctx->cmp.tile_tmp, blocks_bytes), dev_buf(ctx->cmp.n_seeds, 8), dev_buf(ctx->cmp.sub, blocks_bytes * 32)});
	if (rc) return rc;
	EventSet es;
	HIP_TRY(ctx, prof_begin(ctx, es, 2, 2, ctx->stream));
	HIP_TRY(ctx, chaindp::launch_compact(ctx->stream, to_params(par), ctx->n_reads, ctx->total, ctx->d_off, ctx->d_a, ctx->d_f, ctx->d_p,
	                                     ctx->d_v, ctx->d_first_child, ctx->d_seeds_off, ctx->d_seeds, ctx->cmp));
	HIP_TRY(ctx, prof_mark(ctx, es, 1, ctx->stream));
	return CHAINDP_OK;
}

static int compact_on_device(chaindp_ctx *ctx, const chaindp_params_t *par, int64_t *seeds_off)
{
	if (!seeds_off) { ctx->err = "NULL output"; return CHAINDP_ERR_ARG; }
	int rc = compact_launch(ctx, par);
	if (rc) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(seeds_off, ctx->d_seeds_off, (size_t)(ctx->n_reads + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->n_seeds = seeds_off[ctx->n_reads];
	return CHAINDP_OK;
}

extern "C" int chaindp_backtrack(chaindp_ctx_t *ctx, const chaindp_params_t *par, int min_cnt,
                                 int64_t *chains_off, uint64_t *u, int64_t *b_off, chaindp_anchor_t *b)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!ctx->ran || !ctx->d_seeds) { ctx->err = "chaindp_backtrack needs a completed run and compaction"; return CHAINDP_ERR_ARG; }
	if (!chains_off || !b_off) { ctx->err = "NULL output"; return CHAINDP_ERR_ARG; }
	ctx->regs_resident = false;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the record count of the last compaction (it may have been launched asynchronously by chaindp_run_full)
	unsigned long long n_seeds = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&n_seeds, ctx->cmp.n_seeds, 8, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const int64_t m = ctx->total > 0 && ctx->n_reads > 0 ? (int64_t)(uint32_t)n_seeds : 0;
	ctx->n_seeds = m;
	const size_t M = (size_t)ctx->cap_anchors, R = (size_t)ctx->cap_reads, NB = M / 1024 + 2, NS = (NB > R + 2 ? NB : R + 2) * 8;
	chaindp::BottomScratch &s = ctx->bot;
	rc = first_use(ctx, ctx->bot_ready, "backtrack", {
		dev_buf(s.has, M),
		dev_buf(s.owner, M * 4), dev_buf(s.end_rec, M * 4), dev_buf(s.ccnt, M * 4), dev_buf(s.kpos, M * 4), dev_buf(s.bpos, M * 4),
		dev_buf(s.c_src, M * 4), dev_buf(s.c_dst, M * 4),
		dev_buf(s.key, M * 8), dev_buf(s.skey, M * 8), dev_buf(s.cu, M * 8), dev_buf(s.u_tmp, M * 8), dev_buf(s.u_out, M * 8),
		dev_buf(s.b_tmp, M * 16), dev_buf(s.b_out, M * 16), dev_buf(s.w, M * 16),
		dev_buf(s.stacks, (M / 64 + 2 * R + 4) * 12),
		dev_buf(s.block_cnt, NS), dev_buf(s.tile_tmp, NS),
		dev_buf(s.read_tot, (R + 2) * 8), dev_buf(s.total, 8),
		dev_buf(s.ends_off, (R + 2) * 8), dev_buf(s.chains_off, (R + 2) * 8), dev_buf(s.b_off, (R + 2) * 8)});
	if (rc) return rc;
	EventSet es;
	HIP_TRY(ctx, prof_begin(ctx, es, 2, 3, ctx->stream));
	HIP_TRY(ctx, chaindp::launch_backtrack(ctx->stream, min_cnt, par->min_sc, ctx->n_reads, ctx->cap_anchors, ctx->d_seeds_off, ctx->d_seeds,
	                                       ctx->cmp.n_seeds, ctx->bot, m));
	HIP_TRY(ctx, prof_mark(ctx, es, 1, ctx->stream));
	const size_t ob = (size_t)(ctx->n_reads > 0 ? ctx->n_reads + 1 : 1) * 8;
	HIP_TRY(ctx, hipMemcpyAsync(chains_off, ctx->bot.chains_off, ob, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(b_off, ctx->bot.b_off, ob, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const int64_t n_c = ctx->n_reads > 0 ? chains_off[ctx->n_reads] : 0, n_b = ctx->n_reads > 0 ? b_off[ctx->n_reads] : 0;
	ctx->bot_n_reads = ctx->n_reads; ctx->bot_n_chains = n_c; ctx->bot_n_b = n_b;
	if (u && n_c > 0) HIP_TRY(ctx, hipMemcpyAsync(u, ctx->bot.u_out, (size_t)n_c * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (b && n_b > 0) HIP_TRY(ctx, hipMemcpyAsync(b, ctx->bot.b_out, (size_t)n_b * 16, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

// per-read arrays of the hit stages
static int regs_per_read_buffers(chaindp_ctx *ctx)
{
	const size_t R = (size_t)ctx->cap_reads + 2;
	return first_use(ctx, ctx->regs_ready, "hit", {dev_buf(ctx->d_rhash, R * 4), dev_buf(ctx->d_rqlen, R * 4), dev_buf(ctx->d_regs_off, R * 8),
	                                               dev_buf(ctx->d_mp_off_up, R * 8), dev_buf(ctx->d_sum_k, R * 8)});
}

// mini_pos[] of the batch for mm_est_err: the caller's arrays or, with both NULL, what chaindp_collect_seeds left resident.
// mini_pos_check is the argument check (no device work); stage_mini_pos uploads the caller's arrays and the targets' lengths,
// growing their buffers, and returns the offsets and positions the kernel reads.
static int mini_pos_check(chaindp_ctx *ctx, const int64_t *mini_pos_off, const uint64_t *mini_pos)
{
	const bool resident = mini_pos == nullptr && mini_pos_off == nullptr;
	if (resident && (!ctx->mp_resident || !ctx->d_mp_off)) { ctx->err = "no resident mini_pos: pass the arrays, or collect the seeds with chaindp_collect_seeds"; return CHAINDP_ERR_ARG; }
	if (!resident && !mini_pos_off) { ctx->err = "mini_pos without offsets"; return CHAINDP_ERR_ARG; }
	return CHAINDP_OK;
}

static int stage_mini_pos(chaindp_ctx *ctx, int64_t R, const int64_t *mini_pos_off, const uint64_t *mini_pos, const int32_t *ref_len, int32_t n_ref,
                          const int64_t *&d_mpo, const unsigned long long *&d_mp)
{
	hipStream_t st = ctx->stream;
	d_mpo = ctx->d_mp_off; d_mp = ctx->d_mini_pos;
	if (mini_pos || mini_pos_off) {
		const int64_t n_mp = mini_pos_off[R];
		if (n_mp < 0 || (n_mp > 0 && !mini_pos)) { ctx->err = "mini_pos announced but absent"; return CHAINDP_ERR_ARG; }
		HIP_TRY(ctx, dev_grow(ctx, ctx->d_mp_up, ctx->mp_up_cap, (size_t)(n_mp > 0 ? n_mp : 1) * 8));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mp_off_up, mini_pos_off, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, st));
		if (n_mp > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mp_up, mini_pos, (size_t)n_mp * 8, hipMemcpyHostToDevice, st));
		d_mpo = ctx->d_mp_off_up; d_mp = (const unsigned long long*)ctx->d_mp_up;
	}
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_ref_len, ctx->ref_len_cap, (size_t)(n_ref > 0 ? n_ref : 1) * 4));
	if (n_ref > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ref_len, ref_len, (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
	return CHAINDP_OK;
}

// download = false: the hits stay in HBM only (chaindp_map_reads)
static int gen_regs_impl(chaindp_ctx *ctx, const uint32_t *hash, const int32_t *qlen, chaindp_reg_t *regs, bool download)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has) { ctx->err = "chaindp_gen_regs needs the chains of a chaindp_backtrack on this batch"; return CHAINDP_ERR_ARG; }
	const int64_t R = ctx->bot_n_reads, n_c = ctx->bot_n_chains;
	if (R > 0 && (!hash || !qlen)) { ctx->err = "NULL hash or qlen"; return CHAINDP_ERR_ARG; }
	if (download && n_c > 0 && !regs) { ctx->err = "NULL output"; return CHAINDP_ERR_ARG; }
	ctx->regs_resident = false;
	if (R == 0 || n_c == 0) { ctx->regs_resident = true; return CHAINDP_OK; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = regs_per_read_buffers(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_regs, ctx->regs_cap, (size_t)n_c * sizeof(chaindp_reg_t)));
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rhash, hash, (size_t)R * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rqlen, qlen, (size_t)R * 4, hipMemcpyHostToDevice, st));
	// sort keys go to the backtrack's 16-byte scratch (free once the chains are out), range stacks to its stack area
	HIP_TRY(ctx, chaindp::launch_gen_regs(st, R, ctx->bot.chains_off, ctx->bot.b_off, ctx->bot.u_out, ctx->bot.b_out, ctx->d_rhash, ctx->d_rqlen,
	                                      ctx->bot.w, ctx->bot.stacks, ctx->d_regs));
	if (download) HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->d_regs, (size_t)n_c * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	ctx->regs_resident = true;
	return CHAINDP_OK;
}

extern "C" int chaindp_gen_regs(chaindp_ctx_t *ctx, const uint32_t *hash, const int32_t *qlen, chaindp_reg_t *regs)
{
	return gen_regs_impl(ctx, hash, qlen, regs, true);
}

extern "C" int chaindp_est_err(chaindp_ctx_t *ctx, const int64_t *regs_off, chaindp_reg_t *regs, const int32_t *qlen,
                               const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                               int32_t *match_tot)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has) { ctx->err = "chaindp_est_err needs the chains of a chaindp_backtrack on this batch"; return CHAINDP_ERR_ARG; }
	const int64_t R = ctx->bot_n_reads;
	if (R == 0) return CHAINDP_OK;
	if (!regs_off || !qlen || (n_ref > 0 && !ref_len) || n_ref < 0) { ctx->err = "NULL argument"; return CHAINDP_ERR_ARG; }
	if (regs_off[0] != 0) { ctx->err = "regs_off must start at 0"; return CHAINDP_ERR_ARG; }
	for (int64_t r = 0; r < R; ++r) if (regs_off[r + 1] < regs_off[r]) { ctx->err = "regs_off must not decrease"; return CHAINDP_ERR_ARG; }
	const int64_t n_regs = regs_off[R];
	if (n_regs == 0) return CHAINDP_OK;
	if (!regs) { ctx->err = "NULL regs"; return CHAINDP_ERR_ARG; }
	int rc = mini_pos_check(ctx, mini_pos_off, mini_pos);
	if (rc) return rc;
	for (int64_t g = 0; g < n_regs; ++g) if (regs[g].cnt < 0 || regs[g].as < 0) { ctx->err = "hit with a negative count or offset"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if ((rc = regs_per_read_buffers(ctx)) != CHAINDP_OK) return rc;
	hipStream_t st = ctx->stream;
	ctx->regs_resident = false;                                  // the upload below replaces what chaindp_gen_regs left in d_regs / d_rqlen
	// every hit's anchors must lie inside its read's chain anchors: checked here, on the host's copy of the offsets
	{
		std::vector<int64_t> boff((size_t)R + 1);
		HIP_TRY(ctx, hipMemcpyAsync(boff.data(), ctx->bot.b_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		for (int64_t r = 0; r < R; ++r)
			for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g)
				if ((int64_t)regs[g].as + regs[g].cnt > boff[r + 1] - boff[r]) { ctx->err = "hit reaches beyond its read's chain anchors"; return CHAINDP_ERR_ARG; }
	}
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_regs, ctx->regs_cap, (size_t)n_regs * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_reg_counts, ctx->reg_counts_cap, (size_t)n_regs * 8));
	const int64_t *d_mpo = nullptr;
	const unsigned long long *d_mp = nullptr;
	if ((rc = stage_mini_pos(ctx, R, mini_pos_off, mini_pos, ref_len, n_ref, d_mpo, d_mp)) != CHAINDP_OK) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_regs_off, regs_off, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rqlen, qlen, (size_t)R * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_regs, regs, (size_t)n_regs * sizeof(chaindp_reg_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, chaindp::launch_est_err(st, R, n_regs, ctx->d_regs_off, ctx->bot.b_off, ctx->bot.b_out, ctx->d_rqlen, (const int32_t*)ctx->d_ref_len, n_ref,
	                                     d_mpo, d_mp, ctx->d_sum_k, ctx->d_regs, (int32_t*)ctx->d_reg_counts));
	HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->d_regs, (size_t)n_regs * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	if (match_tot) HIP_TRY(ctx, hipMemcpyAsync(match_tot, ctx->d_reg_counts, (size_t)n_regs * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	return CHAINDP_OK;
}

// test hook (not in the public header): units the two-per-wave kernel handed over to k_chain_units in the last run.  When that
// kernel declines the whole batch (long units: map-ont, dense repeats) the word on the device is the marker 0xffffffff, "every
// unit": reported as the batch's unit count
extern "C" int64_t chaindp_debug_leftover(chaindp_ctx_t *ctx)
{
	if (!ctx || !ctx->d_left_cnt) return -1;
	unsigned long long c = 0, cnt = 0;
	if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipMemcpy(&c, ctx->d_left_cnt, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(&cnt, ctx->d_counters, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (uint32_t)c == 0xffffffffu ? (int64_t)(uint32_t)cnt : (int64_t)(uint32_t)c;
}

// test hook (not in the public header): 1 lets k_chain_quad take the batches it can (one cost table, ordinary units), 0 (default) never
extern "C" int chaindp_debug_set_quad(chaindp_ctx_t *ctx, int on)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	ctx->use_quad = on != 0;
	return CHAINDP_OK;
}

// test hook (not in the public header): 1 if k_chain_quad took the last batch
extern "C" int chaindp_debug_quad_took(chaindp_ctx_t *ctx)
{
	if (!ctx || !ctx->d_left_cnt) return -1;
	unsigned long long r = 0;
	if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipMemcpy(&r, ctx->d_left_cnt + 3, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (uint32_t)r == 1u;
}

// test hook (not in the public header): 1 keeps k_chain_twin on its layout with a cost table per half even where the batch has one
// table key (which otherwise takes the layout with one table per wave); 0 (default) lets the device decide
extern "C" int chaindp_debug_set_twin_tables(chaindp_ctx_t *ctx, int two)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	ctx->twin_two_tables = two != 0;
	return CHAINDP_OK;
}

// test hook (not in the public header; no GPU needed): k_chain_twin's LDS bytes per workgroup with one cost table per wave (one_table
// != 0) or one per half, and the most workgroups per CU its launch asks for (samegap: max_dist_y >= max_dist_x)
extern "C" int64_t chaindp_debug_twin_lds_bytes(int one_table) { return (int64_t)chaindp::twin_lds_bytes(one_table != 0); }
extern "C" int chaindp_debug_twin_max_wg_per_cu(int samegap, int one_table) { return chaindp::twin_max_wg_per_cu(samegap != 0, one_table != 0); }

// test hook (not in the public header): which layout k_chain_twin ran the last batch with -- 1 one cost table per wave, 2 one per
// half, 0 neither (k_chain_quad took the batch, or the twin kernel declined it as a whole)
extern "C" int chaindp_debug_twin_tables(chaindp_ctx_t *ctx)
{
	if (!ctx || !ctx->d_left_cnt) return -1;
	unsigned long long r = 0;
	if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipMemcpy(&r, ctx->d_left_cnt + 3, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (uint32_t)r == 2u ? 1 : (uint32_t)r == 3u ? 2 : 0;
}

// test hook (not in the public header): what k_chain_twin hands over whatever the units look like -- 0 nothing extra, 1 every unit
// untouched, 2 every unit after its first 64-anchor tile (k_chain_units resumes behind it)
extern "C" int chaindp_debug_set_twin_handover(chaindp_ctx_t *ctx, int mode)
{
	if (!ctx || mode < 0 || mode > 2) return CHAINDP_ERR_ARG;
	ctx->twin_force_left = mode;
	return CHAINDP_OK;
}

// test hook (not in the public header): 0 keeps every unit in the launch that took it (the deep path of the small rings stays
// covered by the parity tests), 1 (default) hands long units whose scans keep reaching past the ring to k_chain_dense or, when the
// batch is dense all over, k_chain_dense1; 2 any unit with a few such scans, to k_chain_dense; 3 the same to k_chain_dense1; 4 the same
// to k_chain_dense16 (small test inputs reach every kernel)
extern "C" int chaindp_debug_set_deep_handover(chaindp_ctx_t *ctx, int on)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	ctx->deep_handover = on != 0;
	ctx->deep_eager = on >= 2;
	ctx->deep_route = on == 2 ? 1 : on == 3 ? 2 : on == 4 ? 3 : 0;
	return CHAINDP_OK;
}

// test hook (not in the public header): units k_chain_units handed over to k_chain_dense in the last run
extern "C" int64_t chaindp_debug_deep_units(chaindp_ctx_t *ctx)
{
	if (!ctx || !ctx->d_left_cnt) return -1;
	unsigned long long c = 0;
	if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipMemcpy(&c, ctx->d_left_cnt + 1, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (int64_t)(uint32_t)c;
}

// test hook (not in the public header): bytes of device memory the context owns at this moment
extern "C" int64_t chaindp_debug_device_bytes(chaindp_ctx_t *ctx) { return ctx ? (int64_t)ctx->pool.bytes() : -1; }

// test hook (not in the public header; read-only): how the last seed collection was routed -- out[0..2] = the limits the context
// settled on when its first collection reached the sort (max_n, max_n2: the largest reads the two configurations of the LDS sort take;
// lab_cap: digits k_seed_sort_huge keeps in LDS; -1 / -1 / 0 before that), out[3] = buckets k_seed_sort_huge handed to the LDS sort as
// work items, out[4] = units (reads and work items) with equal x that went through the reference's procedure in the second launch.
// The two counts are 0 where the last collection launched no sort (no reads, an error before the sort, no collection yet).
extern "C" int chaindp_debug_seed_route(chaindp_ctx_t *ctx, int64_t out[5])
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!out) { ctx->err = "chaindp_debug_seed_route: no output array"; return CHAINDP_ERR_ARG; }
	unsigned long long c[2] = {0, 0};
	if (ctx->seed_route_valid && ctx->seed.totals) {
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		HIP_TRY(ctx, hipMemcpy(c, ctx->seed.totals + 2, sizeof(c), hipMemcpyDeviceToHost));
	}
	out[0] = ctx->seed_max_n; out[1] = ctx->seed_max_n2; out[2] = ctx->seed_lab_cap;
	out[3] = (int64_t)c[0]; out[4] = (int64_t)c[1];
	return CHAINDP_OK;
}

// test hook (not in the public header): copies one of the backtrack scratch arrays to the host
extern "C" int chaindp_debug_bottom(chaindp_ctx_t *ctx, int which, void *dst, size_t bytes)
{
	if (!ctx || !ctx->bot.has) return CHAINDP_ERR_ARG;
	const void *src = nullptr;
	switch (which) {
	case 0: src = ctx->bot.has; break;
	case 1: src = ctx->bot.owner; break;
	case 2: src = ctx->bot.skey; break;
	case 3: src = ctx->bot.ccnt; break;
	case 4: src = ctx->bot.key; break;
	case 5: src = ctx->bot.end_rec; break;
	case 6: src = ctx->bot.ends_off; break;
	case 7: src = ctx->d_regs; break;           // what chaindp_gen_regs left resident
	case 8: src = ctx->bot.u_out; break;
	case 9: src = ctx->bot.b_out; break;
	default: return CHAINDP_ERR_ARG;
	}
	if (!src || !dst) return CHAINDP_ERR_ARG;   // bot.has exists before any chaindp_gen_regs has run
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
	return CHAINDP_OK;
}

extern "C" int chaindp_run_full(chaindp_ctx_t *ctx, const chaindp_params_t *par)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = chaindp_run(ctx, par);
	if (rc) return rc;
	return compact_launch(ctx, par);
}

extern "C" int chaindp_compact_offsets(chaindp_ctx_t *ctx, const chaindp_params_t *par, int64_t *seeds_off)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	return compact_on_device(ctx, par, seeds_off);
}

extern "C" int chaindp_download_seeds(chaindp_ctx_t *ctx, int64_t first_seed, int64_t n_seeds, chaindp_seed_t *dst)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (first_seed < 0 || n_seeds < 0 || first_seed + n_seeds > ctx->n_seeds || (n_seeds > 0 && !dst)) {
		ctx->err = "seed range outside the last compaction";
		return CHAINDP_ERR_ARG;
	}
	if (n_seeds == 0) return CHAINDP_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(dst, (const chaindp_seed_t*)ctx->d_seeds + first_seed, (size_t)n_seeds * sizeof(chaindp_seed_t),
	                            hipMemcpyDeviceToHost, ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_compact(chaindp_ctx_t *ctx, const chaindp_params_t *par, int64_t *seeds_off, chaindp_seed_t *seeds)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ctx->total > 0 && !seeds) { ctx->err = "NULL output"; return CHAINDP_ERR_ARG; }
	int rc = compact_on_device(ctx, par, seeds_off);
	if (rc) return rc;
	if ((rc = chaindp_download_seeds(ctx, 0, ctx->n_seeds, seeds)) != CHAINDP_OK) return rc;
	return chaindp_sync(ctx);
}

// device array of n_reads host pointers (grown on demand)
static int stage_pointers(chaindp_ctx *ctx, const void *const *ptrs, int64_t n)
{
	if ((size_t)n * sizeof(void*) > ctx->ptr_bytes) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		const size_t cap = (size_t)n + (size_t)n / 2 + 64;
		HIP_TRY(ctx, (hipError_t)ctx->pool.reserve((void**)&ctx->d_ptrs, ctx->ptr_bytes, (size_t)n * sizeof(void*), cap * sizeof(void*), true));
	}
	if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ptrs, ptrs, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_upload_gather_ex(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *off,
                                        const chaindp_anchor_t *const *read_anchors, const int32_t *n_segs_per_read, int pinned)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!pinned) return chaindp_upload_gather(ctx, n_reads, off, read_anchors, n_segs_per_read);
	if (n_reads < 0 || !off || (n_reads > 0 && (off[0] != 0 || !read_anchors))) { ctx->err = "bad offsets"; return CHAINDP_ERR_ARG; }
	const int64_t total = n_reads > 0 ? off[n_reads] : 0;
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) {
		ctx->err = "batch exceeds the capacity the context was created with";
		return CHAINDP_ERR_CAPACITY;
	}
	for (int64_t r = 0; r < n_reads; ++r)
		if (off[r + 1] < off[r] || (off[r + 1] > off[r] && !read_anchors[r])) { ctx->err = "bad read in gather list"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
	int rc = stage_pointers(ctx, (const void *const *)read_anchors, n_reads);
	if (rc) return rc;
	HIP_TRY(ctx, chaindp::launch_gather_reads(ctx->stream, n_reads, ctx->d_off, (const void *const *)ctx->d_ptrs, ctx->d_a));
	HIP_TRY(ctx, stage_n_segs(ctx, n_segs_per_read, n_reads, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));       // the host arrays (off, pointers) may go away after the call
	begin_batch(ctx, n_reads, total);
	return CHAINDP_OK;
}

extern "C" int chaindp_scatter_seeds(chaindp_ctx_t *ctx, int64_t n_reads, chaindp_seed_t *const *dst)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n_reads != ctx->n_reads || (n_reads > 0 && !dst) || !ctx->d_seeds) { ctx->err = "scatter does not match the last compaction"; return CHAINDP_ERR_ARG; }
	for (int64_t r = 0; r < n_reads; ++r) if ((uintptr_t)dst[r] & 15u) { ctx->err = "scatter destinations must be 16-byte aligned"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = stage_pointers(ctx, (const void *const *)dst, n_reads);
	if (rc) return rc;
	HIP_TRY(ctx, chaindp::launch_scatter_seeds(ctx->stream, n_reads, ctx->d_seeds_off, (void *const *)ctx->d_ptrs, ctx->d_seeds));
	return CHAINDP_OK;
}

extern "C" int chaindp_upload_gather(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *off,
                                     const chaindp_anchor_t *const *read_anchors, const int32_t *n_segs_per_read)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n_reads < 0 || !off || (n_reads > 0 && (off[0] != 0 || !read_anchors))) { ctx->err = "bad offsets"; return CHAINDP_ERR_ARG; }
	const int64_t total = n_reads > 0 ? off[n_reads] : 0;
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) {
		ctx->err = "batch exceeds the capacity the context was created with";
		return CHAINDP_ERR_CAPACITY;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
	for (int64_t r = 0; r < n_reads; ++r) {
		const int64_t n = off[r + 1] - off[r];
		if (n < 0 || (n > 0 && !read_anchors[r])) { ctx->err = "bad read in gather list"; return CHAINDP_ERR_ARG; }
		if (n) HIP_TRY(ctx, hipMemcpyAsync((chaindp_anchor_t*)ctx->d_a + off[r], read_anchors[r], (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
	}
	HIP_TRY(ctx, stage_n_segs(ctx, n_segs_per_read, n_reads, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	begin_batch(ctx, n_reads, total);
	return CHAINDP_OK;
}

extern "C" void *chaindp_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
	return p;
}

extern "C" void chaindp_host_free(void *p)
{
	if (p) (void)hipHostFree(p);
}

extern "C" int chaindp_get_kernel_ms(chaindp_ctx_t *ctx, double ms[4], int64_t launches[4], int reset)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	for (auto &es : ctx->pending) {
		HIP_TRY(ctx, hipEventSynchronize(es.e[es.n - 1]));
		for (int k = 0; k + 1 < es.n; ++k) {
			float t = 0;
			HIP_TRY(ctx, hipEventElapsedTime(&t, es.e[k], es.e[k + 1]));
			ctx->ms[es.slot0 + k] += (double)t;
			ctx->launches[es.slot0 + k] += 1;
		}
		for (int k = 0; k < es.n; ++k) (void)hipEventDestroy(es.e[k]);
	}
	ctx->pending.clear();
	for (int k = 0; k < 4; ++k) { if (ms) ms[k] = ctx->ms[k]; if (launches) launches[k] = ctx->launches[k]; }
	if (reset) for (int k = 0; k < 4; ++k) { ctx->ms[k] = 0; ctx->launches[k] = 0; }
	return CHAINDP_OK;
}

extern "C" int chaindp_get_stats(chaindp_ctx_t *ctx, int64_t st[4])
{
	if (!ctx || !st) return CHAINDP_ERR_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	unsigned long long c = 0;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	HIP_TRY(ctx, hipMemcpy(&c, ctx->d_counters, sizeof(c), hipMemcpyDeviceToHost));
	ctx->stats[0] = (int64_t)(c & 0xffffffffull); ctx->stats[1] = (int64_t)(c >> 32);
	for (int k = 0; k < 4; ++k) st[k] = ctx->stats[k];
	return CHAINDP_OK;
}

// ---- seed collection on the GPU (chaindp_seed.hip)

struct chaindp_index {
	int device = -1;
	uint8_t *blob[4] = {nullptr, nullptr, nullptr, nullptr};
	size_t bytes[4] = {0, 0, 0, 0};
	int b_bits = 0;
	bool built = false;              // made by chaindp_index_build / chaindp_debug_index_from_minimizers
	int64_t route[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // what the build did (chaindp_debug_index_route)
	double stage_ms[4] = {0, 0, 0, 0};             // sketch sub-batches with their uploads (host clock); sort, grouping, tables (device, events)
};

extern "C" chaindp_index_t *chaindp_index_create(int device, const void *B, size_t nB, const void *H, size_t nH,
                                                 const void *V, size_t nV, const void *P, size_t nP)
{
	g_create_error.clear();
	if (!B || nB < 16 || !H || !V) { g_create_error = "chaindp_index_create: the image needs its B, H and V blobs"; return nullptr; }
	if (hipSetDevice(device) != hipSuccess) { g_create_error = "chaindp_index_create: no such HIP device (there is no CPU fallback)"; return nullptr; }
	chaindp_index *ix = new chaindp_index();
	ix->device = device;
	const void *src[4] = {B, H, V, P};
	const size_t nb[4] = {nB, nH, nV, nP};
	for (int k = 0; k < 4; ++k) {
		ix->bytes[k] = nb[k];
		const size_t alloc = (nb[k] + 63) & ~(size_t)63;                 // the kernels read whole 64-byte groups
		if (hipMalloc((void**)&ix->blob[k], alloc ? alloc : 64) != hipSuccess ||
		    hipMemset(ix->blob[k], 0, alloc ? alloc : 64) != hipSuccess ||
		    (nb[k] && hipMemcpy(ix->blob[k], src[k], nb[k], hipMemcpyHostToDevice) != hipSuccess)) {
			g_create_error = "chaindp_index_create: out of device memory";
			chaindp_index_destroy(ix);
			return nullptr;
		}
	}
	size_t entries = nB / 16;
	while ((size_t)2 << ix->b_bits <= entries) ++ix->b_bits;          // one 16-byte entry per bucket, 2^b buckets
	return ix;
}

extern "C" void chaindp_index_destroy(chaindp_index_t *ix)
{
	if (!ix) return;
	if (ix->device >= 0) (void)hipSetDevice(ix->device);
	for (int k = 0; k < 4; ++k) if (ix->blob[k]) (void)hipFree(ix->blob[k]);
	delete ix;
}

// oom_is_capacity: a failed allocation of the per-minimizer buffers is reported as CHAINDP_ERR_CAPACITY (chaindp_sketch's contract)
// with every one of them released, so that the next call starts from nothing
static int seed_reserve(chaindp_ctx *ctx, int64_t n_mini, bool oom_is_capacity = false)
{
	const size_t nr = (size_t)ctx->cap_reads;
	const size_t stack_bytes = ((size_t)ctx->cap_anchors / 64 + 2 * nr + 4) * 12, tied_bytes = ((size_t)ctx->cap_anchors / 64 + nr + 8) * 4;
	const int rc = first_use(ctx, ctx->seed_ready, "seed collection", {
		dev_buf(ctx->d_mini_off, (nr + 1) * 8), dev_buf(ctx->d_mp_off, (nr + 1) * 8), dev_buf(ctx->d_bid, (nr + 1) * 4), dev_buf(ctx->d_qlen, (nr + 1) * 4),
		dev_buf(ctx->d_rep_len, (nr + 1) * 4), dev_buf(ctx->seed.totals, 32), dev_buf(ctx->seed.stacks, stack_bytes + tied_bytes)});
	if (rc) return rc;
	ctx->seed.tied = (uint32_t*)((char*)ctx->seed.stacks + stack_bytes);   // (an alias into stacks, not an allocation)
	if (n_mini > ctx->seed_cap_mini) {
		// the per-minimizer buffers grow together: release, then allocate (a lower peak), all of them or none
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		const size_t n = (size_t)n_mini + (size_t)n_mini / 4 + 1024;
		const chaindp::DevBuf grow[7] = {dev_buf(ctx->seed.kept, n * 8), dev_buf(ctx->seed.used, n * 8), dev_buf(ctx->seed.src, n * 8), dev_buf(ctx->seed.mstate, n * 8),
		                                 dev_buf(ctx->seed.tile_tmp, (n / 1024 + 2) * 8), dev_buf(ctx->d_mini, n * 16), dev_buf(ctx->d_mini_pos, n * 8)};
		for (const chaindp::DevBuf &g : grow) ctx->pool.release(g.slot);
		ctx->seed_cap_mini = 0;
		const hipError_t e = (hipError_t)ctx->pool.alloc_group(grow, 7);
		if (e != hipSuccess && !oom_is_capacity) { ctx->err = std::string("hipMalloc (seed collection buffers): ") + hipGetErrorString(e); return CHAINDP_ERR_HIP; }
		if (e != hipSuccess) {
			(void)hipGetLastError();
			ctx->err = std::string("minimizer buffers for ") + std::to_string((long long)n_mini) + " minimizers: " + hipGetErrorString(e);
			return CHAINDP_ERR_CAPACITY;
		}
		ctx->seed_cap_mini = (int64_t)n;
	}
	return CHAINDP_OK;
}

// mini: all minimizers contiguous (read_mini == NULL), or read_mini[r] = read r's minimizers in pinned host memory
static int collect_seeds_impl(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, int64_t n_reads,
                              const int64_t *mini_off, const chaindp_anchor_t *mini, const chaindp_anchor_t *const *read_mini,
                              const uint32_t *bid, const int32_t *qlen,
                              const int32_t *n_segs_per_read, int64_t *off, int32_t *rep_len, int64_t *mini_pos_off)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!ix || ix->device != ctx->device) { ctx->err = "index image missing or on another device"; return CHAINDP_ERR_ARG; }
	// mini == NULL && mini_off == NULL: the minimizers the last chaindp_sketch left in this context (qlen == NULL: the lengths it saw)
	const bool resident = !mini && !mini_off && !read_mini;
	if (resident) {
		if (!ctx->sk_valid || n_reads != ctx->sk_n_reads) { ctx->err = "no minimizers of a chaindp_sketch of n_reads reads are resident in this context"; return CHAINDP_ERR_ARG; }
		mini_off = ctx->sk_mini_off.data();
		if (!qlen) qlen = ctx->sk_qlen.data();
	}
	if (n_reads < 0 || !mini_off || (n_reads > 0 && (mini_off[0] != 0 || !bid || !qlen))) { ctx->err = "bad minimizer offsets"; return CHAINDP_ERR_ARG; }
	const int64_t n_mini = n_reads > 0 ? mini_off[n_reads] : 0;
	if (n_mini < 0 || (n_mini > 0 && !mini && !read_mini && !resident)) { ctx->err = "bad minimizers"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads) { ctx->err = "batch exceeds the capacity the context was created with"; return CHAINDP_ERR_CAPACITY; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	ctx->seed_route_valid = false;
	int rc = seed_reserve(ctx, n_mini);
	if (rc) return rc;
	hipStream_t st = ctx->stream;
	if (!resident) {
		ctx->sk_valid = false;                                     // d_mini is about to hold the caller's minimizers
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mini_off, mini_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
	}
	if (resident) {                                                // they are where the sketch wrote them: d_mini, d_mini_off
	} else if (n_mini && read_mini) {                                     // one kernel pulls every read's minimizers out of its pinned buffer
		rc = stage_pointers(ctx, (const void *const *)read_mini, n_reads);
		if (rc) return rc;
		HIP_TRY(ctx, chaindp::launch_gather_reads(st, n_reads, ctx->d_mini_off, (const void *const *)ctx->d_ptrs, ctx->d_mini));
	} else if (n_mini) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mini, mini, (size_t)n_mini * 16, hipMemcpyHostToDevice, st));
	if (n_reads) {
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bid, bid, (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_qlen, qlen, (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
	}
	HIP_TRY(ctx, stage_n_segs(ctx, n_segs_per_read, n_reads, st));
	chaindp::SeedIndex dix;
	dix.B = ix->blob[0]; dix.H = ix->blob[1]; dix.V = ix->blob[2]; dix.P = ix->blob[3];
	dix.nB = ix->bytes[0]; dix.nH = ix->bytes[1]; dix.nV = ix->bytes[2]; dix.nP = ix->bytes[3];
	dix.b_bits = ix->b_bits;
	HIP_TRY(ctx, chaindp::launch_seed_collect(st, dix, flag, max_occ, n_reads, n_mini, ctx->d_mini_off, ctx->d_mini, ctx->d_bid, ctx->seed,
	                                          ctx->d_off, ctx->d_mp_off, ctx->d_rep_len));
	unsigned long long totals[2] = {0, 0};
	HIP_TRY(ctx, hipMemcpyAsync(totals, ctx->seed.totals, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if ((int64_t)totals[0] > ctx->cap_anchors) {
		begin_batch(ctx, 0, 0);
		ctx->err = "the batch's seeds exceed the anchor capacity the context was created with";
		return CHAINDP_ERR_CAPACITY;
	}
	// unsorted anchors go to the new_seed[] buffer (free at this point of a batch), the sort writes d_a
	if (!ctx->d_seeds) HIP_TRY(ctx, (hipError_t)ctx->pool.alloc(&ctx->d_seeds, (size_t)ctx->cap_anchors * sizeof(chaindp_seed_t) + 16));
	if (ctx->seed_max_n < 0) {
		int lds_limit = 0;
		HIP_TRY(ctx, hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
		int m = 8192, m2 = 65024, cap = (lds_limit - 8192) & ~15;
		// test switches: smaller limits send ordinary reads down the paths made for very large ones
		if (const char *v = getenv("CHAINDP_SEED_MAX_N")) { m = atoi(v) < m ? atoi(v) : m; if (const char *c = strchr(v, ',')) m2 = atoi(c + 1); }
		if (const char *v = getenv("CHAINDP_SEED_LAB_CAP")) cap = atoi(v) < cap ? atoi(v) & ~15 : cap;
		if (m < 64) m = 64;
		if (cap < 256) cap = 256;
		while (m > 0 && chaindp::seed_sort_lds_bytes(m, 32, 8) > (size_t)lds_limit) m -= 512;
		while (m2 > m && chaindp::seed_sort_lds_bytes(m2, 4, 2) > (size_t)lds_limit) m2 -= 64;
		ctx->seed_lab_cap = cap;
		ctx->seed_max_n = m; ctx->seed_max_n2 = m2;
	}
	HIP_TRY(ctx, chaindp::launch_seed_expand_sort(st, dix, flag, n_reads, n_mini, ctx->d_mini_off, ctx->d_mini, ctx->d_bid, ctx->d_qlen, ctx->seed,
	                                              ctx->d_seeds, ctx->d_a, ctx->d_off, ctx->d_mini_pos, ctx->seed_max_n, ctx->seed_max_n2,
	                                              ctx->seed_lab_cap, (int64_t)totals[0]));
	ctx->seed_route_valid = n_reads > 0;                           // (the sort clears its two counters when it has reads)
	if (off) HIP_TRY(ctx, hipMemcpyAsync(off, ctx->d_off, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
	if (mini_pos_off) HIP_TRY(ctx, hipMemcpyAsync(mini_pos_off, ctx->d_mp_off, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
	if (rep_len && n_reads) HIP_TRY(ctx, hipMemcpyAsync(rep_len, ctx->d_rep_len, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	begin_batch(ctx, n_reads, (int64_t)totals[0], true);
	ctx->n_mini_pos = (int64_t)totals[1];
	return CHAINDP_OK;
}

extern "C" int chaindp_collect_seeds(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, int64_t n_reads,
                                     const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid, const int32_t *qlen,
                                     const int32_t *n_segs_per_read, int64_t *off, int32_t *rep_len, int64_t *mini_pos_off)
{
	return collect_seeds_impl(ctx, ix, flag, max_occ, n_reads, mini_off, mini, nullptr, bid, qlen, n_segs_per_read, off, rep_len, mini_pos_off);
}

extern "C" int chaindp_collect_seeds_gather(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, int64_t n_reads,
                                            const int64_t *mini_off, const chaindp_anchor_t *const *read_mini, const uint32_t *bid,
                                            const int32_t *qlen, const int32_t *n_segs_per_read, int64_t *off, int32_t *rep_len,
                                            int64_t *mini_pos_off)
{
	if (ctx && n_reads > 0 && !read_mini) { ctx->err = "bad minimizers"; return CHAINDP_ERR_ARG; }
	return collect_seeds_impl(ctx, ix, flag, max_occ, n_reads, mini_off, nullptr, read_mini, bid, qlen, n_segs_per_read, off, rep_len, mini_pos_off);
}

// What the map calls open with: seeds (resident), DP + compaction, chains, hits -- every stage reads what the one before left in HBM.
// regs_off != NULL (chaindp_map_batch): the chain offsets go there and the hits are downloaded to regs, if regs_cap has room for them;
// NULL: the hits stay in HBM for the post steps.  A NULL qlen with NULL minimizers means the resident sketch's (checked by the seed
// collection); the caller gets it back.
static int map_prefix(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt, int64_t n_reads,
                      const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid, const int32_t *&qlen, const int32_t *n_segs_per_read,
                      const uint32_t *hash, int32_t *rep_len, int64_t *n_anchors, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap)
{
	if (!mini && !mini_off && !qlen && ctx->sk_valid && n_reads == ctx->sk_n_reads) qlen = ctx->sk_qlen.data();
	int rc = collect_seeds_impl(ctx, ix, flag, max_occ, n_reads, mini_off, mini, nullptr, bid, qlen, n_segs_per_read, nullptr, rep_len, nullptr);
	if (rc) return rc;
	if (n_anchors) *n_anchors = ctx->total;
	if ((rc = chaindp_run_full(ctx, par)) != CHAINDP_OK) return rc;
	std::vector<int64_t> c_off((size_t)(regs_off || n_reads <= 0 ? 1 : n_reads + 1)), b_off((size_t)(n_reads > 0 ? n_reads + 1 : 1));
	if ((rc = chaindp_backtrack(ctx, par, min_cnt, regs_off ? regs_off : c_off.data(), nullptr, b_off.data(), nullptr)) != CHAINDP_OK) return rc;
	if (regs_off && (n_reads > 0 ? regs_off[n_reads] : 0) > regs_cap) {
		ctx->err = "more hits than regs has room for (regs_off is valid; chaindp_gen_regs with a larger buffer returns them)";
		return CHAINDP_ERR_CAPACITY;
	}
	return gen_regs_impl(ctx, hash, qlen, regs, regs_off != nullptr);
}

extern "C" int chaindp_map_batch(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                                 int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid, const int32_t *qlen,
                                 const uint32_t *hash, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len, int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && !hash)) { ctx->err = "NULL output or hash"; return CHAINDP_ERR_ARG; }
	return map_prefix(ctx, ix, flag, max_occ, par, min_cnt, n_reads, mini_off, mini, bid, qlen, nullptr, hash, rep_len, n_anchors, regs_off, regs, regs_cap);
}

extern "C" int chaindp_scatter_mini_pos(chaindp_ctx_t *ctx, int64_t n_reads, uint64_t *const *dst)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n_reads != ctx->n_reads || (n_reads > 0 && !dst) || !ctx->d_mp_off) { ctx->err = "scatter does not match the last seed collection"; return CHAINDP_ERR_ARG; }
	for (int64_t r = 0; r < n_reads; ++r) if ((uintptr_t)dst[r] & 15u) { ctx->err = "scatter destinations must be 16-byte aligned"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = stage_pointers(ctx, (const void *const *)dst, n_reads);
	if (rc) return rc;
	HIP_TRY(ctx, chaindp::launch_scatter_words(ctx->stream, n_reads, ctx->d_mp_off, (void *const *)ctx->d_ptrs, ctx->d_mini_pos));
	return CHAINDP_OK;
}

extern "C" int chaindp_download_mini_pos(chaindp_ctx_t *ctx, uint64_t *mini_pos)
{
	if (!ctx || (ctx->n_mini_pos > 0 && !mini_pos)) return CHAINDP_ERR_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->n_mini_pos) HIP_TRY(ctx, hipMemcpyAsync(mini_pos, ctx->d_mini_pos, (size_t)ctx->n_mini_pos * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_download_anchors(chaindp_ctx_t *ctx, chaindp_anchor_t *a)
{
	if (!ctx || (ctx->total > 0 && !a)) return CHAINDP_ERR_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->total) HIP_TRY(ctx, hipMemcpyAsync(a, ctx->d_a, (size_t)ctx->total * 16, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

// ---- sketch on the GPU (include/chaindp.h): bases in, minimizers resident

// Buffers for a batch of n_bases bases in n_chunks chunks of n_seqs sequences.  All or nothing: when an allocation fails everything
// is released, so that the context is as it was before its first sketch.
static int sketch_reserve(chaindp_ctx *ctx, int64_t n_bases, int64_t n_chunks, int64_t n_seqs)
{
	if (!ctx->d_sk_totals) HIP_TRY(ctx, (hipError_t)ctx->pool.alloc((void**)&ctx->d_sk_totals, 4 * 8));
	if (n_bases <= ctx->sk_cap_bases && n_chunks <= ctx->sk_cap_chunks && n_seqs <= ctx->sk_cap_seqs) return CHAINDP_OK;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const size_t nb = (size_t)n_bases + (size_t)n_bases / 8 + 1024, nc = (size_t)n_chunks + (size_t)n_chunks / 8 + 64, nq = (size_t)n_seqs + (size_t)n_seqs / 8 + 64;
	const size_t nt = nb / 256 + 2, nr = (size_t)ctx->cap_reads + 2;
	size_t scan_items = nc + 1 > nt ? nc + 1 : nt;
	if (nr > scan_items) scan_items = nr;
	chaindp::SketchArgs &k = ctx->sk;
	const chaindp::DevBuf bufs[20] = {
		dev_buf(k.seq, nb + 16),
		dev_buf(k.seq_off, (nq + 1) * 8),
		dev_buf(k.chunk_seq, nc * 4),
		dev_buf(k.seq_chunk0, (nq + 1) * 4),
		dev_buf(k.read_seq0, nr * 4),
		dev_buf(k.seq_ybase, nq * 8),
		dev_buf(k.chunk_push, (nc + 1) * 8),
		dev_buf(k.chunk_slot, (nc + 1) * 8),
		dev_buf(k.tile_cnt, nt * 8),
		dev_buf(k.scan_tmp, (scan_items / 1024 + 4) * 8),
		dev_buf(k.pcode, nb + 16),
		dev_buf(k.pstart, nb * 4),
		dev_buf(k.pend, nb * 4),
		dev_buf(k.phz, nb * 8),
		dev_buf(k.sx, nb * 8),
		dev_buf(k.sy, nb * 8),
		dev_buf(k.sn, nb + 16),
		dev_buf(k.slc, nb),
		dev_buf(k.sseq, nb * 4),
		dev_buf(k.scnt, nb * 4)};
	for (const chaindp::DevBuf &b : bufs) ctx->pool.release(b.slot);
	ctx->sk_cap_bases = ctx->sk_cap_chunks = ctx->sk_cap_seqs = -1;
	const hipError_t e = (hipError_t)ctx->pool.alloc_group(bufs, 20);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		ctx->err = std::string("sketch buffers for ") + std::to_string((long long)n_bases) + " bases: " + hipGetErrorString(e);
		return CHAINDP_ERR_CAPACITY;
	}
	ctx->sk_cap_bases = (int64_t)nb - 16; ctx->sk_cap_chunks = (int64_t)nc; ctx->sk_cap_seqs = (int64_t)nq;
	return CHAINDP_OK;
}

// pe_ori >= 0: the segments worker_for turns round before it maps a pair are reverse-complemented on the device first (map.c:608-613)
// rid_base >= 0: the index-side sketch (mm_idx_gen's, index.c:511): y carries rid_base + the sequence's number and no shift
static int sketch_impl(chaindp_ctx *ctx, int w, int k, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const char *seq,
                       const int32_t *n_segs_per_read, int64_t *mini_off, int pe_ori, int64_t rid_base = -1)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (w < 1 || w > 255 || k < 1 || k > 28) { ctx->err = "w must be 1..255 and k 1..28 (sketch.c:84)"; return CHAINDP_ERR_ARG; }
	if (n_seqs < 0 || !seq_off || seq_off[0] != 0 || !mini_off) { ctx->err = "bad sequence offsets or NULL mini_off"; return CHAINDP_ERR_ARG; }
	for (int64_t q = 0; q < n_seqs; ++q) {
		if (seq_off[q + 1] < seq_off[q]) { ctx->err = "sequence offsets must not decrease"; return CHAINDP_ERR_ARG; }
		if (seq_off[q + 1] - seq_off[q] >= 0x7fffffff) { ctx->err = "a sequence of 2^31-1 bases or more"; return CHAINDP_ERR_CAPACITY; }
	}
	const int64_t n_bases = seq_off[n_seqs];
	if (n_bases > 0 && !seq) { ctx->err = "NULL sequence"; return CHAINDP_ERR_ARG; }
	if (n_seqs > 0x7ffffff0) { ctx->err = "too many sequences"; return CHAINDP_ERR_CAPACITY; }
	// reads -> sequences, rid and shift of every sequence (map.c:92-94), lengths of the reads
	int64_t n_reads = n_seqs;
	std::vector<int32_t> read_seq0;
	if (n_segs_per_read) {
		int64_t q = 0;
		for (n_reads = 0; q < n_seqs; ++n_reads) {
			if (n_segs_per_read[n_reads] < 1 || q + n_segs_per_read[n_reads] > n_seqs) { ctx->err = "n_segs_per_read does not add up to n_seqs"; return CHAINDP_ERR_ARG; }
			read_seq0.push_back((int32_t)q);
			q += n_segs_per_read[n_reads];
		}
		read_seq0.push_back((int32_t)n_seqs);
	}
	if (n_reads > ctx->cap_reads) { ctx->err = "batch exceeds the read capacity the context was created with"; return CHAINDP_ERR_CAPACITY; }
	if (n_bases > ctx->sk_max_bases) { ctx->err = "batch exceeds the bases one chaindp_sketch call takes"; return CHAINDP_ERR_CAPACITY; }
	std::vector<int32_t> seq_chunk0((size_t)n_seqs + 1), chunk_seq, qlen((size_t)n_reads);
	std::vector<unsigned long long> ybase((size_t)n_seqs);
	int64_t n_chunks = 0;
	for (int64_t r = 0, q = 0; r < n_reads; ++r) {
		const int64_t q1 = n_segs_per_read ? read_seq0[(size_t)r + 1] : r + 1, first = seq_off[q];
		if (seq_off[q1] - first > 0x7fffffff) { ctx->err = "a read of more than 2^31-1 bases"; return CHAINDP_ERR_CAPACITY; }
		qlen[(size_t)r] = (int32_t)(seq_off[q1] - first);
		for (int64_t rid = 0; q < q1; ++q, ++rid) {
			const int64_t len = seq_off[q + 1] - seq_off[q], nc = len > 0 ? (len + 255) / 256 : 1;
			if (n_chunks + nc > 0x7ffffff0) { ctx->err = "too many sequences"; return CHAINDP_ERR_CAPACITY; }
			seq_chunk0[(size_t)q] = (int32_t)n_chunks;
			chunk_seq.insert(chunk_seq.end(), (size_t)nc, (int32_t)q);
			n_chunks += nc;
			ybase[(size_t)q] = rid_base >= 0 ? (unsigned long long)(rid_base + q) << 32
			                                 : (unsigned long long)rid << 32 | (unsigned long long)(seq_off[q] - first) << 1;
		}
	}
	seq_chunk0[(size_t)n_seqs] = (int32_t)n_chunks;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = sketch_reserve(ctx, n_bases, n_chunks, n_seqs);
	if (rc) return rc;
	if (!ctx->seed_ready && (rc = seed_reserve(ctx, 0)) != CHAINDP_OK) return rc;
	// A sketch starts a new batch.  Its minimizers go to the buffers of the seed collection, which may have to grow (and with them
	// the mini_pos[] an earlier batch left), so that batch is dropped here: its downloads are refused or return nothing from now on.
	begin_batch(ctx, 0, 0);
	ctx->n_seeds = 0; ctx->n_mini_pos = 0; ctx->singles_pending = false; ctx->regs_resident = false; ctx->sk_valid = false;
	hipStream_t st = ctx->stream;
	chaindp::SketchArgs a = ctx->sk;
	a.w = w; a.k = k; a.is_hpc = is_hpc != 0; a.n_seqs = n_seqs; a.n_chunks = n_chunks;
	if (!n_segs_per_read) a.read_seq0 = nullptr;
	if (n_bases) HIP_TRY(ctx, hipMemcpyAsync((void*)a.seq, seq, (size_t)n_bases, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync((void*)a.seq_off, seq_off, (size_t)(n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync((void*)a.seq_chunk0, seq_chunk0.data(), (size_t)(n_seqs + 1) * 4, hipMemcpyHostToDevice, st));
	if (n_chunks) HIP_TRY(ctx, hipMemcpyAsync((void*)a.chunk_seq, chunk_seq.data(), (size_t)n_chunks * 4, hipMemcpyHostToDevice, st));
	if (n_seqs) HIP_TRY(ctx, hipMemcpyAsync((void*)a.seq_ybase, ybase.data(), (size_t)n_seqs * 8, hipMemcpyHostToDevice, st));
	if (n_segs_per_read) HIP_TRY(ctx, hipMemcpyAsync((void*)ctx->sk.read_seq0, read_seq0.data(), (size_t)(n_reads + 1) * 4, hipMemcpyHostToDevice, st));
	if (n_segs_per_read) HIP_TRY(ctx, chaindp::launch_frag_revcomp(st, n_reads, ctx->sk.read_seq0, a.seq_off, (uint8_t*)a.seq, pe_ori));
	hipEvent_t *ev = ctx->sk_ev;
	if (ctx->prof) for (int i = 0; i < 4; ++i) if (!ev[i]) HIP_TRY(ctx, hipEventCreate(&ev[i]));
	if (ctx->prof) HIP_TRY(ctx, hipEventRecord(ev[0], st));
	HIP_TRY(ctx, chaindp::launch_sketch_count(st, a, n_reads, n_bases, (unsigned long long*)ctx->d_mini_off, ctx->d_sk_totals));
	if (ctx->prof) HIP_TRY(ctx, hipEventRecord(ev[1], st));
	unsigned long long totals[4] = {0, 0, 0, 0};
	HIP_TRY(ctx, hipMemcpyAsync(totals, ctx->d_sk_totals, 32, hipMemcpyDeviceToHost, st));
	ctx->sk_mini_off.assign((size_t)n_reads + 1, 0);
	HIP_TRY(ctx, hipMemcpyAsync(ctx->sk_mini_off.data(), ctx->d_mini_off, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const int64_t n_mini = (int64_t)totals[2];
	if (ctx->sk_mini_off[(size_t)n_reads] != n_mini || n_mini < 0 || n_mini > n_bases) { ctx->err = "sketch: inconsistent minimizer counts"; return CHAINDP_ERR_HIP; }
	if ((rc = seed_reserve(ctx, n_mini, true)) != CHAINDP_OK) return rc;
	if (ctx->prof) HIP_TRY(ctx, hipEventRecord(ev[2], st));
	if (n_mini) HIP_TRY(ctx, chaindp::launch_sketch_emit(st, a, n_bases, ctx->d_mini, ctx->seed_cap_mini));
	if (ctx->prof) HIP_TRY(ctx, hipEventRecord(ev[3], st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (ctx->prof) {
		float m0 = 0, m1 = 0;
		HIP_TRY(ctx, hipEventElapsedTime(&m0, ev[0], ev[1]));
		HIP_TRY(ctx, hipEventElapsedTime(&m1, ev[2], ev[3]));
		ctx->sk_ms += (double)m0 + (double)m1; ctx->sk_calls += 1;
	}
	memcpy(mini_off, ctx->sk_mini_off.data(), (size_t)(n_reads + 1) * 8);
	ctx->sk_qlen.swap(qlen);
	ctx->sk_seq_len.resize((size_t)n_seqs);
	for (int64_t q = 0; q < n_seqs; ++q) ctx->sk_seq_len[(size_t)q] = (int32_t)(seq_off[q + 1] - seq_off[q]);
	ctx->sk_n_reads = n_reads; ctx->sk_n_mini = n_mini; ctx->sk_valid = true;
	return CHAINDP_OK;
}

extern "C" int chaindp_sketch(chaindp_ctx_t *ctx, int w, int k, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const char *seq,
                              const int32_t *n_segs_per_read, int64_t *mini_off)
{
	return sketch_impl(ctx, w, k, is_hpc, n_seqs, seq_off, seq, n_segs_per_read, mini_off, -1);
}

extern "C" int chaindp_download_minimizers(chaindp_ctx_t *ctx, chaindp_anchor_t *mini)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!ctx->sk_valid) { ctx->err = "no minimizers of a chaindp_sketch are resident in this context"; return CHAINDP_ERR_ARG; }
	if (ctx->sk_n_mini > 0 && !mini) { ctx->err = "NULL mini"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->sk_n_mini) HIP_TRY(ctx, hipMemcpyAsync(mini, ctx->d_mini, (size_t)ctx->sk_n_mini * 16, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_get_sketch_ms(chaindp_ctx_t *ctx, double *ms, int64_t *calls, int reset)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (ms) *ms = ctx->sk_ms;
	if (calls) *calls = ctx->sk_calls;
	if (reset) { ctx->sk_ms = 0; ctx->sk_calls = 0; }
	return CHAINDP_OK;
}

// ---- the index image built on the device (chaindp_index.hip): target bases in, B/H/V/P resident

namespace {
// device memory of one build: what is still held when the build returns, however it returns, is freed
struct IxMem {
	std::vector<void*> held;
	~IxMem() { for (void *p : held) if (p) (void)hipFree(p); }
	hipError_t alloc(void **p, size_t bytes)
	{
		const hipError_t e = hipMalloc(p, bytes ? bytes : 64);
		if (e == hipSuccess) held.push_back(*p); else *p = nullptr;
		return e;
	}
	void free(void *p) { for (void *&h : held) if (h == p && p) { (void)hipFree(p); h = nullptr; } }
	void *keep(void *p) { for (void *&h : held) if (h == p) h = nullptr; return p; }      // the index owns it from now on
};
struct IxPart { void *d; int64_t n; };
}

#define IX_TRY(ctx, call)                                                                          \
	do {                                                                                           \
		hipError_t e_ = (call);                                                                    \
		if (e_ == hipErrorOutOfMemory) {                                                           \
			(void)hipGetLastError();                                                               \
			(ctx)->err = "chaindp_index_build: the device has no room for the index";              \
			return CHAINDP_ERR_CAPACITY;                                                           \
		}                                                                                          \
		if (e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return CHAINDP_ERR_HIP; } \
	} while (0)

// stages 2-4: the minimizers of all parts (device buffers, x = hash << 8 | span, y = rid << 32 | pos << 1 | strand) -> *out
static int index_from_parts(chaindp_ctx *ctx, IxMem &mem, int b, const std::vector<IxPart> &parts, int64_t n_seqs, const uint32_t *rank,
                            int64_t sub_batches, chaindp_index **out)
{
	hipStream_t st = ctx->stream;
	int64_t n = 0;
	for (const IxPart &p : parts) n += p.n;
	if (n >= 0x7fffffff) { ctx->err = "chaindp_index_build: 2^31-1 minimizers or more in one index part"; return CHAINDP_ERR_CAPACITY; }
	const int64_t nb = (int64_t)1 << b, tiles = (n + IX_TILE - 1) / IX_TILE;
	chaindp::IndexScratch sc = {};
	void *rec[2] = {nullptr, nullptr};
	uint32_t *d_rank = nullptr;
	const int64_t scan_items = 256 * tiles > nb ? 256 * tiles : nb;
	IX_TRY(ctx, mem.alloc((void**)&sc.hist, (size_t)(256 * tiles + 1) * 8));
	IX_TRY(ctx, mem.alloc((void**)&sc.scan_tmp, (size_t)(scan_items / 1024 + 4) * 8));
	IX_TRY(ctx, mem.alloc((void**)&sc.bits, 4 * 8));
	IX_TRY(ctx, mem.alloc((void**)&sc.bk_keys, (size_t)nb * 4));
	IX_TRY(ctx, mem.alloc((void**)&sc.bk_p, (size_t)nb * 4));
	IX_TRY(ctx, mem.alloc((void**)&sc.bk_start, (size_t)nb * 8));
	IX_TRY(ctx, mem.alloc((void**)&sc.bk_h, (size_t)nb * 8));
	IX_TRY(ctx, mem.alloc((void**)&sc.bk_pp, (size_t)nb * 8));
	IX_TRY(ctx, mem.alloc((void**)&sc.totals, 8 * 8));
	IX_TRY(ctx, mem.alloc(&rec[0], (size_t)n * 16));
	if (rank && n_seqs) {
		IX_TRY(ctx, mem.alloc((void**)&d_rank, (size_t)n_seqs * 4));
		IX_TRY(ctx, hipMemcpyAsync(d_rank, rank, (size_t)n_seqs * 4, hipMemcpyHostToDevice, st));
	}
	struct Events { hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } ev;
	for (hipEvent_t &x : ev.e) IX_TRY(ctx, hipEventCreate(&x));
	float ms_prepare = 0, ms_sort = 0, ms_group = 0, ms_tables = 0;
	unsigned long long bits[4] = {0, ~0ull, 0, ~0ull};
	IX_TRY(ctx, hipMemcpyAsync(sc.bits, bits, 32, hipMemcpyHostToDevice, st));
	IX_TRY(ctx, hipEventRecord(ev.e[0], st));
	int64_t at = 0;
	for (const IxPart &p : parts) {
		IX_TRY(ctx, chaindp::launch_index_prepare(st, b, p.n, p.d, (char*)rec[0] + at * 16, sc.bits));
		at += p.n;
	}
	IX_TRY(ctx, hipEventRecord(ev.e[1], st));
	IX_TRY(ctx, hipMemcpyAsync(bits, sc.bits, 32, hipMemcpyDeviceToHost, st));
	IX_TRY(ctx, hipStreamSynchronize(st));
	IX_TRY(ctx, hipEventElapsedTime(&ms_prepare, ev.e[0], ev.e[1]));
	for (const IxPart &p : parts) mem.free(p.d);
	IX_TRY(ctx, mem.alloc(&rec[1], (size_t)n * 16));
	// least significant first: the bytes of y, then those of (bucket, m >> b); a byte that is the same in every record is no digit
	int run = 0, skipped = 0, cur = 0;
	IX_TRY(ctx, hipEventRecord(ev.e[0], st));
	for (int d = 0; d < 16 && n > 0; ++d) {
		const int word = d < 8 ? 1 : 0, shift = (d & 7) * 8;
		const unsigned long long differ = word ? bits[2] ^ bits[3] : bits[0] ^ bits[1];
		if (!((differ >> shift) & 255)) { ++skipped; continue; }
		IX_TRY(ctx, chaindp::launch_index_sort_pass(st, n, rec[cur], rec[cur ^ 1], word, shift, sc.hist, sc.scan_tmp, sc.totals));
		cur ^= 1; ++run;
	}
	chaindp_index *ix = new chaindp_index();
	ix->device = ctx->device; ix->b_bits = b; ix->built = true;
	struct Drop { chaindp_index *p; ~Drop() { if (p) chaindp_index_destroy(p); } } drop{ix};
	ix->bytes[0] = (size_t)nb * 16;
	if (hipMalloc((void**)&ix->blob[0], ix->bytes[0] + 64) != hipSuccess) { (void)hipGetLastError(); ctx->err = "chaindp_index_build: the device has no room for the index"; return CHAINDP_ERR_CAPACITY; }
	IX_TRY(ctx, hipEventRecord(ev.e[1], st));
	IX_TRY(ctx, chaindp::launch_index_group(st, b, n, rec[cur], sc, ix->blob[0]));
	IX_TRY(ctx, hipEventRecord(ev.e[2], st));
	unsigned long long tot[8];
	IX_TRY(ctx, hipMemcpyAsync(tot, sc.totals, 64, hipMemcpyDeviceToHost, st));
	IX_TRY(ctx, hipStreamSynchronize(st));
	IX_TRY(ctx, hipEventElapsedTime(&ms_sort, ev.e[0], ev.e[1]));
	IX_TRY(ctx, hipEventElapsedTime(&ms_group, ev.e[1], ev.e[2]));
	mem.free(rec[cur ^ 1]); mem.free(sc.hist);
	if (tot[0] >= 1ull << 36 || tot[1] >= 1ull << 36) { ctx->err = "chaindp_index_build: a blob passes the 36-bit offsets of B (index.c:624)"; return CHAINDP_ERR_CAPACITY; }
	ix->bytes[1] = (size_t)tot[0] * 8; ix->bytes[2] = (size_t)tot[0] * 8; ix->bytes[3] = (size_t)tot[1] * 8;
	for (int k = 1; k < 4; ++k) {
		const size_t alloc = ((ix->bytes[k] + 63) & ~(size_t)63) + 64;          // the kernels read whole 64-byte groups
		if (hipMalloc((void**)&ix->blob[k], alloc) != hipSuccess) { (void)hipGetLastError(); ctx->err = "chaindp_index_build: the device has no room for the index"; return CHAINDP_ERR_CAPACITY; }
		IX_TRY(ctx, hipMemsetAsync(ix->blob[k], 0, alloc, st));
	}
	if (tot[0]) {
		uint8_t *occ = nullptr;
		const size_t ob = (size_t)tot[0] / 8;
		IX_TRY(ctx, mem.alloc((void**)&occ, 2 * ob));
		IX_TRY(ctx, hipMemsetAsync(occ, 0, 2 * ob, st));
		IX_TRY(ctx, hipEventRecord(ev.e[0], st));
		IX_TRY(ctx, chaindp::launch_index_tables(st, b, n, rec[cur], sc, d_rank, n_seqs, ix->blob[1], ix->blob[2], ix->blob[3], occ, occ + ob));
		IX_TRY(ctx, hipEventRecord(ev.e[1], st));
	}
	IX_TRY(ctx, hipStreamSynchronize(st));
	if (tot[0]) IX_TRY(ctx, hipEventElapsedTime(&ms_tables, ev.e[0], ev.e[1]));
	ix->stage_ms[1] = (double)ms_prepare + (double)ms_sort; ix->stage_ms[2] = ms_group; ix->stage_ms[3] = ms_tables;
	const int64_t route[8] = {sub_batches, n, (int64_t)tot[2], (int64_t)tot[3], (int64_t)tot[4], (int64_t)tot[5], run, skipped};
	memcpy(ix->route, route, sizeof(route));
	drop.p = nullptr;
	*out = ix;
	return CHAINDP_OK;
}

static int index_build_impl(chaindp_ctx *ctx, int w, int k, int b, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const char *seq,
                            const uint32_t *rank, chaindp_index **out)
{
	if (b < 1 || b > 24) { ctx->err = "chaindp_index_build: b (bucket bits) must be 1..24"; return CHAINDP_ERR_ARG; }
	if (w < 1 || w > 255 || k < 1 || k > 28) { ctx->err = "w must be 1..255 and k 1..28 (sketch.c:84)"; return CHAINDP_ERR_ARG; }
	if (n_seqs < 0 || !seq_off || seq_off[0] != 0) { ctx->err = "bad sequence offsets"; return CHAINDP_ERR_ARG; }
	if (n_seqs > (1 << 21)) { ctx->err = "chaindp_index_build: more than 2^21 sequences (the image has 21 bits for a reference id)"; return CHAINDP_ERR_ARG; }
	for (int64_t q = 0; q < n_seqs; ++q) {
		if (seq_off[q + 1] < seq_off[q]) { ctx->err = "sequence offsets must not decrease"; return CHAINDP_ERR_ARG; }
		if (seq_off[q + 1] - seq_off[q] >= (1 << 21)) { ctx->err = "chaindp_index_build: a sequence of 2^21 bases or more (the image has 21 bits for a position)"; return CHAINDP_ERR_ARG; }
		if (rank && rank[q] >= (1u << 21)) { ctx->err = "chaindp_index_build: a rank of 2^21 or more (the image has 21 bits for a rank id)"; return CHAINDP_ERR_ARG; }
	}
	if (seq_off[n_seqs] > 0 && !seq) { ctx->err = "NULL sequence"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	IxMem mem;
	std::vector<IxPart> parts;
	std::vector<int64_t> off, mini_off;
	const int64_t max_bases = ctx->ix_chunk_bases > 0 && ctx->ix_chunk_bases < ctx->sk_max_bases ? ctx->ix_chunk_bases : ctx->sk_max_bases;
	auto fail = [&](int rc) { ctx->sk_valid = false; return rc; };
	const auto t0 = std::chrono::steady_clock::now();
	// sketch sub-batches cut at sequence boundaries: as many sequences as the bases and the context's read capacity allow, at least one
	for (int64_t q0 = 0; q0 < n_seqs;) {
		int64_t q1 = q0 + 1;
		while (q1 < n_seqs && q1 - q0 < ctx->cap_reads && seq_off[q1 + 1] - seq_off[q0] <= max_bases) ++q1;
		off.resize((size_t)(q1 - q0) + 1); mini_off.resize((size_t)(q1 - q0) + 1);
		for (int64_t q = q0; q <= q1; ++q) off[(size_t)(q - q0)] = seq_off[q] - seq_off[q0];
		const int rc = sketch_impl(ctx, w, k, is_hpc, q1 - q0, off.data(), seq ? seq + seq_off[q0] : nullptr, nullptr, mini_off.data(), -1, q0);
		if (rc) return fail(rc);
		IxPart p = {nullptr, ctx->sk_n_mini};
		if (p.n) {
			const hipError_t e = mem.alloc(&p.d, (size_t)p.n * 16);
			if (e != hipSuccess) { (void)hipGetLastError(); ctx->err = "chaindp_index_build: the device has no room for the minimizers"; return fail(CHAINDP_ERR_CAPACITY); }
			if (hipMemcpyAsync(p.d, ctx->d_mini, (size_t)p.n * 16, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess ||
			    hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "chaindp_index_build: copying the minimizers failed"; return fail(CHAINDP_ERR_HIP); }
		}
		parts.push_back(p);
		q0 = q1;
	}
	ctx->sk_valid = false;                     // the resident minimizers are a sub-batch of the target's, nothing a mapping call should take
	const double sketch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	const int rc = index_from_parts(ctx, mem, b, parts, n_seqs, rank, (int64_t)parts.size(), out);
	if (rc == CHAINDP_OK) (*out)->stage_ms[0] = sketch_ms;
	return rc;
}

extern "C" chaindp_index_t *chaindp_index_build(chaindp_ctx_t *ctx, int w, int k, int b, int is_hpc, int64_t n_seqs, const int64_t *seq_off,
                                                const char *seq, const uint32_t *rank)
{
	if (!ctx) return nullptr;
	chaindp_index *ix = nullptr;
	ctx->ix_status = index_build_impl(ctx, w, k, b, is_hpc, n_seqs, seq_off, seq, rank, &ix);
	return ctx->ix_status == CHAINDP_OK ? ix : nullptr;
}

extern "C" int chaindp_index_build_status(const chaindp_ctx_t *ctx) { return ctx ? ctx->ix_status : CHAINDP_ERR_ARG; }


// Exists for tests: enters the build behind the sketch with n minimizers of the caller's (x = hash << 8 | span, y = rid << 32 | pos << 1 | strand).
extern "C" chaindp_index_t *chaindp_debug_index_from_minimizers(chaindp_ctx_t *ctx, int b, int64_t n, const chaindp_anchor_t *mini, int64_t n_seqs,
                                                                const uint32_t *rank)
{
	if (!ctx) return nullptr;
	if (b < 1 || b > 24 || n < 0 || (n > 0 && !mini) || n_seqs < 0 || n_seqs > (1 << 21)) { ctx->err = "chaindp_debug_index_from_minimizers: bad arguments"; return nullptr; }
	if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return nullptr; }
	IxMem mem;
	std::vector<IxPart> parts;
	if (n) {
		IxPart p = {nullptr, n};
		if (mem.alloc(&p.d, (size_t)n * 16) != hipSuccess || hipMemcpy(p.d, mini, (size_t)n * 16, hipMemcpyHostToDevice) != hipSuccess) {
			(void)hipGetLastError(); ctx->err = "chaindp_debug_index_from_minimizers: upload failed"; return nullptr;
		}
		parts.push_back(p);
	}
	chaindp_index *ix = nullptr;
	if (index_from_parts(ctx, mem, b, parts, n_seqs, rank, 0, &ix) != CHAINDP_OK) return nullptr;
	return ix;
}

extern "C" int chaindp_debug_index_chunk_bases(chaindp_ctx_t *ctx, int64_t n)
{
	if (!ctx || n < 0) return CHAINDP_ERR_ARG;
	ctx->ix_chunk_bases = n;
	return CHAINDP_OK;
}

extern "C" int chaindp_debug_index_route(const chaindp_index_t *ix, int64_t out[8])
{
	if (!ix || !out || !ix->built) return CHAINDP_ERR_ARG;
	memcpy(out, ix->route, sizeof(ix->route));
	return CHAINDP_OK;
}

// Exists for measurement (tools/index_probe.py): ms[0] the sketch sub-batches with their uploads and copies (host clock), ms[1] the
// sort (records + radix passes), ms[2] grouping, layout and B, ms[3] the tables -- the last three device time between events.
extern "C" int chaindp_debug_index_stage_ms(const chaindp_index_t *ix, double ms[4])
{
	if (!ix || !ms || !ix->built) return CHAINDP_ERR_ARG;
	memcpy(ms, ix->stage_ms, sizeof(ix->stage_ms));
	return CHAINDP_OK;
}

extern "C" int chaindp_index_sizes(const chaindp_index_t *ix, size_t bytes[4])
{
	if (!ix || !bytes) return CHAINDP_ERR_ARG;
	for (int k = 0; k < 4; ++k) bytes[k] = ix->bytes[k];
	return CHAINDP_OK;
}

extern "C" int chaindp_index_download(const chaindp_index_t *ix, void *B, void *H, void *V, void *P)
{
	if (!ix) return CHAINDP_ERR_ARG;
	if (hipSetDevice(ix->device) != hipSuccess) return CHAINDP_ERR_HIP;
	void *dst[4] = {B, H, V, P};
	for (int k = 0; k < 4; ++k)
		if (dst[k] && ix->bytes[k] && hipMemcpy(dst[k], ix->blob[k], ix->bytes[k], hipMemcpyDeviceToHost) != hipSuccess) return CHAINDP_ERR_HIP;
	return CHAINDP_OK;
}

extern "C" int chaindp_index_cal_max_occ(const chaindp_index_t *ix, float f, int32_t *max_occ)
{
	if (!ix || !max_occ) return CHAINDP_ERR_ARG;
	if (f <= 0.) { *max_occ = INT32_MAX; return CHAINDP_OK; }
	if (hipSetDevice(ix->device) != hipSuccess) return CHAINDP_ERR_HIP;
	const size_t slots = ix->bytes[2] / 8;
	std::vector<uint32_t> cnt(slots);
	if (slots) {
		IxMem mem;
		uint32_t *d_cnt = nullptr;
		unsigned *d_bad = nullptr, bad = 0;
		if (mem.alloc((void**)&d_cnt, slots * 4) != hipSuccess || mem.alloc((void**)&d_bad, 4) != hipSuccess) { (void)hipGetLastError(); return CHAINDP_ERR_CAPACITY; }
		chaindp::SeedIndex dix;
		dix.B = ix->blob[0]; dix.H = ix->blob[1]; dix.V = ix->blob[2]; dix.P = ix->blob[3];
		dix.nB = ix->bytes[0]; dix.nH = ix->bytes[1]; dix.nV = ix->bytes[2]; dix.nP = ix->bytes[3];
		dix.b_bits = ix->b_bits;
		if (hipMemset(d_cnt, 0, slots * 4) != hipSuccess || hipMemset(d_bad, 0, 4) != hipSuccess ||
		    chaindp::launch_index_counts(nullptr, dix, d_cnt, d_bad) != hipSuccess ||
		    hipMemcpy(cnt.data(), d_cnt, slots * 4, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost) != hipSuccess) return CHAINDP_ERR_HIP;
		if (bad) return CHAINDP_ERR_ARG;                   // B points outside H or V: not an image
	}
	size_t n = 0;
	for (size_t s = 0; s < slots; ++s) if (cnt[s]) cnt[n++] = cnt[s];
	if (!n) return CHAINDP_ERR_ARG;                        // the reference selects from an empty array here
	size_t kth = (size_t)(uint32_t)((1. - f) * n);
	if (kth >= n) kth = n - 1;
	std::nth_element(cnt.begin(), cnt.begin() + (ptrdiff_t)kth, cnt.begin() + (ptrdiff_t)n);
	*max_occ = (int32_t)(cnt[kth] + 1);
	return CHAINDP_OK;
}

// ---- streaming pipeline (include/chaindp.h): depth contexts, each with its own stream, round robin

struct PipeSlot {
	chaindp_ctx *ctx = nullptr;
	int64_t *h_seeds_off = nullptr;          // pinned
	chaindp_seed_t *h_seeds = nullptr;       // pinned
	unsigned long long *h_n_seeds = nullptr; // pinned
	hipEvent_t done = nullptr;               // kernels + small downloads of the batch
	hipEvent_t up = nullptr;                 // the batch's upload
	int64_t tag = 0, n_reads = 0, total = 0;
	int state = 0;                           // 0 free, 1 in flight, 2 waited (results in use)
};

struct chaindp_pipe {
	int device = -1, depth = 0;
	hipStream_t s_up = nullptr, s_down = nullptr;   // one stream per copy direction, shared by the slots: uploads and downloads of
	                                         // different batches then run on different DMA engines, at the same time
	std::vector<PipeSlot> slots;
	int head = 0, tail = 0, inflight = 0;    // tail: oldest submitted, head: next to submit
	std::string err;
};

extern "C" const char *chaindp_pipe_last_error(const chaindp_pipe_t *pipe)
{
	return pipe ? pipe->err.c_str() : g_create_error.c_str();
}

extern "C" void chaindp_pipe_destroy(chaindp_pipe_t *pipe)
{
	if (!pipe) return;
	if (pipe->device >= 0) (void)hipSetDevice(pipe->device);
	for (auto &sl : pipe->slots) {
		if (sl.ctx && sl.ctx->stream) (void)hipStreamSynchronize(sl.ctx->stream);
		if (sl.done) (void)hipEventDestroy(sl.done);
		if (sl.up) (void)hipEventDestroy(sl.up);
		if (sl.h_seeds_off) (void)hipHostFree(sl.h_seeds_off);
		if (sl.h_seeds) (void)hipHostFree(sl.h_seeds);
		if (sl.h_n_seeds) (void)hipHostFree(sl.h_n_seeds);
		if (sl.ctx) chaindp_destroy(sl.ctx);
	}
	if (pipe->s_up) { (void)hipStreamSynchronize(pipe->s_up); (void)hipStreamDestroy(pipe->s_up); }
	if (pipe->s_down) { (void)hipStreamSynchronize(pipe->s_down); (void)hipStreamDestroy(pipe->s_down); }
	delete pipe;
}

extern "C" chaindp_pipe_t *chaindp_pipe_create(int device, int depth, int64_t max_anchors, int64_t max_reads)
{
	g_create_error.clear();
	if (depth < 1 || depth > 8) { g_create_error = "chaindp_pipe_create: depth must be 1..8"; return nullptr; }
	chaindp_pipe *pipe = new chaindp_pipe();
	pipe->device = device; pipe->depth = depth;
	pipe->slots.resize((size_t)depth);
	if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&pipe->s_up, hipStreamNonBlocking) != hipSuccess ||
	    hipStreamCreateWithFlags(&pipe->s_down, hipStreamNonBlocking) != hipSuccess) {
		g_create_error = "chaindp_pipe_create: no usable HIP device (there is no CPU fallback)";
		chaindp_pipe_destroy(pipe);
		return nullptr;
	}
	for (auto &sl : pipe->slots) {
		sl.ctx = chaindp_create(device, max_anchors, max_reads);
		if (!sl.ctx) { chaindp_pipe_destroy(pipe); return nullptr; }
		const size_t na = (size_t)sl.ctx->cap_anchors, nr = (size_t)sl.ctx->cap_reads;
		hipError_t e = hipHostMalloc((void**)&sl.h_seeds_off, (nr + 1) * 8, hipHostMallocDefault);
		if (e == hipSuccess) e = hipHostMalloc((void**)&sl.h_seeds, na * sizeof(chaindp_seed_t) + 16, hipHostMallocDefault);
		if (e == hipSuccess) e = hipHostMalloc((void**)&sl.h_n_seeds, 64, hipHostMallocDefault);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.up, hipEventDisableTiming);
		if (e != hipSuccess) {
			g_create_error = std::string("chaindp_pipe_create: ") + hipGetErrorString(e);
			chaindp_pipe_destroy(pipe);
			return nullptr;
		}
	}
	return pipe;
}

extern "C" int chaindp_pipe_submit(chaindp_pipe_t *pipe, const chaindp_params_t *par, int64_t n_reads, const int64_t *off,
                                   const chaindp_anchor_t *a, const int32_t *n_segs_per_read, int64_t tag)
{
	if (!pipe) return CHAINDP_ERR_ARG;
	if (pipe->inflight == pipe->depth) { pipe->err = "every slot of the pipe is in flight: wait for the oldest batch first"; return CHAINDP_ERR_BUSY; }
	PipeSlot &sl = pipe->slots[(size_t)pipe->head];
	chaindp_ctx *ctx = sl.ctx;
	int rc = check_params(ctx, par);
	if (rc) { pipe->err = ctx->err; return rc; }
	if (n_reads < 0 || !off || (n_reads > 0 && off[0] != 0)) { pipe->err = "bad offsets"; return CHAINDP_ERR_ARG; }
	const int64_t total = n_reads > 0 ? off[n_reads] : 0;
	if (total < 0 || (total > 0 && !a)) { pipe->err = "bad anchors"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) { pipe->err = "batch exceeds the capacity the pipe was created with"; return CHAINDP_ERR_CAPACITY; }
	HIP_TRY(pipe, hipSetDevice(pipe->device));
	hipStream_t st = ctx->stream;
	// upload on the pipe's upload stream (the slot's previous batch has been waited for, so its buffers are free); the
	// slot's own stream takes over for the kernels once the upload is in
	HIP_TRY(pipe, hipMemcpyAsync(ctx->d_off, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, pipe->s_up));
	if (total) HIP_TRY(pipe, hipMemcpyAsync(ctx->d_a, a, (size_t)total * 16, hipMemcpyHostToDevice, pipe->s_up));
	HIP_TRY(pipe, stage_n_segs(ctx, n_segs_per_read, n_reads, pipe->s_up));
	HIP_TRY(pipe, hipEventRecord(sl.up, pipe->s_up));
	HIP_TRY(pipe, hipStreamWaitEvent(st, sl.up, 0));
	begin_batch(ctx, n_reads, total);
	rc = chaindp_run_full(ctx, par);
	if (rc) { pipe->err = ctx->err; return rc; }
	HIP_TRY(pipe, hipMemcpyAsync(sl.h_seeds_off, ctx->d_seeds_off, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(pipe, hipMemcpyAsync(sl.h_n_seeds, ctx->cmp.n_seeds, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(pipe, hipEventRecord(sl.done, st));
	sl.tag = tag; sl.n_reads = n_reads; sl.total = total; sl.state = 1;
	pipe->head = (pipe->head + 1) % pipe->depth;
	++pipe->inflight;
	return CHAINDP_OK;
}

extern "C" int chaindp_pipe_wait(chaindp_pipe_t *pipe, chaindp_pipe_result_t *res)
{
	if (!pipe || !res) return CHAINDP_ERR_ARG;
	PipeSlot &sl = pipe->slots[(size_t)pipe->tail];
	if (pipe->inflight == 0 || sl.state != 1) { pipe->err = sl.state == 2 ? "release the batch waited for first" : "nothing in flight"; return CHAINDP_ERR_BUSY; }
	HIP_TRY(pipe, hipSetDevice(pipe->device));
	HIP_TRY(pipe, hipEventSynchronize(sl.done));
	// the record count is known now: download exactly the batch's new_seed[] (the other slots' uploads and kernels go on)
	const int64_t m = sl.total > 0 && sl.n_reads > 0 ? (int64_t)(uint32_t)*sl.h_n_seeds : 0;
	sl.ctx->n_seeds = m;
	if (m > 0) {
		// a few workgroups are enough to fill the link and leave the shader array to the other slots' kernels
		static const int copy_blocks = getenv("CHAINDP_PIPE_COPY_BLOCKS") ? atoi(getenv("CHAINDP_PIPE_COPY_BLOCKS")) : 64;
		if (copy_blocks > 0) HIP_TRY(pipe, chaindp::launch_copy_out(pipe->s_down, sl.h_seeds, sl.ctx->d_seeds, (size_t)m * sizeof(chaindp_seed_t), copy_blocks));
		else HIP_TRY(pipe, hipMemcpyAsync(sl.h_seeds, sl.ctx->d_seeds, (size_t)m * sizeof(chaindp_seed_t), hipMemcpyDeviceToHost, pipe->s_down));
		HIP_TRY(pipe, hipStreamSynchronize(pipe->s_down));
	}
	if (sl.n_reads == 0) sl.h_seeds_off[0] = 0;
	res->tag = sl.tag; res->n_reads = sl.n_reads; res->n_anchors = sl.total; res->n_seeds = m;
	res->seeds_off = sl.h_seeds_off; res->seeds = sl.h_seeds;
	sl.state = 2;
	return CHAINDP_OK;
}

extern "C" int chaindp_pipe_release(chaindp_pipe_t *pipe)
{
	if (!pipe) return CHAINDP_ERR_ARG;
	PipeSlot &sl = pipe->slots[(size_t)pipe->tail];
	if (sl.state != 2) { pipe->err = "no waited batch to release"; return CHAINDP_ERR_ARG; }
	sl.state = 0;
	pipe->tail = (pipe->tail + 1) % pipe->depth;
	--pipe->inflight;
	return CHAINDP_OK;
}

// ---- chain_post + mm_est_err + mm_set_mapq (chaindp_post.hip) -------------------------------------------------------------------

// The integers k in [1, 2^24] where the host's logf((float)k) is not the correctly rounded (float)log((double)k), with the host's value
// there: built once per process.  Through volatile pointers, so that the compiler neither folds nor substitutes the library calls.
static std::once_flag g_logf_once;
static std::vector<uint32_t> g_logf_k;
static std::vector<float> g_logf_v;
static float (*volatile g_host_logf)(float) = logf;
static double (*volatile g_host_log)(double) = log;

static void build_logf_patches()
{
	std::call_once(g_logf_once, [] {
		float (*lf)(float) = g_host_logf;
		double (*ld)(double) = g_host_log;
		for (uint32_t k = 1; k <= (uint32_t)POST_LOGF_MAX; ++k) {
			const float h = lf((float)k), c = (float)ld((double)k);
			if (memcmp(&h, &c, 4) != 0) { g_logf_k.push_back(k); g_logf_v.push_back(h); }
		}
	});
}

extern "C" int64_t chaindp_post_logf_patches(uint32_t *k, float *v, int64_t cap)
{
	build_logf_patches();
	const int64_t n = (int64_t)g_logf_k.size();
	for (int64_t i = 0; i < n && i < cap; ++i) { if (k) k[i] = g_logf_k[(size_t)i]; if (v) v[i] = g_logf_v[(size_t)i]; }
	return n;
}

static int post_logf_upload(chaindp_ctx *ctx)
{
	if (ctx->logf_ready) return CHAINDP_OK;
	build_logf_patches();
	const size_t n = g_logf_k.size(), m = ctx->pool.mark();
	hipError_t e = (hipError_t)ctx->pool.alloc_group({dev_buf(ctx->d_logf_k, (n ? n : 1) * 4), dev_buf(ctx->d_logf_v, (n ? n : 1) * 4)});
	if (e == hipSuccess && n) e = hipMemcpy(ctx->d_logf_k, g_logf_k.data(), n * 4, hipMemcpyHostToDevice);
	if (e == hipSuccess && n) e = hipMemcpy(ctx->d_logf_v, g_logf_v.data(), n * 4, hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		ctx->pool.rollback(m);
		ctx->err = std::string("logf patch tables: ") + hipGetErrorString(e);
		return CHAINDP_ERR_HIP;
	}
	ctx->n_logf = (int)n; ctx->logf_ready = true;
	return CHAINDP_OK;
}

// everything chaindp_chain_post and chaindp_frag_post share on the device, for a batch of n_c chains with n_b chain anchors
static int post_reserve(chaindp_ctx *ctx, int64_t n_c, int64_t n_b)
{
	int rc = regs_per_read_buffers(ctx);
	if (rc) return rc;
	if ((rc = post_logf_upload(ctx)) != CHAINDP_OK) return rc;
	const size_t RB = (size_t)ctx->cap_reads + 2;
	rc = first_use(ctx, ctx->post_ready, "chain_post", {dev_buf(ctx->d_post_off, RB * 8), dev_buf(ctx->d_post_tile, (RB / 1024 + 2) * 8),
	                                                    dev_buf(ctx->d_post_qlen, RB * 4), dev_buf(ctx->d_post_rep, RB * 4), dev_buf(ctx->d_post_err, 4)});
	if (rc) return rc;
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_post_stage, ctx->post_stage_cap, (size_t)n_c * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_post_out, ctx->post_out_cap, (size_t)n_c * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_post_sq, ctx->post_sq_cap, (size_t)(n_b > 0 ? n_b : 1) * 16));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_post_scratch, ctx->post_scratch_cap, (size_t)n_c * POST_SCRATCH_INTS * 4));
	return CHAINDP_OK;
}

extern "C" int64_t chaindp_post_logf_selftest(chaindp_ctx_t *ctx, int32_t kmax)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (kmax < 1 || kmax > POST_LOGF_MAX) { ctx->err = "kmax must lie in [1, 2^24]"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = post_logf_upload(ctx);
	if (rc) return rc;
	float *d_out = nullptr;
	HIP_TRY(ctx, hipMalloc(&d_out, (size_t)kmax * 8));
	int32_t *d_term = (int32_t*)(d_out + kmax);
	std::vector<float> dev((size_t)kmax);
	std::vector<int32_t> term((size_t)kmax);
	hipError_t e = chaindp::launch_post_logf_probe(ctx->stream, kmax, ctx->d_logf_k, ctx->d_logf_v, ctx->n_logf, d_out, d_term);
	if (e == hipSuccess) e = hipMemcpyAsync(dev.data(), d_out, (size_t)kmax * 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(term.data(), d_term, (size_t)kmax * 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	(void)hipFree(d_out);
	if (e != hipSuccess) { ctx->err = std::string("logf self-test: ") + hipGetErrorString(e); return CHAINDP_ERR_HIP; }
	float (*lf)(float) = g_host_logf;
	int64_t bad = 0;
	for (int32_t k = 1; k <= kmax; ++k) {
		const float h = lf((float)k);
		const int t = (int)(4.343f * h + .499f);                     // hit.c:474 as the host evaluates it: float multiply, float add
		bad += memcmp(&h, &dev[(size_t)k - 1], 4) != 0 || t != term[(size_t)k - 1];
	}
	return bad;
}

static chaindp::PostOpt to_post_opt(const chaindp_post_opt_t *o)
{
	chaindp::PostOpt p;
	p.flag = o->flag; p.mask_level = o->mask_level; p.pri_ratio = o->pri_ratio; p.best_n = o->best_n; p.min_diff = o->min_diff;
	p.sub_diff = o->sub_diff; p.max_join_long = o->max_join_long; p.max_join_short = o->max_join_short;
	p.min_join_flank_sc = o->min_join_flank_sc; p.min_cnt = o->min_cnt; p.min_chain_score = o->min_chain_score; p.match_sc = o->match_sc;
	p.is_sr = o->is_sr;
	return p;
}

extern "C" int chaindp_chain_post(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, const int32_t *qlen, const int32_t *rep_len,
                                  const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                                  int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *a_off, chaindp_anchor_t *a)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!opt || !regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || n_ref < 0 || (n_ref > 0 && !ref_len) || (a && !a_off)) {
		ctx->err = "NULL argument"; return CHAINDP_ERR_ARG;
	}
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has || !ctx->regs_resident) {
		ctx->err = "chaindp_chain_post needs the hits of a chaindp_gen_regs on this batch (a chaindp_est_err since has replaced them)";
		return CHAINDP_ERR_ARG;
	}
	const int64_t R = ctx->bot_n_reads, n_c = ctx->bot_n_chains, n_b = ctx->bot_n_b;
	const bool do_mapq = !(opt->flag & CHAINDP_F_CIGAR), do_err = !opt->is_sr;
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// single-segment reads only (mm_select_sub_multi, mm_seg_gen and mm_pair are not here)
	if (ctx->ran_par.n_segs > 1 && !ctx->has_n_segs) { ctx->err = "chaindp_chain_post takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	if (ctx->has_n_segs && R > 0) {
		std::vector<int32_t> ns((size_t)R);
		HIP_TRY(ctx, hipMemcpyAsync(ns.data(), ctx->d_n_segs, (size_t)R * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		for (int32_t v : ns) if (v > 1) { ctx->err = "chaindp_chain_post takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	}
	if (R == 0 || n_c == 0) {
		for (int64_t r = 0; r <= R; ++r) { regs_off[r] = 0; if (a_off) a_off[r] = 0; }
		return CHAINDP_OK;
	}
	int rc = do_err ? mini_pos_check(ctx, mini_pos_off, mini_pos) : CHAINDP_OK;
	if (rc) return rc;
	if (do_mapq && !rep_len && !ctx->mp_resident) { ctx->err = "no resident rep_len: pass it, or collect the seeds with chaindp_collect_seeds"; return CHAINDP_ERR_ARG; }
	if ((rc = post_reserve(ctx, n_c, n_b)) != CHAINDP_OK) return rc;
	const int32_t *d_qlen = ctx->d_rqlen;
	if (qlen) { HIP_TRY(ctx, hipMemcpyAsync(ctx->d_post_qlen, qlen, (size_t)R * 4, hipMemcpyHostToDevice, st)); d_qlen = ctx->d_post_qlen; }
	const int32_t *d_rep = ctx->d_rep_len;
	if (rep_len) { HIP_TRY(ctx, hipMemcpyAsync(ctx->d_post_rep, rep_len, (size_t)R * 4, hipMemcpyHostToDevice, st)); d_rep = ctx->d_post_rep; }
	HIP_TRY(ctx, hipMemsetAsync(ctx->d_post_err, 0, 4, st));
	const chaindp::PostOpt po = to_post_opt(opt);
	HIP_TRY(ctx, chaindp::launch_post_read(st, R, ctx->bot.chains_off, ctx->bot.b_off, ctx->bot.b_out, ctx->d_regs, d_qlen, po,
	                                       (int32_t*)ctx->d_post_scratch, ctx->d_post_stage, ctx->d_post_sq, ctx->d_post_off));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, R, ctx->d_post_off, ctx->d_post_tile, ctx->d_post_off + R));
	HIP_TRY(ctx, chaindp::launch_post_scatter(st, R, ctx->bot.chains_off, ctx->d_post_off, ctx->d_post_stage, ctx->d_post_out));
	HIP_TRY(ctx, hipMemcpyAsync(regs_off, ctx->d_post_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const int64_t n_out = regs_off[R];
	if (n_out > regs_cap) { ctx->err = "more hits than regs has room for (regs_off is valid)"; return CHAINDP_ERR_CAPACITY; }
	if (do_err && n_out > 0) {
		const int64_t *d_mpo = nullptr;
		const unsigned long long *d_mp = nullptr;
		if ((rc = stage_mini_pos(ctx, R, mini_pos_off, mini_pos, ref_len, n_ref, d_mpo, d_mp)) != CHAINDP_OK) return rc;
		// k_regs_div over the packed output, with the anchors as chain_post left them (mm_est_err at map.c:872)
		HIP_TRY(ctx, chaindp::launch_est_err(st, R, n_out, (const int64_t*)ctx->d_post_off, ctx->bot.b_off, ctx->d_post_sq, d_qlen,
		                                     (const int32_t*)ctx->d_ref_len, n_ref, d_mpo, d_mp, ctx->d_sum_k, ctx->d_post_out, nullptr));
	}
	if (do_mapq && n_out > 0)
		HIP_TRY(ctx, chaindp::launch_post_mapq(st, R, ctx->d_post_off, d_rep, opt->min_chain_score, ctx->d_logf_k, ctx->d_logf_v, ctx->n_logf,
		                                       ctx->d_post_out, ctx->d_post_err));
	int32_t err = 0;
	if (n_out > 0) HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->d_post_out, (size_t)n_out * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	if (a_off) HIP_TRY(ctx, hipMemcpyAsync(a_off, ctx->bot.b_off, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, st));
	if (a && n_b > 0) HIP_TRY(ctx, hipMemcpyAsync(a, ctx->d_post_sq, (size_t)n_b * 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(&err, ctx->d_post_err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (err) { ctx->err = "a score or n_sub + 1 above 2^24: beyond the logf patch list"; return CHAINDP_ERR_CAPACITY; }
	return CHAINDP_OK;
}

extern "C" int chaindp_map_reads(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                                 const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid,
                                 const int32_t *qlen, const uint32_t *hash, const int32_t *ref_len, int32_t n_ref, int64_t *regs_off, chaindp_reg_t *regs,
                                 int64_t regs_cap, int32_t *rep_len, int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!opt || !regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && !hash)) { ctx->err = "NULL output, hash or opt"; return CHAINDP_ERR_ARG; }
	if (par->n_segs > 1) { ctx->err = "chaindp_map_reads takes single-segment reads only (n_segs > 1)"; return CHAINDP_ERR_ARG; }
	// the stages of chaindp_map_batch, with the hits left in HBM, then chain_post on them
	rc = map_prefix(ctx, ix, flag, max_occ, par, min_cnt, n_reads, mini_off, mini, bid, qlen, nullptr, hash, rep_len, n_anchors, nullptr, nullptr, 0);
	if (rc) return rc;
	return chaindp_chain_post(ctx, opt, nullptr, nullptr, ref_len, n_ref, nullptr, nullptr, regs_off, regs, regs_cap, nullptr, nullptr);
}

extern "C" int chaindp_map_seqs(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int w, int k, int is_hpc, int flag, int max_occ, const chaindp_params_t *par,
                                int min_cnt, const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const uint32_t *bid,
                                const uint32_t *hash, const int32_t *ref_len, int32_t n_ref, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap,
                                int32_t *rep_len, int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!opt || !regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && (!hash || !bid))) { ctx->err = "NULL output, bid, hash or opt"; return CHAINDP_ERR_ARG; }
	if (!ix || ix->device != ctx->device) { ctx->err = "index image missing or on another device"; return CHAINDP_ERR_ARG; }
	std::vector<int64_t> mini_off((size_t)(n_reads > 0 ? n_reads + 1 : 1));
	if ((rc = chaindp_sketch(ctx, w, k, is_hpc, n_reads, seq_off, seq, nullptr, mini_off.data())) != CHAINDP_OK) return rc;
	return chaindp_map_reads(ctx, ix, flag, max_occ, par, min_cnt, opt, n_reads, nullptr, nullptr, bid, nullptr, hash, ref_len, n_ref, regs_off, regs,
	                         regs_cap, rep_len, n_anchors);
}

// ---- reads of several segments: chain_post with mm_select_sub_multi, mm_seg_gen, per-segment mm_set_parent and mm_set_mapq ----------

extern "C" int chaindp_debug_set_frag_lds_cap(chaindp_ctx_t *ctx, int cap)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (cap < 0 || cap > FRAG_LDS_CAP) { ctx->err = "the fragment kernels keep 0..FRAG_LDS_CAP hits in LDS"; return CHAINDP_ERR_ARG; }
	ctx->frag_lds_cap = cap;
	return CHAINDP_OK;
}

static int frag_post_impl(chaindp_ctx *ctx, const chaindp_post_opt_t *opt, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                          const int32_t *rep_len, const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                          int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *seg_a_off, chaindp_anchor_t *seg_a, int pe_ori,
                          const int32_t *host_qlen = nullptr)   // host_qlen: the caller has just uploaded n_segs_per_read and this qlen itself
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!opt || !seg_regs_off || n_seqs < 0 || regs_cap < 0 || (regs_cap > 0 && !regs) || n_ref < 0 || (n_ref > 0 && !ref_len) || (seg_a && !seg_a_off)) {
		ctx->err = "NULL argument"; return CHAINDP_ERR_ARG;
	}
	if (ctx->bot_n_reads < 0 || ctx->bot_n_reads != ctx->n_reads || !ctx->bot.has || !ctx->regs_resident) {
		ctx->err = "chaindp_frag_post needs the hits of a chaindp_gen_regs on this batch (a chaindp_est_err since has replaced them)";
		return CHAINDP_ERR_ARG;
	}
	const int64_t R = ctx->bot_n_reads, n_c = ctx->bot_n_chains, n_b = ctx->bot_n_b, S = n_seqs;
	const bool do_mapq = !(opt->flag & CHAINDP_F_CIGAR);
	hipStream_t st = ctx->stream;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the reads' segments: the caller's, checked against what the batch was chained with
	std::vector<int32_t> ns((size_t)R, ctx->ran_par.n_segs), read_seq0((size_t)R + 1, 0);
	if (host_qlen && n_segs_per_read) {
		ns.assign(n_segs_per_read, n_segs_per_read + R);
	} else if (ctx->has_n_segs && R > 0) {
		HIP_TRY(ctx, hipMemcpyAsync(ns.data(), ctx->d_n_segs, (size_t)R * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
	}
	bool any_single = false;
	int64_t n_sum = 0;
	for (int64_t r = 0; r < R; ++r) {
		if (n_segs_per_read && n_segs_per_read[r] != ns[(size_t)r]) { ctx->err = "n_segs_per_read differs from the segments the batch was chained with"; return CHAINDP_ERR_ARG; }
		if (ns[(size_t)r] < 1 || ns[(size_t)r] > 255) { ctx->err = "a read owns 1..255 segments (MM_MAX_SEG)"; return CHAINDP_ERR_ARG; }
		any_single |= ns[(size_t)r] == 1;
		n_sum += ns[(size_t)r];
		read_seq0[(size_t)r + 1] = (int32_t)(n_sum <= S ? n_sum : S);
	}
	if (n_sum != S) { ctx->err = "the reads' segments do not add up to n_seqs"; return CHAINDP_ERR_ARG; }
	if (!seg_len) {
		if (!ctx->sk_valid || (int64_t)ctx->sk_seq_len.size() != S) { ctx->err = "no seg_len and no chaindp_sketch of n_seqs sequences resident"; return CHAINDP_ERR_ARG; }
		seg_len = ctx->sk_seq_len.data();
	}
	for (int64_t q = 0; q < S; ++q) if (seg_len[q] < 0) { ctx->err = "negative seg_len"; return CHAINDP_ERR_ARG; }
	if (S == 0 || n_c == 0) {                                    // no hits anywhere: nothing resident to look at (chaindp_gen_regs uploaded nothing)
		for (int64_t q = 0; q <= S; ++q) { seg_regs_off[q] = 0; if (seg_a_off) seg_a_off[q] = 0; }
		return CHAINDP_OK;
	}
	{
		std::vector<int32_t> ql((size_t)R);
		if (host_qlen) {
			ql.assign(host_qlen, host_qlen + R);
		} else {
			HIP_TRY(ctx, hipMemcpyAsync(ql.data(), ctx->d_rqlen, (size_t)R * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(ctx, hipStreamSynchronize(st));
		}
		for (int64_t r = 0; r < R; ++r) {
			int64_t sum = 0;
			for (int32_t q = read_seq0[(size_t)r]; q < read_seq0[(size_t)r + 1]; ++q) sum += seg_len[q];
			if (sum != ql[(size_t)r]) { ctx->err = "seg_len does not add up to the qlen chaindp_gen_regs was given"; return CHAINDP_ERR_ARG; }
		}
	}
	const bool do_err = !opt->is_sr && any_single;               // mm_seg_gen rebuilds the records of the other reads: div = -1 there
	int rc = do_err ? mini_pos_check(ctx, mini_pos_off, mini_pos) : CHAINDP_OK;
	if (rc) return rc;
	if (do_mapq && !rep_len && !ctx->mp_resident) { ctx->err = "no resident rep_len: pass it, or collect the seeds with chaindp_collect_seeds"; return CHAINDP_ERR_ARG; }
	if ((rc = post_reserve(ctx, n_c, n_b)) != CHAINDP_OK) return rc;
	// per sequence: read_seq0[R + 1] | seq_len | seq_read | seq_rep | seq_hash; counts -> offsets: 3 x (S + 1), then the scans' scratch
	const size_t SB = (size_t)S + 2, tile_items = SB / 1024 + 2;
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_seq, ctx->frag_seq_cap, ((size_t)R + 2 + 4 * SB) * 4));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_cnt, ctx->frag_cnt_cap, (3 * SB + tile_items) * 8));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_a, ctx->frag_a_cap, (size_t)(n_b > 0 ? n_b : 1) * 16));
	int32_t *d_read_seq0 = (int32_t*)ctx->d_frag_seq, *d_seq_len = d_read_seq0 + R + 2, *d_seq_read = d_seq_len + SB, *d_seq_rep = d_seq_read + SB;
	uint32_t *d_seq_hash = (uint32_t*)(d_seq_rep + SB);
	unsigned long long *d_g = (unsigned long long*)ctx->d_frag_cnt, *d_o = d_g + SB, *d_a = d_o + SB, *d_tile = d_a + SB;
	HIP_TRY(ctx, hipMemcpyAsync(d_read_seq0, read_seq0.data(), (size_t)(R + 1) * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_seq_len, seg_len, (size_t)S * 4, hipMemcpyHostToDevice, st));
	const int32_t *d_rep = ctx->d_rep_len;
	if (rep_len) { HIP_TRY(ctx, hipMemcpyAsync(ctx->d_post_rep, rep_len, (size_t)R * 4, hipMemcpyHostToDevice, st)); d_rep = ctx->d_post_rep; }
	HIP_TRY(ctx, hipMemsetAsync(ctx->d_post_err, 0, 4, st));
	const chaindp::PostOpt po = to_post_opt(opt);
	// chain_post per read and the first half of mm_seg_gen.  The global scratch of what exceeds the LDS cap is sized for the fragments'
	// hits at this point and grown below for the segments' hits, once their count is known.
	HIP_TRY(ctx, chaindp::launch_frag_read(st, R, ctx->bot.chains_off, ctx->bot.b_off, ctx->bot.b_out, ctx->d_regs, ctx->d_rqlen, d_read_seq0, d_seq_len, po,
	                                       ctx->ran_par.max_dist_x, ctx->frag_lds_cap, (int32_t*)ctx->d_post_scratch, ctx->d_post_stage, ctx->d_post_sq,
	                                       ctx->d_post_off, d_g, d_o, d_a));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, R, ctx->d_post_off, ctx->d_post_tile, ctx->d_post_off + R));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, S, d_g, d_tile, d_g + S));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, S, d_o, d_tile, d_o + S));
	HIP_TRY(ctx, chaindp::launch_scan_u64(st, S, d_a, d_tile, d_a + S));
	unsigned long long tot[4] = {0, 0, 0, 0};
	HIP_TRY(ctx, hipMemcpyAsync(&tot[0], ctx->d_post_off + R, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(&tot[1], d_g + S, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(&tot[2], d_a + S, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(seg_regs_off, d_o, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, st));
	if (seg_a_off) HIP_TRY(ctx, hipMemcpyAsync(seg_a_off, d_a, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const int64_t n_post = (int64_t)tot[0], n_g = (int64_t)tot[1], n_sa = (int64_t)tot[2], n_out = seg_regs_off[S];
	if (n_post > n_c || n_sa > n_b || n_g > n_out) { ctx->err = "chaindp_frag_post: inconsistent counts"; return CHAINDP_ERR_HIP; }
	if (n_out > regs_cap) { ctx->err = "more hits than regs has room for (seg_regs_off is valid)"; return CHAINDP_ERR_CAPACITY; }
	HIP_TRY(ctx, chaindp::launch_post_scatter(st, R, ctx->bot.chains_off, ctx->d_post_off, ctx->d_post_stage, ctx->d_post_out));
	if (do_err && n_post > 0) {
		const int64_t *d_mpo = nullptr;
		const unsigned long long *d_mp = nullptr;
		if ((rc = stage_mini_pos(ctx, R, mini_pos_off, mini_pos, ref_len, n_ref, d_mpo, d_mp)) != CHAINDP_OK) return rc;
		// mm_est_err (map.c:872) on the packed hits of every read; only the one-segment reads keep theirs
		HIP_TRY(ctx, chaindp::launch_est_err(st, R, n_post, (const int64_t*)ctx->d_post_off, ctx->bot.b_off, ctx->d_post_sq, ctx->d_rqlen,
		                                     (const int32_t*)ctx->d_ref_len, n_ref, d_mpo, d_mp, ctx->d_sum_k, ctx->d_post_out, nullptr));
	}
	const size_t ng1 = (size_t)(n_g > 0 ? n_g : 1);
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_u, ctx->frag_u_cap, ng1 * 8));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_stage, ctx->frag_stage_cap, ng1 * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_z, ctx->frag_z_cap, ng1 * 16));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_stacks, ctx->frag_stacks_cap, (ng1 / 64 + 2 * (size_t)S + 4) * 12));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_frag_out, ctx->frag_out_cap, (size_t)(n_out > 0 ? n_out : 1) * sizeof(chaindp_reg_t)));
	HIP_TRY(ctx, dev_grow(ctx, ctx->d_post_scratch, ctx->post_scratch_cap, ng1 * POST_SCRATCH_INTS * 4));
	HIP_TRY(ctx, chaindp::launch_frag_split(st, R, ctx->d_post_off, ctx->d_post_out, ctx->bot.b_off, ctx->d_post_sq, d_read_seq0, d_seq_len, ctx->d_rhash,
	                                        do_mapq ? d_rep : nullptr, d_g, d_o, d_a, (unsigned long long*)ctx->d_frag_u, ctx->d_frag_a, ctx->d_frag_out,
	                                        d_seq_hash, d_seq_rep, d_seq_read));
	// mm_gen_regs per (fragment, segment) (hit.c:393): a segment is a read of its own to k_regs_keys / k_regs_fill
	if (n_g > 0)
		HIP_TRY(ctx, chaindp::launch_gen_regs(st, S, (const int64_t*)d_g, (const int64_t*)d_a, (const unsigned long long*)ctx->d_frag_u, ctx->d_frag_a,
		                                      d_seq_hash, d_seq_len, ctx->d_frag_z, ctx->d_frag_stacks, ctx->d_frag_stage));
	HIP_TRY(ctx, chaindp::launch_frag_seg(st, S, d_read_seq0, d_seq_read, d_g, d_o, ctx->d_frag_stage, opt->mask_level, ctx->frag_lds_cap,
	                                      (int32_t*)ctx->d_post_scratch, ctx->d_frag_out));
	if (do_mapq && n_out > 0)
		HIP_TRY(ctx, chaindp::launch_post_mapq(st, S, d_o, d_seq_rep, opt->min_chain_score, ctx->d_logf_k, ctx->d_logf_v, ctx->n_logf, ctx->d_frag_out,
		                                       ctx->d_post_err));
	HIP_TRY(ctx, chaindp::launch_frag_flip(st, S, d_read_seq0, d_seq_read, d_seq_len, d_o, pe_ori, ctx->d_frag_out));
	int32_t err = 0;
	if (n_out > 0) HIP_TRY(ctx, hipMemcpyAsync(regs, ctx->d_frag_out, (size_t)n_out * sizeof(chaindp_reg_t), hipMemcpyDeviceToHost, st));
	if (seg_a && n_sa > 0) HIP_TRY(ctx, hipMemcpyAsync(seg_a, ctx->d_frag_a, (size_t)n_sa * 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(&err, ctx->d_post_err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (err) { ctx->err = "a score or n_sub + 1 above 2^24: beyond the logf patch list"; return CHAINDP_ERR_CAPACITY; }
	return CHAINDP_OK;
}

extern "C" int chaindp_frag_post(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                                 const int32_t *rep_len, const int32_t *ref_len, int32_t n_ref, const int64_t *mini_pos_off, const uint64_t *mini_pos,
                                 int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *seg_a_off, chaindp_anchor_t *seg_a)
{
	return frag_post_impl(ctx, opt, n_seqs, n_segs_per_read, seg_len, rep_len, ref_len, n_ref, mini_pos_off, mini_pos, seg_regs_off, regs, regs_cap,
	                      seg_a_off, seg_a, -1);
}

static int map_frags_impl(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                          const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid,
                          const int32_t *qlen, const uint32_t *hash, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                          const int32_t *ref_len, int32_t n_ref, int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len,
                          int64_t *n_anchors, int pe_ori)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!opt || !seg_regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && (!hash || !n_segs_per_read))) {
		ctx->err = "NULL output, hash, n_segs_per_read or opt"; return CHAINDP_ERR_ARG;
	}
	// the stages of chaindp_map_batch with the reads' segment counts, the hits left in HBM, then the fragment post steps on them
	rc = map_prefix(ctx, ix, flag, max_occ, par, min_cnt, n_reads, mini_off, mini, bid, qlen, n_segs_per_read, hash, rep_len, n_anchors, nullptr, nullptr, 0);
	if (rc) return rc;
	return frag_post_impl(ctx, opt, n_seqs, n_segs_per_read, seg_len, nullptr, ref_len, n_ref, nullptr, nullptr, seg_regs_off, regs, regs_cap, nullptr, nullptr,
	                      pe_ori, qlen);
}

extern "C" int chaindp_map_frags(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt,
                                 const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid,
                                 const int32_t *qlen, const uint32_t *hash, int64_t n_seqs, const int32_t *n_segs_per_read, const int32_t *seg_len,
                                 const int32_t *ref_len, int32_t n_ref, int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len,
                                 int64_t *n_anchors)
{
	return map_frags_impl(ctx, ix, flag, max_occ, par, min_cnt, opt, n_reads, mini_off, mini, bid, qlen, hash, n_seqs, n_segs_per_read, seg_len, ref_len, n_ref,
	                      seg_regs_off, regs, regs_cap, rep_len, n_anchors, -1);
}

extern "C" int chaindp_map_frag_seqs(chaindp_ctx_t *ctx, const chaindp_index_t *ix, int w, int k, int is_hpc, int flag, int max_occ,
                                     const chaindp_params_t *par, int min_cnt, const chaindp_post_opt_t *opt, int pe_ori, int64_t n_reads, int64_t n_seqs,
                                     const int32_t *n_segs_per_read, const int64_t *seq_off, const char *seq, const uint32_t *bid, const uint32_t *hash,
                                     const int32_t *ref_len, int32_t n_ref, int64_t *seg_regs_off, chaindp_reg_t *regs, int64_t regs_cap, int32_t *rep_len,
                                     int64_t *n_anchors)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (!opt || !seg_regs_off || regs_cap < 0 || (regs_cap > 0 && !regs) || (n_reads > 0 && (!hash || !bid || !n_segs_per_read))) {
		ctx->err = "NULL output, bid, hash, n_segs_per_read or opt"; return CHAINDP_ERR_ARG;
	}
	if (pe_ori < -1 || pe_ori > 3) { ctx->err = "pe_ori must be -1 or 0..3"; return CHAINDP_ERR_ARG; }
	if (!ix || ix->device != ctx->device) { ctx->err = "index image missing or on another device"; return CHAINDP_ERR_ARG; }
	int64_t sum = 0;
	for (int64_t r = 0; r < n_reads; ++r) sum += n_segs_per_read[r] > 0 ? n_segs_per_read[r] : n_seqs + 1;
	if (sum != n_seqs) { ctx->err = "n_segs_per_read does not add up to n_seqs"; return CHAINDP_ERR_ARG; }
	std::vector<int64_t> mini_off((size_t)(n_reads > 0 ? n_reads + 1 : 1));
	if ((rc = sketch_impl(ctx, w, k, is_hpc, n_seqs, seq_off, seq, n_reads > 0 ? n_segs_per_read : nullptr, mini_off.data(), pe_ori)) != CHAINDP_OK) return rc;
	return map_frags_impl(ctx, ix, flag, max_occ, par, min_cnt, opt, n_reads, nullptr, nullptr, bid, nullptr, hash, n_seqs, n_segs_per_read, nullptr, ref_len, n_ref,
	                      seg_regs_off, regs, regs_cap, rep_len, n_anchors, pe_ori);
}
