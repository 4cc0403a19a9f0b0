// chaindp_abi.cpp -- host side of the C ABI declared in include/chaindp.h.
// Owns the per-GPU context (stream, HBM buffers, scratch), stages batches and launches the kernels
// of chaindp_kernels.hip / chaindp_compact.hip.  No CPU implementation of the DP exists in this
// library: without a GPU every entry point fails with CHAINDP_ERR_NODEVICE.
// This file: the context's lifetime and setters, the helpers every stage uses, prepass + DP, upload / run / download, compaction,
// gather / scatter, profiling and the DP's test hooks.  The later stages have a file each (chaindp_abi_*.cpp); chaindp_ctx.h is
// what they share.
#include <stdlib.h>
#include "chaindp_ctx.h"

using namespace chaindp;

thread_local std::string chaindp::g_create_error;

// A first-use group of buffers, all or nothing: an out-of-memory half way leaves the context as it was (what this attempt allocated
// is freed again and the next call tries anew) instead of half-initialised with kernels launched on null scratch pointers.
int chaindp::first_use(chaindp_ctx *ctx, bool &ready, const char *what, std::initializer_list<chaindp::DevBuf> bufs)
{
	if (ready) return CHAINDP_OK;
	const hipError_t e = (hipError_t)ctx->pool.alloc_group(bufs);
	if (e != hipSuccess) { ctx->err = std::string(what) + " buffers: " + hipGetErrorString(e); return CHAINDP_ERR_HIP; }
	ready = true;
	return CHAINDP_OK;
}

// grow-only device buffer with a quarter of slack; a failed growth leaves the old buffer and its capacity
hipError_t chaindp::dev_grow(chaindp_ctx *ctx, DevGrow &g, size_t need)
{
	return (hipError_t)ctx->pool.reserve(g, need, need + need / 4, false);
}

// A new batch is resident (or, with 0 reads, none): what the calls on the one before left is no longer of this batch.
void chaindp::begin_batch(chaindp_ctx *ctx, int64_t n_reads, int64_t total, bool mp_resident)
{
	ctx->n_reads = n_reads; ctx->total = total; ctx->ran = false; ctx->ran_gaps = false; ctx->bot_n_reads = -1; ctx->mp_resident = mp_resident;
	ctx->post_n_reads = -1; ctx->from_sketch = false;
}

// the batch's per-read segment counts, if it has any, on the stream that carries its upload
hipError_t chaindp::stage_n_segs(chaindp_ctx *ctx, const int32_t *n_segs_per_read, int64_t n_reads, hipStream_t st)
{
	ctx->has_n_segs = n_segs_per_read != nullptr;
	if (!n_segs_per_read || !n_reads) return hipSuccess;
	return hipMemcpyAsync(ctx->d_n_segs, n_segs_per_read, (size_t)n_reads * 4, hipMemcpyHostToDevice, st);
}

// Profiling bracket around a launch: n events at consecutive kernel boundaries, their times added to ms[slot0...].  prof_begin
// records the first, prof_mark the k-th; the last one queues the set for chaindp_get_kernel_ms.  Nothing happens while profiling is off.
hipError_t chaindp::prof_begin(chaindp_ctx *ctx, EventSet &es, int n, int slot0, hipStream_t st)
{
	es.n = 0; es.slot0 = slot0;
	if (!ctx->prof) return hipSuccess;
	for (int k = 0; k < n; ++k) if (hipError_t e = hipEventCreate(&es.e[k])) return e;
	es.n = n;
	return hipEventRecord(es.e[0], st);
}

hipError_t chaindp::prof_mark(chaindp_ctx *ctx, EventSet &es, int k, hipStream_t st)
{
	if (!es.n) return hipSuccess;
	const hipError_t e = hipEventRecord(es.e[k], st);
	if (e == hipSuccess && k == es.n - 1) ctx->pending.push_back(es);
	return e;
}

Params chaindp::to_params(const chaindp_params_t *p)
{
	Params q;
	q.max_dist_x = p->max_dist_x; q.max_dist_y = p->max_dist_y; q.bw = p->bw; q.max_skip = p->max_skip;
	q.min_sc = p->min_sc; q.is_cdna = p->is_cdna; q.n_segs = p->n_segs;
	return q;
}

int chaindp::check_params(chaindp_ctx *ctx, const chaindp_params_t *par)
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

// The one-call functions open with this, before anything is launched; chaindp_run checks the resident batch the same way.
int chaindp::check_read_gaps(chaindp_ctx *ctx, int64_t n_reads)
{
	if (ctx->gaps_n < 0 || ctx->gaps_n == n_reads) return CHAINDP_OK;
	ctx->err = "per-read gaps are in force for another number of reads (chaindp_set_read_gaps)";
	return CHAINDP_ERR_ARG;
}

// map.c:358-366 for every read, in the reference's int arithmetic
extern "C" void chaindp_read_gaps(int32_t max_gap, int32_t max_gap_ref, int32_t max_frag_len, int32_t is_sr, int64_t n_reads,
                                  const int32_t *qlen_sum, int32_t *gap_ref, int32_t *gap_qry)
{
	for (int64_t r = 0; r < n_reads; ++r) {
		const int q = qlen_sum[r];
		int g_qry, g_ref;
		if (is_sr) g_qry = q > max_gap ? q : max_gap;
		else g_qry = max_gap;
		if (max_gap_ref > 0) g_ref = max_gap_ref;
		else if (max_frag_len > 0) {
			g_ref = (int)((unsigned)max_frag_len - (unsigned)q);     // (the reference's int subtraction; wraps instead of overflowing)
			if (g_ref < max_gap) g_ref = max_gap;
		} else g_ref = max_gap;
		if (gap_ref) gap_ref[r] = g_ref;
		if (gap_qry) gap_qry[r] = g_qry;
	}
}

extern "C" int chaindp_set_read_gaps(chaindp_ctx_t *ctx, int64_t n_reads, const int32_t *gap_ref, const int32_t *gap_qry)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (n_reads == 0 && !gap_ref && !gap_qry) { ctx->gaps_n = -1; return CHAINDP_OK; }      // cleared: par's gaps again
	if (n_reads < 0 || (n_reads > 0 && (!gap_ref || !gap_qry))) { ctx->err = "chaindp_set_read_gaps: NULL gap array or negative read count"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads) { ctx->err = "chaindp_set_read_gaps: more reads than the context was created for"; return CHAINDP_ERR_ARG; }
	std::vector<int32_t> g((size_t)n_reads * 2);
	for (int64_t r = 0; r < n_reads; ++r) {
		if (gap_ref[r] < 0 || gap_qry[r] < 0) { ctx->err = "chaindp_set_read_gaps: gaps must be >= 0"; return CHAINDP_ERR_ARG; }   // as check_params
		g[(size_t)r * 2] = gap_ref[r]; g[(size_t)r * 2 + 1] = gap_qry[r];
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t need = (size_t)n_reads * 8;
	if (need > ctx->gaps_set.cap) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));           // a run's copy out of the old buffer may be in flight
		HIP_TRY(ctx, dev_grow(ctx, ctx->gaps_set, need));
	}
	ctx->gaps_n = -1;                                              // (an error below leaves none in force)
	if (need) HIP_TRY(ctx, hipMemcpyAsync(ctx->gaps_set.p, g.data(), need, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->gaps_n = n_reads;
	return CHAINDP_OK;
}

// What every upload checks of an incoming batch before it touches the device; the text goes to err (a pipe reports into its own) and
// the batch's anchors to total.  per_read: payload is the list of the reads' own arrays, needed as soon as there are reads (what each
// read holds is the caller's loop to check); else the one array of all anchors, needed when there are any.  owner: "context" or "pipe".
int chaindp::check_batch(const chaindp_ctx *ctx, int64_t n_reads, const int64_t *off, const void *payload, bool per_read, const char *owner,
                         std::string &err, int64_t &total)
{
	if (n_reads < 0 || !off || (n_reads > 0 && (off[0] != 0 || (per_read && !payload)))) { err = "bad offsets"; return CHAINDP_ERR_ARG; }
	total = n_reads > 0 ? off[n_reads] : 0;
	if (!per_read && (total < 0 || (total > 0 && !payload))) { err = "bad anchors"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) {
		err = std::string("batch exceeds the capacity the ") + owner + " was created with";
		return CHAINDP_ERR_CAPACITY;
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

// The rest of DpDevice: the CU count, the stamp buffers of the diagnostic runs that were asked for, and what holds for every DP
// kernel instantiation on this device -- no static LDS, and room for the most dynamic LDS a launch can ask for.  what: the
// kernel an error is about.
static hipError_t dp_device_init(chaindp_ctx *ctx, bool twin_stamp, bool dense_stamp, std::string &what)
{
	DpDevice &d = ctx->dp;
	hipError_t e = hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
	if (e != hipSuccess) return e;
	if (twin_stamp) e = (hipError_t)ctx->pool.alloc((void**)&d.twin_stamp, twin_stamp_bytes(d.cus));
	if (e == hipSuccess && dense_stamp) e = (hipError_t)ctx->pool.alloc((void**)&d.dense_stamp, 16 * sizeof(unsigned long long));
	if (e != hipSuccess) return e;
	DpKernel k[CHAINDP_DP_KERNELS];
	int n = twin_kernels(k);
	n += units_kernels(k + n); n += dense_kernels(k + n); n += dense16_kernels(k + n); n += dense1_kernels(k + n);
	for (int i = 0; i < n; ++i) {
		hipFuncAttributes fa;
		e = hipFuncGetAttributes(&fa, k[i].fn);
		if (e == hipSuccess && fa.sharedSizeBytes != 0) e = hipErrorInvalidConfiguration;   // static LDS in front of the dynamic segment
		if (e == hipSuccess && k[i].max_lds > 64 * 1024) e = hipFuncSetAttribute(k[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k[i].max_lds);
		if (e != hipSuccess) { what = std::string(k[i].name) + ": "; return e; }
	}
	return hipSuccess;
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
	ctx->deep_handover = getenv("CHAINDP_NO_DEEP_HANDOVER") == nullptr;      // diagnostic switches are read here, once per context:
	if (const char *v = getenv("CHAINDP_TWIN_FORCE_LEFT")) ctx->twin_force_left = atoi(v) == 2 ? 2 : 1;   // never on the launch path (contexts run from several host threads)
	if (const char *v = getenv("CHAINDP_SKETCH_MAX_BASES")) { const long long m = atoll(v); if (m >= 0 && m < ctx->sk_max_bases) ctx->sk_max_bases = m; }
	if (const char *v = getenv("CHAINDP_TWIN_WG_PER_CU")) ctx->dp.twin_wg_per_cu = atoi(v);
	std::string what;
	if (e == hipSuccess) e = dp_device_init(ctx, getenv("CHAINDP_TWIN_STAMP") != nullptr, getenv("CHAINDP_DENSE_STAMP") != nullptr, what);
	if (e != hipSuccess) {
		g_create_error = std::string("chaindp_create: ") + what + hipGetErrorString(e);
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
                         int32_t *d_f, int32_t *d_p, int32_t *d_v, hipStream_t st, bool use_gaps = false)
{
	int rc = check_params(ctx, par);
	if (rc) return rc;
	if (use_gaps && (rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
	if (n_reads < 0 || total < 0) { ctx->err = "negative batch size"; return CHAINDP_ERR_ARG; }
	if (n_reads > ctx->cap_reads || total > ctx->cap_anchors) {
		ctx->err = "batch exceeds the capacity the context was created with";
		return CHAINDP_ERR_CAPACITY;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const Params q = to_params(par);
	// per-read gaps: the run keeps a copy of its own, so that setting or clearing gaps afterwards changes nothing for the stages behind it
	const int2 *d_gaps = nullptr;
	if (use_gaps && n_reads > 0) {
		const size_t need = (size_t)n_reads * 8;
		if (need > ctx->gaps_ran.cap) {
			HIP_TRY(ctx, hipStreamSynchronize(st));
			HIP_TRY(ctx, dev_grow(ctx, ctx->gaps_ran, need));
		}
		HIP_TRY(ctx, hipMemcpyAsync(ctx->gaps_ran.p, ctx->gaps_set.p, need, hipMemcpyDeviceToDevice, st));
		d_gaps = (const int2*)ctx->gaps_ran.p;
	}
	EventSet es;
	HIP_TRY(ctx, prof_begin(ctx, es, 3, 0, st));
	HIP_TRY(ctx, chaindp::launch_prepass(st, q, n_reads, total, d_off, d_a, ctx->d_sumq, ctx->d_units, ctx->d_counters, ctx->pre, ctx->d_unit_aux, d_n_segs, ctx->d_left_cnt, d_gaps));
	HIP_TRY(ctx, prof_mark(ctx, es, 1, st));
	// per-read gap-cost table for the fast variant (skipped when the table would not apply)
	uint16_t *lut = nullptr;
	int lut_stride = 0;
	if (ctx->use_lut && !q.is_cdna && q.bw <= CHAINDP_LUT_MAX_BW && n_reads > 0) {
		lut_stride = (q.bw + 1 + 7) & ~7;
		const size_t need = (size_t)n_reads * lut_stride * sizeof(uint16_t);
		if (need > ctx->lut.cap) {
			HIP_TRY(ctx, hipStreamSynchronize(st));
			HIP_TRY(ctx, (hipError_t)ctx->pool.reserve(ctx->lut, need, need, true));
		}
		lut = (uint16_t*)ctx->lut.p;
		HIP_TRY(ctx, chaindp::launch_lut(st, q, n_reads, d_off, ctx->d_sumq, lut_stride, lut));
	}
	if (++ctx->epoch == 0) {                                       // 2^32 runs: start the mark epochs over
		HIP_TRY(ctx, hipMemsetAsync(ctx->d_tg, 0, (size_t)ctx->cap_anchors * 8, st));
		ctx->epoch = 1;
	}
	// (the hand-over words -- counts, queue words, the route flag -- were zeroed by the prepass' first kernel;
	// first_child[] is initialised by the DP kernels themselves, per tile: no batch-wide memset)
	DpBatch b;
	b.st = st; b.par = q; b.total = total;
	b.off = d_off; b.a = d_a; b.n_segs = d_n_segs; b.gaps = d_gaps; b.sumq = ctx->d_sumq; b.lut = lut; b.lut_stride = lut_stride;
	b.units = ctx->d_units; b.aux = ctx->d_unit_aux; b.counters = ctx->d_counters;
	b.f = d_f; b.p = d_p; b.v = d_v; b.first_child = ctx->d_first_child; b.flags = ctx->cmp.flags; b.tg = ctx->d_tg; b.epoch = ctx->epoch;
	b.left = ctx->d_left; b.deep = ctx->deep_handover ? ctx->d_deep : nullptr; b.hw = HandoverWords{ctx->d_left_cnt};
	b.key_range = ctx->pre.key_range; b.long_units = ctx->pre.hist + CHAINDP_LONG_UNIT_CLASS; b.twin_queue = ctx->d_twin_queue;
	b.force_left = ctx->twin_force_left; b.two_tables = ctx->twin_two_tables; b.deep_eager = ctx->deep_eager; b.deep_route = ctx->deep_route;
	// ordinary units two per wave (both layouts are launched, the device decides); what that kernel hands over, and nothing else,
	// goes through k_chain_units
	// a batch with per-read gaps is k_chain_units' alone: the whole list in one launch, every unit kept to its end
	if (d_gaps) b.deep = nullptr;
	const bool twin = ctx->variant == 0 && lut && !d_gaps;
	if (twin) HIP_TRY(ctx, chaindp::launch_chain_twin(ctx->dp, b));
	HIP_TRY(ctx, chaindp::launch_chain(b, ctx->ring, twin));
	// units whose scans kept reaching past the ring (dense repeats): redone by the dense kernels
	if (b.deep && lut) {
		HIP_TRY(ctx, chaindp::launch_chain_dense(ctx->dp, b));
		HIP_TRY(ctx, chaindp::launch_chain_dense16(ctx->dp, b));
		HIP_TRY(ctx, chaindp::launch_chain_dense1(ctx->dp, b));
	}
	HIP_TRY(ctx, prof_mark(ctx, es, 2, st));
	ctx->stats[2] = total; ctx->stats[3] = n_reads;
	return CHAINDP_OK;
}

extern "C" int chaindp_upload(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *off, const chaindp_anchor_t *a,
                              const int32_t *n_segs_per_read)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int64_t total = 0;
	if (int rc = check_batch(ctx, n_reads, off, a, false, "context", ctx->err, total)) return rc;
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
	                       ctx->d_f, ctx->d_p, ctx->d_v, ctx->stream, ctx->gaps_n >= 0);
	if (rc == CHAINDP_OK) { ctx->ran = true; ctx->singles_pending = true; ctx->ran_par = *par; ctx->ran_gaps = ctx->gaps_n >= 0 && ctx->n_reads > 0; }
	return rc;
}

extern "C" int chaindp_run_device(chaindp_ctx_t *ctx, const chaindp_params_t *par, int64_t n_reads, int64_t total_anchors,
                                  const void *d_off, const void *d_a, const void *d_n_segs,
                                  void *d_f, void *d_p, void *d_v, void *stream)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!d_off || (total_anchors > 0 && (!d_a || !d_f || !d_p || !d_v))) { ctx->err = "NULL device pointer"; return CHAINDP_ERR_ARG; }
	if (ctx->gaps_n >= 0) { ctx->err = "chaindp_run_device takes no per-read gaps: clear them (the batch is the caller's)"; return CHAINDP_ERR_ARG; }
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
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
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

// test hook (not in the public header): units the two-per-wave kernel handed over to k_chain_units in the last run.  When that
// kernel declines the whole batch (long units: map-ont, dense repeats) the word on the device is the marker 0xffffffff, "every
// unit": reported as the batch's unit count
extern "C" int64_t chaindp_debug_leftover(chaindp_ctx_t *ctx)
{
	if (!ctx || !ctx->d_left_cnt) return -1;
	unsigned long long c = 0, cnt = 0;
	if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipMemcpy(&c, HandoverWords{ctx->d_left_cnt}.left_word(), sizeof(c), hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(&cnt, ctx->d_counters, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	return (uint32_t)c == 0xffffffffu ? (int64_t)(uint32_t)cnt : (int64_t)(uint32_t)c;
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
// half, 0 neither (the twin kernel declined the batch as a whole, or did not run)
extern "C" int chaindp_debug_twin_tables(chaindp_ctx_t *ctx)
{
	if (!ctx || !ctx->d_left_cnt) return -1;
	unsigned long long r = 0;
	if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipMemcpy(&r, HandoverWords{ctx->d_left_cnt}.route_word(), sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) return -1;
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
	    hipMemcpy(&c, HandoverWords{ctx->d_left_cnt}.deep_word(), sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return -1;
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
	case 7: src = ctx->regs.p; break;           // what chaindp_gen_regs left resident
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
int chaindp::stage_pointers(chaindp_ctx *ctx, const void *const *ptrs, int64_t n)
{
	if ((size_t)n * sizeof(void*) > ctx->ptrs.cap) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		const size_t cap = (size_t)n + (size_t)n / 2 + 64;
		HIP_TRY(ctx, (hipError_t)ctx->pool.reserve(ctx->ptrs, (size_t)n * sizeof(void*), cap * sizeof(void*), true));
	}
	if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->ptrs.p, ptrs, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
	return CHAINDP_OK;
}

extern "C" int chaindp_upload_gather_ex(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *off,
                                        const chaindp_anchor_t *const *read_anchors, const int32_t *n_segs_per_read, int pinned)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	if (!pinned) return chaindp_upload_gather(ctx, n_reads, off, read_anchors, n_segs_per_read);
	int64_t total = 0;
	if (int rc = check_batch(ctx, n_reads, off, read_anchors, true, "context", ctx->err, total)) return rc;
	for (int64_t r = 0; r < n_reads; ++r)
		if (off[r + 1] < off[r] || (off[r + 1] > off[r] && !read_anchors[r])) { ctx->err = "bad read in gather list"; return CHAINDP_ERR_ARG; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
	int rc = stage_pointers(ctx, (const void *const *)read_anchors, n_reads);
	if (rc) return rc;
	HIP_TRY(ctx, chaindp::launch_gather_reads(ctx->stream, n_reads, ctx->d_off, (const void *const *)ctx->ptrs.p, ctx->d_a));
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
	HIP_TRY(ctx, chaindp::launch_scatter_seeds(ctx->stream, n_reads, ctx->d_seeds_off, (void *const *)ctx->ptrs.p, ctx->d_seeds));
	return CHAINDP_OK;
}

extern "C" int chaindp_upload_gather(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *off,
                                     const chaindp_anchor_t *const *read_anchors, const int32_t *n_segs_per_read)
{
	if (!ctx) return CHAINDP_ERR_ARG;
	int64_t total = 0;
	if (int rc = check_batch(ctx, n_reads, off, read_anchors, true, "context", ctx->err, total)) return rc;
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
