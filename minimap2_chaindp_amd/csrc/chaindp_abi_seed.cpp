// chaindp_abi_seed.cpp -- seed collection on the GPU (chaindp_seed.hip): the index image's upload, minimizers in, sorted anchors
// resident; chaindp_map_batch and the prefix every map call opens with.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

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
int chaindp::seed_reserve(chaindp_ctx *ctx, int64_t n_mini, bool oom_is_capacity)
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
int chaindp::collect_seeds_impl(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, int64_t n_reads,
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
		HIP_TRY(ctx, chaindp::launch_gather_reads(st, n_reads, ctx->d_mini_off, (const void *const *)ctx->ptrs.p, ctx->d_mini));
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
	ctx->from_sketch = resident;
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
int chaindp::map_prefix(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt, int64_t n_reads,
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
	if ((rc = check_read_gaps(ctx, n_reads)) != CHAINDP_OK) return rc;
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
	HIP_TRY(ctx, chaindp::launch_scatter_words(ctx->stream, n_reads, ctx->d_mp_off, (void *const *)ctx->ptrs.p, ctx->d_mini_pos));
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
