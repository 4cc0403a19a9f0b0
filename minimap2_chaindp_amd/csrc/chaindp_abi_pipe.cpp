// chaindp_abi_pipe.cpp -- streaming pipeline (include/chaindp.h): depth contexts, each with its own stream, round robin.
#include <stdlib.h>
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

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
	int64_t total = 0;
	if ((rc = check_batch(ctx, n_reads, off, a, false, "pipe", pipe->err, total)) != CHAINDP_OK) return rc;
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
