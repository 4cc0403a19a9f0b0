// chaindp_abi_sketch.cpp -- sketch on the GPU (chaindp_sketch.hip): bases in, minimizers resident.
#include <string.h>
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

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
	// the bases of the last sketch go with their buffer: nothing may take them for resident from here on, whether or not the new
	// buffers can be had (chaindp_align_resident reads sk.seq long after the sketch has finished)
	ctx->sk_valid = false; ctx->from_sketch = false; ctx->post_n_reads = -1;
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
int chaindp::sketch_impl(chaindp_ctx *ctx, int w, int k, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const char *seq,
                       const int32_t *n_segs_per_read, int64_t *mini_off, int pe_ori, int64_t rid_base)
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
