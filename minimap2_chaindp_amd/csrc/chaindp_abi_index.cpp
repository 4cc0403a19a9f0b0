// chaindp_abi_index.cpp -- the index image built on the device (chaindp_index.hip): target bases in, B/H/V/P resident.
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "chaindp_ctx.h"

using namespace chaindp;

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
