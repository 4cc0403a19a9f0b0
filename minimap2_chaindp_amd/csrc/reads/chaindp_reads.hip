// reads/chaindp_reads.hip -- the end of mm_align_skeleton (reference align.c:758-759) over the pool of records chaindp_align_reads kept
// on the device: every region the chaindp_align1 rounds returned and every slot of the one chaindp_align1_inv call.
//
// The host (chaindp_reads_plan.h) lists, read by read and in pool order, the records that stand in a read's list, each with its place
// key; nothing here depends on the order they are listed in.
//   k_reads_keep     a round's regions and extras into pool records
//   k_reads_finish   a wave per read: the placed order by rank of the place key; mm_filter_regs (hit.c:249-268, max_clip_ratio 1.0);
//                    mm_hit_sort_by_dp (hit.c:167-193): nothing for a list of one, else cnt == 0 && !inv dropped and the rest ranked by
//                    dp_max << 32 | hash falling, of equal keys the later placed one first: radix_sort_128x's insertion sort for up to
//                    64 live records is stable, and the list is reversed behind it.  More than 64 live records with equal keys among
//                    them are flagged and their (key, place) pairs written out; the read's final regions and CIGAR words counted
//   k_reads_tied     a wave per flagged read: one lane takes the pairs through bt_radix_128x (chaindp_rsort.h, the digit tables in
//                    LDS), which leaves equal keys where the reference's in-place procedure does; the final order is that, reversed
//   k_reads_scan     the reads' counts to out_off and to the reads' first CIGAR word, one workgroup
//   k_reads_order    a wave per read: every final region's list index and its CIGAR offset
//   k_reads_gather   records and extras word by word, k_reads_gather_cig a wave per region: coalesced, grid-strided stores
// A list of up to lds_cap records is ranked in LDS (24 bytes a record), a longer one through the same code on global work arrays.
// Ranking is by counting: record i stands behind the records whose key is smaller, every lane counts for its own record while the
// wave reads record j from one address.  Lists of more than 64 records take more than one trip of the lanes.
#include "../chaindp_kernels.h"
#include "../chaindp_wave.h"
#include "../chaindp_post_dev.h"
#include "../chaindp_reads_plan.h"
#include "../chaindp_rsort.h"

namespace chaindp {

enum { RD_FILTERED = 0, RD_SOFT_DELETED = 1, RD_LIVE = 2 };      // a record's mark after mm_filter_regs: out; cnt == 0 && !inv; neither

__global__ __launch_bounds__(256) void k_reads_keep(int64_t n, const int32_t *__restrict__ regs, const int32_t *__restrict__ extra, int32_t *__restrict__ rec)
{
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * RD_REC_WORDS; i += (int64_t)gridDim.x * 256) {
		const int64_t g = i / RD_REC_WORDS;
		const int w = (int)(i - g * RD_REC_WORDS);
		rec[i] = w < AL_REG_WORDS ? regs[g * AL_REG_WORDS + w] : extra[g * 5 + (w - AL_REG_WORDS)];
	}
}

// mm_filter_regs' verdict on one record
__device__ __forceinline__ uint32_t reads_mark(const AlignOpt &o, int qlen, const int32_t *__restrict__ r)
{
	const uint32_t bits = (uint32_t)r[15];
	const int cnt = r[1];
	bool flt = !(bits & RD_BIT_INV) && !(bits & RD_BIT_SEG_SPLIT) && cnt < o.min_cnt;
	if (r[AL_REG_WORDS]) {                                                    // r->p
		const float clip = (float)qlen * 1.0f;                                // qlen * opt->max_clip_ratio
		if (r[11] < o.min_chain_score) flt = true;
		else if (r[AL_REG_WORDS + 2] < o.min_dp_max) flt = true;
		else if ((float)r[4] > clip && (float)(qlen - r[5]) > clip) flt = true;
	}
	return flt ? RD_FILTERED : (bits & RD_BIT_INV) || cnt > 0 ? RD_LIVE : RD_SOFT_DELETED;
}

// One read's list of n records, key[0..n) in listed order; it, k2, mk: n entries each of LDS or of global work memory.
template <typename KI, typename KO, typename I, typename M>
__device__ __forceinline__ void reads_finish_one(const AlignOpt &o, int lane, int n, int qlen, int64_t base, KI key, const int32_t *__restrict__ item,
                                                 const int32_t *__restrict__ rec, I it, KO k2, M mk, int32_t *__restrict__ placed, int32_t *__restrict__ final_order,
                                                 int32_t *cnt_out, int64_t *words_out, int32_t *tied_out, ulonglong2 *__restrict__ pairs)
{
	// the placed order, and at each place the record's verdict and sort key
	for (int i = lane; i < n; i += 64) {
		const unsigned long long ki = key[i];
		int rank = 0;
		for (int j = 0; j < n; ++j) rank += key[j] < ki;
		const int32_t *r = rec + (int64_t)item[base + i] * RD_REC_WORDS;
		it[rank] = (int32_t)(base + i);
		k2[rank] = (unsigned long long)(uint32_t)r[AL_REG_WORDS + 2] << 32 | (uint32_t)r[16];
		mk[rank] = reads_mark(o, qlen, r);
		placed[base + rank] = (int32_t)(base + i);
	}
	__syncthreads();
	int kept = 0;
	for (int p = lane; p < n; p += 64) kept += mk[p] != RD_FILTERED;
	kept = wave_sum_i(kept);
	const uint32_t live_from = kept <= 1 ? RD_SOFT_DELETED : RD_LIVE;        // mm_hit_sort_by_dp returns at once when n <= 1
	int n_final = 0, tie = 0;
	long long words = 0;
	for (int p = lane; p < n; p += 64) {
		if (mk[p] < live_from) continue;
		const unsigned long long kp = k2[p];
		int rank = 0;
		for (int q = 0; q < n; ++q) {
			const bool live = mk[q] >= live_from, same = k2[q] == kp;
			rank += live && (k2[q] > kp || (same && q > p));
			tie |= live && same && q != p;
		}
		final_order[base + rank] = it[p];
		++n_final;
		words += max(rec[(int64_t)item[it[p]] * RD_REC_WORDS + AL_REG_WORDS + 4], 0);
	}
	n_final = wave_sum_i(n_final);
	long long w64 = words;
	for (int d = 32; d; d >>= 1) w64 += __shfl_xor(w64, d);
	// the threshold is radix_sort_128x's, on the live records (n_aux): past it equal keys end where its in-place procedure leaves them
	const int tied = n_final > 64 && wave_sum_i(tie) != 0;
	if (tied)
		for (int p = lane; p < n; p += 64) {
			if (mk[p] < RD_LIVE) continue;
			int at = 0;
			for (int q = 0; q < p; ++q) at += mk[q] >= RD_LIVE;
			pairs[base + at] = make_ulonglong2(k2[p], (unsigned long long)p);     // the live records in placed order, as aux[] holds them
		}
	if (lane == 0) { *cnt_out = n_final; *words_out = w64; *tied_out = tied; }
}

__global__ __launch_bounds__(64) void k_reads_finish(AlignOpt o, ReadsDev d, int lds_cap)
{
	__shared__ unsigned long long s_key[RD_LDS_CAP], s_k2[RD_LDS_CAP];
	__shared__ uint32_t s_mk[RD_LDS_CAP];
	__shared__ int32_t s_it[RD_LDS_CAP];
	const int lane = threadIdx.x;
	for (int64_t r = blockIdx.x; r < d.n_reads; r += gridDim.x) {
		const int64_t base = d.list_off[r];
		const int n = (int)(d.list_off[r + 1] - base);
		const int qlen = (int)(d.seq_off[r + 1] - d.seq_off[r]);
		__syncthreads();                                                      // the read before is done with the LDS
		if (n <= lds_cap) {
			for (int i = lane; i < n; i += 64) s_key[i] = d.key[base + i];
			__syncthreads();
			reads_finish_one(o, lane, n, qlen, base, (unsigned long long*)s_key, d.item, d.rec, (int32_t*)s_it, (unsigned long long*)s_k2, (uint32_t*)s_mk,
			                 d.placed, d.final_order, d.cnt + r, d.words + r, d.tied + r, (ulonglong2*)d.pairs);
		} else {
			reads_finish_one(o, lane, n, qlen, base, (const unsigned long long*)(d.key + base), d.item, d.rec, d.src + base, d.sort_key + base,      // src: free until k_reads_order
			                 d.mark + base, d.placed, d.final_order, d.cnt + r, d.words + r, d.tied + r, (ulonglong2*)d.pairs);
		}
	}
}

// The reads k_reads_finish flagged: pairs[base .. base + cnt) are the live records' (key, place) in placed order and placed[] names the
// record at every place.  radix_sort_128x is sequential; the other lanes wait and then write the order out, last first.
__global__ __launch_bounds__(64) void k_reads_tied(ReadsDev d)
{
	__shared__ int32_t s_head[256], s_tail[256];
	const int lane = threadIdx.x;
	for (int64_t r = blockIdx.x; r < d.n_reads; r += gridDim.x) {
		if (!d.tied[r]) continue;
		const int64_t base = d.list_off[r];
		const int m = d.cnt[r];
		ulonglong2 *a = (ulonglong2*)d.pairs + base;
		if (lane == 0) bt_radix_128x(a, m, (BtRange*)d.stack + base / 65 + 2 * r, s_head, s_tail);
		__syncthreads();
		for (int i = lane; i < m; i += 64) d.final_order[base + m - 1 - i] = d.placed[base + (int64_t)a[i].y];
		__syncthreads();
	}
}

// exclusive running sums of the reads' counts, one workgroup: 256 reads a trip, the carry in LDS
__global__ __launch_bounds__(256) void k_reads_scan(ReadsDev d)
{
	__shared__ long long s_c[256], s_w[256];
	__shared__ long long carry[2];
	const int t = threadIdx.x;
	if (t == 0) carry[0] = carry[1] = 0;
	__syncthreads();
	for (int64_t r0 = 0; r0 < d.n_reads; r0 += 256) {
		const int64_t r = r0 + t;
		const long long c = r < d.n_reads ? d.cnt[r] : 0, w = r < d.n_reads ? d.words[r] : 0;
		s_c[t] = c; s_w[t] = w;
		__syncthreads();
		for (int k = 1; k < 256; k <<= 1) {
			const long long ac = t >= k ? s_c[t - k] : 0, aw = t >= k ? s_w[t - k] : 0;
			__syncthreads();
			s_c[t] += ac; s_w[t] += aw;
			__syncthreads();
		}
		if (r < d.n_reads) { d.out_off[r] = carry[0] + s_c[t] - c; d.word_off[r] = carry[1] + s_w[t] - w; }
		__syncthreads();
		if (t == 255) { carry[0] += s_c[255]; carry[1] += s_w[255]; }
		__syncthreads();
	}
	if (t == 0) {
		d.out_off[d.n_reads] = carry[0]; d.word_off[d.n_reads] = carry[1];
		d.need[0] = carry[0]; d.need[1] = carry[1];
		d.cigar_off[carry[0]] = carry[1];
	}
}

__global__ __launch_bounds__(64) void k_reads_order(ReadsDev d)
{
	const int lane = threadIdx.x;
	for (int64_t r = blockIdx.x; r < d.n_reads; r += gridDim.x) {
		const int64_t base = d.list_off[r], f0 = d.out_off[r];
		const int n = d.cnt[r];
		int64_t at = d.word_off[r];
		for (int p0 = 0; p0 < n; p0 += 64) {
			const int p = p0 + lane;
			int k = 0, m = 0;
			if (p < n) { k = d.final_order[base + p]; m = max(d.rec[(int64_t)d.item[k] * RD_REC_WORDS + AL_REG_WORDS + 4], 0); }
			int incl = m;
			for (int s = 1; s < 64; s <<= 1) { const int v = __shfl_up(incl, s); if (lane >= s) incl += v; }
			if (p < n) { d.src[f0 + p] = k; d.cigar_off[f0 + p] = at + incl - m; }
			at += __shfl(incl, 63);
		}
	}
}

__global__ __launch_bounds__(256) void k_reads_gather(ReadsDev d)
{
	const int64_t total = d.need[0];
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total * RD_REC_WORDS; i += (int64_t)gridDim.x * 256) {
		const int64_t f = i / RD_REC_WORDS;
		const int w = (int)(i - f * RD_REC_WORDS);
		const int32_t v = d.rec[(int64_t)d.item[d.src[f]] * RD_REC_WORDS + w];
		if (w < AL_REG_WORDS) d.out_regs[f * AL_REG_WORDS + w] = v;
		else d.out_extra[f * 5 + (w - AL_REG_WORDS)] = v;
	}
}

// a wave per final region: a CIGAR is a few words to a few hundred
__global__ __launch_bounds__(64) void k_reads_gather_cig(ReadsDev d)
{
	const int64_t total = d.need[0];
	for (int64_t f = blockIdx.x; f < total; f += gridDim.x) {
		const int k = d.src[f];
		const int64_t m = d.cigar_off[f + 1] - d.cigar_off[f];
		const uint32_t *from = d.cig + d.cig_at[k];
		uint32_t *to = d.out_cig + d.cigar_off[f];
		for (int64_t c = threadIdx.x; c < m; c += 64) to[c] = from[c];
	}
}

static unsigned reads_grid(int64_t n) { return (unsigned)(n < 1 ? 1 : n < 65536 ? n : 65536); }

hipError_t launch_reads_keep(hipStream_t st, int64_t n, const int32_t *d_regs, const int32_t *d_extra, int32_t *d_rec)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_reads_keep, dim3(reads_grid((n * RD_REC_WORDS + 255) / 256)), dim3(256), 0, st, n, d_regs, d_extra, d_rec);
	return hipGetLastError();
}

hipError_t launch_reads_finish(hipStream_t st, const AlignOpt &o, const ReadsDev &d, int lds_cap)
{
	if (d.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_reads_finish, dim3(reads_grid(d.n_reads)), dim3(64), 0, st, o, d, lds_cap < RD_LDS_CAP ? lds_cap : RD_LDS_CAP);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_reads_tied, dim3(reads_grid(d.n_reads)), dim3(64), 0, st, d);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(k_reads_scan, dim3(1), dim3(256), 0, st, d);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(k_reads_order, dim3(reads_grid(d.n_reads)), dim3(64), 0, st, d);
	return hipGetLastError();
}

hipError_t launch_reads_gather(hipStream_t st, const ReadsDev &d)
{
	if (d.n_listed <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_reads_gather, dim3(reads_grid((d.n_listed * RD_REC_WORDS + 255) / 256)), dim3(256), 0, st, d);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_reads_gather_cig, dim3(reads_grid(d.n_listed)), dim3(64), 0, st, d);
	return hipGetLastError();
}

} // namespace chaindp
