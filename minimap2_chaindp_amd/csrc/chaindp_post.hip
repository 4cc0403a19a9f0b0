// chaindp_post.hip -- what the reference does with a read's hits after mm_gen_regs when nothing is aligned (MM_F_CIGAR unset,
// one segment): chain_post (map.c:238-247: mm_set_parent, mm_select_sub, mm_join_long) and mm_set_mapq (hit.c:437-480), over the
// hits chaindp_gen_regs left in HBM.  mm_est_err sits between the two (map.c:872) and is k_regs_div of chaindp_regs.hip, run on
// this file's output and the anchors as chain_post left them.
//
//   k_post_read     one wave (and one workgroup) per read.  The hits' mutable fields are staged as one int array per field, in LDS
//                   for reads of up to POST_LDS_CAP hits and in a global scratch area (the same code through the same generic
//                   pointers) above.  mm_set_parent's outer loop is sequential; its scan of the primaries is spread over the lanes
//                   (the overlapping ones gathered in w order by ballot, the length of their union without a sort, the first one
//                   that passes the mask test by the lowest lane of a ballot).  mm_select_sub, the join walk of mm_join_long, its
//                   parent fix-up and mm_filter_regs are the reference's in-place loops, run by every lane in step (every lane
//                   computes and stores the same values, so no lane waits for another).  mm_squeeze_a, mm_sync_regs and the fuzzy
//                   lengths of a joined chain use the whole wave.  Output: the read's hits at the positions its input occupied
//                   (slot k at chains_off[r] + k), their count, and the read's anchors as chain_post leaves them.
//   (scan)          exclusive scan of the counts: the CSR offsets of the output (launch_scan_u64)
//   k_post_scatter  wave per read: packs the records
//   k_post_mapq     wave per read, lane per hit: mm_set_mapq with the r->p == NULL branch; sum_sc by a wave reduction.
//
// Types and order of operations follow the reference (float where it computes in float, the one double add of sc_thres, float
// division that rounds correctly -- hipcc's default).  logf of an integer is the host's (post_logf_int).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "chaindp_kernels.h"
#include "chaindp_wave.h"
#include "chaindp_post_dev.h"

namespace chaindp {

template <bool IN_LDS>
__device__ void post_read(int64_t r, const int64_t *__restrict__ chains_off, const int64_t *__restrict__ b_off, const ulonglong2 *__restrict__ b,
                          const int32_t *__restrict__ regs, const int32_t *__restrict__ qlen, PostOpt o, int32_t *__restrict__ scratch,
                          int32_t *__restrict__ stage, ulonglong2 *__restrict__ sq, unsigned long long *__restrict__ n_out, int *lds)
{
	const int lane = threadIdx.x & 63;
	const int64_t c0 = chains_off[r];
	const int n0 = (int)(chains_off[r + 1] - c0);
	const int64_t a0 = b_off[r];
	const int n_b = (int)(b_off[r + 1] - a0);
	PostFields F;
	if (IN_LDS) { F.base = lds; F.stride = POST_LDS_CAP; }
	else { F.base = scratch + c0 * PF_NF; F.stride = n0; }
	const int32_t *in = regs + c0 * 20;
	for (int s = lane; s < n0; s += 64) {
		const int32_t *g = in + s * 20;
		F(PF_ID, s) = g[0]; F(PF_CNT, s) = g[1]; F(PF_RID, s) = g[2]; F(PF_SCORE, s) = g[3]; F(PF_QS, s) = g[4]; F(PF_QE, s) = g[5];
		F(PF_RS, s) = g[6]; F(PF_RE, s) = g[7]; F(PF_PARENT, s) = g[8]; F(PF_SUBSC, s) = g[9]; F(PF_AS, s) = g[10]; F(PF_MLEN, s) = g[11];
		F(PF_BLEN, s) = g[12]; F(PF_NSUB, s) = g[13]; F(PF_BITS, s) = g[15]; F(PF_ORIG, s) = s;
	}
	__syncthreads();
	int n = n0;
	const ulonglong2 *ba = b + a0;
	ulonglong2 *sa = sq + a0;
	if (!(o.flag & POST_F_ALL_CHAINS)) {                                 // chain_post, map.c:238-247
		post_set_parent(F, n, o.mask_level, lane);
		n = post_select_sub(F, n, o.pri_ratio, o.min_diff, o.best_n, lane);
		if (!(o.flag & (POST_F_SPLICE | POST_F_SR | POST_F_NO_LJOIN))) n = post_join_long(F, n, o, qlen[r], ba, sa, n_b, lane);
		else for (int t = lane; t < n_b; t += 64) sa[t] = ba[t];
	} else {
		for (int t = lane; t < n_b; t += 64) sa[t] = ba[t];
	}
	for (int s = lane; s < n; s += 64) {
		const int32_t *g = in + F(PF_ORIG, s) * 20;
		int32_t *d = stage + (c0 + s) * 20;
		d[0] = F(PF_ID, s); d[1] = F(PF_CNT, s); d[2] = F(PF_RID, s); d[3] = F(PF_SCORE, s); d[4] = F(PF_QS, s); d[5] = F(PF_QE, s);
		d[6] = F(PF_RS, s); d[7] = F(PF_RE, s); d[8] = F(PF_PARENT, s); d[9] = F(PF_SUBSC, s); d[10] = F(PF_AS, s); d[11] = F(PF_MLEN, s);
		d[12] = F(PF_BLEN, s); d[13] = F(PF_NSUB, s); d[14] = g[14]; d[15] = F(PF_BITS, s); d[16] = g[16]; d[17] = g[17]; d[18] = g[18]; d[19] = g[19];
	}
	if (lane == 0) n_out[r] = (unsigned long long)n;
}

__global__ __launch_bounds__(64) void k_post_read(int64_t n_reads, const int64_t *__restrict__ chains_off, const int64_t *__restrict__ b_off,
                                                  const ulonglong2 *__restrict__ b, const int32_t *__restrict__ regs, const int32_t *__restrict__ qlen,
                                                  PostOpt o, int32_t *__restrict__ scratch, int32_t *__restrict__ stage, ulonglong2 *__restrict__ sq,
                                                  unsigned long long *__restrict__ n_out)
{
	__shared__ int lds[PF_NF * POST_LDS_CAP];
	const int64_t r = blockIdx.x;
	if (r >= n_reads) return;
	const int64_t n = chains_off[r + 1] - chains_off[r];
	if (n <= POST_LDS_CAP) post_read<true>(r, chains_off, b_off, b, regs, qlen, o, scratch, stage, sq, n_out, lds);
	else post_read<false>(r, chains_off, b_off, b, regs, qlen, o, scratch, stage, sq, n_out, lds);
}

__global__ __launch_bounds__(256) void k_post_scatter(int64_t n_reads, const int64_t *__restrict__ chains_off, const unsigned long long *__restrict__ out_off,
                                                      const int32_t *__restrict__ stage, int32_t *__restrict__ out)
{
	const int lane = threadIdx.x & 63;
	const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (r >= n_reads) return;
	const int64_t o0 = (int64_t)out_off[r], words = ((int64_t)out_off[r + 1] - o0) * 20;
	const int32_t *src = stage + chains_off[r] * 20;
	int32_t *dst = out + o0 * 20;
	for (int64_t t = lane; t < words; t += 64) dst[t] = src[t];
}

// mm_set_mapq (hit.c:437-480) with r->p == NULL; mm_set_inv_mapq is a no-op here (no hit has its inv bit without alignment, and
// the inv branch is kept for completeness).  err: set when a logf argument lies beyond the patch list.
__global__ __launch_bounds__(256) void k_post_mapq(int64_t n_reads, const unsigned long long *__restrict__ out_off, const int32_t *__restrict__ rep_len,
                                                   int min_chain_sc, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch,
                                                   int32_t *__restrict__ out, int32_t *__restrict__ err)
{
	const int lane = threadIdx.x & 63;
	const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (r >= n_reads) return;
	const int64_t o0 = (int64_t)out_off[r];
	const int n = (int)((int64_t)out_off[r + 1] - o0);
	int32_t *regs = out + o0 * 20;
	long long sum_sc = 0;
	for (int i = lane; i < n; i += 64) if (regs[i * 20 + 8] == regs[i * 20]) sum_sc += regs[i * 20 + 3];
	for (int d = 32; d > 0; d >>= 1) sum_sc += __shfl_xor(sum_sc, d);
	const float uniq_ratio = (float)sum_sc / (float)(sum_sc + rep_len[r]);
	for (int i = lane; i < n; i += 64) {
		int32_t *g = regs + i * 20;
		const uint32_t bits = (uint32_t)g[15];
		int mapq_out;
		if (bits & BIT_INV) {
			mapq_out = 0;
		} else if (g[8] == g[0]) {
			const int score = g[3], cnt = g[1], n_sub = g[13];
			if (score > POST_LOGF_MAX || n_sub + 1 > POST_LOGF_MAX) *err = 1;
			const float pen_s1 = (score > 100 ? 1.0f : 0.01f * (float)score) * uniq_ratio;
			float pen_cm = cnt > 10 ? 1.0f : 0.1f * (float)cnt;
			pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
			const int subsc = g[9] > min_chain_sc ? g[9] : min_chain_sc;
			const float x = (float)subsc / (float)g[14];
			const float q = pen_cm * 40.0f * (1.0f - x) * post_logf_int(score, pk, pv, n_patch);
			int mapq = post_f2i(q);
			const int sub = post_nsub_term(n_sub + 1, pk, pv, n_patch);
			mapq = (int)((uint32_t)mapq - (uint32_t)sub);               // wraps as the reference's int subtraction does on x86
			mapq = mapq > 0 ? mapq : 0;
			mapq_out = mapq < 60 ? mapq : 60;
		} else {
			mapq_out = 0;
		}
		g[15] = (int32_t)((bits & ~0xffu) | ((uint32_t)mapq_out & 0xffu));
	}
}

// the device half of the logf self-test: out[k - 1] = post_logf_int(k), term[k - 1] = post_nsub_term(k) for k in [1, kmax]
__global__ __launch_bounds__(256) void k_post_logf_probe(int kmax, const uint32_t *__restrict__ pk, const float *__restrict__ pv, int n_patch,
                                                         float *__restrict__ out, int32_t *__restrict__ term)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= kmax) return;
	out[g] = post_logf_int((int)g + 1, pk, pv, n_patch);
	term[g] = post_nsub_term((int)g + 1, pk, pv, n_patch);
}

hipError_t launch_post_read(hipStream_t st, int64_t n_reads, const int64_t *d_chains_off, const int64_t *d_b_off, const void *d_b, const void *d_regs,
                            const int32_t *d_qlen, const PostOpt &o, int32_t *d_scratch, void *d_stage, void *d_sq, unsigned long long *d_n_out)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_read, dim3((unsigned)n_reads), dim3(64), 0, st, n_reads, d_chains_off, d_b_off, (const ulonglong2*)d_b,
	                   (const int32_t*)d_regs, d_qlen, o, d_scratch, (int32_t*)d_stage, (ulonglong2*)d_sq, d_n_out);
	return hipGetLastError();
}

hipError_t launch_post_scatter(hipStream_t st, int64_t n_reads, const int64_t *d_chains_off, const unsigned long long *d_out_off, const void *d_stage,
                               void *d_out)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_scatter, dim3((unsigned)((n_reads * 64 + 255) / 256)), dim3(256), 0, st, n_reads, d_chains_off, d_out_off,
	                   (const int32_t*)d_stage, (int32_t*)d_out);
	return hipGetLastError();
}

hipError_t launch_post_mapq(hipStream_t st, int64_t n_reads, const unsigned long long *d_out_off, const int32_t *d_rep_len, int min_chain_sc,
                            const uint32_t *d_pk, const float *d_pv, int n_patch, void *d_out, int32_t *d_err)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_mapq, dim3((unsigned)((n_reads * 64 + 255) / 256)), dim3(256), 0, st, n_reads, d_out_off, d_rep_len, min_chain_sc,
	                   d_pk, d_pv, n_patch, (int32_t*)d_out, d_err);
	return hipGetLastError();
}

hipError_t launch_post_logf_probe(hipStream_t st, int kmax, const uint32_t *d_pk, const float *d_pv, int n_patch, float *d_out, int32_t *d_term)
{
	if (kmax <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_post_logf_probe, dim3((unsigned)((kmax + 255) / 256)), dim3(256), 0, st, kmax, d_pk, d_pv, n_patch, d_out, d_term);
	return hipGetLastError();
}

} // namespace chaindp
