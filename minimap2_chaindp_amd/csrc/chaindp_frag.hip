// chaindp_frag.hip -- what the reference does with a fragment's hits after mm_gen_regs when nothing is aligned and the read has
// several segments (read_result_handle, map.c:870-890 without MM_F_CIGAR): chain_post with mm_select_sub_multi (pe.c:6-43) in the
// place of mm_select_sub, mm_seg_gen (hit.c:347-401) and, per segment, mm_set_parent and mm_set_mapq.  A batch may mix reads of one
// segment (orphans) with reads of up to 255; the one-segment reads take the steps of k_post_read and give the same bytes.
//
//   k_frag_read     one wave (and one workgroup) per read: chain_post as k_post_read runs it (the device functions of
//                   chaindp_post_dev.h over the same per-field arrays), with frag_select_sub_multi for reads of several segments.
//                   Then the first half of mm_seg_gen: per segment the chains it keeps (hits with an anchor in it) and its anchors,
//                   counted by ballot over a lane per anchor.  Arrays in LDS for reads of up to FRAG_LDS_CAP hits -- 5 KB per
//                   workgroup, so that LDS allows the tiny fragments of paired short reads eight waves per SIMD (the kernel's 77
//                   VGPRs make it six) -- and in global scratch above.
//   (existing)      the scan and k_post_scatter pack the fragments' hits, k_regs_div gives the one-segment reads their div
//   (scans)         per sequence: chains for mm_gen_regs, final hits, anchors -> three CSR offset arrays
//   k_frag_split    wave per read, the second half of mm_seg_gen: u[] of every segment with the zeros squeezed out, the anchors
//                   split stably by segment (hit order, then position in the hit: a rank by ballot) with the strand-dependent y
//                   offset of hit.c:388 taken off.  A one-segment read's hits and anchors are copied to where its sequence's go.
//   (existing)      k_regs_keys / k_regs_fill: mm_gen_regs with every (fragment, segment) as a read (hit.c:393)
//   k_frag_seg      wave per segment: seg_split and seg_id (hit.c:396-397), mm_set_parent (map.c:883), the records to their place
//   (existing)      k_post_mapq per sequence, with the fragment's rep_len (map.c:885)
//   k_frag_revcomp  worker_for's reverse complement of a pair's segments (map.c:609-610), in place, before the sketch
//   k_frag_flip     ... and the flip of their hits back to the read's strand (map.c:624-630)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "chaindp_kernels.h"
#include "chaindp_wave.h"
#include "chaindp_post_dev.h"

namespace chaindp {

#define FRAG_SEG_SHIFT 48                  // mmpriv.h:22-23: the segment of an anchor, y bits 48-55
#define FRAG_BIT_SEG_ID_SHIFT 16           // mm_reg1_t::seg_id, bits 16-23 of the bit-field word

// mm_select_sub_multi (pe.c:6-43).  Like mm_select_sub it compacts in place while it reads r[p]: a kept hit may already sit in slot p.
// Every lane the same.
__device__ int frag_select_sub_multi(const PostFields &F, int n, float pri_ratio, int max_gap_ref, int min_diff, int best_n, int n_segs,
                                     int ql0, int ql1, int lane)
{
	if (!(pri_ratio > 0.0f && n > 0)) return n;
	const float pri1 = 0.2f, pri2 = 0.7f;                                // map.c:243
	const int max_dist = n_segs == 2 ? ql0 + ql1 + max_gap_ref : 0;
	int k = 0, n_2nd = 0;
	for (int i = 0; i < n; ++i) {
		const int p = F(PF_PARENT, i);
		bool keep = false;
		if (p == i) {
			keep = true;
		} else if (p >= 0 && p < n) {                                    // (always: every hit has a parent after mm_set_parent)
			const int si = F(PF_SCORE, i), sp = F(PF_SCORE, p);
			if (si + min_diff >= sp) {
				keep = true;
			} else if (!((F(PF_BITS, p) ^ F(PF_BITS, i)) & BIT_REV) && F(PF_RID, p) == F(PF_RID, i) && F(PF_RE, i) - F(PF_RS, p) < max_dist &&
			           F(PF_RE, p) - F(PF_RS, i) < max_dist) {           // child and parent are close on the reference
				keep = (float)si >= sp * pri1;
			} else {
				const bool par_both = n_segs == 2 && F(PF_QS, p) < ql0 && F(PF_QE, p) > ql0;
				const bool chi_both = n_segs == 2 && F(PF_QS, i) < ql0 && F(PF_QE, i) > ql0;
				if (chi_both || chi_both == par_both) keep = (float)si >= sp * pri_ratio;
				else keep = (float)si >= sp * pri2;
			}
		}
		if (keep && p != i && n_2nd++ >= best_n) keep = false;           // pe.c:34-36: counted whether or not it is kept
		if (keep) { post_copy(F, k, i); ++k; }
	}
	__syncthreads();
	if (k != n) post_sync_regs(F, k, lane);
	return k;
}

template <bool IN_LDS>
__device__ void frag_read(int64_t r, const int64_t *__restrict__ chains_off, const int64_t *__restrict__ b_off, const ulonglong2 *__restrict__ b,
                          const int32_t *__restrict__ regs, const int32_t *__restrict__ qlen, const int32_t *__restrict__ read_seq0,
                          const int32_t *__restrict__ seq_len, PostOpt o, int max_gap_ref, int32_t *__restrict__ scratch,
                          int32_t *__restrict__ stage, ulonglong2 *__restrict__ sq, unsigned long long *__restrict__ n_out,
                          unsigned long long *__restrict__ cnt_g, unsigned long long *__restrict__ cnt_o, unsigned long long *__restrict__ cnt_a, int *lds)
{
	const int lane = threadIdx.x & 63;
	const int64_t c0 = chains_off[r];
	const int n0 = (int)(chains_off[r + 1] - c0);
	const int64_t a0 = b_off[r];
	const int n_b = (int)(b_off[r + 1] - a0);
	const int q0 = read_seq0[r], n_segs = read_seq0[r + 1] - q0;
	PostFields F;
	if (IN_LDS) { F.base = lds; F.stride = FRAG_LDS_CAP; }
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
		if (n_segs <= 1) n = post_select_sub(F, n, o.pri_ratio, o.min_diff, o.best_n, lane);
		else n = frag_select_sub_multi(F, n, o.pri_ratio, max_gap_ref, o.min_diff, o.best_n, n_segs, seq_len[q0], seq_len[q0 + 1], lane);
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
	if (n_segs <= 1) {                                                   // its sequence takes the read's hits and anchors as they are
		if (lane == 0) { cnt_g[q0] = 0; cnt_o[q0] = (unsigned long long)n; cnt_a[q0] = (unsigned long long)n_b; }
		return;
	}
	__syncthreads();                                                     // sa[] as written above, read by other lanes below
	for (int s = 0; s < n_segs; ++s) {                                   // hit.c:363-375: chains and anchors of segment s
		int nu = 0, na = 0;
		for (int i = 0; i < n; ++i) {
			const int as = F(PF_AS, i), cnt = F(PF_CNT, i);
			int c = 0;
			for (int base = 0; base < cnt; base += 64) {
				const int t = base + lane;
				const bool mine = t < cnt && (int)(sa[as + t].y >> FRAG_SEG_SHIFT & 0xff) == s;
				c += __popcll(__ballot(mine));
			}
			nu += c != 0; na += c;
		}
		if (lane == 0) { cnt_g[q0 + s] = (unsigned long long)nu; cnt_o[q0 + s] = (unsigned long long)nu; cnt_a[q0 + s] = (unsigned long long)na; }
	}
}

__global__ __launch_bounds__(64) void k_frag_read(int64_t n_reads, const int64_t *__restrict__ chains_off, const int64_t *__restrict__ b_off,
                                                  const ulonglong2 *__restrict__ b, const int32_t *__restrict__ regs, const int32_t *__restrict__ qlen,
                                                  const int32_t *__restrict__ read_seq0, const int32_t *__restrict__ seq_len, PostOpt o, int max_gap_ref,
                                                  int lds_cap, int32_t *__restrict__ scratch, int32_t *__restrict__ stage, ulonglong2 *__restrict__ sq,
                                                  unsigned long long *__restrict__ n_out, unsigned long long *__restrict__ cnt_g,
                                                  unsigned long long *__restrict__ cnt_o, unsigned long long *__restrict__ cnt_a,
                                                  const int2 *__restrict__ read_gaps)
{
	__shared__ int lds[PF_NF * FRAG_LDS_CAP];
	const int64_t r = blockIdx.x;
	if (r >= n_reads) return;
	if (read_gaps) max_gap_ref = read_gaps[r].x;                         // the run's own gap_ref of read r (chaindp_set_read_gaps)
	const int64_t n = chains_off[r + 1] - chains_off[r];
	if (n <= lds_cap) frag_read<true>(r, chains_off, b_off, b, regs, qlen, read_seq0, seq_len, o, max_gap_ref, scratch, stage, sq, n_out, cnt_g, cnt_o, cnt_a, lds);
	else frag_read<false>(r, chains_off, b_off, b, regs, qlen, read_seq0, seq_len, o, max_gap_ref, scratch, stage, sq, n_out, cnt_g, cnt_o, cnt_a, lds);
}

// the second half of mm_seg_gen (hit.c:371-391) over the packed hits of k_post_scatter; a one-segment read is copied through
__global__ __launch_bounds__(256) void k_frag_split(int64_t n_reads, const unsigned long long *__restrict__ post_off, const int32_t *__restrict__ post_out,
                                                    const int64_t *__restrict__ b_off, const ulonglong2 *__restrict__ sq,
                                                    const int32_t *__restrict__ read_seq0, const int32_t *__restrict__ seq_len,
                                                    const uint32_t *__restrict__ hash, const int32_t *__restrict__ rep_len,
                                                    const unsigned long long *__restrict__ g_off, const unsigned long long *__restrict__ o_off,
                                                    const unsigned long long *__restrict__ a_off, unsigned long long *__restrict__ seg_u,
                                                    ulonglong2 *__restrict__ seg_a, int32_t *__restrict__ out, uint32_t *__restrict__ seq_hash,
                                                    int32_t *__restrict__ seq_rep, int32_t *__restrict__ seq_read)
{
	const int lane = threadIdx.x & 63;
	const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (r >= n_reads) return;
	const int q0 = read_seq0[r], n_segs = read_seq0[r + 1] - q0;
	const int64_t p0 = (int64_t)post_off[r];
	const int n = (int)((int64_t)post_off[r + 1] - p0);
	const ulonglong2 *sa = sq + b_off[r];
	for (int s = lane; s < n_segs; s += 64) {
		seq_hash[q0 + s] = hash[r]; seq_read[q0 + s] = (int32_t)r;
		if (rep_len) seq_rep[q0 + s] = rep_len[r];
	}
	if (n_segs <= 1) {
		const int32_t *src = post_out + p0 * 20;
		int32_t *dst = out + (int64_t)o_off[q0] * 20;
		for (int t = lane; t < n * 20; t += 64) dst[t] = src[t];
		const int n_b = (int)(b_off[r + 1] - b_off[r]);
		ulonglong2 *da = seg_a + (int64_t)a_off[q0];
		for (int t = lane; t < n_b; t += 64) da[t] = sa[t];
		return;
	}
	int qlen_sum = 0;
	for (int s = 0; s < n_segs; ++s) qlen_sum += seq_len[q0 + s];
	int acc = 0;                                                         // acc_qlen[s], hit.c:353-354
	for (int s = 0; s < n_segs; ++s) {
		const int ql = seq_len[q0 + s];
		const unsigned long long off_fwd = (unsigned long long)(long long)acc, off_rev = (unsigned long long)(long long)(qlen_sum - (ql + acc));
		unsigned long long *du = seg_u + (int64_t)g_off[q0 + s];
		ulonglong2 *da = seg_a + (int64_t)a_off[q0 + s];
		int nu = 0, run = 0;
		for (int i = 0; i < n; ++i) {
			const int32_t *rec = post_out + (p0 + i) * 20;
			const int cnt = rec[1], as = rec[10], score = rec[3];
			int c = 0;
			for (int base = 0; base < cnt; base += 64) {
				const int t = base + lane;
				ulonglong2 a1 = make_ulonglong2(0, 0);
				bool mine = false;
				if (t < cnt) { a1 = sa[as + t]; mine = (int)(a1.y >> FRAG_SEG_SHIFT & 0xff) == s; }
				const uint64_t m = __ballot(mine);
				if (mine) {
					a1.y -= a1.x >> 63 ? off_rev : off_fwd;              // hit.c:388
					da[run + c + lanes_below(m)] = a1;
				}
				c += __popcll(m);
			}
			if (c) {                                                     // hit.c:361,367,373-375
				if (lane == 0) du[nu] = ((unsigned long long)(long long)score << 32) + (unsigned long long)c;
				++nu;
			}
			run += c;
		}
		acc += ql;
	}
}

// hit.c:396-397 and the per-segment mm_set_parent of map.c:883 on what mm_gen_regs made of one segment's chains
template <bool IN_LDS>
__device__ void frag_seg(int n, int seg, const int32_t *__restrict__ src, int32_t *__restrict__ dst, float mask_level, int32_t *__restrict__ scratch, int *lds)
{
	const int lane = threadIdx.x & 63;
	PostFields F;
	if (IN_LDS) { F.base = lds; F.stride = FRAG_LDS_CAP; }
	else { F.base = scratch; F.stride = n; }
	for (int s = lane; s < n; s += 64) {
		const int32_t *g = src + s * 20;
		F(PF_ID, s) = g[0]; F(PF_CNT, s) = g[1]; F(PF_SCORE, s) = g[3]; F(PF_QS, s) = g[4]; F(PF_QE, s) = g[5];
		F(PF_PARENT, s) = g[8]; F(PF_SUBSC, s) = g[9]; F(PF_NSUB, s) = g[13];
	}
	__syncthreads();
	post_set_parent(F, n, mask_level, lane);
	for (int s = lane; s < n; s += 64) {
		const int32_t *g = src + s * 20;
		int32_t *d = dst + s * 20;
		d[0] = F(PF_ID, s); d[1] = g[1]; d[2] = g[2]; d[3] = g[3]; d[4] = g[4]; d[5] = g[5]; d[6] = g[6]; d[7] = g[7];
		d[8] = F(PF_PARENT, s); d[9] = F(PF_SUBSC, s); d[10] = g[10]; d[11] = g[11]; d[12] = g[12]; d[13] = F(PF_NSUB, s); d[14] = g[14];
		d[15] = (int32_t)((uint32_t)g[15] | BIT_SEG_SPLIT | (uint32_t)seg << FRAG_BIT_SEG_ID_SHIFT);
		d[16] = g[16]; d[17] = g[17]; d[18] = g[18]; d[19] = g[19];
	}
}

__global__ __launch_bounds__(64) void k_frag_seg(int64_t n_seqs, const int32_t *__restrict__ read_seq0, const int32_t *__restrict__ seq_read,
                                                 const unsigned long long *__restrict__ g_off, const unsigned long long *__restrict__ o_off,
                                                 const int32_t *__restrict__ seg_stage, float mask_level, int lds_cap, int32_t *__restrict__ scratch,
                                                 int32_t *__restrict__ out)
{
	__shared__ int lds[PF_NF * FRAG_LDS_CAP];
	const int64_t q = blockIdx.x;
	if (q >= n_seqs) return;
	const int r = seq_read[q], q0 = read_seq0[r];
	if (read_seq0[r + 1] - q0 <= 1) return;                              // a one-segment read: k_frag_split has put its hits in place
	const int64_t g0 = (int64_t)g_off[q];
	const int n = (int)((int64_t)g_off[q + 1] - g0);
	if (n <= 0) return;
	const int32_t *src = seg_stage + g0 * 20;
	int32_t *dst = out + (int64_t)o_off[q] * 20;
	if (n <= lds_cap) frag_seg<true>(n, (int)(q - q0), src, dst, mask_level, scratch + g0 * PF_NF, lds);
	else frag_seg<false>(n, (int)(q - q0), src, dst, mask_level, scratch + g0 * PF_NF, lds);
}

// mm_revcomp_bseq of the segments worker_for turns round before mapping a pair (map.c:609-610): segment 0 if pe_ori >> 1 & 1, segment 1
// if pe_ori & 1, of reads with exactly two segments.  In place, a thread per pair of bases.  A <-> T, C <-> G in either case, U -> A;
// every other byte stays what it is (ambiguous for the sketch, like its complement in the reference's table; the bytes 0..3 are their
// own complement there).
__device__ __forceinline__ uint8_t frag_comp(uint8_t c)
{
	switch (c) {
	case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'U': return 'A';
	case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a'; case 'u': return 'a';
	default: return c;
	}
}

__global__ __launch_bounds__(256) void k_frag_revcomp(int64_t n_reads, const int32_t *__restrict__ read_seq0, const int64_t *__restrict__ seq_off,
                                                      uint8_t *__restrict__ seq, int pe_ori)
{
	const int64_t r = blockIdx.x;
	if (r >= n_reads) return;
	const int q0 = read_seq0[r];
	if (read_seq0[r + 1] - q0 != 2) return;
	for (int j = 0; j < 2; ++j) {
		if (!(j == 0 ? pe_ori >> 1 & 1 : pe_ori & 1)) continue;
		uint8_t *s = seq + seq_off[q0 + j];
		const int64_t len = seq_off[q0 + j + 1] - seq_off[q0 + j];
		for (int64_t i = threadIdx.x; i < (len + 1) / 2; i += blockDim.x) {
			const uint8_t lo = s[i], hi = s[len - 1 - i];                // i == len - 1 - i in the middle of an odd length
			s[i] = frag_comp(hi); s[len - 1 - i] = frag_comp(lo);
		}
	}
}

// map.c:624-630 on the final hits of those segments
__global__ __launch_bounds__(256) void k_frag_flip(int64_t n_seqs, const int32_t *__restrict__ read_seq0, const int32_t *__restrict__ seq_read,
                                                   const int32_t *__restrict__ seq_len, const unsigned long long *__restrict__ o_off, int pe_ori,
                                                   int32_t *__restrict__ out)
{
	const int lane = threadIdx.x & 63;
	const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	if (q >= n_seqs) return;
	const int r = seq_read[q], q0 = read_seq0[r];
	if (read_seq0[r + 1] - q0 != 2) return;
	if (!(q == q0 ? pe_ori >> 1 & 1 : pe_ori & 1)) return;
	const int ql = seq_len[q];
	const int64_t o0 = (int64_t)o_off[q];
	const int n = (int)((int64_t)o_off[q + 1] - o0);
	for (int i = lane; i < n; i += 64) {
		int32_t *g = out + (o0 + i) * 20;
		const int t = g[4];
		g[4] = ql - g[5]; g[5] = ql - t;
		g[15] = (int32_t)((uint32_t)g[15] ^ BIT_REV);
	}
}

hipError_t launch_frag_read(hipStream_t st, int64_t n_reads, const int64_t *d_chains_off, const int64_t *d_b_off, const void *d_b, const void *d_regs,
                            const int32_t *d_qlen, const int32_t *d_read_seq0, const int32_t *d_seq_len, const PostOpt &o, int max_gap_ref, int lds_cap,
                            int32_t *d_scratch, void *d_stage, void *d_sq, unsigned long long *d_n_out, unsigned long long *d_cnt_g,
                            unsigned long long *d_cnt_o, unsigned long long *d_cnt_a, const int2 *d_read_gaps)
{
	if (n_reads <= 0) return hipSuccess;
	if (lds_cap > FRAG_LDS_CAP || lds_cap < 0) lds_cap = FRAG_LDS_CAP;
	hipLaunchKernelGGL(k_frag_read, dim3((unsigned)n_reads), dim3(64), 0, st, n_reads, d_chains_off, d_b_off, (const ulonglong2*)d_b,
	                   (const int32_t*)d_regs, d_qlen, d_read_seq0, d_seq_len, o, max_gap_ref, lds_cap, d_scratch, (int32_t*)d_stage, (ulonglong2*)d_sq,
	                   d_n_out, d_cnt_g, d_cnt_o, d_cnt_a, d_read_gaps);
	return hipGetLastError();
}

hipError_t launch_frag_split(hipStream_t st, int64_t n_reads, const unsigned long long *d_post_off, const void *d_post_out, const int64_t *d_b_off,
                             const void *d_sq, const int32_t *d_read_seq0, const int32_t *d_seq_len, const uint32_t *d_hash, const int32_t *d_rep_len,
                             const unsigned long long *d_g_off, const unsigned long long *d_o_off, const unsigned long long *d_a_off,
                             unsigned long long *d_seg_u, void *d_seg_a, void *d_out, uint32_t *d_seq_hash, int32_t *d_seq_rep, int32_t *d_seq_read)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_frag_split, dim3((unsigned)((n_reads * 64 + 255) / 256)), dim3(256), 0, st, n_reads, d_post_off, (const int32_t*)d_post_out,
	                   d_b_off, (const ulonglong2*)d_sq, d_read_seq0, d_seq_len, d_hash, d_rep_len, d_g_off, d_o_off, d_a_off, d_seg_u,
	                   (ulonglong2*)d_seg_a, (int32_t*)d_out, d_seq_hash, d_seq_rep, d_seq_read);
	return hipGetLastError();
}

hipError_t launch_frag_seg(hipStream_t st, int64_t n_seqs, const int32_t *d_read_seq0, const int32_t *d_seq_read, const unsigned long long *d_g_off,
                           const unsigned long long *d_o_off, const void *d_seg_stage, float mask_level, int lds_cap, int32_t *d_scratch, void *d_out)
{
	if (n_seqs <= 0) return hipSuccess;
	if (lds_cap > FRAG_LDS_CAP || lds_cap < 0) lds_cap = FRAG_LDS_CAP;
	hipLaunchKernelGGL(k_frag_seg, dim3((unsigned)n_seqs), dim3(64), 0, st, n_seqs, d_read_seq0, d_seq_read, d_g_off, d_o_off,
	                   (const int32_t*)d_seg_stage, mask_level, lds_cap, d_scratch, (int32_t*)d_out);
	return hipGetLastError();
}

hipError_t launch_frag_revcomp(hipStream_t st, int64_t n_reads, const int32_t *d_read_seq0, const int64_t *d_seq_off, uint8_t *d_seq, int pe_ori)
{
	if (n_reads <= 0 || pe_ori < 0 || !(pe_ori & 3)) return hipSuccess;
	hipLaunchKernelGGL(k_frag_revcomp, dim3((unsigned)n_reads), dim3(256), 0, st, n_reads, d_read_seq0, d_seq_off, d_seq, pe_ori);
	return hipGetLastError();
}

hipError_t launch_frag_flip(hipStream_t st, int64_t n_seqs, const int32_t *d_read_seq0, const int32_t *d_seq_read, const int32_t *d_seq_len,
                            const unsigned long long *d_o_off, int pe_ori, void *d_out)
{
	if (n_seqs <= 0 || pe_ori < 0 || !(pe_ori & 3)) return hipSuccess;
	hipLaunchKernelGGL(k_frag_flip, dim3((unsigned)((n_seqs * 64 + 255) / 256)), dim3(256), 0, st, n_seqs, d_read_seq0, d_seq_read, d_seq_len, d_o_off,
	                   pe_ori, (int32_t*)d_out);
	return hipGetLastError();
}

} // namespace chaindp
