// handoff/chaindp_handoff.hip -- from chain_post to the alignment stages without leaving the device: mm_squeeze_a (reference
// hit.c:270-288) as mm_align_skeleton runs it first (align.c:721), over the final regions chaindp_chain_post packed (MM_F_CIGAR: it
// stopped after mm_est_err) and each read's chain anchors as chain_post left them.
//
//   k_handoff_count  a thread per read: the squeezed total, the sum of cnt over the read's regions (launch_scan_u64 makes a_off of them)
//   k_handoff_move   a wave per list (a read's regions): every region's place in (as, slot) order, as radix_sort_64 of as << 32 | i
//                    gives it, is the sum of the counts of the regions ranked before it; its anchors go there, its `as` becomes that
// Source and destination are different buffers: the reference's in-place memmove sequence never reads what it has overwritten (sources
// lie at or above their destinations, in ascending order; chaindp_post_dev.h, post_join_long), so copying from the unsqueezed array
// gives the same anchors.  The regions are copied beside them (chain_post's own stay as they are, the call can be repeated).
// A list of up to lds_cap regions keeps as, cnt and the new as in LDS, a longer one reads the regions and writes the new as in global
// memory through the same code.  Ranking is by counting, a lane per region while the wave reads region t from one address; lists of
// more than 64 regions take more than one trip of the lanes.  Anchors move 16 bytes a lane, the whole wave on one region at a time.
#include "../chaindp_kernels.h"
#include "../chaindp_wave.h"
#include "../chaindp_handoff_plan.h"

namespace chaindp {

__global__ __launch_bounds__(256) void k_handoff_count(HandoffDev d)
{
	for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < d.n_reads; r += (int64_t)gridDim.x * 256) {
		unsigned long long tot = 0;
		for (int64_t g = (int64_t)d.regs_off[r]; g < (int64_t)d.regs_off[r + 1]; ++g) tot += (unsigned long long)max(d.regs[g * HO_REG_WORDS + HO_REG_CNT], 0);
		d.a_off[r] = tot;
	}
}

// where a list's as, cnt and new as are: in LDS ...
struct HoLds {
	int32_t *as_, *cnt_, *to_;
	__device__ __forceinline__ int as(int t) const { return as_[t]; }
	__device__ __forceinline__ int cnt(int t) const { return cnt_[t]; }
	__device__ __forceinline__ int to(int t) const { return to_[t]; }
	__device__ __forceinline__ void set_to(int t, int v) const { to_[t] = v; }
};
// ... or in the regions themselves: the input's as and cnt, the output's as
struct HoGlobal {
	const int32_t *in; int32_t *out;
	__device__ __forceinline__ int as(int t) const { return in[(int64_t)t * HO_REG_WORDS + HO_REG_AS]; }
	__device__ __forceinline__ int cnt(int t) const { return max(in[(int64_t)t * HO_REG_WORDS + HO_REG_CNT], 0); }
	__device__ __forceinline__ int to(int t) const { return out[(int64_t)t * HO_REG_WORDS + HO_REG_AS]; }
	__device__ __forceinline__ void set_to(int t, int v) const { out[(int64_t)t * HO_REG_WORDS + HO_REG_AS] = v; }
};

// One list of n regions: n_b anchors of the read at src, room for the squeezed total n_a at dst.
template <typename V>
__device__ __forceinline__ void handoff_one(const V &v, int lane, int n, int n_b, int n_a, const ulonglong2 *__restrict__ src, ulonglong2 *__restrict__ dst, int32_t *err)
{
	for (int s = lane; s < n; s += 64) {
		const int as = v.as(s);
		int to = 0;
		for (int t = 0; t < n; ++t) { const int at = v.as(t); if (at < as || (at == as && t < s)) to += v.cnt(t); }
		v.set_to(s, to);
	}
	// On the global route the new `as` went to global memory and other lanes read it back below: this relies on __syncthreads'
	// workgroup-scope fence for those stores (the workgroup is one wave); a plain wave barrier would not do.
	__syncthreads();
	for (int s = 0; s < n; ++s) {
		const int from = v.as(s), to = v.to(s), cnt = v.cnt(s);
		if (from < 0 || from + cnt > n_b || to + cnt > n_a) {                    // never: chain_post keeps every region inside its read's anchors
			if (lane == 0) *err = 1;                                             // nothing is copied from or to a place outside them; the host refuses the batch
			continue;
		}
		for (int t = lane; t < cnt; t += 64) dst[to + t] = src[from + t];
	}
}

__global__ __launch_bounds__(64, 8) void k_handoff_move(HandoffDev d, int lds_cap)
{
	__shared__ int32_t s_as[HO_LDS_CAP], s_cnt[HO_LDS_CAP], s_to[HO_LDS_CAP];
	const int lane = threadIdx.x;
	for (int64_t list = blockIdx.x; list < d.n_reads; list += gridDim.x) {
		const int64_t base = (int64_t)d.regs_off[list];
		const int n = (int)((int64_t)d.regs_off[list + 1] - base);
		const int64_t a0 = (int64_t)d.a_off[list];
		const int n_a = (int)((int64_t)d.a_off[list + 1] - a0), n_b = (int)(d.b_off[list + 1] - d.b_off[list]);
		const ulonglong2 *src = (const ulonglong2*)d.sq + d.b_off[list];
		ulonglong2 *dst = (ulonglong2*)d.a + a0;
		const int32_t *in = d.regs + base * HO_REG_WORDS;
		int32_t *out = d.out_regs + base * HO_REG_WORDS;
		// the regions beside the anchors, every word but `as`
		for (int w = lane; w < n * HO_REG_WORDS; w += 64)
			if (w % HO_REG_WORDS != HO_REG_AS) out[w] = in[w];
		__syncthreads();                                                          // the list before is done with the LDS
		if (n <= lds_cap) {
			for (int s = lane; s < n; s += 64) { s_as[s] = in[s * HO_REG_WORDS + HO_REG_AS]; s_cnt[s] = max(in[s * HO_REG_WORDS + HO_REG_CNT], 0); }
			__syncthreads();
			handoff_one(HoLds{s_as, s_cnt, s_to}, lane, n, n_b, n_a, src, dst, d.err);
			for (int s = lane; s < n; s += 64) out[s * HO_REG_WORDS + HO_REG_AS] = s_to[s];
		} else {
			handoff_one(HoGlobal{in, out}, lane, n, n_b, n_a, src, dst, d.err);
		}
	}
}

hipError_t launch_handoff(hipStream_t st, const HandoffDev &d, unsigned long long *d_tile, int lds_cap)
{
	if (d.n_reads <= 0) return hipSuccess;
	const int64_t R = d.n_reads;
	hipLaunchKernelGGL(k_handoff_count, dim3((unsigned)std::min<int64_t>((R + 255) / 256, 2048)), dim3(256), 0, st, d);
	if (hipError_t e = hipGetLastError()) return e;
	if (hipError_t e = launch_scan_u64(st, R, d.a_off, d_tile, d.a_off + R)) return e;
	hipLaunchKernelGGL(k_handoff_move, dim3((unsigned)std::min<int64_t>(R, 8192)), dim3(64), 0, st, d, std::max(1, std::min(lds_cap, HO_LDS_CAP)));
	return hipGetLastError();
}

} // namespace chaindp
