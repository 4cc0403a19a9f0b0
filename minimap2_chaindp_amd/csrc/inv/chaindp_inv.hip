// inv/chaindp_inv.hip -- mm_align1_inv (reference align.c:638-693) between two regions that mm_align1 split at a potential inversion.
//
// The host has done the early returns (chaindp_inv_plan.h: it needs every pair's fields for its refusals anyway) and hands over the
// candidates; one wave per candidate or per survivor:
//   k_inv_ll       ksw_ll_i16 (ksw2_ll_sse.c:80-147) WITH its end positions: score, qe, te of the two reversed stretches, the query
//                  padded to a multiple of 8 rows as the reference's striped layout pads it
//   k_inv_gather   the bases of the extension from (q_off, t_off) on -- q_off may lie up to seven bases before the stretch
//   (k_ksw_extd, chaindp_ksw.hip, unchanged)
//   k_inv_finish   n_cigar == 0, the fields of r_inv, mm_fix_cigar and mm_update_extra
//   k_inv_skip     the rule of the loop around it (align.c:747-753), a thread per read over its slots in order
//   k_inv_pack     the CIGARs to their CSR places
// Every base is fetched through a bounds check: where the reference would index outside a strand the answer is unspecified, but nothing
// is read or written outside a buffer.
#include "../chaindp_kernels.h"
#include "../chaindp_wave.h"
#include "../chaindp_post_dev.h"
#include "../chaindp_align_dev.h"
#include "../chaindp_inv_plan.h"

namespace chaindp {

// ksw_ll_i16 as the compiled reference behaves: a local DP over ql8 = 8 * slen rows (slen = (ql + 7) / 8; a row past ql scores 0 against
// every base but is a cell like any other), H floored at 0, the diagonal add saturating at 32767, E and F floored at 0.  te is the last
// column whose maximum equals the global one; qe is, of that column's rows p with H == the maximum, the one with the greatest
// (p % slen, p / slen): the reference's scan over its striped H (:144-145) keeps the last hit.
//
// The wave sweeps the target in stripes of 64 columns.  Lane l owns column c0 + l for all rows and is l steps behind lane 0, so that a
// step is an anti-diagonal of the stripe: H and E of the column to the left arrive by a one-lane shift, the query row with its rank
// (p % slen) * 8 + p / slen travels the same way, F and the column's record H << 16 | rank stay in registers.  The only memory is the
// stripe's right edge, H | E << 16 per row in LDS: read 64 rows at a time into a register that lane 0 is fed from, written 64 rows at a
// time from a register that collects lane 63's results, behind the reads.
extern __shared__ __attribute__((aligned(16))) uint32_t inv_lds[];
__global__ __launch_bounds__(64) void k_inv_ll(AlignOpt o, int n, const InvCand *__restrict__ cand, const int64_t *__restrict__ seq_off,
                                               const char *__restrict__ seq_all, const int64_t *__restrict__ t_off, const uint8_t *__restrict__ tcodes,
                                               int lds_rows, int32_t *__restrict__ out3, int32_t *made)
{
	const int lane = threadIdx.x;
	for (int c = blockIdx.x; c < n; c += gridDim.x) {
		const InvCand C = cand[c];
		const int ql = C.ql, tl = C.tl, slen = (ql + 7) / 8, ql8 = slen * 8;
		if (ql <= 0 || tl <= 0 || ql8 > lds_rows) {
			if (lane == 0) { out3[3 * c] = 0; out3[3 * c + 1] = -1; out3[3 * c + 2] = -1; made[C.slot] = INV_LOW_SCORE; }
			continue;
		}
		const char *seq = seq_all + seq_off[C.read];
		const uint8_t *t = tcodes + t_off[C.rid];
		const int oe = o.q + o.e, ge = o.e, n_steps = ql8 + 63;
		for (int k = lane; k < ql8; k += 64) inv_lds[k] = 0;
		wave_mem_fence();
		int best_h = -1, best_col = -1, best_rank = 0;
		for (int c0 = 0; c0 < tl; c0 += 64) {
			const int col = c0 + lane;
			const bool col_on = col < tl, last = c0 + 64 >= tl;
			const int tc = col_on ? al_tbase(t, C.tlen, C.ts + tl - 1 - col) : 4;        // the target stretch reversed
			int h_out = 0, e_out = 0, f = 0, diag = 0, pipe = 0, rec = -1;
			for (int t0 = 0; t0 < n_steps; t0 += 64) {
				const int row = t0 + lane;
				uint32_t edge_in = 0, edge_out = 0;
				int feed = 0;                    // code | 8 (a row of the padded query) | rank << 4
				if (row < ql8) {
					edge_in = inv_lds[row];
					const int code = row < ql ? al_qbase(seq, C.qlen, !C.rev1, C.qb + ql - 1 - row) : 4;       // the query stretch reversed
					feed = code | 8 | ((row % slen) * 8 + row / slen) << 4;
				}
				const int kmax = n_steps - t0 < 64 ? n_steps - t0 : 64;
				for (int k = 0; k < kmax; ++k) {
					const uint32_t ein = (uint32_t)__builtin_amdgcn_readlane((int)edge_in, k);
					const int left_h = wave_shift_up1(h_out, (int)(ein & 0xffff)), left_e = wave_shift_up1(e_out, (int)(ein >> 16));
					pipe = wave_shift_up1(pipe, __builtin_amdgcn_readlane(feed, k));
					const bool on = (pipe & 8) && col_on;
					const int cq = pipe & 7;
					f = max(max(f - ge, h_out - oe), 0);                      // h_out: H of the row above in this column
					int h = min(diag + al_mat(o, tc, cq), 32767);
					h = max(max(h, left_e), f);
					const int e = max(max(left_e - ge, h - oe), 0);           // E of this row in the next column
					diag = left_h;
					h_out = on ? h : 0; e_out = on ? e : 0; f = on ? f : 0;
					if (on) rec = max(rec, h << 16 | pipe >> 4);
					if (!last) {
						const int v = __builtin_amdgcn_readlane(h_out | e_out << 16, 63);      // lane 63 is at row t0 + k - 63
						if (lane == k) edge_out = (uint32_t)v;
					}
				}
				const int row_w = t0 + lane - 63;
				if (!last && row_w >= 0 && row_w < ql8 && lane < kmax) inv_lds[row_w] = edge_out;
				wave_mem_fence();
			}
			if (col_on && rec >> 16 >= best_h) { best_h = rec >> 16; best_col = col; best_rank = rec & 0xffff; }
		}
		const int gmax = wave_max_i(best_h), te = wave_max_i(best_h == gmax ? best_col : -1), rank = wave_max_i(best_col == te ? best_rank : -1);
		if (lane == 0) {
			out3[3 * c] = gmax; out3[3 * c + 1] = (rank & 7) * slen + (rank >> 3); out3[3 * c + 2] = te;
			if (gmax < o.min_dp_max) made[C.slot] = INV_LOW_SCORE;
		}
	}
}

// the bases of every extension: the query from the strand opposite to r1, the target from the resident codes
__global__ __launch_bounds__(64) void k_inv_gather(int n, const KswProb *__restrict__ prob, const InvSurv *__restrict__ surv,
                                                   const InvCand *__restrict__ cand, const int64_t *__restrict__ seq_off, const char *__restrict__ seq_all,
                                                   const int64_t *__restrict__ t_off, const uint8_t *__restrict__ tcodes, uint8_t *bases)
{
	const int lane = threadIdx.x;
	for (int s = blockIdx.x; s < n; s += gridDim.x) {
		const KswProb p = prob[s];
		const InvSurv S = surv[s];
		const InvCand C = cand[S.cand];
		const char *seq = seq_all + seq_off[C.read];
		const uint8_t *t = tcodes + t_off[C.rid];
		for (int k = lane; k < p.qlen; k += 64) bases[p.q_beg + k] = (uint8_t)al_qbase(seq, C.qlen, !C.rev1, C.qb + S.q_off + k);
		for (int k = lane; k < p.tlen; k += 64) bases[p.t_beg + k] = (uint8_t)al_tbase(t, C.tlen, C.ts + S.t_off + k);
	}
}

// align.c:670-689 on the extension's answer: r_inv, then mm_fix_cigar and mm_update_extra (k_align_extra's, chaindp_align_dev.h) on its
// CIGAR in place
__global__ __launch_bounds__(64) void k_inv_finish(AlignOpt o, int n, const KswProb *__restrict__ prob, const InvSurv *__restrict__ surv,
                                                   const InvCand *__restrict__ cand, const int64_t *__restrict__ seq_off, const char *__restrict__ seq_all,
                                                   const int64_t *__restrict__ t_off, const uint8_t *__restrict__ tcodes, const int32_t *__restrict__ ez_all,
                                                   uint32_t *cig, int32_t *r_inv, int32_t *extra, int32_t *made)
{
	const int lane = threadIdx.x;
	for (int s = blockIdx.x; s < n; s += gridDim.x) {
		const InvSurv S = surv[s];
		const InvCand C = cand[S.cand];
		const int32_t *ez = ez_all + (int64_t)s * KSW_EZ_WORDS;
		const int n_cg = ez[10];
		if (n_cg <= 0) { if (lane == 0) made[C.slot] = INV_NO_CIGAR; continue; }
		int32_t *r = r_inv + (int64_t)C.slot * AL_REG_WORDS, *ex = extra + (int64_t)C.slot * 5;
		const char *seq = seq_all + seq_off[C.read];
		const uint8_t *t = tcodes + t_off[C.rid];
		const int rrev = !C.rev1, qs0 = C.qb + S.q_off, rs0 = C.ts + S.t_off;
		if (lane == 0) {
			r[0] = -1; r[2] = C.rid; r[8] = -1;                                        // id, rid, parent = MM_PARENT_UNSET
			r[15] = (int32_t)(INV_BIT_INV | (rrev ? INV_BIT_REV : 0u));
			r[17] = (int32_t)0xbf800000u;                                              // div = -1.0f
			if (!rrev) { r[4] = C.r2qe + S.q_off; r[5] = r[4] + ez[2] + 1; }
			else { r[5] = C.r2qs - S.q_off; r[4] = r[5] - (ez[2] + 1); }
			r[6] = rs0; r[7] = rs0 + ez[3] + 1;
		}
		al_fix_and_extra(o, lane, seq, C.qlen, rrev, qs0, t, C.tlen, rs0, cig + prob[s].cig_beg, n_cg, ez[0], r, ex);
		if (lane == 0) made[C.slot] = INV_MADE;
	}
}

// The loop's rule (align.c:747-753): an inversion is inserted behind its right region and stepped over, so the next region's left
// neighbour is the inversion record, whose split bits are 0.  In the order of a read's slots: a candidate behind a made pair is never
// tested (code 3, nothing kept of what was computed for it).
__global__ __launch_bounds__(64) void k_inv_skip(int64_t n_reads, const int64_t *__restrict__ regs_off, const int32_t *__restrict__ slot_cand,
                                                 int32_t *made, int32_t *r_inv, int32_t *extra)
{
	for (int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * 64) {
		bool prev = false;
		for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g) {
			if (prev && slot_cand[g] >= 0) {
				made[g] = INV_SKIPPED;
				for (int k = 0; k < AL_REG_WORDS; ++k) r_inv[g * AL_REG_WORDS + k] = 0;
				for (int k = 0; k < 5; ++k) extra[g * 5 + k] = 0;
			}
			prev = made[g] == INV_MADE;
		}
	}
}

__global__ __launch_bounds__(64) void k_inv_pack(int n, const KswProb *__restrict__ prob, const InvSurv *__restrict__ surv, const InvCand *__restrict__ cand,
                                                 const int32_t *__restrict__ extra, const int64_t *__restrict__ off, const uint32_t *__restrict__ cig,
                                                 uint32_t *__restrict__ out)
{
	for (int s = blockIdx.x; s < n; s += gridDim.x) {
		const int slot = cand[surv[s].cand].slot, m = extra[(int64_t)slot * 5 + 4];
		const uint32_t *src = cig + prob[s].cig_beg;
		uint32_t *dst = out + off[slot];
		for (int k = threadIdx.x; k < m; k += 64) dst[k] = src[k];
	}
}

static unsigned inv_grid(int64_t n) { return (unsigned)(n < 1 ? 1 : n < 65536 ? n : 65536); }

hipError_t launch_inv_ll(hipStream_t st, const AlignOpt &o, const InvDev &d, int lds_rows, int32_t *d_out3)
{
	if (d.n_cand <= 0) return hipSuccess;
	const size_t lds = (size_t)lds_rows * sizeof(uint32_t);
	const hipError_t e = hipFuncSetAttribute((const void*)k_inv_ll, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds > 65536 ? lds : 65536));
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_inv_ll, dim3(inv_grid(d.n_cand)), dim3(64), lds, st, o, d.n_cand, d.cand, d.seq_off, d.seq, d.t_off, d.tcodes, lds_rows, d_out3, d.made);
	return hipGetLastError();
}

hipError_t launch_inv_gather(hipStream_t st, const InvDev &d, uint8_t *d_bases)
{
	if (d.n_surv <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_inv_gather, dim3(inv_grid(d.n_surv)), dim3(64), 0, st, d.n_surv, d.prob, d.surv, d.cand, d.seq_off, d.seq, d.t_off, d.tcodes, d_bases);
	return hipGetLastError();
}

hipError_t launch_inv_finish(hipStream_t st, const AlignOpt &o, const InvDev &d, const int32_t *d_ez, uint32_t *d_cig)
{
	if (d.n_surv <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_inv_finish, dim3(inv_grid(d.n_surv)), dim3(64), 0, st, o, d.n_surv, d.prob, d.surv, d.cand, d.seq_off, d.seq, d.t_off, d.tcodes, d_ez,
	                   d_cig, d.r_inv, d.extra, d.made);
	return hipGetLastError();
}

hipError_t launch_inv_skip(hipStream_t st, const InvDev &d)
{
	if (d.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_inv_skip, dim3(inv_grid((d.n_reads + 63) / 64)), dim3(64), 0, st, d.n_reads, d.regs_off, d.slot_cand, d.made, d.r_inv, d.extra);
	return hipGetLastError();
}

hipError_t launch_inv_pack(hipStream_t st, const InvDev &d, const int64_t *d_off, const uint32_t *d_cig, uint32_t *d_out)
{
	if (d.n_surv <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_inv_pack, dim3(inv_grid(d.n_surv)), dim3(64), 0, st, d.n_surv, d.prob, d.surv, d.cand, d.extra, d_off, d_cig, d_out);
	return hipGetLastError();
}

} // namespace chaindp
