// chaindp_align_dev.h -- what the kernels of chaindp_align.hip and inv/chaindp_inv.hip share: the bits of a region's bit-field word and of
// the DP's flag, the bounds-checked base fetches, the scoring of a pair of bases, and mm_fix_cigar with mm_update_extra by one wave.
#ifndef CHAINDP_ALIGN_DEV_H
#define CHAINDP_ALIGN_DEV_H
#include "chaindp_wave.h"
#include "chaindp_post_dev.h"
#include "chaindp_align_plan.h"

namespace chaindp {

#define AL_BIT_SPLIT (1u << 8)
#define AL_BIT_SPLIT_INV (1u << 24)
#define AL_EZ_RIGHT 0x02
#define AL_EZ_APPROX_MAX 0x08
#define AL_EZ_EXTZ_ONLY 0x40
#define AL_EZ_REV_CIGAR 0x80
#define AL_LEN_MAX ((1 << 26) - 1)     // of one sequence of a problem: the DP takes q_len + t_len below 2^27

__device__ __forceinline__ int al_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// seq_nt4_table: A C G T/U in either case and the bytes 0..3 themselves; everything else is ambiguous
__device__ __forceinline__ int al_nt4(uint32_t b)
{
	if (b < 4) return (int)b;
	const uint32_t l = b | 0x20u;
	return l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : (l == 't' || l == 'u') ? 3 : 4;
}
// qseq0[rev][i] of a read given as characters; 4 outside it
__device__ __forceinline__ int al_qbase(const char *seq, int qlen, int rev, int i)
{
	if ((unsigned)i >= (unsigned)qlen) return 4;
	if (!rev) return al_nt4((uint8_t)seq[i]);
	const int c = al_nt4((uint8_t)seq[qlen - 1 - i]);
	return c < 4 ? 3 - c : 4;
}
__device__ __forceinline__ int al_tbase(const uint8_t *t, int tlen, int i) { return (unsigned)i < (unsigned)tlen ? (int)t[i] : 4; }
__device__ __forceinline__ int al_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ int al_span(ulonglong2 a) { return (int)(a.y >> 32 & 0xff); }
__device__ __forceinline__ int al_mat(const AlignOpt &o, int ct, int cq) { return ct > 3 || cq > 3 ? 0 : ct == cq ? o.a : -o.b; }

__device__ __forceinline__ int al_scan_add(int v, int lane)
{
	for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v += t; }
	return v;
}
__device__ __forceinline__ int al_scan_min(int v, int lane)
{
	for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v = min(v, t); }
	return v;
}

// mm_fix_cigar and mm_update_extra (align.c:90-193) by one wave on the n words at cg, in place: the query is the read's strand rrev from
// qs1 on, the target t from rs1 on.  r: the region's words (a leading I or D shifts qs / qe / rs; mlen and blen are written); ex: its extra.
__device__ __forceinline__ void al_fix_and_extra(const AlignOpt &o, int lane, const char *seq, int qlen, int rrev, int qs1, const uint8_t *t, int tlen,
                                                 int rs1, uint32_t *cg, int n, int dp_score, int32_t *r, int32_t *ex)
{
	int qshift = 0, tshift = 0;
	auto qb = [&](int i) { return al_qbase(seq, qlen, rrev, qs1 + i); };
	auto tb = [&](int i) { return al_tbase(t, tlen, rs1 + i); };
	if (lane == 0 && n > 1) {       // mm_fix_cigar
		int toff = 0, qoff = 0, to_shrink = 0;
		for (int k = 0; k < n; ++k) {
			const int op = cg[k] & 0xf, len = (int)(cg[k] >> 4);
			if (len == 0) to_shrink = 1;
			if (op == 0) { toff += len; qoff += len; }
			else if (op == 1 || op == 2) {
				if (k > 0 && k < n - 1 && (cg[k - 1] & 0xf) == 0 && (cg[k + 1] & 0xf) == 0) {
					const int prev_len = (int)(cg[k - 1] >> 4);
					int l;
					if (op == 1) { for (l = 0; l < prev_len; ++l) if (qb(qoff - 1 - l) != qb(qoff + len - 1 - l)) break; }
					else { for (l = 0; l < prev_len; ++l) if (tb(toff - 1 - l) != tb(toff + len - 1 - l)) break; }
					if (l > 0) { cg[k - 1] -= (uint32_t)l << 4; cg[k + 1] += (uint32_t)l << 4; qoff -= l; toff -= l; }
					if (l == prev_len) to_shrink = 1;
				}
				if (op == 1) qoff += len; else toff += len;
			} else if (op == 3) toff += len;
		}
		if (to_shrink) {
			int l = 0;
			for (int k = 0; k < n; ++k) if (cg[k] >> 4 != 0) cg[l++] = cg[k];
			n = l;
			for (int k = l = 0; k < n; ++k)
				if (k == n - 1 || (cg[k] & 0xf) != (cg[k + 1] & 0xf)) cg[l++] = cg[k];
				else cg[k + 1] += cg[k] >> 4 << 4;
			n = l;
		}
		if (n > 0 && ((cg[0] & 0xf) == 1 || (cg[0] & 0xf) == 2)) {
			const int l = (int)(cg[0] >> 4);
			if ((cg[0] & 0xf) == 1) {
				if (rrev) r[5] -= l; else r[4] += l;
				qshift = l;
			} else { r[6] += l; tshift = l; }
			--n;
			for (int k = 0; k < n; ++k) cg[k] = cg[k + 1];
		}
	}
	wave_global_fence();
	n = al_uniform(n); qshift = al_uniform(qshift); tshift = al_uniform(tshift);
	// mm_update_extra: counts and scores of an op by the lanes; s and max follow the reference's clamp at 0 through a scan per 64 bases
	int blen = 0, mlen = 0, n_ambi_all = 0, s = 0, mx = 0, toff = tshift, qoff = qshift;
	for (int k = 0; k < n; ++k) {
		const uint32_t w = cg[k];
		const int op = w & 0xf, len = (int)(w >> 4);
		if (op == 0) {
			int n_ambi = 0, n_diff = 0;
			for (int b0 = 0; b0 < len; b0 += 64) {
				const int l = b0 + lane;
				int v = 0;
				if (l < len) {
					const int cq = qb(qoff + l), ct = tb(toff + l);
					if (ct > 3 || cq > 3) ++n_ambi;
					else if (ct != cq) ++n_diff;
					v = al_mat(o, ct, cq);
				}
				const int Q = s + al_scan_add(v, lane);
				const int m = min(al_scan_min(Q, lane), 0);
				mx = max(mx, wave_max_i(Q - m));
				s = __shfl(Q - m, 63);
			}
			n_ambi = wave_sum_i(n_ambi); n_diff = wave_sum_i(n_diff);
			blen += len - n_ambi; mlen += len - (n_ambi + n_diff); n_ambi_all += n_ambi;
			toff += len; qoff += len;
		} else if (op == 1 || op == 2) {
			int n_ambi = 0;
			for (int l = lane; l < len; l += 64) n_ambi += (op == 1 ? qb(qoff + l) : tb(toff + l)) > 3;
			n_ambi = wave_sum_i(n_ambi);
			blen += len - n_ambi; n_ambi_all += n_ambi;
			s -= o.q + o.e * len;
			if (s < 0) s = 0;
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	if (lane == 0) {
		r[12] = blen; r[11] = mlen;
		ex[0] = 1; ex[1] = dp_score; ex[2] = mx; ex[3] = n_ambi_all & 0x3fffffff; ex[4] = n;
	}
}

} // namespace chaindp
#endif
