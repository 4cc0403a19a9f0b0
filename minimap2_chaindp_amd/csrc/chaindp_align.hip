// chaindp_align.hip -- mm_align1 (reference align.c:423-636, without MM_F_SR / MM_F_SPLICE) around the dual-gap DP of chaindp_ksw.hip.
//
// One wave per region (k_align_plan, k_align_stitch, k_align_extra) or per problem (k_align_gather, k_align_zdrop):
//   k_align_plan     the anchors taken (mm_fix_bad_ends, mm_filter_bad_seeds with its MM_SEED_IGNORE marks, mm_adjust_minier), the bounds
//                    rs0 / qs0 / re0 / qe0, and one problem per extension and per gap fill: a gap fill's coordinates come from anchors alone,
//                    so all of them are known before any DP has run.  The right extension and the fills behind a Z-drop are computed on
//                    speculation and dropped by the stitcher.
//   k_align_gather   the problems' bases into the DP's base buffer, once the host has laid the problems out (the left extension reversed)
//   k_align_zdrop    mm_test_zdrop of every first-pass fill: the CIGAR walk, and where it fires the inversion score (ksw_ll_i16's return value)
//   k_align_stitch   left extension, fills up to the first drop (the second pass's answer where there is one), mm_split_reg, right extension
//   k_align_extra    mm_fix_cigar and mm_update_extra
//   k_align_pack     the CIGARs to their CSR places
// The anchor walks and the CIGAR walks are sequential in the reference and stay on lane 0; the gap count of mm_filter_bad_seeds, the
// gathers, mm_reg_set_coor's sums, the inversion score and the per-base part of mm_update_extra run on all lanes.
// Every base is fetched through a bounds check and every length is clamped to its sequence: where the reference would trip an assert the
// answer is unspecified, but nothing is read or written outside a buffer.
#include "chaindp_kernels.h"
#include "chaindp_wave.h"
#include "chaindp_post_dev.h"
#include "chaindp_align_plan.h"
#include "chaindp_align_dev.h"

namespace chaindp {

#define AL_SEED_LONG_JOIN (1ull << 40)
#define AL_SEED_IGNORE (1ull << 41)
#define AL_SEED_TANDEM (1ull << 42)
#define AL_SEED_SELF (1ull << 43)
__global__ __launch_bounds__(256) void k_align_encode(int64_t n, const char *__restrict__ seq, uint8_t *__restrict__ codes)
{
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) codes[i] = (uint8_t)al_nt4((uint8_t)seq[i]);
}

// mm_adjust_minier (align.c:254-269)
__device__ void al_adjust_minier(const AlignOpt &o, const char *seq, int qlen, const uint8_t *t, int tlen, ulonglong2 a, int &r, int &q)
{
	if (o.is_hpc) {
		const int rev = (int)(a.x >> 63);
		q = (int32_t)a.y;
		const int c = al_qbase(seq, qlen, rev, q);
		int i;
		for (i = q - 1; i > 0; --i)
			if (al_qbase(seq, qlen, rev, i) != c) break;
		q = i + 1;
		const int x = (int32_t)a.x, ct = al_tbase(t, tlen, x);
		for (i = x - 1; i >= 0; --i)
			if (al_tbase(t, tlen, i) != ct) break;
		r = x + 1 - (x - i);
	} else {
		r = (int32_t)a.x - (o.k >> 1);
		q = (int32_t)a.y - (o.k >> 1);
	}
}

__device__ __forceinline__ int al_gap(const ulonglong2 *a, int i)      // of mm_filter_bad_seeds: 32-bit arithmetic, as the reference's truncation leaves it
{
	return (int)(((uint32_t)a[i].y - (uint32_t)a[i - 1].y) - ((uint32_t)a[i].x - (uint32_t)a[i - 1].x));
}

// mm_filter_bad_seeds (align.c:271-315) once more than one long gap was counted: K[] in kbuf (room for cnt1 entries).  One lane.
__device__ void al_filter_bad_seeds(ulonglong2 *a, int cnt1, int *K, int min_gap, int diff_thres, int max_ext_len, int max_ext_cnt)
{
	int n = 0;
	for (int i = 1; i < cnt1; ++i) {
		const int gap = al_gap(a, i);
		if (gap < -min_gap || gap > min_gap) K[n++] = i;
	}
	int max = 0, max_st = -1, max_en = -1;
	for (int k = 0;; ++k) {
		if (k == n || k >= max_en) {
			if (max_en > 0)
				for (int i = K[max_st]; i < K[max_en]; ++i) a[i].y |= AL_SEED_IGNORE;
			max = 0; max_st = max_en = -1;
			if (k == n) break;
		}
		const int i = K[k];
		int gap = al_gap(a, i), n_ins = 0, n_del = 0, max_diff = 0, max_diff_l = -1;
		if (gap > 0) n_ins += gap; else n_del += -gap;
		const int qs = (int32_t)a[i - 1].y, rs = (int32_t)a[i - 1].x;
		for (int l = k + 1; l < n && l <= k + max_ext_cnt; ++l) {
			const int j = K[l];
			if ((int32_t)a[j].y - qs > max_ext_len || (int32_t)a[j].x - rs > max_ext_len) break;
			gap = al_gap(a, j);
			if (gap > 0) n_ins += gap; else n_del += -gap;
			const int d = n_ins - n_del, diff = n_ins + n_del - (d < 0 ? -d : d);
			if (max_diff < diff) { max_diff = diff; max_diff_l = l; }
		}
		if (max_diff > diff_thres && max_diff > max) { max = max_diff; max_st = k; max_en = max_diff_l; }
	}
}

__global__ __launch_bounds__(64) void k_align_plan(AlignOpt o, int n_regs, const int32_t *__restrict__ reg_read, const int64_t *__restrict__ seq_off,
                                                   const char *__restrict__ seq_all, const int64_t *__restrict__ a_off, ulonglong2 *a_all,
                                                   const int32_t *__restrict__ regs, int32_t *regs2, const int64_t *__restrict__ t_off,
                                                   const uint8_t *__restrict__ tcodes, const int64_t *__restrict__ slot_off, KswProb *slots,
                                                   AlignSide *side, AlignReg *areg, int32_t *kbuf)
{
	const int lane = threadIdx.x;
	for (int g = blockIdx.x; g < n_regs; g += gridDim.x) {
		const int32_t *r = regs + (int64_t)g * AL_REG_WORDS;
		const int cnt0 = r[1], as0 = r[10];
		if (lane == 0) regs2[(int64_t)g * AL_REG_WORDS + 1] = 0;
		if (cnt0 <= 0) {
			if (lane == 0) { AlignReg R = {}; areg[g] = R; }
			continue;
		}
		const int read = reg_read[g];
		ulonglong2 *a = a_all + a_off[read];
		const int n_a = (int)(a_off[read + 1] - a_off[read]);
		const char *seq = seq_all + seq_off[read];
		const int qlen = (int)(seq_off[read + 1] - seq_off[read]);
		const ulonglong2 a0 = a[as0];
		const int rid = (int)(a0.x << 1 >> 33), rev = (int)(a0.x >> 63);
		const uint8_t *t = tcodes + t_off[rid];
		const int tlen = (int)(t_off[rid + 1] - t_off[rid]);
		// mm_fix_bad_ends (align.c:317-351)
		int as1 = as0, cnt1 = cnt0;
		if (lane == 0 && cnt0 >= 3) {
			const int bw = o.bw, min_match = o.min_chain_score * 2, mlen = r[11];
			int m, l;
			m = l = al_span(a[as0]);
			for (int i = as0 + 1; i < as0 + cnt0 - 1; ++i) {
				if (a[i].y & AL_SEED_LONG_JOIN) break;
				const int q_span = al_span(a[i]);
				const int lr = (int32_t)a[i].x - (int32_t)a[i - 1].x, lq = (int32_t)a[i].y - (int32_t)a[i - 1].y;
				const int mn = lr < lq ? lr : lq, mx = lr > lq ? lr : lq;
				if (mx - mn > l >> 1) as1 = i;
				l += mn;
				m += mn < q_span ? mn : q_span;
				if (l >= bw << 1 || (m >= min_match && m >= bw) || m >= mlen >> 1) break;
			}
			cnt1 = as0 + cnt0 - as1;
			m = l = al_span(a[as0 + cnt0 - 1]);
			for (int i = as0 + cnt0 - 2; i > as1; --i) {
				if (a[i + 1].y & AL_SEED_LONG_JOIN) break;
				const int q_span = al_span(a[i + 1]);
				const int lr = (int32_t)a[i + 1].x - (int32_t)a[i].x, lq = (int32_t)a[i + 1].y - (int32_t)a[i].y;
				const int mn = lr < lq ? lr : lq, mx = lr > lq ? lr : lq;
				if (mx - mn > l >> 1) cnt1 = i + 1 - as1;
				l += mn;
				m += mn < q_span ? mn : q_span;
				if (l >= bw << 1 || (m >= min_match && m >= bw) || m >= mlen >> 1) break;
			}
		}
		as1 = al_uniform(as1); cnt1 = al_uniform(cnt1);
		// mm_filter_bad_seeds: the long gaps counted by all lanes; the walk over them, where there are two or more, by one
		int n_long = 0;
		for (int i = 1 + lane; i < cnt1; i += 64) {
			const int gap = al_gap(a + as1, i);
			n_long += gap < -10 || gap > 10;
		}
		n_long = wave_sum_i(n_long);
		if (lane == 0) {
		if (n_long > 1) al_filter_bad_seeds(a + as1, cnt1, kbuf + slot_off[g], 10, 40, o.max_gap >> 1, 10);
		int rs, qs, re, qe;
		al_adjust_minier(o, seq, qlen, t, tlen, a[as1], rs, qs);
		al_adjust_minier(o, seq, qlen, t, tlen, a[as1 + cnt1 - 1], re, qe);
		// the bounds (align.c:478-538)
		int rs0 = (int32_t)a0.x + 1 - al_span(a0), qs0 = (int32_t)a0.y + 1 - al_span(a0), rs1 = 0, qs1 = 0, l = 0;
		if (rs0 < 0) rs0 = 0;
		for (int i = as0 - 1; i >= 0 && a[i].x >> 32 == a0.x >> 32; --i) {
			const int x = (int32_t)a[i].x + 1 - al_span(a[i]), y = (int32_t)a[i].y + 1 - al_span(a[i]);
			if (x < rs0 && y < qs0) {
				if (++l > o.min_cnt) {
					l = rs0 - x > qs0 - y ? rs0 - x : qs0 - y;
					rs1 = rs0 - l; qs1 = qs0 - l;
					break;
				}
			}
		}
		if (qs > 0 && rs > 0) {
			l = qs < o.max_gap ? qs : o.max_gap;
			qs1 = qs1 > qs - l ? qs1 : qs - l;
			qs0 = qs0 < qs1 ? qs0 : qs1;
			l += l * o.a > o.q ? (o.e ? (l * o.a - o.q) / o.e : 0) : 0;
			l = l < o.max_gap ? l : o.max_gap;
			l = l < rs ? l : rs;
			rs1 = rs1 > rs - l ? rs1 : rs - l;
			rs0 = rs0 < rs1 ? rs0 : rs1;
		} else { rs0 = rs; qs0 = qs; }
		const ulonglong2 al = a[as0 + cnt0 - 1];
		int re0 = (int32_t)al.x + 1, qe0 = (int32_t)al.y + 1, re1 = tlen, qe1 = qlen;
		l = 0;
		for (int i = as0 + cnt0; i < n_a && a[i].x >> 32 == a0.x >> 32; ++i) {
			const int x = (int32_t)a[i].x + 1, y = (int32_t)a[i].y + 1;
			if (x > re0 && y > qe0) {
				if (++l > o.min_cnt) {
					l = x - re0 > y - qe0 ? x - re0 : y - qe0;
					re1 = re0 + l; qe1 = qe0 + l;
					break;
				}
			}
		}
		if (qe < qlen && re < tlen) {
			l = qlen - qe < o.max_gap ? qlen - qe : o.max_gap;
			qe1 = qe1 < qe + l ? qe1 : qe + l;
			qe0 = qe0 > qe1 ? qe0 : qe1;
			l += l * o.a > o.q ? (o.e ? (l * o.a - o.q) / o.e : 0) : 0;
			l = l < o.max_gap ? l : o.max_gap;
			l = l < tlen - re ? l : tlen - re;
			re1 = re1 < re + l ? re1 : re + l;
			re0 = re0 > re1 ? re0 : re1;
		} else { re0 = re; qe0 = qe; }
		if (a0.y & AL_SEED_SELF) {
			int max_ext = r[4] > r[6] ? r[4] - r[6] : r[6] - r[4];
			if (r[6] - rs0 > max_ext) rs0 = r[6] - max_ext;
			if (r[4] - qs0 > max_ext) qs0 = r[4] - max_ext;
			max_ext = r[5] > r[7] ? r[5] - r[7] : r[7] - r[5];
			if (re0 - r[7] > max_ext) re0 = r[7] + max_ext;
			if (qe0 - r[5] > max_ext) qe0 = r[5] + max_ext;
		}
		// the problems, in the order mm_align1 runs them
		const int64_t s0 = slot_off[g];
		const int room = (int)(slot_off[g + 1] - s0);
		const int bw = (int)(o.bw * 1.5 + 1.);
		int np = 0;
		auto emit = [&](int kind, int i, int rs_, int qs_, int tl, int ql, int w, int zdrop, int end_bonus, int flag) {
			if (np >= room) return;
			ql = al_clamp(ql, 0, qlen < AL_LEN_MAX ? qlen : AL_LEN_MAX); tl = al_clamp(tl, 0, tlen < AL_LEN_MAX ? tlen : AL_LEN_MAX);
			const int wmax = ql > tl ? ql : tl;
			slots[s0 + np] = KswProb{0, 0, 0, ql, tl, w < wmax ? w : wmax, zdrop, end_bonus, flag};
			side[s0 + np] = AlignSide{g, kind, i, rs_, qs_, 0};
			++np;
		};
		AlignReg R = {as1, cnt1, rid, rev, rs, qs, 0, 0, rs0, qs0, re0, qe0, 0, qlen, tlen, 0};
		if (qs > 0 && rs > 0)
			emit(AL_LEFT, 0, rs0, qs0, rs - rs0, qs - qs0, bw, (r[15] & AL_BIT_SPLIT_INV) ? o.zdrop_inv : o.zdrop, o.end_bonus,
			     AL_EZ_EXTZ_ONLY | AL_EZ_RIGHT | AL_EZ_REV_CIGAR);
		for (int i = 1; i < cnt1; ++i) {
			const ulonglong2 ai = a[as1 + i];
			if ((ai.y & (AL_SEED_IGNORE | AL_SEED_TANDEM)) && i != cnt1 - 1) continue;
			al_adjust_minier(o, seq, qlen, t, tlen, ai, re, qe);
			if (i == cnt1 - 1 || (ai.y & AL_SEED_LONG_JOIN) || (qe - qs >= o.min_ksw_len && re - rs >= o.min_ksw_len)) {
				int bw1 = bw;
				if (ai.y & AL_SEED_LONG_JOIN) bw1 = qe - qs > re - rs ? qe - qs : re - rs;
				emit(AL_FILL, i, rs, qs, re - rs, qe - qs, bw1, o.zdrop, -1, AL_EZ_APPROX_MAX);
				rs = re; qs = qe;
			}
		}
		R.re = re; R.qe = qe;
		if (qe < qe0 && re < re0) emit(AL_RIGHT, cnt1, re, qe, re0 - re, qe0 - qe, bw, o.zdrop, o.end_bonus, AL_EZ_EXTZ_ONLY);
		R.n_prob = np;
		areg[g] = R;
		}      // lane 0
	}
}

// the bases of every problem: the query from the read's mapped strand, the target from the resident codes, the left extension reversed
__global__ __launch_bounds__(64) void k_align_gather(int n, const KswProb *__restrict__ prob, const int32_t *__restrict__ src_slot,
                                                     const AlignSide *__restrict__ side, const AlignReg *__restrict__ areg,
                                                     const int32_t *__restrict__ reg_read, const int64_t *__restrict__ seq_off,
                                                     const char *__restrict__ seq_all, const int64_t *__restrict__ t_off,
                                                     const uint8_t *__restrict__ tcodes, uint8_t *bases)
{
	const int lane = threadIdx.x;
	for (int c = blockIdx.x; c < n; c += gridDim.x) {
		const KswProb p = prob[c];
		const AlignSide sd = side[src_slot[c]];
		const AlignReg R = areg[sd.reg];
		const int read = reg_read[sd.reg];
		const char *seq = seq_all + seq_off[read];
		const uint8_t *t = tcodes + t_off[R.rid];
		const bool left = sd.kind == AL_LEFT;
		for (int k = lane; k < p.qlen; k += 64) bases[p.q_beg + k] = (uint8_t)al_qbase(seq, R.qlen, R.rev, left ? sd.qs + p.qlen - 1 - k : sd.qs + k);
		for (int k = lane; k < p.tlen; k += 64) bases[p.t_beg + k] = (uint8_t)al_tbase(t, R.tlen, left ? sd.rs + p.tlen - 1 - k : sd.rs + k);
	}
}

// mm_test_zdrop (align.c:46-88) of the first-pass fill c: code[c] = 0, 1 (Z-drop) or 2 (a potential inversion).  lds_t: entries per LDS array.
extern __shared__ __attribute__((aligned(16))) uint16_t al_lds[];
__global__ __launch_bounds__(64) void k_align_zdrop(AlignOpt o, int n, const KswProb *__restrict__ prob, const int32_t *__restrict__ src_slot,
                                                    const AlignSide *__restrict__ side, const uint8_t *__restrict__ bases,
                                                    const int32_t *__restrict__ ez, const uint32_t *__restrict__ cig, int lds_t, int32_t *code)
{
	const int lane = threadIdx.x;
	for (int c = blockIdx.x; c < n; c += gridDim.x) {
		if (side[src_slot[c]].kind != AL_FILL) { if (lane == 0) code[c] = 0; continue; }
		const KswProb p = prob[c];
		const uint8_t *qseq = bases + p.q_beg, *tseq = bases + p.t_beg;
		int max_zdrop = 0, p00 = -1, p01 = -1, p10 = -1, p11 = -1;
		if (lane == 0) {
			const int n_cigar = ez[(int64_t)c * KSW_EZ_WORDS + 10];
			const uint32_t *cg = cig + p.cig_beg;
			int score = 0, max = INT_MIN, max_i = -1, max_j = -1, i = 0, j = 0;
			auto update = [&](int i_, int j_) {
				if (score < max) {
					const int li = i_ - max_i, lj = j_ - max_j, diff = li > lj ? li - lj : lj - li, z = max - score - diff * o.e;
					if (z > max_zdrop) { max_zdrop = z; p00 = max_i; p01 = i_ + 1; p10 = max_j; p11 = j_ + 1; }
				} else { max = score; max_i = i_; max_j = j_; }
			};
			for (int k = 0; k < n_cigar; ++k) {
				const int op = cg[k] & 0xf, len = (int)(cg[k] >> 4);
				if (op == 0) {
					if (i + len > p.tlen || j + len > p.qlen) break;
					for (int l = 0; l < len; ++l) {
						score += al_mat(o, tseq[i + l], qseq[j + l]);
						update(i + l, j + l);
					}
					i += len; j += len;
				} else if (op == 1 || op == 2 || op == 3) {
					score -= o.q + o.e * len;
					if (op == 1) j += len; else i += len;
					update(i, j);
				}
			}
		}
		max_zdrop = al_uniform(max_zdrop); p00 = al_uniform(p00); p01 = al_uniform(p01); p10 = al_uniform(p10); p11 = al_uniform(p11);
		const int q_len = p11 - p10, t_len = p01 - p00;
		int result = max_zdrop > o.zdrop ? 1 : 0;
		const bool in_range = p00 >= 0 && p10 >= 0 && p01 <= p.tlen && p11 <= p.qlen && q_len > 0 && t_len > 0 && t_len + 1 <= lds_t;
		if (!(o.flag & AL_F_NO_INV_TEST) && max_zdrop > o.zdrop_inv && q_len < o.max_gap && t_len < o.max_gap && in_range) {
			// ksw_ll_i16's return value: the local score of the stretch's reverse complement against the target stretch, gap of length l
			// costing q + l e, cells floored at 0 and capped at 32767.  Anti-diagonals; of a diagonal, 64 target bases at a time from the top
			// down, so that the in-place arrays (index i + 1 = target base i; H of the last two diagonals, E, F) are read before written.
			uint16_t *H1 = al_lds, *H2 = H1 + lds_t, *E = H2 + lds_t, *F = E + lds_t;
			for (int k = lane; k < 4 * lds_t; k += 64) al_lds[k] = 0;
			wave_mem_fence();
			const int oe = o.q + o.e, ge = o.e;
			int best = 0;
			for (int d = 0; d < q_len + t_len - 1; ++d) {
				const int lo = d - q_len + 1 > 0 ? d - q_len + 1 : 0, hi = d < t_len - 1 ? d : t_len - 1;
				for (int top = hi; top >= lo; top -= 64) {
					const int i = top - lane;
					int h = 0, e = 0, f = 0, old = 0;
					const bool on = i >= lo;
					if (on) {
						const int cq0 = qseq[p11 - 1 - (d - i)], cq = cq0 >= 4 ? 4 : 3 - cq0, ct = tseq[p00 + i];
						const int h_up = H1[i], h_left = H1[i + 1];
						old = h_left;
						e = max(max(h_up - oe, (int)E[i] - ge), 0);
						f = max(max(h_left - oe, (int)F[i + 1] - ge), 0);
						h = min((int)H2[i] + al_mat(o, ct, cq), 32767);
						h = max(max(h, e), f);
					}
					wave_mem_fence();
					if (on) { H1[i + 1] = (uint16_t)h; H2[i + 1] = (uint16_t)old; E[i + 1] = (uint16_t)e; F[i + 1] = (uint16_t)f; }
					wave_mem_fence();
					best = max(best, h);
				}
			}
			best = wave_max_i(best);
			if (best >= o.min_chain_score * o.a && best >= o.min_dp_max) result = 2;
		}
		if (lane == 0) code[c] = result;
		wave_mem_fence();
	}
}

// left extension, fills up to the first drop, mm_split_reg, right extension (align.c:543-625): the appended CIGAR into stage, the
// region's new coordinates into regs, the split-off region into regs2.
__global__ __launch_bounds__(64) void k_align_stitch(AlignOpt o, int n_regs, int64_t n_prob, int64_t cig_total, const int32_t *__restrict__ reg_read,
                                                     const int64_t *__restrict__ seq_off, const int64_t *__restrict__ a_off,
                                                     const ulonglong2 *__restrict__ a_all, int32_t *regs, int32_t *regs2,
                                                     const AlignReg *__restrict__ areg, const int64_t *__restrict__ first,
                                                     const int32_t *__restrict__ src_slot, const AlignSide *__restrict__ side,
                                                     const KswProb *__restrict__ prob, const int32_t *__restrict__ ez1, const uint32_t *__restrict__ cig1,
                                                     const int32_t *__restrict__ code, const int32_t *__restrict__ sec, const KswProb *__restrict__ prob2,
                                                     const int32_t *__restrict__ ez2, const uint32_t *__restrict__ cig2, uint32_t *stage, AlignStitch *stitch)
{
	__shared__ int pf[PF_NF * 2];
	const int lane = threadIdx.x;
	for (int g = blockIdx.x; g < n_regs; g += gridDim.x) {
		int32_t *r = regs + (int64_t)g * AL_REG_WORDS, *r2 = regs2 + (int64_t)g * AL_REG_WORDS;
		AlignStitch S = {};
		if (r[1] <= 0) { if (lane == 0) stitch[g] = S; continue; }
		const AlignReg R = areg[g];
		const int read = reg_read[g];
		const ulonglong2 *a = a_all + a_off[read];
		const int qlen = (int)(seq_off[read + 1] - seq_off[read]);
		int split_n = 0, split_code = 0;
		if (lane == 0) {
			const int64_t c0 = first[g], c1 = first[g + 1];
			const int64_t beg = c0 < c1 ? prob[c0].cig_beg : 0, end = c0 < c1 ? (c1 < n_prob ? prob[c1].cig_beg : cig_total) : 0;
			uint32_t *out = stage + beg;
			const int64_t room = end - beg;
			int n = 0, dp = 0, has_p = 0, dropped = 0;
			auto append = [&](const uint32_t *src, int m) {        // mm_append_cigar
				if (m <= 0) return;
				has_p = 1;
				int k = 0;
				if (n > 0 && (out[n - 1] & 0xf) == (src[0] & 0xf)) { out[n - 1] += src[0] >> 4 << 4; k = 1; }
				for (; k < m && n < room; ++k) out[n++] = src[k];
			};
			int rs1 = R.rs, qs1 = R.qs, re1 = R.re, qe1 = R.qe;
			for (int64_t c = c0; c < c1; ++c) {
				const AlignSide sd = side[src_slot[c]];
				const int32_t *ez = ez1 + c * KSW_EZ_WORDS;
				const uint32_t *cg = cig1 + prob[c].cig_beg;
				if (sd.kind == AL_LEFT) {
					if (ez[10] > 0) { append(cg, ez[10]); dp += ez[0]; }
					rs1 = R.rs - (ez[9] ? ez[5] + 1 : ez[3] + 1);
					qs1 = R.qs - (ez[9] ? R.qs - R.qs0 : ez[2] + 1);
				} else if (sd.kind == AL_FILL) {
					if (dropped) continue;
					if (sec[c] >= 0) { ez = ez2 + (int64_t)sec[c] * KSW_EZ_WORDS; cg = cig2 + prob2[sec[c]].cig_beg; }
					append(cg, ez[10]);
					if (ez[1]) {
						int j;
						for (j = sd.i - 1; j >= 0; --j)
							if ((int32_t)a[R.as1 + j].x <= sd.rs + ez[3]) break;
						dropped = 1;
						if (j < 0) j = 0;
						dp += ez[0];
						re1 = sd.rs + (ez[3] + 1); qe1 = sd.qs + (ez[2] + 1);
						if (R.cnt1 - (j + 1) >= o.min_cnt) { split_n = R.as1 + j + 1 - r[10]; split_code = code[c]; }
					} else dp += ez[8];
				} else if (!dropped) {
					if (ez[10] > 0) { append(cg, ez[10]); dp += ez[0]; }
					re1 = R.re + (ez[9] ? ez[5] + 1 : ez[3] + 1);
					qe1 = R.qe + (ez[9] ? R.qe0 - R.qe : ez[2] + 1);
				}
			}
			S.n_cigar = n; S.dp_score = dp; S.has_p = has_p; S.rs1 = rs1; S.re1 = re1; S.qs1 = qs1; S.qe1 = qe1;
			stitch[g] = S;
		}
		split_n = al_uniform(split_n); split_code = al_uniform(split_code);
		const int cnt = r[1];
		if (split_n > 0 && split_n < cnt) {          // mm_split_reg (hit.c:90-107); slot 0 is r, slot 1 is r2
			const PostFields Fd = {pf, 2};
			const int score = r[3], cnt2 = cnt - split_n;
			const int score2 = (int)((double)((float)score * ((float)cnt2 / (float)cnt)) + .499);
			if (lane == 0) {
				Fd(PF_AS, 0) = r[10]; Fd(PF_CNT, 0) = split_n; Fd(PF_BITS, 0) = (int)((uint32_t)r[15] | AL_BIT_SPLIT);
				Fd(PF_AS, 1) = r[10] + split_n; Fd(PF_CNT, 1) = cnt2;
				Fd(PF_BITS, 1) = (int)((((uint32_t)r[15] & ~(BIT_SAM_PRI | AL_BIT_SPLIT_INV)) | AL_BIT_SPLIT << 1) | (split_code == 2 ? AL_BIT_SPLIT_INV : 0u));
			}
			wave_mem_fence();
			post_set_coor(Fd, 1, qlen, a, lane);
			post_set_coor(Fd, 0, qlen, a, lane);
			wave_mem_fence();
			if (lane == 0) {
				for (int k = 0; k < AL_REG_WORDS; ++k) r2[k] = r[k];
				r2[0] = -1; r2[1] = cnt2; r2[3] = score2; r2[10] = r[10] + split_n;
				if (r[8] == r[0]) r2[8] = POST_PARENT_TMP_PRI;
				r2[2] = Fd(PF_RID, 1); r2[4] = Fd(PF_QS, 1); r2[5] = Fd(PF_QE, 1); r2[6] = Fd(PF_RS, 1); r2[7] = Fd(PF_RE, 1);
				r2[11] = Fd(PF_MLEN, 1); r2[12] = Fd(PF_BLEN, 1); r2[15] = Fd(PF_BITS, 1); r2[18] = 0; r2[19] = 0;
				r[1] = split_n; r[3] = score - score2; r[2] = Fd(PF_RID, 0); r[11] = Fd(PF_MLEN, 0); r[12] = Fd(PF_BLEN, 0); r[15] = Fd(PF_BITS, 0);
			}
			wave_mem_fence();
		}
		if (lane == 0) {
			r[6] = S.rs1; r[7] = S.re1;
			if (R.rev) { r[4] = qlen - S.qe1; r[5] = qlen - S.qs1; }
			else { r[4] = S.qs1; r[5] = S.qe1; }
		}
	}
}

// mm_update_extra with mm_fix_cigar (align.c:90-193) on the stitched CIGAR of every region that has one
__global__ __launch_bounds__(64) void k_align_extra(AlignOpt o, int n_regs, int64_t n_prob, const int32_t *__restrict__ reg_read,
                                                    const int64_t *__restrict__ seq_off, const char *__restrict__ seq_all,
                                                    const int64_t *__restrict__ t_off, const uint8_t *__restrict__ tcodes, int32_t *regs,
                                                    const AlignReg *__restrict__ areg, const int64_t *__restrict__ first,
                                                    const KswProb *__restrict__ prob, uint32_t *stage, const AlignStitch *__restrict__ stitch, int32_t *extra)
{
	const int lane = threadIdx.x;
	for (int g = blockIdx.x; g < n_regs; g += gridDim.x) {
		int32_t *r = regs + (int64_t)g * AL_REG_WORDS, *ex = extra + (int64_t)g * 5;
		const AlignStitch S = stitch[g];
		if (r[1] <= 0 || !S.has_p) {
			if (lane < 5) ex[lane] = 0;
			continue;
		}
		const AlignReg R = areg[g];
		const int read = reg_read[g];
		const char *seq = seq_all + seq_off[read];
		const uint8_t *t = tcodes + t_off[R.rid];
		const int rrev = (int)((uint32_t)r[15] >> 10 & 1);
		uint32_t *cg = stage + (first[g] < n_prob ? prob[first[g]].cig_beg : 0);
		al_fix_and_extra(o, lane, seq, R.qlen, rrev, S.qs1, t, R.tlen, S.rs1, cg, S.n_cigar, S.dp_score, r, ex);
	}
}

__global__ __launch_bounds__(64) void k_align_pack(int n_regs, int64_t n_prob, const int64_t *__restrict__ first, const KswProb *__restrict__ prob,
                                                   const int32_t *__restrict__ extra, const int64_t *__restrict__ off, const uint32_t *__restrict__ stage,
                                                   uint32_t *__restrict__ out)
{
	for (int g = blockIdx.x; g < n_regs; g += gridDim.x) {
		const int m = extra[(int64_t)g * 5 + 4];
		const uint32_t *src = stage + (first[g] < n_prob ? prob[first[g]].cig_beg : 0);
		uint32_t *dst = out + off[g];
		for (int k = threadIdx.x; k < m; k += 64) dst[k] = src[k];
	}
}

static unsigned al_grid(int64_t n) { return (unsigned)(n < 1 ? 1 : n < 65536 ? n : 65536); }

hipError_t launch_align_encode(hipStream_t st, int64_t n, const char *d_seq, uint8_t *d_codes)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_align_encode, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, st, n, d_seq, d_codes);
	return hipGetLastError();
}

hipError_t launch_align_plan(hipStream_t st, const AlignOpt &o, const AlignDev &d)
{
	if (d.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_align_plan, dim3(al_grid(d.n_regs)), dim3(64), 0, st, o, d.n_regs, d.reg_read, d.seq_off, d.seq, d.a_off, (ulonglong2*)d.a, d.regs,
	                   d.regs2, d.t_off, d.tcodes, d.slot_off, d.slots, d.side, d.areg, d.kbuf);
	return hipGetLastError();
}

hipError_t launch_align_gather(hipStream_t st, const AlignDev &d, uint8_t *d_bases)
{
	if (d.n_prob <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_align_gather, dim3(al_grid(d.n_prob)), dim3(64), 0, st, (int)d.n_prob, d.prob, d.src_slot, d.side, d.areg, d.reg_read, d.seq_off, d.seq,
	                   d.t_off, d.tcodes, d_bases);
	return hipGetLastError();
}

hipError_t launch_align_zdrop(hipStream_t st, const AlignOpt &o, const AlignDev &d, const uint8_t *d_bases, const int32_t *d_ez, const uint32_t *d_cig, int lds_t)
{
	if (d.n_prob <= 0) return hipSuccess;
	const size_t lds = (size_t)lds_t * 4 * sizeof(uint16_t);
	const hipError_t e = hipFuncSetAttribute((const void*)k_align_zdrop, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds > 65536 ? lds : 65536));
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_align_zdrop, dim3(al_grid(d.n_prob)), dim3(64), lds, st, o, (int)d.n_prob, d.prob, d.src_slot, d.side, d_bases, d_ez, d_cig, lds_t, d.code);
	return hipGetLastError();
}

hipError_t launch_align_stitch(hipStream_t st, const AlignOpt &o, const AlignDev &d, int64_t cig_total, const KswProb *d_prob2, const int32_t *d_ez2,
                               const uint32_t *d_cig2)
{
	if (d.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_align_stitch, dim3(al_grid(d.n_regs)), dim3(64), 0, st, o, d.n_regs, d.n_prob, cig_total, d.reg_read, d.seq_off, d.a_off,
	                   (const ulonglong2*)d.a, d.regs, d.regs2, d.areg, d.first, d.src_slot, d.side, d.prob, d.ez1, d.cig1, d.code, d.sec, d_prob2, d_ez2,
	                   d_cig2, d.stage, d.stitch);
	return hipGetLastError();
}

hipError_t launch_align_extra(hipStream_t st, const AlignOpt &o, const AlignDev &d)
{
	if (d.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_align_extra, dim3(al_grid(d.n_regs)), dim3(64), 0, st, o, d.n_regs, d.n_prob, d.reg_read, d.seq_off, d.seq, d.t_off, d.tcodes, d.regs,
	                   d.areg, d.first, d.prob, d.stage, d.stitch, d.extra);
	return hipGetLastError();
}

hipError_t launch_align_pack(hipStream_t st, const AlignDev &d, const int64_t *d_off, uint32_t *d_out)
{
	if (d.n_regs <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_align_pack, dim3(al_grid(d.n_regs)), dim3(64), 0, st, d.n_regs, d.n_prob, d.first, d.prob, d.extra, d_off, d.stage, d_out);
	return hipGetLastError();
}

} // namespace chaindp
