/*
 * chaindp_align_post.h -- aligned reads finished on the device (the tail of align_regs and mm_set_mapq) of the C ABI in chaindp.h
 * (libchaindp_hip.so).  chaindp.h includes this header behind chaindp_align_reads.h, whose result it works on; including chaindp.h
 * gives all of them.
 */
#ifndef CHAINDP_ALIGN_POST_H
#define CHAINDP_ALIGN_POST_H

#include "chaindp_align_reads.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- what the reference does with a read's regions between mm_align_skeleton and the output (map.c:253-257, 876) ---------------------
 * mm_set_parent with r->p set (dp_max2 and the sub_diff rule of hit.c:152-155), mm_select_sub (a dropped region's CIGAR goes with
 * it), mm_set_sam_pri; then mm_set_mapq with its r->p branches and mm_set_inv_mapq.  With CHAINDP_F_ALL_CHAINS only the mapq step
 * runs, as in the reference.  Single-segment reads; nothing is repaired: mm_set_parent resets neither r[0].n_sub nor any subsc,
 * mm_select_sub compacts in place while it reads r[p], identical hits after DP set no dp_max2, an inversion (as == 0) gets the mapq
 * of whatever neighbours the (as, i) order of the primaries gives it, and (int) of a float outside the int range is INT_MIN.
 *   opt                              match_sc, sub_diff, is_sr are read here; min_cnt and the join limits are not
 *   rep_len[n_reads]                 mm_set_mapq's rep_len per read
 *   out_off[n_reads + 1]             out: read i's final regions are out_regs[out_off[i] .. out_off[i + 1])
 *   out_regs, out_extra, out_dp_max2 out: room for regs_cap regions: every word of each region (id, parent, subsc, n_sub, and in the
 *                                    bit-field word mapq and sam_pri, as the reference leaves them), what r->p holds beside the CIGAR,
 *                                    and r->p->dp_max2 (0 where has_extra == 0)
 *   cigar_off[regs_cap + 1], cigar   out: the CIGAR words of the final regions, CSR; room for cigar_cap words
 *   need[2]                          out, always: the final regions and their CIGAR words
 * CHAINDP_ERR_CAPACITY if regs_cap < need[0] or cigar_cap < need[1]: out_off and need are exact, the other outputs untouched, and
 * chaindp_align_post_fetch delivers the same result into larger arrays without computing anything again.  The result stays resident,
 * in buffers of its own, until the next of these calls on the context.  The arrays may be NULL with their capacity 0.
 * CHAINDP_ERR_CAPACITY (no result resident) also where mm_set_mapq would take the logarithm of a dp_max, a score or an n_sub + 1
 * above 2^24: the guarantee that logf is the host's, bit for bit, ends there.
 * CHAINDP_ERR_ARG (nothing launched, context usable): MM_F_SR or MM_F_SPLICE in opt->flag; match_sc <= 0; a negative rep_len or
 * capacity; a capacity without its arrays; NULL opt, out_off, need or rep_len; and what each call says below. */

/* On the resident result of the last chaindp_align_reads of the context, which stays valid (chaindp_align_reads_fetch works as before).
 * CHAINDP_ERR_ARG also when no such result is resident or it is not of n_reads reads. */
int chaindp_align_post(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, int64_t *out_off, chaindp_reg_t *out_regs,
                       chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap,
                       int64_t need[2]);
/* On regions from the host, in the form chaindp_align_reads returns them: regs_off[n_reads + 1], regs, extra, in_cigar_off[n + 1],
 * in_cigar, all only read.  A region with has_extra == 0 takes the reference's r->p == NULL branches.  CHAINDP_ERR_ARG also for
 * offsets that do not ascend from 0, an extra.n_cigar that disagrees with in_cigar_off, has_extra outside 0 / 1. */
int chaindp_align_post_regs(chaindp_ctx_t *ctx, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, const int64_t *regs_off,
                            const chaindp_reg_t *regs, const chaindp_align_extra_t *extra, const int64_t *in_cigar_off, const uint32_t *in_cigar, int64_t *out_off,
                            chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar,
                            int64_t cigar_cap, int64_t need[2]);
/* chaindp_align_reads and chaindp_align_post in one call: only the final result comes down.  The arguments and refusals of both; a
 * comes back with its marks, and both results are resident afterwards. */
int chaindp_align_reads_post(chaindp_ctx_t *ctx, const chaindp_align_opt_t *aopt, const chaindp_post_opt_t *opt, int64_t n_reads, const int64_t *seq_off,
                             const char *seq, const int64_t *a_off, chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, const int32_t *rep_len,
                             int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off,
                             uint32_t *cigar, int64_t cigar_cap, int64_t need[2]);
/* The resident result of the last of the three calls above once more.  CHAINDP_ERR_ARG when none is resident or n_reads is not that
 * call's; CHAINDP_ERR_CAPACITY as above. */
int chaindp_align_post_fetch(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2,
                             int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2]);

/* ---- test and tuning hooks -- NOT part of the stable ABI, in the sense of chaindp_debug.h */
/* No GPU needed: what chaindp_align_post_regs makes of its arguments before anything touches the device (regs_off NULL: what
 * chaindp_align_post makes of opt, rep_len and the capacities).  Returns CHAINDP_OK or CHAINDP_ERR_ARG; out[0] = regions, out[1] =
 * CIGAR words handed in. */
int chaindp_align_post_debug_check(const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, const int64_t *regs_off, const chaindp_reg_t *regs,
                                   const chaindp_align_extra_t *extra, const int64_t *in_cigar_off, const uint32_t *in_cigar, int64_t regs_cap, int64_t cigar_cap,
                                   int64_t out[2]);
/* Lists of up to cap regions (1 .. the built-in cap, which 0 restores) are staged in LDS, longer ones in global memory.  Launches nothing;
 * out_cap (or NULL) receives the built-in cap. */
int chaindp_align_post_debug_set_lds_cap(chaindp_ctx_t *ctx, int cap, int32_t *out_cap);
/* Device milliseconds of the last of the three calls made while profiling was on: k_apost_read with the scans, the gathers; -1 each
 * before. */
int chaindp_align_post_debug_ms(chaindp_ctx_t *ctx, double ms[2]);
/* The dp_max in [1, 2^24] at which the host's logf((float)dp_max / match_sc) is not the float the device computes by itself, with the
 * host's values (needs no GPU): returns their number and fills the first cap of k and v (either may be NULL); -1 for match_sc <= 0. */
int64_t chaindp_apost_logf_patches(int32_t match_sc, uint32_t *k, float *v, int64_t cap);
/* The number of dp_max in [1, kmax] at which the device's logf((float)dp_max / match_sc) differs from the host's in any bit; a
 * negative error code. */
int64_t chaindp_apost_logf_selftest(chaindp_ctx_t *ctx, int32_t match_sc, int32_t kmax);

#ifdef __cplusplus
}
#endif
#endif
