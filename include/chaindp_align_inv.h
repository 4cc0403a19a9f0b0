/*
 * chaindp_align_inv.h -- the inversion between two split regions (mm_align1_inv) of the C ABI in chaindp.h (libchaindp_hip.so).
 * chaindp.h includes this header behind chaindp_align.h, whose types and targets it uses; including chaindp.h gives all of them.
 */
#ifndef CHAINDP_ALIGN_INV_H
#define CHAINDP_ALIGN_INV_H

#include "chaindp_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mm_align1_inv between the regions mm_align1 split at a potential inversion (align.c:638-693, the loop's rule :747-753) ----------
 * After all chaindp_align1 rounds: regs holds each read's regions in mm_align_skeleton's order, what regs2 split off inserted behind
 * its region and no inversion records among them.  The call only reads regs (split, id, parent, rid, rev, split_inv, qs, qe, rs, re).
 * Slot g, region i >= 1 of its read, describes the pair (i - 1, i); a read's first slot is always 0.  For a pair that passes the early
 * returns, the stretch between the two regions is aligned on the opposite strand: ksw_ll_i16 with its end positions on the reversed
 * stretches (the query padded to a multiple of eight bases as the reference's striped layout pads it, so that the start of the
 * extension may lie up to seven read bases before the stretch), then chaindp_ksw_extd's kernel from there with w = (int)(bw * 1.5),
 * end_bonus -1, zdrop and KSW_EZ_EXTZ_ONLY, then mm_update_extra with mm_fix_cigar.
 *   made[n_regions]                  out: 0 split_inv unset or an early return; 1 made; 2 tested, score < min_dp_max; 3 a candidate that
 *                                    the loop never tests because the pair before it was made; 4 the extension gave no CIGAR
 *   r_inv[n_regions]                 out: every word as the reference leaves it (id -1, parent MM_PARENT_UNSET, inv, rev = !r1->rev,
 *                                    div -1); all zero where made != 1
 *   extra[n_regions], cigar_off[n_regions + 1], cigar, cigar_cap    as chaindp_align1's, over the slots
 * The targets are the ones chaindp_align_set_targets left resident.
 * Where the reference would index outside the strand or trip one of mm_update_extra's asserts the result is unspecified; the call
 * still returns without faulting.
 * CHAINDP_ERR_ARG (nothing launched, context usable): flag & (MM_F_SR | MM_F_SPLICE); q == q2 && e == e2; a scoring value outside
 * 0..127; max_gap above 20000; no targets set; NULL arrays; a pair that passes the early returns whose rid is no target or whose
 * target stretch [r1->re, r2->rs) lies outside its sequence. */
int chaindp_align1_inv(chaindp_ctx_t *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                       const int64_t *regs_off, const chaindp_reg_t *regs, int32_t *made, chaindp_reg_t *r_inv,
                       chaindp_align_extra_t *extra, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap);

/* ---- test and tuning hooks -- NOT part of the stable ABI, in the sense of chaindp_debug.h */
/* No GPU needed: what chaindp_align1_inv makes of its arguments.  Returns CHAINDP_OK or CHAINDP_ERR_ARG; out[0] = slots (regions),
 * out[1] = pairs that pass the early returns (the candidates, in slot order). */
int chaindp_align_inv_debug_check(const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const int64_t *regs_off,
                                  const chaindp_reg_t *regs, int64_t n_t, const int64_t *t_off, int64_t out[2]);
/* score, qe, te of ksw_ll_i16 for each of the n candidates of the last chaindp_align1_inv, as the device computed them on the reversed
 * stretches, before they are turned back into q_off and t_off.  CHAINDP_ERR_ARG unless n is that call's candidate count. */
int chaindp_align_inv_debug_ll(chaindp_ctx_t *ctx, int64_t n, int32_t *out3);
/* Device milliseconds of the last chaindp_align1_inv made while profiling was on: local score, gather with the DP, finish with the
 * skip rule, pack; -1 each before. */
int chaindp_align_inv_debug_ms(chaindp_ctx_t *ctx, double ms[4]);

#ifdef __cplusplus
}
#endif
#endif
