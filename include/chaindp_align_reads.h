/*
 * chaindp_align_reads.h -- whole reads in one call (mm_align_skeleton) of the C ABI in chaindp.h (libchaindp_hip.so).
 * chaindp.h includes this header behind chaindp_align_inv.h, whose stages it runs; including chaindp.h gives all of them.
 */
#ifndef CHAINDP_ALIGN_READS_H
#define CHAINDP_ALIGN_READS_H

#include "chaindp_align_inv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the loop around mm_align1 and mm_align1_inv (align.c:705-761) for a batch of reads -----------------------------------------------
 * What mm_align_skeleton leaves behind, as the reference runs it with MM_F_SR and MM_F_SPLICE unset and q != q2 || e != e2: every
 * region aligned (chaindp_align1), what a Z-drop split off aligned in turn and put behind its region, round after round until nothing
 * is split off; the inversions between split regions (chaindp_align1_inv) put behind their right regions; mm_filter_regs (with
 * max_clip_ratio 1.0, as mm_mapopt_init sets it); mm_hit_sort_by_dp.  The reads' bases, the anchors and the CIGAR words stay on the
 * device between the rounds; between them only region-sized records cross the bus.
 *   seq_off, seq, a_off, a, regs_off, regs     as chaindp_align1 takes them (anchors AFTER mm_squeeze_a, as relative to the read); a
 *                                    comes back with its MM_SEED_IGNORE marks, regs is only read
 *   out_off[n_reads + 1]             out: read i's final regions are out_regs[out_off[i] .. out_off[i + 1])
 *   out_regs, out_extra              out: room for regs_cap regions: every word of each surviving region, in mm_hit_sort_by_dp's
 *                                    order, and what r->p holds beside the CIGAR
 *   cigar_off[regs_cap + 1], cigar   out: the CIGAR words (len << 4 | op), CSR over the final regions; room for cigar_cap words
 *   need[2]                          out, always: the final regions and the CIGAR words of the batch
 * CHAINDP_ERR_CAPACITY if regs_cap < need[0] or cigar_cap < need[1]: out_off, need and a are exact, the other outputs untouched, and
 * chaindp_align_reads_fetch delivers the same result into larger arrays without computing anything again.  The result stays resident
 * until the next chaindp_align_reads on the context.  out_regs, out_extra, cigar_off may be NULL with regs_cap 0, cigar with cigar_cap 0.
 * The targets are the ones chaindp_align_set_targets left resident.  n_reads == 0 is a valid empty call.
 * Where either stage's result is unspecified, or a region would reach the sort with r->p == NULL (the reference's assert), the result
 * is unspecified; the call still returns without faulting.  Two regions of a read with equal dp_max << 32 | hash keep the order the
 * loop placed them in (the reference's order there is an accident of its radix sort).
 * CHAINDP_ERR_ARG (nothing launched, context usable): everything chaindp_align1 or chaindp_align1_inv refuses about these arguments;
 * a negative capacity; NULL out_off or need.  A refusal of a later round (chaindp_last_error names the round) means an earlier round's
 * result was unspecified. */
int chaindp_align_reads(chaindp_ctx_t *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                        const int64_t *a_off, chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs,
                        int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int64_t regs_cap,
                        int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2]);
/* The resident result of the last chaindp_align_reads once more.  CHAINDP_ERR_ARG when none is resident or n_reads is not that
 * call's; CHAINDP_ERR_CAPACITY as above. */
int chaindp_align_reads_fetch(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra,
                              int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2]);

/* ---- test and tuning hooks -- NOT part of the stable ABI, in the sense of chaindp_debug.h */
/* No GPU needed: what chaindp_align_reads makes of its arguments before anything touches the device.  Returns CHAINDP_OK or
 * CHAINDP_ERR_ARG; out[0] = regions of round 0, out[1] = reads. */
int chaindp_align_reads_debug_check(const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const int64_t *a_off,
                                    const chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, int64_t n_t, const int64_t *t_off,
                                    int64_t regs_cap, int64_t cigar_cap, int64_t out[2]);
/* Each read's list of the last chaindp_align_reads as it stood ahead of mm_filter_regs, split-off regions and inversions in their
 * places (the sort hides the places): placed_off[n_reads + 1] always, the records where placed_cap holds them (else
 * CHAINDP_ERR_CAPACITY with placed_off filled). */
int chaindp_align_reads_debug_placed(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *placed_off, chaindp_reg_t *placed, int64_t placed_cap);
/* The rounds of chaindp_align1 the last chaindp_align_reads made: out[0] = their number, out[1 + k] = regions of round k for the first
 * cap - 1 of them. */
int chaindp_align_reads_debug_rounds(chaindp_ctx_t *ctx, int64_t *out, int64_t cap);
/* Device milliseconds of the last chaindp_align_reads made while profiling was on: the rounds (all of chaindp_align1's stages), the
 * inversion call, the finish (placed order, filter, sort, scans), the gather; -1 each before. */
int chaindp_align_reads_debug_ms(chaindp_ctx_t *ctx, double ms[4]);
/* Lists of up to cap records (1 .. the built-in cap, which 0 restores) are ranked in LDS, longer ones in global memory.  Launches nothing;
 * out_cap (or NULL) receives the built-in cap. */
int chaindp_align_reads_debug_set_lds_cap(chaindp_ctx_t *ctx, int cap, int32_t *out_cap);

#ifdef __cplusplus
}
#endif
#endif
