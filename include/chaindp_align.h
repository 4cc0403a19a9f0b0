/*
 * chaindp_align.h -- base-level alignment of one region at a time (mm_align1) of the C ABI in chaindp.h (libchaindp_hip.so).
 * chaindp.h includes this header; including either one gives both.
 */
#ifndef CHAINDP_ALIGN_H
#define CHAINDP_ALIGN_H

#include "chaindp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the fields of mm_mapopt_t and mm_idx_t that mm_align1 (align.c:423-636) reads */
typedef struct {
	int32_t a, b, q, e, q2, e2;                 /* scoring, each in 0..127; q != q2 or e != e2 */
	int32_t bw, zdrop, zdrop_inv, end_bonus;
	int32_t min_cnt, min_chain_score, min_dp_max, min_ksw_len, max_gap;
	int32_t flag;                               /* MM_F_*; MM_F_SR (0x1000) and MM_F_SPLICE (0x80) are refused */
	int32_t k, is_hpc;                          /* of the index: mi->k, mi->flag & MM_I_HPC */
} chaindp_align_opt_t;

/* what mm_align1 leaves in r->p beside the CIGAR; all 0 where r->p stays NULL */
typedef struct { int32_t has_extra, dp_score, dp_max, n_ambi, n_cigar; } chaindp_align_extra_t;

/* ---- the target sequences ----------------------------------------------------------------------------------------------------------
 * n_seqs sequences as characters, sequence i = seq[seq_off[i] .. seq_off[i + 1]) (the shape chaindp_index_build takes them in).  They
 * are encoded on the device with the reference's seq_nt4_table -- the codes 0..4 mm_idx_getseq returns -- and stay resident on the
 * context until the next chaindp_align_set_targets or chaindp_align_clear_targets.  The buffers are the context's own and grow with
 * the call; a context that never aligns has none.  CHAINDP_ERR_ARG: NULL arrays with n_seqs > 0, offsets that do not start at 0 or
 * fall, a sequence of 2^31 - 1 bases or more. */
int chaindp_align_set_targets(chaindp_ctx_t *ctx, int64_t n_seqs, const int64_t *seq_off, const char *seq);
int chaindp_align_clear_targets(chaindp_ctx_t *ctx);

/* ---- mm_align1 for every region of a batch of reads --------------------------------------------------------------------------------
 * As the reference runs it with MM_F_SR and MM_F_SPLICE unset and q != q2 || e != e2 (map-ont, map-pb with HPC, ava-*, asm5/10/20):
 * the choice of anchors (mm_fix_bad_ends, mm_filter_bad_seeds, mm_adjust_minier), the bounds of the extensions, the left extension,
 * the gap fills with mm_test_zdrop and its inversion test and the second pass, the split at a Z-drop (mm_split_reg), the right
 * extension, mm_append_cigar and mm_update_extra with mm_fix_cigar.  Every extension and fill is a problem of chaindp_ksw_extd's
 * kernel; the bookkeeping around them runs on the device too.
 *   seq_off[n_reads + 1], seq        the reads' bases as characters (forward strand)
 *   a_off[n_reads + 1], a            in/out: each read's anchors AFTER mm_squeeze_a, packed as the reference packs them; mm_filter_bad_seeds
 *                                    writes MM_SEED_IGNORE into a[].y
 *   regs_off[n_reads + 1], regs      in/out: each read's regions; the fields mm_align1 reads are read (as, cnt, mlen, qs, qe, rs, re, id,
 *                                    parent, score, the bit-field word with rev and split_inv), rs / re / qs / qe / mlen / blen, and at a
 *                                    split cnt / score / split, are written.  The anchor ranges of one read's regions must not overlap
 *                                    (mm_gen_regs never makes them overlap); as is relative to the read's first anchor.
 *   regs2[n_regions]                 out: cnt = 0 where nothing was split off (the other fields are left as they were), else every
 *                                    field as mm_split_reg leaves it (id -1, parent MM_PARENT_TMP_PRI where r was primary, split_inv)
 *   extra[n_regions]                 out
 *   cigar_off[n_regions + 1], cigar  out: the CIGAR words (len << 4 | op) of every region, CSR; room for cigar_cap words:
 *                                    CHAINDP_ERR_CAPACITY, with everything else filled in, if there are more.  cigar may be NULL with
 *                                    cigar_cap 0.
 * A region with cnt == 0 leaves regs2.cnt = 0, extra all 0 and nothing else touched; n_reads == 0 is a valid empty call.
 * Where the reference would dereference a NULL r->p (a Z-drop before any CIGAR word exists) or trip one of its asserts (qs0 < 0,
 * re0 <= rs0, qe1 > qlen, the coordinate checks of mm_fix_cigar / mm_update_extra) the result is unspecified; the call still returns
 * without faulting.
 * CHAINDP_ERR_ARG (nothing launched, context usable): flag & (MM_F_SR | MM_F_SPLICE); q == q2 && e == e2; a scoring value outside
 * 0..127; a region whose anchors do not all carry its first anchor's rid and strand, or that reaches outside the read's anchors; an
 * anchor with a rid that is no target or a position outside its sequence; no targets set; max_gap above 20000 (the state of the
 * inversion test is kept in LDS); NULL arrays.  CHAINDP_ERR_CAPACITY also when the device has no room for the path matrices. */
int chaindp_align1(chaindp_ctx_t *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                   const int64_t *a_off, chaindp_anchor_t *a, const int64_t *regs_off, chaindp_reg_t *regs, chaindp_reg_t *regs2,
                   chaindp_align_extra_t *extra, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap);

/* ---- test and tuning hooks -- NOT part of the stable ABI, in the sense of chaindp_debug.h */
/* No GPU needed: what chaindp_align1 makes of its arguments before anything touches the device.  t_off[n_t + 1]: the targets' offsets as
 * chaindp_align_set_targets takes them.  Returns CHAINDP_OK or CHAINDP_ERR_ARG; out[0] = regions, out[1] = problem slots (cnt + 1 per region). */
int chaindp_align_debug_check(const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const int64_t *a_off,
                              const chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, int64_t n_t, const int64_t *t_off,
                              int64_t out[2]);
/* Device milliseconds of the last chaindp_align1 made while profiling was on: plan (with the gathers), DP (both passes), zdrop, stitch,
 * extra (with the pack); -1 each before. */
int chaindp_align_debug_ms(chaindp_ctx_t *ctx, double ms[5]);

#ifdef __cplusplus
}
#endif
#endif
