/*
 * chaindp_map_align.h -- reads mapped with base alignment in one call (bases in, CIGAR hits out) of the C ABI in chaindp.h
 * (libchaindp_hip.so).  chaindp.h includes this header behind chaindp_align_post.h, whose stages it joins to the mapping calls;
 * including chaindp.h gives all of them.
 */
#ifndef CHAINDP_MAP_ALIGN_H
#define CHAINDP_MAP_ALIGN_H

#include "chaindp_align_post.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- what the reference does with a read between chain_post and its output when MM_F_CIGAR is set (map.c:870-877, n_segs == 1) -----
 * With CHAINDP_F_CIGAR chaindp_chain_post stops after mm_est_err.  chaindp_align_resident takes it from there, on the device: the
 * hand-off (mm_squeeze_a as mm_align_skeleton runs it first, align.c:721: each read's anchors packed in (as, slot) order of its final
 * regions, every region's `as` rewritten), then the stages of chaindp_align_reads_post (mm_align_skeleton's loop, the tail of
 * align_regs, mm_set_mapq).
 *   Works on the batch for which chaindp_chain_post (or chaindp_map_reads / chaindp_map_seqs) last ran on this context with
 *   CHAINDP_F_CIGAR, on the bases of that batch's chaindp_sketch, the rep_len of its seed collection, and the targets of
 *   chaindp_align_set_targets.  chain_post's own result stays as it was: the call can be repeated.
 *   What moves between host and device: the squeezed anchors (16 B per chain anchor), their offsets and the regions (80 B each) come
 *   down ONCE, because the alignment stages plan their rounds on the host; neither the bases nor the anchors go up again.  Then the
 *   stages' own per-round records, as in chaindp_align_reads, and the result.
 *   aopt as in chaindp_align_reads, popt as in chaindp_align_post (the same record chain_post was given; its flag must carry
 *   CHAINDP_F_CIGAR).  out_off, out_regs, out_extra, out_dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need as in chaindp_align_post:
 *   CHAINDP_ERR_CAPACITY when a capacity is short, with out_off and need exact, and chaindp_align_post_fetch delivers the resident result.
 *   a_off[n_reads + 1] / a (both optional; a needs as many entries as chain_post's a): what the reference leaves in a[] -- the squeezed
 *   anchors with the MM_SEED_IGNORE marks of the alignment; `as` of a region before alignment pointed into them.
 * CHAINDP_ERR_ARG, with nothing launched and the context usable: no such batch or no such bases resident (a new batch, a sketch, a
 * chaindp_est_err upload, chaindp_frag_post or a new chaindp_backtrack / chaindp_gen_regs replaced them; the batch's minimizers were
 * not the sketch's); n_reads not theirs; chain_post ran without CHAINDP_F_CIGAR or popt->flag lacks it; no targets set, or targets
 * whose number or lengths are not the n_ref / ref_len chain_post was given; no resident rep_len; whatever chaindp_align_reads and
 * chaindp_align_post refuse.  (A batch with a read of n_segs > 1 never gets here: chaindp_chain_post refuses it.) */
int chaindp_align_resident(chaindp_ctx_t *ctx, const chaindp_align_opt_t *aopt, const chaindp_post_opt_t *popt, int64_t n_reads, int64_t *out_off,
                           chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar,
                           int64_t cigar_cap, int64_t need[2], int64_t *a_off, chaindp_anchor_t *a);

/* chaindp_map_seqs with CHAINDP_F_CIGAR followed by chaindp_align_resident in one call: bases in, the reference's final hits of a -c
 * run with their CIGARs out.  The arguments of chaindp_map_seqs (popt is its opt; the hits before alignment are not returned, so its
 * regs_off / regs / regs_cap are the final outputs' here) plus aopt and the outputs of chaindp_align_resident.  The targets must have
 * been set (chaindp_align_set_targets).  Bit-identical to the separate calls; n_reads == 0 and a batch in which no read has a region
 * are valid.  rep_len (may be NULL) and n_anchors (may be NULL) are by-products. */
int chaindp_map_align_seqs(chaindp_ctx_t *ctx, const chaindp_index_t *idx, int w, int k, int is_hpc, int flag, int max_occ, const chaindp_params_t *par,
                           int min_cnt, const chaindp_post_opt_t *popt, const chaindp_align_opt_t *aopt, int64_t n_reads, const int64_t *seq_off, const char *seq,
                           const uint32_t *bid, const uint32_t *hash, const int32_t *ref_len, int32_t n_ref, int64_t *out_off, chaindp_reg_t *out_regs,
                           chaindp_align_extra_t *out_extra, int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap,
                           int64_t need[2], int64_t *a_off, chaindp_anchor_t *a, int32_t *rep_len, int64_t *n_anchors);

/* The squeezed anchors of the last of the two calls above, with the marks of its alignment, from where they are resident: for a caller
 * who did not know their number when it made the call.  a_off[n_reads + 1]; a has room for a_cap anchors.  CHAINDP_ERR_CAPACITY with
 * a_off filled in when a_cap is short; CHAINDP_ERR_ARG when no such result is resident (a later chaindp_align_reads* call on the context
 * replaces it) or n_reads is not its. */
int chaindp_align_resident_anchors(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *a_off, chaindp_anchor_t *a, int64_t a_cap);

/* ---- test and tuning hooks -- NOT part of the stable ABI, in the sense of chaindp_debug.h */
/* Lists of up to cap regions (1 .. the built-in cap, which 0 restores) are ranked in LDS by the hand-off, longer ones in global memory.
 * Launches nothing; out_cap (or NULL) receives the built-in cap. */
int chaindp_map_align_debug_set_lds_cap(chaindp_ctx_t *ctx, int cap, int32_t *out_cap);
/* Device milliseconds of the last chaindp_align_resident made while profiling was on: ms[0] the hand-off's kernels with their scan,
 * ms[1..4] chaindp_align_reads_debug_ms's, ms[5..6] chaindp_align_post_debug_ms's; -1 each before. */
int chaindp_map_align_debug_ms(chaindp_ctx_t *ctx, double ms[7]);
/* The regions as the hand-off of the last chaindp_align_resident left them, before any alignment (the host's copy, nothing is launched):
 * regs_off[n_reads + 1], regs (room for regs_cap; `as` points into the squeezed anchors), a_off[n_reads + 1].  CHAINDP_ERR_CAPACITY with
 * the offsets filled in where regs_cap is short; CHAINDP_ERR_ARG when there was no such call or n_reads is not its. */
int chaindp_map_align_debug_handoff(chaindp_ctx_t *ctx, int64_t n_reads, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *a_off);

/* The hand-off alone on regions and anchors from the host, for tests that need lists and counts no mapped read of a test's size has:
 * regs_off[n_reads + 1], regs, b_off[n_reads + 1], b in the form chaindp_chain_post returns them (regs_off, regs, a_off, a); out_regs
 * (as many as regs) receives the regions with their new `as`, a_off[n_reads + 1] and a (room for b_off[n_reads]) the squeezed anchors.
 * CHAINDP_ERR_ARG for offsets that do not ascend from 0 and for a region outside its read's anchors (nothing is launched). */
int chaindp_map_align_debug_run_handoff(chaindp_ctx_t *ctx, int64_t n_reads, const int64_t *regs_off, const chaindp_reg_t *regs, const int64_t *b_off,
                                        const chaindp_anchor_t *b, chaindp_reg_t *out_regs, int64_t *a_off, chaindp_anchor_t *a);

#ifdef __cplusplus
}
#endif
#endif
