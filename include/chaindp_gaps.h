/*
 * chaindp_gaps.h -- per-read chaining gaps of the C ABI in chaindp.h (libchaindp_hip.so).  chaindp.h includes this header; including
 * either one gives both.
 */
#ifndef CHAINDP_GAPS_H
#define CHAINDP_GAPS_H

#include "chaindp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-read chaining gaps: reads of mixed lengths in one call ---------------------------------------------------------------
 * The reference derives both gaps per read from the read's total length (map.c:358-366).  chaindp_read_gaps computes exactly that for
 * every read, in the reference's int arithmetic, on the host (no GPU needed): gap_qry = is_sr ? max(qlen_sum, max_gap) : max_gap;
 * gap_ref = max_gap_ref if > 0, else max(max_frag_len - qlen_sum, max_gap) if max_frag_len > 0, else max_gap.
 * chaindp_set_read_gaps puts one (gap_ref, gap_qry) pair per read in force on ctx (the arrays are copied to the device; synchronous).
 * While they are in force every run of the chain DP on ctx -- chaindp_run, chaindp_run_full, chaindp_chain_batch and the run inside
 * chaindp_map_batch, chaindp_map_reads, chaindp_map_seqs, chaindp_map_frags, chaindp_map_frag_seqs -- chains read r with its own pair in
 * the place of par->max_dist_x / par->max_dist_y (which are ignored; bw, max_skip, min_sc, is_cdna and n_segs stay the batch's), and
 * returns CHAINDP_ERR_ARG if the batch does not have n_reads reads (the one-call functions before anything is launched; the context
 * stays usable).  chaindp_run_device returns CHAINDP_ERR_ARG while gaps are in force; the pipe and the packet shim never set any.
 * A run keeps a copy of the gaps it ran with: chaindp_frag_post behind it takes read r's gap_ref as mm_select_sub_multi's max_gap_ref
 * whatever has been set or cleared since.  chaindp_set_read_gaps(ctx, 0, NULL, NULL) clears them: the next run is par's again.
 * CHAINDP_ERR_ARG for a negative gap, a NULL array with n_reads > 0, or more reads than ctx was created for.  Per read the results
 * equal a run of that read alone with its pair as par's (such a batch goes through k_chain_units only, every unit to its end). */
void chaindp_read_gaps(int32_t max_gap, int32_t max_gap_ref, int32_t max_frag_len, int32_t is_sr, int64_t n_reads,
                       const int32_t *qlen_sum, int32_t *gap_ref, int32_t *gap_qry);
int chaindp_set_read_gaps(chaindp_ctx_t *ctx, int64_t n_reads, const int32_t *gap_ref, const int32_t *gap_qry);

#ifdef __cplusplus
}
#endif
#endif
