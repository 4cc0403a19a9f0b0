/*
 * chaindp_debug.h -- test and tuning hooks of libchaindp_hip.so.
 *
 * NOT part of the stable ABI (that is chaindp.h): these exist for the test suite and the probes under tools/, and may change or
 * disappear with the code they look into.  They are declared here so that the definitions (chaindp_abi*.cpp, through chaindp_ctx.h)
 * are held to one prototype and every caller binds the same one.
 */
#ifndef CHAINDP_DEBUG_H
#define CHAINDP_DEBUG_H

#include <stddef.h>
#include <stdint.h>
#include "chaindp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Units the two-per-wave kernel handed over to k_chain_units in the last run (the batch's unit count when it declined the batch). */
int64_t chaindp_debug_leftover(chaindp_ctx_t *ctx);
/* Units k_chain_units handed over to k_chain_dense in the last run. */
int64_t chaindp_debug_deep_units(chaindp_ctx_t *ctx);
/* Bytes of device memory the context owns at this moment. */
int64_t chaindp_debug_device_bytes(chaindp_ctx_t *ctx);
/* two != 0 keeps k_chain_twin on its layout with a cost table per half even where the batch has one table key; 0 lets the device decide. */
int chaindp_debug_set_twin_tables(chaindp_ctx_t *ctx, int two);
/* Which layout k_chain_twin ran the last batch with: 1 one cost table per wave, 2 one per half, 0 neither. */
int chaindp_debug_twin_tables(chaindp_ctx_t *ctx);
/* What k_chain_twin hands over whatever the units look like: 0 nothing extra, 1 every unit untouched, 2 every unit after its first tile. */
int chaindp_debug_set_twin_handover(chaindp_ctx_t *ctx, int mode);
/* 0 keeps every unit in the launch that took it, 1 (default) hands long deep units over; 2 / 3 / 4 any unit with a few deep scans, to
 * k_chain_dense / k_chain_dense1 / k_chain_dense16. */
int chaindp_debug_set_deep_handover(chaindp_ctx_t *ctx, int on);
/* No GPU needed: k_chain_twin's LDS bytes per workgroup with one cost table per wave (one_table != 0) or one per half. */
int64_t chaindp_debug_twin_lds_bytes(int one_table);
/* No GPU needed: the most workgroups per CU k_chain_twin's launch asks for (samegap: max_dist_y >= max_dist_x). */
int chaindp_debug_twin_max_wg_per_cu(int samegap, int one_table);
/* How the last seed collection was routed: out = max_n, max_n2, lab_cap (the limits the context settled on), items (buckets
 * k_seed_sort_huge handed to the LDS sort), tied (units with equal x). */
int chaindp_debug_seed_route(chaindp_ctx_t *ctx, int64_t out[5]);
/* Copies one of the backtrack scratch arrays (which = 0..9; 7 = what chaindp_gen_regs left resident) to the host. */
int chaindp_debug_bottom(chaindp_ctx_t *ctx, int which, void *dst, size_t bytes);
/* Fragments (and segments) with more than cap hits (0..64) keep their work arrays in global scratch, not LDS. */
int chaindp_debug_set_frag_lds_cap(chaindp_ctx_t *ctx, int cap);
/* The index build behind the sketch, from n minimizers of the caller's (x = hash << 8 | span, y = rid << 32 | pos << 1 | strand). */
chaindp_index_t *chaindp_debug_index_from_minimizers(chaindp_ctx_t *ctx, int b, int64_t n, const chaindp_anchor_t *mini, int64_t n_seqs,
                                                     const uint32_t *rank);
/* Bases per sketch sub-batch of chaindp_index_build (0: as many as a sketch takes). */
int chaindp_debug_index_chunk_bases(chaindp_ctx_t *ctx, int64_t n);
/* What the build of ix did: sub_batches, minimizers, distinct, buckets, expanded, max_keys, passes_run, passes_skipped. */
int chaindp_debug_index_route(const chaindp_index_t *ix, int64_t out[8]);
/* Milliseconds the build of ix spent: ms[0] sketch sub-batches with their uploads (host clock), ms[1] sort, ms[2] grouping, ms[3] tables. */
int chaindp_debug_index_stage_ms(const chaindp_index_t *ix, double ms[4]);

#ifdef __cplusplus
}
#endif
#endif
