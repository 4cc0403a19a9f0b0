/*
 * chaindp_ksw.h -- the dual-gap extension alignment of the C ABI in chaindp.h (libchaindp_hip.so).  chaindp.h includes this header;
 * including either one gives both.
 */
#ifndef CHAINDP_KSW_H
#define CHAINDP_KSW_H

#include "chaindp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the reference's KSW_EZ_* bits this call takes (ksw2.h:8-14); every other bit is refused */
#define CHAINDP_KSW_SCORE_ONLY 0x01   /* no path matrix, no CIGAR */
#define CHAINDP_KSW_RIGHT      0x02   /* right-align gaps */
#define CHAINDP_KSW_APPROX_MAX 0x08   /* no 32-bit H[]: max, mqe, mte stay reset, score follows one cell per diagonal */
#define CHAINDP_KSW_EXTZ_ONLY  0x40   /* extension: the CIGAR ends at the query's end or at the maximum */
#define CHAINDP_KSW_REV_CIGAR  0x80   /* CIGAR in traceback order */
#define CHAINDP_KSW_FLAGS      0xcb

/* ---- ksw_extd2_sse for a batch of problems (ksw2_extd2_sse.c, the path without KSW_EZ_GENERIC_SC) -------------------------------
 * What mm_align_pair (align.c:220-243) calls for every gap between two anchors and every chain end under every preset with q != q2:
 * a banded anti-diagonal DP with two affine gap costs in int8 difference arithmetic, a 32-bit H[] for the exact maximum, Z-drop and
 * a traceback.  Problem i aligns the query bases[q_beg[i] .. + q_len[i]) to the target bases[t_beg[i] .. + t_len[i]); bases holds
 * codes 0..4 (4 is the wildcard) as the reference's callers pass them, reversed already where mm_seq_rev reverses.
 *   a, b, q, e, q2, e2   one scoring set per call, each in 0..127: mat = ksw_gen_simple_mat(5, a, b), the two gap costs in either order;
 *   w, zdrop, end_bonus, flag   per problem, as ksw_extd2_sse takes them (w < 0: no band; zdrop < 0: none).  flag is any combination of
 *                        the CHAINDP_KSW_* bits; one problem with another bit refuses the whole call;
 *   ez_out[n][10]        max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end of every problem's ksw_extz_t;
 *   cigar_off[n + 1], cigar   the CIGAR words (len << 4 | op) of every problem, CSR; room for cigar_cap words: CHAINDP_ERR_CAPACITY,
 *                        with ez_out and cigar_off filled in, if there are more (the sum of q_len + t_len is always enough).
 *                        cigar may be NULL with cigar_cap 0.
 * A problem with q_len == 0 or t_len == 0, and every problem when b > 2 (q + e) of the cheaper gap cost, gives the reset ksw_extz_t
 * (0, 0, -1, -1, KSW_NEG_INF, -1, KSW_NEG_INF, -1, KSW_NEG_INF, 0) and no CIGAR, as the reference's early returns do.  n == 0 is a
 * valid empty call (cigar_off[0] = 0).  Every field and every CIGAR word equals the reference's, including what it makes of the cells
 * outside the band and its order among equal maxima (tests/test_gpu_ksw.py).
 * CHAINDP_ERR_ARG (nothing launched, context usable): a NULL array with n > 0, a negative length or start, a base above 4
 * inside a problem, a scoring value outside 0..127, an unknown flag bit, q_len + t_len of 2^27 or more.  CHAINDP_ERR_CAPACITY also when the
 * device has no room for the batch's path matrices; the context stays usable.  The buffers are the context's own and grow with the
 * batch; a context that never makes this call has none of them. */
int chaindp_ksw_extd(chaindp_ctx_t *ctx, int64_t n, const uint8_t *bases, const int64_t *q_beg, const int32_t *q_len,
                     const int64_t *t_beg, const int32_t *t_len, int a, int b, int q, int e, int q2, int e2, const int32_t *w,
                     const int32_t *zdrop, const int32_t *end_bonus, const int32_t *flag, int32_t *ez_out, int64_t *cigar_off,
                     uint32_t *cigar, int64_t cigar_cap);

/* ---- test and tuning hooks of the alignment -- NOT part of the stable ABI, in the sense of chaindp_debug.h: they look into this call
 * alone and may change or disappear with it.  (They are declared here, under names of this call, because the set of chaindp_debug_*
 * symbols is pinned by tests/test_abi_and_host.py.) */
/* No GPU needed: what chaindp_ksw_extd routes a problem by.  out = the LDS budget in bytes, then the bytes of state per target base, per
 * query base (both lengths rounded up to 16 first) and per problem: a problem whose sum fits the budget keeps its state in LDS; out[4] = the sum above which a
 * problem in LDS gets out[5] waves instead of one. */
int chaindp_ksw_debug_routing(int64_t out[6]);
/* The route every problem of the last chaindp_ksw_extd (n of them) took, as the device reported it: 0 the reference's early return,
 * 1 state in LDS, 2 state in global scratch, 3 state in LDS and several waves. */
int chaindp_ksw_debug_route(chaindp_ctx_t *ctx, int64_t n, int32_t *route);
/* Launches nothing.  cap > 0: every later plan of the DP (chaindp_ksw_extd, chaindp_align1, chaindp_align1_inv) launches at most cap
 * workgroups of either kind, so that a workgroup takes problem after problem; 0 (the default) leaves the plan alone; negative is
 * CHAINDP_ERR_ARG. */
int chaindp_ksw_debug_set_grid_cap(chaindp_ctx_t *ctx, int cap);
/* Launches nothing.  The last plan of the DP on this context: out = the problems of the one-wave and of the several-wave launch, their
 * workgroups, the LDS bytes of state each workgroup of them asked for, the bytes of each one's slice of path matrix.  All 0 before. */
int chaindp_ksw_debug_launch(chaindp_ctx_t *ctx, int64_t out[8]);
/* Device milliseconds of the DP kernel in the last chaindp_ksw_extd made while profiling was on (chaindp_set_profiling); -1 before. */
double chaindp_ksw_debug_ms(chaindp_ctx_t *ctx);

#ifdef __cplusplus
}
#endif
#endif
