// chaindp_handoff_plan.h -- what the host decides about a chaindp_align_resident call (include/chaindp_map_align.h): the checks of the
// call's own arguments and of what has to be resident in the context, and the reads' offsets from the lengths the sketch saw.
// No HIP in here, as chaindp_apost_plan.h: a stand-alone program runs it under the sanitizers.
#ifndef CHAINDP_HANDOFF_PLAN_H
#define CHAINDP_HANDOFF_PLAN_H
#include <limits.h>
#include "chaindp_apost_plan.h"

namespace chaindp {

#define HO_LDS_CAP 256                // regions of a read k_handoff_move ranks in LDS (12 bytes each: 3 KB, so that LDS leaves room for eight
                                      // one-wave workgroups per SIMD); longer lists take the global route
#define HO_F_CIGAR 0x004
#define HO_REG_WORDS 20
#define HO_REG_CNT 1                  // words of a region the hand-off reads and rewrites
#define HO_REG_AS 10

// The call's own arguments.  0, or -1 with err.
inline int handoff_check_call(const ApostOpt *popt, bool has_aopt, int64_t n_reads, int64_t regs_cap, int64_t cigar_cap, bool has_out_off_need, bool has_reg_arrays,
                              bool has_cigar, bool has_a_off, bool has_a, std::string &err)
{
	if (!has_aopt) { err = "NULL aopt"; return -1; }
	if (n_reads < 0) { err = "negative n_reads"; return -1; }
	if (apost_check_call(popt, 0, nullptr, regs_cap, cigar_cap, has_out_off_need, has_reg_arrays, has_cigar, err)) return -1;
	if (!(popt->flag & HO_F_CIGAR)) { err = "opt->flag lacks MM_F_CIGAR: chain_post of such a run ends with mm_set_mapq, there is nothing to align"; return -1; }
	if (has_a && !has_a_off) { err = "a without a_off"; return -1; }
	return 0;
}

// What the context holds when the call arrives.
struct HandoffResident {
	int64_t post_n_reads = -1;        // reads of the batch chaindp_chain_post finished on this context (-1: none, or overwritten since)
	bool post_cigar = false;          // ... with MM_F_CIGAR, so that it stopped after mm_est_err
	bool hits_resident = false;       // no chaindp_est_err upload has replaced the hits since
	bool rep_resident = false;        // rep_len of the batch's seed collection
	bool from_sketch = false;         // the batch's minimizers were the resident sketch's
	bool sketch_valid = false;        // ... and no later sketch or upload has replaced its bases
	int64_t sketch_reads = -1, sketch_seqs = -1;
	int64_t n_t = -1;                 // targets of chaindp_align_set_targets (-1: none set)
	const int64_t *t_off = nullptr;
	int64_t n_ref = 0;                // what chain_post was given
	const int32_t *ref_len = nullptr;
};

// 0, or -1 with err: the batch, its bases and the targets are the ones the call needs.
inline int handoff_check_resident(const HandoffResident &h, int64_t n_reads, std::string &err)
{
	if (h.post_n_reads < 0 || !h.hits_resident) { err = "no batch of a chaindp_chain_post is resident (a new batch, a chaindp_est_err or another post step has replaced it)"; return -1; }
	if (!h.post_cigar) { err = "the resident batch's chain_post ran without MM_F_CIGAR"; return -1; }
	if (n_reads != h.post_n_reads) { err = "n_reads is not the resident batch's"; return -1; }
	if (!h.from_sketch || !h.sketch_valid || h.sketch_reads != n_reads || h.sketch_seqs != n_reads) { err = "the bases of the batch's chaindp_sketch are not resident"; return -1; }
	if (!h.rep_resident) { err = "no resident rep_len"; return -1; }
	if (h.n_t < 0) { err = "no targets: chaindp_align_set_targets first"; return -1; }
	if (h.n_t != h.n_ref) { err = "the targets are not the n_ref sequences chain_post was given"; return -1; }
	for (int64_t t = 0; t < h.n_t; ++t)
		if (h.t_off[t + 1] - h.t_off[t] != (int64_t)h.ref_len[t]) { err = "target " + std::to_string((long long)t) + " does not have the ref_len chain_post was given"; return -1; }
	return 0;
}

// Regions and anchors a test hands to the hand-off from the host (chaindp_map_align_debug_run_handoff): offsets that ascend from 0, every
// region inside its read's anchors, so that the kernel reads and writes nothing outside them.  0, or -1 with err.
inline int handoff_check_up(int64_t n_reads, const int64_t *regs_off, const int32_t *regs, const int64_t *b_off, bool has_b, bool has_out_regs, bool has_a_off,
                            bool has_a, std::string &err)
{
	if (n_reads < 0 || !has_a_off) { err = "negative n_reads or NULL a_off"; return -1; }
	if (n_reads == 0) return 0;
	if (!regs_off || !b_off || regs_off[0] != 0 || b_off[0] != 0) { err = "offsets missing or not starting at 0"; return -1; }
	for (int64_t r = 0; r < n_reads; ++r) {
		if (regs_off[r + 1] < regs_off[r] || b_off[r + 1] < b_off[r]) { err = "offsets fall at read " + std::to_string((long long)r); return -1; }
		if (regs_off[r + 1] - regs_off[r] > INT32_MAX / HO_REG_WORDS || b_off[r + 1] - b_off[r] > INT32_MAX) { err = "too many regions or anchors in read " + std::to_string((long long)r); return -1; }
	}
	if ((regs_off[n_reads] > 0 && (!regs || !has_out_regs)) || (b_off[n_reads] > 0 && (!has_b || !has_a))) { err = "regions or anchors announced but absent"; return -1; }
	for (int64_t r = 0; r < n_reads; ++r) {
		const int64_t n_b = b_off[r + 1] - b_off[r];
		int64_t sum = 0;
		for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g) {
			const int64_t cnt = regs[g * HO_REG_WORDS + HO_REG_CNT], as = regs[g * HO_REG_WORDS + HO_REG_AS];
			if (cnt < 0 || as < 0 || as + cnt > n_b) { err = "region " + std::to_string((long long)g) + " outside its read's anchors"; return -1; }
			sum += cnt;
		}
		if (sum > n_b) { err = "the regions of read " + std::to_string((long long)r) + " hold more anchors than the read"; return -1; }
	}
	return 0;
}

// seq_off[n + 1] of the reads from the lengths the sketch saw
inline void handoff_seq_off(const std::vector<int32_t> &len, std::vector<int64_t> &seq_off)
{
	seq_off.assign(len.size() + 1, 0);
	for (size_t q = 0; q < len.size(); ++q) seq_off[q + 1] = seq_off[q] + len[q];
}

// The regions and anchors as they came down, as the kernels must have left them: offsets that ascend from 0 and agree, every region
// inside its read's squeezed anchors.  0, or -1 with err (a device fault, not a caller's).
inline int handoff_check_down(int64_t n_reads, const int64_t *regs_off, const int32_t *regs, const int64_t *a_off, std::string &err)
{
	if (n_reads == 0) return 0;
	if (regs_off[0] != 0 || a_off[0] != 0) { err = "offsets do not start at 0"; return -1; }
	for (int64_t r = 0; r < n_reads; ++r) {
		if (regs_off[r + 1] < regs_off[r] || a_off[r + 1] < a_off[r]) { err = "offsets fall at read " + std::to_string((long long)r); return -1; }
		int64_t sum = 0;
		const int64_t n_a = a_off[r + 1] - a_off[r];
		for (int64_t g = regs_off[r]; g < regs_off[r + 1]; ++g) {
			const int64_t cnt = regs[g * HO_REG_WORDS + HO_REG_CNT], as = regs[g * HO_REG_WORDS + HO_REG_AS];
			if (cnt < 0 || as < 0 || as + cnt > n_a) { err = "region " + std::to_string((long long)g) + " outside its read's anchors"; return -1; }
			sum += cnt;
		}
		if (sum != n_a) { err = "the anchors of read " + std::to_string((long long)r) + " are not the sum of its regions'"; return -1; }
	}
	return 0;
}

} // namespace chaindp
#endif
