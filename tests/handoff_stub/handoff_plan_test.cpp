// TEST INFRASTRUCTURE ONLY: chaindp_handoff_plan.h on heap arrays of exactly the stated lengths, so that a read or write past one is an
// AddressSanitizer report: every refusal of the call's arguments and of what is resident, the valid calls beside them (no reads, reads
// without regions), the checks of regions that go up and come down against a squeeze written the plain way.
#include "../../minimap2_chaindp_amd/csrc/chaindp_handoff_plan.h"
#include <algorithm>
#include <assert.h>
#include <memory>
#include <random>
#include <stdio.h>

using namespace chaindp;

static int n_ok = 0, n_refused = 0;
#define OK(x) do { std::string e_; int rc_ = (x); if (rc_) { printf("line %d: refused: %s\n", __LINE__, e_.c_str()); return 1; } ++n_ok; } while (0)
#define NO(x) do { std::string e_; int rc_ = (x); if (!rc_ || e_.empty()) { printf("line %d: not refused\n", __LINE__); return 1; } ++n_refused; } while (0)

static ApostOpt opt(int flag) { ApostOpt o = {flag, 0.5f, 0.8f, 5, 30, 8, 20000, 2000, 1000, 3, 40, 2, 0}; return o; }

int main()
{
	// the call's own arguments
	ApostOpt good = opt(HO_F_CIGAR), nocigar = opt(0), sr = opt(HO_F_CIGAR | AP_F_SR), splice = opt(HO_F_CIGAR | AP_F_SPLICE), badsc = opt(HO_F_CIGAR);
	badsc.match_sc = 0;
	OK(handoff_check_call(&good, true, 0, 0, 0, true, false, false, false, false, e_));
	OK(handoff_check_call(&good, true, 7, 3, 9, true, true, true, true, true, e_));
	OK(handoff_check_call(&good, true, 7, 3, 9, true, true, true, true, false, e_));
	NO(handoff_check_call(nullptr, true, 1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, false, 1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, -1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&nocigar, true, 1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&sr, true, 1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&splice, true, 1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&badsc, true, 1, 0, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, 1, 0, 0, false, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, 1, -1, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, 1, 0, -1, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, 1, 1, 0, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, 1, 0, 1, true, false, false, false, false, e_));
	NO(handoff_check_call(&good, true, 1, 0, 0, true, false, false, false, true, e_));

	// what is resident
	std::unique_ptr<int64_t[]> t_off(new int64_t[4]{0, 10, 10, 35});
	std::unique_ptr<int32_t[]> ref_len(new int32_t[3]{10, 0, 25}), other(new int32_t[3]{10, 1, 25});
	HandoffResident h;
	h.post_n_reads = 5; h.post_cigar = h.hits_resident = h.rep_resident = h.from_sketch = h.sketch_valid = true;
	h.sketch_reads = h.sketch_seqs = 5; h.n_t = 3; h.t_off = t_off.get(); h.n_ref = 3; h.ref_len = ref_len.get();
	OK(handoff_check_resident(h, 5, e_));
	{ HandoffResident z = h; z.post_n_reads = z.sketch_reads = z.sketch_seqs = 0; OK(handoff_check_resident(z, 0, e_)); }
	{ HandoffResident z = h; z.n_t = z.n_ref = 0; z.t_off = nullptr; z.ref_len = nullptr; OK(handoff_check_resident(z, 5, e_)); }
	NO(handoff_check_resident(h, 4, e_));
	{ HandoffResident z = h; z.post_n_reads = -1; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.hits_resident = false; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.post_cigar = false; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.from_sketch = false; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.sketch_valid = false; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.sketch_reads = 6; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.sketch_seqs = 10; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.rep_resident = false; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.n_t = -1; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.n_ref = 2; NO(handoff_check_resident(z, 5, e_)); }
	{ HandoffResident z = h; z.ref_len = other.get(); NO(handoff_check_resident(z, 5, e_)); }

	// the reads' offsets
	{
		std::vector<int32_t> len = {0, 5, 0, 7};
		std::vector<int64_t> off;
		handoff_seq_off(len, off);
		assert(off.size() == 5 && off[0] == 0 && off[1] == 0 && off[2] == 5 && off[3] == 5 && off[4] == 12);
		handoff_seq_off(std::vector<int32_t>(), off);
		assert(off.size() == 1 && off[0] == 0);
	}

	// regions up and down: seeded batches, squeezed the plain way
	std::mt19937 rng(20261021);
	for (int round = 0; round < 40; ++round) {
		const int R = (int)(rng() % 6);
		std::vector<int64_t> regs_off(R + 1, 0), b_off(R + 1, 0), a_off(R + 1, 0);
		std::vector<std::vector<std::pair<int, int>>> reads(R);            // (as, cnt) per region
		for (int r = 0; r < R; ++r) {
			const int n = (int)(rng() % 5);
			int at = 0;
			for (int g = 0; g < n; ++g) { at += (int)(rng() % 3); const int c = (int)(rng() % 70); reads[r].push_back({at, c}); at += c; }
			std::shuffle(reads[r].begin(), reads[r].end(), rng);
			regs_off[r + 1] = regs_off[r] + n; b_off[r + 1] = b_off[r] + at + (int)(rng() % 3);
		}
		const int64_t N = R ? regs_off[R] : 0;
		std::unique_ptr<int32_t[]> regs(new int32_t[(size_t)N * HO_REG_WORDS]()), down(new int32_t[(size_t)N * HO_REG_WORDS]());
		for (int r = 0; r < R; ++r) {
			std::vector<int> order(reads[r].size());
			for (size_t g = 0; g < order.size(); ++g) order[g] = (int)g;
			std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return reads[r][x].first < reads[r][y].first; });
			int to = 0;
			for (size_t g = 0; g < reads[r].size(); ++g) {
				int32_t *w = regs.get() + (regs_off[r] + g) * HO_REG_WORDS;
				w[HO_REG_AS] = reads[r][g].first; w[HO_REG_CNT] = reads[r][g].second;
			}
			for (int g : order) {
				int32_t *w = down.get() + (regs_off[r] + g) * HO_REG_WORDS;
				w[HO_REG_AS] = to; w[HO_REG_CNT] = reads[r][g].second;
				to += reads[r][g].second;
			}
			a_off[r + 1] = a_off[r] + to;
		}
		OK(handoff_check_up(R, regs_off.data(), regs.get(), b_off.data(), true, true, true, true, e_));
		OK(handoff_check_down(R, regs_off.data(), down.get(), a_off.data(), e_));
		if (N) {
			// a region past its read's anchors, a negative count, a falling offset
			int r = 0;
			while (regs_off[r + 1] == regs_off[r]) ++r;
			int32_t *w = regs.get() + regs_off[r] * HO_REG_WORDS, *d = down.get() + regs_off[r] * HO_REG_WORDS;
			const int32_t as = w[HO_REG_AS], cnt = w[HO_REG_CNT], das = d[HO_REG_AS];
			w[HO_REG_AS] = (int32_t)(b_off[r + 1] - b_off[r]) - cnt + 1;
			NO(handoff_check_up(R, regs_off.data(), regs.get(), b_off.data(), true, true, true, true, e_));
			w[HO_REG_AS] = as; w[HO_REG_CNT] = -1;
			NO(handoff_check_up(R, regs_off.data(), regs.get(), b_off.data(), true, true, true, true, e_));
			w[HO_REG_CNT] = cnt;
			NO(handoff_check_up(R, regs_off.data(), regs.get(), b_off.data(), true, false, true, true, e_));
			d[HO_REG_AS] = (int32_t)(a_off[r + 1] - a_off[r]) + 1;
			NO(handoff_check_down(R, regs_off.data(), down.get(), a_off.data(), e_));
			d[HO_REG_AS] = das;
			a_off[R] += 1;
			NO(handoff_check_down(R, regs_off.data(), down.get(), a_off.data(), e_));
			a_off[R] -= 1;
			regs_off[0] = 1;
			NO(handoff_check_up(R, regs_off.data(), regs.get(), b_off.data(), true, true, true, true, e_));
			regs_off[0] = 0;
		}
		NO(handoff_check_up(R, regs_off.data(), regs.get(), b_off.data(), true, true, false, true, e_));
	}
	NO(handoff_check_up(-1, nullptr, nullptr, nullptr, false, false, true, false, e_));
	OK(handoff_check_up(0, nullptr, nullptr, nullptr, false, false, true, false, e_));
	printf("handoff plan ok: %d accepted, %d refused\n", n_ok, n_refused);
	return 0;
}
