// The host side of chaindp_align_post on its own (csrc/chaindp_apost_plan.h): every refusal, the empty calls, seeded batches whose
// counts are checked, the layout of the staged batch (pieces on 16 bytes, none overlapping, all inside their buffers) and the logf
// list over a short range.  The arrays are heap blocks of exactly the stated lengths, so that a read past an end is a sanitizer report.
#include <assert.h>
#include <stdio.h>
#include <memory>
#include <random>
#include "../../minimap2_chaindp_amd/csrc/chaindp_apost_plan.h"

using namespace chaindp;

template <typename T> static std::unique_ptr<T[]> exact(const std::vector<T> &v)
{
	std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
	for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
	return p;
}

struct Batch {
	ApostOpt o{0, 0.5f, 0.8f, 5, 30, 8, 20000, 2000, 1000, 3, 40, 2, 0};
	std::vector<int32_t> rep_len;
	std::vector<int64_t> regs_off{0}, cigar_off{0};
	std::vector<int32_t> regs, extra;
	std::vector<uint32_t> cigar;
	int64_t regs_cap = 0, cigar_cap = 0;
	void read(int rl) { rep_len.push_back(rl); regs_off.push_back(regs_off.back()); }
	void region(int has_extra, int n_cigar)
	{
		regs.insert(regs.end(), AP_REG_WORDS, 0);
		const int32_t x[AP_EXTRA_WORDS] = {has_extra, 10, 12, 0, n_cigar};
		extra.insert(extra.end(), x, x + AP_EXTRA_WORDS);
		for (int i = 0; i < n_cigar; ++i) cigar.push_back((uint32_t)(i + 1) << 4);
		cigar_off.push_back(cigar_off.back() + n_cigar);
		++regs_off.back();
	}
	int call(std::string &err, bool out = true, bool arrays = true, bool cig = true, bool null_rep = false) const
	{
		auto rl = exact(rep_len);
		return apost_check_call(&o, (int64_t)rep_len.size(), null_rep ? nullptr : rl.get(), regs_cap, cigar_cap, out, arrays, cig, err);
	}
	int regions(std::string &err, int64_t &N, int64_t &W, int null_which = -1) const
	{
		auto ro = exact(regs_off), co = exact(cigar_off);
		auto rv = exact(regs), xv = exact(extra);
		auto cv = exact(cigar);
		return apost_check_regs((int64_t)rep_len.size(), null_which == 0 ? nullptr : ro.get(), null_which == 1 || regs.empty() ? nullptr : rv.get(),
		                        null_which == 2 || extra.empty() ? nullptr : xv.get(), null_which == 3 ? nullptr : co.get(),
		                        null_which == 4 || cigar.empty() ? nullptr : cv.get(), N, W, err);
	}
};

static int n_ok = 0, n_refused = 0;

static void accept(const Batch &b, int64_t N_want, int64_t W_want)
{
	std::string err;
	int64_t N = -1, W = -1;
	assert(b.call(err) == 0 && b.regions(err, N, W) == 0 && N == N_want && W == W_want);
	++n_ok;
}

static void refuse_call(const Batch &b, bool out = true, bool arrays = true, bool cig = true, bool null_rep = false)
{
	std::string err;
	assert(b.call(err, out, arrays, cig, null_rep) == -1 && !err.empty());
	++n_refused;
}

static void refuse_regs(const Batch &b, int null_which = -1)
{
	std::string err;
	int64_t N, W;
	assert(b.regions(err, N, W, null_which) == -1 && !err.empty());
	++n_refused;
}

static void layout(size_t R, size_t N, size_t W, bool from_host)
{
	const ApostLayout L(R, N, W, from_host);
	struct Piece { size_t at, bytes, buf; };
	std::vector<Piece> ps = {{L.in_rep, R * 4, 0}, {L.w_cnt, (R + 1) * 8, 1}, {L.w_words, (R + 1) * 8, 1}, {L.w_tile, (R / 1024 + 2) * 8, 1}, {L.w_st_regs, N * 80, 1},
	                         {L.w_st_dp2, N * 4, 1}, {L.w_st_src, N * 4, 1}, {L.w_st_wpre, N * 4, 1}, {L.w_fsrc, N * 8, 1}, {L.w_scratch, N * AP_NF * 4, 1}, {L.w_err, 4, 1},
	                         {L.o_need, 16, 2}, {L.o_regs, N * 80, 2}, {L.o_extra, N * 20, 2}, {L.o_dp2, N * 4, 2}, {L.o_cigar_off, (N + 1) * 8, 2}};
	if (from_host) {
		const Piece in[] = {{L.in_regs_off, (R + 1) * 8, 0}, {L.in_regs, N * 80, 0}, {L.in_extra, N * 20, 0}, {L.in_cigar_off, (N + 1) * 8, 0}, {L.in_cigar, W * 4, 0}};
		ps.insert(ps.end(), in, in + 5);
	}
	const size_t size[3] = {L.in_bytes, L.work_bytes, L.out_bytes};
	for (size_t i = 0; i < ps.size(); ++i) {
		assert(ps[i].at % 16 == 0 && ps[i].at + ps[i].bytes <= size[ps[i].buf]);
		for (size_t j = 0; j < i; ++j)
			assert(ps[i].buf != ps[j].buf || ps[i].at + ps[i].bytes <= ps[j].at || ps[j].at + ps[j].bytes <= ps[i].at || !ps[i].bytes || !ps[j].bytes);
	}
	assert(L.out_cig_bytes >= W * 4);
}

int main()
{
	{   // the empty call, reads without regions, one region
		Batch b;
		accept(b, 0, 0);
		b.read(0); b.read(5);
		accept(b, 0, 0);
		b.region(1, 3);
		accept(b, 1, 3);
		b.read(0); b.region(0, 0); b.region(1, 0); b.region(1, 2);
		accept(b, 4, 5);
		b.regs_cap = 4; b.cigar_cap = 5;
		accept(b, 4, 5);
	}
	std::mt19937 rng(20240607);
	for (int it = 0; it < 20; ++it) {   // seeded batches
		Batch b;
		int64_t N = 0, W = 0;
		const int R = 1 + (int)(rng() % 7);
		for (int r = 0; r < R; ++r) {
			b.read((int)(rng() % 300));
			for (int g = (int)(rng() % 5); g > 0; --g) { const int p = (int)(rng() % 4 != 0), c = p ? (int)(rng() % 6) : 0; b.region(p, c); ++N; W += c; }
		}
		accept(b, N, W);
		layout((size_t)R, (size_t)N, (size_t)W, it % 2 == 0);
	}
	layout(0, 0, 0, true); layout(1, 0, 0, false); layout(3000, 12345, 777777, true);
	{   // the refusals
		Batch b;
		b.read(3); b.region(1, 2); b.region(1, 1); b.read(0); b.region(0, 0);
		accept(b, 3, 3);
		{ Batch c = b; c.o.flag = AP_F_SR; refuse_call(c); c.o.flag = AP_F_SPLICE; refuse_call(c); c.o.flag = AP_F_SR; c.o.is_sr = 1; refuse_call(c); }
		{ Batch c = b; c.o.is_sr = 1; std::string e; assert(c.call(e) == 0); }
		{ Batch c = b; c.o.match_sc = 0; refuse_call(c); c.o.match_sc = -1; refuse_call(c); }
		{ Batch c = b; c.rep_len[1] = -1; refuse_call(c); }
		{ Batch c = b; c.regs_cap = -1; refuse_call(c); c.regs_cap = 0; c.cigar_cap = -1; refuse_call(c); }
		{ Batch c = b; c.regs_cap = 1; refuse_call(c, true, false, true); c.regs_cap = 0; c.cigar_cap = 1; refuse_call(c, true, true, false); }
		refuse_call(b, false); refuse_call(b, true, true, true, true);
		{ std::string e; assert(apost_check_call(nullptr, 0, nullptr, 0, 0, true, true, true, e) == -1); ++n_refused; }
		{ Batch c = b; c.regs_off[1] = 4; refuse_regs(c); }                      // falling offsets
		{ Batch c = b; c.regs_off[0] = 1; refuse_regs(c); }                      // not from 0
		{ Batch c = b; c.cigar_off[1] = 4; refuse_regs(c); }                     // falling CIGAR offsets (and a disagreeing n_cigar)
		{ Batch c = b; c.cigar_off[0] = 1; refuse_regs(c); }
		{ Batch c = b; c.extra[4] = 1; refuse_regs(c); }                         // n_cigar disagrees with cigar_off
		{ Batch c = b; c.extra[AP_EXTRA_WORDS] = 2; refuse_regs(c); c.extra[AP_EXTRA_WORDS] = -1; refuse_regs(c); }   // has_extra outside 0 / 1
		for (int which = 0; which < 5; ++which) refuse_regs(b, which);           // an array missing
	}
	{   // the logf list over a short range: sorted, inside the range, the host's values; x = 1 is not on it
		for (int sc = 1; sc <= 4; ++sc) {
			std::vector<uint32_t> k;
			std::vector<float> v;
			apost_logf_build(sc, 1 << 16, k, v);
			assert(k.size() == v.size());
			for (size_t i = 0; i < k.size(); ++i) {
				assert(k[i] >= 1 && k[i] <= (1u << 16) && (i == 0 || k[i - 1] < k[i]));
				const float h = apost_host_logf((int32_t)k[i], sc);
				assert(memcmp(&h, &v[i], 4) == 0);
			}
			assert(apost_host_logf(sc, sc) == 0.0f);
		}
	}
	printf("apost plan ok: %d batches accepted, %d calls refused\n", n_ok, n_refused);
	return 0;
}
