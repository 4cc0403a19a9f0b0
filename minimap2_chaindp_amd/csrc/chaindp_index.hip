// chaindp_index.hip -- the index image (blobs B, H, V, P of index.c:603-720) built on the device from the target's minimizers:
// what the reference does in worker_post (index.c:340-416) and in the serialisation loop of mm_idx_gen (index.c:612-701).
//
// With b = bucket bits and m = x >> 8, a minimizer lives in bucket m & (2^b - 1); inside a bucket the reference groups by m
// (ascending) and orders a group by y.  The pairs (m, y) are distinct, so any correct sort gives the one order.
//
//   prepare  k_ix_prepare: record = (m rotated right by b inside 56 bits, y), so that one unsigned compare of the first word orders
//            by (bucket, m >> b); m has at most 2k <= 56 bits.  The OR and the AND of both words over the input tell the host which
//            of the sixteen bytes differ anywhere: the others are no sort digits.
//   sort     stable LSD radix sort, 8-bit digits, one pass per byte that varies: k_ix_hist (digit counts per tile of 1024
//            records), launch_scan_u64 over (digit, tile), k_ix_scatter.  Inside a tile a wave owns four runs of 64 consecutive
//            records; a record's rank among the wave's equal digits comes from eight ballots, the waves' counts are added up in
//            tile order, so the pass is stable without any atomic.
//   group    k_ix_group: a record starts a group where the first word changes; keys and P words per bucket by one atomic per
//            (wave, bucket) after a segmented count over ballots; first record of every bucket.  k_ix_layout: slots of every
//            bucket's table as khash sizes it; two scans give the first slot (allh) and first P word (allp) of every bucket;
//            k_ix_bentries writes B.
//   tables   k_ix_tables: one lane per bucket replays khash (khash.h:232-336) on the bucket's groups in order: kh_resize(n_keys),
//            the puts, and the one expansion with its kick-out rehash when n_keys passes the upper bound of the first size.  It works
//            in place in H and V (which the host zero-filled), keeps "occupied" as one bit per slot in two scratch byte arrays (a
//            bucket's slots start at a multiple of eight, so every byte has one owner), zeroes what a moved element left behind and
//            writes the flag words last.  Empty slots therefore hold zero keys and values: the canonical image.
//   counts   k_ix_counts: occurrences per occupied slot of any image (1 for a key with bit 0 set, else the low word of the value),
//            what mm_idx_cal_max_occ (index.c:307-328) selects from.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chaindp_kernels.h"

namespace chaindp {

#define IX_WAVES 4
#define IX_ROUNDS 4                              // IX_TILE == IX_WAVES * IX_ROUNDS * 64
#define IX_REDUCE_BLOCKS 1024

// ---------------------------------------------------------------- prepare

__global__ __launch_bounds__(256) void k_ix_prepare(int64_t n, int b, const ulonglong2 *__restrict__ mini, ulonglong2 *__restrict__ rec,
                                                    unsigned long long *__restrict__ bits)
{
	const unsigned long long bmask = (1ull << b) - 1;
	unsigned long long o0 = 0, a0 = ~0ull, o1 = 0, a1 = ~0ull;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
		const ulonglong2 v = mini[i];
		const unsigned long long m = v.x >> 8;
		const unsigned long long key = (m & bmask) << (56 - b) | m >> b;
		rec[i] = make_ulonglong2(key, v.y);
		o0 |= key; a0 &= key; o1 |= v.y; a1 &= v.y;
	}
	for (int d = 1; d < 64; d <<= 1) {
		o0 |= __shfl_xor(o0, d, 64); a0 &= __shfl_xor(a0, d, 64);
		o1 |= __shfl_xor(o1, d, 64); a1 &= __shfl_xor(a1, d, 64);
	}
	if ((threadIdx.x & 63) == 0) {
		atomicOr(&bits[0], o0); atomicAnd(&bits[1], a0);
		atomicOr(&bits[2], o1); atomicAnd(&bits[3], a1);
	}
}

hipError_t launch_index_prepare(hipStream_t st, int b, int64_t n, const void *d_mini, void *d_rec, unsigned long long *d_bits)
{
	if (n <= 0) return hipSuccess;
	const int64_t blocks = (n + 255) / 256;
	hipLaunchKernelGGL(k_ix_prepare, dim3((unsigned)(blocks < IX_REDUCE_BLOCKS ? blocks : IX_REDUCE_BLOCKS)), dim3(256), 0, st, n, b,
	                   (const ulonglong2*)d_mini, (ulonglong2*)d_rec, d_bits);
	return hipGetLastError();
}

// ---------------------------------------------------------------- sort

__device__ __forceinline__ unsigned ix_digit(const ulonglong2 &v, int word, int shift)
{
	return (unsigned)((word ? v.y : v.x) >> shift) & 255u;
}

// hist[d * n_tiles + tile] = records of the tile with digit d
__global__ __launch_bounds__(256) void k_ix_hist(int64_t n, const ulonglong2 *__restrict__ src, int word, int shift,
                                                 unsigned long long *__restrict__ hist, int64_t n_tiles)
{
	__shared__ unsigned s_cnt[256];
	s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const int64_t base = (int64_t)blockIdx.x * IX_TILE;
	const unsigned long long *w = (const unsigned long long*)src + word;
	for (int r = 0; r < IX_TILE / 256; ++r) {
		const int64_t i = base + r * 256 + threadIdx.x;
		if (i < n) atomicAdd(&s_cnt[(unsigned)(w[2 * i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = s_cnt[threadIdx.x];
}

// hist scanned: first output place of the tile's records with digit d
__global__ __launch_bounds__(256) void k_ix_scatter(int64_t n, const ulonglong2 *__restrict__ src, ulonglong2 *__restrict__ dst, int word, int shift,
                                                    const unsigned long long *__restrict__ hist, int64_t n_tiles)
{
	__shared__ unsigned s_cnt[IX_WAVES][256];
	__shared__ unsigned long long s_base[IX_WAVES][256];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int k = 0; k < IX_WAVES; ++k) s_cnt[k][threadIdx.x] = 0;
	__syncthreads();
	const int64_t base = (int64_t)blockIdx.x * IX_TILE + wave * (IX_ROUNDS * 64) + lane;
	const unsigned long long below = (1ull << lane) - 1;
	ulonglong2 v[IX_ROUNDS];
	unsigned rank[IX_ROUNDS];
#pragma unroll
	for (int r = 0; r < IX_ROUNDS; ++r) {
		const int64_t i = base + r * 64;
		const bool valid = i < n;
		v[r] = valid ? src[i] : make_ulonglong2(0, 0);
		const unsigned d = ix_digit(v[r], word, shift);
		unsigned long long same = __ballot(valid);
#pragma unroll
		for (int bit = 0; bit < 8; ++bit) {
			const bool on = (d >> bit) & 1;
			const unsigned long long bal = __ballot(valid && on);
			same &= on ? bal : ~bal;
		}
		rank[r] = 0;
		if (valid) {
			const unsigned old = s_cnt[wave][d];
			rank[r] = old + (unsigned)__popcll(same & below);
			__builtin_amdgcn_wave_barrier();                      // every lane has read the count before the first of its digit moves it on
			if ((same & below) == 0) s_cnt[wave][d] = old + (unsigned)__popcll(same);
		}
		__builtin_amdgcn_wave_barrier();
	}
	__syncthreads();
	{
		unsigned long long run = hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x];
		for (int k = 0; k < IX_WAVES; ++k) { s_base[k][threadIdx.x] = run; run += s_cnt[k][threadIdx.x]; }
	}
	__syncthreads();
#pragma unroll
	for (int r = 0; r < IX_ROUNDS; ++r) {
		const int64_t i = base + r * 64;
		if (i < n) {
			const unsigned long long o = s_base[wave][ix_digit(v[r], word, shift)] + rank[r];
			if (o < (unsigned long long)n) dst[o] = v[r];
		}
	}
}

hipError_t launch_index_sort_pass(hipStream_t st, int64_t n, const void *d_src, void *d_dst, int word, int shift, unsigned long long *d_hist,
                                  unsigned long long *d_scan_tmp, unsigned long long *d_total)
{
	if (n <= 0) return hipSuccess;
	const int64_t tiles = (n + IX_TILE - 1) / IX_TILE;
	hipLaunchKernelGGL(k_ix_hist, dim3((unsigned)tiles), dim3(256), 0, st, n, (const ulonglong2*)d_src, word, shift, d_hist, tiles);
	if (hipError_t e = launch_scan_u64(st, 256 * tiles, d_hist, d_scan_tmp, d_total)) return e;
	hipLaunchKernelGGL(k_ix_scatter, dim3((unsigned)tiles), dim3(256), 0, st, n, (const ulonglong2*)d_src, (ulonglong2*)d_dst, word, shift, d_hist, tiles);
	return hipGetLastError();
}

// ---------------------------------------------------------------- group, layout, B

__global__ __launch_bounds__(256) void k_ix_group(int64_t n, int b, const ulonglong2 *__restrict__ rec, IndexScratch sc)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	const int lane = threadIdx.x & 63;
	const bool valid = i < n;
	unsigned long long key = 0, prev = 0, next = 0;
	bool has_prev = false, has_next = false;
	if (valid) {
		key = rec[i].x;
		if (i > 0) { prev = rec[i - 1].x; has_prev = true; }
		if (i + 1 < n) { next = rec[i + 1].x; has_next = true; }
	}
	const bool eq_prev = has_prev && prev == key, eq_next = has_next && next == key;
	const bool start = valid && !eq_prev, multi = valid && (eq_prev || eq_next);
	const unsigned bucket = (unsigned)(key >> (56 - b));
	const bool head = valid && (!has_prev || (unsigned)(prev >> (56 - b)) != bucket);
	if (head) sc.bk_start[bucket] = (unsigned long long)i;
	const unsigned long long H = __ballot(head || (valid && lane == 0)), S = __ballot(start), M = __ballot(multi);
	if (head || (valid && lane == 0)) {
		const unsigned long long from = ~0ull << lane;
		const unsigned long long above = lane == 63 ? 0ull : H & (~0ull << (lane + 1));
		const unsigned long long seg = above ? from & ((1ull << (__ffsll((long long)above) - 1)) - 1) : from;
		const unsigned nk = (unsigned)__popcll(S & seg), np = (unsigned)__popcll(M & seg);
		if (nk) atomicAdd(&sc.bk_keys[bucket], nk);
		if (np) atomicAdd(&sc.bk_p[bucket], np);
	}
}

// kh_resize(n_keys) on an empty table, and the expansion the puts run into (khash.h:237-239, 291, 298-303)
__device__ __forceinline__ unsigned ix_upper(unsigned long long N) { return (unsigned)((double)N * 0.77 + 0.5); }
__device__ __forceinline__ unsigned long long ix_first_size(unsigned n_keys)
{
	unsigned long long N = 4;
	while (N < n_keys) N <<= 1;
	return N;
}

__global__ __launch_bounds__(256) void k_ix_layout(int64_t n_buckets, IndexScratch sc)
{
	const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n_buckets) return;
	const unsigned n_keys = sc.bk_keys[k];
	unsigned long long slots = 0;
	if (n_keys) {
		unsigned long long N = ix_first_size(n_keys);
		const bool grown = n_keys > ix_upper(N);
		if (grown) N <<= 1;
		slots = (N + 7) & ~7ull;
		atomicAdd(&sc.totals[2], (unsigned long long)n_keys);
		atomicAdd(&sc.totals[3], 1ull);
		if (grown) atomicAdd(&sc.totals[4], 1ull);
		atomicMax(&sc.totals[5], (unsigned long long)n_keys);
	}
	sc.bk_h[k] = slots;
	sc.bk_pp[k] = sc.bk_p[k];
}

__global__ __launch_bounds__(256) void k_ix_bentries(int64_t n_buckets, IndexScratch sc, ulonglong2 *__restrict__ B)
{
	const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n_buckets) return;
	const unsigned n_keys = sc.bk_keys[k];
	ulonglong2 e = make_ulonglong2(0, 0);
	if (n_keys) {
		unsigned long long N = ix_first_size(n_keys);
		if (n_keys > ix_upper(N)) N <<= 1;
		const unsigned long long allh = sc.bk_h[k], allp = sc.bk_pp[k];
		e.x = (allp & 0xff) << 56 | N << 24;
		e.y = allh << 28 | allp >> 8;
	}
	B[k] = e;
}

hipError_t launch_index_group(hipStream_t st, int b, int64_t n, const void *d_rec, IndexScratch sc, void *d_B)
{
	const int64_t nb = (int64_t)1 << b;
	hipError_t e;
	if ((e = hipMemsetAsync(sc.bk_keys, 0, (size_t)nb * 4, st)) != hipSuccess) return e;
	if ((e = hipMemsetAsync(sc.bk_p, 0, (size_t)nb * 4, st)) != hipSuccess) return e;
	if ((e = hipMemsetAsync(sc.totals, 0, 8 * 8, st)) != hipSuccess) return e;
	if (n > 0) hipLaunchKernelGGL(k_ix_group, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, b, (const ulonglong2*)d_rec, sc);
	const dim3 g((unsigned)((nb + 255) / 256));
	hipLaunchKernelGGL(k_ix_layout, g, dim3(256), 0, st, nb, sc);
	if ((e = launch_scan_u64(st, nb, sc.bk_h, sc.scan_tmp, sc.totals + 0)) != hipSuccess) return e;
	if ((e = launch_scan_u64(st, nb, sc.bk_pp, sc.scan_tmp, sc.totals + 1)) != hipSuccess) return e;
	hipLaunchKernelGGL(k_ix_bentries, g, dim3(256), 0, st, nb, sc, (ulonglong2*)d_B);
	return hipGetLastError();
}

// ---------------------------------------------------------------- tables

// the 48-bit key of slot s (slots counted over the whole blob): 64-byte groups of a flag word, eight keys, twelve bytes of padding
__device__ __forceinline__ uint16_t *ix_key_at(uint8_t *H, unsigned long long s) { return (uint16_t*)(H + (s >> 3) * 64 + 4 + 6 * (s & 7)); }
__device__ __forceinline__ unsigned long long ix_key_get(uint8_t *H, unsigned long long s)
{
	const uint16_t *p = ix_key_at(H, s);
	return (unsigned long long)p[0] | (unsigned long long)p[1] << 16 | (unsigned long long)p[2] << 32;
}
__device__ __forceinline__ void ix_key_put(uint8_t *H, unsigned long long s, unsigned long long key)
{
	uint16_t *p = ix_key_at(H, s);
	p[0] = (uint16_t)key; p[1] = (uint16_t)(key >> 16); p[2] = (uint16_t)(key >> 32);
}
__device__ __forceinline__ bool ix_bit(const uint8_t *occ, unsigned long long s) { return (occ[s >> 3] >> (s & 7)) & 1; }
__device__ __forceinline__ void ix_bit_set(uint8_t *occ, unsigned long long s) { occ[s >> 3] = (uint8_t)(occ[s >> 3] | 1u << (s & 7)); }
__device__ __forceinline__ void ix_bit_clear(uint8_t *occ, unsigned long long s) { occ[s >> 3] = (uint8_t)(occ[s >> 3] & ~(1u << (s & 7))); }

// the position word of index.c:382-385 / 394-397
__device__ __forceinline__ unsigned long long ix_pos_word(unsigned long long y, const uint32_t *rank, int64_t n_seqs)
{
	const unsigned long long rid = y >> 32;
	const unsigned long long rk = !rank ? rid : rid < (unsigned long long)n_seqs ? rank[rid] : 0;
	return (rid & 0x1FFFFF) << 43 | (y & 0x3FFFFF) << 21 | (rk & 0x1FFFFF);
}

__global__ __launch_bounds__(64) void k_ix_tables(int64_t n, int b, const ulonglong2 *__restrict__ rec, IndexScratch sc, const uint32_t *__restrict__ rank,
                                                  int64_t n_seqs, uint8_t *__restrict__ H, unsigned long long *__restrict__ V,
                                                  unsigned long long *__restrict__ P, uint8_t *__restrict__ occ_a, uint8_t *__restrict__ occ_b)
{
	const int64_t bk = (int64_t)blockIdx.x * 64 + threadIdx.x;
	if (bk >= ((int64_t)1 << b)) return;
	const unsigned n_keys = sc.bk_keys[bk];
	if (!n_keys) return;
	const unsigned long long h0 = sc.bk_h[bk], p0 = sc.bk_pp[bk];
	const unsigned long long N0 = ix_first_size(n_keys);
	const unsigned upper = ix_upper(N0);
	unsigned long long N = N0;
	uint8_t *occ = occ_a + (h0 >> 3);
	uint8_t *Hb = H + (h0 >> 3) * 64;           // slots relative to the bucket from here on
	unsigned long long *Vb = V + h0;
	const unsigned long long low = (1ull << (56 - b)) - 1;
	unsigned long long start_p = 0;
	unsigned n_occ = 0;
	int64_t i = (int64_t)sc.bk_start[bk];
	for (unsigned g = 0; g < n_keys && i < n; ++g) {
		const unsigned long long key2 = rec[i].x;
		int64_t j = i + 1;
		while (j < n && rec[j].x == key2) ++j;
		const unsigned long long c = (unsigned long long)(j - i);
		unsigned long long key = (key2 & low) << 1, val;
		if (c == 1) {
			key |= 1;
			val = ix_pos_word(rec[i].y, rank, n_seqs);
		} else {
			for (int64_t t = i; t < j; ++t) P[p0 + start_p + (unsigned long long)(t - i)] = ix_pos_word(rec[t].y, rank, n_seqs);
			val = start_p << 32 | c;
			start_p += c;
		}
		i = j;
		if (n_occ >= upper && N == N0) {
			// kh_resize to 2 N0 (khash.h:256-282): old slots in order; an element is re-probed in the new flags and swaps with an
			// element of the old half that has not moved yet
			uint8_t *neu = occ_b + (h0 >> 3);
			const unsigned long long mask = 2 * N0 - 1;
			for (unsigned long long s = 0; s < N0; ++s) {
				if (!ix_bit(occ, s)) continue;
				unsigned long long mk = ix_key_get(Hb, s), mv = Vb[s];
				ix_bit_clear(occ, s);
				for (;;) {
					unsigned long long at = (uint32_t)(mk >> 1) & mask, step = 0;
					while (ix_bit(neu, at)) at = (at + ++step) & mask;
					ix_bit_set(neu, at);
					if (at < N0 && ix_bit(occ, at)) {
						const unsigned long long tk = ix_key_get(Hb, at), tv = Vb[at];
						ix_key_put(Hb, at, mk); Vb[at] = mv;
						mk = tk; mv = tv;
						ix_bit_clear(occ, at);
					} else {
						ix_key_put(Hb, at, mk); Vb[at] = mv;
						break;
					}
				}
			}
			occ = neu;
			N = 2 * N0;
		}
		unsigned long long at = (uint32_t)(key >> 1) & (N - 1), step = 0;
		while (ix_bit(occ, at)) at = (at + ++step) & (N - 1);
		ix_bit_set(occ, at);
		ix_key_put(Hb, at, key); Vb[at] = val;
		++n_occ;
	}
	const unsigned long long slots = (N + 7) & ~7ull;
	if (N != N0)                                 // what moved elements left behind in slots that ended up empty
		for (unsigned long long s = 0; s < N0; ++s) if (!ix_bit(occ, s)) { ix_key_put(Hb, s, 0); Vb[s] = 0; }
	// flag words (two bits per slot, sixteen slots per word, both groups of a word carry it): occupied 00, everything else 10
	for (unsigned long long g = 0; g < slots / 8; ++g) {
		uint32_t word = 0xAAAAAAAAu;
		const unsigned long long s0 = (g >> 1) * 16;
		for (unsigned long long t = 0; t < 16 && s0 + t < N; ++t) if (ix_bit(occ, s0 + t)) word &= ~(3u << (2 * t));
		*(uint32_t*)(Hb + g * 64) = word;
	}
}

hipError_t launch_index_tables(hipStream_t st, int b, int64_t n, const void *d_rec, IndexScratch sc, const uint32_t *d_rank, int64_t n_seqs,
                               void *d_H, void *d_V, void *d_P, uint8_t *d_occ_a, uint8_t *d_occ_b)
{
	const int64_t nb = (int64_t)1 << b;
	hipLaunchKernelGGL(k_ix_tables, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, n, b, (const ulonglong2*)d_rec, sc, d_rank, n_seqs,
	                   (uint8_t*)d_H, (unsigned long long*)d_V, (unsigned long long*)d_P, d_occ_a, d_occ_b);
	return hipGetLastError();
}

// ---------------------------------------------------------------- occurrence counts (mm_idx_cal_max_occ)

// counts[slot] = occurrences of the slot's minimizer, 0 for an empty slot; *bad is set if a B entry points outside H or V
__global__ __launch_bounds__(64) void k_ix_counts(SeedIndex ix, uint32_t *__restrict__ counts, unsigned *__restrict__ bad)
{
	const int64_t bk = (int64_t)blockIdx.x * 64 + threadIdx.x;
	if (bk >= ((int64_t)1 << ix.b_bits) || (uint64_t)(bk + 1) * 16 > ix.nB) return;
	const ulonglong2 e = ((const ulonglong2*)ix.B)[bk];
	const unsigned long long N = (e.x >> 24) & 0xffffffffull, h0 = e.y >> 28;
	if (!N) return;
	const unsigned long long slots = (N + 7) & ~7ull;
	if ((h0 & 7) || (h0 + slots) * 8 > ix.nV || (h0 + slots) / 8 * 64 > ix.nH) { *bad = 1; return; }
	for (unsigned long long s = 0; s < N; ++s) {
		const uint8_t *grp = ix.H + ((h0 + s) >> 3) * 64;
		const uint32_t fw = *(const uint32_t*)grp;
		if ((fw >> (2 * (s & 15))) & 3) continue;
		const uint32_t key_lo = *(const uint16_t*)(grp + 4 + 6 * (s & 7));
		counts[h0 + s] = (key_lo & 1) ? 1u : (uint32_t)((const unsigned long long*)ix.V)[h0 + s];
	}
}

hipError_t launch_index_counts(hipStream_t st, const SeedIndex &ix, uint32_t *d_counts, unsigned *d_bad)
{
	const int64_t nb = (int64_t)1 << ix.b_bits;
	hipLaunchKernelGGL(k_ix_counts, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, ix, d_counts, d_bad);
	return hipGetLastError();
}

} // namespace chaindp
