// chaindp_sketch.hip -- mm_sketch (sketch.c:77-143) + collect_minimizers' shift (map.c:87-99) for a batch of sequences, parallel
// inside every sequence, result identical to the reference in content and order.
//
// The reference walks a sequence base by base with a ring of the last w window entries.  Here nothing is carried from base to base:
// every step is one lane per element, and the three places where an element needs its rank among the elements before it are
// exclusive scans over 256-element tiles (count per tile, launch_scan_u64 over the tiles, a scan inside the tile).
//
//   pushes   the bases that shift into the k-mer: every unambiguous base; with homopolymer compression the last base of a run
//            (its first base writes the run's start under the same rank: no run end lies between the two).
//            k_sk_push_count -> scan -> k_sk_push: code, end and start position of every push, by rank.
//   k-mers   forward and reverse k-mer of push p from the codes of pushes p-k+1..p of its sequence (the reference never clears the
//            two words at an ambiguous base, and shifting into zeroed words equals leaving out the missing pushes).  A push whose
//            two k-mers are equal takes no window entry (sketch.c:106) -- with even k only -- so the entries ("slots") are the
//            ambiguous bases and the other pushes, in base order.  k_sk_kmer: hash and strand per push, slots per tile -> scan.
//   slots    k_sk_slots: x = hash << 8 | span, y, "ambiguous" per slot.  span = k, or under compression end(p) - start(p-k+1) + 1
//            (the k runs are contiguous when l >= k); span >= 256 leaves an empty entry that still occupies the window.
//            k_sk_value: l = slots since the last ambiguous one, counted backwards, never further than w + k; x stays only where
//            l >= k.  l matters through l >= k, l == w+k-1, l >= w+k only.
//   window   after every entry the reference's `min` is the rightmost smallest entry of the ring, so what slot s pushes depends on
//            the values of slots s-w..s and on l(s) alone (P = rightmost smallest of s-w..s-1, Q of s-w+1..s):
//              l == w+k-1, P not empty:  the slots of s-w+1..s-1 that tie with P              (sketch.c:117-122)
//              x(s) <= x(P):             P if l >= w+k                                          (sketch.c:123-125)
//              else if P is slot s-w:    P if l >= w+k-1; then the window's ties with Q         (sketch.c:126-138)
//              last slot:                the current minimum                                    (sketch.c:141-142)
//            The ring is not cleared at an ambiguous base and neither is this window; slots before the sequence's first are empty.
//            k_sk_window<false> counts per slot and per tile -> scan -> k_sk_read_off (mini_off) and k_sk_window<true>, which writes
//            the minimizers at their offsets: the order is the slot order, no atomic is involved.
//
// Tiles of bases never straddle sequences (the host lists the 256-base chunks of every sequence, an empty sequence gets one empty
// chunk), tiles of slots do: a slot carries its sequence.  The index-side sketch (mm_idx_gen's, rid = the sequence's number) is the same
// kernels with another seq_ybase (chaindp_index_build).  Out of scope: mm_dust_minier (sdust_thres is 0 in every preset), 2-bit packed
// input, sequence packets through the fpga_* shim.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chaindp_kernels.h"

namespace chaindp {

#define SK_TILE 256
#define SK_NONE 0xffffffffffffffffull

// seq_nt4_table: A C G T/U in either case and the bytes 0..3 themselves; everything else is ambiguous
__device__ __forceinline__ int sk_nt4(uint32_t b)
{
	if (b < 4) return (int)b;
	const uint32_t l = b | 0x20u;
	return l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : (l == 't' || l == 'u') ? 3 : 4;
}

// hash64 of sketch.c:28-38
__device__ __forceinline__ uint64_t sk_hash64(uint64_t key, uint64_t mask)
{
	key = (~key + (key << 21)) & mask;
	key = key ^ key >> 24;
	key = ((key + (key << 3)) + (key << 8)) & mask;
	key = key ^ key >> 14;
	key = ((key + (key << 2)) + (key << 4)) & mask;
	key = key ^ key >> 28;
	key = (key + (key << 31)) & mask;
	return key;
}

// exclusive scan of one int per thread over the 256 threads of a block; total = the block's sum.  s_w: 4 ints of LDS.
__device__ __forceinline__ int sk_block_scan(int v, int *s_w, int &total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int incl = v;
	for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
	__syncthreads();                       // the previous scan's readers are done with s_w
	if (lane == 63) s_w[wave] = incl;
	__syncthreads();
	int woff = 0, all = 0;
	for (int k = 0; k < 4; ++k) { const int t = s_w[k]; if (k < wave) woff += t; all += t; }
	total = all;
	return woff + incl - v;
}

// what a thread of a base tile knows about its base
struct SkBase {
	int seq, pos, len;       // sequence, position in it, its length; pos >= len: no base
	int c;                   // code, 4 ambiguous, 5 no base
	bool end, start;         // shifts into the k-mer / first base of such a run
};

__device__ __forceinline__ SkBase sk_base(const SketchArgs &a, int chunk)
{
	SkBase b;
	b.seq = a.chunk_seq[chunk];
	const int64_t s0 = a.seq_off[b.seq];
	b.len = (int)(a.seq_off[b.seq + 1] - s0);
	b.pos = (chunk - a.seq_chunk0[b.seq]) * SK_TILE + (int)threadIdx.x;
	b.c = 5; b.end = b.start = false;
	if (b.pos < b.len) {
		const uint8_t *p = a.seq + s0 + b.pos;
		b.c = sk_nt4(p[0]);
		if (b.c < 4) {
			b.end = !a.is_hpc || b.pos + 1 >= b.len || sk_nt4(p[1]) != b.c;
			b.start = !a.is_hpc || b.pos == 0 || sk_nt4(p[-1]) != b.c;
		}
	}
	return b;
}

__global__ __launch_bounds__(SK_TILE) void k_sk_push_count(SketchArgs a)
{
	__shared__ int s_w[4];
	const SkBase b = sk_base(a, blockIdx.x);
	int total;
	(void)sk_block_scan(b.end ? 1 : 0, s_w, total);
	if (threadIdx.x == 0) a.chunk_push[blockIdx.x] = (unsigned long long)total;
	if (blockIdx.x == 0 && threadIdx.x == 0) a.chunk_push[a.n_chunks] = 0;
}

__global__ __launch_bounds__(SK_TILE) void k_sk_push(SketchArgs a)
{
	__shared__ int s_w[4];
	const SkBase b = sk_base(a, blockIdx.x);
	int total;
	const int64_t rank = (int64_t)a.chunk_push[blockIdx.x] + sk_block_scan(b.end ? 1 : 0, s_w, total);
	if (b.end) { a.pcode[rank] = (uint8_t)b.c; a.pend[rank] = b.pos; }
	if (b.start && a.is_hpc) a.pstart[rank] = b.pos;
}

__global__ __launch_bounds__(SK_TILE) void k_sk_kmer(SketchArgs a)
{
	__shared__ int s_w[4];
	const SkBase b = sk_base(a, blockIdx.x);
	int total;
	const int64_t rank = (int64_t)a.chunk_push[blockIdx.x] + sk_block_scan(b.end ? 1 : 0, s_w, total);
	bool slot = b.c == 4;
	if (b.end) {
		const int64_t p0 = (int64_t)a.chunk_push[a.seq_chunk0[b.seq]];
		const int64_t have = rank - p0 + 1;
		const int n = have < a.k ? (int)have : a.k;
		uint64_t k0 = 0, k1 = 0;
		const unsigned long long *pw = (const unsigned long long*)a.pcode;      // eight codes per load (pcode is padded to a multiple of 8)
		int64_t wi = rank >> 3;
		unsigned long long word = pw[wi];
		for (int j = 0; j < n; ++j) {
			const int64_t q = rank - j;
			if ((q >> 3) != wi) { wi = q >> 3; word = pw[wi]; }
			const uint64_t c = (word >> (8 * (int)(q & 7))) & 3;
			k0 |= c << (2 * j);
			k1 |= (3ull ^ c) << (2 * (a.k - 1 - j));
		}
		unsigned long long hz = SK_NONE;              // symmetric: no strand, no slot
		if (k0 != k1) {
			const int z = k0 < k1 ? 0 : 1;
			hz = sk_hash64(z ? k1 : k0, (1ull << 2 * a.k) - 1) << 1 | (unsigned)z;
			slot = true;
		}
		a.phz[rank] = hz;
	}
	(void)sk_block_scan(slot ? 1 : 0, s_w, total);
	if (threadIdx.x == 0) a.chunk_slot[blockIdx.x] = (unsigned long long)total;
	if (blockIdx.x == 0 && threadIdx.x == 0) a.chunk_slot[a.n_chunks] = 0;
}

__global__ __launch_bounds__(SK_TILE) void k_sk_slots(SketchArgs a)
{
	__shared__ int s_w[4];
	const SkBase b = sk_base(a, blockIdx.x);
	int total;
	const int64_t rank = (int64_t)a.chunk_push[blockIdx.x] + sk_block_scan(b.end ? 1 : 0, s_w, total);
	unsigned long long hz = SK_NONE;
	if (b.end) hz = a.phz[rank];
	const bool slot = b.c == 4 || hz != SK_NONE;
	const int64_t s = (int64_t)a.chunk_slot[blockIdx.x] + sk_block_scan(slot ? 1 : 0, s_w, total);
	if (!slot) return;
	unsigned long long x = SK_NONE, y = SK_NONE;
	if (b.c < 4) {
		const int64_t p0 = (int64_t)a.chunk_push[a.seq_chunk0[b.seq]];
		int span = a.k;
		if (a.is_hpc) span = rank - a.k + 1 >= p0 ? b.pos - a.pstart[rank - a.k + 1] + 1 : 256;   // fewer than k pushes: l < k, no entry
		if (span < 256) {
			x = (hz >> 1) << 8 | (unsigned)span;
			y = a.seq_ybase[b.seq] + ((unsigned long long)(uint32_t)b.pos << 1 | (hz & 1));
		}
	}
	a.sx[s] = x; a.sy[s] = y;
	a.sn[s] = b.c == 4 ? 1 : 0;
	a.sseq[s] = b.seq;
}

// l of every slot and what it means: lcode 0 (l < w+k-1), 1 (l == w+k-1), 2 (l >= w+k); x goes where l < k
__global__ __launch_bounds__(SK_TILE) void k_sk_value(SketchArgs a)
{
	const int64_t n_slots = (int64_t)a.chunk_slot[a.n_chunks];
	const int64_t s = (int64_t)blockIdx.x * SK_TILE + threadIdx.x;
	if (s >= n_slots) return;
	const int64_t s0 = (int64_t)a.chunk_slot[a.seq_chunk0[a.sseq[s]]];
	const int cap = a.w + a.k;
	int l = 0;
	if (!a.sn[s]) {
		// the nearest ambiguous slot among s0 .. s-1, no further back than cap slots: eight flag bytes per load (sn is padded to a
		// multiple of 8 and the bytes outside lo..s are masked off)
		const int64_t lo = s - cap + 1 > s0 ? s - cap + 1 : s0;
		l = (int)(s - lo + 1);
		const unsigned long long *words = (const unsigned long long*)a.sn;
		for (int64_t wi = s >> 3; wi >= (lo >> 3); --wi) {
			unsigned long long m = words[wi];
			const int64_t b0 = wi << 3;
			if (b0 + 7 > s) m &= ~0ull >> (8 * (int)(b0 + 7 - s));          // bytes after s
			if (b0 < lo) m &= ~0ull << (8 * (int)(lo - b0));                // bytes before lo
			if (m) { l = (int)(s - (b0 + ((63 - __builtin_clzll(m)) >> 3))); break; }
		}
	}
	if (l < a.k) a.sx[s] = SK_NONE;        // nobody else reads sx before the next kernel
	a.slc[s] = l >= cap ? 2 : l == cap - 1 ? 1 : 0;
}

// EMIT == false: minimizers per slot (scnt: the count, and in bits 16.. the distance to the pushed slot where it is one) and per tile
// of slots (tile_cnt).
// EMIT == true: tile_cnt holds the tiles' output offsets; the slots that push write theirs in order.
template <bool EMIT>
__global__ __launch_bounds__(SK_TILE) void k_sk_window(SketchArgs a, ulonglong2 *__restrict__ out, int64_t out_cap)
{
	__shared__ int s_w[4];
	__shared__ unsigned long long s_x[EMIT ? 1 : 2 * SK_TILE];
	const int64_t n_slots = (int64_t)a.chunk_slot[a.n_chunks];
	const int64_t tile0 = (int64_t)blockIdx.x * SK_TILE, s = tile0 + threadIdx.x;
	const int w = a.w;
	if (!EMIT) {       // the values of slots tile0-w .. tile0+255 (w <= 255): s_x[t - tile0 + 256]
		for (int j = threadIdx.x; j < 2 * SK_TILE; j += SK_TILE) {
			const int64_t t = tile0 - SK_TILE + j;
			s_x[j] = t >= 0 && t < n_slots ? a.sx[t] : SK_NONE;
		}
		__syncthreads();
	}
	auto X = [&](int64_t t) -> unsigned long long { return EMIT ? a.sx[t] : s_x[t - tile0 + SK_TILE]; };
	int cnt = 0;
	int64_t o = 0, last = 0;
	if (EMIT) {
		const uint32_t c = s < n_slots ? a.scnt[s] : 0;
		cnt = (int)(c & 0xffffu);
		int total;
		o = (int64_t)a.tile_cnt[blockIdx.x] + sk_block_scan(cnt, s_w, total);
		if (cnt == 0) return;
		if (cnt == 1) {                      // nearly every slot that pushes pushes one: the count pass left its distance
			const int64_t t = s - (int64_t)(c >> 16);
			if (o < out_cap) out[o] = make_ulonglong2(a.sx[t], a.sy[t]);
			return;
		}
		cnt = 0;
	}
	auto push = [&](int64_t t) {
		if (EMIT) { if (o + cnt < out_cap) out[o + cnt] = make_ulonglong2(a.sx[t], a.sy[t]); }
		last = t;
		++cnt;
	};
	if (s < n_slots) {
		const int seq = a.sseq[s];
		const int64_t s0 = (int64_t)a.chunk_slot[a.seq_chunk0[seq]], s1 = (int64_t)a.chunk_slot[a.seq_chunk0[seq + 1]];
		const int lc = a.slc[s];
		const int64_t lo = s - w + 1 > s0 ? s - w + 1 : s0;                 // first real slot of the window that ends at s
		unsigned long long px = SK_NONE;
		int64_t pt = s - w;
		for (int64_t t = s - w > s0 ? s - w : s0; t < s; ++t) { const unsigned long long v = X(t); if (v <= px) { px = v; pt = t; } }
		const unsigned long long xs = X(s);
		if (lc == 1 && px != SK_NONE)
			for (int64_t t = lo; t < s; ++t) if (X(t) == px && t != pt) push(t);
		int64_t cur = pt;
		unsigned long long cx = px;
		if (xs <= px) {
			if (lc == 2 && px != SK_NONE) push(pt);
			cur = s; cx = xs;
		} else if (pt == s - w) {
			if (lc >= 1) push(pt);
			cx = SK_NONE;
			for (int64_t t = lo; t <= s; ++t) { const unsigned long long v = X(t); if (v <= cx) { cx = v; cur = t; } }
			if (lc >= 1 && cx != SK_NONE)
				for (int64_t t = lo; t <= s; ++t) if (X(t) == cx && t != cur) push(t);
		}
		if (s == s1 - 1 && cx != SK_NONE) push(cur);
	}
	if (!EMIT) {
		if (s < n_slots) a.scnt[s] = (uint32_t)cnt | (cnt == 1 ? (uint32_t)(s - last) << 16 : 0u);
		int total;
		(void)sk_block_scan(cnt, s_w, total);
		if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = (unsigned long long)total;
	}
}

// mini_off[r] = minimizers pushed by the slots before the first slot of read r's first sequence: its tile's offset plus the counts
// of the slots of that tile before it
__global__ __launch_bounds__(256) void k_sk_read_off(SketchArgs a, int64_t n_reads, const unsigned long long *__restrict__ total,
                                                     unsigned long long *__restrict__ mini_off)
{
	const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (r > n_reads) return;
	const int64_t n_slots = a.n_chunks ? (int64_t)a.chunk_slot[a.n_chunks] : 0;
	unsigned long long o = *total;
	if (r < n_reads) {
		const int64_t s0 = (int64_t)a.chunk_slot[a.seq_chunk0[a.read_seq0 ? a.read_seq0[r] : (int)r]];
		if (s0 < n_slots) {
			o = a.tile_cnt[s0 / SK_TILE];
			for (int64_t t = s0 / SK_TILE * SK_TILE; t < s0; ++t) o += a.scnt[t] & 0xffffu;
		}
	}
	mini_off[r] = o;
}

hipError_t launch_sketch_count(hipStream_t st, const SketchArgs &a, int64_t n_reads, int64_t n_bases, unsigned long long *d_mini_off,
                               unsigned long long *d_totals)
{
	hipError_t e;
	const unsigned chunks = (unsigned)a.n_chunks, tiles = (unsigned)((n_bases + SK_TILE - 1) / SK_TILE);
	if ((e = hipMemsetAsync(d_totals, 0, 4 * 8, st)) != hipSuccess) return e;
	if (chunks) {
		hipLaunchKernelGGL(k_sk_push_count, dim3(chunks), dim3(SK_TILE), 0, st, a);
		if ((e = launch_scan_u64(st, a.n_chunks + 1, a.chunk_push, a.scan_tmp, d_totals)) != hipSuccess) return e;
		hipLaunchKernelGGL(k_sk_push, dim3(chunks), dim3(SK_TILE), 0, st, a);
		hipLaunchKernelGGL(k_sk_kmer, dim3(chunks), dim3(SK_TILE), 0, st, a);
		if ((e = launch_scan_u64(st, a.n_chunks + 1, a.chunk_slot, a.scan_tmp, d_totals + 1)) != hipSuccess) return e;
		hipLaunchKernelGGL(k_sk_slots, dim3(chunks), dim3(SK_TILE), 0, st, a);
	}
	if (tiles) {
		// the slot count stays on the device: the grid covers the most there can be (one per base), the rest return at once
		hipLaunchKernelGGL(k_sk_value, dim3(tiles), dim3(SK_TILE), 0, st, a);
		hipLaunchKernelGGL(k_sk_window<false>, dim3(tiles), dim3(SK_TILE), 0, st, a, (ulonglong2*)nullptr, (int64_t)0);
		if ((e = launch_scan_u64(st, tiles, a.tile_cnt, a.scan_tmp, d_totals + 2)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_sk_read_off, dim3((unsigned)((n_reads + 256) / 256)), dim3(256), 0, st, a, n_reads, d_totals + 2, d_mini_off);
	return hipGetLastError();
}

hipError_t launch_sketch_emit(hipStream_t st, const SketchArgs &a, int64_t n_bases, void *d_mini, int64_t mini_cap)
{
	const unsigned tiles = (unsigned)((n_bases + SK_TILE - 1) / SK_TILE);
	if (tiles) hipLaunchKernelGGL(k_sk_window<true>, dim3(tiles), dim3(SK_TILE), 0, st, a, (ulonglong2*)d_mini, mini_cap);
	return hipGetLastError();
}

} // namespace chaindp
