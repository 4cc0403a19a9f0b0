"""Constructive inputs for seed collection (csrc/chaindp_seed.hip): index images built anchor by anchor, so that a case dictates every
anchor's x -- the strand digit (byte 7), three id digits (bytes 6..4), the always-zero byte 3 and three position digits (bytes 2..0)
-- and through the hit counts the exact number of anchors of every read.  One constructor per group of routing edges: the sizes at
which the per-read sort takes another instantiation, LDS layout or kernel, the bucket and queue limits of the reference's procedure
restated in LDS, the limits of k_seed_sort_huge, and the read / block / chunk / tile edges of the probe, expand and reads kernels.

A case is (image, flag, max_occ, mini_off, mini, bid, qlen) plus a dict `props` of what it claims; tests/test_seed_edge_shapes_cpu.py
proves the claims, tests/test_gpu_seed_edges.py runs the cases on the GPU.  Cases are built relative to the limits handed in
(Limits: max_n, max_n2, lab_cap), never to literal sizes of one device.

An index position is rid << 43 | rpos << 22 | strand << 21 | rank (rank: the id skip_seed compares with bid).  A minimizer's hits
all get the minimizer's y, so two anchors of equal x always come from two minimizers: the order the sort leaves them in shows in y."""
import collections

import numpy as np

Limits = collections.namedtuple("Limits", "max_n max_n2 lab_cap")
Case = collections.namedtuple("Case", "image flag max_occ mini_off mini bid qlen")

HUGE_STACK = 320                         # SEED_HUGE_STACK
F_NO_DIAG, F_NO_DUAL, F_FOR_ONLY, F_REV_ONLY = 0x001, 0x002, 0x100000, 0x200000
TANDEM_BIT, SELF_BIT = 1 << 42, 1 << 43
ABSENT = 1 << 40                         # minimizers from here on are in no image


def cap_of(L):
    return max(L.max_n, L.max_n2)


def huge_max(L):
    return HUGE_STACK * cap_of(L)


def position(rid, rpos, strand=0, rank=0):
    return rid << 43 | rpos << 22 | strand << 21 | rank


def anchor_x(rid, rpos, rev=0):
    return rev << 63 | rid << 32 | rpos


# ---------------------------------------------------------------- the image (index.c:603-720) with khash's probing (khash.h:218-231)

def build_image(table, b_bits=6):
    """{minimizer: [positions]} -> (the blobs B, H, V, P, {minimizer: occupied slots its probe passes before it finds its key}).
    Minimizers go into their bucket's hash table in the dict's order; one position is stored in V, several as a list in P."""
    mask = (1 << b_bits) - 1
    buckets = [[] for _ in range(1 << b_bits)]
    for m in table:
        buckets[m & mask].append(m)
    B, H, V, Pa, collisions = bytearray(), bytearray(), [], [], {}
    allh = allp = 0
    for bk in buckets:
        if not bk:
            B += (0).to_bytes(16, "little")
            continue
        nb = 4
        while nb < 2 * len(bk):
            nb <<= 1
        slots_k, slots_v, used, p_local = [0] * nb, [0] * nb, [False] * nb, []
        for m in bk:
            pos = table[m]
            key = (m >> b_bits) << 1
            i, step = (key >> 1) & (nb - 1), 0
            while used[i]:
                step += 1
                i = (i + step) & (nb - 1)
            used[i] = True
            collisions[m] = step
            if len(pos) == 1:
                slots_k[i], slots_v[i] = key | 1, pos[0]
            else:
                slots_k[i], slots_v[i] = key, len(p_local) << 32 | len(pos)
                p_local += pos
        tmp_nb = (nb + 7) & ~7
        B += (((allp & 0xff) << 56) | (nb << 24)).to_bytes(8, "little") + ((allh << 28) | (allp >> 8)).to_bytes(8, "little")
        flags = [0] * max(1, nb >> 4)
        for i in range(nb):
            if not used[i]:
                flags[i >> 4] |= 2 << ((i & 15) << 1)                 # "empty" (khash.h:166)
        for g0 in range(0, tmp_nb, 8):
            H += (flags[g0 >> 4] & 0xffffffff).to_bytes(4, "little")
            for i in range(g0, g0 + 8):
                H += ((slots_k[i] if i < nb else 0) & 0xffffffffffff).to_bytes(6, "little")
                V.append(slots_v[i] if i < nb else 0)
            H += bytes(12)
        Pa += p_local
        allh += tmp_nb
        allp += len(p_local)
    blobs = [np.frombuffer(bytes(B), np.uint8).copy(), np.frombuffer(bytes(H), np.uint8).copy(),
             np.array(V, np.uint64).view(np.uint8).copy(), np.array(Pa, np.uint64).view(np.uint8).copy()]
    return blobs, collisions


def random_table(rng, n_keys, max_cnt, b_bits=6, rid_pool=None, pos_bits=21):
    """Random minimizers with 1..max_cnt random positions each, in the order build_image stores them -> ({minimizer: [positions]}, keys)."""
    keys = rng.choice(1 << 34, size=n_keys, replace=False).astype(np.uint64) + np.uint64(1)
    buckets = [[] for _ in range(1 << b_bits)]
    for m in keys:
        buckets[int(m) & ((1 << b_bits) - 1)].append(int(m))
    table = {}
    for bk in buckets:
        for m in bk:
            cnt = int(rng.integers(1, max_cnt + 1))
            table[m] = [int(rng.integers(0, rid_pool or 1 << 20)) << 43 | int(rng.integers(0, 1 << pos_bits)) << 22 | int(rng.integers(0, 2)) << 21 | int(rng.integers(0, 1 << 10))
                        for _ in range(cnt)]
    return table, keys


class Batch:
    """Reads over one image.  key() registers a minimizer with its positions; read() appends a read of (key, span, q_pos, q_strand)
    minimizers; anchors() appends a read that yields exactly the given x values, in the given order."""

    def __init__(self, flag=0, max_occ=64, b_bits=6):
        self.flag, self.max_occ, self.b_bits = flag, max_occ, b_bits
        self.table, self.rows, self.mini_off, self.bid, self.qlen, self._next = {}, [], [0], [], [], 0
        self.unsorted = {}                                   # read -> its anchors as k_seed_expand writes them (reads made by anchors())
        self.shared, self.parts, self._mark = False, [], 0   # shared: several constructors add their reads (combined()); parts: what each claimed

    def key(self, positions, at=None):
        if at is None:
            self._next += 1
            at = self._next
        assert at not in self.table and at < ABSENT
        self.table[at] = list(positions)
        return at

    def read(self, minis, bid=0, qlen=None):
        for k, span, qpos, qstrand in minis:
            self.rows.append((k << 8 | span, qpos << 1 | qstrand))
        self.mini_off.append(len(self.rows))
        self.bid.append(bid)
        self.qlen.append(qlen if qlen is not None else max([q for _, _, q, _ in minis], default=0) + 200)
        return len(self.bid) - 1

    def anchors(self, xs, per=None, bid=0):
        """A read whose anchors are xs, in this order (x = rev << 63 | rid << 32 | rpos): `per` hits a minimizer."""
        per = per or (1 if len(xs) <= 64 else 16)
        assert per < self.max_occ
        minis = []
        for k in range(0, len(xs), per):
            part = [int(x) for x in xs[k:k + per]]
            assert len(set(part)) == len(part), "anchors of equal x must come from different minimizers"
            minis.append((self.key([position(x >> 32 & 0x1fffff, x & 0x1fffff, x >> 63) for x in part]), 15, 40 + 30 * (k // per), 0))
        r = self.read(minis, bid=bid)
        ql = self.qlen[r]
        ys = [15 << 32 | ((ql - (40 + 30 * (k // per) + 1 - 15) - 1) & 0xffffffff if int(x) >> 63 else 40 + 30 * (k // per)) for k, x in enumerate(xs)]
        self.unsorted[r] = np.array([[int(x), y] for x, y in zip(xs, ys)], np.uint64).reshape(-1, 2)
        return r

    def build(self):
        """-> (the case, {minimizer: occupied slots its probe passes})"""
        image, collisions = build_image(self.table, self.b_bits)
        return Case(image, self.flag, self.max_occ, np.array(self.mini_off, np.int64), np.array(self.rows, np.uint64).reshape(-1, 2),
                    np.array(self.bid, np.uint32), np.array(self.qlen, np.int32)), collisions

    def case(self):
        return self.build()[0]


# ---------------------------------------------------------------- reads for the sort

def sorted_xs(n):
    """n distinct x, ascending: the first ceil(n / 2) on the forward strand, the rest on the reverse; 97 positions per id."""
    fwd = (n + 1) // 2
    return [anchor_x(j // 97, (j % 97) * 523 + (j // 97) * 3, 0) for j in range(fwd)] + [anchor_x(j // 97, (j % 97) * 523 + (j // 97) * 3, 1) for j in range(n - fwd)]


TIES = (None, "front", "mid", "end")


def tie_place(n, tie):
    """The sorted place p of the tied pair (p, p + 1): front (0, 1); mid (1023, 1024), the last thread of the tie detector's first
    stride; end (n - 2, n - 1).  None where the read has no such places."""
    p = {None: None, "front": 0, "mid": 1023, "end": n - 2}[tie]
    return p if p is not None and 0 <= p and p + 1 < n else None


def shuffled(xs, seed, per, apart=None):
    """xs in a seeded order; apart = (i, j): xs[i] and xs[j] (the tied pair) fall into different minimizers of `per` hits."""
    perm = [int(i) for i in np.random.default_rng(seed).permutation(len(xs))]
    if apart is not None:
        i, j = apart
        ki, kj = perm.index(i), perm.index(j)
        if ki // per == kj // per:
            k2 = (kj + per) % len(xs)
            assert k2 // per != ki // per
            perm[k2], perm[kj] = perm[kj], perm[k2]
    return [xs[i] for i in perm]


def shuffled_pairs(firsts, seconds, rest, seed):
    """Tied pairs (firsts[i] == seconds[i]) and tie-free `rest` in a seeded order that keeps partners at least len(firsts) >= 16
    places apart: the partners' halves take the same permutation, the rest follows shuffled."""
    assert len(firsts) == len(seconds) >= 16
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(firsts))
    return [firsts[i] for i in perm] + [seconds[i] for i in perm] + [rest[i] for i in rng.permutation(len(rest))]


def add_sorted_read(b, n, tie=None):
    """A read of n anchors with distinct x but for one tied pair at tie_place(n, tie).  -> props of the read"""
    xs = sorted_xs(n)
    p = tie_place(n, tie)
    per = 1 if n <= 64 else 16
    if p is not None:
        xs[p + 1] = xs[p]
    b.anchors(shuffled(xs, 7 * n + TIES.index(tie), per, apart=(p, p + 1) if p is not None else None), per=per)
    return dict(n=n, tied_pairs=int(p is not None), tie_at=p)


def lds_route(L, n):
    """What takes a read of n anchors: the sixteen-wave layout, the four-wave layout, k_seed_sort_huge or the one-thread kernel."""
    return "lds16" if n <= L.max_n else "lds4" if n <= cap_of(L) else "huge" if n <= huge_max(L) else "big"


def _finish(b, reads=None, **more):
    """The end of every constructor.  reads: what it claims per read it added (n, tied_pairs; None for the cases that are not about
    the sort).  A batch of its own -> (case, props); a shared batch -> the claims are noted in b.parts and combined() finishes."""
    added = len(b.bid) - b._mark
    reads = reads if reads is not None else [dict(n=None, tied_pairs=None) for _ in range(added)]
    assert len(reads) == added
    b._mark = len(b.bid)
    if b.shared:
        b.parts.append((reads, more))
        return None
    props = dict(n=[r["n"] for r in reads], tied_pairs=[r["tied_pairs"] for r in reads], reads=reads, unsorted=b.unsorted)
    props.update(more)
    return b.case(), props


def sorted_read(L, n, tie=None, b=None):
    """Radix instantiation edges (n = 1024 k, 1024 k + 1: the last thread holds 0, 1 or I words), layout edges (max_n, max_n2 and
    one more), the pair network's sizes under CHAINDP_SEED_MAX_N=64,512, and 129 / 40960 / 40961 anchors under 128,128."""
    b = b or Batch()
    r = add_sorted_read(b, n, tie)
    return _finish(b, [r], route=lds_route(L, n), radix_items=-(-n // 1024))


def layout_read(L, which, plus, tie=None, b=None):
    """A read of max_n, max_n2 (which) or one more (plus) anchors: the last read of the sixteen-wave layout and the first of the
    four-wave one; the last read sorted in LDS and the smallest for k_seed_sort_huge."""
    return sorted_read(L, getattr(L, which) + plus, tie, b=b)


def whole_small_read(L, n, b=None):
    """A read of n <= 65 anchors in which every fourth sorted place is tied with the next: 64 anchors are insertion-sorted as a whole
    (stable), 65 go through the radix passes, which do not keep equal x in their order of generation."""
    xs = sorted_xs(n)
    for p in range(0, n - 1, 4):
        xs[p + 1] = xs[p]
    b = b or Batch()
    b.anchors(shuffled(xs, 4242 + n, 1), per=1)
    return _finish(b, [dict(n=n, tied_pairs=len(range(0, n - 1, 4)))], route=lds_route(L, n))


RADIX_SIZES = [1, 2, 63] + [1024 * k + d for k in range(1, 13) for d in (0, 1)]
PAIR_SIZES = [65, 127, 128, 129, 255, 256, 257, 511, 512]


def level_bucket(L, shift, size, b=None):
    """The reference's procedure: a read of 200 anchors in which the pass at `shift` (48, 40, 32: id digits; 16, 8: position
    digits) leaves one bucket of exactly `size` anchors (64: insertion-sorted, which keeps equal x in their order; 65: down a level,
    where the passes do not) beside smaller ones; the bucket holds eight tied pairs; the levels above have one digit and are skipped.  shift 0: `size` anchors
    of one x (a bucket of the last pass) among the 200."""
    assert size <= 100 and shift in (48, 40, 32, 16, 8, 0)
    base = anchor_x(0x050505, 0x050505)                                          # digit 5 in every byte but 3 and 7
    lo = 32 if shift >= 40 else 0                                                # a byte below `shift` that tells the anchors apart

    def put(x, sh, d):
        return (x & ~(0xff << sh)) | d << sh
    narrow = shift in (48, 16)                                                   # bytes 6 and 2 hold five bits
    xs = [base if shift == 0 else put(base, lo, 6 + j - (j % 8 == 1)) for j in range(size)]       # (every eighth anchor of the bucket tied with the one before)
    for j in range(200 - size):                                                  # the others: another digit at `shift`, a few per digit
        xs.append(put(base, 0, 6 + j) if shift == 0 else put(put(base, shift, 6 + j % 26 if narrow else 6 + (j >> 1)), lo, 6 + j))
    ties = size - 1 if shift == 0 else len(range(1, size, 8))
    assert max(xs) < 1 << 53 and all(x & 0xffe00000 == 0 for x in xs) and len(set(xs)) == 200 - ties
    b = b or Batch()
    b.anchors(shuffled(xs, 1000 + shift + size, 1), per=1)                       # a minimizer per anchor: the order of equal x shows in y
    return _finish(b, [dict(n=200, tied_pairs=ties)], route=lds_route(L, 200), bucket=(shift, size))


def top_digits(L, n_digits, b=None):
    """A tied read of 200 anchors and the digits of its first level that is not skipped: 1 -- one strand, one id (every level down to the
    positions is skipped); 2 -- two strands (the closed form at shift 56); 3 -- one strand, three values of byte 6 (the serial walk)."""
    if n_digits == 1:
        xs = [anchor_x(7, 11 * j) for j in range(200)]
    elif n_digits == 2:
        xs = [anchor_x(7, 11 * j, j % 2) for j in range(200)]
    else:
        xs = [anchor_x((j % 3) << 16 | 7, 11 * j) for j in range(200)]
    xs[-1] = xs[-3]
    b = b or Batch()
    b.anchors(shuffled(xs, 50 + n_digits, 16, apart=(199, 197)))
    return _finish(b, [dict(n=200, tied_pairs=1)], route=lds_route(L, 200), top_digits=n_digits)


def closed_form(L, cycles, where="inner", n=200, b=None):
    """Two strands, n / 2 anchors each, one tie: places [0, n/2) are A (forward), [n/2, n) are B.  `cycles` places of A hold a reverse
    anchor and as many of B a forward one (64 and 65: the lists cross a 64-lane ballot).  where: "mid" -- place n/2 holds an A element,
    "end" -- place n - 1 does, "inner" -- neither."""
    half = n // 2
    assert cycles <= half - 2
    fwd = [anchor_x(3, 5 * j) for j in range(half)]
    rev = [anchor_x(3, 5 * j, 1) for j in range(half)]
    rev[-1] = rev[-2]                                                            # the tie
    a_places = list(range(1, 1 + cycles))                                        # places of A that hold a B element
    b_places = [half + 1 + j for j in range(cycles)]
    if cycles and where == "mid":
        b_places[0] = half
    if cycles and where == "end":
        b_places[-1] = n - 1
    xs = fwd + rev                                                               # x of the anchor at every place, before the swaps
    for pa, pb in zip(a_places, b_places):
        xs[pa], xs[pb] = xs[pb], xs[pa]
    per = 1                                                                      # the order of generation is the point: one hit a minimizer
    b = b or Batch()
    b.anchors(xs, per=per)
    return _finish(b, [dict(n=n, tied_pairs=1)], route=lds_route(L, n), cycles=cycles, a_at_mid=int(cycles > 0 and where == "mid"),
                   a_at_end=int(cycles > 0 and where == "end"))


def pair_ranges(pairs, groups, rev=0):
    """`pairs` tied pairs on `pairs` ids, `groups` values of id byte 1 with pairs / groups ids each: the pass at shift 40 leaves
    `groups` buckets, and the passes at shift 32 -- all in one round -- `pairs` ranges of two."""
    per = -(-pairs // groups)
    xs = []
    for i in range(pairs):
        xs += [anchor_x((i // per) << 8 | (i % per), 77, rev)] * 2
    return xs


def slot_overflow16(L, pairs=1030, b=None):
    """The sixteen-wave layout keeps 1024 slots for small ranges: 2 * pairs anchors, five buckets at shift 40 (each above 64 anchors),
    then `pairs` ranges of two from one round (1024: they just fit; 1025, 1030: the surplus is sorted by the lane that made it)."""
    xs = pair_ranges(pairs, 5)
    b = b or Batch()
    b.anchors(shuffled_pairs(xs[0::2], xs[1::2], [], pairs))
    return _finish(b, [dict(n=2 * pairs, tied_pairs=pairs)], route=lds_route(L, 2 * pairs), small_ranges_in_a_round=pairs, slots=1024)


def slot_overflow4(L, pairs=260, b=None):
    """The four-wave layout keeps 256 slots: a read of max_n + 1 anchors, `pairs` tied pairs on the forward strand (two buckets at
    shift 40, then `pairs` ranges of two from one round) and tie-free filler on the reverse strand."""
    n = L.max_n + 1
    assert n >= 2 * pairs + 66 and n <= cap_of(L)
    xs = pair_ranges(pairs, 2)
    b = b or Batch()
    b.anchors(shuffled_pairs(xs[0::2], xs[1::2], [anchor_x(0, j, 1) for j in range(n - 2 * pairs)], pairs))
    return _finish(b, [dict(n=n, tied_pairs=pairs)], route=lds_route(L, n), small_ranges_in_a_round=pairs, slots=256)


# ---------------------------------------------------------------- k_seed_sort_huge (CHAINDP_SEED_MAX_N=128,128, CHAINDP_SEED_LAB_CAP=1024)

def huge_level48(L, tie=False, b=None):
    """One strand; the pass at shift 48 leaves buckets of exactly 64 (sorted by its thread), 65 (a work item), min_n (a work item) and
    min_n + 1 (pushed on the stack; its pass at shift 40 leaves 65, an item, and min_n - 64 <= 64)."""
    m = cap_of(L)
    assert 65 < m <= 128
    xs = []
    for d, size in enumerate((64, 65, m, m + 1)):
        for j in range(size):
            xs.append(anchor_x(d << 16 | (1 if d == 3 and j < 65 else 0) << 8 | j % 67, 9 * j))
    if tie:
        xs[64 + 65 + 1] = xs[64 + 65]                                            # inside the bucket of min_n: that item is the tied unit
    n = len(xs)
    assert cap_of(L) < n <= huge_max(L) and n <= L.lab_cap
    b = b or Batch()
    b.anchors(shuffled(xs, 48, 16, apart=(64 + 65, 64 + 65 + 1)))
    return _finish(b, [dict(n=n, tied_pairs=int(tie))], route="huge", items=3, tied_units=int(tie))


def huge_edge(L, plus, tie=None, b=None):
    """SEED_HUGE_STACK x the LDS sort's limit anchors: the last read k_seed_sort_huge takes; one more goes to the one-thread kernel."""
    return sorted_read(L, huge_max(L) + plus, tie, b=b)


def huge_range(L, plus, strands=2, tie=False, b=None):
    """A read of n = lab_cap + plus anchors for k_seed_sort_huge around lab_cap: up to lab_cap the digits of a level stay in LDS, one more and they are
    packed eight to a word (n % 8 = 1, 2, 0 at lab_cap + 1, + 2, + 8).  strands = 1, one id: every level down to the positions is
    one bucket (the .y fields must be restored each time); strands = 2: a two-bucket level over global digits (the serial walk);
    strands = 0: one x for all n anchors, a minimizer each -- every level is one bucket, and after the last no pass rewrites the
    scratch copy, so what the restore of the .y fields leaves is the output."""
    n = L.lab_cap + plus
    assert cap_of(L) < n <= huge_max(L)
    if strands == 0:
        b = b or Batch()
        b.anchors([anchor_x(0x030201, 0x010203)] * n, per=1)
        return _finish(b, [dict(n=n, tied_pairs=n - 1)], route="huge", global_digits=int(n > L.lab_cap), strands=0)
    if strands == 1:
        xs = [anchor_x(0x030201, 3 * j) for j in range(n)]
    else:
        xs = sorted_xs(n)
    if tie:
        xs[n - 1] = xs[n - 2]
    b = b or Batch()
    b.anchors(shuffled(xs, n + strands, 16, apart=(n - 2, n - 1)))
    return _finish(b, [dict(n=n, tied_pairs=int(tie))], route="huge", global_digits=int(n > L.lab_cap), strands=strands)


# ---------------------------------------------------------------- probe, expand and reads kernels

def _plain_minis(b, count, q0=40, hits=(1, 2, 3)):
    """`count` fresh minimizers with 1, 2, 3, 1, .. hits on distinct ids."""
    out = []
    for j in range(count):
        h = hits[j % len(hits)]
        k = b.key([position(b._next * 4 + i + 1, 100 + 13 * j + i, (j + i) & 1) for i in range(h)])
        out.append((k, 10 + j % 19, q0 + 21 * j, j & 1))
    return out


BLOCK_LAYOUTS = {0: [0, 0, 0], 255: [0, 100, 0, 0, 0, 0, 0, 155, 0], 256: [0, 256, 0, 0], 257: [0, 256, 0, 0, 0, 1, 0],
                 600: [0, 256, 0, 100, 0, 0, 0, 0, 0, 0, 0, 156, 88, 0]}


def read_blocks(L, n_mini, b=None):
    """seed_read_of_block: reads laid out over the 256-minimizer blocks -- empty reads first and last, a read boundary exactly at
    256 (and 512), many empty reads inside one block, 0 / 255 / 256 / 257 minimizers in all (0: reads but no minimizer)."""
    b = b or Batch()
    b.key([position(1, 1)])                                                      # (an image is never empty)
    for size in BLOCK_LAYOUTS[n_mini]:
        b.read(_plain_minis(b, size), qlen=9000)
    return _finish(b, n_mini=n_mini, per_read=BLOCK_LAYOUTS[n_mini])


def tandem_boundary(L, across=True, b=None):
    """The tandem flag looks at the neighbouring minimizers of the same read only.  across: read 0 ends at minimizer 255 with the
    minimizer read 1 starts with at 256 (a read boundary on a block edge): neither is tandem.  not across: the equal neighbours are
    255 and 256 of one read: both are.  A second equal pair inside read 0 is tandem either way."""
    b = b or Batch()
    m = _plain_minis(b, 300, hits=(2, 1))
    m[256] = (m[255][0], 12, m[256][2], 0)                                        # the same minimizer value on both sides of 255 | 256
    m[21] = (m[20][0], 11, m[21][2], 1)
    if across:
        b.read(m[:256], qlen=9000)
        b.read(m[256:], qlen=9000)
    else:
        b.read(m[:3], qlen=9000)
        b.read(m[3:], qlen=9000)
    return _finish(b, across=across, equal_at=(255, 256), tandem_minis=2 if across else 4)


def occ_edges(L, b=None):
    """max_occ = M (8 in a batch of its own): minimizers with 0 (absent: used, a mini_pos entry, no anchor), 1 (stored in V), 2 (a list
    in P), M - 1 (used) and M, M + 1 hits (skipped); three minimizers of one bucket and one home slot, the third found after two
    collisions (in a batch of its own, where nothing else is in that bucket)."""
    b = b or Batch(max_occ=8)
    M = b.max_occ
    own, minis, hits = not b.shared, [], [0, 1, 2, M - 1, M, M + 1, 1, M - 1, M, 0, 2]
    for j, h in enumerate(hits):
        k = ABSENT + 1000 + j if h == 0 else b.key([position(50 + j, 10 * j + 3 * i, i & 1) for i in range(h)])
        minis.append((k, 14, 30 + 17 * j, j & 1))
    bucket = 0                                                                   # (empty but for these three: fewer than 64 other minimizers)
    coll = [b.key([position(70 + j, 5 * j + i) for i in range(1 + j)], at=(1 << 30 | j << 18 | 5) << b.b_bits | bucket) for j in range(3)]
    for j, k in enumerate(coll):
        minis.append((k, 14, 400 + 17 * j, 0))
    b.read(minis, qlen=2000)
    b.read(list(reversed(minis[:9])), qlen=2000)
    collisions = b.build()[1] if own else {}
    return _finish(b, hits=hits + [1, 2, 3], collisions=[collisions.get(k) for k in coll], max_occ=M)


def rep_len_chunks(L, b=None):
    """k_seed_reads, a wave per read, 64 minimizers a round: skipped minimizers (max_occ + 1 hits; max_occ = 4 in a batch of its own) at lane 63 of one chunk and lane
    0 of the next, chunks without any, a gap of two whole chunks, a pair with st == pe and one with st == pe + 1, and a first skipped
    minimizer whose interval starts below 0.  In a batch of its own the read starts at minimizer 10."""
    b = b or Batch(max_occ=4)
    M = b.max_occ
    heavy = [b.key([position(900 + t, 7 * i + t, i & 1) for i in range(M + 1)]) for t in range(3)]
    b.read(_plain_minis(b, 10), qlen=60000)
    minis = _plain_minis(b, 64 * 7 + 5, q0=3, hits=(1, 2))
    skipped = {}

    def skip(i, span):
        qpos = minis[i][2]
        minis[i] = (heavy[i % 3], span, qpos, i & 1)
        skipped[i] = (qpos + 1 - span, qpos + 1)                                  # (st, en)
    skip(0, 20)                                                                  # st = 3 + 1 - 20 < 0
    skip(63, 15); skip(64, 15)                                                   # lane 63, then lane 0 of the next chunk
    skip(65, 21)                                                                 # minimizers are 21 apart: st == en of the previous skipped one
    skip(66, 20)                                                                 # st == en + 1
    skip(64 * 4 + 31, 28)                                                        # after chunks 2 and 3 without a skipped minimizer
    skip(64 * 6 + 63, 28); skip(64 * 7, 28)                                      # lane 63 and lane 0 again, the last chunk a partial one
    r = b.read(minis, qlen=60000)
    b.read(_plain_minis(b, 3), qlen=60000)
    return _finish(b, read=r, skipped=skipped)


def scan_minis(L, n_mini, b=None):
    """launch_scan_u64 per minimizer: 1024 (one tile), 1025 (two), 1024 * 1024 + 1 (1025 tiles: the second level takes two tiles a
    thread).  The small ones have hits; the large one absent minimizers only, a read per 4096 of them: no anchors, a mini_pos entry
    per minimizer, so the scan of `used` is a scan of ones."""
    b = b or Batch()
    if n_mini <= 4096:
        sizes = [300, 0, n_mini - 300 - 1, 1]
        for s in sizes:
            b.read(_plain_minis(b, s), qlen=60000)
        return _finish(b, n_mini=n_mini, tiles=-(-n_mini // 1024))
    assert not b.shared
    b.key([position(1, 1)])
    c = b.case()
    i = np.arange(n_mini, dtype=np.uint64)
    mini = np.stack([(np.uint64(ABSENT) + i) << np.uint64(8) | (i % np.uint64(23) + np.uint64(5)), (i % np.uint64(4096) * np.uint64(9) + np.uint64(30)) << np.uint64(1)], 1)
    off = np.minimum(np.arange(0, n_mini + 4096, 4096, dtype=np.int64), n_mini)
    n_reads = len(off) - 1
    return (Case(c.image, 0, 64, off, mini, np.zeros(n_reads, np.uint32), np.full(n_reads, 60000, np.int32)),
            dict(n_mini=n_mini, tiles=-(-n_mini // 1024)))


SKIP_FLAGS = [F_NO_DIAG, F_NO_DIAG | F_NO_DUAL, F_NO_DUAL, F_FOR_ONLY, F_REV_ONLY, F_NO_DIAG | F_FOR_ONLY]


def skip_seed(L, flag, b=None):
    """skip_seed: hits whose id (rank) is one below, equal to and one above the read's bid, with and without bid's bit 31, at the
    query position and elsewhere, on both strands; a reverse-strand hit in a read so short that the 32-bit subtraction wraps."""
    b = b or Batch(flag=flag)
    assert b.flag == flag
    qpos = 500
    hits = [position(3, p, s, rank) for rank in (9, 10, 11) for p in (qpos, 800) for s in (0, 1)]
    k1, k2 = b.key(hits), b.key([position(4, qpos, 0, 10)])
    for bid in (10, 10 | 1 << 31, 9, 9 | 1 << 31, 11, 11 | 1 << 31):
        b.read([(k1, 15, qpos, 0), (k2, 15, qpos, 1), (k1, 15, qpos + 50, 1)], bid=bid, qlen=5000)
    b.read([(k1, 15, qpos, 0)], bid=10 | 1 << 31, qlen=5)                          # qlen - (q_pos + 1 - span) - 1 wraps
    return _finish(b, flag=flag, block_opens=bool(flag & 1))


# ---------------------------------------------------------------- many reads, and all of the small cases in one batch

def many_small(L, count=2100, b=None):
    """`count` reads of 2..5 anchors, every other one with a tie: more units than the per-read sort's grid has workgroups (2048) and
    more tied units than its second launch has (256), so a workgroup goes on to a second, third, .. unit."""
    b = b or Batch()
    reads = []
    for i in range(count):
        xs = sorted_xs(2 + i % 4)
        if i % 2 == 0:
            xs[1] = xs[0]
        b.anchors(xs[::-1], per=1)
        reads.append(dict(n=len(xs), tied_pairs=int(i % 2 == 0)))
    return _finish(b, reads, route="batch", units=count)


def small_cases(L, setting):
    """(constructor, args) of the cases that go into the combined batch of a limit setting: every case of the setting but the reads
    of thousands of anchors whose point is a size, and the cases that need a flag or a max_occ of their own (skip_seed)."""
    tied = ("sorted_read", 4096, "front")                                        # 256 minimizers: what follows starts on a block edge
    if setting == "default":
        c = [("tandem_boundary", True)]                                          # first: its read boundary stays on the block edge
        c += [("sorted_read", n, t) for n, t in ((1, None), (2, "end"), (63, None), (65, "front"), (129, None), (200, "end"), (1024, None), (1025, "mid"), (2048, None), (2049, "end"))]
        for sh in (48, 40, 32, 16, 8, 0):
            c += [("level_bucket", sh, 64), ("sorted_read", 63 + sh, None), ("level_bucket", sh, 65)]
        c += [("whole_small_read", n) for n in (2, 64, 65)] + [("top_digits", k) for k in (1, 2, 3)]
        c += [("closed_form", 0), ("closed_form", 1, "mid"), ("sorted_read", 300, None), ("closed_form", 1, "end"), ("closed_form", 64), ("closed_form", 65, "mid"), ("closed_form", 65, "end")]
        c += [("slot_overflow16", 1024), ("slot_overflow16", 1030), ("slot_overflow4",), ("read_blocks", 600), ("occ_edges",), ("rep_len_chunks",), ("scan_minis", 1025),
              ("many_small", 2100)]
    elif setting == "pair":
        c = [("sorted_read", n, t) for n in PAIR_SIZES for t in (None, "end")] + [("many_small", 300)]
    else:
        c = [("sorted_read", 129, None), ("sorted_read", 129, "end"), ("huge_level48", False), ("huge_level48", True)]
        c += [("huge_range", plus, 2, t) for plus in (0, 1, 2, 8) for t in (False, True)] + [("huge_range", 1, 1, True), ("huge_range", 0, 0, True), ("huge_range", 1, 0, True), ("many_small", 300)]
    return [tied] + c + [("sorted_read", 300, "front")]                           # tied reads first and last, tied and tie-free ones alternating between


def combined(L, setting):
    """All of small_cases(L, setting) as ONE batch over ONE image (flag 0, max_occ 64): every constructor adds its reads to the same
    Batch, so the reads that take the reference's procedure are some of many units of the second launch, the work items of
    k_seed_sort_huge come from several reads, and there are more units than workgroups.  props: per read n and tied_pairs (None for
    the reads that are not about the sort), parts = (constructor, args, first read, reads, what the constructor claimed)."""
    b = Batch()
    b.shared = True
    parts = []
    for name, *args in small_cases(L, setting):
        first = len(b.bid)
        globals()[name](L, *args, b=b)
        parts.append((name, tuple(args), first, len(b.bid) - first, b.parts[-1][1]))
    reads = [r for rs, _ in b.parts for r in rs]
    b.shared, b._mark = False, 0
    return _finish(b, reads, route="batch", parts=parts)
