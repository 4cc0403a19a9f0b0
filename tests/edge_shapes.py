"""Inputs that sit exactly on the constants which route a read or a unit to one kernel or another (numpy only).

Every constructor returns the batch -- (par, off, a) or (par, off, a, min_cnt) -- and a dict of the properties it claims,
e.g. {"records": 10113, "ends": 257, "kept": 65}.  tests/test_edge_shapes_cpu.py proves every claim with the oracle,
tests/test_gpu_edges.py runs the batches on the GPU.  A constructor that cannot reach its edge raises: it never falls back
to a nearby size.  An anchor is (x, y) = (rid << 32 | ref pos, q_span << 32 | query pos), sorted by x within a read."""
import numpy as np

from minimap2_chaindp_amd import params as P

# the constants the shapes sit on (csrc/chaindp_bottom.hip, chaindp_kernels.h, chaindp_fast.h, chaindp_twin.hip)
BT_LDS_RECS, BT_LDS_RECS_MAX = 10112, 20000
BT_INSERTION_MAX = 64                    # kept chains: insertion sort up to here, the reference's radix sort above
DENSE_BITCAP, DENSE_UNITS, DENSE16_MAX_UNITS, DEEP_HANDOVER_LEFT = 65536, 2048, 256, 2048
LUT_MAX_BW, TWIN_LUT_BYTES, SHORT_UNIT_AVG = 4095, 512, 512
TILE, BLOCK = 64, 1024


def anchors(x, q, span=15):
    x = np.asarray(x, np.uint64)
    q = np.asarray(q, np.uint64)
    s = np.broadcast_to(np.asarray(span, np.uint64), q.shape)
    return np.stack([x, (s << np.uint64(32)) | q], 1)


def batch(reads):
    """reads: list of uint64[n, 2] -> (off int64[n_reads + 1], a uint64[total, 2])."""
    off = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.int64)
    a = np.concatenate([r.reshape(-1, 2) for r in reads] + [np.zeros((0, 2), np.uint64)]).astype(np.uint64)
    return off, np.ascontiguousarray(a)


def sort_read(a):
    return np.ascontiguousarray(a[np.lexsort((a[:, 1], a[:, 0]))])


def unit_lengths(par, off, a):
    """Lengths of the units (maximal runs of a read whose consecutive x are at most max_dist_x apart; length 1: a singleton)
    and the batch position of each unit's first anchor."""
    x = a[:, 0]
    start = np.ones(len(x), bool)
    if len(x) > 1:
        start[1:] = (x[1:] - x[:-1]) > np.uint64(par.max_dist_x)       # unsigned 64-bit, as chain.c:252
    start[off[:-1][off[:-1] < len(x)]] = True
    pos = np.flatnonzero(start)
    return np.diff(np.concatenate((pos, [len(x)]))), pos


def colinear(n, x0, q0, step=9, span=15):
    k = np.arange(n, dtype=np.int64)
    return anchors(x0 + step * k, q0 + step * k, span)


def small_units(rng, n_units, mdx, x0=1000, q0=1000, lo=2, hi=60, step=9, span=15):
    """One read of n_units colinear units of lo..hi anchors, more than max_dist_x apart: nothing but the tested condition
    hands any of them over."""
    parts, x, q = [], x0, q0
    for L in rng.integers(lo, hi + 1, n_units):
        parts.append(colinear(int(L), x, q, step, span))
        x += step * int(L) + mdx + 1000
        q += step * int(L) + 50
    return np.concatenate(parts)


# ---------------------------------------------------------------- backtracker

BT_PAR = dict(min_sc=10, max_dist_y=50, max_dist_x=5000)
BT_MIN_CNT = 2
FORK_TRUNK, FORK_MAIN, FORK_KEPT, FORK_DROPPED = 25, 30, 25, 8
# (records, ends, kept chains): both sides of 10112 and of 20000 records, 64 and 65 kept chains in each of the three regimes,
# 256 / 257 and 1024 / 1025 ends (k_bt_rank: rounds of 256 keys over tiles of 1024)
BT_EDGES = [
    (10112, 256, 64), (10112, 257, 65), (700, 256, 65),
    (10113, 257, 65), (10113, 1024, 64), (20000, 1025, 64), (20000, 1024, 65),
    (20001, 1025, 65), (20001, 65, 64), (20001, 1024, 64),
]


def _fork(x0, q0, n_branch):
    """A trunk of 25 anchors, a branch of 30 that continues it and a second branch of n_branch anchors that starts at (+10, +40)
    behind the trunk with steps (9, 49): a step of the second branch gains 1 (9 - (int(40 * .01 * 15) + (5 >> 1))), so 25
    anchors make a chain that stops at the older one and 8 anchors gain less than min_sc."""
    main = colinear(FORK_TRUNK + FORK_MAIN, x0, q0)
    xt, qt = x0 + 9 * (FORK_TRUNK - 1), q0 + 9 * (FORK_TRUNK - 1)
    k = np.arange(n_branch, dtype=np.int64)
    return np.concatenate([main, anchors(xt + 10 + 9 * k, qt + 40 + 49 * k)])


def bt_read(records, ends, kept, share=4):
    """One read in which every anchor becomes a record: `kept` chains survive min_cnt = 2 (two of them from the forks: the
    main chain and the second branch that stopped at it; a third fork's second branch is dropped by min_sc), the other ends
    are one-anchor runs.  `share` consecutive runs start at the same x, 50000 apart in q."""
    n_fork = 2 * (FORK_TRUNK + FORK_MAIN) + FORK_KEPT + FORK_DROPPED
    n_long = kept - 3
    n_single = ends - 4 - n_long
    n_long_anchors = records - n_fork - n_single
    if n_long < share or n_single < 0 or n_long_anchors < 2 * n_long:
        raise ValueError(f"no read with {records} records, {ends} ends and {kept} kept chains")
    lens = [n_long_anchors // n_long + (1 if i < n_long_anchors % n_long else 0) for i in range(n_long)] + [1] * n_single
    parts = []
    for i, L in enumerate(lens):
        parts.append(colinear(L, 1000 + 100_000 * (i // share), 1000 + 50_000 * (i % share)))
    g = (len(lens) + share - 1) // share
    parts.append(_fork(1000 + 100_000 * g, 1000, FORK_KEPT))
    parts.append(_fork(1000 + 100_000 * (g + 1), 1000, FORK_DROPPED))
    a = sort_read(np.concatenate(parts))
    assert len(a) == records
    return a, dict(records=records, ends=ends, kept=kept, shared_first_x=min(share, n_long))


def bt_par():
    return P.preset("map-ont", **BT_PAR)


def bt_single_reads():
    """[(par, off, a, min_cnt), props] for every edge read on its own."""
    out = []
    for rec, ends, kept in BT_EDGES:
        a, props = bt_read(rec, ends, kept)
        off, a = batch([a])
        out.append(((bt_par(), off, a, BT_MIN_CNT), props))
    return out


def bt_combined():
    """All edge reads in one call (the three record regimes share the scratch arrays), between reads without anchors and
    without records; then a 1024-record block that spans three reads and an empty one, the first of them starting at a
    multiple of 1024 records."""
    empty = np.zeros((0, 2), np.uint64)
    norec = anchors(1000 + 20_000 * np.arange(5), 1000 + 20 * np.arange(5), span=5)    # five singletons with span 5 < min_sc
    reads, rec, edge_at = [empty], [0], {}
    for i, (r, e, k) in enumerate(BT_EDGES):
        if i == 3:
            reads += [empty, empty]; rec += [0, 0]
        if i == 6:
            reads.append(norec); rec.append(0)
        edge_at[len(reads)] = i
        reads.append(bt_read(r, e, k)[0]); rec.append(r)
    pad = -sum(rec) % BLOCK
    if pad:
        reads.append(colinear(pad, 1000, 1000)); rec.append(pad)
    aligned = len(reads)
    for n in (300, 0, 300, 500):
        reads.append(colinear(n, 1000, 1000) if n else empty); rec.append(n)
    reads += [empty, empty]; rec += [0, 0]
    off, a = batch(reads)
    props = dict(records=rec, edge_at=edge_at, aligned_read=aligned, block_reads=[aligned, aligned + 1, aligned + 2, aligned + 3],
                 empty_middle=(4, 5), norec_read=next(i for i, r in enumerate(reads) if r is norec))
    return (bt_par(), off, a, BT_MIN_CNT), props


def bt_other_batch():
    """A different batch for the same context (what it leaves in the scratch arrays is stale for the next call)."""
    rng = np.random.default_rng(17)
    reads = [bt_read(3000, 300, 40)[0], small_units(rng, 50, 5000), bt_read(12000, 90, 80)[0]]
    off, a = batch(reads)
    return (bt_par(), off, a, BT_MIN_CNT), {}


# ---------------------------------------------------------------- DP routing

def lut_last_entry(bw, spans):
    """The last entry of a read's cost table, 1 - cost(bw), with the operations of k_build_lut and k_unit_scatter: an f32 divide
    of the span sum by the anchor count (chain.c:241), then f64."""
    avg = np.float32(np.uint64(int(np.sum(spans)))) / np.float32(len(spans))
    assert avg.dtype == np.float32
    lg = int(bw).bit_length() - 1 if bw else 0
    return 1 - (int(np.float64(bw) * .01 * np.float64(avg)) + (lg >> 1))


def int8_batches(n_reads=6, n_units=40):
    """bw = 500: a read whose spans are all 25 has the last table entry -128 (fits a signed byte: k_chain_twin keeps it), a
    read with spans 25, 25, 25, 25, 26 repeated has -129 (handed over).  Three batches: fitting, non-fitting, mixed."""
    par = P.preset("map-ont", bw=500)
    rng = np.random.default_rng(8)

    def read(fit):
        a = small_units(rng, n_units, par.max_dist_x, span=25)
        a = a[:len(a) - len(a) % 5] if len(a) % 5 else a
        if unit_lengths(par, np.array([0, len(a)]), a)[0][-1] < 2:
            a = a[:-5]
        if not fit:
            a[4::5, 1] += np.uint64(1 << 32)
        spans = (a[:, 1] >> np.uint64(32)).astype(np.int64)
        entry = lut_last_entry(par.bw, spans)
        assert entry == (-128 if fit else -129), entry
        return a

    out = {}
    for name, fits in (("fit", [True] * n_reads), ("nofit", [False] * n_reads), ("mixed", [i % 2 == 0 for i in range(n_reads)])):
        reads = [read(f) for f in fits]
        off, a = batch(reads)
        lens = [unit_lengths(par, np.array([0, len(r)]), r)[0] for r in reads]
        assert all((l >= 2).all() for l in lens)
        out[name] = ((par, off, a), dict(fits=fits, units=[len(l) for l in lens], last_entry=[-128 if f else -129 for f in fits],
                                         units_nofit=sum(len(l) for l, f in zip(lens, fits) if not f)))
    return out


def bw_batch(bw, span, run):
    """Two units that end in a jump with |dr - dq| = bw (chains, chain.c:260) and = bw + 1 (cannot), then small units.  The run
    before the jump has steps and spans of `span`, long enough for its score to outweigh the jump's cost."""
    par = P.preset("map-ont", bw=bw)
    rng = np.random.default_rng(bw)
    cost = int(bw * .01 * span) + ((bw.bit_length() - 1) >> 1)
    if span * run <= cost + span:
        raise ValueError("the run before the jump scores too little to chain over it")
    parts, jumps, x, n = [], [], 1000, 0
    for dd in (bw, bw + 1):
        r = colinear(run, x, 1000, step=span, span=span)
        xl, ql = x + span * (run - 1), 1000 + span * (run - 1)
        if 200 + dd > par.max_dist_x:
            raise ValueError("jump out of the window")
        parts += [r, anchors([xl + 200 + dd], [ql + 200], span)]
        jumps.append(dict(anchor=n + run, pred=n + run - 1, dd=dd, chains=dd <= bw))
        n += run + 1
        x = xl + 200 + dd + par.max_dist_x + 1000
    parts.append(small_units(rng, 30, par.max_dist_x, x0=x, q0=50_000, span=span, step=min(span, 9)))
    off, a = batch([np.concatenate(parts)])
    return (par, off, a), dict(bw=bw, jumps=jumps, units=int((unit_lengths(par, off, a)[0] >= 2).sum()))


def largest_mdx(factor, bits):
    """The largest max_dist_x with (max_dist_x + 1) * factor < 2^bits (the kernels' 32-bit exactness bounds)."""
    m = ((1 << bits) - 1) // factor - 1
    assert (m + 1) * factor < (1 << bits) <= (m + 2) * factor
    return m


def mdx_twin_batch(mdx):
    """k_chain_twin's bound 129 * (max_dist_x + 1) < 2^31.  One unit whose gaps are exactly max_dist_x, max_dist_x - 1 and small,
    q following x within bw so that pairs chain across the large gaps; a gap of max_dist_x + 1 splits a second unit off."""
    par = P.preset("map-ont", max_dist_x=mdx, max_dist_y=mdx, bw=500)
    rng = np.random.default_rng(3)
    gx, gq = [], []
    for k in range(60):
        for g in (mdx if k % 2 == 0 else mdx - 1, 9, 7, 9):
            gx.append(g); gq.append(g - (2 if len(gx) % 2 else -2) if g > 100 else g)
    x = 1000 + np.concatenate(([0], np.cumsum(gx)))
    q = 1000 + np.concatenate(([0], np.cumsum(gq)))
    assert q[-1] < (1 << 31) and x[-1] < (1 << 32)
    first = anchors(x, q)
    second = colinear(30, int(x[-1]) + mdx + 1, int(q[-1]) + 9)
    rest = small_units(rng, 12, mdx, x0=int(second[-1, 0]) + mdx + 1000, q0=int(q[-1]) + 1000)
    off, a = batch([np.concatenate([first, second, rest])])
    assert int(a[-1, 1] & np.uint64(0xffffffff)) < (1 << 31)
    lens, _ = unit_lengths(par, off, a)
    return (par, off, a), dict(mdx=mdx, first_units=[len(first), len(second)], units=int((lens >= 2).sum()), large_gaps=60)


def mdx_ring_batch(mdx, ring, dense_head=0):
    """The ring bounds (max_dist_x + 1) * (ring + 1) < 2^32.  One unit: (dense_head anchors with deep scans, for the dense
    hand-over,) ring + 8 anchors with gaps of exactly max_dist_x and max_dist_x - 1 -- the ring then spans all but 2^32, and x
    runs past 2^32 --, then clusters that chain inside; a gap of max_dist_x + 1 splits a second unit off.  q cannot follow x
    (31 bits): pairs chain inside the head and the clusters only."""
    par = P.preset("ava-ont", max_dist_x=mdx)
    rng = np.random.default_rng(ring)
    parts, x, q = [], (1 << 32) - 3 * mdx - 50, 1000
    if dense_head:
        d = dense_unit(rng, dense_head, x0=x, q0=q)
        parts.append(d)
        x, q = int(d[-1, 0]) + mdx, 600_000
    n = ring + 8
    gaps = np.where(np.arange(n) % 3 == 2, mdx - 1, mdx)
    sx = x + np.concatenate(([0], np.cumsum(gaps[:-1])))
    parts.append(anchors(sx, q + 9 * np.arange(n)))
    x, q = int(sx[-1]), q + 9 * n
    for L in rng.integers(2, 60, 10):
        x += mdx if L % 2 else 200
        parts.append(colinear(int(L), x, q)); x += 9 * (int(L) - 1); q += 9 * int(L) + 600
    first = np.concatenate(parts)
    second = colinear(40, x + mdx + 1, q)
    off, a = batch([np.concatenate([first, second])])
    assert a[0, 0] < (1 << 32) <= a[-1, 0]
    lens, _ = unit_lengths(par, off, a)
    assert list(lens) == [len(first), len(second)]
    return (par, off, a), dict(mdx=mdx, ring=ring, unit_lens=[len(first), len(second)], units=2)


def short_units_batches():
    """k_chain_twin takes a batch whose units have at most 512 anchors on average: (total - singletons) == 512 * units, and one
    anchor more."""
    par = P.preset("map-ont")
    out = {}
    for name, extra in (("equal", 0), ("above", 1)):
        lens = [512 * 4 - 3 * 60 + extra, 60, 60, 60]
        parts, x = [], 1000
        for i, L in enumerate(lens):
            parts.append(colinear(L, x, 1000 + 9 * i)); x += 9 * L + par.max_dist_x + 1
            parts.append(anchors([x], [500])); x += par.max_dist_x + 1                  # a singleton between the units
        off, a = batch([np.concatenate(parts)])
        out[name] = ((par, off, a), dict(units=4, singletons=4, total=len(a)))
        assert (len(a) - 4 == SHORT_UNIT_AVG * 4) == (extra == 0)
    return out


def dense_unit(rng, n, x0=1000, q0=1000):
    """n anchors with x gaps 1..9 and q a random walk of such steps plus one of 12 offsets 40000 apart: under max_dist_x = 1000
    the window holds about 200 predecessors, one in twelve of them chains, and the scans run to the window's end."""
    x = x0 + np.cumsum(rng.integers(1, 10, n))
    q = q0 + np.cumsum(rng.integers(1, 10, n)) + 40_000 * rng.integers(0, 12, n)
    return anchors(x, q)


def dense_par():
    return P.preset("ava-ont", max_dist_x=1000)


def dense_bitmap_batch(n):
    """One unit of n anchors (65536: handed to the dense kernel; 65537: more distances than its mark bitmap has bits)."""
    off, a = batch([dense_unit(np.random.default_rng(65536), n)])
    par = dense_par()
    lens, _ = unit_lengths(par, off, a)
    assert list(lens) == [n]
    return (par, off, a), dict(unit_lens=[n], units=1)


def dense_units_batch(n_units, unit_len, per_read):
    """n_units dense units of unit_len anchors, 5000 apart in x, per_read of them in a read."""
    rng = np.random.default_rng(n_units)
    par = dense_par()
    reads = []
    for u0 in range(0, n_units, per_read):
        parts, x = [], 1000
        for _ in range(min(per_read, n_units - u0)):
            d = dense_unit(rng, unit_len, x0=x)
            parts.append(d); x = int(d[-1, 0]) + 5000
        reads.append(np.concatenate(parts))
    off, a = batch(reads)
    lens, _ = unit_lengths(par, off, a)
    assert len(lens) == n_units and (lens == unit_len).all()
    return (par, off, a), dict(units=n_units, unit_len=unit_len)


# ---------------------------------------------------------------- alignment

ALIGN_PAR = dict(min_sc=10)


def _read_of(n, k):
    """A read of n anchors: colinear, every 13th gap beyond max_dist_x (several units), every 29th anchor a singleton."""
    if n == 0:
        return np.zeros((0, 2), np.uint64)
    i = np.arange(n)
    gaps = np.where(i % 13 == 12, 6000, 9)
    gaps = np.where((i % 29 == 28) | (i % 29 == 0), 7000, gaps)
    x = 1000 + k % 7 + np.concatenate(([0], np.cumsum(gaps[1:])))
    return anchors(x, 1000 + 9 * i)


def confetti_batch(block_multiple=False):
    """Thousands of reads of 0..3 anchors around a few of 60..70 and 1020..1030, their lengths chosen so that reads start on
    lanes 0, 1 and 63 of a 64-anchor tile and on the first and last anchor of a 1024-anchor block, one-anchor reads sit on
    those places, a tile holds dozens of read boundaries, a block hundreds of reads, 75 empty reads follow each other, and the
    batch ends with a tile of one anchor (or, block_multiple, on a block boundary)."""
    lens = []
    g = 0
    cyc = [1, 0, 2, 1, 3, 0, 1, 1]

    def emit(n):
        nonlocal g
        lens.append(n); g += n

    def fill_to(target):
        k = 0
        while g < target:
            emit(min(cyc[k % len(cyc)], target - g)); k += 1

    emit(0)
    emit(1)                      # a one-anchor read on lane 0 of a tile and on the first anchor of a block
    emit(62)                     # starts on lane 1
    emit(1)                      # lane 63
    emit(65)                     # starts on lane 0
    fill_to(BLOCK - 1)
    emit(1)                      # the last anchor of a block
    emit(1025)                   # starts on a block's first anchor
    fill_to(3 * BLOCK - 1)
    emit(1021)                   # starts on a block's last anchor
    for _ in range(75):
        emit(0)
    fill_to(g + 700)
    emit(70)
    fill_to(g + 800)
    emit(63); emit(1030); emit(60)
    fill_to(g + 1200)
    if block_multiple:
        fill_to((g + BLOCK - 1) // BLOCK * BLOCK)
    else:
        fill_to((g + TILE - 1) // TILE * TILE)
        emit(1)                  # a last tile of one anchor
    reads = [_read_of(n, k) for k, n in enumerate(lens)]
    off, a = batch(reads)
    par = P.preset("map-ont", **ALIGN_PAR)
    ln, st = np.diff(off), off[:-1]
    one = st[ln == 1]
    nz = st[ln > 0]
    props = dict(
        n_reads=len(lens), total=int(off[-1]),
        starts_lane={m: int((nz % TILE == m).sum()) for m in (0, 1, 63)},
        starts_block={m: int((nz % BLOCK == m).sum()) for m in (0, BLOCK - 1)},
        one_anchor={"lane0": int((one % TILE == 0).sum()), "lane63": int((one % TILE == 63).sum()),
                    "block_first": int((one % BLOCK == 0).sum()), "block_last": int((one % BLOCK == BLOCK - 1).sum())},
        max_boundaries_in_tile=int(np.bincount(st[1:] // TILE).max()),
        max_reads_in_block=int(np.bincount(nz // BLOCK).max()),
        longest_empty_run=int(max(len(s) for s in "".join("e" if n == 0 else " " for n in lens).split())),
        last_tile=int(off[-1] % TILE), mid_reads=int(((ln >= 60) & (ln <= 70)).sum()), long_reads=int(((ln >= 1020) & (ln <= 1030)).sum()),
    )
    return (par, off, a, 1), props


def adjacent_reads_batch():
    """Neighbouring reads whose x ranges touch: the first x of read 1 is within max_dist_x of read 0's last x and colinear with it
    (one unit if the boundary were missed), read 2 starts below read 1's last x, read 4 follows an empty read in reach."""
    par = P.preset("map-ont", **ALIGN_PAR)
    r0 = colinear(40, 1000, 1000)
    r1 = colinear(30, int(r0[-1, 0]) + 9, int(r0[-1, 1] & np.uint64(0xffffffff)) + 9)
    r2 = colinear(70, int(r1[-1, 0]) - 100, 5000)
    r4 = colinear(1, int(r2[-1, 0]) + 9, 5000 + 9 * 70)
    off, a = batch([r0, r1, r2, np.zeros((0, 2), np.uint64), r4])
    return (par, off, a, 1), dict(unit_lens=[40, 30, 70, 1], within=(0, 1), below=(1, 2))


UNIT_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def unit_lengths_batch():
    """Units of 1, 2, 31 .. 129 anchors, each once with its first anchor on lane 0 of a 64-anchor tile and once on lane 63 (filler
    units pad in between), in one read."""
    par = P.preset("map-ont", **ALIGN_PAR)
    parts, placed, g, x = [], [], 0, 1000

    def unit(n):
        nonlocal g, x
        parts.append(colinear(n, x, 1000 + g)); x += 9 * n + par.max_dist_x + 1; g += n

    for L in UNIT_LENGTHS:
        for lane in (0, 63):
            pad = (lane - g) % TILE
            if pad:
                unit(pad)
            placed.append((g, L)); unit(L)
    off, a = batch([np.concatenate(parts)])
    return (par, off, a, 1), dict(placed=placed)
