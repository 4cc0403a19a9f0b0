"""The tile flush's v[] loop, restated in numpy, and the inputs its tests share.

The DP kernels work on units (a read's anchors, split where the gap in x exceeds max_dist_x: no chain crosses such a gap) in tiles of
64 anchors from the unit's start, one anchor per lane.  When a tile is finished they compute v[i] = max(f[i], v[p[i]]) (chain.c:284)
over it by pointer doubling: after r rounds a lane holds the maximum of f over itself and its first 2^r - 1 ancestors inside the tile,
with the final v of an ancestor in an earlier tile folded in at the start, and points at the ancestor behind those.  The loop has
three ways out:

  "none"    no lane's pointer is inside the tile (before round 1, or after a round that moved the last of them out);
  "quiet"   the round that was just started would raise no lane's value.  The values are final then: val[ptr] <= val wherever ptr is
            inside the tile, so lane by lane in tile order (p[i] < i) v[ptr] = val[ptr] by induction and v = max(val, v[ptr]) = val;
  "count"   six rounds have run (2^6 = 64 anchors: no pointer can still be inside the tile).

`flush_v` does exactly that, all tiles of a batch side by side, and says for each tile how many rounds it started and which way it
left; it uses its own v for the earlier tiles, never the oracle's."""
import numpy as np

from minimap2_chaindp_amd import anchorgen as ag, params as P

TILE = 64
ROUNDS = 6

# (generator, generator overrides, DP preset, reads): anchorgen.generate(..., seed=SEED)
SEED = 4321
SEEDED = [
    ("ava-ont", {}, "ava-ont", 200),
    ("ava-ont", dict(noise_pct=40, tie_pct=20), "ava-ont", 120),
    ("skew", dict(skew_max=30000), "ava-ont", 100),
    ("map-ont", {}, "map-ont", 60),
    ("ties", {}, "map-ont", 200),
]


def seeded(i):
    gen, over, preset, n_reads = SEEDED[i]
    off, a = ag.generate(gen, n_reads=n_reads, seed=SEED, **over)
    return P.preset(preset), off, a


def built_read(k, run, rid):
    """One read, one unit (ava-ont parameters, q_span 15): `run` anchors on one diagonal, 15 apart, so that f climbs by 15 an anchor
    up to a peak; one anchor that gains 1 (dq = 1) and pays the gap cost of a diagonal 480 away (bw = 500), so that its f falls well
    below the peak and stays above what a chain of its own would score; and 2^k anchors one base apart on that new diagonal (+1
    each), all of them below the peak.  Every anchor behind the peak has v = the peak's f, and the j-th of them is j ancestors
    away from it: its value rises in round ceil(log2(j + 1)), so the tile needs more rounds the longer the tail is."""
    q_span = 15
    xs = [1000 + 15 * i for i in range(run)]
    ys = [100 + 15 * i for i in range(run)]
    xs.append(xs[-1] + 481); ys.append(ys[-1] + 1)
    for _ in range(1 << k):
        xs.append(xs[-1] + 1); ys.append(ys[-1] + 1)
    a = np.empty((len(xs), 2), np.uint64)
    a[:, 0] = np.array(xs, np.uint64) | np.uint64(rid << 32)
    a[:, 1] = np.array(ys, np.uint64) | np.uint64(q_span << 32)
    return a


def built():
    """The hand-built reads as one batch.  run = 12: peak, fall and tail in the unit's first tile (a short one), the last rise in
    round 2, 2, 3, 4, 5, 6 for k = 0 .. 5.  run = 30: lanes with more than 32 ancestors in the tile, so that a sixth round starts
    (k = 4: it is quiet; k = 5: it still raises a value and the count ends the loop).  run = 64: the peak is the last anchor of the
    first tile, the fall and the tail open the second tile with a predecessor outside it whose v exceeds their f."""
    reads = [built_read(k, run, rid) for rid, (k, run) in enumerate([(0, 12), (1, 12), (2, 12), (3, 12), (4, 12), (5, 12),
                                                                     (4, 30), (3, 64), (5, 64), (5, 30)])]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return P.preset("ava-ont"), off, np.ascontiguousarray(np.concatenate(reads))


def unit_starts(par, off, a):
    """bool[n]: the anchor opens a unit (a read's first anchor, or a gap in x above max_dist_x: chain.c:252)."""
    n = int(off[-1])
    first = np.zeros(n, bool)
    first[off[:-1][off[:-1] < n]] = True
    x = a[:n, 0]
    first[1:] |= (x[1:] - x[:-1]) > np.uint64(par.max_dist_x)          # (x is sorted within a read; across reads `first` is set already)
    return first


def flush_v(par, off, a, f, p):
    """The flush's v of every anchor from f and the read-relative p, with per tile: anchors, anchors of its unit, rounds started, the
    way out, whether a lane's predecessor in an earlier tile had a v above the lane's f.  Returns (v, dict of per-tile arrays)."""
    n = int(off[-1])
    idx = np.arange(n, dtype=np.int64)
    read_of = np.searchsorted(off, idx, side="right") - 1
    gp = np.where(p >= 0, p.astype(np.int64) + off[read_of], -1)           # predecessor as a batch index
    first = unit_starts(par, off, a)
    ustart = np.maximum.accumulate(np.where(first, idx, 0))
    rank = (idx - ustart) // TILE                                          # the tile's number within its unit
    tstart = ustart + rank * TILE                                          # first anchor of the lane's tile
    new_tile = np.ones(n, bool)
    new_tile[1:] = tstart[1:] != tstart[:-1]
    tile_of = np.cumsum(new_tile) - 1
    n_tiles = int(tile_of[-1]) + 1 if n else 0
    assert (gp < idx).all() and (gp[gp >= 0] >= ustart[gp >= 0]).all()     # p[i] < i, and inside the unit

    v = np.zeros(n, np.int64)
    rounds = np.zeros(n_tiles, np.int64)
    way = np.full(n_tiles, "", dtype=object)
    ext_above = np.zeros(n_tiles, bool)
    for k in range(int(rank.max()) + 1 if n else 0):                       # tiles in unit order: earlier tiles' v are final
        lanes = np.flatnonzero(rank == k)
        t = tile_of[lanes]
        val = f[lanes].astype(np.int64)
        ptr = gp[lanes].copy()
        ext = (ptr >= 0) & (ptr < tstart[lanes])
        vext = v[np.where(ext, ptr, 0)]
        np.logical_or.at(ext_above, t[ext & (vext > val)], True)
        val = np.where(ext, np.maximum(val, vext), val)
        ptr[ext] = -1
        live = np.ones(len(lanes), bool)                                   # lanes of tiles still in the loop
        for r in range(1, ROUNDS + 1):
            inside = live & (ptr >= tstart[lanes])
            any_in = np.zeros(n_tiles, bool)
            np.logical_or.at(any_in, t[inside], True)
            left = live & ~any_in[t]
            way[np.unique(t[left])] = "none"
            live &= any_in[t]
            if not live.any():
                break
            inside &= live
            rounds[np.unique(t[live])] = r
            src = np.searchsorted(lanes, np.where(inside, ptr, lanes))     # (ds_bpermute's source lane) lanes with no pointer in the tile read themselves
            pv, pp = val[src], ptr[src]
            rises = np.zeros(n_tiles, bool)
            np.logical_or.at(rises, t[live & (pv > val)], True)
            quiet = live & ~rises[t]
            way[np.unique(t[quiet])] = "quiet"
            live &= rises[t]
            val = np.where(live, np.maximum(val, pv), val)
            ptr = np.where(live, pp, ptr)
        way[np.unique(t[live])] = "count"
        v[lanes] = val
    cnt = np.bincount(tile_of, minlength=n_tiles)
    unit_len = np.bincount(np.cumsum(first) - 1)[np.cumsum(first) - 1]     # anchors of the lane's unit
    return v.astype(np.int32), dict(tile_of=tile_of, anchors=cnt, unit_len=unit_len[new_tile], rounds=rounds, way=way, ext_above=ext_above)
