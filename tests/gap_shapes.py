"""CHECKER ONLY: anchor batches whose reads carry their own chaining gaps (chaindp_set_read_gaps), numpy only.

Every constructor returns a Shape: the batch (par, off, a, n_segs or None) and one (gap_ref, gap_qry) pair per read, empty reads
included.  The anchors of a read sit exactly on its own gaps -- a distance of g and of g + 1 under gap g -- and its neighbours in the
batch carry other gaps, so that a kernel which takes a gap from the wrong read (the one before, the one behind, the batch's) cuts,
filters or routes differently.  tests/test_gap_shapes_cpu.py proves that with the oracle, tests/test_gpu_read_gaps.py runs the batches
on the GPU.  An anchor is (x, y) = (ref pos, seg << 48 | q_span << 32 | query pos), sorted by x within a read."""
import types

import numpy as np

import oracle_lib as ol
from minimap2_chaindp_amd import params as P

TILE, BLOCK = 64, 1024
EMPTY_GAP = (7, 3)                       # what an empty read carries: no read of any shape has these


def anchors(x, q, span=15, seg=0):
    x, q = np.asarray(x, np.uint64), np.asarray(q, np.uint64)
    s = np.broadcast_to(np.asarray(span, np.uint64), q.shape)
    g = np.broadcast_to(np.asarray(seg, np.uint64), q.shape)
    return np.stack([x, g << np.uint64(48) | s << np.uint64(32) | q], 1)


def walk(dx, dq=None, x0=1000, q0=1000, span=15):
    """Anchors at the running sums of the steps dx (reference) and dq (query; None: the same steps, a diagonal)."""
    dx = np.asarray(dx, np.int64)
    dq = dx if dq is None else np.asarray(dq, np.int64)
    return anchors(x0 + np.concatenate(([0], np.cumsum(dx))), q0 + np.concatenate(([0], np.cumsum(dq))), span)


def pack(name, par, reads, gaps, n_segs=None, **claims):
    """reads: list of uint64[n, 2] (or None: an empty read, which gets EMPTY_GAP); gaps: one pair per non-empty read."""
    rs, gs, it = [], [], iter(gaps)
    for r in reads:
        rs.append(np.zeros((0, 2), np.uint64) if r is None else np.asarray(r, np.uint64).reshape(-1, 2))
        gs.append(EMPTY_GAP if r is None else next(it))
    assert next(it, None) is None, "one gap pair per non-empty read"
    off = np.concatenate(([0], np.cumsum([len(r) for r in rs]))).astype(np.int64)
    a = np.ascontiguousarray(np.concatenate(rs + [np.zeros((0, 2), np.uint64)]).astype(np.uint64))
    g = np.array(gs, np.int64).reshape(-1, 2)
    return types.SimpleNamespace(name=name, par=par, off=off, a=a, n_segs=None if n_segs is None else np.asarray(n_segs, np.int32),
                                 gap_ref=g[:, 0].astype(np.int32), gap_qry=g[:, 1].astype(np.int32), claims=claims)


def par1(**over):
    """`sr` chaining parameters for reads of one segment; the gaps are placeholders no read of a shape carries."""
    return P.preset("sr", **{**dict(n_segs=1, max_dist_x=11, max_dist_y=13), **over})


# ---- the oracle, read by read ----------------------------------------------------------------------------------------------------------

def read_par(par, gap_ref, gap_qry, n_segs=None):
    p = ol.CoParams(*[getattr(par, k) for k, _ in ol.CoParams._fields_])
    p.max_dist_x, p.max_dist_y = int(gap_ref), int(gap_qry)
    if n_segs is not None:
        p.n_segs = int(n_segs)
    return p


def expected(sh, gap_ref=None, gap_qry=None, use_ref=False):
    """f, p, v of the batch and new_seed[] per read (seeds_off, seeds) with read r chained under its own gaps -- by oracle_fpv /
    oracle_compact, or (use_ref) by the compiled reference's mm_chain_dp_fpga."""
    gr = sh.gap_ref if gap_ref is None else gap_ref
    gq = sh.gap_qry if gap_qry is None else gap_qry
    F, Pp, V, S = [], [], [], []
    for r in range(len(sh.off) - 1):
        a = np.ascontiguousarray(sh.a[sh.off[r]:sh.off[r + 1]])
        pr = read_par(sh.par, gr[r], gq[r], None if sh.n_segs is None else sh.n_segs[r])
        if use_ref:
            f, p, v, seeds = ol.ref_fpv_seeds(pr, a) if len(a) else (np.zeros(0, np.int32),) * 3 + (np.zeros(0, ol.SEED_DTYPE),)
        else:
            f, p, v, _ = ol.oracle_fpv(pr, a)
            seeds = ol.oracle_compact(pr, a, f.copy(), p.copy(), v.copy())
        F.append(f.copy()); Pp.append(p.copy()); V.append(v.copy()); S.append(seeds)
    cat = lambda xs, dt: np.concatenate(xs + [np.zeros(0, dt)]).astype(dt)
    soff = np.concatenate(([0], np.cumsum([len(s) for s in S]))).astype(np.int64)
    return cat(F, np.int32), cat(Pp, np.int32), cat(V, np.int32), soff, cat(S, ol.SEED_DTYPE)


def neighbours(sh, k):
    """The gaps with every read taking those of the read k places on (k = 1, -1), empty reads counted."""
    return np.roll(sh.gap_ref, -k), np.roll(sh.gap_qry, -k)


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------

CUT_GAPS = (1, 100, 499, 500, 740)


def cut_edge():
    """chain.c:252: consecutive anchors exactly g and g + 1 apart, the same anchors under gap g - 1, g and g + 1 side by side, in both
    orders.  Under g the read is cut behind every second anchor, under g + 1 nowhere, under g - 1 everywhere (g = 1: gap 0)."""
    reads, gaps = [], []
    for g in CUT_GAPS:
        a = walk([g, g + 1, g, g + 1, g, g, g + 1])
        for own in (g, g + 1, g - 1, g + 1, g):
            reads.append(a.copy()); gaps.append((own, 2000))
    return pack("cut_edge", par1(bw=100), reads, gaps)


def singletons():
    """Anchors that are singletons under their read's gap and chain under the neighbour's, and the reverse; q_span on both sides of
    min_sc (25), so that some singletons are emitted and some are not; singletons and units in one read."""
    s = 300
    lone = walk([s] * 9, span=[15, 30] * 5)                          # every step s: all alone under s - 1, one unit under s
    mixed = walk([s, 5, 5, s, s, 7, s], span=[30, 15, 15, 15, 30, 15, 15, 30])
    reads = [lone, lone.copy(), mixed, mixed.copy(), lone.copy(), None, mixed.copy()]
    gaps = [(s - 1, 2000), (s, 2000), (s, 2000), (s - 1, 2000), (s, 2000), (s - 1, 2000)]
    return pack("singletons", par1(bw=100), reads, gaps)


GEOMETRY_LENS = (64, 0, 65, 62, 1, 1, 2, 15, 0, 1, 2, 811, 2200, 0, 37)
GEOMETRY_GAPS = (100, 250, 101, 499, 99, 740, 500, 1, 333, 120, 260, 90, 410)


def geometry():
    """Prepass geometry: read boundaries at lane 0 (anchor 64), lane 1 (129) and lane 63 (191) of a 64-anchor tile, a tile with reads of
    1, 1, 2, 15, 1 and 2 anchors, a boundary on the 1023 | 1024 block edge, a read over three blocks (1024 .. 3224) and a last block
    that is not full, with empty reads in between.  Every read steps g, g + 1, g, ... under its own gap g; no two neighbours share one."""
    reads, gaps, it = [], [], iter(GEOMETRY_GAPS)
    for n in GEOMETRY_LENS:
        if n == 0:
            reads.append(None)
            continue
        g = next(it)
        reads.append(walk(([g, g + 1] * n)[:n - 1], x0=5000, q0=100))
        gaps.append((g, 1 << 20))
    sh = pack("geometry", par1(bw=100), reads, gaps)
    b = sh.off[1:][np.diff(sh.off) > 0]
    assert {64, 129, 191, BLOCK}.issubset(set(b.tolist())) and sh.off[12] == BLOCK and sh.off[13] == 3224 and sh.off[-1] % BLOCK
    return sh


def _pair(dr, dq, seg1=0):
    return np.concatenate([anchors([1000], [1000], seg=0), anchors([1000 + dr], [1000 + dq], seg=seg1)])


def filters():
    """The filters that read a gap, at their exact values (value: the pair chains; value + 1: it does not), each pair under the gap G,
    under G + 1 and under G - 1:  dq against gap_qry in one segment (chain.c:258), dq against gap_ref across segments (chain.c:258,
    n_segs = 2), dr against gap_qry in one segment of a read with n_segs = 2 (chain.c:261)."""
    reads, gaps, ns = [], [], []
    G = 300                                                          # dq vs gap_qry, same segment (gap_ref 500, bw 100)
    for val, gq in ((G, G), (G + 1, G + 1), (G + 1, G), (G, G - 1)):
        reads.append(_pair(val, val)); gaps.append((500, gq)); ns.append(1)
    G = 500                                                          # dq vs gap_ref, different segments (dr 40: in the window either way)
    for val, gr in ((G, G), (G + 1, G + 1), (G + 1, G), (G, G - 1)):
        reads.append(_pair(40, val, seg1=1)); gaps.append((gr, 60)); ns.append(2)
    G = 300                                                          # dr vs gap_qry, same segment of a two-segment read (dq 250 <= gap_qry)
    for val, gq in ((G, G), (G + 1, G + 1), (G + 1, G), (G, G - 1)):
        reads.append(_pair(val, 250)); gaps.append((500, gq)); ns.append(2)
    return pack("filters", par1(bw=100), reads, gaps, n_segs=ns)


DEEP_LEN, DEEP_PERIOD = 600, 250


def deep_unit():
    """600 anchors one base apart whose only predecessors that pass the filters lie 200 .. 300 anchors back (the query position falls by
    one per anchor and jumps up by 250 every 250 anchors): under gap_ref 300 every scan runs through the whole window, past a ring of
    128 (and of 256) anchors, and nothing in it is marked."""
    i = np.arange(DEEP_LEN, dtype=np.int64)
    return anchors(50000 + i, 5000 - (i % DEEP_PERIOD) + DEEP_PERIOD * (i // DEEP_PERIOD))


def variants():
    """The variant k_chain_units picks per unit, in one batch: gap_qry >= gap_ref and gap_qry < gap_ref (the two table-driven
    variants), a read whose (gap_ref + 1) * (ring + 1) passes 2^32 (gap_ref = 2^25: the general variant at every ring) between reads
    that stay below, and a unit of 600 anchors on the deep path between short ones."""
    big = 1 << 25
    short = lambda g: walk([g, g + 1, g, 3, 4, g + 1, g])
    qry_below = walk([500, 501, 500, 3, 4, 501, 500], [450, 451, 450, 3, 4, 450, 451])      # dq at gap_qry = 450 < gap_ref = 500 and one above
    reads = [short(300), qry_below, walk([big, big + 1, big, big, big + 1]), short(200), deep_unit(), short(250), None, short(120)]
    gaps = [(300, 400), (500, 450), (big, big), (200, 200), (300, 400), (250, 300), (120, 4000)]
    sh = pack("variants", par1(bw=100), reads, gaps)
    assert all((int(g) + 1) * (ring + 1) >= 1 << 32 for g in (big,) for ring in (128, 256, 512))
    return sh


def all_shapes():
    return [cut_edge(), singletons(), geometry(), filters(), variants()]


_cache = {}


def shape_with_expected(name):
    """(shape, (f, p, v, seeds_off, seeds)) by name, computed once per process and shared."""
    if name not in _cache:
        sh = {s.name: s for s in all_shapes()}[name]
        _cache[name] = (sh, expected(sh))
    return _cache[name]


NAMES = ("cut_edge", "singletons", "geometry", "filters", "variants")
