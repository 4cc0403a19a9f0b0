"""Inputs of the edge tier of Device.align_reads (chaindp_align_reads): reads whose lists, as the loop leaves them for mm_filter_regs and
as mm_hit_sort_by_dp returns them, have the lengths at which the kernels at the end of the call (csrc/reads/chaindp_reads.hip) take
another path: 1 and 2 (mm_hit_sort_by_dp returns at once for a list of one), 64 and 65 (one trip of a wave's lanes, and a second),
the cap up to which k_reads_finish ranks a list in LDS and one past it (a scene names the cap it is meant for, lowered through the
debug setter: the built-in RD_LDS_CAP would need a read of a thousand regions), a read whose every region is filtered, reads without
regions first and last in the batch, and a split-off region and a made inversion inside a list that takes the global route.

A read is stitched from shuffled exact copies of 90-120 bases of distinct stretches of one target, one region each: no two pieces are
colinear, every piece is aligned on its own, and the pieces' lengths give the sort keys an order of their own.  classes() counts a class
per edge from a scene's recorded outputs; tests/golden/make_align_reads_golden.py asserts every class reached.

The tie scenes (TIE_NAMES) hold the order of equal sort keys: their reads' regions share one hash, so pieces of one length tie on
dp_max << 32 | hash, and mm_hit_sort_by_dp's radix_sort_128x with the reversal behind it decides -- a stable insertion sort up to 64
live regions (the later region first), the in-place byte-wise procedure above.  A copy's alignment runs on into its neighbours while
the bases there happen to agree, so pieces of one length need not tie: where a read's keys are all to be equal, its pieces are
LEVEL bases each from slots chosen so that at every joint the two bases on either side disagree (apart).  The lengths are given
or drawn from the seeds in TIE_SEEDS; the generator's search over the reference found the seeds (and asserts that it still does);
tie_classes() counts the classes from the recorded outputs alone."""
import collections
import os

import numpy as np

import align_shapes as S
import skeleton_model as K
import skeleton_shapes as SS
from align_shapes import rand_seq, region

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_reads")
NAMES = ("trips", "lds_cap")
TIE_NAMES = ("ties_small", "ties_64", "ties_130", "ties_cap", "ties_unaided")
RD_LDS_CAP = 1024                      # csrc/chaindp_reads_plan.h
SCENE_CAP = 16                         # the cap the scene lds_cap is run under
SLOT = 160                             # a piece's stretch of the target: at most 120 bases copied, the rest keeps neighbours apart
CLASSES = tuple("%s_len_%s" % (w, n) for w in ("placed", "final") for n in ("1", "2", "64", "65", "cap", "cap_plus_1")) + (
    "every_region_filtered", "empty_read_first", "empty_read_last", "split_off_in_a_global_route_list", "inversion_in_a_global_route_list",
    "filtered_in_a_global_route_list", "sort_changes_order_past_one_trip")
TIE_CLASSES = ("final_len_2_keys_equal", "final_len_3_one_tied_pair", "final_len_64_several_groups", "placed_longer_live_64_tied", "final_len_65_tied",
               "final_len_130_plus_group_in_neither_order", "final_past_64_all_keys_equal", "tie_across_placed_63_and_64",
               "filtered_and_inversion_between_tied", "global_route_live_64_tied", "global_route_live_65_tied", "final_past_64_tied_of_longer_placed")
UNAIDED = "tie_without_help"           # wanted, with a fallback: see unaided_scene
TIE_SEEDS = dict(ties_small=1, ties_64=10, ties_130=0, ties_unaided=0)
LEVEL = 100                            # the length of every piece of a read whose keys are all to be equal
SEARCH = 64                            # seeds the generator tries for each entry of TIE_SEEDS
SHORT = 50                             # a piece of two anchors: below min_cnt, filtered


def empty(rng, name):
    return dict(name=name, seq=rand_seq(rng, 60), a=np.zeros((0, 2), np.uint64), regs=[])


def stitched(rng, name, T, slots, n, short=0, special=None, lens=None):
    """n pieces from the next n free slots of T (slots: the shuffled free slot numbers, consumed), the first `short` of them 50 bases long
    (two anchors: below min_cnt); special = (t0, t1, edits): one more piece, align_shapes.mutate's copy of T[t0:t1], in the middle.
    lens: the n pieces' lengths given, nothing drawn."""
    seq, a, cuts = [], [], []
    at = 0
    if lens is not None:
        assert len(lens) == n and not short
        pieces = [("slot", slots.pop(), int(ln)) for ln in lens]
    else:
        pieces = [("slot", slots.pop(), SHORT if j < short else int(rng.integers(90, 121))) for j in range(n)]
    if special:
        pieces.insert(len(pieces) // 2, ("special",) + tuple(special))
    for kind, *what in pieces:
        if kind == "slot":
            t0 = what[0] * SLOT + 20
            s, path, step = T[t0:t0 + what[1]], list(range(t0, t0 + what[1])), 25
        else:
            s, path = S.mutate(rng, T, what[0], what[1], sub=0, indel=0, edits=what[2])
            step = 30
        pa = S.anchors_of(path, 15, 0, 0, step)
        pa[:, 1] += np.uint64(at)
        cuts.append((sum(len(x) for x in a), len(pa)))
        seq.append(s); a.append(pa)
        at += len(s)
    seq, a = "".join(seq), np.concatenate(a)
    return dict(name=name, seq=seq, a=a, regs=[region(a, len(seq), as_, cnt, id_=j, parent=j) for j, (as_, cnt) in enumerate(cuts)])


def all_scenes():
    rng = np.random.default_rng(20250301)
    n_slots = 1 + 2 + 64 + 65 + SCENE_CAP + SCENE_CAP + 1 + 3 + 20 + 8
    T = rand_seq(rng, n_slots * SLOT + 1200)
    slots = [int(x) for x in rng.permutation(n_slots)]
    tail = n_slots * SLOT + 100           # the special piece's stretch: behind every slot

    def scene(name, cap, reads):
        sc = S._finish(SS.set_hashes(dict(name=name, opt=dict(S.OPTS["lowz"]), targets=[T], reads=reads)))
        sc["lds_cap"] = cap
        return sc
    trips = scene("trips", RD_LDS_CAP, [empty(rng, "empty_first")] + [stitched(rng, "pieces_%d" % n, T, slots, n) for n in (1, 2, 64, 65)] + [empty(rng, "empty_last")])
    cap = scene("lds_cap", SCENE_CAP, [stitched(rng, "pieces_cap", T, slots, SCENE_CAP), stitched(rng, "pieces_cap_plus_1", T, slots, SCENE_CAP + 1),
                                       stitched(rng, "all_filtered", T, slots, 3, short=3),
                                       stitched(rng, "split_and_inversion", T, slots, 18, short=2, special=(tail, tail + 900, [(tail + 400, "inv", 160)]))])
    return [trips, cap]


def one_hash(rd, h):
    for r in rd["regs"]:
        r["hash"] = h
    return rd


def _drawn(rng, n, shorts=()):
    """n lengths of 90-120 and a filtered piece ahead of each position in shorts."""
    lens = [int(x) for x in rng.integers(90, 121, n)]
    for at in sorted(shorts, reverse=True):
        lens.insert(at, SHORT)
    return lens


def apart(T, slots, n):
    """Moves n of the free slots to the end of the list, where stitched takes them from, so that pieces of LEVEL bases from them, in
    that order, do not run on into each other: behind a piece the target's next three bases all differ from the first three of the piece
    that follows in the read, ahead of that piece the target's three bases all differ from the last three of the piece before, and no
    piece lies within three slots of either of the two before it (an alignment would reach across)."""
    t0 = lambda sl: sl * SLOT + 20
    took = [slots.pop()]
    while len(took) < n:
        a = t0(took[-1])
        sl = next(x for x in reversed(slots) if all(abs(x - y) > 3 for y in took[-2:])
                  and all(T[a + LEVEL + i] != T[t0(x) + i] and T[t0(x) - 1 - i] != T[a + LEVEL - 1 - i] for i in (0, 1, 2)))
        slots.remove(sl)
        took.append(sl)
    slots += took[::-1]


def tie_scene(name, seed=None):
    """One of TIE_NAMES[:4]; seed: the lengths' seed where TIE_SEEDS has an entry for the scene."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lr = np.random.default_rng(seed)              # the searched lengths only
    plans = dict(
        # two equal pieces; two equal pieces around a longer one; two equal pieces with a filtered piece, a region that splits at an
        # inverted stretch and the inversion made there between them
        ties_small=lambda: (RD_LDS_CAP, [("pair", [LEVEL] * 2, None), ("pair_and_one", [100, 110, 100], None), ("around", [100, SHORT, 100], "inv")]),
        # 64 pieces of 31 lengths; 64 live pieces among 67; 65 pieces, the last two equal; 70 pieces of one length
        ties_64=lambda: (RD_LDS_CAP, [("final_64", _drawn(rng, 64), None), ("live_64_of_67", _drawn(rng, 64, (5, 30, 64)), None),
                              ("final_65", (lambda l: l[:64] + [l[63]])(_drawn(rng, 64)), None), ("all_equal_70", [LEVEL] * 70, None)]),
        ties_130=lambda: (RD_LDS_CAP, [("final_130", _drawn(lr, 130), None)]),
        ties_cap=lambda: (SCENE_CAP, [("live_64_of_66", _drawn(rng, 64, (0, 40)), None), ("final_65", _drawn(rng, 65), None),
                              ("live_70_of_73", _drawn(rng, 70, (2, 33, 66)), None)]))
    cap, reads = plans[name]()
    n_slots = sum(len(l) for _, l, _ in reads) + 40               # spare slots: apart() has a choice, and few pieces are no neighbours on the target
    T = rand_seq(rng, n_slots * SLOT + 1200)
    slots = [int(x) for x in rng.permutation(n_slots)]
    tail = n_slots * SLOT + 100
    out = []
    if name == "ties_small":                       # whether two pieces of one length tie rests on their neighbours: the seed decides the slots
        slots = [int(slots[i]) for i in lr.permutation(len(slots))]
    for rd_name, lens, special in reads:
        if lens == [LEVEL] * len(lens):
            if len(lens) > 2:                      # an alignment can still gain beyond a joint, behind a gap; the seed decides the slots
                slots = [int(slots[i]) for i in lr.permutation(len(slots))]
            apart(T, slots, len(lens))
        out.append(stitched(rng, rd_name, T, slots, len(lens), lens=lens, special=(tail, tail + 900, [(tail + 400, "inv", 160)]) if special else None))
    sc = SS.set_hashes(dict(name=name, opt=dict(S.OPTS["lowz"]), targets=[T], reads=out))
    sc = S._finish(dict(sc, reads=[one_hash(rd, 0x1234567 + i) for i, rd in enumerate(out)]))
    sc["lds_cap"] = cap
    return sc


def unaided_scene(seed):
    """Every region with a hash of its own: a tie has to arise in the loop.  A read with an inverted stretch in its middle, copied
    exactly: mm_split_reg gives the region split off there its parent's hash (hit.c:93), and the two tie where their dp_max agree.  A
    read with three inverted stretches of one length: the loop tests the first and the third pair, and the two inversions made there
    have hash 0 (mm_align1_inv zeroes r_inv)."""
    rng = np.random.default_rng(seed)
    T = [rand_seq(rng, 3200)]
    reads = [S.read_of(rng, "inversion_in_the_middle", T, 0, 100, 1160, sub=0, indel=0, edits=[(550, "inv", 160)]),
             S.read_of(rng, "three_inversions", T, 0, 1200, 3100, sub=0, indel=0, edits=[(1600, "inv", 160), (2100, "inv", 160), (2600, "inv", 160)])]
    sc = S._finish(SS.set_hashes(dict(name="ties_unaided", opt=dict(S.OPTS["lowz"]), targets=T, reads=reads)))
    sc["lds_cap"] = RD_LDS_CAP
    return sc


def tie_scenes(seeds=None):
    seeds = TIE_SEEDS if seeds is None else seeds
    return [tie_scene(n, seeds.get(n)) for n in TIE_NAMES[:4]] + ([unaided_scene(seeds["ties_unaided"])] if seeds["ties_unaided"] is not None else [])


def pack(scene):
    return dict(S.pack(scene), lds_cap=np.int64(scene["lds_cap"]))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def classes(g):
    """The edge classes a recorded scene reaches (g: pack()'s arrays and the *_out of the reference)."""
    c = collections.Counter()
    cap = int(g["lds_cap"])
    named = {1: "1", 2: "2", 64: "64", 65: "65", cap: "cap", cap + 1: "cap_plus_1"}
    n_in, n_placed, n_final = (np.diff(g[k]) for k in ("regs_off", "placed_off_out", "regs_off_out"))
    for which, lens in (("placed", n_placed), ("final", n_final)):
        for n in lens:
            if int(n) in named:
                c["%s_len_%s" % (which, named[int(n)])] += 1
    c["every_region_filtered"] += int(((n_placed > 0) & (n_final == 0)).sum())
    c["empty_read_first"] += int(n_in[0] == 0)
    c["empty_read_last"] += int(n_in[-1] == 0)
    for rd in np.flatnonzero(n_placed > cap):
        placed = g["placed_out"][int(g["placed_off_out"][rd]):int(g["placed_off_out"][rd + 1])]
        c["split_off_in_a_global_route_list"] += int(((placed["bits"] >> 9 & 1) == 1).sum())               # split & 2: this region was split off
        c["inversion_in_a_global_route_list"] += int(((placed["bits"] & K.BIT_INV) != 0).sum())
        c["filtered_in_a_global_route_list"] += int(n_placed[rd] > n_final[rd])
    for rd in np.flatnonzero(n_final > 64):
        key = (g["extra_out"]["dp_max"].astype(np.int64) << 32 | g["regs_out"]["hash"])[int(g["regs_off_out"][rd]):int(g["regs_off_out"][rd + 1])]
        assert (np.diff(key) <= 0).all()
        ids = g["regs_out"]["id"][int(g["regs_off_out"][rd]):int(g["regs_off_out"][rd + 1])]
        c["sort_changes_order_past_one_trip"] += int((np.diff(ids) < 0).any())     # the input regions' ids rise along the read
    return c


def tie_groups(g, rd):
    """The read's final list: [(key, [placed position of every region with that key, in final order])] for the keys that occur twice or
    more, and the placed position of every final region.  A region is found in the placed list by its words."""
    p0, p1, f0, f1 = (int(g[k][rd + i]) for k in ("placed_off_out", "regs_off_out") for i in (0, 1))
    placed, final = g["placed_out"][p0:p1], g["regs_out"][f0:f1]
    at = {r.tobytes(): i for i, r in enumerate(placed)}
    assert len(at) == len(placed)
    pos = [at[r.tobytes()] for r in final]
    key = (g["extra_out"]["dp_max"][f0:f1].astype(np.int64) << 32 | final["hash"]).tolist()
    assert all(x >= y for x, y in zip(key, key[1:]))
    groups = collections.OrderedDict()
    for k, p in zip(key, pos):
        groups.setdefault(k, []).append(p)
    return [(k, ps) for k, ps in groups.items() if len(ps) > 1], pos


def tie_classes(g):
    """The tie classes a recorded scene reaches, from its recorded outputs."""
    c = collections.Counter()
    cap = int(g["lds_cap"])
    n_placed, n_final = (np.diff(g[k]) for k in ("placed_off_out", "regs_off_out"))
    for rd in range(len(n_final)):
        groups, pos = tie_groups(g, rd)
        if not groups:
            continue
        nf, npl, tied = int(n_final[rd]), int(n_placed[rd]), sum(len(ps) for _, ps in groups)
        r0 = int(g["regs_off"][rd])
        helped = len(set(g["regs"]["hash"][r0:int(g["regs_off"][rd + 1])].tolist())) < int(g["regs_off"][rd + 1]) - r0
        c[UNAIDED] += int(not helped)
        c["final_len_2_keys_equal"] += int(nf == 2)
        c["final_len_3_one_tied_pair"] += int(nf == 3 and tied == 2)
        c["final_len_64_several_groups"] += int(nf == 64 and len(groups) > 1)
        c["placed_longer_live_64_tied"] += int(nf == 64 and npl > 64)
        c["final_len_65_tied"] += int(nf == 65)
        c["final_len_130_plus_group_in_neither_order"] += int(nf >= 130 and any(ps != sorted(ps) and ps != sorted(ps, reverse=True) for _, ps in groups))
        c["final_past_64_all_keys_equal"] += int(nf > 64 and tied == nf and len(groups) == 1)
        c["tie_across_placed_63_and_64"] += int(any(63 in ps and 64 in ps for _, ps in groups))
        c["final_past_64_tied_of_longer_placed"] += int(nf > 64 and npl > nf)
        c["global_route_live_64_tied"] += int(cap < RD_LDS_CAP and npl > cap and nf == 64)
        c["global_route_live_65_tied"] += int(cap < RD_LDS_CAP and npl > cap and nf == 65)
        p0 = int(g["placed_off_out"][rd])
        inv = {i for i in pos if int(g["placed_out"]["bits"][p0 + i]) & K.BIT_INV}
        gone = set(range(npl)) - set(pos)
        c["filtered_and_inversion_between_tied"] += int(any(any(lo < i < hi for i in inv) and any(lo < i < hi for i in gone)
                                                                for _, ps in groups for lo in ps for hi in ps))
    return c
