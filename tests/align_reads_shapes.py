"""Inputs of the edge tier of Device.align_reads (chaindp_align_reads): reads whose lists, as the loop leaves them for mm_filter_regs and
as mm_hit_sort_by_dp returns them, have the lengths at which the kernels at the end of the call (csrc/reads/chaindp_reads.hip) take
another path: 1 and 2 (mm_hit_sort_by_dp returns at once for a list of one), 64 and 65 (one trip of a wave's lanes, and a second),
the cap up to which k_reads_finish ranks a list in LDS and one past it (a scene names the cap it is meant for, lowered through the
debug setter: the built-in RD_LDS_CAP would need a read of a thousand regions), a read whose every region is filtered, reads without
regions first and last in the batch, and a split-off region and a made inversion inside a list that takes the global route.

A read is stitched from shuffled exact copies of 90-120 bases of distinct stretches of one target, one region each: no two pieces are
colinear, every piece is aligned on its own, and the pieces' lengths give the sort keys an order of their own.  classes() counts a class
per edge from a scene's recorded outputs; tests/golden/make_align_reads_golden.py asserts every class reached."""
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
RD_LDS_CAP = 1024                      # csrc/chaindp_reads_plan.h
SCENE_CAP = 16                         # the cap the scene lds_cap is run under
SLOT = 160                             # a piece's stretch of the target: at most 120 bases copied, the rest keeps neighbours apart
CLASSES = tuple("%s_len_%s" % (w, n) for w in ("placed", "final") for n in ("1", "2", "64", "65", "cap", "cap_plus_1")) + (
    "every_region_filtered", "empty_read_first", "empty_read_last", "split_off_in_a_global_route_list", "inversion_in_a_global_route_list",
    "filtered_in_a_global_route_list", "sort_changes_order_past_one_trip")


def empty(rng, name):
    return dict(name=name, seq=rand_seq(rng, 60), a=np.zeros((0, 2), np.uint64), regs=[])


def stitched(rng, name, T, slots, n, short=0, special=None):
    """n pieces from the next n free slots of T (slots: the shuffled free slot numbers, consumed), the first `short` of them 50 bases long
    (two anchors: below min_cnt); special = (t0, t1, edits): one more piece, align_shapes.mutate's copy of T[t0:t1], in the middle."""
    seq, a, cuts = [], [], []
    at = 0
    pieces = [("slot", slots.pop(), 50 if j < short else int(rng.integers(90, 121))) for j in range(n)]
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
        assert (np.diff(key) < 0).all()
        ids = g["regs_out"]["id"][int(g["regs_off_out"][rd]):int(g["regs_off_out"][rd + 1])]
        c["sort_changes_order_past_one_trip"] += int((np.diff(ids) < 0).any())     # the input regions' ids rise along the read
    return c
