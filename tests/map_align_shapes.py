"""CHECKER ONLY: the scenes of the map-with-alignment tier (tests/test_map_align_cpu.py, tests/test_gpu_map_align.py) and what both
tiers share: tiny seeded batches of e2e_model.scenario in the long-read presets, each with post options that carry MM_F_CIGAR and the
alignment options of its preset; the numpy restatement of mm_squeeze_a (hit.c:270-288); the hand-off's rule restated the way the
kernel states it (ranks, running sums, strided copies), and three wrong rules beside it.  numpy only; no GPU."""
import functools
import types

import numpy as np

import e2e_model as em
from minimap2_chaindp_amd import params as P

SEED_IGNORE = np.uint64(1 << 41)       # MM_SEED_IGNORE (mmpriv.h): what the alignment marks anchors with
HO_LDS_CAP = 256                       # chaindp_handoff_plan.h

# name -> (mode of e2e_model.MODES, reads, seed, longest read, genome length, alignment preset, overrides of it, flags added to the post options)
SCENES = {
    "map-ont": ("map-ont", 48, 11, 3000, 9000, "map-ont", {}, 0),
    "map-pb": ("map-pb", 40, 12, 3000, 9000, "map-pb", {}, 0),
    "ava-ont": ("ava-ont", 48, 13, 2500, 6000, "ava-ont", {}, 0),
    "asm5": ("map-ont", 32, 14, 3000, 9000, "asm5", dict(k=15), 0),        # asm5's scoring on map-ont's index
    # mm_select_sub without mm_join_long behind it (--no-long-join): the only way a read of several regions reaches the alignment with
    # anchors that no region refers to.  With mm_join_long its own mm_squeeze_a has packed them, and what its mm_filter_regs drops
    # afterwards has no anchors left (the joined region's cnt is 0); with MM_F_ALL_CHAINS nothing is dropped at all
    "no-ljoin": ("map-ont", 64, 15, 3000, 9000, "map-ont", {}, P.MM_F_NO_LJOIN),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene: e2e_model.scenario's namespace with opt carrying MM_F_CIGAR, aopt, and the targets as align_set_targets takes them."""
    mode, n_reads, seed, max_len, genome_len, preset, over, post_flag = SCENES[name]
    sc = em.scenario(mode, n_reads=n_reads, seed=seed, max_len=max_len, genome_len=genome_len)
    if not mode.startswith("ava"):
        # two reads that lack 600-900 bases of their target between flanks of 500-700: more than the chaining bandwidth, so two chains,
        # which mm_join_long joins (the scenario's own deletions need flanks longer than these reads)
        rng = np.random.default_rng([seed, 4242])
        for _ in range(2):
            g = sc.targets[int(rng.integers(0, 3))]
            n1, n2, gap = int(rng.integers(500, 700)), int(rng.integers(500, 700)), int(rng.integers(600, 900))
            at = int(rng.integers(0, len(g) - (n1 + gap + n2)))
            sc.reads.append(em.mutate(rng, g[at:at + n1] + g[at + n1 + gap:at + n1 + gap + n2], .03))
            sc.kinds.append("deletion")
        sc.bid = np.concatenate((sc.bid, sc.bid[:2]))
        sc.hash_ = np.concatenate((sc.hash_, rng.integers(0, 1 << 32, size=2, dtype=np.uint64).astype(np.uint32)))
    d = sc.opt.asdict()
    d["flag"] |= P.MM_F_CIGAR | post_flag
    sc.aopt = P.align_opt(preset, **over)
    # one mm_mapopt_t in the reference: what both records hold of it agrees
    d.update(match_sc=sc.aopt.a, sub_diff=2 * sc.aopt.a + sc.aopt.b)
    sc.opt = P.PostOpt(**d)
    assert sc.opt.min_diff == 2 * sc.aopt.k == 2 * sc.k and sc.opt.min_chain_score == sc.aopt.min_chain_score and sc.opt.min_cnt == sc.aopt.min_cnt == sc.min_cnt
    assert bool(sc.aopt.is_hpc) == bool(sc.hpc)
    sc.tseq, sc.tseq_off = em.batch(sc.targets)
    sc.seq, sc.seq_off = em.batch(sc.reads)
    return sc


def tiled(sc, n):
    """The scene's reads repeated to n reads (reads are mapped independently): a namespace with reads, bid, hash_, seq, seq_off."""
    at = np.arange(n) % len(sc.reads)
    t = types.SimpleNamespace(at=at, reads=[sc.reads[i] for i in at], bid=sc.bid[at], hash_=sc.hash_[at])
    t.seq, t.seq_off = em.batch(t.reads)
    return t


# ---- mm_squeeze_a

def squeeze_read(regs, a):
    """mm_squeeze_a on one read: (regs with `as` rewritten, a[:total]) -- the reference's loop, its memmove done in place."""
    regs, a = regs.copy(), a.copy()
    order = sorted(range(len(regs)), key=lambda i: (int(regs["as"][i]) << 32) | i)
    at = 0
    for i in order:
        s, c = int(regs["as"][i]), int(regs["cnt"][i])
        if s != at:
            a[at:at + c] = a[s:s + c].copy()
            regs["as"][i] = at
        at += c
    return regs, a[:at]


def squeeze(regs_off, regs, a_off, a, rule=squeeze_read):
    """`rule` read by read over a batch: (regs, a_off, a) as the alignment stages take them."""
    out_r, out_a = [], []
    for r in range(len(regs_off) - 1):
        x, y = rule(regs[regs_off[r]:regs_off[r + 1]], a[a_off[r]:a_off[r + 1]])
        out_r.append(x); out_a.append(y)
    new_off = np.concatenate(([0], np.cumsum([len(y) for y in out_a]))).astype(np.int64)
    cat = lambda parts, empty: np.concatenate(parts) if len(parts) and sum(len(p) for p in parts) else empty
    return cat(out_r, regs[:0].copy()), new_off, cat(out_a, np.zeros((0, 2), np.uint64))


# ---- the hand-off as k_handoff_count / k_handoff_move state it

def handoff_read(regs, a, lds_cap=HO_LDS_CAP, rank=None, keep_as=False, skip_one=False):
    """A wave on one list: every region's place is the sum of the counts ranked before it in (as, slot) order, counted a lane per
    region in trips of 64; the anchors go from the unsqueezed array to a second one, 64 at a time, region after region; `as` is
    rewritten.  (lds_cap only chooses where as / cnt / to live: the rule is the same.)  rank / keep_as / skip_one: the wrong rules."""
    n = len(regs)
    as_, cnt = regs["as"].astype(np.int64), np.maximum(regs["cnt"].astype(np.int64), 0)
    total = int(cnt.sum())                                                     # k_handoff_count
    out = regs.copy()
    if skip_one and n < 2:
        return out, a.copy()
    before = rank or (lambda t, s: as_[t] < as_[s] or (as_[t] == as_[s] and t < s))
    to = np.zeros(n, np.int64)
    for trip in range(0, n, 64):
        for s in range(trip, min(trip + 64, n)):                               # the lanes of this trip
            to[s] = sum(int(cnt[t]) for t in range(n) if before(t, s))
    dst = np.zeros((total, 2), np.uint64)
    for s in range(n):
        for t0 in range(0, int(cnt[s]), 64):
            k = min(64, int(cnt[s]) - t0)
            if to[s] + t0 + k <= total:
                dst[to[s] + t0:to[s] + t0 + k] = a[as_[s] + t0:as_[s] + t0 + k]
    if not keep_as:
        out["as"] = to
    return out, dst


WRONG_RULES = {
    "rank_by_slot": dict(rank=lambda t, s: t < s),
    "keep_as": dict(keep_as=True),
    "skip_one_region": dict(skip_one=True),
}


def wrong(name):
    return lambda regs, a: handoff_read(regs, a, **WRONG_RULES[name])


# ---- hand-made regions and anchors: the list lengths and counts no mapped read of a test's size has

REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")]
                     + [("bits", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("reserved", "<u4", (2,))])
SCENE_CAP = 5                          # the lowered cap of the GPU tier: lists of 5 stay in LDS, lists of 6 do not
# class -> the counts of one read's regions, in slot order (the places in a[] are shuffled, with unreferenced anchors between them)
SYNTHETIC = {
    "cnt_65": [3, 65, 7], "cnt_257": [257, 4], "cnt_64": [64, 64], "cnt_0_tie": [5, 0, 0, 9],
    "regs_1": [12], "regs_5": [3] * SCENE_CAP, "regs_6": [4] * (SCENE_CAP + 1), "regs_64": [3] * 64, "regs_65": [2] * 65, "regs_129": [1, 2] * 64 + [70],
    "regs_256": [1] * HO_LDS_CAP, "regs_257": [1] * (HO_LDS_CAP + 1), "none": [],
}


@functools.lru_cache(maxsize=None)
def synthetic():
    """One batch with a read per class of SYNTHETIC, in that order: (regs_off, regs, b_off, b).  Every read's regions lie in a[] in an
    order that is not the slots', with a gap in front of each (so every `as` moves) and a tail behind the last."""
    rng = np.random.default_rng(20261021)
    regs, b = [], []
    for name, counts in SYNTHETIC.items():
        n = len(counts)
        r = np.zeros(n, REG_DTYPE)
        for k in REG_DTYPE.names:
            if k not in ("reserved", "div"):
                r[k] = rng.integers(0, 1 << 20, n)
        r["div"] = rng.random(n).astype(np.float32)
        r["cnt"] = counts
        at = 0
        for i in rng.permutation(n):
            at += int(rng.integers(1, 4))                                  # anchors no region refers to
            r["as"][i] = at
            at += counts[i]
        if name == "cnt_0_tie":                                            # the empty regions start where the next region starts: (as, slot) decides
            r["as"][1] = r["as"][2] = r["as"][3]
        regs.append(r)
        b.append(rng.integers(0, 1 << 63, (at + int(rng.integers(0, 5)), 2), dtype=np.uint64))
    off = lambda parts: np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
    return off(regs), np.concatenate(regs), off(b), np.concatenate(b)
