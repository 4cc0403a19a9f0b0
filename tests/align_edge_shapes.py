"""Inputs of the edge tier of the region alignment (chaindp_align1): scenes that reach what the recorded scenes of align_shapes never do --
the DP's wide and global routes under align1, both of them in one batch and in the second pass; a second 64-lane stride in the
bookkeeping kernels (anchors of a region, bases of an M run, target bases of an inversion stretch); a region that fills all its slots;
and `tiny`, the unit the GPU test repeats until every grid-stride loop takes a second turn.

Every scene is built on align_shapes.mutate / anchors_of / region / pack, shares the targets of targets() and draws from a generator
seeded by the read's own name, so that adding or dropping a read changes no other.  Scenes of one opt can be concatenated into one call
(concat()).  COUNTERS names the classes align_model counts; tests/test_align_edges_cpu.py runs the model and wants every one reached."""
import zlib

import numpy as np

import align_model as A
import align_shapes as S

# gap6000: with the default max_gap = 5000 no extension can be global: the target side of an extension is at most max_gap long, and
# 12 * 5008 + 16 is below the 65 536 bytes of LDS even before the query's share; 12 * 5600 + 2800 + 16 is above
OPTS = dict(S.OPTS, gap6000=dict(S.OPTS["lowz"], max_gap=6000))

COUNTERS = ("route_wide_ext_left", "route_wide_ext_right", "route_wide_fill_pass1", "route_wide_fill_pass2", "route_wide_long_join", "route_global",
            "cnt1_gt_64", "cnt1_gt_128", "long_gaps_only_past_64", "split_both_sides_gt_64",
            "inv_t_le_64", "inv_t_65_128", "inv_t_gt_128", "inv_t_mod64_0", "inv_t_mod64_1", "inv_q_gt_t", "inv_q_lt_t", "inv_below_threshold",
            "inv_skipped_max_gap",
            "extra_clamp_at_63", "extra_clamp_at_0", "extra_max_at_63", "extra_max_at_0", "extra_clamp_then_max_later_block", "extra_gap_clamps",
            "n_ambi_in_gap", "m_run_64", "m_run_65", "m_run_128", "m_run_129", "slots_full")


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def targets():
    rng = np.random.default_rng(20240923)
    return [S.rand_seq(rng, 9600), S.rand_seq(rng, 6000)]


def other(c):
    return S.ACGT[(S.ACGT.index(c) + 1) % 4]


def compose(rng, tseq, pieces):
    """A read on the forward strand from pieces: ("copy", t0, t1) exact target bases, ("mut", t0, t1, sub, indel) align_shapes.mutate,
    ("pat", t0, "MMX...") one target base per letter, copied (M) or replaced by another one (X), ("inv", t0, t1) the stretch
    reverse-complemented, ("lit", str) bases of no target position.  Returns (read, path, starts): path as mutate's, starts[i] the read
    position where piece i begins."""
    out, path, starts = [], [], []
    n = 0
    for p in pieces:
        starts.append(n)
        if p[0] == "copy":
            s, pa = tseq[p[1]:p[2]], list(range(p[1], p[2]))
        elif p[0] == "mut":
            s, pa = S.mutate(rng, tseq, p[1], p[2], sub=p[3], indel=p[4])
        elif p[0] == "pat":
            s = "".join(c if m == "M" else other(c) for c, m in zip(tseq[p[1]:p[1] + len(p[2])], p[2]))
            pa = [p[1] + i if m == "M" else -1 for i, m in enumerate(p[2])]
        elif p[0] == "inv":
            s = S.rc(tseq[p[1]:p[2]]); pa = [-1] * len(s)
        else:
            s = p[1]; pa = [-1] * len(s)
        out.append(s); path += pa; n += len(s)
    return "".join(out), path, starts


def read(name, T, rid, pieces, rev=0, step=15, jitter=False, k=15, keep=None, whole=True):
    """keep(y, starts): which anchors stay, by their read position on the mapped strand."""
    rng = rng_of(name)
    seq, path, starts = compose(rng, T[rid], pieces)
    a = S.anchors_of(path, k, rid, rev, step, rng if jitter else None)
    if keep is not None and len(a):
        a = a[[bool(keep(int(y) & 0xffffffff, starts)) for y in a[:, 1]]]
    rd = dict(name=name, seq=S.rc(seq) if rev else seq, a=a, regs=[], starts=starts)
    if whole and len(a):
        rd["regs"] = [S.region(a, len(seq), 0, len(a))]
    return rd


# the inverted stretches of the scene `inversions`: (length, bases dropped (< 0) or added (> 0) in the stretch's middle).  Searched on
# the CPU with the model until the inv_* classes of COUNTERS were hit: the stretch mm_test_zdrop cuts out is a little longer than the inverted bases
INVERSIONS = ((45, 0), (62, 0), (63, 0), (75, 0), (100, 0), (126, 0), (127, 0), (160, 0), (192, 0), (230, 0), (260, 0), (300, 0), (90, -4), (150, -6), (150, 7))


def inversion_read(T, ln, d, tag=""):
    t0 = 200 + 37 * ln % 1500
    p = t0 + 330
    if d == 0:
        mid = [("inv", p, p + ln)]
    else:
        h = ln // 2
        mid = [("inv", p + h, p + ln)] + ([("lit", "ACGTACGTAC"[:d])] if d > 0 else []) + [("inv", p, p + h + (d if d < 0 else 0))]
    return read(f"inv_{ln}_{d}{tag}", T, 1, [("mut", t0, p, .02, .01)] + mid + [("mut", p + ln, p + ln + 330, .02, .01)], step=30, jitter=True)


def scenes():
    T = targets()
    out = []

    def scene(name, opt, reads):
        for rd in reads:
            rd.pop("starts", None)
        out.append(S._finish(dict(name=name, opt=dict(OPTS[opt]), targets=T, reads=reads)))

    # ---- DP routes under align1.  No anchor on the first (last) 460 bases: an extension of 460 x 918, 4 waves; the left one is gathered reversed
    scene("wide_ext", "ont", [read("wide_left", T, 0, [("mut", 2000, 3000, .03, .02)], step=30, jitter=True, keep=lambda y, s: y >= 460),
                              read("wide_left_rev", T, 0, [("mut", 3200, 4200, .03, .02)], rev=1, step=30, jitter=True, keep=lambda y, s: y >= 460),
                              read("wide_right", T, 1, [("mut", 1000, 2000, .03, .02)], step=30, jitter=True, keep=lambda y, s: y < 520)])
    # 700 random bases between anchors: a fill of 720 x 720 that is wide in the first pass, Z-drops, is wide again in the second, and splits
    # the region with more than 64 anchors on either side; the same around an inverted stretch (code 2, the split-off region marked)
    side = 1500
    scene("wide_fill_two_pass", "lowz", [read("junk_700", T, 0, [("mut", 300, 300 + side, .01, .005), ("lit", S.rand_seq(rng_of("junk_700_lit"), 700)),
                                                                 ("mut", 1000 + side, 1000 + 2 * side, .01, .005)]),
                                         read("inv_split_wide", T, 0, [("mut", 4000, 4000 + side, .01, .005), ("inv", 4000 + side, 4160 + side),
                                                                       ("mut", 4160 + side, 4160 + 2 * side, .01, .005)], rev=1)])
    # MM_SEED_LONG_JOIN behind 550 read bases without an anchor that span 750 target bases: bw1 = max(qe - qs, re - rs), the full band, 4 waves
    lj = read("long_join_wide", T, 1, [("mut", 2500, 2800, .03, .02), ("copy", 2800, 3050), ("copy", 3250, 3550), ("mut", 3550, 3900, .03, .02)],
              step=30, jitter=True, keep=lambda y, s: y < s[1] or y >= s[3] + 14)
    first_behind = int(np.flatnonzero((lj["a"][:, 1] & np.uint64(0xffffffff)) >= np.uint64(lj["starts"][3]))[0])
    lj["a"][first_behind, 1] |= np.uint64(A.SEED_LONG_JOIN)
    lj["regs"] = [S.region(lj["a"], len(lj["seq"]), 0, len(lj["a"]))]
    scene("long_join_wide", "ont", [lj])
    # 2 800 read bases ahead of the first anchor, 8 500 target bases ahead of it, max_gap 6 000: an extension of 2 827 x 5 654 whose state lies
    # in global scratch; beside it a read whose second pass is one wide fill, so that a second pass of wide problems alone follows a first
    # pass with all three routes
    scene("global_left", "gap6000", [read("global_left", T, 0, [("mut", 5700, 8800, .03, .02)], step=30, jitter=True, keep=lambda y, s: y >= 2800),
                                     read("junk_700_short", T, 1, [("mut", 3000, 3400, .02, .01), ("lit", S.rand_seq(rng_of("junk_700_short_lit"), 700)),
                                                                   ("mut", 4100, 4500, .02, .01)], step=30, jitter=True)])
    # ---- 64-lane strides.  Anchors every 15 bases of an exact read: 146 of them; an insertion and a deletion of 25, 60 bases apart, at anchor
    # 73 or so (only a second stride sees two long gaps), and one long gap below anchor 64 with one beyond anchor 128
    ins = S.rand_seq(rng_of("ins25"), 25)
    many = [read("gaps_past_64", T, 0, [("copy", 3000, 4100), ("lit", ins), ("copy", 4100, 4160), ("copy", 4185, 5200)]),
            read("gaps_20_and_132", T, 0, [("copy", 6000, 6300), ("lit", ins), ("copy", 6300, 8000), ("copy", 8025, 8200)], rev=1)]
    for cnt, as_ in ((64, 40), (65, 41), (129, 8)):             # cut from a longer list: neighbours on both sides
        rd = read(f"cnt_{cnt}", T, 1, [("copy", 500 + cnt, 2700 + cnt)])
        rd["regs"] = [S.region(rd["a"], len(rd["seq"]), as_, cnt)]
        many.append(rd)
    scene("many_anchors", "ont", many)
    # exact reads: the whole alignment is one M of 64, 65, 127, 128, 129, 193 bases
    scene("exact_runs", "ont", [read(f"exact_{ln}", T, 1, [("copy", 3000 + 250 * i, 3000 + 250 * i + ln)], rev=i & 1) for i, ln in enumerate((64, 65, 127, 128, 129, 193))])
    # mm_update_extra's running score s, clamped at 0, and its maximum, relative to the 64-base blocks of an M run.  Mismatches among
    # matches, which no gap gets around, inside the first fill: 42 matches and 22 mismatches bring s to 0 at offset 62 and below it at 63
    # (22 matches, then 22 mismatches with a match between each two: below 0 at 64), and the exact bases behind put the maximum into a later block of the same run.  end_bonus = 100 lets the
    # right extension reach the read's end through a tail that costs more than it gains: s peaks on the last base of block 0 (the first of block 1)
    t0 = 700
    at63, at64 = "M" * 21 + "XM" * 20 + "MXX", "M" * 22 + "XM" * 21 + "X"
    clamp = [read("clamp_at_63", T, 1, [("pat", t0, at63), ("copy", t0 + 64, t0 + 330)]),
             read("clamp_at_64", T, 1, [("pat", t0 + 405, at64), ("copy", t0 + 470, t0 + 735)], rev=1),     # a place where no gap pays: one M
             read("max_at_63", T, 1, [("copy", t0 + 800, t0 + 864), ("pat", t0 + 864, "XXM" * 8)]),
             read("max_at_64", T, 1, [("copy", t0 + 900, t0 + 965), ("pat", t0 + 965, "XXM" * 8)]),
             read("gap_clamps", T, 1, [("copy", t0 + 1000, t0 + 1010), ("copy", t0 + 1022, t0 + 1200)]),        # 10 matches, then 12D: 20 - 28 < 0
             read("n_in_insertion", T, 1, [("copy", t0 + 1300, t0 + 1420), ("lit", "GATTACAGGCTT" + "NNNNN" + "CATCGGATAGCCT"), ("copy", t0 + 1420, t0 + 1540)])]
    scene("clamp_edges", "bonus", clamp)
    # inverted stretches of 45 to 300 bases, with and without small indels inside; one so thinned out (every third base replaced) that
    # its inversion score stays below min_chain_score * a; and under gap600 one of max_gap bases or more, where the test is skipped
    invs = [inversion_read(T, ln, d) for ln, d in INVERSIONS]
    invs.append(read("inv_diverged", T, 1, [("mut", 4000, 4330, .02, .01), ("lit", S.rc("".join(other(c) if i % 3 == 0 else c for i, c in enumerate(T[1][4330:4530])))),
                                            ("mut", 4530, 4860, .02, .01)], step=30, jitter=True))
    scene("inversions", "lowz", invs)
    scene("inv_skipped", "gap600", [read("inv_650", T, 0, [("mut", 1000, 1330, .02, .01), ("inv", 1330, 1980), ("mut", 1980, 2310, .02, .01)], step=30, jitter=True)])
    # every anchor makes a fill (45 apart, min_ksw_len 40) and both extensions exist: cnt + 1 problems in cnt + 1 slots, other reads' regions on both sides
    scene("slots_full", "ont", [read("before", T, 0, [("mut", 100, 400, .03, .02)], step=30, jitter=True),
                                read("full", T, 1, [("copy", 5000, 5000 + 14 + 45 * 7 + 21)], step=45),
                                read("after", T, 0, [("mut", 500, 800, .03, .02)], rev=1, step=30, jitter=True)])
    # ---- the batch: 16 reads of 40 to 60 bases, cnt 1 or 2, both strands, one region of no anchors, one read of no region
    tiny = []
    for i in range(16):
        ln = 40 + (i * 7) % 21
        rd = read(f"tiny{i}", T, i & 1, [("mut", 150 + 90 * i, 150 + 90 * i + ln, .02, 0.)], rev=(i >> 1) & 1, step=25)
        n = len(rd["a"])
        cnt = min(n, 1 + i % 2)
        rd["regs"] = [S.region(rd["a"], len(rd["seq"]), n - cnt if i & 4 else 0, cnt)] if cnt else []
        if i == 5:
            rd["regs"] = [S.region(rd["a"], len(rd["seq"]), 0, 0)] + rd["regs"]
        if i == 11:
            rd["regs"] = []
        tiny.append(rd)
    scene("tiny", "ont", tiny)
    return out


def concat(packed):
    """The packed scenes (pack()'s dicts or loaded goldens, outputs included where present) of one opt and one target list as one call."""
    first = packed[0]
    assert all(np.array_equal(p["opt"], first["opt"]) and np.array_equal(p["tseq"], first["tseq"]) for p in packed)
    out = dict(opt=first["opt"], tseq=first["tseq"], tseq_off=first["tseq_off"])
    for k in ("seq", "a", "regs", "regs_out", "regs2", "extra", "a_out", "read_name"):
        if k in first:
            out[k] = np.concatenate([p[k] for p in packed])
    for k, of in (("seq_off", "seq"), ("a_off", "a"), ("regs_off", "regs"), ("cigar_off", "cigar")):
        if k in first:
            base = np.cumsum([0] + [int(p[k][-1]) for p in packed[:-1]])
            out[k] = np.concatenate([first[k][:1]] + [p[k][1:] + b for p, b in zip(packed, base)]).astype(np.int64)
    if "cigar" in first:
        out["cigar"] = np.concatenate([p["cigar"] for p in packed])
    return out


def reorder(g, order):
    """The packed scene g (outputs included where present) with its reads in the given order."""
    order = [int(i) for i in order]
    out = dict(opt=g["opt"], tseq=g["tseq"], tseq_off=g["tseq_off"], read_name=g["read_name"][order])
    for k, of in (("seq", "seq_off"), ("a", "a_off"), ("regs", "regs_off")):
        out[k] = np.concatenate([g[k][g[of][i]:g[of][i + 1]] for i in order]) if order else g[k][:0]
        out[of] = np.concatenate([[0], np.cumsum([g[of][i + 1] - g[of][i] for i in order])]).astype(np.int64)
    if "regs_out" in g:
        ro = g["regs_off"]
        regs = np.concatenate([np.arange(ro[i], ro[i + 1]) for i in order]).astype(np.int64) if order else np.zeros(0, np.int64)
        for k in ("regs_out", "regs2", "extra"):
            out[k] = g[k][regs]
        out["a_out"] = np.concatenate([g["a_out"][g["a_off"][i]:g["a_off"][i + 1]] for i in order])
        co = g["cigar_off"]
        out["cigar"] = np.concatenate([g["cigar"][co[j]:co[j + 1]] for j in regs]) if len(regs) else g["cigar"][:0]
        out["cigar_off"] = np.concatenate([[0], np.cumsum(co[regs + 1] - co[regs])]).astype(np.int64)
    return out
