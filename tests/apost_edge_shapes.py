"""Named scenes for Device.align_post whose inputs sit on the lane, route and arithmetic edges of k_apost_read and its two gathers: each
is built with apost_shapes.reg and packed with apost_shapes.pack, so the loaders of the functional tier work on them.  The goldens
tests/golden/align_post_edges/*.npz (tests/golden/make_apost_edge_golden.py) hold what the compiled reference makes of them;
tests/test_align_post_edges_cpu.py proves, edge by edge, that a subtly wrong restatement gives other words there.

A scene that rests on the host's logf patch lists takes the keys the generator picked (`picks`, recorded in its file): for a list, the
first listed key >= 100 ("key"), the first one whose listed value is not the float (float)log((double)x) ("key_d"), and a subsc and
score0 at which one ulp of the logarithm moves the mapq ("subsc", "score0")."""
import os

import numpy as np

import apost_shapes as PS
from apost_shapes import BIT_INV, MM_F_ALL_CHAINS, OPT, reg

GOLDEN = os.path.join(PS.HERE, "golden", "align_post_edges")
PATCH_SC = (1, 3, 4)
SCENES = ("cover64_first", "cover64_none", "cover64_late", "cover_union", "sum64", "sum_wide", "nsub_term") + tuple("patch_sc%d" % m for m in PATCH_SC) + (
    "mapq_wrap", "sub_above_parent", "sub_above_parent_sr", "inv_wide", "inv_all_chains", "words", "lds_edge")
NO_PICK = dict(key=0, key_d=0, subsc=0, score0=0)
PICK_FIELDS = ("key", "key_d", "subsc", "score0")
PICK_LISTS = ("int",) + tuple("sc%d" % m for m in PATCH_SC)            # the integer list, then the dp_max list of each match_sc
NSUB_EDGE = 141264                                                      # n_sub + 1 = 141265: the first integer where a double add of .499f gives another term
INV_SIZES = (47, 48, 49, 64, 65, 66)
LDS_SIZES = (PS.AP_LDS_CAP - 1, PS.AP_LDS_CAP, PS.AP_LDS_CAP + 1)
WORDS_FINAL = 66


def with_cigar(rec, n_words):
    """The record with a CIGAR of n_words words, each carrying the low bits of the region's hash (its serial) and its own place."""
    r, x, _ = rec
    tag = int(r["hash"]) & 0x7ffff
    cig = np.array([tag << 13 | k << 4 | k % 3 for k in range(n_words)], np.uint32)
    x = x.copy()
    x["has_extra"], x["n_cigar"] = 1, n_words
    return r, x, cig


# ---- mm_set_parent: a region H, ranked last, that overlaps 64 / 65 primaries

def _disjoint_cover(k):
    """k primaries of 98 bases, 100 apart, and H over all of them: 1 - uncov / |H| is 0.98 with all k counted, 0.965 with 64 of 65."""
    pri = [reg(100 * j, 100 * j + 98, 1000, dp_max=1000, cnt=20) for j in range(k)]
    return pri + [reg(0, 100 * k, 900, dp_max=995, cnt=10)]


def _staggered(n_left, n_right, after=0):
    """n_left + n_right primaries of 700 bases, 20 apart, over the two ends of H (each fails against its neighbour: 680/700 - 20/700 is
    below the 0.95 of these scenes, and overlaps H by at most 640), then P, which contains H, then `after` primaries that overlap H and
    fail against all of these; H last.  H passes at P alone: at rank n_left + n_right."""
    E = 4000
    left = [reg(20 * j, 20 * j + 700, 1000 - j, dp_max=2000, cnt=20) for j in range(n_left)]
    right = [reg(E - 20 * j - 700, E - 20 * j, 900 - j, dp_max=1800, cnt=20) for j in range(n_right)]
    P = [reg(0, E, 800, dp_max=1000, cnt=20)]
    X = [reg(E - 700, E + 3000, 700, dp_max=1400, cnt=20)][:after]
    H = [reg(680, E - 680, 700, dp_max=996, cnt=10)]
    return left + right + P + X + H


def _cover64_late():
    return [(0, _staggered(32, 31)), (0, _staggered(32, 31, after=1)), (0, _staggered(32, 32))]        # P at rank 63 of 64, 63 of 65, 64 of 65


def _cover_union():
    far = lambda: reg(5000, 6000, 300)
    return [
        (0, [reg(0, 1000, 1000), reg(600, 1600, 900), reg(500, 2400, 800)]),        # clipped to 500..1000 and 600..1600: the starts differ
        (0, [reg(0, 1000, 1000), reg(600, 1600, 900), reg(700, 2400, 800)]),        # clipped to 700..1000 and 700..1600: one start, two ends
        (0, [reg(0, 1000, 1000), reg(0, 2100, 900), far()]),                        # 1 - 1100/2100 < 0.5
        (0, [reg(0, 1000, 1000), reg(0, 2000, 900), far()]),                        # 1 - 1000/2000 == mask_level: the strict > decides
    ]


# ---- sum_sc and uniq_ratio

def _sum64():
    row = lambda n: [reg(100 * k, 100 * k + 90, 150 if k < 64 else 3000, score0=60, as_=3 * k) for k in range(n)]
    return [(9600, row(64)), (9600, row(65))]


def _sum_wide():
    three = lambda: [reg(2000 * k, 2000 * k + 1000, 1 << 30, dp_max=1000 + k, score0=42) for k in range(3)]
    odd = [reg(0, 1000, 1 << 23, dp_max=1000, score0=42), reg(2000, 3000, (1 << 23) + 1, dp_max=1001, score0=42)]
    return [(0, three()), (1 << 30, three()), ((1 << 23) + 1, odd)]


# ---- the n_sub term and the patch lists

def _nsub_term(pk):
    one = lambda **kw: [reg(0, 1000, 1000, has_extra=0, **kw)]
    reads = [(0, one(n_sub=NSUB_EDGE - 1, score0=53)), (0, one(n_sub=NSUB_EDGE, score0=53))]
    if pk["key"]:
        reads += [(0, one(n_sub=pk["key"] - 1, score0=49)), (0, [reg(0, 1000, pk["key"], has_extra=0, score0=45)]),
                  (0, [reg(0, 1000, pk["key"] + 1, has_extra=0, score0=45)])]
    if pk["key_d"] and pk["subsc"]:
        reads += [(0, [reg(0, 1000, pk["key_d"] + d, has_extra=0, subsc=pk["subsc"], score0=pk["score0"])]) for d in (1, 0)]      # the key after it, then the key
    return reads


def _patch_sc(pk):
    reads = PS._patch(pk["key"] or 1000)
    if pk["key_d"] and pk["subsc"]:
        reads += [(0, [reg(0, 1000, 500, dp_max=pk["key_d"] + d, subsc=pk["subsc"], score0=pk["score0"])]) for d in (1, 0)]       # the key after it, then the key
    return reads


# ---- the mapq subtraction

def _mapq_wrap():
    cases = [dict(score=1000, mlen=700, blen=0), dict(score=1000, score0=0), dict(score=1000, mlen=0, blen=0), dict(score=1000, dp_max=0), dict(score=1000, dp_max=-5),
             dict(score=0, has_extra=0), dict(score=-3, has_extra=0)]
    return [(0, [reg(0, 1000, n_sub=n_sub, **c)]) for c in cases for n_sub in (1, 0)]


def _sub_above_parent():
    return [
        (0, [reg(0, 1000, 1000, dp_max=1000, cnt=4, score0=2000), reg(10, 990, 900, dp_max=1500, cnt=2)]),     # counted by dp_max alone: cnt 2 < 4
        (0, [reg(0, 1000, 1000, dp_max=1000, cnt=4, score0=2000), reg(10, 990, 900, dp_max=1500, cnt=4)]),     # ... and by cnt as well
        (0, [reg(0, 1000, 1000, dp_max=1000, cnt=4, score0=2000), reg(10, 990, 900, dp_max=1009, cnt=2), reg(20, 980, 880, dp_max=990, cnt=2)]),
    ]


# ---- mm_set_inv_mapq

def _inv_row(n, at, rank):
    """n regions: n - 1 disjoint primaries of different mapq in `as` order and one inversion, at input place `at`, `rank`-th in (as, i)."""
    pri = [reg(100 * k, 100 * k + 90, 30 + 7 * k % 40, score0=80, as_=4 * k) for k in range(n - 1)]
    inv = reg(100 * rank - 10, 100 * rank, 0, dp_max=90, cnt=0, as_=4 * rank - 2, bits=BIT_INV)
    return pri[:at] + [inv] + pri[at:]


def _inv_wide():
    iv = dict(cnt=0, bits=BIT_INV)
    pri = lambda k, as_: reg(100 * k, 100 * k + 90, 30 + 7 * k % 40, score0=80, as_=as_)
    reads = [(0, _inv_row(n, n // 2, n - 2)) for n in INV_SIZES]                                        # (a): rank 63 of 65 regions, 64 of 66
    # (b): region 0 and the inversion, region 64, have one `as`, between those of regions 32 and 33: the index puts region 0 first
    tie = [reg(0, 90, 69, score0=80, as_=130)] + [pri(k, 4 * k) for k in range(1, 64)] + [reg(6390, 6400, 0, dp_max=90, as_=130, **iv)] + [pri(k, 4 * k) for k in (64, 65)]
    reads.append((0, tie))
    reads.append((0, [reg(0, 1000, 60, score0=80, as_=0), reg(100, 200, 0, dp_max=90, as_=10, **iv), reg(1100, 2000, 45, score0=80, as_=30),
                      reg(1000, 1100, 0, dp_max=95, as_=15, **iv)]))                                    # (c): the first inversion is a secondary
    reads.append((0, [reg(0, 1000, 60, score0=80, as_=-5), reg(1000, 1100, 0, dp_max=90, as_=10, **iv), reg(1100, 2000, 45, score0=80, as_=0)]))   # (d)
    return reads


def _inv_all_chains():
    iv = dict(cnt=0, bits=BIT_INV)
    return [(0, [reg(0, 1000, 60, score0=80, as_=0, id_=0, parent=0), reg(3000, 3500, 50, score0=80, as_=10, id_=1, parent=-1),
                 reg(1000, 1100, 0, dp_max=90, as_=20, id_=2, parent=2, **iv), reg(1100, 2000, 45, score0=80, as_=30, id_=3, parent=3)])]   # (e)


# ---- records out

def _words():
    n_in = 1 + (WORDS_FINAL - 1) * 3 // 2                               # one primary and secondaries of which every third goes: 66 stay
    recs, slot = [reg(0, 10000, 5000)], 0
    for k in range(1, n_in):
        dropped = k % 3 == 0
        slot += not dropped
        wide = not dropped and 62 <= slot <= 65
        rec = reg(10 + k, 9900 - k, 100 if dropped else 4990 - 10 * k, has_extra=1 if wide or k % 7 != 5 else 0)
        recs.append(with_cigar(rec, 64 + slot % 2) if wide else rec)
    assert slot == WORDS_FINAL - 1
    alone = [reg(0, 1000, 1000)] + [reg(10 + k, 990 - k, 100) for k in range(4)]
    return [(0, recs), (0, alone), (0, [with_cigar(reg(0, 1000, 500), 64)]), (0, [with_cigar(reg(0, 1000, 500), 65)])]


def _lds_edge():
    def one(n):
        row = PS._row(n - 2)
        return [row[0], reg(5, 80, 290)] + row[1:] + [reg(105, 180, 10)]     # a kept secondary (dp_max2 of primary 0), a dropped one (of primary 1)
    return [(n % 3, one(n)) for n in LDS_SIZES]


def scene(name, picks=None):
    """dict(name, opt, lds_cap, reads = [(rep_len, [records])]).  picks: {list name: dict of PICK_FIELDS}."""
    picks = picks or {}
    pk = lambda k: dict(NO_PICK, **picks.get(k, {}))
    PS._serial[0] = 1000 * (20 + SCENES.index(name))
    opt = {}
    if name.startswith("patch_sc"):
        m = int(name[len("patch_sc"):])
        reads, opt = _patch_sc(pk("sc%d" % m)), dict(match_sc=m)
    elif name == "nsub_term":
        reads = _nsub_term(pk("int"))
    else:
        reads, opt = dict(
            cover64_first=(lambda: [(0, _disjoint_cover(64)), (0, _disjoint_cover(65))], dict(mask_level=0.97)),
            cover64_none=(lambda: [(0, _disjoint_cover(64)), (0, _disjoint_cover(65))], dict(mask_level=0.99)),
            cover64_late=(_cover64_late, dict(mask_level=0.95)),
            cover_union=(_cover_union, {}), sum64=(_sum64, {}), sum_wide=(_sum_wide, {}), mapq_wrap=(_mapq_wrap, {}),
            sub_above_parent=(_sub_above_parent, {}), sub_above_parent_sr=(_sub_above_parent, dict(is_sr=1)),
            inv_wide=(_inv_wide, {}), inv_all_chains=(_inv_all_chains, dict(flag=MM_F_ALL_CHAINS)),
            words=(_words, dict(best_n=100)), lds_edge=(_lds_edge, {}))[name]
        reads = reads()
    return dict(name=name, opt=dict(OPT, **opt), lds_cap=PS.AP_LDS_CAP, reads=reads)


def picks_row(picks):
    return np.array([[int(dict(NO_PICK, **picks.get(l, {}))[f]) for f in PICK_FIELDS] for l in PICK_LISTS], np.int64)


def picks_of(row):
    return {l: dict(zip(PICK_FIELDS, (int(v) for v in row[i]))) for i, l in enumerate(PICK_LISTS)}


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}
