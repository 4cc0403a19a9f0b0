"""Named scenes of synthetic aligned regions for Device.align_post (chaindp_align_post_regs): each record is a region, its extra and a
short CIGAR no other region has, so that a misplaced word shows.  Every size is the smallest at which its case can occur.  The goldens
tests/golden/align_post/*.npz (tests/golden/make_apost_golden.py) hold what the compiled reference makes of them; tests/apost_model.py
restates it.  The real scenes (alignments of skeleton_shapes and align_reads_shapes) are listed here too: their inputs are those
goldens' own, with a seeded rep_len per read.

The first region of a read is always its own parent, so mm_select_sub never drops it: the places a dropped region can have are the
second, a middle one and the last."""
import os

import numpy as np

from align_shapes import EXTRA_DTYPE, REG_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_post")
MM_F_ALL_CHAINS = 0x800000
BIT_REV, BIT_INV = 1 << 10, 1 << 11
AP_LDS_CAP = 48                     # csrc/chaindp_apost_plan.h
SCENE_CAP = 5                       # the lowered cap of the "lds_cap" scene: lists of 5 stay in LDS, lists of 6 do not
OPT_FIELDS = ("flag", "mask_level", "pri_ratio", "best_n", "min_diff", "sub_diff", "max_join_long", "max_join_short", "min_join_flank_sc", "min_cnt",
              "min_chain_score", "match_sc", "is_sr")
OPT = dict(flag=0, mask_level=0.5, pri_ratio=0.8, best_n=5, min_diff=30, sub_diff=8, max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000,
           min_cnt=3, min_chain_score=40, match_sc=2, is_sr=0)
SYNTHETIC = ("structure", "keeps_all", "best1", "all_chains", "mapq", "mapq_sr", "inv", "sizes", "lds_cap", "patch")
REAL = ("skeleton_asm", "skeleton_filters", "skeleton_fuzz", "skeleton_inv_edges", "skeleton_rounds", "skeleton_zdrop_to_the_end", "reads_trips", "reads_lds_cap")
PATCH_MATCH_SC = 2

_serial = [0]


def reg(qs, qe, score, dp_max=None, rs=None, rid=0, cnt=20, score0=None, subsc=0, n_sub=0, as_=0, mlen=None, blen=None, bits=0, has_extra=1, parent=-1, id_=-1):
    """One record: (region, extra, cigar).  rs defaults to 10 * qs, re = rs + (qe - qs); mlen, blen to 9/10 and all of the span."""
    _serial[0] += 1
    r, x = np.zeros(1, REG_DTYPE), np.zeros(1, EXTRA_DTYPE)
    rs = 10 * qs if rs is None else rs
    r["id"], r["parent"], r["cnt"], r["rid"], r["score"], r["qs"], r["qe"], r["rs"], r["re"] = id_, parent, cnt, rid, score, qs, qe, rs, rs + (qe - qs)
    r["subsc"], r["as"], r["n_sub"], r["score0"] = subsc, as_, n_sub, score if score0 is None else score0
    r["mlen"], r["blen"] = (qe - qs) * 9 // 10 if mlen is None else mlen, qe - qs if blen is None else blen
    r["bits"], r["hash"], r["div"] = bits, 0x9e3779b1 * _serial[0] & 0xffffffff, np.float32(0.01 * (_serial[0] % 7))
    # (reserved stays 0: in the reference these eight bytes are the pointer p, which no golden records)
    cig = np.array([(100 + _serial[0]) << 4 | k % 3 for k in range(1 + _serial[0] % 3)], np.uint32) if has_extra else np.zeros(0, np.uint32)
    x["has_extra"], x["dp_score"], x["dp_max"], x["n_ambi"], x["n_cigar"] = has_extra, (2 * score if dp_max is None else dp_max) - 3, 2 * score if dp_max is None else dp_max, _serial[0] % 4, len(cig)
    if not has_extra:
        x[:] = 0
    return r[0], x[0], cig


def _structure():
    return [
        (7, [reg(0, 1000, 1000), reg(100, 900, 100)]),                            # the first read of the batch drops: pri_ratio, the last region
        (0, []),                                                                     # a read without regions
        (3, [reg(0, 500, 400)]),                                                     # one region
        (5, [reg(0, 1000, 900, dp_max=1800, rs=5000), reg(0, 1000, 900, dp_max=1800, rs=5000)]),     # identical after DP: no dp_max2; and dropped as identical
        (0, [reg(0, 1000, 900, dp_max=1000), reg(50, 1000, 880, dp_max=992, cnt=10)]),              # dp_max - dp_max == sub_diff: counts as a sub
        (0, [reg(0, 1000, 900, dp_max=1000), reg(50, 1000, 880, dp_max=991, cnt=10)]),              # sub_diff + 1: does not
        (9, [reg(0, 1000, 100), reg(20, 990, 75)]),                                  # 75 < 0.8 * 100, saved by min_diff
        (2, [reg(0, 1000, 1000), reg(10, 990, 100), reg(20, 980, 900), reg(2000, 3000, 800)]),       # dropped second of four
        (2, [reg(0, 1000, 1000), reg(10, 990, 900), reg(20, 980, 100), reg(30, 970, 880), reg(2000, 3000, 800)]),   # dropped in the middle
        # mm_select_sub reads a slot a later region has moved into: r[1] goes, r[2] (primary) moves to slot 1, r[3]'s parent is 2
        (2, [reg(0, 1000, 1000), reg(10, 990, 100), reg(2000, 3000, 500), reg(2010, 2990, 450), reg(2020, 2980, 100)]),
        (1, [reg(0, 1000, 1000), reg(100, 900, 100)]),                            # the last read of the batch drops
    ]


def _keeps_all():
    return [(4, [reg(0, 1000, 1000), reg(10, 990, 900)]), (0, [reg(0, 300, 200), reg(400, 800, 300), reg(900, 1500, 500)]), (2, [reg(0, 100, 80)])]


def _best1():
    return [(0, [reg(0, 1000, 1000), reg(10, 990, 950), reg(20, 980, 940), reg(30, 970, 930)])]


def _all_chains():
    return [(3, [reg(0, 1000, 1000, id_=0, parent=0), reg(10, 990, 100, id_=1, parent=0), reg(2000, 2500, 300, id_=2, parent=2, as_=40)]),
            (0, [reg(0, 1000, 500, id_=0, parent=0, as_=0), reg(1100, 2000, 600, id_=1, parent=1, as_=30), reg(1000, 1100, 0, cnt=0, dp_max=90, bits=BIT_INV, id_=2, parent=2)]),
            (0, [])]


def _mapq():
    return [
        (0, [reg(0, 1000, 1000), reg(2000, 3000, 800, has_extra=0), reg(10, 990, 900, has_extra=0)]),           # has_extra 0 and 1 in one read; p == NULL primary
        (0, [reg(0, 1000, 1000, dp_max=1000), reg(10, 990, 900, dp_max=990)]),                                   # dp_max2 > 0: the alternative is lower
        (0, [reg(0, 1000, 1000, dp_max=1000), reg(10, 990, 900, dp_max=100)]),                                   # ... higher; and the clamp at 60
        (0, [reg(0, 1000, 1000)]),                                                                               # p, dp_max2 == 0
        (0, [reg(0, 1000, 1000, score0=40)]),                                                                    # x == 1: mapq 0 -> 1
        (0, [reg(0, 1000, 50, n_sub=5000, has_extra=0)]),                                                        # the n_sub term is larger: negative -> 0
        (0, [reg(0, 1000, 1000, mlen=700, blen=0)]),                                                             # blen == 0: a float outside the int range
        (0, [reg(0, 1000, 90, cnt=30), reg(2000, 2600, 60, cnt=30)]),                                            # rep_len 0 ...
        (150, [reg(0, 1000, 90, cnt=30), reg(2000, 2600, 60, cnt=30)]),                                          # ... and sum_sc + rep_len = 2 sum_sc: another mapq
    ]


def _inv():
    iv = dict(cnt=0, as_=0, bits=BIT_INV)
    return [
        (0, [reg(0, 1000, 500), reg(1000, 1100, 0, dp_max=90, **iv)]),                                           # fewer than three regions
        (0, [reg(0, 1000, 500), reg(1100, 2000, 600, as_=30), reg(2100, 2500, 300, as_=60)]),                    # three, no inversion
        (2, [reg(0, 1000, 500, as_=0), reg(1100, 2000, 80, as_=30, cnt=5), reg(1000, 1100, 0, dp_max=90, **iv)]),   # (0, 0) (0, 2) (30, 1): between two primaries
        (0, [reg(0, 1000, 500, as_=7), reg(1100, 2000, 600, as_=30), reg(1000, 1100, 0, dp_max=90, **iv)]),      # as == 0 comes first in the order: untouched
        (0, [reg(0, 1000, 500, as_=0), reg(1100, 2000, 600, as_=0), reg(1000, 1100, 0, dp_max=90, **iv)]),       # every as == 0: the inversion is last
        (0, [reg(0, 1000, 500, as_=0), reg(1000, 1100, 0, dp_max=90, **iv), reg(1100, 1200, 0, dp_max=95, **iv), reg(1300, 2000, 70, as_=30, cnt=4)]),   # two inversions side by side
    ]


def _row(n, k0=0, score=lambda k: 300 + k):
    return [reg(100 * k, 100 * k + 90, score(k), as_=3 * k) for k in range(k0, k0 + n)]


def _sizes():
    many = [reg(0, 6400, 5000)] + [reg(10 + k, 6300 - k, 4990 - 10 * k if k % 3 else 100) for k in range(64)]     # 65 regions, one primary, every third secondary dropped
    return [(0, _row(64)), (1, _row(65)), (2, many), (0, _row(2) + [reg(5, 80, 200)] + _row(62, 2))]


def _lds_cap():
    return [(0, _row(SCENE_CAP)), (0, _row(SCENE_CAP + 1)), (3, _row(SCENE_CAP - 1) + [reg(5, 80, 10)]), (3, _row(SCENE_CAP) + [reg(5, 80, 10)])]


def _patch(dp_max):
    return [(0, [reg(0, 1000, 500, dp_max=dp_max)]), (0, [reg(0, 1000, 500, dp_max=dp_max), reg(10, 990, 450, dp_max=dp_max - 20)])]


def scene(name, patch_dp_max=1000):
    """dict(name, opt, lds_cap, reads = [(rep_len, [records])])."""
    _serial[0] = 1000 * SYNTHETIC.index(name)
    reads = dict(structure=_structure, keeps_all=_keeps_all, best1=_best1, all_chains=_all_chains, mapq=_mapq, mapq_sr=_mapq, inv=_inv, sizes=_sizes,
                 lds_cap=_lds_cap, patch=lambda: _patch(int(patch_dp_max)))[name]()
    opt = dict(OPT, **dict(best1=dict(best_n=1), all_chains=dict(flag=MM_F_ALL_CHAINS), mapq_sr=dict(is_sr=1), patch=dict(match_sc=PATCH_MATCH_SC)).get(name, {}))
    return dict(name=name, opt=opt, lds_cap=SCENE_CAP if name == "lds_cap" else AP_LDS_CAP, reads=reads)


def opt_row(opt):
    return np.array([float(opt[k]) for k in OPT_FIELDS], np.float64)


def opt_of(row):
    return {k: (float(v) if k in ("mask_level", "pri_ratio") else int(v)) for k, v in zip(OPT_FIELDS, row)}


def post_opt(row):
    """params.PostOpt of a recorded opt row."""
    from minimap2_chaindp_amd import params
    return params.PostOpt(**opt_of(row))


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)


def pack(sc):
    """A scene's flat inputs: opt (row of OPT_FIELDS), lds_cap, rep_len, regs_off, regs, extra, cigar_off, cigar."""
    recs = [x for _, rd in sc["reads"] for x in rd]
    cat = lambda parts, dt: np.array(parts, dt) if len(parts) else np.zeros(0, dt)
    cigs = [c for _, _, c in recs]
    return dict(opt=opt_row(sc["opt"]), lds_cap=np.int64(sc["lds_cap"]), rep_len=np.array([rl for rl, _ in sc["reads"]], np.int32),
                regs_off=offsets([len(rd) for _, rd in sc["reads"]]), regs=cat([r for r, _, _ in recs], REG_DTYPE), extra=cat([x for _, x, _ in recs], EXTRA_DTYPE),
                cigar_off=offsets([len(c) for c in cigs]), cigar=np.concatenate(cigs).astype(np.uint32) if cigs else np.zeros(0, np.uint32))


INPUTS = ("opt", "lds_cap", "rep_len", "regs_off", "regs", "extra", "cigar_off", "cigar")


def load(name):
    """A scene's golden; a scene of the edge tier (apost_edge_shapes.py) loads by the same call from its own directory."""
    path = os.path.join(GOLDEN, name + ".npz")
    with np.load(path if os.path.exists(path) else os.path.join(HERE, "golden", "align_post_edges", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def real_source(name):
    """The golden a real scene's alignment inputs come from: (module's load function, its name there)."""
    kind, _, sub = name.partition("_")
    if kind == "skeleton":
        from test_skeleton_cpu import load as load_skeleton
        return load_skeleton, sub
    import align_reads_shapes as RS
    return RS.load, sub


def real_rep_len(name, n_reads):
    """The seeded rep_len of a real scene: a third of the reads 0, the others up to 400."""
    rng = np.random.default_rng(REAL.index(name) + 77)
    return np.where(rng.integers(0, 3, n_reads) == 0, 0, rng.integers(1, 401, n_reads)).astype(np.int32)


def real_opt(align_opt_row):
    """The tail's options that go with a real scene's alignment options (align_model.OPT_FIELDS): match_sc = a, sub_diff = 2 a + b,
    min_diff = 2 k, its min_chain_score."""
    a, b, k, mcs = int(align_opt_row[0]), int(align_opt_row[1]), int(align_opt_row[16]), int(align_opt_row[11])
    return dict(OPT, match_sc=a, sub_diff=2 * a + b, min_diff=2 * k, min_chain_score=mcs)
