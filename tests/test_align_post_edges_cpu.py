"""CPU proof of the align-post edge tier: the goldens tests/golden/align_post_edges/*.npz (tests/golden/make_apost_edge_golden.py, from
the unmodified reference) load, are the scenes of tests/apost_edge_shapes.py, are reproduced by tests/apost_model.py and reach every
class of its EDGE_COVER; chaindp.align_post_check accepts them.  Then, edge by edge, a subtly wrong restatement of the step -- written
here, with the right one beside it -- gives the reference's words below the edge and other words on or above it; where a flavour
cannot tell the two apart, a test says so."""
import contextlib
import glob
import os

import numpy as np
import pytest

import apost_edge_shapes as E
import apost_model as M
import apost_shapes as PS
import post_oracle as po
from post_oracle import BIT_INV, F32, INT_MIN, _cvtt, _wrap32, host_logf
from test_align_post_cpu import inputs, same


def picks():
    return E.picks_of(E.load("nsub_term")["picks"])


def mapq_of(out, rd):
    o = out["regs_off_out"] if "regs_off_out" in out else out["regs_off"]
    regs = out["regs_out"] if "regs_out" in out else out["regs"]
    return (regs["bits"][int(o[rd]):int(o[rd + 1])] & 0xff).tolist()


# ---------------------------------------------------------------- the goldens

def test_fixtures_are_there_and_small():
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(E.GOLDEN, "*.npz")))
    assert files == sorted(E.SCENES)
    assert all(os.path.getsize(os.path.join(E.GOLDEN, n + ".npz")) < 1 << 20 for n in files)


def test_shapes_are_what_was_recorded():
    pk = E.load(E.SCENES[0])["picks"]
    for name in E.SCENES:
        g = E.load(name)
        assert same(g["picks"], pk), name                                         # one set of picks for all files
        p = PS.pack(E.scene(name, E.picks_of(g["picks"])))
        for k in PS.INPUTS:
            assert same(np.asarray(p[k]), g[k]), (name, k)
        assert int(g["lds_cap"]) == PS.AP_LDS_CAP


def test_model_reproduces_the_reference_and_reaches_every_edge_class():
    M.cover.clear()
    for name in E.SCENES:
        g, *args = inputs(name)
        got = M.run(*args)
        for k in M.OUTPUTS:
            assert same(got[k], g[k + "_out"]), (name, k)
    assert not [k for k in M.EDGE_COVER if not M.cover[k]], dict(M.cover)


def test_debug_check_accepts_the_scenes():
    from minimap2_chaindp_amd import chaindp
    for name in E.SCENES:
        g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
        assert chaindp.align_post_check(PS.post_opt(g["opt"]), rep_len, regs_off, regs, extra, cigar_off, cigar) == (0, len(regs), len(cigar)), name


def test_picked_keys_are_on_this_hosts_lists():
    """The goldens' logarithms are the generating host's; the keys it picked are listed here too, or the test says which are not."""
    from minimap2_chaindp_amd import chaindp
    pk = picks()
    lists = {"int": chaindp.post_logf_patches()[0]}
    lists.update({"sc%d" % m: chaindp.apost_logf_patches(m)[0] for m in E.PATCH_SC})
    for l in E.PICK_LISTS:
        print("list", l, "recorded picks", pk[l], "; on this host's list of", len(lists[l]), ":", [int(k) for k in (pk[l]["key"], pk[l]["key_d"]) if k in lists[l]])
        assert pk[l]["key"] > 0 or len(lists[l][lists[l] >= 100]) == 0
        if pk[l]["key"] and len(lists[l]):
            assert pk[l]["key"] >= 100 and pk[l]["key_d"] >= pk[l]["key"]


# ---------------------------------------------------------------- the restatements: right with every flag off, wrong with one on

@np.errstate(all="ignore")
def restated_set_parent(r, has_p, dp_max, dp_max2, mask_level, sub_diff, first64=False, no_tie_in_union=False, ge=False):
    """mm_set_parent with r->p as k_apost_read states it: the overlapping primaries collected in w order, the union counted interval by
    interval against the ones before it in (start, end, place) order, the first that passes.
      first64           only the first 64 primaries are looked at (one ballot round)
      no_tie_in_union   an interval sees only those that start before it: equal starts are both counted in full
      ge                >= for the mask test"""
    n = len(r)
    if n <= 0:
        return
    r["id"] = np.arange(n)
    w = [0]
    r[0]["parent"] = 0
    ml = F32(mask_level)
    for i in range(1, n):
        si, ei = int(r[i]["qs"]), int(r[i]["qe"])
        cov = []
        for p in (w[:64] if first64 else w):
            sj, ej = int(r[p]["qs"]), int(r[p]["qe"])
            if not (ej <= si or sj >= ei):
                cov.append((p, max(sj, si), min(ej, ei)))
        found, ol = -1, 0
        if cov:
            covered = 0
            for j, (_, s, e) in enumerate(cov):
                m = s
                for l, (_, sl, el) in enumerate(cov):
                    before = sl < s if no_tie_in_union else (sl < s or (sl == s and (el < e or (el == e and l < j))))
                    if before:
                        m = max(m, el)
                if e > m:
                    covered += e - m
            uncov = (ei - si) - covered
            for p, _, _ in cov:
                sj, ej = int(r[p]["qs"]), int(r[p]["qe"])
                mn, mx = min(ej - sj, ei - si), max(ej - sj, ei - si)
                ol = (0 if ei < sj else ei - sj if ei < ej else ej - sj) if si < sj else (0 if ej < si else ej - si if ej < ei else ei - si)
                v = F32(ol) / F32(mn) - F32(uncov) / F32(mx)
                if (v >= ml) if ge else (v > ml):
                    found = p
                    break
        if found >= 0:
            rp = r[found]
            r[i]["parent"] = rp["parent"]
            rp["subsc"] = max(int(rp["subsc"]), int(r[i]["score"]))
            cnt_sub = bool(r[i]["cnt"] >= rp["cnt"])
            if has_p[found] and has_p[i] and (rp["rid"] != r[i]["rid"] or rp["rs"] != r[i]["rs"] or rp["re"] != r[i]["re"] or ol != mn):
                dp_max2[found] = max(int(dp_max2[found]), int(dp_max[i]))
                if _wrap32(int(dp_max[found]) - int(dp_max[i])) <= sub_diff:
                    cnt_sub = True
            if cnt_sub:
                rp["n_sub"] += 1
        else:
            w.append(i)
            r[i]["parent"] = i
            r[i]["n_sub"] = 0


def device_logf(x):
    """(float)log((double)x): what the device computes where no list patches it."""
    return F32(np.log(np.float64(F32(x))))


@np.errstate(all="ignore")
def restated_set_mapq(r, has_p, dp_max, dp_max2, min_chain_sc, match_sc, rep_len, is_sr, sum64=False, sum_i32=False, double_add=False, no_patch=False,
                      saturate=False, inv_first64=False, inv_no_tie=False):
    """mm_set_mapq and mm_set_inv_mapq as k_apost_read states them.
      sum64        sum_sc over the first 64 slots (one lane stride)        sum_i32      sum_sc in int32
      double_add   the n_sub term's .499f added in double                  no_patch     logf without the patch lists
      saturate     a mapq - sub that stops at INT_MIN                      inv_first64  only slots 0..63 are ranked
      inv_no_tie   equal `as` are not ordered by the region index (here: the later region first)"""
    n = len(r)
    logf = device_logf if no_patch else host_logf
    sum_sc = int(sum(int(x["score"]) for x in (r[:64] if sum64 else r) if x["parent"] == x["id"]))
    if sum_i32:
        sum_sc = _wrap32(sum_sc)
    uniq_ratio = F32(sum_sc) / F32(sum_sc + rep_len)
    for i, x in enumerate(r):
        bits, mq = int(x["bits"]), 0
        if not bits & BIT_INV and x["parent"] == x["id"]:
            score, cnt = int(x["score"]), int(x["cnt"])
            pen_s1 = (F32(1.0) if score > 100 else F32(0.01) * F32(score)) * uniq_ratio
            pen_cm = F32(1.0) if cnt > 10 else F32(0.1) * F32(cnt)
            pen_cm = pen_s1 if pen_s1 < pen_cm else pen_cm
            subsc = max(int(x["subsc"]), min_chain_sc)
            p, dm, d2 = bool(has_p[i]), int(dp_max[i]), int(dp_max2[i])
            lg = logf(F32(dm) / F32(match_sc)) if p else logf(score)
            if p and d2 > 0 and dm > 0:
                identity = F32(int(x["mlen"])) / F32(int(x["blen"]))
                xx = F32(d2) * F32(subsc) / F32(dm) / F32(int(x["score0"]))
                mapq = _cvtt(identity * pen_cm * F32(40.0) * (F32(1.0) - xx * xx) * lg)
                if not is_sr:
                    alt = _cvtt(F32(6.02) * identity * identity * F32(dm - d2) / F32(match_sc) + F32(.499))
                    mapq = mapq if mapq < alt else alt
            else:
                xx = F32(subsc) / F32(int(x["score0"]))
                identity = F32(int(x["mlen"])) / F32(int(x["blen"])) if p else F32(1.0)
                mapq = _cvtt(identity * pen_cm * F32(40.0) * (F32(1.0) - xx) * lg) if p else _cvtt(pen_cm * F32(40.0) * (F32(1.0) - xx) * lg)
            term = F32(4.343) * logf(int(x["n_sub"]) + 1)
            sub = int(np.float64(term) + np.float64(F32(.499))) if double_add else _cvtt(term + F32(.499))
            mapq = max(mapq - sub, INT_MIN) if saturate else _wrap32(mapq - sub)
            mq = min(max(mapq, 0), 60)
            if p and dm > d2 and mq == 0:
                mq = 1
        x["bits"] = (bits & ~0xff) | (mq & 0xff)
    if n < 3 or not any(int(x["bits"]) & BIT_INV for x in r):
        return
    ranked = [i for i in range(64 if inv_first64 else n)[:n] if r[i]["parent"] == i or r[i]["parent"] < 0]
    aux = sorted(ranked, key=lambda i: (int(np.uint32(r[i]["as"])), -i if inv_no_tie else i))
    for j in range(1, len(aux) - 1):
        v = r[aux[j]]
        if int(v["bits"]) & BIT_INV:
            v["bits"] = (int(v["bits"]) & ~0xff) | min(int(r[aux[j - 1]]["bits"]) & 0xff, int(r[aux[j + 1]]["bits"]) & 0xff)


@contextlib.contextmanager
def restated(**flags):
    """apost_model with the two steps above in the place of its own, the given flags on."""
    pf = {k: v for k, v in flags.items() if k in ("first64", "no_tie_in_union", "ge")}
    mf = {k: v for k, v in flags.items() if k not in pf}
    keep = M.set_parent, M.set_mapq
    M.set_parent = lambda *a: restated_set_parent(*a, **pf)
    M.set_mapq = lambda *a: restated_set_mapq(*a, **mf)
    try:
        yield
    finally:
        M.set_parent, M.set_mapq = keep


def reads_equal(name, **flags):
    """Per read of the scene: whether the restatement with these flags gives every recorded word."""
    g, opt, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
    res = []
    with restated(**flags):
        for rd in range(len(rep_len)):
            g0, g1 = int(regs_off[rd]), int(regs_off[rd + 1])
            o0, o1 = int(g["regs_off_out"][rd]), int(g["regs_off_out"][rd + 1])
            out, ex, d2, cigs = M.post_read(opt, int(rep_len[rd]), regs[g0:g1], extra[g0:g1], [cigar[int(cigar_off[q]):int(cigar_off[q + 1])] for q in range(g0, g1)])
            want = g["cigar_out"][int(g["cigar_off_out"][o0]):int(g["cigar_off_out"][o1])]
            res.append(same(out, g["regs_out"][o0:o1]) and same(ex, g["extra_out"][o0:o1]) and same(d2, g["dp_max2_out"][o0:o1])
                       and same(np.concatenate(cigs + [np.zeros(0, np.uint32)]), want))
    return res


WRONG = {}            # edge -> (lower side equal, upper side different), filled below and checked at the end


def verdict(edge, lower_same, upper_differs):
    WRONG[edge] = (bool(lower_same), bool(upper_differs))
    assert lower_same, (edge, "the wrong restatement differs below the edge")
    assert upper_differs, (edge, "the scene on the edge does not tell the wrong restatement from the right one")


def test_the_right_restatement_reproduces_every_scene():
    """With every flag off the restatements here are the reference: what a flag changes is the flag's doing."""
    for name in E.SCENES:
        assert all(reads_equal(name)), name


# ---------------------------------------------------------------- apost_set_parent

def _h_values(name, rd):
    """The last region of a read against the primaries before it: (overlapping primaries in w order, the mask values, mask_level)."""
    g, opt, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
    r = regs[int(regs_off[rd]):int(regs_off[rd + 1])].copy()
    n = len(r)
    x = extra[int(regs_off[rd]):int(regs_off[rd + 1])]
    M.set_parent(r[:n - 1], x["has_extra"][:n - 1].astype(bool), x["dp_max"].astype(np.int64), np.zeros(n, np.int64), opt["mask_level"], opt["sub_diff"])
    w = [j for j in range(n - 1) if r[j]["parent"] == j]
    si, ei = int(r[n - 1]["qs"]), int(r[n - 1]["qe"])
    ov = [p for p in w if not (int(r[p]["qe"]) <= si or int(r[p]["qs"]) >= ei)]
    covered = np.zeros(ei - si, bool)
    for p in ov:
        covered[max(int(r[p]["qs"]), si) - si:min(int(r[p]["qe"]), ei) - si] = True
    uncov = int((~covered).sum())
    vals = []
    for p in ov:
        sj, ej = int(r[p]["qs"]), int(r[p]["qe"])
        ol = min(ej, ei) - max(sj, si)
        vals.append(F32(ol) / F32(min(ej - sj, ei - si)) - F32(uncov) / F32(max(ej - sj, ei - si)))
    return ov, vals, F32(opt["mask_level"])


@pytest.mark.parametrize("name,rd,k,rank", [("cover64_first", 0, 64, 0), ("cover64_first", 1, 65, 0), ("cover64_none", 0, 64, -1), ("cover64_none", 1, 65, -1),
                                             ("cover64_late", 0, 64, 63), ("cover64_late", 1, 65, 63), ("cover64_late", 2, 65, 64)])
def test_cover64_is_what_it_is_named_for(name, rd, k, rank):
    g = E.load(name)
    ov, vals, ml = _h_values(name, rd)
    assert len(ov) == k
    passing = [j for j, v in enumerate(vals) if v > ml]
    assert (passing[:1] == [rank]) if rank >= 0 else not passing
    if rank == 64:
        assert passing == [64]                                                    # the 64 primaries before it all fail
    assert min(abs(float(v) - float(ml)) for v in vals) > 1e-3
    o0, o1 = int(g["regs_off_out"][rd]), int(g["regs_off_out"][rd + 1])
    out, d2 = g["regs_out"][o0:o1], g["dp_max2_out"][o0:o1]
    assert len(out) == k + 1                                                      # H is kept by mm_select_sub
    H = out[-1]
    if rank >= 0:
        par = int(H["parent"])
        assert par == ov[rank] and H["id"] == k                                   # ... and its parent changed after DP: dp_max2 and, by sub_diff alone, n_sub
        assert d2[par] == g["extra_out"]["dp_max"][o0 + k] > 0 and out[par]["n_sub"] == 1 and H["cnt"] < out[par]["cnt"]
    else:
        assert H["parent"] == H["id"] == k and not d2.any()


def test_set_parent_over_the_first_64_primaries():
    first, late = reads_equal("cover64_first", first64=True), reads_equal("cover64_late", first64=True)
    verdict("set_parent: 64 / 65 overlapping primaries, the first passes (the union needs all 65)", first[0], not first[1])
    verdict("set_parent: 64 / 65 overlapping primaries, the one that passes is at rank 63 / 64", late[0], not late[2])


def test_cover64_none_and_rank_63_cannot_differ():
    """Looking at fewer primaries only lowers every mask value, and with the passing primary at rank 63 the 65th is neither it nor needed
    for the union (the passing one contains H): the first-64 restatement agrees on both sides, by construction."""
    assert all(reads_equal("cover64_none", first64=True)) and reads_equal("cover64_late", first64=True)[1]
    WRONG["set_parent: 64 / 65 overlapping primaries (none)"] = (True, False)
    WRONG["set_parent: 65 overlapping primaries, the one at rank 63 passes (none)"] = (True, False)


def test_cover_union_order_and_strict_mask():
    g = E.load("cover_union")
    par = [g["regs_out"]["parent"][int(o):int(o) + 3].tolist() for o in g["regs_off_out"][:-1]]
    assert par == [[0, 1, 1], [0, 1, 2], [0, 1, 2], [0, 1, 2]]                    # on each edge H stays a primary
    res = reads_equal("cover_union", no_tie_in_union=True)
    verdict("set_parent: the union of clipped intervals, different starts / one start and two ends", res[0], not res[1])
    assert all(res[2:])
    res = reads_equal("cover_union", ge=True)
    verdict("set_parent: the mask test below / exactly at mask_level", res[2], not res[3])
    assert all(res[:2])


# ---------------------------------------------------------------- sum_sc, uniq_ratio

def test_sum_sc_over_64_and_65_primaries():
    g = E.load("sum64")
    assert np.diff(g["regs_off_out"]).tolist() == [64, 65] and (g["regs_out"]["parent"] == g["regs_out"]["id"]).all()
    assert all(0 < q < 60 for rd in (0, 1) for q in mapq_of(g, rd))               # no mapq clamps
    assert mapq_of(g, 0) != mapq_of(g, 1)[:64]                                    # the primary at slot 64 moves the others' mapq
    res = reads_equal("sum64", sum64=True)
    verdict("mapq: sum_sc over 64 / 65 primaries", res[0], not res[1])


def test_sum_sc_beyond_int32():
    g = E.load("sum_wide")
    a, b, c = (mapq_of(g, rd) for rd in range(3))
    assert a != b and all(0 < q < 60 for q in a + b + c), (a, b, c)               # rep_len 0 / 2^30 with sum_sc = 3 * 2^30
    assert int(g["regs"]["score"][:3].astype(np.int64).sum()) == 3 << 30 and int(g["regs"]["score"][6:].astype(np.int64).sum()) == (1 << 24) + 1
    assert g["rep_len"][2] % 2 == 1
    res = reads_equal("sum_wide", sum_i32=True)
    verdict("mapq: sum_sc of 2^24 + 1 / of 3 * 2^30 in int32", res[2], not res[1])
    assert res[0]                                                                 # (with rep_len 0 the wrapped sum divides by itself: 1 either way)


# ---------------------------------------------------------------- the n_sub term and the patch lists

def test_nsub_term_float_add():
    g = E.load("nsub_term")
    assert g["regs"]["n_sub"][:2].tolist() == [E.NSUB_EDGE - 1, E.NSUB_EDGE] and not g["extra"]["has_extra"].any()
    assert all(0 < q[0] < 60 for q in (mapq_of(g, rd) for rd in range(len(g["rep_len"])))), [mapq_of(g, rd) for rd in range(len(g["rep_len"]))]
    term = lambda k: F32(4.343) * host_logf(k)
    for k, differ in ((E.NSUB_EDGE, False), (E.NSUB_EDGE + 1, True)):
        assert (int(np.float64(term(k)) + np.float64(F32(.499))) != _cvtt(term(k) + F32(.499))) == differ
    res = reads_equal("nsub_term", double_add=True)
    verdict("mapq: the n_sub term at n_sub + 1 = 141264 / 141265, .499f added in float", res[0], not res[1])
    assert all(res[2:])


def _listed(l):
    from minimap2_chaindp_amd import chaindp
    return set((chaindp.post_logf_patches() if l == "int" else chaindp.apost_logf_patches(int(l[2:])))[0].tolist())


@pytest.mark.parametrize("l", E.PICK_LISTS)
def test_logf_without_the_patch_list(l):
    pk = picks()[l]
    name = "nsub_term" if l == "int" else "patch_sc" + l[2:]
    g = E.load(name)
    if not pk["key_d"]:
        pytest.fail("no listed key of list %s moved a mapq on the generating host: the list cannot be proved needed" % l)
    n = len(g["rep_len"])
    lower, upper = n - 2, n - 1                                                   # the key after the listed one, then the listed one
    key = g["regs"]["score"] if l == "int" else g["extra"]["dp_max"]
    at = [int(g["regs_off"][rd]) for rd in (lower, upper)]
    assert [int(key[a]) for a in at] == [pk["key_d"] + 1, pk["key_d"]]
    listed = _listed(l)
    if pk["key_d"] not in listed or pk["key_d"] + 1 in listed:
        pytest.fail("this host's list %s differs from the generating host's at the picked key %d" % (l, pk["key_d"]))
    assert 0 < mapq_of(g, lower)[0] < 60 and 0 < mapq_of(g, upper)[0] < 60
    res = reads_equal(name, no_patch=True)
    verdict("mapq: logf beside / on a key of the patch list " + l, res[lower], not res[upper])


def test_patch_scenes_use_the_first_listed_key():
    pk = picks()
    for m in E.PATCH_SC:
        g = E.load("patch_sc%d" % m)
        assert PS.opt_of(g["opt"])["match_sc"] == m and g["extra"]["dp_max"][0] == g["extra"]["dp_max"][1] == (pk["sc%d" % m]["key"] or 1000)
    g = E.load("nsub_term")
    if pk["int"]["key"]:
        assert g["regs"]["n_sub"][2] + 1 == pk["int"]["key"] == g["regs"]["score"][3]


# ---------------------------------------------------------------- the mapq subtraction

def test_mapq_subtraction_wraps():
    g = E.load("mapq_wrap")
    q = [mapq_of(g, rd)[0] for rd in range(len(g["rep_len"]))]
    assert g["regs"]["n_sub"].tolist() == [1, 0] * 7
    assert q[0::2] == [60] * 7 and set(q[1::2]) <= {0, 1}, q                      # INT_MIN - 3 wraps to a large positive int; INT_MIN - 0 does not
    res = reads_equal("mapq_wrap", saturate=True)
    verdict("mapq: INT_MIN minus the n_sub term, n_sub 0 / 1", all(res[1::2]), not any(res[0::2]))


def test_sub_above_parent():
    for name in ("sub_above_parent", "sub_above_parent_sr"):
        g = E.load(name)
        o = g["regs_off_out"]
        x, d2, r = g["extra_out"], g["dp_max2_out"], g["regs_out"]
        for rd in (0, 1):
            assert d2[o[rd]] == 1500 > x["dp_max"][o[rd]] and r["n_sub"][o[rd]] == 1      # in read 0 by dp_max alone (cnt 2 < 4)
        assert g["regs"]["cnt"][:2].tolist() == [4, 2]
        q = [mapq_of(g, rd)[0] for rd in range(3)]
        assert (q[0] == 0) if name == "sub_above_parent" else (0 < q[0] < 60), q  # the alternative is negative; without it (is_sr) the mapq stands
    assert PS.opt_of(E.load("sub_above_parent_sr")["opt"])["is_sr"] == 1


# ---------------------------------------------------------------- mm_set_inv_mapq

def test_inv_wide_is_what_it_is_named_for():
    g = E.load("inv_wide")
    assert np.diff(g["regs_off"])[:6].tolist() == list(E.INV_SIZES) and np.array_equal(g["regs_off"], g["regs_off_out"])
    o, r = g["regs_off_out"], g["regs_out"]
    for rd, n in enumerate(E.INV_SIZES):                                          # (a): between two primaries of different mapq, the lower one taken
        rr = r[o[rd]:o[rd + 1]]
        order = sorted(range(n), key=lambda i: (int(np.uint32(rr["as"][i])), i))
        j = [k for k, i in enumerate(order) if rr["bits"][i] & BIT_INV]
        assert j == [n - 2]
        ml, mr = (int(rr["bits"][order[j[0] + d]]) & 0xff for d in (-1, 1))
        assert ml != mr and 0 < min(ml, mr) < 60 and int(rr["bits"][order[j[0]]]) & 0xff == min(ml, mr)
    rr = r[o[6]:o[7]]                                                             # (b)
    assert rr["as"][0] == rr["as"][64] and rr["as"][32] < rr["as"][0] < rr["as"][33] and rr["bits"][64] & BIT_INV
    assert int(rr["bits"][64]) & 0xff == min(int(rr["bits"][0]) & 0xff, int(rr["bits"][33]) & 0xff) > int(rr["bits"][32]) & 0xff > 0
    rr = r[o[7]:o[8]]                                                             # (c): a secondary inversion stays, has mapq 0, and is no neighbour
    assert rr["parent"].tolist() == [0, 0, 2, 3] and rr["bits"][1] & BIT_INV and int(rr["bits"][1]) & 0xff == 0
    assert int(rr["bits"][3]) & 0xff == min(int(rr["bits"][0]) & 0xff, int(rr["bits"][2]) & 0xff) > 0
    rr = r[o[8]:o[9]]                                                             # (d): as = -5 sorts last, unsigned
    assert rr["as"][0] < 0 and int(rr["bits"][1]) & 0xff == min(int(rr["bits"][0]) & 0xff, int(rr["bits"][2]) & 0xff) > 0
    g = E.load("inv_all_chains")                                                  # (e)
    rr = g["regs_out"]
    assert rr["parent"].tolist() == [0, -1, 2, 3] and [int(b) & 0xff for b in rr["bits"]][1:3] == [0, 0] and int(rr["bits"][0]) & 0xff > 0 < int(rr["bits"][3]) & 0xff


def test_inv_ranks_beyond_the_first_64():
    res = reads_equal("inv_wide", inv_first64=True)
    verdict("inv_mapq: 64 / 65 regions ranked", all(res[:4]), not res[4] and not res[5] and not res[6])
    res = reads_equal("inv_wide", inv_no_tie=True)
    verdict("inv_mapq: different / equal `as` across a lane stride", all(res[:6]), not res[6])


# ---------------------------------------------------------------- records out

def packed(cigs, carry=True, max_words=None):
    """A read's cigar_off and CIGAR words as the kernels lay them out: per 64-slot block a prefix of the lengths on top of what the blocks
    before carried, then each region's words copied to its offset.  carry False: nothing is carried; max_words: only so many words move."""
    lens = [len(c) for c in cigs]
    off, carried = [], 0
    for b in range(0, len(lens), 64):
        acc = 0
        for m in lens[b:b + 64]:
            off.append((carried if carry else 0) + acc)
            acc += m
        carried += acc
    words = np.zeros(sum(lens), np.uint32)
    for o, c in zip(off, cigs):
        m = len(c) if max_words is None else min(len(c), max_words)
        words[o:o + m] = c[:m]
    return np.array(off + [sum(lens)], np.int64), words


def _words_read(rd):
    g = E.load("words")
    o0, o1 = int(g["regs_off_out"][rd]), int(g["regs_off_out"][rd + 1])
    off = g["cigar_off_out"][o0:o1 + 1]
    return g, [g["cigar_out"][int(off[i]):int(off[i + 1])] for i in range(o1 - o0)], off - off[0], g["cigar_out"][int(off[0]):int(off[-1])]


def test_words_is_what_it_is_named_for():
    g, cigs, off, words = _words_read(0)
    lens = [len(c) for c in cigs]
    assert len(cigs) == E.WORDS_FINAL and lens[62:66] == [64, 65, 64, 65] and 0 in lens and max(lens[:62]) <= 3
    assert sum(lens[:64]) > 64                                                    # what block 0 hands to block 1
    n_in = int(g["regs_off"][1])
    assert n_in - len(cigs) == (n_in - 1) // 3                                    # every third secondary went
    for c, h in zip(cigs[62:66], g["regs_out"]["hash"][62:66]):                   # each word names its region and its place
        assert (c >> 13 == int(h) & 0x7ffff).all() and ((c >> 4 & 0x1ff) == np.arange(len(c))).all()
    assert np.diff(g["regs_off_out"]).tolist()[1:] == [1, 1, 1] and np.diff(g["regs_off"]).tolist()[1] == 5      # one primary, all secondaries dropped


def test_word_prefix_carried_between_blocks_of_64_slots():
    res = {}
    for rd in (0, 1):
        g, cigs, off, words = _words_read(rd)
        assert all(same(a, b) for a, b in zip(packed(cigs), (off, words))), rd    # the right layout is the recorded one
        res[rd] = all(same(a, b) for a, b in zip(packed(cigs, carry=False), (off, words)))
    verdict("records out: a final list of 1 / 66 regions, the word prefix carried into the second block", res[1], not res[0])


def test_cigars_of_64_and_65_words():
    res = {}
    for rd in (2, 3):
        g, cigs, off, words = _words_read(rd)
        res[len(cigs[0])] = same(packed(cigs, max_words=64)[1], words)
    verdict("records out: a CIGAR of 64 / 65 words", res[64], not res[65])


def test_lds_edge_is_what_it_is_named_for():
    g = E.load("lds_edge")
    assert np.diff(g["regs_off"]).tolist() == list(E.LDS_SIZES) == [PS.AP_LDS_CAP - 1, PS.AP_LDS_CAP, PS.AP_LDS_CAP + 1]
    assert (np.diff(g["regs_off"]) - np.diff(g["regs_off_out"])).tolist() == [1, 1, 1]
    for o in g["regs_off_out"][:-1]:
        assert g["dp_max2_out"][o] == 580 and g["regs_out"]["parent"][o + 1] == 0 and g["dp_max2_out"][o + 2] == 20


def test_zz_every_wrong_restatement_gave_its_verdict():
    """(Runs last in the file.)  Same below the edge, different on or above it -- but for the flavours that cannot differ."""
    assert len(WRONG) >= 16
    for edge, (lower, upper) in WRONG.items():
        assert lower and (upper or "(none)" in edge), edge
