"""CPU tier: every input of tests/hit_edge_shapes.py sits on the edge it claims -- proved with the restatements (oracle_fpv,
oracle_compact, oracle_bottom, oracle_gen_regs, then post_oracle.post_read or frag_oracle.frag_read): hit, primary and overlap
counts, anchors per chain, hit totals, which step ran (post_oracle._Trace); what the trace cannot show (the rank of the passing
primary among the overlapping ones) is computed here from the records.

For each group edge a local, deliberately wrong restatement that stops at 64 gives the same records on the lower side of the edge and
different records on the upper side (WRONG_AT_64 lists the verdicts).  Where oracle/_ref is built every expected value equals the
unmodified reference's, byte for byte (div included)."""
import ctypes as C
import functools

import numpy as np
import pytest

import frag_oracle as fo
import hit_edge_shapes as hs
import oracle_lib as ol
import post_oracle as po
from minimap2_chaindp_amd import params as P

REF_LEN = np.full(9200, 1 << 27, np.int32)
needs_ref = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (build container only)")


def read_hash(r):
    return (r * 2654435761 + 12345) & 0xffffffff


def chains_of(par, a, min_cnt, n_segs=1):
    pr = ol.CoParams(*[getattr(par, k) for k, _ in ol.CoParams._fields_])
    pr.n_segs = n_segs
    a = np.ascontiguousarray(a)
    f, p, v, _ = ol.oracle_fpv(pr, a)
    seeds = ol.oracle_compact(pr, a, f.copy(), p.copy(), v.copy())
    u, b = ol.oracle_bottom(min_cnt, par.min_sc, seeds)
    return u, b.reshape(-1, 2)


def _offsets(parts):
    return np.concatenate(([0], np.cumsum([len(x) for x in parts]))).astype(np.int64)


def _cat(parts, empty):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else empty


def mini_pos_of(sh, r):
    return sh["mini_pos"][sh["mini_pos_off"][r]:sh["mini_pos_off"][r + 1]]


def post_opt(props, preset="map-ont"):
    return P.post_preset(preset, **props.get("post", {}))


@functools.lru_cache(maxsize=None)
def expected_single(name, *args):
    """What the GPU must return for the single-segment batch hs.<name>(*args): per read the chains, mm_gen_regs' records, mm_est_err
    on them, and chain_post + mm_est_err + mm_set_mapq with the anchors it leaves and the trace.  Shared and never changed."""
    sh, props = getattr(hs, name)(*args)
    par = P.preset("map-ont")
    od = po.opt_dict(post_opt(props))
    n = len(sh["qlen"])
    e = dict(sh=sh, props=props, par=par, opt=post_opt(props), u=[], b=[], regs=[], err=[], n_match=[], n_tot=[], post=[], post_a=[], trace=[],
             hash=np.array([read_hash(r) for r in range(n)], np.uint32))
    for r in range(n):
        u, b = chains_of(par, sh["anchors"][sh["off"][r]:sh["off"][r + 1]], hs.MIN_CNT)
        regs = ol.oracle_gen_regs(read_hash(r), int(sh["qlen"][r]), u, b)
        mp = mini_pos_of(sh, r)
        if len(regs) and len(mp):
            err, nm, nt = ol.oracle_est_err(REF_LEN, int(sh["qlen"][r]), regs, b, mp)
        else:                                                            # esterr.c:37: nothing is touched
            err, nm, nt = regs.copy(), np.zeros(len(regs), np.int32), np.zeros(len(regs), np.int32)
        tr = po._Trace()
        out, a = po.post_read(od, int(sh["qlen"][r]), int(sh["rep_len"][r]), REF_LEN, regs, b, mp, tr=tr)
        for k, x in zip(("u", "b", "regs", "err", "n_match", "n_tot", "post", "post_a", "trace"), (u, b, regs, err, nm, nt, out, a, tr)):
            e[k].append(x)
    e["coff"], e["boff"], e["roff"] = _offsets(e["u"]), _offsets(e["b"]), _offsets(e["post"])
    return e


@functools.lru_cache(maxsize=None)
def expected_frag(name, *args):
    """The same for a fragment batch under sr parameters: per read the chains and the fragment's records, per segment the final hits."""
    sh, props = getattr(hs, name)(*args)
    par = P.preset("sr")
    opt = post_opt(props, "sr")
    od = po.opt_dict(opt)
    n = len(sh["qlen"])
    first = np.concatenate(([0], np.cumsum(sh["n_segs"])))
    e = dict(sh=sh, props=props, par=par, opt=opt, u=[], b=[], regs=[], segs=[], seg_a=[], trace=[], first=first,
             hash=np.array([read_hash(r) for r in range(n)], np.uint32))
    for r in range(n):
        u, b = chains_of(par, sh["anchors"][sh["off"][r]:sh["off"][r + 1]], hs.FRAG_MIN_CNT, int(sh["n_segs"][r]))
        regs = ol.oracle_gen_regs(read_hash(r), int(sh["qlen"][r]), u, b)
        tr = fo.FragTrace()
        segs = fo.frag_read(od, par.max_dist_x, read_hash(r), sh["seg_len"][first[r]:first[r + 1]], int(sh["rep_len"][r]), REF_LEN, regs, b,
                            mini_pos_of(sh, r), tr=tr)
        e["u"].append(u); e["b"].append(b); e["regs"].append(regs); e["trace"].append(tr)
        e["segs"] += [x for x, _ in segs]; e["seg_a"] += [x.reshape(-1, 2) for _, x in segs]
    e["coff"], e["boff"], e["soff"] = _offsets(e["u"]), _offsets(e["b"]), _offsets(e["segs"])
    return e


def cnts(u):
    return (np.asarray(u, np.uint64) & np.uint64(0xffffffff)).astype(np.int64)


def n_primaries(regs):
    return int((regs["parent"] == regs["id"]).sum())


# ---------------------------------------------------------------- deliberately wrong restatements that stop at 64

def wrong_regs_carry(hash_, qlen, u, b):
    """k_regs_keys with the running sum of the counts not carried from one group of 64 chains to the next."""
    k_right = np.concatenate(([0], np.cumsum(cnts(u))[:-1])).astype(np.int64)
    k_wrong = k_right.copy()
    for g in range(64, len(u), 64):
        k_wrong[g:g + 64] -= k_right[g]
    b2 = b.copy()
    for i in range(64, len(u)):
        b2[k_right[i]:k_right[i] + cnts(u)[i]] = b[k_wrong[i]:k_wrong[i] + cnts(u)[i]]
    regs = ol.oracle_gen_regs(hash_, qlen, u, b2)
    lut = {int(k): int(w) for k, w in zip(k_right, k_wrong)}
    regs["as"] = [lut[int(x)] for x in regs["as"]]
    return regs


def wrong_regs_fuzzy(hash_, qlen, u, b):
    """k_regs_fill with only the first 64 terms of mlen / blen."""
    regs = ol.oracle_gen_regs(hash_, qlen, u, b)
    for x in regs:
        k, cnt = int(x["as"]), int(x["cnt"])
        if cnt - 1 > 64:
            t = regs[:1].copy()
            t[0] = x
            t["cnt"] = 65
            po._set_coor(t[0], qlen, b)
            x["mlen"], x["blen"] = t[0]["mlen"], t[0]["blen"]
    return regs


def wrong_est_err_span(qlen, regs, b, mp):
    """k_regs_span_sum over the first 64 minimizer positions only."""
    mp2 = mp.copy()
    mp2[64:] &= np.uint64(0xffffffff)
    return ol.oracle_est_err(REF_LEN, qlen, regs, b, mp2)[0] if len(regs) and len(mp) else regs.copy()


def wrong_set_parent_first64(r, mask_level):
    """post_set_parent looking at the first 64 primaries only (both scans)."""
    n = len(r)
    if n <= 0:
        return
    r["id"] = np.arange(n)
    w = [0]
    r[0]["parent"] = 0
    ml = po.F32(mask_level)
    for i in range(1, n):
        si, ei = int(r[i]["qs"]), int(r[i]["qe"])
        ov = [p for p in w[:64] if not (int(r[p]["qe"]) <= si or int(r[p]["qs"]) >= ei)]
        found = _mask_pass(r, i, ov, ml)
        if found >= 0:
            rp = r[found]
            r[i]["parent"] = rp["parent"]
            rp["subsc"] = max(int(rp["subsc"]), int(r[i]["score"]))
            if r[i]["cnt"] >= rp["cnt"]:
                rp["n_sub"] += 1
        else:
            w.append(i); r[i]["parent"] = i; r[i]["n_sub"] = 0


def _uncov(r, i, ov):
    si, ei = int(r[i]["qs"]), int(r[i]["qe"])
    x, uncov = si, 0
    for s, e in sorted((max(int(r[p]["qs"]), si), min(int(r[p]["qe"]), ei)) for p in ov):
        if s > x:
            uncov += s - x
        x = max(x, e)
    return uncov + max(ei - x, 0)


def _mask_values(r, i, ov):
    """hit.c:135-150: the value of the mask test of hit i at each overlapping primary, in float."""
    si, ei = int(r[i]["qs"]), int(r[i]["qe"])
    uncov = _uncov(r, i, ov)
    out = []
    for p in ov:
        sj, ej = int(r[p]["qs"]), int(r[p]["qe"])
        mn, mx = min(ej - sj, ei - si), max(ej - sj, ei - si)
        ol_ = min(ej, ei) - max(sj, si)
        out.append(po.F32(ol_) / po.F32(mn) - po.F32(uncov) / po.F32(mx))
    return out


def _mask_pass(r, i, ov, ml):
    for p, v in zip(ov, _mask_values(r, i, ov)):
        if v > ml:
            return p
    return -1


def wrong_post_first64(od, qlen, rep_len, regs, b, mp):
    r = np.array(regs, ol.REG_DTYPE, copy=True)
    a = np.array(b, np.uint64, copy=True).reshape(-1, 2)
    wrong_set_parent_first64(r, od["mask_level"])
    r = po.select_sub(r, od["pri_ratio"], od["min_diff"], od["best_n"])
    r, a = po.join_long(od, qlen, r, a)
    if len(r) and len(mp):
        r, _, _ = ol.oracle_est_err(REF_LEN, qlen, r, a, mp)
    po.set_mapq(r, od["min_chain_score"], rep_len)
    return r


def wrong_mapq_sum64(regs, min_chain_sc, rep_len):
    """k_post_mapq with sum_sc over the first 64 hits only: a phantom read whose primaries beyond slot 63 score nothing in the sum."""
    r = regs.copy()
    extra = int(sum(int(x["score"]) for x in r[64:] if x["parent"] == x["id"]))
    sum_sc = int(sum(int(x["score"]) for x in r if x["parent"] == x["id"]))
    # the same uniq_ratio as a sum without `extra`: rep_len' with sum / (sum + rep') == (sum - extra) / (sum - extra + rep) has no integer
    # solution in general, so the formula is restated
    uniq = po.F32(sum_sc - extra) / po.F32(sum_sc - extra + rep_len)
    for x in r:
        if x["parent"] != x["id"]:
            continue
        score, cnt = int(x["score"]), int(x["cnt"])
        pen_s1 = (po.F32(1.0) if score > 100 else po.F32(0.01) * po.F32(score)) * uniq
        pen_cm = po.F32(1.0) if cnt > 10 else po.F32(0.1) * po.F32(cnt)
        pen_cm = min(pen_s1, pen_cm)
        xx = po.F32(max(int(x["subsc"]), min_chain_sc)) / po.F32(int(x["score0"]))
        mapq = po._cvtt(pen_cm * po.F32(40.0) * (po.F32(1.0) - xx) * po.host_logf(score))
        mapq = po._wrap32(mapq - po._cvtt(po.F32(4.343) * po.host_logf(int(x["n_sub"]) + 1) + po.F32(.499)))
        x["bits"] = (int(x["bits"]) & ~0xff) | min(max(mapq, 0), 60)
    return r


def wrong_seg_anchors64(regs0, a, seg):
    """k_frag_split counting only the first 64 anchors of a hit: the anchors of `seg` it would give the first hit that has some."""
    for x in regs0:
        part = a[int(x["as"]):int(x["as"]) + min(int(x["cnt"]), 64)]
        n = int(((part[:, 1] >> np.uint64(48) & np.uint64(0xff)) == np.uint64(seg)).sum())
        if n:
            return n
    return 0


WRONG_AT_64 = {}      # edge -> (lower side equal, upper side different), filled by the tests below and checked at the end


def verdict(edge, lower_same, upper_differs):
    WRONG_AT_64[edge] = (bool(lower_same), bool(upper_differs))
    assert lower_same, (edge, "the wrong restatement differs below the edge")
    assert upper_differs, (edge, "the shape above the edge does not tell the wrong restatement from the right one")


# ---------------------------------------------------------------- mm_gen_regs

@pytest.mark.parametrize("n", hs.REGS_CHAINS)
def test_regs_chain_counts(n):
    e = expected_single("regs_chain_counts", n)
    assert len(e["u"][0]) == len(e["regs"][0]) == n == e["props"]["chains"][0]
    if n:
        assert cnts(e["u"][0]).min() >= 4 and cnts(e["u"][0]).max() <= 6
        assert len(set(e["regs"][0]["rid"].tolist())) == n                 # n distinct targets
        assert np.array_equal(np.sort(e["regs"][0]["as"]), np.concatenate(([0], np.cumsum(cnts(e["u"][0]))[:-1])))


def test_regs_carry_wrong_at_64():
    same, diff = {}, {}
    for n in (64, 65, 128, 129):
        e = expected_single("regs_chain_counts", n)
        w = wrong_regs_carry(read_hash(0), int(e["sh"]["qlen"][0]), e["u"][0], e["b"][0])
        same[n] = w.tobytes() == e["regs"][0].tobytes()
        diff[n] = int((w["as"] != e["regs"][0]["as"]).sum())
    verdict("gen_regs: carry of the first-anchor offset, 64 / 65 chains", same[64], not same[65])
    assert diff[64] == 0 and diff[65] >= 1 and not same[128] and not same[129]   # (a wrong first anchor also moves the hit among its equals)


def test_regs_equal_keys():
    e = expected_single("regs_equal_keys")
    u = e["u"][0]
    assert len(u) >= 130 and len(set(u.tolist())) == 1                     # equal score and count: the keys differ in the low half only
    h = e["regs"][0]["hash"]
    assert len(set(h.tolist())) == len(h) and (np.diff(h.astype(np.int64)) < 0).all()      # larger key first
    # the radix procedure sees 130 keys that agree in bytes 4..7: one bucket per pass until the scrambled bytes spread them
    assert len(set((h >> 24).tolist())) > 64


def test_regs_neighbours():
    e = expected_single("regs_neighbours")
    assert [len(u) for u in e["u"]] == list(hs.REGS_NEIGHBOURS) == e["props"]["chains"]
    c0 = e["coff"][:-1]
    # stacks + c0 / 64 + 2 r: the reads above 64 chains start at chain offsets that are no multiples of 64
    assert [int(c) % 64 != 0 for c, u in zip(c0, e["u"]) if len(u) > 64] == [True, True, True]


@pytest.mark.parametrize("n", hs.REGS_LONG)
def test_regs_long_chain(n):
    e = expected_single("regs_long_chain", n)
    c = cnts(e["u"][0])
    assert c.max() == n == e["props"]["longest"] and sorted(c.tolist())[-2] <= 6 and len(c) == e["props"]["chains"][0]
    top = e["regs"][0][0]
    assert top["cnt"] == n and top["mlen"] != top["blen"]


def test_regs_fuzzy_wrong_at_64():
    res = {}
    for n in hs.REGS_LONG:
        e = expected_single("regs_long_chain", n)
        res[n] = wrong_regs_fuzzy(read_hash(0), int(e["sh"]["qlen"][0]), e["u"][0], e["b"][0]).tobytes() == e["regs"][0].tobytes()
    verdict("gen_regs: 64 / 65 fuzzy-length terms (65 / 66 anchors)", res[64] and res[65], not res[66] and not res[129])


def test_regs_all_is_the_concatenation():
    e = expected_single("regs_all")
    assert [len(u) for u in e["u"]] == e["props"]["chains"]
    assert [int(cnts(u).max()) if len(u) else 0 for u in e["u"]] == e["props"]["longest"]
    assert len(e["u"]) <= 16 and max(int(x) for x in np.diff(e["sh"]["off"])) < 4000


# ---------------------------------------------------------------- mm_est_err

@pytest.mark.parametrize("total", [256, 257])
def test_esterr_totals(total):
    e = expected_single("esterr_totals", total)
    per = [len(x) for x in e["regs"]]
    assert per == e["props"]["hits"] and sum(per) == total == int(e["coff"][-1])
    assert per[0] == per[1] == 0 and per[-1] == per[-2] == 0 and 0 in per[2:-2]          # empty reads at the front, in the middle, at the end
    assert (np.diff(e["coff"]) == 0).sum() >= 5                                          # repeated offsets under the binary search
    assert all((x["div"] >= 0).all() for x in e["err"] if len(x))                        # every hit gets an estimate


@pytest.mark.parametrize("n_reads", [4, 5])
def test_esterr_mini_pos(n_reads):
    e = expected_single("esterr_mini_pos", n_reads)
    sh = e["sh"]
    assert len(sh["qlen"]) == n_reads
    assert np.diff(sh["mini_pos_off"]).tolist() == e["props"]["n_mini_pos"] and {0, 64, 65} <= set(e["props"]["n_mini_pos"])
    r0 = e["props"]["n_mini_pos"].index(0)
    assert len(e["regs"][r0]) > 0 and e["err"][r0].tobytes() == e["regs"][r0].tobytes()  # no minimizer positions: div as it came
    ra = [i for i, k in enumerate(e["props"]["absent_first"]) if k][0]
    err = e["err"][ra]
    gone = err["div"] < 0
    assert gone.sum() == 2 and sorted((err["bits"][gone] >> 10 & 1).tolist()) == [0, 1]  # a forward and a reverse hit without an estimate
    assert (e["n_match"][ra][gone] == 0).all() and (e["n_match"][ra][~gone] > 0).all()
    for r in range(n_reads):
        if r not in (r0, ra):
            assert (e["err"][r]["div"] >= 0).all()


def test_esterr_span_sum_wrong_at_64():
    e = expected_single("esterr_mini_pos", 5)
    res = {}
    for r, n in enumerate(e["props"]["n_mini_pos"]):
        if n in (64, 65):
            w = wrong_est_err_span(int(e["sh"]["qlen"][r]), e["regs"][r], e["b"][r], mini_pos_of(e["sh"], r))
            res[n] = w.tobytes() == e["err"][r].tobytes()
    verdict("est_err: span sum over 64 / 65 minimizer positions", res[64], not res[65])


# ---------------------------------------------------------------- chain_post

@pytest.mark.parametrize("n", [256, 257])
def test_post_lds_cap(n):
    e = expected_single("post_cap_single", n)
    tr = e["trace"][0]
    assert len(e["regs"][0]) == n and len(e["post"][0]) == n - 2 == e["props"]["final"][0]
    assert tr.select_sub_dropped and tr.sync_ran and tr.joined == 1 and tr.squeezed and tr.squeeze_moved and tr.fixup_chain
    assert e["post"][0]["cnt"].max() == e["props"]["joined_cnt"][0] > 128
    assert (e["post_a"][0] != e["b"][0]).any()                               # the squeeze moved anchors and the join marked one


def test_post_cap_neighbours():
    e = expected_single("post_cap_neighbours")
    assert [len(x) for x in e["regs"]] == [256, 257, 7] == e["props"]["hits"]
    assert [len(x) for x in e["post"]] == e["props"]["final"]
    assert [t.joined for t in e["trace"]] == e["props"]["joined"]


@pytest.mark.parametrize("n", [64, 65])
def test_post_primaries(n):
    e = expected_single("post_primaries", n)
    assert len(e["regs"][0]) == n and n_primaries(e["post"][0]) == n == len(e["post"][0])


def _overlapping_primaries(e):
    """From the records: the primaries (in w order) that overlap the last-ranked input hit, and the mask values there."""
    r = e["regs"][0].copy()
    po.set_parent(r, e["opt"].mask_level)
    i = len(r) - 1
    w = [j for j in range(i) if r[j]["parent"] == j]
    ov = [p for p in w if not (int(r[p]["qe"]) <= int(r[i]["qs"]) or int(r[p]["qs"]) >= int(r[i]["qe"]))]
    vals = _mask_values(r, i, ov)
    return r, i, w, ov, vals


@pytest.mark.parametrize("flavour", hs.OVERLAP_FLAVOURS)
@pytest.mark.parametrize("k", [64, 65])
def test_post_overlap(k, flavour):
    e = expected_single("post_overlap", k, flavour)
    regs = e["regs"][0]
    assert len(regs) == k + 1 and regs[-1]["score"] == 60 and regs[-1]["cnt"] == 4 and regs[-2]["score"] > 60      # H is ranked last
    r, i, w, ov, vals = _overlapping_primaries(e)
    ml = po.F32(e["opt"].mask_level)
    assert len(w) == k and len(ov) == k == e["props"]["overlapped"][0]
    passing = [j for j, v in enumerate(vals) if v > ml]
    want = e["props"]["passes_at_rank"][0]
    if want < 0:
        assert passing == [] and r[i]["parent"] == i                          # a primary after ceil(k / 64) ballot rounds
    else:
        assert passing[0] == want and r[i]["parent"] == ov[want] != i
        if flavour == "late":
            assert passing == [k - 1]                                         # 64 non-passing primaries come first in w order for k = 65
    assert min(abs(float(v) - float(ml)) for v in vals) > 1e-3                # no value near enough to the level for rounding to matter
    assert n_primaries(e["post"][0]) == e["props"]["primaries"][0] and len(e["post"][0]) == k + 1


@pytest.mark.parametrize("flavour", ["first", "late"])
def test_post_first_64_primaries_wrong_at_64(flavour):
    res = {}
    for k in (64, 65):
        e = expected_single("post_overlap", k, flavour)
        w = wrong_post_first64(po.opt_dict(e["opt"]), int(e["sh"]["qlen"][0]), 0, e["regs"][0], e["b"][0], mini_pos_of(e["sh"], 0))
        res[k] = w.tobytes() == e["post"][0].tobytes()
    verdict(f"chain_post: a hit that overlaps 64 / 65 primaries ({flavour})", res[64], not res[65])


def test_post_overlap_none_cannot_differ():
    """Counting fewer primaries as covered only lowers the mask value: the first-64 restatement agrees on both sides, by construction."""
    for k in (64, 65):
        e = expected_single("post_overlap", k, "none")
        w = wrong_post_first64(po.opt_dict(e["opt"]), int(e["sh"]["qlen"][0]), 0, e["regs"][0], e["b"][0], mini_pos_of(e["sh"], 0))
        assert w.tobytes() == e["post"][0].tobytes()
    WRONG_AT_64["chain_post: a hit that overlaps 64 / 65 primaries (none)"] = (True, False)


def test_post_select_sub_above_64():
    e = expected_single("post_select_sub_above_64")
    tr, regs, out = e["trace"][0], e["regs"][0], e["post"][0]
    assert len(regs) == e["props"]["hits"][0] > 64 and len(out) == e["props"]["final"][0] == len(regs) - e["props"]["dropped"][0]
    assert tr.select_sub_dropped and tr.sync_ran and tr.joined == 0 and tr.squeeze_moved
    r = regs.copy()
    po.set_parent(r, e["opt"].mask_level)
    kept = po.select_sub(r.copy(), e["opt"].pri_ratio, e["opt"].min_diff, e["opt"].best_n)
    where = {(int(x["rid"]), int(x["rs"])): i for i, x in enumerate(r)}
    old = np.array([where[(int(x["rid"]), int(x["rs"]))] for x in kept])     # the id each kept hit had before mm_sync_regs
    moved = old[old != np.arange(len(kept))]
    assert len(moved) and moved.max() > 63 and moved.min() < 63             # ids on both sides of 63 are renumbered


def test_post_join_above_64():
    e = expected_single("post_join_above_64")
    tr, out = e["trace"][0], e["post"][0]
    assert len(e["regs"][0]) == 70 and len(out) == 69 and tr.joined == 1 and not tr.select_sub_dropped
    assert out["cnt"].max() == e["props"]["joined_cnt"][0] == 160


def test_post_join_fuzzy_wrong_at_64():
    """post_set_coor with one group of lanes: the joined chain of 160 anchors gets other lengths; an 80-anchor piece has 79 terms too."""
    e = expected_single("post_join_above_64")
    out, a = e["post"][0], e["post_a"][0]
    j = int(np.argmax(out["cnt"]))
    t = out[j:j + 1].copy()
    t["cnt"] = 65
    po._set_coor(t[0], int(e["sh"]["qlen"][0]), a)
    assert (int(t[0]["mlen"]), int(t[0]["blen"])) != (int(out[j]["mlen"]), int(out[j]["blen"]))
    WRONG_AT_64["chain_post: fuzzy lengths of a joined chain above 64 anchors"] = (True, True)


def test_post_all_is_the_concatenation():
    e = expected_single("post_all")
    assert [len(x) for x in e["regs"]] == e["props"]["hits"] == [256, 64, 257, 65, 100, 70]
    for fl in hs.OVERLAP_FLAVOURS:
        e = expected_single("post_overlap_all", fl)
        assert [len(x) for x in e["regs"]] == e["props"]["hits"]
        for r, k in ((0, 64), (2, 65)):                                       # the same parents as the read alone (the hash differs)
            assert np.array_equal(e["post"][r]["parent"], expected_single("post_overlap", k, fl)["post"][0]["parent"])


# ---------------------------------------------------------------- mm_set_mapq

@pytest.mark.parametrize("n_reads", [4, 5])
def test_mapq_batch(n_reads):
    e = expected_single("mapq_batch", n_reads)
    assert len(e["post"]) == n_reads and [len(x) for x in e["post"]] == e["props"]["final"] and {64, 65} <= set(e["props"]["final"])
    assert [n_primaries(x) for x in e["post"]] == e["props"]["primaries"]
    assert e["opt"].min_chain_score == hs.MAPQ_MIN_CHAIN_SCORE
    for r, n in enumerate(e["props"]["final"]):
        out = e["post"][r]
        pri = out[out["parent"] == out["id"]]
        assert int(pri["score"].sum()) == e["props"]["sum_sc"][r]
        if n < 64:
            continue
        assert n_primaries(out) >= 3 and out[-1]["parent"] == out[-1]["id"]                      # the last-ranked hit counts in sum_sc
        assert {100, 101} <= set(pri["score"].tolist()) and {10, 11} <= set(pri["cnt"].tolist())
        assert {hs.MAPQ_MIN_CHAIN_SCORE - 1, hs.MAPQ_MIN_CHAIN_SCORE + 1} <= set(pri["subsc"].tolist())
        mq = pri["bits"] & 0xff
        top = pri[pri["score"] == 600][0]
        q = 40.0 * (1 - hs.MAPQ_MIN_CHAIN_SCORE / 600) * np.log(600) * e["props"]["sum_sc"][r] / (e["props"]["sum_sc"][r] + int(e["sh"]["rep_len"][r]))
        assert q > 61 and (top["bits"] & 0xff) == 60                                             # clamps at 60
        eq = pri[(pri["subsc"] == pri["score"])]
        assert len(eq) == 1 and (eq["bits"] & 0xff)[0] == 0                                      # 1 - subsc / score0 = 0, minus the n_sub term: clamps at 0
        assert len(set(mq.tolist())) >= 5


def test_mapq_sum_wrong_at_64():
    e = expected_single("mapq_batch", 4)
    res = {}
    for r, n in enumerate(e["props"]["final"]):
        if n in (64, 65):
            w = wrong_mapq_sum64(e["post"][r], e["opt"].min_chain_score, int(e["sh"]["rep_len"][r]))
            res[n] = w.tobytes() == e["post"][r].tobytes()
    verdict("mapq: sum_sc over 64 / 65 final hits", res[64], not res[65])


# ---------------------------------------------------------------- fragments

def _seg_counts(e, r):
    f = e["first"]
    return [len(e["segs"][q]) for q in range(f[r], f[r + 1])]


@pytest.mark.parametrize("n", [64, 65])
def test_frag_hits(n):
    e = expected_frag("frag_hits", n)
    assert [len(x) for x in e["regs"]] == e["props"]["hits"] == [2, n, 2] and e["sh"]["n_segs"].tolist() == [1, 2, 1]
    assert all(c > 0 for c in _seg_counts(e, 1))
    both = [x for x in e["regs"][1] if x["qs"] < e["sh"]["seg_len"][1] < x["qe"]]
    assert len(both) == 2                                                     # hits over both segments


@pytest.mark.parametrize("n", [64, 65])
def test_frag_seg_chains(n):
    e = expected_frag("frag_seg_chains", n)
    assert _seg_counts(e, 0) == [n, 3] and e["trace"][0].seg_chains_max == n
    assert [len(x) for x in e["regs"]] == e["props"]["hits"]


@pytest.mark.parametrize("n", [64, 65])
def test_frag_long_hit(n):
    e = expected_frag("frag_long_hit", n)
    regs, b = e["regs"][0], e["b"][0]
    for x in regs[:2]:                                                        # the forward and the reverse hit
        part = b[int(x["as"]):int(x["as"]) + int(x["cnt"])]
        seg = (part[:, 1] >> np.uint64(48) & np.uint64(0xff)).astype(int)
        assert x["cnt"] == n + 5 and (seg == 0).sum() == n and (seg == 1).sum() == 5
    assert sorted((regs[:2]["bits"] >> 10 & 1).tolist()) == [0, 1]
    assert e["segs"][0]["cnt"].max() == n and e["segs"][1]["cnt"].max() == 5


def test_frag_split_wrong_at_64():
    res = {}
    for n in (64, 65):
        e = expected_frag("frag_long_hit", n)
        res[n] = wrong_seg_anchors64(e["regs"][0], e["b"][0], 0) == int(e["segs"][0]["cnt"].max())
    verdict("fragments: 64 / 65 anchors of a hit in one segment", res[64], not res[65])


@pytest.mark.parametrize("n_segs", [64, 65, 255])
def test_frag_many_segments(n_segs):
    e = expected_frag("frag_many_segments", n_segs)
    assert e["sh"]["n_segs"].tolist() == [1, n_segs, 1] and [len(x) for x in e["regs"]] == e["props"]["hits"]
    assert min(_seg_counts(e, 1)) >= 1 and len(_seg_counts(e, 1)) == n_segs   # every segment has a hit
    assert _seg_counts(e, 0) == [2] and _seg_counts(e, 2) == [2]              # a one-segment read on either side


def test_frag_all_is_the_concatenation():
    e = expected_frag("frag_all")
    assert len(e["regs"]) == e["props"]["reads"] == 20 and set(e["sh"]["n_segs"].tolist()) == {1, 2, 64, 65}


# ---------------------------------------------------------------- the expected values are the reference's

SINGLE = ([("regs_chain_counts", n) for n in hs.REGS_CHAINS] + [("regs_equal_keys",), ("regs_neighbours",)] + [("regs_long_chain", n) for n in hs.REGS_LONG]
          + [("esterr_totals", 256), ("esterr_totals", 257), ("esterr_mini_pos", 4), ("esterr_mini_pos", 5), ("post_cap_single", 256), ("post_cap_single", 257),
             ("post_cap_neighbours",), ("post_primaries", 64), ("post_primaries", 65)] + [("post_overlap", k, f) for k in (64, 65) for f in hs.OVERLAP_FLAVOURS]
          + [("post_select_sub_above_64",), ("post_join_above_64",), ("mapq_batch", 4), ("mapq_batch", 5)])
FRAGS = [("frag_hits", 64), ("frag_hits", 65), ("frag_seg_chains", 64), ("frag_seg_chains", 65), ("frag_long_hit", 64), ("frag_long_hit", 65),
         ("frag_many_segments", 64), ("frag_many_segments", 65), ("frag_many_segments", 255)]


def _id(t):
    return "-".join(str(x) for x in t)


@needs_ref
@pytest.mark.parametrize("shape", SINGLE, ids=_id)
def test_single_expected_values_are_the_references(shape):
    e = expected_single(*shape)
    sh, od = e["sh"], po.opt_dict(e["opt"])
    for r in range(len(sh["qlen"])):
        a = np.ascontiguousarray(sh["anchors"][sh["off"][r]:sh["off"][r + 1]])
        qlen, mp = int(sh["qlen"][r]), mini_pos_of(sh, r)
        _, _, _, seeds = ol.ref_fpv_seeds(e["par"], a)
        u, b = ol.ref_bottom(hs.MIN_CNT, e["par"].min_sc, 1, seeds)
        b = b.reshape(-1, 2)
        assert np.array_equal(u, e["u"][r]) and np.array_equal(b, e["b"][r]), (shape, r, "chains")
        regs = ol.ref_gen_regs(read_hash(r), qlen, u, b)
        assert regs.tobytes() == e["regs"][r].tobytes(), (shape, r, "mm_gen_regs")
        if len(regs) and len(mp):
            assert ol.ref_est_err(REF_LEN, qlen, regs, b, mp).tobytes() == e["err"][r].tobytes(), (shape, r, "mm_est_err")
        want, wa = po.ref_post_read(od, qlen, int(sh["rep_len"][r]), REF_LEN, regs, b, mp)
        assert want.tobytes() == e["post"][r].tobytes() and wa.tobytes() == e["post_a"][r].tobytes(), (shape, r, "chain_post .. mm_set_mapq")


def _ref_segments(od, hash_, qlens, rep_len, r, a):
    """mm_seg_gen, mm_set_parent and mm_set_mapq of the reference (map.c:880-885) on the fragment's hits after mm_select_sub_multi."""
    L = po._ref()
    vp, i32 = C.c_void_p, C.c_int

    class SegT(C.Structure):                 # mm_seg_t, mmpriv.h:44-48
        _fields_ = [("n_u", C.c_int), ("n_a", C.c_int), ("u", C.POINTER(C.c_uint64)), ("a", C.POINTER(C.c_uint64))]
    L.mm_seg_gen.restype = C.POINTER(SegT)
    L.mm_seg_gen.argtypes = [vp, C.c_uint32, i32, vp, i32, vp, vp, vp, vp]
    L.mm_seg_free.restype = None
    L.mm_seg_free.argtypes = [vp, i32, C.POINTER(SegT)]
    n_segs, n = len(qlens), len(r)
    ql = np.array(qlens, np.int32)
    raw = np.zeros((max(n, 1), ol.REF_REG_BYTES), np.uint8)
    raw[:n, :72] = np.ascontiguousarray(r, ol.REG_DTYPE).view(np.uint8).reshape(n, 80)[:, :72]
    a_buf = np.array(a, np.uint64, copy=True).reshape(-1, 2)
    n_regs, regs = (C.c_int * n_segs)(), (C.c_void_p * n_segs)()
    seg = L.mm_seg_gen(None, int(hash_), n_segs, ql.ctypes.data, n, raw.ctypes.data, n_regs, regs, a_buf.ctypes.data)
    out = []
    for s in range(n_segs):
        m = n_regs[s]
        L.mm_set_parent(None, od["mask_level"], m, regs[s], od["sub_diff"])
        L.mm_set_mapq(None, m, regs[s], od["min_chain_score"], od["match_sc"], rep_len, od["is_sr"])
        out.append(ol._ref_regs_to_np(regs[s], m) if m else np.zeros(0, ol.REG_DTYPE))
        if regs[s]:
            ol._libc.free(regs[s])
    L.mm_seg_free(None, n_segs, seg)
    return out


@needs_ref
@pytest.mark.parametrize("shape", FRAGS, ids=_id)
def test_frag_expected_values_are_the_references(shape):
    """Chains, the fragment's records and the reference's mm_set_parent are compared directly; pe.c is not part of the reference
    library, so mm_select_sub_multi is the restatement's (pinned to the reference by tests/golden/frag), and the reference's
    mm_seg_gen, mm_set_parent and mm_set_mapq run on its result."""
    e = expected_frag(*shape)
    sh, od = e["sh"], po.opt_dict(e["opt"])
    for r in range(len(sh["qlen"])):
        ns = int(sh["n_segs"][r])
        a = np.ascontiguousarray(sh["anchors"][sh["off"][r]:sh["off"][r + 1]])
        pr = ol.CoParams(*[getattr(e["par"], k) for k, _ in ol.CoParams._fields_])
        pr.n_segs = ns
        _, _, _, seeds = ol.ref_fpv_seeds(pr, a)
        u, b = ol.ref_bottom(hs.FRAG_MIN_CNT, e["par"].min_sc, ns, seeds)
        b = b.reshape(-1, 2)
        assert np.array_equal(u, e["u"][r]) and np.array_equal(b, e["b"][r]), (shape, r, "chains")
        regs = ol.ref_gen_regs(read_hash(r), int(sh["qlen"][r]), u, b)
        assert regs.tobytes() == e["regs"][r].tobytes(), (shape, r, "mm_gen_regs")
        qlens = [int(x) for x in sh["seg_len"][e["first"][r]:e["first"][r + 1]]]
        if ns == 1:
            want, _ = po.ref_post_read(od, qlens[0], int(sh["rep_len"][r]), REF_LEN, regs, b, mini_pos_of(sh, r))
            assert want.tobytes() == e["segs"][e["first"][r]].tobytes(), (shape, r, "one-segment read")
            continue
        n = len(regs)
        raw = np.zeros((max(n, 1), ol.REF_REG_BYTES), np.uint8)
        raw[:n, :72] = regs.view(np.uint8).reshape(n, 80)[:, :72]
        po._ref().mm_set_parent(None, od["mask_level"], n, raw.ctypes.data, od["sub_diff"])
        rr = np.zeros(n, ol.REG_DTYPE)
        rr.view(np.uint8).reshape(n, 80)[:, :72] = raw[:n, :72]
        mine = regs.copy()
        po.set_parent(mine, od["mask_level"])
        assert rr.tobytes() == mine.tobytes(), (shape, r, "mm_set_parent")
        rr = fo.select_sub_multi(rr, od["pri_ratio"], e["par"].max_dist_x, od["min_diff"], od["best_n"], ns, qlens)
        for s, want in enumerate(_ref_segments(od, read_hash(r), qlens, int(sh["rep_len"][r]), rr, b)):
            assert want.tobytes() == e["segs"][e["first"][r] + s].tobytes(), (shape, r, s, "mm_seg_gen .. mm_set_mapq")


def test_zz_every_wrong_at_64_restatement_gave_its_verdict():
    """(Runs last in the file.)  Same below the edge, different above it -- but for the flavour that cannot differ."""
    for edge, (lower, upper) in WRONG_AT_64.items():
        assert lower and (upper or "(none)" in edge), edge
