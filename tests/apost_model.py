"""CHECKER ONLY: a restatement of what the reference does with one read's regions once they carry alignments -- the tail of align_regs
(map.c:253-257: mm_set_parent with r->p, mm_select_sub, mm_set_sam_pri) and mm_set_mapq with mm_set_inv_mapq (map.c:876,
hit.c:411-480) -- on numpy records.  It builds on tests/post_oracle.py (float32 steps, host_logf through libm, _cvtt) and adds the
r->p branches; mm_select_sub and mm_sync_regs are post_oracle's own, run on records that carry their input index along.

A read is (regs REG_DTYPE[n], extra EXTRA_DTYPE[n], cigars [n arrays]); post_read() returns (regs, extra, dp_max2 int32[], cigars).
tests/golden/make_apost_golden.py proves it equal to the compiled reference before the goldens are trusted.  Every case the tests name
is counted in `cover`; the counters change no result."""
import collections

import numpy as np

import post_oracle as po
from align_shapes import EXTRA_DTYPE, REG_DTYPE
from post_oracle import BIT_INV, BIT_SAM_PRI, F32, INT_MIN, MM_F_ALL_CHAINS, _cvtt, _wrap32, host_logf

COVER = ("read_without_regions", "one_region", "identical_after_dp", "dp_max2_set", "sub_diff_exact", "sub_diff_plus_1",
         "dropped_pri_ratio", "saved_min_diff", "dropped_best_n", "dropped_identical", "dropped_second", "dropped_middle", "dropped_last",
         "read_keeps_all", "select_sub_reads_overwritten_slot", "all_chains", "mixed_has_extra",
         "mapq_dp2_alt_lower", "mapq_dp2_alt_higher", "mapq_dp2_is_sr", "mapq_p_dp2_zero", "mapq_no_p", "mapq_zero_to_one", "mapq_clamped_60",
         "mapq_negative", "mapq_float_outside_int", "inv_mapq_fewer_than_3", "inv_mapq_no_inversion", "inv_between_primaries", "inv_first_in_order",
         "inv_last_in_order", "list_over_64", "primaries_over_64")
# the classes of the edge tier (tests/apost_edge_shapes.py), counted like COVER
EDGE_COVER = ("overlaps_over_64", "found_at_rank_0_of_over_64", "found_at_rank_63", "found_at_rank_64", "none_found_of_over_64", "union_equal_start",
              "mask_equals_level", "sum_sc_over_int32", "sum_sc_over_2p24", "nsub_float_add_decides", "mapq_wraps_to_60", "dp_max_not_positive_with_p",
              "score_not_positive_without_p", "score0_zero", "identity_nan", "sub_dp_max_above_parent", "sub_above_parent_by_dp_only", "mapq_alt_negative",
              "inv_at_rank_63", "inv_at_rank_64", "inv_index_decides", "inv_is_secondary", "inv_as_top_bit", "aux_parent_unset", "cigar_64_words",
              "cigar_65_words", "cigar_none_beside_some", "final_over_64")
SRC_DTYPE = np.dtype(REG_DTYPE.descr + [("src", "<i4")])

cover = collections.Counter()


def logf_dp(dp_max, match_sc):
    """logf((float)dp_max / match_sc) as the host computes it."""
    with np.errstate(all="ignore"):
        return host_logf(F32(dp_max) / F32(match_sc))


@np.errstate(all="ignore")
def set_parent(r, has_p, dp_max, dp_max2, mask_level, sub_diff):
    """mm_set_parent (hit.c:109-165) with the r->p branch; dp_max2 is updated in place."""
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
        for p in w:
            sj, ej = int(r[p]["qs"]), int(r[p]["qe"])
            if ej <= si or sj >= ei:
                continue
            cov.append((max(sj, si), min(ej, ei)))
        found = -1
        if cov:
            if len(cov) > 64:
                cover["overlaps_over_64"] += 1
            if len(set(s for s, _ in cov)) < len(cov):
                cover["union_equal_start"] += 1
            cov.sort()
            rank = -1
            x, uncov = si, 0
            for s, e in cov:
                if s > x:
                    uncov += s - x
                x = max(x, e)
            if ei > x:
                uncov += ei - x
            for p in w:
                sj, ej = int(r[p]["qs"]), int(r[p]["qe"])
                if ej <= si or sj >= ei:
                    continue
                mn, mx = min(ej - sj, ei - si), max(ej - sj, ei - si)
                ol_ = (0 if ei < sj else ei - sj if ei < ej else ej - sj) if si < sj else (0 if ej < si else ej - si if ej < ei else ei - si)
                rank += 1
                val = F32(ol_) / F32(mn) - F32(uncov) / F32(mx)
                if val == ml:
                    cover["mask_equals_level"] += 1
                if val > ml:
                    found = p
                    if rank in (63, 64):
                        cover["found_at_rank_%d" % rank] += 1
                    elif rank == 0 and len(cov) > 64:
                        cover["found_at_rank_0_of_over_64"] += 1
                    break
            if found < 0 and len(cov) > 64:
                cover["none_found_of_over_64"] += 1
        if found >= 0:
            rp = r[found]
            r[i]["parent"] = rp["parent"]
            rp["subsc"] = max(int(rp["subsc"]), int(r[i]["score"]))
            cnt_sub = bool(r[i]["cnt"] >= rp["cnt"])
            if has_p[found] and has_p[i]:
                if rp["rid"] != r[i]["rid"] or rp["rs"] != r[i]["rs"] or rp["re"] != r[i]["re"] or ol_ != mn:
                    dp_max2[found] = max(int(dp_max2[found]), int(dp_max[i]))
                    cover["dp_max2_set"] += 1
                    if dp_max[i] > dp_max[found]:
                        cover["sub_dp_max_above_parent"] += 1
                        if not cnt_sub:
                            cover["sub_above_parent_by_dp_only"] += 1
                    diff = _wrap32(int(dp_max[found]) - int(dp_max[i]))
                    if diff <= sub_diff:
                        if diff == sub_diff and not cnt_sub:
                            cover["sub_diff_exact"] += 1
                        cnt_sub = True
                    elif diff == sub_diff + 1 and not cnt_sub:
                        cover["sub_diff_plus_1"] += 1
                else:
                    cover["identical_after_dp"] += 1
            if cnt_sub:
                rp["n_sub"] += 1
        else:
            w.append(i)
            r[i]["parent"] = i
            r[i]["n_sub"] = 0
    if len(w) > 64:
        cover["primaries_over_64"] += 1


def select_sub(r, pri_ratio, min_diff, best_n):
    """mm_select_sub (hit.c:230-247): post_oracle's, on records that carry `src`; the counters name why a region went."""
    n = len(r)
    if F32(pri_ratio) > F32(0) and n > 0:                       # the verdicts, by a dry run of the same in-place loop
        t, k, n_2nd, pr = r.copy(), 0, 0, F32(pri_ratio)
        for i in range(n):
            p = int(t[i]["parent"])
            if p == i or int(t[i]["bits"]) & BIT_INV:
                t[k] = t[i]; k += 1
                continue
            rp = t[p]
            si, sp = int(t[i]["score"]), int(rp["score"])
            by_ratio, by_diff = bool(F32(si) >= F32(sp) * pr), si + min_diff >= sp
            why = None
            if not (by_ratio or by_diff):
                why = "dropped_pri_ratio"
            elif not n_2nd < best_n:
                why = "dropped_best_n"
            elif t[i]["qs"] == rp["qs"] and t[i]["qe"] == rp["qe"] and t[i]["rid"] == rp["rid"] and t[i]["rs"] == rp["rs"] and t[i]["re"] == rp["re"]:
                why = "dropped_identical"
            if why:
                cover[why] += 1
                cover["dropped_last" if i == n - 1 else "dropped_second" if i == 1 else "dropped_middle"] += 1   # r[0] is its own parent: never dropped
            else:
                if by_diff and not by_ratio:
                    cover["saved_min_diff"] += 1
                t[k] = t[i]; k += 1; n_2nd += 1
        if k == n:
            cover["read_keeps_all"] += 1
    tr = po._Trace()
    out = po.select_sub(r, pri_ratio, min_diff, best_n, tr)
    if tr.slot_overwritten_read:
        cover["select_sub_reads_overwritten_slot"] += 1
    return out


def set_sam_pri(r):
    n_pri = 0
    for x in r:
        if x["id"] == x["parent"]:
            n_pri += 1
            sp = n_pri == 1
        else:
            sp = False
        x["bits"] = (int(x["bits"]) & ~BIT_SAM_PRI) | (BIT_SAM_PRI if sp else 0)


@np.errstate(all="ignore")
def set_mapq(r, has_p, dp_max, dp_max2, min_chain_sc, match_sc, rep_len, is_sr):
    """mm_set_mapq (hit.c:437-480) with both r->p branches, then mm_set_inv_mapq (hit.c:411-435).  has_p, dp_max, dp_max2: per record."""
    n = len(r)
    sum_sc = int(sum(int(x["score"]) for x in r if x["parent"] == x["id"]))
    uniq_ratio = F32(sum_sc) / F32(sum_sc + rep_len)
    if sum_sc > 1 << 24:
        cover["sum_sc_over_int32" if sum_sc >= 1 << 31 else "sum_sc_over_2p24"] += 1
    q_coef = F32(40.0)
    for i, x in enumerate(r):
        bits = int(x["bits"])
        if bits & BIT_INV:
            mq = 0
        elif x["parent"] == x["id"]:
            score, cnt = int(x["score"]), int(x["cnt"])
            pen_s1 = (F32(1.0) if score > 100 else F32(0.01) * F32(score)) * uniq_ratio
            pen_cm = F32(1.0) if cnt > 10 else F32(0.1) * F32(cnt)
            pen_cm = pen_s1 if pen_s1 < pen_cm else pen_cm
            subsc = max(int(x["subsc"]), min_chain_sc)
            p, dm, d2 = bool(has_p[i]), int(dp_max[i]), int(dp_max2[i])
            if p and d2 > 0 and dm > 0:
                identity = F32(int(x["mlen"])) / F32(int(x["blen"]))
                xx = F32(d2) * F32(subsc) / F32(dm) / F32(int(x["score0"]))
                mapq = _cvtt(identity * pen_cm * q_coef * (F32(1.0) - xx * xx) * logf_dp(dm, match_sc))
                if not is_sr:
                    alt = _cvtt(F32(6.02) * identity * identity * F32(dm - d2) / F32(match_sc) + F32(.499))
                    if alt < 0:
                        cover["mapq_alt_negative"] += 1
                    cover["mapq_dp2_alt_lower" if alt < mapq else "mapq_dp2_alt_higher"] += 1
                    mapq = mapq if mapq < alt else alt
                else:
                    cover["mapq_dp2_is_sr"] += 1
            else:
                xx = F32(subsc) / F32(int(x["score0"]))
                if p:
                    identity = F32(int(x["mlen"])) / F32(int(x["blen"]))
                    mapq = _cvtt(identity * pen_cm * q_coef * (F32(1.0) - xx) * logf_dp(dm, match_sc))
                    cover["mapq_p_dp2_zero"] += 1
                else:
                    mapq = _cvtt(pen_cm * q_coef * (F32(1.0) - xx) * host_logf(score))
                    cover["mapq_no_p"] += 1
            if mapq == INT_MIN:
                cover["mapq_float_outside_int"] += 1
            if p and dm <= 0:
                cover["dp_max_not_positive_with_p"] += 1
            if not p and score <= 0:
                cover["score_not_positive_without_p"] += 1
            if int(x["score0"]) == 0:
                cover["score0_zero"] += 1
            if p and int(x["mlen"]) == 0 and int(x["blen"]) == 0:
                cover["identity_nan"] += 1
            lg_sub = F32(4.343) * host_logf(int(x["n_sub"]) + 1)
            sub = _cvtt(lg_sub + F32(.499))
            if int(np.float64(lg_sub) + np.float64(np.float32(.499))) != sub:
                cover["nsub_float_add_decides"] += 1
            if mapq == INT_MIN and sub > 0:
                cover["mapq_wraps_to_60"] += 1
            mapq = _wrap32(mapq - sub)
            if mapq < 0 and mapq != _wrap32(INT_MIN - sub):
                cover["mapq_negative"] += 1
            if mapq > 60:
                cover["mapq_clamped_60"] += 1
            mq = min(max(mapq, 0), 60)
            if p and dm > d2 and mq == 0:
                mq = 1
                cover["mapq_zero_to_one"] += 1
        else:
            mq = 0
        x["bits"] = (bits & ~0xff) | (mq & 0xff)
    # mm_set_inv_mapq
    if n < 3:
        cover["inv_mapq_fewer_than_3"] += 1
        return
    if not any(int(x["bits"]) & BIT_INV for x in r):
        cover["inv_mapq_no_inversion"] += 1
        return
    aux = sorted((int(np.uint32(r[i]["as"])) << 32 | i) for i in range(n) if r[i]["parent"] == i or r[i]["parent"] < 0)
    if any(int(x["bits"]) & BIT_INV and x["parent"] != x["id"] and x["parent"] >= 0 for x in r):
        cover["inv_is_secondary"] += 1
    if any(r[i]["parent"] < 0 and r[i]["id"] != r[i]["parent"] for i in range(n)):
        cover["aux_parent_unset"] += 1
    if any(r[i]["as"] < 0 for i in range(n) if r[i]["parent"] == i):
        cover["inv_as_top_bit"] += 1
    for j, key in enumerate(aux):
        if int(r[key & 0xffffffff]["bits"]) & BIT_INV:
            if j in (63, 64) and j < len(aux) - 1:
                cover["inv_at_rank_%d" % j] += 1
            if (j > 0 and aux[j - 1] >> 32 == key >> 32) or (j < len(aux) - 1 and aux[j + 1] >> 32 == key >> 32):
                cover["inv_index_decides"] += 1
            cover["inv_first_in_order" if j == 0 else "inv_last_in_order" if j == len(aux) - 1 else "inv_between_primaries"] += 1
    for j in range(1, len(aux) - 1):
        v = r[aux[j] & 0xffffffff]
        if int(v["bits"]) & BIT_INV:
            ml, mr = int(r[aux[j - 1] & 0xffffffff]["bits"]) & 0xff, int(r[aux[j + 1] & 0xffffffff]["bits"]) & 0xff
            v["bits"] = (int(v["bits"]) & ~0xff) | min(ml, mr)


def post_read(opt, rep_len, regs, extra, cigars):
    """One read.  opt: dict of params.PostOpt's fields.  Returns (regs, extra, dp_max2, cigars) of the final regions."""
    n = len(regs)
    r = np.zeros(n, SRC_DTYPE)
    for k in REG_DTYPE.names:
        r[k] = regs[k]
    r["src"] = np.arange(n)
    extra = np.asarray(extra, EXTRA_DTYPE)
    has_p, dp_max, dp2 = extra["has_extra"].astype(bool), extra["dp_max"].astype(np.int64), np.zeros(n, np.int64)
    cover["read_without_regions" if n == 0 else "one_region" if n == 1 else "list_over_64" if n > 64 else "_other"] += 1
    if n and has_p.any() and not has_p.all():
        cover["mixed_has_extra"] += 1
    if not opt["flag"] & MM_F_ALL_CHAINS:
        set_parent(r, has_p, dp_max, dp2, opt["mask_level"], opt["sub_diff"])
        r = select_sub(r, opt["pri_ratio"], opt["min_diff"], opt["best_n"])
        set_sam_pri(r)
    elif n:
        cover["all_chains"] += 1
    src = r["src"].astype(np.int64)
    set_mapq(r, has_p[src], dp_max[src], dp2[src], opt["min_chain_score"], opt["match_sc"], rep_len, opt["is_sr"])
    out = np.zeros(len(r), REG_DTYPE)
    for k in REG_DTYPE.names:
        out[k] = r[k]
    lens = [len(cigars[i]) for i in src]
    for m in (64, 65):
        if m in lens:
            cover["cigar_%d_words" % m] += 1
    if lens and min(lens) == 0 < max(lens):
        cover["cigar_none_beside_some"] += 1
    if len(r) > 64:
        cover["final_over_64"] += 1
    return out, extra[src].copy(), dp2[src].astype(np.int32), [np.asarray(cigars[i], np.uint32) for i in src]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)


def run(opt, rep_len, regs_off, regs, extra, cigar_off, cigar):
    """A batch in the CSR form of Device.align_post: dict(regs_off, regs, extra, dp_max2, cigar_off, cigar)."""
    outs = []
    for rd in range(len(regs_off) - 1):
        g0, g1 = int(regs_off[rd]), int(regs_off[rd + 1])
        outs.append(post_read(opt, int(rep_len[rd]), regs[g0:g1], extra[g0:g1], [cigar[int(cigar_off[g]):int(cigar_off[g + 1])] for g in range(g0, g1)]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if sum(len(x) for x in parts) else np.zeros(0, dt)
    cigs = [c for o in outs for c in o[3]]
    return dict(regs_off=offsets([len(o[0]) for o in outs]), regs=cat([o[0] for o in outs], REG_DTYPE), extra=cat([o[1] for o in outs], EXTRA_DTYPE),
                dp_max2=cat([o[2] for o in outs], np.int32), cigar_off=offsets([len(c) for c in cigs]), cigar=cat(cigs, np.uint32))


OUTPUTS = ("regs_off", "regs", "extra", "dp_max2", "cigar_off", "cigar")
