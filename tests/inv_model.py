"""Python restatement of the reference's mm_align1_inv (align.c:638-693) and of the rule of the loop around it (align.c:747-753), on top
of align_model (mm_update_extra, mm_fix_cigar) and ksw_model.ksw_extd, plus the model of ksw_ll_i16 WITH its end positions.
tests/golden/make_align_inv_golden.py proves all of it equal to the compiled reference before the goldens are trusted.

ksw_ll_i16's striped layout pads the query to ql8 = 8 * slen rows, slen = (ql + 7) / 8.  A padded row scores 0 against every base but
is a DP cell like any other: it counts in the column maximum and in the scan for qe.  So where the best local alignment reaches the
query's last base, the maximum runs on diagonally through the padding, te moves with it and qe >= ql.

Every branch the tests name is counted in `cover`; the counters change no result."""
import collections

import numpy as np

import align_model as A
import ksw_model as K
import ksw_shapes as KS

PARENT_UNSET, PARENT_TMP_PRI = -1, -2
BIT_SPLIT1, BIT_SPLIT2, BIT_REV, BIT_INV, BIT_SPLIT_INV = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 24
NONE, MADE, LOW_SCORE, SKIPPED, NO_CIGAR = 0, 1, 2, 3, 4
EZ_EXTZ_ONLY = 0x40

cover = collections.Counter()
problems = []         # (qlen, tlen, w) of every extension, in the order align1_inv makes them
ll_seen = []          # (query, target, gapo, gape, a, b, (score, qe, te)) of every stretch given to ll_ends


def ll_ends(query, target, mat, gapo, gape, pad=True, tie="striped", count=False):
    """(score, qe, te) of ksw_ll_i16 (ksw2_ll_sse.c:80-147).  A plain local DP over the padded query: H floored at 0, the diagonal add
    saturating at 32767, E and F floored at 0; te the LAST column whose maximum equals the global one; qe, of that column's rows p with
    H equal to it, the one with the greatest (p % slen, p / slen).  pad=False (ql rows) and tie="first" / "last" (by p) are the
    wrong models the tests hold the scenes against."""
    q, t = np.asarray(query, np.int64), np.asarray(target, np.int64)
    ql, tl = len(q), len(t)
    if ql == 0 or tl == 0:
        return 0, -1, -1
    slen = (ql + 7) // 8
    rows = slen * 8 if pad else ql
    qp = np.full(rows, 4, np.int64)
    qp[:ql] = q
    oe, rampe = gapo + gape, np.arange(rows, dtype=np.int64) * gape
    H, E = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    gmax, te, hmax = 0, -1, H
    for i in range(tl):
        diag = np.concatenate([[0], H[:-1]])
        h = np.maximum(np.maximum(np.minimum(diag + mat[t[i], qp], 32767), E), 0)
        # F[p] = max over p' < p of h[p'] - oe - (p - 1 - p') * gape, floored at 0: an H that F raised opens nothing better (gapo >= 0)
        run = np.maximum.accumulate(h + rampe)
        F = np.concatenate([[0], np.maximum(run[:-1] - oe - rampe[:-1], 0)])
        h = np.maximum(h, F)
        E = np.maximum(np.maximum(E - gape, h - oe), 0)
        H = h
        imax = int(h.max())
        if imax >= gmax:
            gmax, te, hmax = imax, i, h
    p = np.nonzero(hmax == gmax)[0]
    if tie == "striped":
        qe = int(p[np.lexsort((p // slen, p % slen))[-1]])
    else:
        qe = int(p[0] if tie == "first" else p[-1])
    if count:
        if qe >= ql:
            cover["qe_in_padding"] += 1
        if len(p) >= 3 and qe not in (int(p[0]), int(p[-1])):
            cover["qe_tie_middle"] += 1
        if gmax == 32767:
            cover["saturated"] += 1
    return gmax, qe, te


def early_return(opt, r1, r2):
    """The name of the early return the pair takes (align.c:646-653, and :748 for split_inv), or None for a candidate with (ql, tl)."""
    if not r2["bits"] & BIT_SPLIT_INV:
        return "no_split_inv", None
    if not r1["bits"] & BIT_SPLIT1:
        return "split1", None
    if not r2["bits"] & BIT_SPLIT2:
        return "split2", None
    if r1["id"] != r1["parent"] and r1["parent"] != PARENT_TMP_PRI:
        return "parent1", None
    if r2["id"] != r2["parent"] and r2["parent"] != PARENT_TMP_PRI:
        return "parent2", None
    if r1["rid"] != r2["rid"]:
        return "rid", None
    if (r1["bits"] ^ r2["bits"]) & BIT_REV:
        return "rev", None
    ql = r1["qs"] - r2["qe"] if r1["bits"] & BIT_REV else r2["qs"] - r1["qe"]
    tl = r2["rs"] - r1["re"]
    if ql < opt["min_chain_score"]:
        return "ql_low", None
    if ql > opt["max_gap"]:
        return "ql_high", None
    if tl < opt["min_chain_score"]:
        return "tl_low", None
    if tl > opt["max_gap"]:
        return "tl_high", None
    return None, (ql, tl)


def zero_reg():
    return dict(zip(A.REG_FIELDS, (0,) * len(A.REG_FIELDS)))


def align1_inv(opt, tcodes, qf, r1, r2, ksw=K.ksw_extd):
    """mm_align1_inv on the pair (r1, r2) of the read with forward codes qf; tcodes[rid] the targets' codes.  Returns (code, r_inv dict,
    extra dict, cigar uint32[], ll) with ll = (score, qe, te) of a candidate or None; code as the ABI's made[] before the loop's rule."""
    none = dict(zip(A.EXTRA_FIELDS, (0,) * 5))
    nocig = np.zeros(0, np.uint32)
    why, lens = early_return(opt, r1, r2)
    if why:
        cover["early_" + why] += 1
        return NONE, zero_reg(), none, nocig, None
    ql, tl = lens
    for r in (r1, r2):
        cover["parent_is_id" if r["id"] == r["parent"] else "parent_tmp_pri"] += 1
    for v, nm in ((ql, "ql"), (tl, "tl")):
        if v == opt["min_chain_score"]:
            cover[nm + "_at_min"] += 1
        if v == opt["max_gap"]:
            cover[nm + "_at_max_gap"] += 1
        if v in (63, 64, 65, 127, 128, 129):
            cover["%s_%d" % (nm, v)] += 1
    cover["ql_lt_tl" if ql < tl else "ql_gt_tl" if ql > tl else "ql_eq_tl"] += 1
    cover["ql_mod8_%d" % (ql % 8)] += 1
    qlen = len(qf)
    rev1 = 1 if r1["bits"] & BIT_REV else 0
    cover["strand_%d" % rev1] += 1
    strand = np.asarray(qf, np.uint8) if rev1 else A.revcomp(qf)
    qb = r2["qe"] if rev1 else qlen - r2["qs"]
    tseq_all = tcodes[r1["rid"]]
    if qb < 0 or qb + ql > qlen or r1["re"] < 0 or r2["rs"] > len(tseq_all):
        raise A.Undefined("the stretch leaves its sequence")
    qseq, tseq = strand[qb:qb + ql], tseq_all[r1["re"]:r2["rs"]]
    mat = A.simple_mat(opt["a"], opt["b"])
    ll = ll_ends(qseq[::-1], tseq[::-1], mat, opt["q"], opt["e"], count=True)
    ll_seen.append((qseq[::-1].copy(), np.array(tseq[::-1], np.uint8), opt["q"], opt["e"], opt["a"], opt["b"], ll))
    score, qe, te = ll
    if score == opt["min_dp_max"]:
        cover["score_at_min_dp_max"] += 1
    if score == opt["min_dp_max"] - 1:
        cover["score_below_min_dp_max_by_1"] += 1
    if score < opt["min_dp_max"]:
        cover["low_score"] += 1
        return LOW_SCORE, zero_reg(), none, nocig, ll
    q_off, t_off = ql - (qe + 1), tl - (te + 1)
    cover["q_off_%d" % q_off if q_off < 0 else "q_off_0" if q_off == 0 else "q_off_pos"] += 1
    if q_off == 0 and ql % 8 == 0:
        cover["q_off_0_no_padding"] += 1
    if qb + q_off < 0:
        raise A.Undefined("q_off leaves the strand")
    qs_, ts_ = strand[qb + q_off:qb + ql], tseq[t_off:]
    if q_off >= 0 and (qs_[0] > 3 or ts_[0] > 3):
        cover["wildcard_behind_best"] += 1
    sc = tuple(opt[k] for k in ("a", "b", "q", "e", "q2", "e2"))
    w = int(opt["bw"] * 1.5)
    problems.append((len(qs_), len(ts_), w))
    cover["route_" + A.ROUTE_NAMES[KS.expected_route(len(qs_), len(ts_), sc)]] += 1
    ez, cig = ksw(qs_, ts_, *sc, w, opt["zdrop"], -1, EZ_EXTZ_ONLY)
    if ez[1]:
        cover["ext_zdropped"] += 1
    if len(cig) == 0:
        cover["no_cigar"] += 1
        return NO_CIGAR, zero_reg(), none, nocig, ll
    r = zero_reg()
    r.update({"id": -1, "parent": PARENT_UNSET, "rid": r1["rid"], "div": -1.0, "bits": BIT_INV | (0 if rev1 else BIT_REV)})
    if rev1:            # r_inv->rev == 0
        r["qs"] = r2["qe"] + q_off
        r["qe"] = r["qs"] + int(ez[2]) + 1
    else:
        r["qe"] = r2["qs"] - q_off
        r["qs"] = r["qe"] - (int(ez[2]) + 1)
    r["rs"] = r1["re"] + t_off
    r["re"] = r["rs"] + int(ez[3]) + 1
    p = {"dp_score": int(ez[0]), "dp_max": 0, "n_ambi": 0, "cigar": [int(v) for v in cig]}
    before = A.cover["fix_cigar_leading_I"], A.cover["fix_cigar_leading_D"], A.cover["n_ambi"]
    A.update_extra(r, p, qs_, ts_, mat, opt["q"], opt["e"])
    for k, b in zip(("fix_cigar_leading_I", "fix_cigar_leading_D", "n_ambi"), before):
        if A.cover[k] > b:
            cover["%s_strand_%d" % (k, rev1)] += 1
    if not p["cigar"]:
        raise A.Undefined("the CIGAR is empty after mm_fix_cigar")
    cover["made"] += 1
    extra = {"has_extra": 1, "dp_score": p["dp_score"], "dp_max": p["dp_max"], "n_ambi": p["n_ambi"], "n_cigar": len(p["cigar"])}
    return MADE, r, extra, np.array(p["cigar"], np.uint32), ll


def read_pairs(opt, tcodes, qf, regs, ksw=K.ksw_extd):
    """Every slot of one read with the loop's rule (align.c:747-753) applied in order: a list of (code, r_inv, extra, cigar, ll) per region.
    ll is kept for a skipped candidate too (the device computes it on speculation)."""
    none = dict(zip(A.EXTRA_FIELDS, (0,) * 5))
    out, prev = [], False
    if len(regs) == 0:
        cover["read_without_regions"] += 1
    if len(regs) == 1:
        cover["read_with_one_region"] += 1
    for i, r in enumerate(regs):
        if i == 0:
            out.append((NONE, zero_reg(), none, np.zeros(0, np.uint32), None))
            prev = False
            continue
        code, r_inv, extra, cig, ll = align1_inv(opt, tcodes, qf, regs[i - 1], r, ksw)
        if prev and ll is not None:
            cover["skipped_behind_made"] += 1
            code, r_inv, extra, cig = SKIPPED, zero_reg(), none, np.zeros(0, np.uint32)
        elif code == MADE and i >= 2 and out[i - 1][4] is not None:
            cover["made_behind_failed"] += 1
        out.append((code, r_inv, extra, cig, ll))
        prev = code == MADE
    return out
