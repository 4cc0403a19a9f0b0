"""Python restatement of the reference's mm_align1 (align.c:423-636) as it runs with MM_F_SR and MM_F_SPLICE unset and q != q2 or
e != e2, on top of ksw_model.ksw_extd, plus the local-score model of ksw_ll_i16's return value.  tests/golden/make_align_golden.py
proves both equal to the compiled reference on every case of tests/align_shapes.py before the goldens are trusted.

A region is a dict of the REG_FIELDS (chaindp_reg_t / mm_reg1_t; `bits` is the bit-field word).  Anchors are two Python lists of
ints (x, y of mm128_t) that align1 changes in place (MM_SEED_IGNORE).  Every branch the tests name is counted in `cover`, and every DP
call is listed in `problems` as (kind, qlen, tlen, w, flag, pass): kind "left", "fill" or "right", pass 1 or 2.  The counters of the edge
tier (tests/align_edge_shapes.py) say where a size falls relative to what the device kernels do 64 lanes, 64 bases or one launch at a
time; none of them changes a result."""
import collections

import numpy as np

import ksw_model as K
import ksw_shapes as KS

SEED_LONG_JOIN, SEED_IGNORE, SEED_TANDEM, SEED_SELF = 1 << 40, 1 << 41, 1 << 42, 1 << 43
F_SPLICE, F_SR, F_FOR_ONLY, F_REV_ONLY = 0x80, 0x1000, 0x100000, 0x200000
PARENT_TMP_PRI = -2
BIT_SPLIT, BIT_REV, BIT_SAM_PRI, BIT_SPLIT_INV = 1 << 8, 1 << 10, 1 << 12, 1 << 24
EZ_RIGHT, EZ_APPROX_MAX, EZ_EXTZ_ONLY, EZ_REV_CIGAR = 0x02, 0x08, 0x40, 0x80
REG_FIELDS = ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0", "bits", "hash", "div")
OPT_FIELDS = ("a", "b", "q", "e", "q2", "e2", "bw", "zdrop", "zdrop_inv", "end_bonus", "min_cnt", "min_chain_score", "min_dp_max",
              "min_ksw_len", "max_gap", "flag", "k", "is_hpc")
EXTRA_FIELDS = ("has_extra", "dp_score", "dp_max", "n_ambi", "n_cigar")
M64 = (1 << 64) - 1

cover = collections.Counter()
problems = []         # (kind, qlen, tlen, w, flag, pass) of every DP call, in the order align1 makes them
ROUTE_NAMES = {KS.ROUTE_NONE: "none", KS.ROUTE_LDS: "lds", KS.ROUTE_GLOBAL: "global", KS.ROUTE_WIDE: "wide"}


class Undefined(Exception):
    """The reference would dereference a NULL r->p or trip an assert: no answer is specified."""


def i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def nt4(seq):
    """seq_nt4_table over a str or bytes: codes 0..4 as uint8."""
    t = np.full(256, 4, np.uint8)
    for c, v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("U", 3)):
        t[ord(c)] = t[ord(c.lower())] = v
    t[:4] = np.arange(4)
    return t[np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)]


def revcomp(codes):
    c = np.asarray(codes, np.uint8)[::-1]
    return np.where(c >= 4, 4, 3 - c).astype(np.uint8)


def simple_mat(a, b):
    mat = np.zeros((5, 5), np.int32)
    mat[:4, :4] = -abs(b)
    mat[np.arange(4), np.arange(4)] = abs(a)
    return mat


def ll_score(query, target, mat, gapo, gape):
    """The return value of ksw_ll_i16: the local affine Smith-Waterman score, gap of length l costing gapo + l * gape, 0 <= H <= 32767.
    Anti-diagonal by anti-diagonal, as the device kernel does it."""
    q, t = np.asarray(query, np.int64), np.asarray(target, np.int64)
    ql, tl = len(q), len(t)
    if ql == 0 or tl == 0:
        return 0
    oe = gapo + gape
    # index i + 1 holds the cell of target base i of a diagonal; index 0 is the border
    h1, h2, e1, f1 = (np.zeros(tl + 1, np.int64) for _ in range(4))
    best = 0
    for d in range(ql + tl - 1):
        lo, hi = max(0, d - ql + 1), min(tl - 1, d)
        i = np.arange(lo, hi + 1)
        s = mat[t[i], q[d - i]]
        e = np.maximum(h1[i] - oe, e1[i] - gape)              # from (i - 1, j): diagonal d - 1, index i
        f = np.maximum(h1[i + 1] - oe, f1[i + 1] - gape)      # from (i, j - 1): diagonal d - 1, index i + 1
        h = np.maximum(np.maximum(np.minimum(h2[i] + s, 32767), 0), np.maximum(e, f))     # _mm_adds_epi16 saturates
        e = np.maximum(e, 0); f = np.maximum(f, 0)
        nh, ne, nf = np.zeros(tl + 1, np.int64), np.zeros(tl + 1, np.int64), np.zeros(tl + 1, np.int64)
        nh[i + 1], ne[i + 1], nf[i + 1] = h, e, f
        h2, h1, e1, f1 = h1, nh, ne, nf
        best = max(best, int(h.max()))
    return best


def set_coor(r, qlen, ax, ay):
    """mm_reg_set_coor + mm_cal_fuzzy_len (hit.c:8-38)."""
    k, cnt = r["as"], r["cnt"]
    q_span = ay[k] >> 32 & 0xff
    rev = ax[k] >> 63
    r["bits"] = (r["bits"] & ~BIT_REV) | (rev << 10)
    r["rid"] = ((ax[k] << 1) & M64) >> 33
    r["rs"] = i32(ax[k]) + 1 - q_span if i32(ax[k]) + 1 > q_span else 0
    r["re"] = i32(ax[k + cnt - 1]) + 1
    if not rev:
        r["qs"], r["qe"] = i32(ay[k]) + 1 - q_span, i32(ay[k + cnt - 1]) + 1
    else:
        r["qs"], r["qe"] = qlen - (i32(ay[k + cnt - 1]) + 1), qlen - (i32(ay[k]) + 1 - q_span)
    mlen = blen = q_span
    for i in range(k + 1, k + cnt):
        span = ay[i] >> 32 & 0xff
        tl, ql = i32(ax[i]) - i32(ax[i - 1]), i32(ay[i]) - i32(ay[i - 1])
        blen += max(tl, ql)
        mlen += span if tl > span and ql > span else min(tl, ql)
    r["mlen"], r["blen"] = mlen, blen


def split_reg(r, r2, n, qlen, ax, ay):
    """mm_split_reg (hit.c:90-107); r2 is filled in place.  False where it returns early."""
    if n <= 0 or n >= r["cnt"]:
        return False
    r2.clear(); r2.update(r)
    r2["id"] = -1
    r2["bits"] &= ~(BIT_SAM_PRI | BIT_SPLIT_INV)
    r2["cnt"] = r["cnt"] - n
    ratio = np.float32(r2["cnt"]) / np.float32(r["cnt"])
    r2["score"] = int(float(np.float32(r["score"]) * ratio) + .499)
    r2["as"] = r["as"] + n
    if r["parent"] == r["id"]:
        r2["parent"] = PARENT_TMP_PRI
    set_coor(r2, qlen, ax, ay)
    r["cnt"] -= r2["cnt"]
    r["score"] -= r2["score"]
    set_coor(r, qlen, ax, ay)
    r["bits"] |= BIT_SPLIT; r2["bits"] |= BIT_SPLIT << 1
    return True


def fix_bad_ends(r, ax, ay, bw, min_match):
    as0, cnt0 = r["as"], r["cnt"]
    as1, cnt1 = as0, cnt0
    if cnt0 < 3:
        return as1, cnt1
    m = l = ay[as0] >> 32 & 0xff
    for i in range(as0 + 1, as0 + cnt0 - 1):
        q_span = ay[i] >> 32 & 0xff
        if ay[i] & SEED_LONG_JOIN:
            break
        lr, lq = i32(ax[i]) - i32(ax[i - 1]), i32(ay[i]) - i32(ay[i - 1])
        mn, mx = min(lr, lq), max(lr, lq)
        if mx - mn > l >> 1:
            as1 = i
        l += mn
        m += min(mn, q_span)
        if l >= bw << 1 or (m >= min_match and m >= bw) or m >= r["mlen"] >> 1:
            break
    cnt1 = as0 + cnt0 - as1
    m = l = ay[as0 + cnt0 - 1] >> 32 & 0xff
    for i in range(as0 + cnt0 - 2, as1, -1):
        q_span = ay[i + 1] >> 32 & 0xff
        if ay[i + 1] & SEED_LONG_JOIN:
            break
        lr, lq = i32(ax[i + 1]) - i32(ax[i]), i32(ay[i + 1]) - i32(ay[i])
        mn, mx = min(lr, lq), max(lr, lq)
        if mx - mn > l >> 1:
            cnt1 = i + 1 - as1
        l += mn
        m += min(mn, q_span)
        if l >= bw << 1 or (m >= min_match and m >= bw) or m >= r["mlen"] >> 1:
            break
    if as1 != as0:
        cover["fix_bad_ends_start"] += 1
    if as1 + cnt1 != as0 + cnt0:
        cover["fix_bad_ends_end"] += 1
    return as1, cnt1


def filter_bad_seeds(as1, cnt1, ax, ay, min_gap, diff_thres, max_ext_len, max_ext_cnt):
    def gap_at(i):
        return i32((i32(ay[as1 + i]) - i32(ay[as1 + i - 1])) - (i32(ax[as1 + i]) - i32(ax[as1 + i - 1])))
    K_ = [i for i in range(1, cnt1) if gap_at(i) < -min_gap or gap_at(i) > min_gap]
    n = len(K_)
    if n <= 1:
        cover["filter_n_le_1"] += 1
        return
    mx, max_st, max_en, runs = 0, -1, -1, 0
    k = 0
    while True:
        if k == n or k >= max_en:
            if max_en > 0:
                for i in range(K_[max_st], K_[max_en]):
                    ay[as1 + i] |= SEED_IGNORE
                runs += 1
            mx, max_st, max_en = 0, -1, -1
            if k == n:
                break
        i = K_[k]
        gap = gap_at(i)
        n_ins, n_del = (gap, 0) if gap > 0 else (0, -gap)
        qs, rs = i32(ay[as1 + i - 1]), i32(ax[as1 + i - 1])
        max_diff, max_diff_l = 0, -1
        l = k + 1
        while l < n and l <= k + max_ext_cnt:
            j = K_[l]
            if i32(ay[as1 + j]) - qs > max_ext_len or i32(ax[as1 + j]) - rs > max_ext_len:
                break
            gap = gap_at(j)
            if gap > 0:
                n_ins += gap
            else:
                n_del += -gap
            diff = n_ins + n_del - abs(n_ins - n_del)
            if max_diff < diff:
                max_diff, max_diff_l = diff, l
            l += 1
        if max_diff > diff_thres and max_diff > mx:
            mx, max_st, max_en = max_diff, k, max_diff_l
        k += 1
    cover["filter_runs_%d" % min(runs, 2)] += 1


def adjust_minier(opt, tcodes, qseq0, x, y):
    if opt["is_hpc"]:
        qseq = qseq0[x >> 63]
        q = i32(y)
        c = qseq[q]
        i = q - 1
        while i > 0 and qseq[i] == c:
            i -= 1
        q = i + 1
        t = tcodes[((x << 1) & M64) >> 33]
        off = i32(x)
        c = t[off]
        i = off - 1
        while i >= 0 and t[i] == c:
            i -= 1
        return i32(x) + 1 - (off - i), q
    return i32(x) - (opt["k"] >> 1), i32(y) - (opt["k"] >> 1)


def test_zdrop(opt, qseq, tseq, cigar, mat):
    """mm_test_zdrop (align.c:46-88)."""
    score, mx, max_i, max_j, i, j, max_zdrop = 0, -(1 << 31), -1, -1, 0, 0, 0
    pos = [[-1, -1], [-1, -1]]

    def update(score, i, j):
        nonlocal mx, max_i, max_j, max_zdrop
        if score < mx:
            li, lj = i - max_i, j - max_j
            z = mx - score - abs(li - lj) * opt["e"]
            if z > max_zdrop:
                max_zdrop = z
                pos[0][0], pos[0][1], pos[1][0], pos[1][1] = max_i, i + 1, max_j, j + 1
        else:
            mx, max_i, max_j = score, i, j

    for c in cigar:
        op, ln = int(c) & 0xf, int(c) >> 4
        if op == 0:
            for l in range(ln):
                score += int(mat[tseq[i + l], qseq[j + l]])
                update(score, i + l, j + l)
            i += ln; j += ln
        elif op in (1, 2, 3):
            score -= opt["q"] + opt["e"] * ln
            if op == 1:
                j += ln
            else:
                i += ln
            update(score, i, j)
    q_len, t_len = pos[1][1] - pos[1][0], pos[0][1] - pos[0][0]
    if not opt["flag"] & (F_SPLICE | F_SR | F_FOR_ONLY | F_REV_ONLY) and max_zdrop > opt["zdrop_inv"] and not (q_len < opt["max_gap"] and t_len < opt["max_gap"]):
        cover["inv_skipped_max_gap"] += 1
    if not opt["flag"] & (F_SPLICE | F_SR | F_FOR_ONLY | F_REV_ONLY) and max_zdrop > opt["zdrop_inv"] and q_len < opt["max_gap"] and t_len < opt["max_gap"]:
        qseq2 = revcomp(qseq[pos[1][0]:pos[1][1]])
        score = ll_score(qseq2, tseq[pos[0][0]:pos[0][1]], mat, opt["q"], opt["e"])
        cover["zdrop_inv_test"] += 1
        ll_seen.append((qseq2.copy(), np.array(tseq[pos[0][0]:pos[0][1]], np.uint8), score))
        inv_seen.append((q_len, t_len, score))
        cover["inv_t_le_64" if t_len <= 64 else "inv_t_65_128" if t_len <= 128 else "inv_t_gt_128"] += 1
        if t_len % 64 < 2:
            cover["inv_t_mod64_%d" % (t_len % 64)] += 1
        if q_len != t_len:
            cover["inv_q_gt_t" if q_len > t_len else "inv_q_lt_t"] += 1
        if score >= opt["min_chain_score"] * opt["a"] and score >= opt["min_dp_max"]:
            return 2
        cover["inv_below_threshold"] += 1
    return 1 if max_zdrop > opt["zdrop"] else 0


ll_seen = []          # (query, target, score) of every stretch test_zdrop gave to ll_score: the golden generator checks them against ksw_ll_i16
inv_seen = []         # (q_len, t_len, score) of the same stretches


def fix_cigar(r, cig, qseq, tseq):
    """mm_fix_cigar (align.c:90-146): cig is a list of words, changed in place; returns (qshift, tshift)."""
    if len(cig) <= 1:
        return 0, 0
    toff = qoff = 0
    to_shrink = False
    n = len(cig)
    for k in range(n):
        op, ln = cig[k] & 0xf, cig[k] >> 4
        if ln == 0:
            to_shrink = True
        if op == 0:
            toff += ln; qoff += ln
        elif op in (1, 2):
            if 0 < k < n - 1 and cig[k - 1] & 0xf == 0 and cig[k + 1] & 0xf == 0:
                prev_len = cig[k - 1] >> 4
                s, off = (qseq, qoff) if op == 1 else (tseq, toff)
                l = 0
                while l < prev_len and s[off - 1 - l] == s[off + ln - 1 - l]:
                    l += 1
                if l > 0:
                    cig[k - 1] -= l << 4; cig[k + 1] += l << 4; qoff -= l; toff -= l
                    cover["fix_cigar_shift"] += 1
                if l == prev_len:
                    to_shrink = True
                    cover["fix_cigar_shift_whole_M"] += 1
            if op == 1:
                qoff += ln
            else:
                toff += ln
        elif op == 3:
            toff += ln
    if to_shrink:
        kept = [c for c in cig if c >> 4]
        out = []
        for k, c in enumerate(kept):
            if k == len(kept) - 1 or c & 0xf != kept[k + 1] & 0xf:
                out.append(c)
            else:
                kept[k + 1] += c >> 4 << 4
        cig[:] = out
    qshift = tshift = 0
    if cig[0] & 0xf in (1, 2):
        l = cig[0] >> 4
        if cig[0] & 0xf == 1:
            if r["bits"] & BIT_REV:
                r["qe"] -= l
            else:
                r["qs"] += l
            qshift = l
            cover["fix_cigar_leading_I"] += 1
        else:
            r["rs"] += l
            tshift = l
            cover["fix_cigar_leading_D"] += 1
        del cig[0]
    return qshift, tshift


def update_extra(r, p, qseq, tseq, mat, q, e):
    """mm_update_extra (align.c:148-193) on p = dict(dp_score, dp_max, n_ambi, cigar)."""
    qshift, tshift = fix_cigar(r, p["cigar"], qseq, tseq)
    qseq, tseq = qseq[qshift:], tseq[tshift:]
    r["blen"] = r["mlen"] = 0
    toff = qoff = s = mx = 0
    mx_at = None          # (index of the M op, offset in it) where the final dp_max was first reached
    clamps = []           # (index of the M op, offset in it) of every clamp of s at 0 inside an M run
    for k, c in enumerate(p["cigar"]):
        op, ln = c & 0xf, c >> 4
        if op == 0:
            cq, ct = qseq[qoff:qoff + ln].astype(np.int64), tseq[toff:toff + ln].astype(np.int64)
            ambi = (cq > 3) | (ct > 3)
            n_ambi, n_diff = int(ambi.sum()), int((~ambi & (cq != ct)).sum())
            for l, v in enumerate(mat[ct, cq]):
                s += int(v)
                if s < 0:
                    s = 0
                    clamps.append((k, l))
                elif s > mx:
                    mx, mx_at = s, (k, l)
            if ln in (64, 65, 128, 129):
                cover["m_run_%d" % ln] += 1
            r["blen"] += ln - n_ambi; r["mlen"] += ln - (n_ambi + n_diff); p["n_ambi"] += n_ambi
            toff += ln; qoff += ln
        elif op in (1, 2):
            seq, off = (qseq, qoff) if op == 1 else (tseq, toff)
            n_ambi = int((seq[off:off + ln] > 3).sum())
            r["blen"] += ln - n_ambi; p["n_ambi"] += n_ambi
            if n_ambi:
                cover["n_ambi_in_gap"] += 1
            if s - (q + e * ln) < 0:
                cover["extra_gap_clamps"] += 1
            s = max(s - (q + e * ln), 0)
            if op == 1:
                qoff += ln
            else:
                toff += ln
        elif op == 3:
            toff += ln
    p["dp_max"] = mx
    if p["n_ambi"]:
        cover["n_ambi"] += 1
    # offsets past the first 64-base block of an M run, where the device carries s and the maximum from one block to the next
    for k, l in clamps:
        if l >= 63 and l % 64 in (63, 0):
            cover["extra_clamp_at_%d" % (l % 64)] += 1
    if mx_at is not None and mx_at[1] >= 63 and mx_at[1] % 64 in (63, 0):
        cover["extra_max_at_%d" % (mx_at[1] % 64)] += 1
    if mx_at is not None and any(k == mx_at[0] and l // 64 < mx_at[1] // 64 for k, l in clamps):
        cover["extra_clamp_then_max_later_block"] += 1


def align1(opt, tcodes, qf, ax, ay, r, ksw=K.ksw_extd):
    """mm_align1 on region r (changed in place) of the read with forward codes qf; tcodes[rid] are the targets' codes.  Returns
    (r2, extra, cigar): r2 a dict with cnt == 0 where nothing was split off, extra a dict of EXTRA_FIELDS, cigar a uint32 array."""
    r2 = {"cnt": 0}
    none = dict(zip(EXTRA_FIELDS, (0,) * 5))
    if r["cnt"] == 0:
        cover["cnt_0"] += 1
        return r2, none, np.zeros(0, np.uint32)
    qlen = len(qf)
    qseq0 = (np.asarray(qf, np.uint8), revcomp(qf))
    sc = tuple(opt[k] for k in ("a", "b", "q", "e", "q2", "e2"))
    mat = simple_mat(opt["a"], opt["b"])
    as0, cnt0 = r["as"], r["cnt"]
    rid, rev = ((ax[as0] << 1) & M64) >> 33, ax[as0] >> 63
    tseq_all, tlen = tcodes[rid], len(tcodes[rid])
    bw = int(opt["bw"] * 1.5 + 1.)
    n_a = len(ax)
    p = None
    cover["cnt_%d" % min(cnt0, 3)] += 1
    cover["strand_%d" % rev] += 1

    def append(cig):
        nonlocal p
        if len(cig) == 0:
            return
        if p is None:
            p = {"dp_score": 0, "dp_max": 0, "n_ambi": 0, "cigar": []}
        c = p["cigar"]
        if c and c[-1] & 0xf == int(cig[0]) & 0xf:
            c[-1] += int(cig[0]) >> 4 << 4
            c.extend(int(v) for v in cig[1:])
            cover["stitch_equal_ops"] += 1
        else:
            c.extend(int(v) for v in cig)

    def need_p():
        if p is None:
            raise Undefined("r->p is NULL")
        return p

    n_first_pass = 0

    def dp(kind, pas, long_join, qseq, tseq, w, zdrop, end_bonus, flag):
        nonlocal n_first_pass
        problems.append((kind, len(qseq), len(tseq), w, flag, pas))
        n_first_pass += pas == 1
        route = ROUTE_NAMES[KS.expected_route(len(qseq), len(tseq), sc)]
        cover["route_" + route] += 1
        if route == "wide":
            cover["route_wide_" + ("ext_" + kind if kind != "fill" else "long_join" if long_join else "fill_pass%d" % pas)] += 1
        return ksw(qseq, tseq, *sc, w, zdrop, end_bonus, flag)

    as1, cnt1 = fix_bad_ends(r, ax, ay, opt["bw"], opt["min_chain_score"] * 2)
    if cnt1 > 64:
        cover["cnt1_gt_64"] += 1
    if cnt1 > 128:
        cover["cnt1_gt_128"] += 1
    long_gaps = [i for i in range(1, cnt1) if abs(i32((i32(ay[as1 + i]) - i32(ay[as1 + i - 1])) - (i32(ax[as1 + i]) - i32(ax[as1 + i - 1])))) > 10]
    if len(long_gaps) >= 2 and sum(i <= 64 for i in long_gaps) <= 1:       # the first 64-lane stride alone would count at most one
        cover["long_gaps_only_past_64"] += 1
    filter_bad_seeds(as1, cnt1, ax, ay, 10, 40, opt["max_gap"] >> 1, 10)
    rs, qs = adjust_minier(opt, tcodes, qseq0, ax[as1], ay[as1])
    re, qe = adjust_minier(opt, tcodes, qseq0, ax[as1 + cnt1 - 1], ay[as1 + cnt1 - 1])

    span0 = ay[as0] >> 32 & 0xff
    rs0, qs0 = max(i32(ax[as0]) + 1 - span0, 0), i32(ay[as0]) + 1 - span0
    if qs0 < 0:
        raise Undefined("qs0 < 0")
    rs1 = qs1 = 0
    l, i = 0, as0 - 1
    while i >= 0 and ax[i] >> 32 == ax[as0] >> 32:
        sp = ay[i] >> 32 & 0xff
        x, y = i32(ax[i]) + 1 - sp, i32(ay[i]) + 1 - sp
        if x < rs0 and y < qs0:
            l += 1
            if l > opt["min_cnt"]:
                l = max(rs0 - x, qs0 - y)
                rs1, qs1 = rs0 - l, qs0 - l
                cover["neighbour_left"] += 1
                break
        i -= 1
    if qs > 0 and rs > 0:
        l = min(qs, opt["max_gap"])
        if qs1 > qs - l:
            cover["neighbour_left_binds_q"] += 1
        qs1 = max(qs1, qs - l)
        qs0 = min(qs0, qs1)
        l += (l * opt["a"] - opt["q"]) // opt["e"] if l * opt["a"] > opt["q"] else 0
        l = min(l, opt["max_gap"], rs)
        if rs1 > rs - l:
            cover["neighbour_left_binds_r"] += 1
        rs1 = max(rs1, rs - l)
        rs0 = min(rs0, rs1)
    else:
        rs0, qs0 = rs, qs
    re0, qe0 = i32(ax[as0 + cnt0 - 1]) + 1, i32(ay[as0 + cnt0 - 1]) + 1
    re1, qe1 = tlen, qlen
    l, i = 0, as0 + cnt0
    while i < n_a and ax[i] >> 32 == ax[as0] >> 32:
        x, y = i32(ax[i]) + 1, i32(ay[i]) + 1
        if x > re0 and y > qe0:
            l += 1
            if l > opt["min_cnt"]:
                l = max(x - re0, y - qe0)
                re1, qe1 = re0 + l, qe0 + l
                cover["neighbour_right"] += 1
                break
        i += 1
    if qe < qlen and re < tlen:
        l = min(qlen - qe, opt["max_gap"])
        if qe1 < qe + l:
            cover["neighbour_right_binds_q"] += 1
        qe1 = min(qe1, qe + l)
        qe0 = max(qe0, qe1)
        l += (l * opt["a"] - opt["q"]) // opt["e"] if l * opt["a"] > opt["q"] else 0
        l = min(l, opt["max_gap"], tlen - re)
        if re1 < re + l:
            cover["neighbour_right_binds_r"] += 1
        re1 = min(re1, re + l)
        re0 = max(re0, re1)
    else:
        re0, qe0 = re, qe
        cover["no_right_ext_" + ("read_end" if qe >= qlen else "target_end")] += 1
    if ay[as0] & SEED_SELF:
        cover["seed_self"] += 1
        max_ext = abs(r["qs"] - r["rs"])
        if r["rs"] - rs0 > max_ext:
            rs0 = r["rs"] - max_ext
        if r["qs"] - qs0 > max_ext:
            qs0 = r["qs"] - max_ext
        max_ext = abs(r["qe"] - r["re"])
        if re0 - r["re"] > max_ext:
            re0 = r["re"] + max_ext
        if qe0 - r["qe"] > max_ext:
            qe0 = r["qe"] + max_ext
    if not re0 > rs0:
        raise Undefined("re0 <= rs0")

    split_inv_in = bool(r["bits"] & BIT_SPLIT_INV)
    if split_inv_in:
        cover["split_inv_in"] += 1
    if qs > 0 and rs > 0:
        qseq = qseq0[rev][qs0:qs][::-1]
        tseq = tseq_all[rs0:rs][::-1]
        ez, cig = dp("left", 1, False, qseq, tseq, bw, opt["zdrop_inv"] if split_inv_in else opt["zdrop"], opt["end_bonus"],
                     EZ_EXTZ_ONLY | EZ_RIGHT | EZ_REV_CIGAR)
        if len(cig):
            append(cig)
            p["dp_score"] += int(ez[0])
        rs1 = rs - (int(ez[5]) + 1 if ez[9] else int(ez[3]) + 1)
        qs1 = qs - (qs - qs0 if ez[9] else int(ez[2]) + 1)
        cover["left_ext"] += 1
    else:
        rs1, qs1 = rs, qs
        cover["no_left_ext_" + ("qs" if qs <= 0 else "rs")] += 1
    re1, qe1 = rs, qs
    if qs1 < 0 or rs1 < 0:
        raise Undefined("qs1 < 0 or rs1 < 0")

    dropped = False
    for i in range(1, cnt1):
        y = ay[as1 + i]
        if y & (SEED_IGNORE | SEED_TANDEM) and i != cnt1 - 1:
            cover["skip_ignore" if y & SEED_IGNORE else "skip_tandem"] += 1
            continue
        re, qe = adjust_minier(opt, tcodes, qseq0, ax[as1 + i], y)
        re1, qe1 = re, qe
        if i == cnt1 - 1 or y & SEED_LONG_JOIN or (qe - qs >= opt["min_ksw_len"] and re - rs >= opt["min_ksw_len"]):
            bw1 = bw
            if y & SEED_LONG_JOIN:
                bw1 = max(qe - qs, re - rs)
                cover["long_join_" + ("last" if i == cnt1 - 1 else "inner")] += 1
            if y & SEED_TANDEM:
                cover["tandem_last"] += 1
            if qe < qs or re < rs:
                raise Undefined("negative fill")
            qseq, tseq = qseq0[rev][qs:qe], tseq_all[rs:re]
            long_join = bool(y & SEED_LONG_JOIN)
            ez, cig = dp("fill", 1, long_join, qseq, tseq, bw1, opt["zdrop"], -1, EZ_APPROX_MAX)
            code = test_zdrop(opt, qseq, tseq, cig, mat)
            cover["zdrop_code_%d" % code] += 1
            if code:
                ez, cig = dp("fill", 2, long_join, qseq, tseq, bw1, opt["zdrop_inv"] if code == 2 else opt["zdrop"], -1, 0)
            append(cig)
            if ez[1]:
                j = i - 1
                while j >= 0 and not i32(ax[as1 + j]) <= rs + int(ez[3]):
                    j -= 1
                dropped = True
                j = max(j, 0)
                need_p()["dp_score"] += int(ez[0])
                re1, qe1 = rs + int(ez[3]) + 1, qs + int(ez[2]) + 1
                if cnt1 - (j + 1) >= opt["min_cnt"]:
                    cover["drop_split"] += 1
                    if split_reg(r, r2, as1 + j + 1 - r["as"], qlen, ax, ay):
                        cover["drop_split_done"] += 1
                        if r["cnt"] > 64 and r2["cnt"] > 64:
                            cover["split_both_sides_gt_64"] += 1
                        if code == 2:
                            r2["bits"] |= BIT_SPLIT_INV
                            cover["drop_split_inv"] += 1
                else:
                    cover["drop_no_split"] += 1
                break
            need_p()["dp_score"] += int(ez[8])
            rs, qs = re, qe
        else:
            cover["skip_short"] += 1

    if not dropped and qe < qe0 and re < re0:
        ez, cig = dp("right", 1, False, qseq0[rev][qe:qe0], tseq_all[re:re0], bw, opt["zdrop"], opt["end_bonus"], EZ_EXTZ_ONLY)
        if len(cig):
            append(cig)
            p["dp_score"] += int(ez[0])
        re1 = re + (int(ez[5]) + 1 if ez[9] else int(ez[3]) + 1)
        qe1 = qe + (qe0 - qe if ez[9] else int(ez[2]) + 1)
        cover["right_ext"] += 1
        if qe0 == qlen:
            cover["right_ext_to_read_end"] += 1
        if re0 == tlen:
            cover["right_ext_to_target_end"] += 1
    if qe1 > qlen:
        raise Undefined("qe1 > qlen")
    if n_first_pass == cnt0 + 1:          # every slot the device gives the region holds a problem
        cover["slots_full"] += 1
    r["rs"], r["re"] = rs1, re1
    r["qs"], r["qe"] = (qlen - qe1, qlen - qs1) if rev else (qs1, qe1)
    if p is None:
        return r2, none, np.zeros(0, np.uint32)
    update_extra(r, p, qseq0[1 if r["bits"] & BIT_REV else 0][qs1:], tseq_all[rs1:re1], mat, opt["q"], opt["e"])
    extra = {"has_extra": 1, "dp_score": p["dp_score"], "dp_max": p["dp_max"], "n_ambi": p["n_ambi"], "n_cigar": len(p["cigar"])}
    return r2, extra, np.array(p["cigar"], np.uint32)
