"""CHECKER ONLY: a restatement of what the reference does with one read's hits after mm_gen_regs when nothing is aligned (map.c:870-877,
one segment): chain_post (map.c:238-247: mm_set_parent, mm_select_sub, mm_join_long), mm_est_err (through oracle_lib's C restatement)
and mm_set_mapq (hit.c:437-480), in Python with numpy float32 where the reference computes in float; logf is the host's, through libm.

Also the composition of the UNMODIFIED reference functions (oracle/_ref/libmm2chain_ref.so, where it is built) in the same order:
ref_post_read().  Both take and return REG_DTYPE records (tests/oracle_lib.py) and a read's chain anchors (uint64 [n, 2]).

`variant` restates one step the way it would read if the reference did not do what it does -- only the generator of the fixtures uses
it, to show that the fixtures tell the two apart:
  "meant_parent"    mm_select_sub compares with the r[p] it meant (the parent's record before any compaction) instead of the one it
                    reads (slot p, which may already hold a later kept hit)
  "mask_double"     mm_set_parent's mask test in double instead of float
  "sc_thres_float"  mm_join_long's sc_thres with a float add of .499 instead of the double add"""
import ctypes as C
import ctypes.util

import numpy as np

import oracle_lib as ol

MM_F_CIGAR, MM_F_SPLICE, MM_F_NO_LJOIN, MM_F_SR, MM_F_ALL_CHAINS = 0x004, 0x080, 0x400, 0x1000, 0x800000
MM_SEED_LONG_JOIN = np.uint64(1 << 40)
BIT_REV, BIT_INV, BIT_SAM_PRI, BIT_SEG_SPLIT = 1 << 10, 1 << 11, 1 << 12, 1 << 15
F32 = np.float32
INT_MIN = -(1 << 31)

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def host_logf(x):
    return F32(_libm.logf(float(F32(x))))


def _i32(x):
    return int(np.int64(x).astype(np.int32)) if -(1 << 63) <= x < (1 << 63) else int(np.uint64(x & ((1 << 64) - 1)).astype(np.int32))


def _cvtt(f):
    """(int)f as x86-64 converts it (cvttss2si): INT_MIN for NaN and outside the int range."""
    f = float(f)
    if not (f > -2147483904.0 and f < 2147483648.0):
        return INT_MIN
    return int(f)


def _wrap32(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


class _Trace:
    """What happened on a read (the generator's trap assertions read it)."""
    def __init__(self):
        self.select_sub_dropped = False
        self.slot_overwritten_read = False     # mm_select_sub compared a hit with a slot that a later hit had overwritten
        self.joined = 0
        self.fixup_chain = False               # the parent fix-up moved a parent
        self.squeezed = False
        self.squeeze_moved = False             # mm_squeeze_a changed some `as`
        self.sync_ran = False
        self.mapq_nonfinite = False            # mm_set_mapq converted a float outside the int range (or NaN) to int


def _set_coor(r, qlen, a):
    k, cnt = int(r["as"]), int(r["cnt"])
    f, l = a[k], a[k + cnt - 1]
    q_span = int(f[1] >> np.uint64(32) & np.uint64(0xff))
    rev = int(f[0] >> np.uint64(63))
    fx, fy, lx, ly = _i32(int(f[0])), _i32(int(f[1])), _i32(int(l[0])), _i32(int(l[1]))
    r["bits"] = (int(r["bits"]) & ~BIT_REV) | rev << 10
    r["rid"] = (int(f[0]) << 1 & ((1 << 64) - 1)) >> 33
    r["rs"] = fx + 1 - q_span if fx + 1 > q_span else 0
    r["re"] = lx + 1
    if not rev:
        r["qs"], r["qe"] = fy + 1 - q_span, ly + 1
    else:
        r["qs"], r["qe"] = qlen - (ly + 1), qlen - (fy + 1 - q_span)
    mlen = blen = q_span
    for i in range(k + 1, k + cnt):
        span = int(a[i][1] >> np.uint64(32) & np.uint64(0xff))
        tl = _i32(int(a[i][0])) - _i32(int(a[i - 1][0]))
        ql = _i32(int(a[i][1])) - _i32(int(a[i - 1][1]))
        blen += tl if tl > ql else ql
        mlen += span if (tl > span and ql > span) else (tl if tl < ql else ql)
    r["mlen"], r["blen"] = mlen, blen


@np.errstate(all="ignore")
def set_parent(r, mask_level, tr=None, variant=None):
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
            cov.sort()
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
                if variant == "mask_double":
                    v = ol_ / mn - uncov / mx if mn and mx else float(F32(ol_) / F32(mn) - F32(uncov) / F32(mx))
                    passed = v > float(ml)
                else:
                    passed = F32(ol_) / F32(mn) - F32(uncov) / F32(mx) > ml
                if passed:
                    found = p
                    break
        if found >= 0:
            rp = r[found]
            r[i]["parent"] = rp["parent"]
            rp["subsc"] = max(int(rp["subsc"]), int(r[i]["score"]))
            if r[i]["cnt"] >= rp["cnt"]:
                rp["n_sub"] += 1
        else:
            w.append(i)
            r[i]["parent"] = i
            r[i]["n_sub"] = 0


def sync_regs(r, tr=None):
    n = len(r)
    if n <= 0:
        return
    if tr is not None:
        tr.sync_ran = True
    max_id = int(r["id"].max())
    tmp = np.full(max_id + 1, -1, np.int64)
    for i in range(n):
        if r[i]["id"] >= 0:
            tmp[r[i]["id"]] = i
    for i in range(n):
        r[i]["id"] = i
        p = int(r[i]["parent"])
        if p == -2:
            r[i]["parent"] = i
        elif p >= 0 and p <= max_id and tmp[p] >= 0:
            r[i]["parent"] = tmp[p]
        else:
            r[i]["parent"] = -1
    n_pri = 0
    for i in range(n):
        if r[i]["id"] == r[i]["parent"]:
            n_pri += 1
            sp = n_pri == 1
        else:
            sp = False
        r[i]["bits"] = (int(r[i]["bits"]) & ~BIT_SAM_PRI) | (BIT_SAM_PRI if sp else 0)


def select_sub(r, pri_ratio, min_diff, best_n, tr=None, variant=None):
    n = len(r)
    if not (F32(pri_ratio) > F32(0) and n > 0):
        return r
    orig = r.copy()
    k = n_2nd = 0
    pr = F32(pri_ratio)
    for i in range(n):
        p = int(r[i]["parent"])
        if p == i or int(r[i]["bits"]) & BIT_INV:
            r[k] = r[i]; k += 1
            continue
        rp = orig[p] if variant == "meant_parent" else r[p]
        if tr is not None and r[p]["id"] != p:
            tr.slot_overwritten_read = True
        si, sp = int(r[i]["score"]), int(rp["score"])
        if (F32(si) >= F32(sp) * pr or si + min_diff >= sp) and n_2nd < best_n:
            if not (r[i]["qs"] == rp["qs"] and r[i]["qe"] == rp["qe"] and r[i]["rid"] == rp["rid"] and r[i]["rs"] == rp["rs"] and r[i]["re"] == rp["re"]):
                r[k] = r[i]; k += 1; n_2nd += 1
    r = r[:k].copy()
    if k != n:
        if tr is not None:
            tr.select_sub_dropped = True
        sync_regs(r, tr)
    return r


def squeeze_a(r, a, tr=None):
    order = sorted(range(len(r)), key=lambda i: (int(r[i]["as"]), i))
    out = a.copy()
    as_ = 0
    for i in order:
        if r[i]["as"] != as_:
            out[as_:as_ + r[i]["cnt"]] = a[r[i]["as"]:r[i]["as"] + r[i]["cnt"]]
            r[i]["as"] = as_
            if tr is not None:
                tr.squeeze_moved = True
        as_ += int(r[i]["cnt"])
    return out


def join_long(opt, qlen, r, a, tr=None, variant=None):
    n = len(r)
    if n < 2:
        return r, a
    if tr is not None:
        tr.squeezed = True
    a = squeeze_a(r, a, tr)
    aux = sorted([i for i in range(n) if r[i]["parent"] == i or r[i]["parent"] < 0], key=lambda i: (int(r[i]["as"]), i))
    n_drop = 0
    for ii in range(len(aux) - 1, 0, -1):
        r0, r1 = r[aux[ii - 1]], r[aux[ii]]
        if r0["as"] + r0["cnt"] != r1["as"]:
            continue
        if r0["rid"] != r1["rid"] or (int(r0["bits"]) ^ int(r1["bits"])) & BIT_REV:
            continue
        a0e, a1s = a[r0["as"] + r0["cnt"] - 1], a[r1["as"]]
        if int(a1s[0]) <= int(a0e[0]) or _i32(int(a1s[1])) <= _i32(int(a0e[1])):
            continue
        max_gap = min_gap = _i32(int(a1s[1])) - _i32(int(a0e[1]))
        dx = int(a1s[0]) - int(a0e[0])
        max_gap = max_gap if max_gap > dx else _i32(dx)
        min_gap = min_gap if min_gap < dx else _i32(dx)
        if max_gap > opt["max_join_long"] or min_gap > opt["max_join_short"]:
            continue
        fv = F32(opt["min_join_flank_sc"]) / F32(opt["max_join_long"]) * F32(max_gap)
        sc_thres = int(float(F32(fv) + F32(.499))) if variant == "sc_thres_float" else int(float(fv) + .499)
        if r0["score"] < sc_thres or r1["score"] < sc_thres:
            continue
        if r0["re"] - r0["rs"] < max_gap >> 1 or r0["qe"] - r0["qs"] < max_gap >> 1:
            continue
        if r1["re"] - r1["rs"] < max_gap >> 1 or r1["qe"] - r1["qs"] < max_gap >> 1:
            continue
        a[r1["as"]][1] |= MM_SEED_LONG_JOIN
        r0["cnt"] += r1["cnt"]
        r0["score"] += r1["score"]
        _set_coor(r0, qlen, a)
        r1["cnt"] = 0
        r1["parent"] = r0["id"]
        n_drop += 1
    if n_drop > 0:
        if tr is not None:
            tr.joined += n_drop
        for i in range(n):
            p = int(r[i]["parent"])
            if p >= 0 and r[i]["id"] != p:
                pp = int(r[p]["parent"])
                if pp >= 0 and pp != p:
                    if tr is not None and pp != p:
                        tr.fixup_chain = True
                    r[i]["parent"] = pp
        keep = [i for i in range(n) if not (not (int(r[i]["bits"]) & BIT_INV) and not (int(r[i]["bits"]) & BIT_SEG_SPLIT) and r[i]["cnt"] < opt["min_cnt"])]
        r = r[keep].copy()
        sync_regs(r, tr)
    return r, a


@np.errstate(all="ignore")
def set_mapq(r, min_chain_sc, rep_len, tr=None):
    sum_sc = int(sum(int(x["score"]) for x in r if x["parent"] == x["id"]))
    uniq_ratio = F32(sum_sc) / F32(sum_sc + rep_len)
    for x in r:
        bits = int(x["bits"])
        if bits & BIT_INV:
            mq = 0
        elif x["parent"] == x["id"]:
            score, cnt = int(x["score"]), int(x["cnt"])
            pen_s1 = (F32(1.0) if score > 100 else F32(0.01) * F32(score)) * uniq_ratio
            pen_cm = F32(1.0) if cnt > 10 else F32(0.1) * F32(cnt)
            pen_cm = pen_s1 if pen_s1 < pen_cm else pen_cm
            subsc = max(int(x["subsc"]), min_chain_sc)
            xx = F32(subsc) / F32(int(x["score0"]))
            q = pen_cm * F32(40.0) * (F32(1.0) - xx) * host_logf(score)
            mapq = _cvtt(q)
            if tr is not None and mapq == INT_MIN:
                tr.mapq_nonfinite = True
            sub = _cvtt(F32(4.343) * host_logf(int(x["n_sub"]) + 1) + F32(.499))
            mapq = _wrap32(mapq - sub)
            mapq = max(mapq, 0)
            mq = min(mapq, 60)
        else:
            mq = 0
        x["bits"] = (bits & ~0xff) | (mq & 0xff)


def post_read(opt, qlen, rep_len, ref_len, regs, b, mini_pos, tr=None, variant=None):
    """The restatement: one read's hits (mm_gen_regs' records) and chain anchors -> (final records, anchors as chain_post left them)."""
    r = np.array(regs, ol.REG_DTYPE, copy=True)
    a = np.array(b, np.uint64, copy=True).reshape(-1, 2)
    if not (opt["flag"] & MM_F_ALL_CHAINS):
        set_parent(r, opt["mask_level"], tr, variant)
        r = select_sub(r, opt["pri_ratio"], opt["min_diff"], opt["best_n"], tr, variant)
        if not (opt["flag"] & (MM_F_SPLICE | MM_F_SR | MM_F_NO_LJOIN)):
            r, a = join_long(opt, qlen, r, a, tr, variant)
    if not opt["is_sr"] and len(r) and len(mini_pos):
        r, _, _ = ol.oracle_est_err(ref_len, qlen, r, a, mini_pos)
    if not (opt["flag"] & MM_F_CIGAR):
        set_mapq(r, opt["min_chain_score"], rep_len, tr)
    return r, a


# ---- the unmodified reference, composed in chain_post's order -------------------------------------------------------------------

class MapOpt(C.Structure):
    """mm_mapopt_t (minimap.h:124-159)."""
    _fields_ = [("seed", C.c_int), ("sdust_thres", C.c_int), ("flag", C.c_int), ("bw", C.c_int), ("max_gap", C.c_int), ("max_gap_ref", C.c_int),
                ("max_frag_len", C.c_int), ("max_chain_skip", C.c_int), ("min_cnt", C.c_int), ("min_chain_score", C.c_int),
                ("mask_level", C.c_float), ("pri_ratio", C.c_float), ("best_n", C.c_int),
                ("max_join_long", C.c_int), ("max_join_short", C.c_int), ("min_join_flank_sc", C.c_int),
                ("a", C.c_int), ("b", C.c_int), ("q", C.c_int), ("e", C.c_int), ("q2", C.c_int), ("e2", C.c_int), ("noncan", C.c_int),
                ("zdrop", C.c_int), ("zdrop_inv", C.c_int), ("end_bonus", C.c_int), ("min_dp_max", C.c_int), ("min_ksw_len", C.c_int),
                ("anchor_ext_len", C.c_int), ("anchor_ext_shift", C.c_int), ("max_clip_ratio", C.c_float), ("pe_ori", C.c_int), ("pe_bonus", C.c_int),
                ("mid_occ_frac", C.c_float), ("min_mid_occ", C.c_int32), ("mid_occ", C.c_int32), ("max_occ", C.c_int32), ("mini_batch_size", C.c_int)]


_bound = False


def _ref():
    global _bound
    L = ol.ref()
    if not _bound:
        vp, i32 = C.c_void_p, C.c_int
        L.mm_set_parent.restype = None
        L.mm_set_parent.argtypes = [vp, C.c_float, i32, vp, i32]
        L.mm_select_sub.restype = None
        L.mm_select_sub.argtypes = [vp, C.c_float, i32, i32, vp, vp]
        L.mm_join_long.restype = None
        L.mm_join_long.argtypes = [vp, vp, i32, vp, vp, vp]
        L.mm_set_mapq.restype = None
        L.mm_set_mapq.argtypes = [vp, i32, vp, i32, i32, i32, i32]
        _bound = True
    return L


def ref_post_read(opt, qlen, rep_len, ref_len, regs, b, mini_pos):
    """map.c:870-877 for one single-segment read, by the reference's own functions: chain_post's body, mm_est_err, mm_set_mapq."""
    L = _ref()
    n = len(regs)
    raw = np.zeros((max(n, 1), ol.REF_REG_BYTES), np.uint8)
    raw[:n, :72] = np.ascontiguousarray(regs, ol.REG_DTYPE).view(np.uint8).reshape(n, 80)[:, :72]
    a = np.array(b, np.uint64, copy=True).reshape(-1, 2)
    a_buf = a if len(a) else np.zeros((1, 2), np.uint64)
    mo = MapOpt(flag=opt["flag"], min_cnt=opt["min_cnt"], min_chain_score=opt["min_chain_score"], mask_level=opt["mask_level"],
                pri_ratio=opt["pri_ratio"], best_n=opt["best_n"], max_join_long=opt["max_join_long"], max_join_short=opt["max_join_short"],
                min_join_flank_sc=opt["min_join_flank_sc"], a=opt["match_sc"], b=opt["sub_diff"] - 2 * opt["match_sc"])
    nn = C.c_int(n)
    if not (opt["flag"] & MM_F_ALL_CHAINS):
        L.mm_set_parent(None, opt["mask_level"], nn.value, raw.ctypes.data, opt["sub_diff"])
        L.mm_select_sub(None, opt["pri_ratio"], opt["min_diff"], opt["best_n"], C.addressof(nn), raw.ctypes.data)
        if not (opt["flag"] & (MM_F_SPLICE | MM_F_SR | MM_F_NO_LJOIN)):
            L.mm_join_long(None, C.addressof(mo), qlen, C.addressof(nn), raw.ctypes.data, a_buf.ctypes.data)
    n = nn.value
    out = np.zeros(n, ol.REG_DTYPE)
    out.view(np.uint8).reshape(n, 80)[:, :72] = raw[:n, :72]
    if not opt["is_sr"] and n and len(mini_pos):
        out = ol.ref_est_err(ref_len, qlen, out, a_buf, mini_pos)
        raw[:n, :72] = out.view(np.uint8).reshape(n, 80)[:, :72]
    if not (opt["flag"] & MM_F_CIGAR):
        L.mm_set_mapq(None, n, raw.ctypes.data, opt["min_chain_score"], opt["match_sc"], rep_len, opt["is_sr"])
        out.view(np.uint8).reshape(n, 80)[:, :72] = raw[:n, :72]
    return out, a_buf[:len(a)]


def opt_dict(po):
    """A PostOpt (ctypes) or a dict -> the dict the functions above take."""
    if isinstance(po, dict):
        return dict(po)
    d = po.asdict()
    d["mask_level"], d["pri_ratio"] = float(F32(d["mask_level"])), float(F32(d["pri_ratio"]))
    return d
