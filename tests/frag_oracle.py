"""CHECKER ONLY: a restatement of what the reference does with one fragment's hits after mm_gen_regs when nothing is aligned and the read
has several segments (read_result_handle, map.c:870-890): chain_post with mm_select_sub_multi (pe.c:6-43) in the place of mm_select_sub,
mm_seg_gen (hit.c:347-401) and per segment mm_set_parent and mm_set_mapq -- in Python on top of tests/post_oracle.py (the steps shared
with the one-segment path) and oracle_lib.oracle_gen_regs (mm_gen_regs, pinned to the reference by the CPU tier).  A read of one
segment goes through post_oracle.post_read unchanged.

`variant` restates one step the way it would read if the reference did not do what it does -- only the generator of the fixtures uses
it, to show that the fixtures tell the two apart:
  "pri1_double"    p->score * pri1 (pe.c:20) as a double product instead of the float product
  "no_chi_both"    pe.c:25 without `is_chi_both ||`"""
import numpy as np

import oracle_lib as ol
import post_oracle as po

F32 = np.float32
MM_SEED_SEG_SHIFT = np.uint64(48)
BIT_SEG_ID_SHIFT = 16
PRI1, PRI2 = F32(0.2), F32(0.7)           # map.c:243
BRANCHES = ("primary", "min_diff", "close", "close_pri1", "chi_both", "equal_pri_ratio", "par_only_pri2")


class FragTrace(po._Trace):
    """What happened on a fragment (the generator's trap assertions read it).  branch[name] = [times false, times true] for every
    test of pe.c:13-32."""
    def __init__(self):
        super().__init__()
        self.branch = {k: [0, 0] for k in BRANCHES}
        self.best_n_cut = False
        self.multi_dropped = False
        self.squeezed_zero = False            # a hit without anchors in some segment (hit.c:373-375)
        self.empty_segment = False            # a segment without hits
        self.reverse_hit = False
        self.seg_chains_max = 0               # most chains one segment's mm_gen_regs got
        self.seg_equal_keys = False           # ... and whether two of them had equal sort keys

    def _b(self, name, val):
        self.branch[name][1 if val else 0] += 1
        return val


def select_sub_multi(r, pri_ratio, max_gap_ref, min_diff, best_n, n_segs, qlens, tr=None, variant=None):
    n = len(r)
    if not (F32(pri_ratio) > F32(0) and n > 0):
        return r
    tr = tr if tr is not None else FragTrace()
    pr = F32(pri_ratio)
    max_dist = qlens[0] + qlens[1] + max_gap_ref if n_segs == 2 else 0
    k = n_2nd = 0
    for i in range(n):
        q = r[i]
        par = int(q["parent"])
        keep = False
        if tr._b("primary", par == i):
            keep = True
        else:
            p = r[par]
            if p["id"] != par:
                tr.slot_overwritten_read = True
            si, sp = int(q["score"]), int(p["score"])
            if tr._b("min_diff", si + min_diff >= sp):
                keep = True
            elif tr._b("close", not ((int(p["bits"]) ^ int(q["bits"])) & po.BIT_REV) and p["rid"] == q["rid"] and int(q["re"]) - int(p["rs"]) < max_dist
                       and int(p["re"]) - int(q["rs"]) < max_dist):
                thr = float(sp) * float(PRI1) if variant == "pri1_double" else F32(sp) * PRI1
                keep = tr._b("close_pri1", (float(si) if variant == "pri1_double" else F32(si)) >= thr)
            else:
                par_both = n_segs == 2 and p["qs"] < qlens[0] and p["qe"] > qlens[0]
                chi_both = n_segs == 2 and q["qs"] < qlens[0] and q["qe"] > qlens[0]
                tr._b("chi_both", chi_both)
                first = (chi_both == par_both) if variant == "no_chi_both" else (chi_both or chi_both == par_both)
                if first:
                    keep = F32(si) >= F32(sp) * pr
                    if not chi_both:
                        tr._b("equal_pri_ratio", keep)
                else:
                    keep = F32(si) >= F32(sp) * PRI2
                    if not chi_both:
                        tr._b("par_only_pri2", keep)
        if keep and par != i:
            if n_2nd >= best_n:
                keep = False
                tr.best_n_cut = True
            n_2nd += 1
        if keep:
            r[k] = r[i]; k += 1
    r = r[:k].copy()
    if k != n:
        tr.multi_dropped = True
        tr.select_sub_dropped = True
        po.sync_regs(r, tr)
    return r


def seg_gen(hash_, qlens, regs0, a, tr=None):
    """mm_seg_gen: -> per segment (records of mm_gen_regs with seg_split / seg_id set, the segment's anchors)."""
    n_segs = len(qlens)
    acc = np.concatenate(([0], np.cumsum(qlens)[:-1])).astype(np.int64)
    qlen_sum = int(np.sum(qlens))
    us = [[] for _ in range(n_segs)]
    as_ = [[] for _ in range(n_segs)]
    for x in regs0:
        k, cnt = int(x["as"]), int(x["cnt"])
        part = a[k:k + cnt]
        sid = (part[:, 1] >> MM_SEED_SEG_SHIFT & np.uint64(0xff)).astype(np.int64)
        if tr is not None and (int(x["bits"]) & po.BIT_REV):
            tr.reverse_hit = True
        for s in range(n_segs):
            mine = part[sid == s].copy()
            if not len(mine):
                if tr is not None:
                    tr.squeezed_zero = True
                continue
            off = np.where(mine[:, 0] >> np.uint64(63) != 0, qlen_sum - (int(qlens[s]) + int(acc[s])), int(acc[s])).astype(np.int64)
            mine[:, 1] = mine[:, 1] - off.astype(np.uint64)                 # hit.c:388 (uint64 arithmetic)
            us[s].append((int(x["score"]) << 32) + len(mine))
            as_[s].append(mine)
    out = []
    for s in range(n_segs):
        u = np.array(us[s], np.uint64)
        sa = np.concatenate(as_[s]) if as_[s] else np.zeros((0, 2), np.uint64)
        regs = ol.oracle_gen_regs(int(hash_), int(qlens[s]), u, sa)
        regs["bits"] |= np.uint32(po.BIT_SEG_SPLIT | s << BIT_SEG_ID_SHIFT)
        if tr is not None:
            tr.empty_segment |= len(u) == 0
            tr.seg_chains_max = max(tr.seg_chains_max, len(u))
            if len(u) > 1:
                key = regs["score"].astype(np.uint64) << np.uint64(32) | regs["hash"].astype(np.uint64)
                tr.seg_equal_keys |= len(np.unique(key)) < len(key)
        out.append((regs, sa))
    return out


def frag_read(opt, max_gap_ref, hash_, qlens, rep_len, ref_len, regs_in, b, mini_pos, tr=None, variant=None):
    """The restatement: one read's hits (mm_gen_regs' records on the fragment) and chain anchors -> per segment (final records, anchors)."""
    qlens = [int(x) for x in qlens]
    qlen = sum(qlens)
    if len(qlens) == 1:
        r, a = po.post_read(opt, qlen, rep_len, ref_len, regs_in, b, mini_pos, tr=tr)
        return [(r, a)]
    r = np.array(regs_in, ol.REG_DTYPE, copy=True)
    a = np.array(b, np.uint64, copy=True).reshape(-1, 2)
    if not (opt["flag"] & po.MM_F_ALL_CHAINS):                              # chain_post, map.c:238-247
        po.set_parent(r, opt["mask_level"], tr)
        r = select_sub_multi(r, opt["pri_ratio"], max_gap_ref, opt["min_diff"], opt["best_n"], len(qlens), qlens, tr, variant)
        if not (opt["flag"] & (po.MM_F_SPLICE | po.MM_F_SR | po.MM_F_NO_LJOIN)):
            r, a = po.join_long(opt, qlen, r, a, tr)
    out = []                                                                # (mm_est_err, map.c:872: its div does not survive mm_seg_gen)
    for regs, sa in seg_gen(hash_, qlens, r, a, tr):
        po.set_parent(regs, opt["mask_level"])
        if not (opt["flag"] & po.MM_F_CIGAR):
            po.set_mapq(regs, opt["min_chain_score"], rep_len)
        out.append((regs, sa))
    return out


def flip_back(regs, qlen):
    """map.c:624-630 on one segment's final hits."""
    regs = regs.copy()
    qs = regs["qs"].copy()
    regs["qs"] = qlen - regs["qe"]
    regs["qe"] = qlen - qs
    regs["bits"] ^= np.uint32(po.BIT_REV)
    return regs
