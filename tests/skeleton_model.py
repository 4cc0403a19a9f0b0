"""The loop around the alignment stages (the reference's mm_align_skeleton, align.c:705-761), written once over two callables, so that
the CPU tier and the GPU tier run the same loop code and differ only in the stage implementation:

  align1_batch(seq_off, seq, a_off, a, regs_off, regs) -> (a, regs, regs2, extra, cigar_off, cigar)       as Device.align1
  inv_batch(seq_off, seq, regs_off, regs)              -> (made, r_inv, extra, cigar_off, cigar)          as Device.align1_inv

run() composes them the way a batched host must: round 0 aligns every region of every read, round k exactly the regions round k - 1
split off (regs2.cnt > 0) with the anchors as round k - 1 returned them, until nothing is split off; each split-off region stands
behind its parent (mm_insert_reg); one inv_batch call over the final lists; every made == 1 record behind its right region; then
mm_filter_regs (hit.c:249-268, max_clip_ratio at mm_mapopt_init's 1.0) and mm_hit_sort_by_dp (hit.c:167-193) as restatements, the sort
with the order radix_sort_128x gives equal keys (sort_pairs).  Where a record stood in the list cannot be read off the final regions:
run() also returns the list as it stands before the filter, which the golden generator records from the reference's own loop.
tests/golden/make_skeleton_golden.py proves run() over the CPU models equal to the compiled mm_align_skeleton before the goldens are
trusted.  Every loop case the tests name is counted in `cover`; the counters change no result."""
import collections

import numpy as np

import align_model as A
import align_shapes as S
import inv_model as M
import inv_shapes as IS
from align_shapes import EXTRA_DTYPE, REG_DTYPE

BIT_INV, BIT_SEG_SPLIT = 1 << 11, 1 << 15
MAX_CLIP_RATIO = np.float32(1.0)
COVER = ("rounds_1", "rounds_2", "rounds_3plus", "r2_range_has_ignored_seed", "r2_filtered_after_alignment", "read_pending_beside_read_done",
         "inv_made", "inv_low_score", "inv_skipped_behind_made", "inv_made_behind_failed", "inv_early_return_on_device_made_regions",
         "filtered_min_cnt", "filtered_mlen", "filtered_dp_max", "sort_changes_order", "strand_0", "strand_1", "read_on_two_targets")
OUTPUTS = ("placed_off", "placed", "regs_off", "regs", "extra", "cigar_off", "cigar", "a")

cover = collections.Counter()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)


def words(x):
    return x.view(np.uint32) if x.dtype.fields else x


def _cat(parts, dtype):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)


def _slot(reg, born, extra=None, cigar=None):
    return dict(reg=np.array(reg, REG_DTYPE).reshape(1), extra=np.zeros(1, EXTRA_DTYPE) if extra is None else np.array(extra, EXTRA_DTYPE).reshape(1),
                cigar=np.zeros(0, np.uint32) if cigar is None else np.array(cigar, np.uint32), born=born)


def filter_regs(opt, qlen, slots):
    """mm_filter_regs over one read's slots."""
    kept = []
    for s in slots:
        r, bits = s["reg"][0], int(s["reg"]["bits"][0])
        flt = why = None
        if not bits & BIT_INV and not bits & BIT_SEG_SPLIT and int(r["cnt"]) < opt["min_cnt"]:
            flt = why = "min_cnt"
        if s["extra"]["has_extra"][0]:            # r->p: these filters are only applied when base-alignment is available
            if int(r["mlen"]) < opt["min_chain_score"]:
                flt = "mlen"
            elif int(s["extra"]["dp_max"][0]) < opt["min_dp_max"]:
                flt = "dp_max"
            elif np.float32(int(r["qs"])) > np.float32(qlen) * MAX_CLIP_RATIO and np.float32(qlen - int(r["qe"])) > np.float32(qlen) * MAX_CLIP_RATIO:
                flt = "clip"
        if why:
            cover["filtered_min_cnt"] += 1
        if flt and flt != "min_cnt":
            cover["filtered_" + flt] += 1
        if flt and s["born"] >= 1 and s["extra"]["has_extra"][0] and not bits & BIT_INV:
            cover["r2_filtered_after_alignment"] += 1
        if not flt:
            kept.append(s)
    return kept


def _insertion(a, beg, end):
    """Rising by key, an element moved only past strictly larger ones: equal keys keep their order."""
    for i in range(beg + 1, end):
        if a[i][0] < a[i - 1][0]:
            t, j = a[i], i
            while j > beg and t[0] < a[j - 1][0]:
                a[j] = a[j - 1]
                j -= 1
            a[j] = t


def sort_pairs(pairs, top=64):
    """The order the reference's radix_sort_128x (ksort.h:101-151) leaves (key, y) pairs in, rising by key, as csrc/chaindp_rsort.h follows
    it: up to 64 pairs by insertion, stable; more in place, byte by byte from the top one -- count the range's digits, walk the buckets
    upwards and carry each element that lies in a wrong bucket to the next free place of its own, taking up what lies there, until one
    comes back for the place the walk left; then every bucket of more than 64 is a range of the next byte and every one of 2 to 64 is
    sorted by insertion.  Equal keys end where the carrying left them.  top: the first threshold, for a test to move."""
    a = list(pairs)
    if len(a) <= top:
        _insertion(a, 0, len(a))
        return a
    stack = [(0, len(a), 56)]
    while stack:
        beg, end, shift = stack.pop()
        digit = lambda q: a[q][0] >> shift & 0xff
        tail = [0] * 256
        for q in range(beg, end):
            tail[digit(q)] += 1
        head, acc = [0] * 256, beg
        for d in range(256):
            head[d] = acc
            acc += tail[d]
            tail[d] = acc
        d = 0
        while d < 256:
            if head[d] == tail[d]:
                d += 1
                continue
            to = digit(head[d])
            if to != d:
                carry = a[head[d]]
                while to != d:
                    carry, a[head[to]] = a[head[to]], carry
                    head[to] += 1
                    to = carry[0] >> shift & 0xff
                a[head[d]] = carry
            head[d] += 1
        if shift:
            b = beg
            for d in range(256):
                e = tail[d]
                if e - b > 64:
                    stack.append((b, e, max(shift - 8, 0)))
                elif e - b > 1:
                    _insertion(a, b, e)
                b = e
    return a


def hit_sort_by_dp(slots):
    """mm_hit_sort_by_dp over one read's slots: by dp_max << 32 | hash, falling; equal keys as radix_sort_128x over the live regions and
    the reversal behind it leave them (up to 64 live regions: the later one first)."""
    if len(slots) <= 1:
        return slots
    live = [s for s in slots if int(s["reg"]["bits"][0]) & BIT_INV or int(s["reg"]["cnt"][0]) > 0]
    if not all(s["extra"]["has_extra"][0] for s in live):
        raise A.Undefined("a region reaches the sort with p == NULL")
    keys = [int(s["extra"]["dp_max"][0]) << 32 | int(s["reg"]["hash"][0]) for s in live]
    order = [i for _, i in sort_pairs(list(zip(keys, range(len(live)))))][::-1]
    if order != list(range(len(live))):
        cover["sort_changes_order"] += 1
    if len(set(keys)) != len(keys):
        cover["sort_key_tie"] += 1
    return [live[i] for i in order]


def run(opt, reads, align1_batch, inv_batch, trace=None):
    """opt: dict of align_model.OPT_FIELDS.  reads: [dict(seq uint8[] characters, a uint64[n, 2] after mm_squeeze_a, regs REG_DTYPE[m])].
    Returns dict(placed_off, placed, regs_off, regs, extra, cigar_off, cigar, a): each read's list as the loop leaves it for
    mm_filter_regs (split-off regions and inversions in their places; the sort hides the places afterwards), its final regions (every
    word of REG_DTYPE), what r->p holds beside the CIGAR, the CIGARs as CSR over the regions, and the anchors with their marks (a_off
    is the input's); beside these OUTPUTS placed_extra, what r->p holds for every record of placed.  trace, a list, gets one dict per stage call with its inputs and outputs."""
    seq_off, seq = offsets([len(rd["seq"]) for rd in reads]), _cat([np.asarray(rd["seq"], np.uint8) for rd in reads], np.uint8)
    a_off = offsets([len(rd["a"]) for rd in reads])
    a = _cat([np.asarray(rd["a"], np.uint64).reshape(-1, 2) for rd in reads], np.uint64).reshape(-1, 2)
    lists = [[_slot(r, 0) for r in rd["regs"]] for rd in reads]
    pending = [list(l) for l in lists]
    rnd = 0
    while any(pending):
        regs_off = offsets([len(p) for p in pending])
        regs = _cat([s["reg"] for p in pending for s in p], REG_DTYPE)
        if rnd >= 1:
            if any(not p and l for p, l in zip(pending, lists)):
                cover["read_pending_beside_read_done"] += 1
            for rd, p in enumerate(pending):
                for s in p:
                    lo = int(a_off[rd]) + int(s["reg"]["as"][0])
                    if (a[lo:lo + int(s["reg"]["cnt"][0]), 1] & np.uint64(A.SEED_IGNORE)).any():
                        cover["r2_range_has_ignored_seed"] += 1
        a_in = a
        a, regs_out, regs2, extra, coff, cig = align1_batch(seq_off, seq, a_off, a_in, regs_off, regs)
        if trace is not None:
            trace.append(dict(stage="align1", round=rnd, seq_off=seq_off, seq=seq, a_off=a_off, a_in=a_in, regs_off=regs_off, regs_in=regs, a=a,
                              regs=regs_out, regs2=regs2, extra=extra, cigar_off=coff, cigar=cig))
        g, nxt = 0, []
        for rd, p in enumerate(pending):
            new = []
            for s in p:
                s["reg"], s["extra"] = regs_out[g:g + 1].copy(), extra[g:g + 1].copy()
                s["cigar"] = np.array(cig[int(coff[g]):int(coff[g + 1])], np.uint32)
                if int(regs2["cnt"][g]) > 0:                                    # align.c:747: behind its parent
                    t = _slot(regs2[g], rnd + 1)
                    lists[rd].insert(next(i for i, x in enumerate(lists[rd]) if x is s) + 1, t)
                    new.append(t)
                g += 1
            nxt.append(new)
        pending, rnd = nxt, rnd + 1
    for l in lists:
        if l:
            n = 1 + max(s["born"] for s in l)
            cover["rounds_%d" % n if n < 3 else "rounds_3plus"] += 1
    # one inversion call over the final lists (align.c:748-752)
    regs_off = offsets([len(l) for l in lists])
    regs = _cat([s["reg"] for l in lists for s in l], REG_DTYPE)
    made, r_inv, iextra, icoff, icig = inv_batch(seq_off, seq, regs_off, regs)
    if trace is not None:
        trace.append(dict(stage="align1_inv", round=rnd, seq_off=seq_off, seq=seq, regs_off=regs_off, regs_in=regs, made=made, r_inv=r_inv, extra=iextra,
                          cigar_off=icoff, cigar=icig))
    g, final = 0, []
    for l in lists:
        out = []
        for i, s in enumerate(l):
            out.append(s)
            code = int(made[g])
            if code == M.MADE:                                                  # :750: behind the right region, and stepped over
                out.append(_slot(r_inv[g], rnd, iextra[g], icig[int(icoff[g]):int(icoff[g + 1])]))
                cover["inv_made"] += 1
                if i >= 2 and int(made[g - 1]) not in (M.NONE, M.MADE):
                    cover["inv_made_behind_failed"] += 1
            elif code == M.LOW_SCORE:
                cover["inv_low_score"] += 1
            elif code == M.SKIPPED:
                cover["inv_skipped_behind_made"] += 1
            elif code == M.NO_CIGAR:
                cover["inv_no_cigar"] += 1
            elif i >= 1 and s["born"] >= 1 and int(s["reg"]["bits"][0]) & M.BIT_SPLIT_INV:
                cover["inv_early_return_on_device_made_regions"] += 1
            g += 1
        final.append(out)
    placed_off, placed = offsets([len(l) for l in final]), _cat([s["reg"] for l in final for s in l], REG_DTYPE)
    placed_extra = _cat([s["extra"] for l in final for s in l], EXTRA_DTYPE)
    for rd, l in enumerate(final):
        final[rd] = l = hit_sort_by_dp(filter_regs(opt, int(seq_off[rd + 1] - seq_off[rd]), l))
        for s in l:
            cover["strand_%d" % (int(s["reg"]["bits"][0]) >> 10 & 1)] += 1
        if len({int(s["reg"]["rid"][0]) for s in l}) > 1:
            cover["read_on_two_targets"] += 1
    flat = [s for l in final for s in l]
    return dict(placed_off=placed_off, placed=placed, placed_extra=placed_extra, regs_off=offsets([len(l) for l in final]), regs=_cat([s["reg"] for s in flat], REG_DTYPE), extra=_cat([s["extra"] for s in flat], EXTRA_DTYPE),
                cigar_off=offsets([len(s["cigar"]) for s in flat]), cigar=_cat([s["cigar"] for s in flat], np.uint32), a=a)


def cpu_stages(opt_row, tseq_off, tseq):
    """The CPU pair: align_model.align1 and inv_model.read_pairs over the targets, as align_shapes / inv_shapes batch them."""
    base = dict(opt=np.asarray(opt_row, np.int32), tseq_off=np.asarray(tseq_off, np.int64), tseq=np.asarray(tseq, np.uint8))

    def align1_batch(seq_off, seq, a_off, a, regs_off, regs):
        return S.model_scene(dict(base, seq_off=seq_off, seq=seq, a_off=a_off, a=a, regs_off=regs_off, regs=regs))

    def inv_batch(seq_off, seq, regs_off, regs):
        return IS.model_scene(dict(base, seq_off=seq_off, seq=seq, regs_off=regs_off, regs=regs))[:5]
    return align1_batch, inv_batch


def reads_of(p):
    """The reads of a packed scene (align_shapes.pack's arrays or a loaded golden) as run() takes them."""
    return [dict(seq=p["seq"][int(p["seq_off"][i]):int(p["seq_off"][i + 1])], a=p["a"][int(p["a_off"][i]):int(p["a_off"][i + 1])],
                 regs=p["regs"][int(p["regs_off"][i]):int(p["regs_off"][i + 1])]) for i in range(len(p["seq_off"]) - 1)]


def opt_dict(opt_row):
    return dict(zip(A.OPT_FIELDS, (int(v) for v in opt_row)))


def run_scene(p, stages=None, trace=None):
    """run() over a packed scene, by default with the CPU pair."""
    return run(opt_dict(p["opt"]), reads_of(p), *(stages or cpu_stages(p["opt"], p["tseq_off"], p["tseq"])), trace=trace)
