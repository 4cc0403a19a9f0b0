"""CHECKER ONLY: bases in, final hits with CIGARs out on the CPU, by composing the restatements the CPU tier pins to the reference --
e2e_model.model_map with MM_F_CIGAR in the post options (it stops after mm_est_err), the anchors as chain_post left them
(post_oracle.post_read once more on the model's own intermediates), mm_squeeze_a (map_align_shapes.squeeze), skeleton_model.run over
align_model and inv_model, and apost_model.run -- with nothing but glue in between.  tests/golden/make_map_align_golden.py proves the
composition equal to the compiled reference before the goldens are trusted.  numpy and the oracle libraries only; no GPU."""
import collections

import numpy as np

import apost_model as AM
import e2e_model as em
import map_align_shapes as S
import oracle_lib as ol
import post_oracle as po
import skeleton_model as K
from minimap2_chaindp_amd import params as P

OUTPUTS = ("regs_off", "regs", "extra", "dp_max2", "cigar_off", "cigar")
# What a scene's hand-off meets and what it feeds: the classes of the cover table that mapped reads of this size reach.  (cnt_65, cnt_257,
# regs_64, regs_65 and the lists on both sides of the LDS cap are map_align_shapes.SYNTHETIC's: hand-made regions and anchors.)
COVER = ("kept", "one_as_gt0", "order_differs", "joined_tail_cut", "no_ljoin_moved", "no_regions", "empty", "short", "n_only", "split", "inv_made",
         "sub_dropped")
# joined_then_moved -- mm_join_long joined, its mm_filter_regs dropped a region, and the skeleton's squeeze then moves an anchor -- is
# counted like the others and never occurs: mm_join_long's own mm_squeeze_a has packed the anchors, the region its filter drops has given
# its anchors to its neighbour (cnt 0), and mm_gen_regs makes no region below min_cnt.  What the skeleton's squeeze does to such a read is
# cut the tail that mm_select_sub's drops left above the packed anchors (joined_tail_cut).  tests/test_map_align_cpu.py holds both.
UNREACHABLE = ("joined_then_moved",)
cover = collections.Counter()


def align_row(aopt):
    """The row of align_model.OPT_FIELDS of a params.AlignOpt."""
    return np.array([getattr(aopt, k) for k, _ in aopt._fields_], np.int32)


def chain_post(sc, m):
    """(regs_off, regs, a_off, a, traces): every read's regions and anchors as chain_post and mm_est_err leave them, before the squeeze."""
    od = po.opt_dict(sc.opt)
    regs, a, traces = [], [], []
    for r in range(len(sc.reads)):
        tr = po._Trace()
        x, y = po.post_read(od, int(m.qlen[r]), int(m.rep_len[r]), sc.ref_len, m.regs_in[m.chains_off[r]:m.chains_off[r + 1]], m.b[m.b_off[r]:m.b_off[r + 1]],
                            m.mini_pos[m.mp_off[r]:m.mp_off[r + 1]], tr=tr)
        regs.append(x); a.append(y); traces.append(tr)
    cat = lambda parts, empty: np.concatenate(parts) if sum(len(p) for p in parts) else empty
    return (K.offsets([len(x) for x in regs]), cat(regs, np.zeros(0, ol.REG_DTYPE)), K.offsets([len(y) for y in a]), cat(a, np.zeros((0, 2), np.uint64)), traces)


def classify(sc, m, roff, regs, aoff, a, traces, out):
    """Counts the classes of COVER a scene reaches, read by read; returns the counter of this scene."""
    c = collections.Counter()
    for r in range(len(sc.reads)):
        x, n_b = regs[roff[r]:roff[r + 1]], int(aoff[r + 1] - aoff[r])
        kind = sc.kinds[r]
        if kind in ("empty", "short") or kind == "only_n":
            c["n_only" if kind == "only_n" else kind] += 1
        if len(x) == 0:
            c["no_regions"] += 1
            continue
        sq, _ = S.squeeze_read(x, a[aoff[r]:aoff[r + 1]])
        moved = bool((sq["as"] != x["as"]).any())
        if not moved and int(x["cnt"].sum()) == n_b:
            c["kept"] += 1
        if len(x) == 1 and int(x["as"][0]) > 0:
            c["one_as_gt0"] += 1
        if moved and list(np.argsort(x["as"], kind="stable")) != list(range(len(x))):
            c["order_differs"] += 1
        no_ljoin = bool(sc.opt.flag & (P.MM_F_NO_LJOIN | P.MM_F_ALL_CHAINS))
        if not no_ljoin and traces[r].joined > 0:
            c["joined_then_moved" if moved else "joined_tail_cut" if int(x["cnt"].sum()) < n_b else "joined_whole"] += 1
        if moved and no_ljoin and len(x) > 1:
            c["no_ljoin_moved"] += 1
    return c


def run(sc):
    """The scene through every stage: dict of OUTPUTS, a (the squeezed anchors with the alignment's marks) and a_off, and the hand-off's
    own result beside them (sq_regs_off, sq_regs, sq_a_off, sq_a) with rep_len and n_anchors."""
    m = em.model_of(sc)
    roff, regs, aoff, a, traces = chain_post(sc, m)
    assert np.array_equal(roff, m.regs_off) and regs.tobytes() == m.regs.tobytes()
    sq_regs, sq_aoff, sq_a = S.squeeze(roff, regs, aoff, a)
    reads = [dict(seq=np.frombuffer(sc.reads[r], np.uint8), a=sq_a[sq_aoff[r]:sq_aoff[r + 1]], regs=sq_regs[roff[r]:roff[r + 1]]) for r in range(len(sc.reads))]
    row = align_row(sc.aopt)
    trace = []
    sk = K.run(K.opt_dict(row), reads, *K.cpu_stages(row, sc.tseq_off, sc.tseq), trace=trace)
    ap = AM.run(po.opt_dict(sc.opt), m.rep_len, sk["regs_off"], sk["regs"], sk["extra"], sk["cigar_off"], sk["cigar"])
    c = classify(sc, m, roff, regs, aoff, a, traces, ap)
    c["split"] += sum(int((t["regs2"]["cnt"] > 0).sum()) for t in trace if t["stage"] == "align1")
    c["inv_made"] += int((trace[-1]["made"] == 1).sum())
    c["sub_dropped"] += int(len(sk["regs"]) - len(ap["regs"]))
    cover.update(c)
    out = {k: ap[k] for k in OUTPUTS}
    out.update(a_off=sq_aoff, a=sk["a"], sq_regs_off=roff, sq_regs=sq_regs, sq_a_off=sq_aoff, sq_a=sq_a, rep_len=m.rep_len, n_anchors=np.int64(m.n_anchors), cover=c)
    return out
