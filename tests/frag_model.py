"""CHECKER ONLY: seeded inputs and the composed CPU model for reads of several segments (paired reads).

  shapes()        hand-made and seeded fragments as anchors (sorted by x per read, as map.c:233 leaves them; y = seg << 48 | span << 32 |
                  position in the concatenated fragment, map.c:220-227) whose chains under `sr` chaining parameters give the hit layouts
                  mm_select_sub_multi and mm_seg_gen are sensitive to: tests/golden/make_frag_golden.py runs the reference on them.
  scenario()      a seeded `sr` batch of 2 x 150 bp fragments as bases (targets, pairs, orphans, empty and all-N segments, mates on
                  different targets, near and far mates, repeats), for the end-to-end test.
  model_map()     bases in, per-segment final hits out on the CPU: sketch_model.sketch per segment with the shift of map.c:87-99 ->
                  oracle_lib.SeedIndex.collect_seeds -> oracle_fpv -> oracle_compact -> oracle_bottom -> oracle_gen_regs ->
                  frag_oracle.frag_read, with nothing but glue in between (and worker_for's reverse complement and flip for pe_ori).
numpy and the oracle libraries only; no GPU.  Imports tests/e2e_model.py's helpers and leaves that file alone."""
import types

import numpy as np

import e2e_model as em
import frag_oracle as fo
import index_image
import oracle_lib as ol
import post_oracle as po
import sketch_model as sm
from minimap2_chaindp_amd import params as P

SPAN = 21


# ---- anchor-level shapes -----------------------------------------------------------------------------------------------------------

def _place(rid, r0, pos, qlens, rev=False, span=SPAN):
    """Collinear anchors: pos = [(segment, position of the k-mer's last base in the segment)] -> uint64[n, 2].  The reference position
    grows with the position in the concatenated fragment (the reversed one for rev), so that consecutive anchors have dr == dq."""
    acc = np.concatenate(([0], np.cumsum(qlens)[:-1]))
    qsum = int(np.sum(qlens))
    Y = np.array([(qsum - (qlens[s] + acc[s]) if rev else acc[s]) + q for s, q in pos], np.int64)
    seg = np.array([s for s, _ in pos], np.uint64)
    order = np.argsort(Y, kind="stable")
    Y, seg = Y[order], seg[order]
    x = (np.uint64(1 << 63) if rev else np.uint64(0)) | np.uint64(rid) << np.uint64(32) | (np.uint64(r0) + (Y - Y[0]).astype(np.uint64))
    y = seg << np.uint64(48) | np.uint64(span) << np.uint64(32) | Y.astype(np.uint64)
    return np.stack([x, y], 1)


def _run(seg, q0, n, step=10):
    return [(seg, q0 + i * step) for i in range(n)]


def _frag(chains, qlens, rep_len=0):
    a = np.concatenate(chains) if chains else np.zeros((0, 2), np.uint64)
    a = a[np.lexsort((a[:, 1], a[:, 0]))]
    qsum = int(np.sum(qlens))
    qpos = []                                                    # minimizer positions, as tests/post_shapes.py makes them
    for x, y in a:
        span, p = int(y >> np.uint64(32) & np.uint64(0xff)), int(y & np.uint64(0xffffffff))
        qpos.append(qsum - 1 - (p + 1 - span) if int(x) >> 63 else p)
    qpos = sorted(set(q for q in qpos if 0 <= q < qsum) | set(range(7, qsum, 97)))
    return a, list(qlens), np.array([SPAN << 32 | q for q in qpos], np.uint64), rep_len


Q2 = (150, 150)


def branches_frag(rev=False):
    """A primary over both segments (271) and children for pe.c:15-31: min_diff keep, close on the reference kept / dropped by the 0.2
    ratio, over both segments elsewhere kept / dropped by pri_ratio, in one segment elsewhere dropped by the 0.7 ratio."""
    c = lambda rid, r0, pos: _place(rid, r0, pos, Q2, rev)
    return _frag([c(0, 10000, _run(0, 20, 13) + _run(1, 20, 13)), c(1, 10000, _run(0, 20, 12) + _run(1, 20, 11)),
                  c(0, 10400, _run(0, 20, 9)), c(0, 9700, [(0, 30), (0, 45)]),
                  c(2, 5000, _run(0, 70, 8) + _run(1, 20, 8)), c(3, 5000, _run(0, 110, 4) + _run(1, 20, 4)),
                  c(4, 5000, _run(0, 20, 13))], Q2)


def pri2_keep_frag():
    """parent over both segments (182), child in segment 0 elsewhere (131): kept by the 0.7 ratio"""
    return _frag([_place(0, 20000, _run(0, 30, 12) + _run(1, 20, 4), Q2), _place(4, 7000, _run(0, 25, 12), Q2)], Q2)


def equal_flags_frag():
    """parent and children in segment 0 only: pri_ratio keeps one (91 of 141) and drops one (61); segment 1 has no hits"""
    return _frag([_place(0, 30000, _run(0, 20, 13), Q2), _place(1, 8000, _run(0, 30, 8), Q2), _place(2, 8000, _run(0, 30, 5), Q2)], Q2)


def chi_both_frag():
    """parent in segment 0 (146), child over both segments elsewhere with 84: between 0.5 and 0.7 of the parent -- kept because
    is_chi_both sends it to pri_ratio"""
    return _frag([_place(0, 40000, _run(0, 20, 26, 5), Q2), _place(1, 9000, [(0, 60), (0, 100), (0, 140), (1, 25)], Q2)], Q2)


def pri1_frag():
    """parent 255, child 51 close on the reference: 255 * 0.2f is 51 in float (kept) and just above 51 in double (dropped)"""
    par = [(0, 20), (0, 24)] + _run(0, 34, 12) + [(1, 20)] + _run(1, 30, 8) + [(1, 109)]
    return _frag([_place(0, 50000, par, Q2), _place(0, 50500, [(0, 40), (0, 61), (0, 70)], Q2)], Q2)


def quirk_frag():
    """A 241 (segment 0), D 111 (its secondary, dropped), B 101 (segment 1, moves to slot 1), E 51 (B's secondary, kept: lands in B's old
    slot 2), F 31 (parent 2): compared with E (kept by min_diff) where B was meant (dropped)"""
    ql = (250, 250)
    return _frag([_place(0, 60000, _run(0, 20, 23), ql), _place(1, 3000, _run(0, 40, 10), ql), _place(2, 3000, _run(1, 20, 9), ql),
                  _place(3, 3000, _run(1, 30, 4), ql), _place(4, 3000, _run(1, 40, 2), ql)], ql)


def three_seg_frag(rev=False):
    ql = (100, 120, 90)
    c = lambda rid, r0, pos: _place(rid, r0, pos, ql, rev)
    return _frag([c(0, 70000, _run(0, 20, 8) + _run(1, 20, 10) + _run(2, 20, 7)), c(1, 2000, _run(1, 30, 8) + _run(2, 20, 5)),
                  c(2, 2000, _run(0, 25, 6)), c(0, 70600, _run(2, 25, 4)), c(3, 2000, _run(1, 20, 4))], ql)


def orphan_read(rng):
    """one segment: what chaindp_chain_post handles, inside a paired batch"""
    ql = (150,)
    return _frag([_place(0, 80000, _run(0, 20, 13), ql), _place(1, 1000, _run(0, 30, 9), ql, rev=True), _place(2, 1000, _run(0, 40, 4), ql)], ql,
                 int(rng.integers(0, 40)))


def big_frag(rng, n_hits=200):
    """more hits than the fragment kernels keep in LDS: two-anchor chains all over, a few over both segments"""
    chains = []
    for h in range(n_hits):
        seg = int(rng.integers(0, 2))
        q0 = int(rng.integers(20, 120))
        step = int(rng.integers(4, 25))
        pos = [(seg, q0), (seg, q0 + step)] if h % 9 else [(0, 140), (1, 25), (1, 40)]
        chains.append(_place(int(rng.integers(0, 5000)), int(rng.integers(1, 1 << 18)) * 64, pos, Q2, rev=bool(rng.random() < 0.3)))
    return _frag(chains, Q2, int(rng.integers(0, 60)))


def repeat_frag(rng, n_hits):
    """seeded overlapping hits: equal-score duplicates, near and far mates, either strand"""
    chains = []
    for h in range(n_hits):
        kind = rng.random()
        n0, n1 = int(rng.integers(2, 13)), int(rng.integers(2, 13))
        q0, q1 = int(rng.integers(20, 150 - 10 * n0 + 10)) if n0 <= 12 else 20, int(rng.integers(20, 150 - 10 * n1 + 10))
        if kind < 0.4:
            pos = _run(0, q0, n0) + _run(1, q1, n1)
        elif kind < 0.7:
            pos = _run(0, q0, n0)
        else:
            pos = _run(1, q1, n1)
        rid = int(rng.integers(0, 6))
        r0 = int(rng.choice([10000, 10300, 10700, 12000, 30000])) + int(rng.integers(0, 3)) * 1000 * (h % 3)
        chains.append(_place(rid, r0 + 7 * h, pos, Q2, rev=bool(rng.random() < 0.3)))
    return _frag(chains, Q2, int(rng.integers(0, 80)))


def _pack(reads):
    a = [r[0] for r in reads]
    off = np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.int64)
    mpo = np.concatenate([[0], np.cumsum([len(r[2]) for r in reads])]).astype(np.int64)
    return dict(off=off, anchors=np.concatenate(a).astype(np.uint64), n_segs=np.array([len(r[1]) for r in reads], np.int32),
                seg_len=np.array([q for r in reads for q in r[1]], np.int32), qlen=np.array([sum(r[1]) for r in reads], np.int32),
                mini_pos_off=mpo, mini_pos=np.concatenate([r[2] for r in reads]).astype(np.uint64), rep_len=np.array([r[3] for r in reads], np.int32))


def shapes(seed=7, n_random=14):
    """The paired set: the trap fragments, seeded repeat fragments, an orphan, one fragment above the LDS cap."""
    rng = np.random.default_rng(seed)
    reads = [branches_frag(), branches_frag(rev=True), pri2_keep_frag(), equal_flags_frag(), chi_both_frag(), pri1_frag(), quirk_frag(),
             orphan_read(rng)]
    for _ in range(n_random):
        reads.append(repeat_frag(rng, int(rng.integers(3, 40))))
    reads.append(big_frag(rng))
    reads.append(orphan_read(rng))
    return _pack(reads)


def shapes3(seed=11):
    """A batch of three-segment reads (max_dist = 0 in mm_select_sub_multi), with an orphan."""
    rng = np.random.default_rng(seed)
    return _pack([three_seg_frag(), three_seg_frag(rev=True), orphan_read(rng), three_seg_frag()])


# ---- bases in, per-segment hits out ---------------------------------------------------------------------------------------------------

def batch(frags):
    """A list of fragments (each a list of byte strings) -> (seq uint8[...], seq_off int64[n_seqs + 1], n_segs int32[n_reads])."""
    seqs = [s for f in frags for s in f]
    seq, seq_off = em.batch(seqs)
    return seq, seq_off, np.array([len(f) for f in frags], np.int32)


def _wants_flip(n_segs, j, pe_ori):
    return pe_ori >= 0 and n_segs == 2 and ((j == 0 and pe_ori >> 1 & 1) or (j == 1 and pe_ori & 1))


def model_map(img_or_index, w, k, is_hpc, flag, max_occ, par, min_cnt, opt, frags, bid, hash_, ref_len, pe_ori=-1):
    """What chaindp_map_frag_seqs returns -- seg_regs_off, regs, rep_len, n_anchors (also as .result) -- and per read the
    frag_oracle.FragTrace of the post steps (traces), the chains (chains_off) and the anchors (a_off)."""
    own = not isinstance(img_or_index, ol.SeedIndex)
    ix = ol.SeedIndex(img_or_index) if own else img_or_index
    od = po.opt_dict(opt)
    ref_len = np.ascontiguousarray(ref_len, np.int32)
    regs_out, rep_len, traces, n_a, n_c = [], [], [], [], []
    try:
        for r, f in enumerate(frags):
            f = [em.revcomp(s) if _wants_flip(len(f), j, pe_ori) else s for j, s in enumerate(f)]     # map.c:608-613
            qlens = [len(s) for s in f]
            parts, shift = [], 0
            for j, s in enumerate(f):                                                                 # collect_minimizers, map.c:87-99
                x, y = sm.sketch(s, w, k, is_hpc)
                y = (np.asarray(y, np.uint64) & np.uint64(0xffffffff)) + np.uint64(shift << 1) | np.uint64(j) << np.uint64(32)
                parts.append(np.stack((np.asarray(x, np.uint64), y), 1).reshape(-1, 2))
                shift += len(s)
            mini = np.concatenate(parts) if parts else np.zeros((0, 2), np.uint64)
            a, rl, mp = ix.collect_seeds(flag, max_occ, int(bid[r]), sum(qlens), mini)
            pr = ol.CoParams(*[getattr(par, key) for key, _ in ol.CoParams._fields_])
            pr.n_segs = len(f)
            fv, pv, vv, _ = ol.oracle_fpv(pr, a)
            seeds = ol.oracle_compact(pr, a, fv.copy(), pv.copy(), vv.copy())
            u, b = ol.oracle_bottom(min_cnt, par.min_sc, seeds)
            b = b.reshape(-1, 2)
            regs_in = ol.oracle_gen_regs(int(hash_[r]), sum(qlens), u, b)
            tr = fo.FragTrace()
            segs = fo.frag_read(od, par.max_dist_x, int(hash_[r]), qlens, rl, ref_len, regs_in, b, mp, tr=tr)
            for j, (regs, _) in enumerate(segs):
                regs_out.append(fo.flip_back(regs, qlens[j]) if _wants_flip(len(f), j, pe_ori) else regs)   # map.c:620-631
            rep_len.append(rl); traces.append(tr); n_a.append(len(a)); n_c.append(len(u))
    finally:
        if own:
            ix.close()
    m = types.SimpleNamespace(rep_len=np.array(rep_len, np.int32), traces=traces, n_segs=np.array([len(f) for f in frags], np.int32),
                              seg_regs_off=em._offsets(regs_out), regs=em._cat(regs_out, np.zeros(0, ol.REG_DTYPE)),
                              a_off=np.concatenate(([0], np.cumsum(n_a))).astype(np.int64), chains_off=np.concatenate(([0], np.cumsum(n_c))).astype(np.int64))
    m.n_anchors = int(m.a_off[-1])
    m.result = (m.seg_regs_off, m.regs, m.rep_len, m.n_anchors)
    return m


def coverage(m):
    """What a batch exercises, counted on the model."""
    so, first = m.seg_regs_off, np.concatenate(([0], np.cumsum(m.n_segs)))
    both = sum(1 for r in range(len(m.n_segs)) if m.n_segs[r] == 2 and so[first[r] + 1] > so[first[r]] and so[first[r] + 2] > so[first[r] + 1])
    return dict(reads=len(m.n_segs), both_segments=int(both), multi_dropped=int(sum(t.multi_dropped for t in m.traces)),
                reverse=int((m.regs["bits"] >> 10 & 1).sum()), one_segment=int((m.n_segs == 1).sum()), final_hits=int(so[-1]),
                secondary=int((m.regs["parent"] != m.regs["id"]).sum()), empty_segments=int((np.diff(so) == 0).sum()),
                max_chains=int(np.diff(m.chains_off).max()) if len(m.n_segs) else 0, anchors=m.n_anchors)


SR_W, SR_K = 11, 21                                                  # options.c:117-118


def scenario(n_frags=3000, seed=1, read_len=150):
    """A seeded `sr` batch: pairs drawn from a few targets that carry dispersed and diverged repeats (secondaries), the second mate
    reverse-complemented as a sequencer reports it; mates closer than and farther than max_dist, mates on different targets, orphans
    (one segment), empty and all-N segments, unrelated mates.  One gap group: every segment has read_len bases (but the empty ones)."""
    rng = np.random.default_rng([seed, 77])
    unit = em.rand_seq(rng, 400)
    targets = []
    for _ in range(3):
        parts = [unit, em.mutate(rng, unit, .03), em.revcomp(unit), em.mutate(rng, unit, .05), unit]
        targets.append(em._target(rng, 30000, [parts[i] for i in rng.permutation(len(parts))]))
    kinds_p = (("near", .55), ("far", .08), ("split", .06), ("orphan", .10), ("empty_mate", .03), ("n_mate", .03), ("unrelated_mate", .05), ("repeat", .10))
    names, probs = [n for n, _ in kinds_p], np.array([p for _, p in kinds_p])
    kinds = [str(x) for x in rng.choice(names, size=n_frags, p=probs / probs.sum())]
    for i, kd in enumerate(names):
        kinds[(i * 7919) % n_frags] = kd
    frags = []
    for kd in kinds:
        g = targets[int(rng.integers(0, 3))]
        L = read_len
        if kd == "repeat":                                           # inside a copy of the repeat unit
            at = g.find(unit)
            s0 = at + int(rng.integers(0, 400 - L)) if at >= 0 else int(rng.integers(0, len(g) - 1000))
        else:
            s0 = int(rng.integers(0, len(g) - 3000))
        ins = int(rng.integers(L, 500)) if kd != "far" else int(rng.integers(1200, 2500))
        m1 = em.mutate(rng, g[s0:s0 + L], .02)[:L].ljust(L, b"A")
        m2src = g[s0 + ins - L:s0 + ins] if kd != "split" else em._piece(rng, targets[int(rng.integers(0, 3))], L)
        m2 = em.revcomp(em.mutate(rng, m2src, .02)[:L].ljust(L, b"A"))
        if rng.random() < 0.5:                                       # the fragment from the other strand: the mates change places
            m1, m2 = m2, m1
        if kd == "orphan":
            frags.append([m1])
        elif kd == "empty_mate":
            frags.append([m1, b""])
        elif kd == "n_mate":
            frags.append([b"N" * L, m2])
        elif kd == "unrelated_mate":
            frags.append([m1, em.rand_seq(rng, L)])
        else:
            frags.append([m1, m2])
    n = len(frags)
    sc = types.SimpleNamespace(frags=frags, kinds=kinds, targets=targets, w=SR_W, k=SR_K, hpc=0, par=P.preset("sr"), min_cnt=2, opt=P.post_preset("sr"),
                               hash_=rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), max_occ=1000, flag=P.MM_F_SR,
                               bid=rng.integers(0, 1 << 10, size=n, dtype=np.uint32), ref_len=np.array([len(t) for t in targets], np.int32))
    cache = []

    def image():
        if not cache:
            cache.append(index_image.build_image(index_image.index_entries(sc.targets, sc.w, sc.k, sc.hpc)))
        return cache[0]
    sc.image = image
    return sc


def model_of(sc, img=None, sel=None, pe_ori=-1, frags=None):
    sel = range(len(sc.frags)) if sel is None else sel
    frags = sc.frags if frags is None else frags
    return model_map(img if img is not None else sc.image(), sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt,
                     [frags[i] for i in sel], sc.bid[list(sel)], sc.hash_[list(sel)], sc.ref_len, pe_ori=pe_ori)
