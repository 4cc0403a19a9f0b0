"""CHECKER ONLY: the composed CPU model of tests/frag_model.py with the chaining gaps taken per read, and a seeded batch of trimmed pairs.

  model_map()     the loop of frag_model.model_map, read by read: read r is chained with max_dist_x / max_dist_y = its own
                  (gap_ref, gap_qry) and mm_select_sub_multi gets its gap_ref as max_gap_ref (map.c:243,358-366).
  scenario()      `sr` pairs after adapter / quality trimming: mates of 30..150 bases, most inserts between 420 and 820 -- across the
                  range of gap_ref = max(800 - qlen_sum, 100) -- the second mate reverse-complemented as a sequencer reports it, so
                  that under pe_ori = 1 both mates end on one strand; orphans and empty mates included.  sc.gaps = (gap_ref, gap_qry).
numpy and the oracle libraries only; no GPU.  Imports tests/frag_model.py's helpers and leaves that file alone."""
import types

import numpy as np

import e2e_model as em
import frag_model as fm
import index_image
import oracle_lib as ol
from minimap2_chaindp_amd import params as P

MAX_GAP, MAX_GAP_REF, MAX_FRAG_LEN = 100, -1, 800                    # options.c:115-131 (sr): max_gap, max_gap_ref unset, max_frag_len
PE_ORI = 1


def gaps_py(max_gap, max_gap_ref, max_frag_len, is_sr, qlen_sum):
    """map.c:358-366 restated, for int32 inputs whose differences stay in int32."""
    q = np.asarray(qlen_sum, np.int64)
    gq = np.where(q > max_gap, q, max_gap) if is_sr else np.full(len(q), max_gap)
    if max_gap_ref > 0:
        gr = np.full(len(q), max_gap_ref)
    elif max_frag_len > 0:
        gr = np.maximum(max_frag_len - q, max_gap)
    else:
        gr = np.full(len(q), max_gap)
    return gr.astype(np.int32), gq.astype(np.int32)


def model_map(img_or_index, w, k, is_hpc, flag, max_occ, par, min_cnt, opt, frags, bid, hash_, ref_len, gaps, pe_ori=-1):
    """frag_model.model_map with read r under gaps[0][r], gaps[1][r]: the same fields (.result = seg_regs_off, regs, rep_len, n_anchors;
    .per_read = every read's own (seg_regs_off, regs))."""
    own = not isinstance(img_or_index, ol.SeedIndex)
    ix = ol.SeedIndex(img_or_index) if own else img_or_index
    regs, counts, rep, per_read, n_a = [], [], [], [], 0
    try:
        for r, f in enumerate(frags):
            pr = P.ChainParams(*par.astuple())
            pr.max_dist_x, pr.max_dist_y = int(gaps[0][r]), int(gaps[1][r])
            m = fm.model_map(ix, w, k, is_hpc, flag, max_occ, pr, min_cnt, opt, [f], bid[r:r + 1], hash_[r:r + 1], ref_len, pe_ori=pe_ori)
            regs.append(m.regs); counts.extend(np.diff(m.seg_regs_off).tolist()); rep.append(int(m.rep_len[0])); n_a += m.n_anchors
            per_read.append((m.seg_regs_off, m.regs))
    finally:
        if own:
            ix.close()
    out = types.SimpleNamespace(seg_regs_off=np.concatenate(([0], np.cumsum(counts))).astype(np.int64),
                                regs=np.concatenate(regs + [np.zeros(0, ol.REG_DTYPE)]).astype(ol.REG_DTYPE), rep_len=np.array(rep, np.int32),
                                n_anchors=int(n_a), n_segs=np.array([len(f) for f in frags], np.int32), per_read=per_read)
    out.result = (out.seg_regs_off, out.regs, out.rep_len, out.n_anchors)
    return out


def scenario(n_frags=320, seed=5):
    """See the module's text.  Returns frag_model.scenario's namespace plus gaps, qlen_sum and pe_ori."""
    rng = np.random.default_rng([seed, 358])
    unit = em.rand_seq(rng, 400)
    targets = []
    for _ in range(3):
        parts = [unit, em.mutate(rng, unit, .03), em.revcomp(unit), em.mutate(rng, unit, .05), unit]
        targets.append(em._target(rng, 30000, [parts[i] for i in rng.permutation(len(parts))]))
    kinds_p = (("pair", .80), ("short_insert", .06), ("orphan", .07), ("empty_mate", .04), ("repeat", .03))
    names, probs = [n for n, _ in kinds_p], np.array([p for _, p in kinds_p])
    kinds = [str(x) for x in rng.choice(names, size=n_frags, p=probs / probs.sum())]
    for i, kd in enumerate(names):
        kinds[(i * 7919) % n_frags] = kd
    frags = []
    for kd in kinds:
        g = targets[int(rng.integers(0, 3))]
        L1, L2 = int(rng.integers(30, 151)), int(rng.integers(30, 151))         # what trimming left of 2 x 150
        if kd == "repeat":
            at = g.find(unit)
            s0 = at + int(rng.integers(0, 400 - L1)) if at >= 0 else int(rng.integers(0, len(g) - 2000))
        else:
            s0 = int(rng.integers(0, len(g) - 2000))
        ins = int(rng.integers(max(L1, L2), 400)) if kd == "short_insert" else int(rng.integers(420, 821))
        m1 = em.mutate(rng, g[s0:s0 + L1], .02)[:L1].ljust(L1, b"A")
        m2 = em.revcomp(em.mutate(rng, g[s0 + ins - L2:s0 + ins], .02)[:L2].ljust(L2, b"A"))
        if rng.random() < 0.5:                                       # the fragment from the other strand: the mates change places
            m1, m2 = m2, m1
        frags.append([m1] if kd == "orphan" else [m1, b""] if kd == "empty_mate" else [m1, m2])
    n = len(frags)
    sc = types.SimpleNamespace(frags=frags, kinds=kinds, targets=targets, w=fm.SR_W, k=fm.SR_K, hpc=0, par=P.preset("sr"), min_cnt=2, opt=P.post_preset("sr"),
                               hash_=rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), max_occ=1000, flag=P.MM_F_SR,
                               bid=rng.integers(0, 1 << 10, size=n, dtype=np.uint32), ref_len=np.array([len(t) for t in targets], np.int32),
                               pe_ori=PE_ORI)
    sc.qlen_sum = np.array([sum(len(s) for s in f) for f in frags], np.int32)
    sc.gaps = gaps_py(MAX_GAP, MAX_GAP_REF, MAX_FRAG_LEN, 1, sc.qlen_sum)
    cache = []

    def image():
        if not cache:
            cache.append(index_image.build_image(index_image.index_entries(sc.targets, sc.w, sc.k, sc.hpc)))
        return cache[0]
    sc.image = image
    return sc


def groups(sc):
    """The reads of every distinct (gap_ref, gap_qry) pair, in the batch's order: [((gap_ref, gap_qry), [read, ...]), ...]."""
    by = {}
    for r, key in enumerate(zip(sc.gaps[0].tolist(), sc.gaps[1].tolist())):
        by.setdefault(key, []).append(r)
    return list(by.items())


def model_of(sc, gaps=None, img=None):
    return model_map(img if img is not None else sc.image(), sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, sc.frags, sc.bid,
                     sc.hash_, sc.ref_len, sc.gaps if gaps is None else gaps, pe_ori=sc.pe_ori)


def uniform(sc, gap_ref, gap_qry):
    n = len(sc.frags)
    return np.full(n, gap_ref, np.int32), np.full(n, gap_qry, np.int32)


def reads_that_differ(a, b):
    """Reads whose final hits (offsets or bytes) differ between two model runs."""
    return [r for r, (x, y) in enumerate(zip(a.per_read, b.per_read)) if not (np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes())]


_cache = {}


def scenario_with_model():
    """(scenario, its model under its own gaps), computed once per process and shared."""
    if "m" not in _cache:
        sc = scenario()
        _cache["m"] = (sc, model_of(sc))
    return _cache["m"]
