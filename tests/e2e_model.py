"""CHECKER ONLY: bases in, final hits out on the CPU, by composing the restatements that the CPU tier pins to the reference --
sketch_model.sketch -> an index image (index_image.build_image) opened by oracle_lib.SeedIndex -> collect_seeds -> oracle_fpv ->
oracle_compact -> oracle_bottom -> oracle_gen_regs -> post_oracle.post_read -- with nothing but glue in between, and a seeded
generator of the batches the end-to-end tests map (scenario()).  numpy and the oracle libraries only; no GPU."""
import functools
import types

import numpy as np

import index_image
import oracle_lib as ol
import post_oracle as po
import sketch_model as sm
from minimap2_chaindp_amd import params as P


def batch(seqs):
    """A list of byte strings -> (seq uint8[...], seq_off int64[n + 1]) as chaindp_sketch / chaindp_map_seqs take them."""
    return np.frombuffer(b"".join(seqs), np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)


def _cat(parts, empty):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else empty


def _offsets(parts):
    return np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)


def model_map(img_or_index, w, k, is_hpc, flag, max_occ, par, min_cnt, opt, seqs, bid, hash_, ref_len):
    """What chaindp_map_seqs returns -- regs_off, regs, rep_len, n_anchors (also as .result) -- and every stage's output on the way:
    mini_off / mini, a_off / anchors, mp_off / mini_pos, f / p / v, seeds_off / seeds (new_seed[]), chains_off / u and b_off / b,
    regs_in (mm_gen_regs' hits, at chains_off), and per read the post_oracle._Trace of the post steps (traces)."""
    own = not isinstance(img_or_index, ol.SeedIndex)
    ix = ol.SeedIndex(img_or_index) if own else img_or_index
    od = po.opt_dict(opt)
    ref_len = np.ascontiguousarray(ref_len, np.int32)
    S = {key: [] for key in ("mini", "anchors", "mini_pos", "f", "p", "v", "seeds", "u", "b", "regs_in", "regs")}
    rep_len, traces = [], []
    try:
        for r, s in enumerate(seqs):
            qlen = len(s)
            x, y = sm.sketch(s, w, k, is_hpc)
            mini = np.stack((x, y), 1).astype(np.uint64).reshape(-1, 2)
            a, rl, mp = ix.collect_seeds(flag, max_occ, int(bid[r]), qlen, mini)
            f, p, v, _ = ol.oracle_fpv(par, a)
            seeds = ol.oracle_compact(par, a, f.copy(), p.copy(), v.copy())
            u, b = ol.oracle_bottom(min_cnt, par.min_sc, seeds)
            b = b.reshape(-1, 2)
            regs_in = ol.oracle_gen_regs(int(hash_[r]), qlen, u, b)
            tr = po._Trace()
            regs, _ = po.post_read(od, qlen, rl, ref_len, regs_in, b, mp, tr=tr)
            for key, val in (("mini", mini), ("anchors", a), ("mini_pos", mp), ("f", f), ("p", p), ("v", v), ("seeds", seeds), ("u", u), ("b", b),
                             ("regs_in", regs_in), ("regs", regs)):
                S[key].append(val)
            rep_len.append(rl); traces.append(tr)
    finally:
        if own:
            ix.close()
    e2, ei, er = np.zeros((0, 2), np.uint64), np.zeros(0, np.int32), np.zeros(0, ol.REG_DTYPE)
    m = types.SimpleNamespace(
        qlen=np.array([len(s) for s in seqs], np.int32), rep_len=np.array(rep_len, np.int32), traces=traces,
        mini_off=_offsets(S["mini"]), mini=_cat(S["mini"], e2), a_off=_offsets(S["anchors"]), anchors=_cat(S["anchors"], e2),
        mp_off=_offsets(S["mini_pos"]), mini_pos=_cat(S["mini_pos"], np.zeros(0, np.uint64)),
        f=_cat(S["f"], ei), p=_cat(S["p"], ei), v=_cat(S["v"], ei),
        seeds_off=_offsets(S["seeds"]), seeds=_cat(S["seeds"], np.zeros(0, ol.SEED_DTYPE)),
        chains_off=_offsets(S["u"]), u=_cat(S["u"], np.zeros(0, np.uint64)), b_off=_offsets(S["b"]), b=_cat(S["b"], e2),
        regs_in=_cat(S["regs_in"], er), regs_off=_offsets(S["regs"]), regs=_cat(S["regs"], er))
    m.n_anchors = int(m.a_off[-1])
    m.result = (m.regs_off, m.regs, m.rep_len, m.n_anchors)
    return m


def unit_lengths(m, max_dist_x):
    """Anchors per DP unit ("Wave formulation": a read's anchors split where x grows by more than max_dist_x)."""
    if not len(m.anchors):
        return np.zeros(0, np.int64)
    x = m.anchors[:, 0]
    cut = np.zeros(len(x), bool)
    cut[0] = True
    cut[1:] = (x[1:] - x[:-1]) > np.uint64(max_dist_x)
    cut[m.a_off[:-1][m.a_off[:-1] < len(x)]] = True
    return np.diff(np.concatenate((np.nonzero(cut)[0], [len(x)])))


def coverage(m, par):
    """What a batch exercises, counted from the model's intermediates (the CPU tier asserts each > 0 where the issue asks for it)."""
    n_mini, n_a, n_c, n_out = np.diff(m.mini_off), np.diff(m.a_off), np.diff(m.chains_off), np.diff(m.regs_off)
    R = len(n_mini)
    sec = drop = spans = 0
    for r in range(R):
        x = m.regs[m.regs_off[r]:m.regs_off[r + 1]]
        sec += bool((x["parent"] != x["id"]).any())
        drop += m.traces[r].select_sub_dropped
        a = m.anchors[m.a_off[r]:m.a_off[r + 1]]
        spans += len(a) > 0 and len(np.unique(a[:, 1] >> np.uint64(32) & np.uint64(0xff))) > 1
    mapq = m.regs["bits"] & 0xff
    units = unit_lengths(m, par.max_dist_x)
    ties = 0
    for r in range(R):
        x = m.anchors[m.a_off[r]:m.a_off[r + 1], 0]
        ties += int((x[1:] == x[:-1]).sum())
    return dict(reads=R, bases=int(m.qlen.sum()), minimizers=int(m.mini_off[-1]), anchors=m.n_anchors, chains=int(m.chains_off[-1]),
                final_hits=int(m.regs_off[-1]),
                no_minimizers=int((n_mini == 0).sum()), no_anchors=int(((n_mini > 0) & (n_a == 0)).sum()),
                no_chains=int(((n_a > 0) & (n_c == 0)).sum()), multi_hit=int((n_out > 1).sum()), secondary=int(sec), dropped=int(drop),
                joined=int(sum(t.joined > 0 for t in m.traces)), mapq0=int((mapq == 0).sum()), mapq60=int((mapq == 60).sum()),
                rep_len=int((m.rep_len > 0).sum()), reverse=int((m.regs["bits"] >> 10 & 1).sum()), x_ties=ties,
                max_chains=int(n_c.max()) if R else 0, max_unit=int(units.max()) if len(units) else 0, max_anchors=int(n_a.max()) if R else 0,
                mixed_q_span=int(spans))


# ---- the seeded batches ------------------------------------------------------------------------------------------------------------

MODES = {                       # w, k, hpc, chain parameters, post options, collect_seeds flag
    "map-ont": (10, 15, 0, "map-ont", "map-ont", 0),
    "map-pb": (10, 19, 1, "map-ont", "map-pb", 0),          # map-pb chains with the default parameters, which are map-ont's
    "ava-ont": (5, 15, 0, "ava-ont", "ava-ont", None),
    "ava-pb": (5, 19, 1, "ava-pb", "ava-pb", None),
}
AVA_BID = 0x80000000            # an all-vs-all read is also target `rank`: bit 31 set, as the syn_repeats_ava* seed fixtures have it
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return _ACGT[rng.integers(0, 4, int(n))].tobytes()


def mutate(rng, s, rate):
    """Substitutions, deletions and insertions, a third of `rate` each."""
    a = np.frombuffer(s, np.uint8).copy()
    if not len(a):
        return s
    r = rng.random(len(a))
    sub = (r >= rate / 3) & (r < 2 * rate / 3)
    ins = (r >= 2 * rate / 3) & (r < rate)
    a[sub] = _ACGT[rng.integers(0, 4, int(sub.sum()))]
    reps = np.ones(len(a), np.int64)
    reps[r < rate / 3] = 0
    reps[ins] = 2
    out = np.repeat(a, reps)
    at = (np.cumsum(reps) - 1)[ins]
    out[at] = _ACGT[rng.integers(0, 4, len(at))]
    return out.tobytes()


def _target(rng, length, parts):
    """Random sequence of about `length` bases with `parts` spliced in at random places, in their order."""
    gaps = rng.dirichlet(np.ones(len(parts) + 1)) * max(length - sum(len(p) for p in parts), 1000 * (len(parts) + 1))
    out = []
    for g, p in zip(gaps, parts + [b""]):
        out += [rand_seq(rng, max(int(g), 200)), p]
    return b"".join(out)


def _genome(rng, n_targets, length, family_unit=None):
    """Targets with dispersed, inverted and tandem repeats and diverged long repeats; with family_unit, eight more that carry 400
    diverged copies of it."""
    unit, long_unit, t_short, t_long = rand_seq(rng, 1200), rand_seq(rng, 3000), rand_seq(rng, 37), rand_seq(rng, 180)
    targets = []
    for _ in range(n_targets):
        parts = [unit, t_short * int(rng.integers(12, 40)), mutate(rng, long_unit, rng.uniform(.02, .08)), revcomp(unit),
                 t_long * int(rng.integers(20, 45)), unit, mutate(rng, revcomp(long_unit), rng.uniform(.02, .08)), mutate(rng, unit, .04)]
        parts = [parts[i] for i in rng.permutation(len(parts))]
        targets.append(_target(rng, length, parts))
    if family_unit is not None:
        for _ in range(8):
            targets.append(b"".join(rand_seq(rng, rng.integers(900, 1500)) + mutate(rng, family_unit, .06) for _ in range(50)))
    return targets, t_long, unit


def _piece(rng, g, n):
    n = min(int(n), len(g))
    s = int(rng.integers(0, len(g) - n + 1))
    return g[s:s + n]


def _read(rng, kind, genome, t_long, k, max_len):
    g = genome[int(rng.integers(0, len(genome)))]
    n = int(np.exp(rng.uniform(np.log(30), np.log(max_len))))
    rate = rng.uniform(.02, .15)
    if kind == "empty":
        return b""
    if kind == "short":
        return _piece(rng, g, rng.integers(1, k))
    if kind == "only_n":
        return b"N" * int(rng.integers(1, 400))
    if kind == "unrelated":
        return rand_seq(rng, n)
    if kind == "tandem":                                                     # wholly inside a tandem repeat
        rep = t_long * 20
        return mutate(rng, _piece(rng, rep, min(n, len(rep) - 180)), rate)
    if kind == "chimeric":                                                   # two places, joined
        s = mutate(rng, _piece(rng, g, n // 2 + 20), rate) + mutate(rng, _piece(rng, genome[int(rng.integers(0, len(genome)))], n // 2 + 20), rate)
    elif kind == "inverted":                                                 # the middle third turned round
        s = _piece(rng, g, max(n, 90))
        s = mutate(rng, s[:len(s) // 3] + revcomp(s[len(s) // 3:2 * len(s) // 3]) + s[2 * len(s) // 3:], rate)
    elif kind == "deletion":                                                 # 0.6-1.9 kb of the target missing between two long flanks: what mm_join_long joins
        n1, n2, d = int(rng.integers(2500, 6000)), int(rng.integers(2500, 6000)), int(rng.integers(600, 1900))
        s = _piece(rng, g, n1 + d + n2)
        s = mutate(rng, s[:n1] + s[n1 + d:], rng.uniform(.02, .06)) if len(s) == n1 + d + n2 else mutate(rng, s, rate)
    else:
        s = mutate(rng, _piece(rng, g, n), rate)
        if kind == "n_runs":                                                 # runs of N and lower case
            a = bytearray(s)
            for _ in range(int(rng.integers(1, 6))):
                at, ln = int(rng.integers(0, len(a) + 1)), int(rng.integers(1, 40))
                a[at:at] = b"N" * ln
            lo, hi = sorted(int(x) for x in rng.integers(0, len(a) + 1, 2))
            s = bytes(a[:lo]) + bytes(a[lo:hi]).lower() + bytes(a[hi:])
    return revcomp(s) if rng.random() < 1 / 3 else s


KINDS = (("plain", .60), ("unrelated", .05), ("chimeric", .05), ("inverted", .04), ("deletion", .04), ("n_runs", .06), ("empty", .02),
         ("short", .04), ("only_n", .02), ("tandem", .08))


def scenario(mode, n_reads=2000, seed=1, family=False, max_len=30000, genome_len=None):
    """A seeded batch of one of MODES.  Returns a namespace: targets, reads, kinds, bid, hash_, ref_len, flag, max_occ, w, k, hpc,
    par, min_cnt, opt and image() (the index image of the targets, built on first use).  The map modes index a few targets; the ava
    modes index the reads themselves.  family: eight more targets with 400 diverged copies of a 300-base unit, a read that holds
    the unit twice, and a max_occ that lets the family through."""
    w, k, hpc, chain, post, flag = MODES[mode]
    ava = mode.startswith("ava")
    rng = np.random.default_rng([seed, sorted(MODES).index(mode), int(family)])
    unit = rand_seq(rng, 300) if family else None
    if ava:                                                                  # the reads cover their genome about four times over
        genome, t_long, unit_d = _genome(rng, 3, genome_len or max(n_reads * 360, 60000), None)
    else:
        genome, t_long, unit_d = _genome(rng, 3, genome_len or 90000, unit)
    names, probs = [n for n, _ in KINDS], np.array([p for _, p in KINDS])
    kinds = [str(x) for x in rng.choice(names, size=n_reads, p=probs / probs.sum())]
    for i, kd in enumerate(names):                                           # one of every kind, whatever n_reads is
        if i < n_reads:
            kinds[(i * 7919) % n_reads] = kd
    reads = [_read(rng, kd, genome[:3], t_long, k, max_len) for kd in kinds]
    if n_reads >= 40:                                                        # the ends of the length range are always there
        at = [i for i, kd in enumerate(kinds) if kd == "plain"][:2]
        g0 = genome[0]                                                       # (the long one crosses a dispersed repeat: more anchors than minimizers)
        lo = max(0, min(g0.find(unit_d) - 1000, len(g0) - max_len))
        reads[at[0]] = mutate(rng, g0[lo:lo + max_len], .03)[:max_len]
        reads[at[1]] = _piece(rng, genome[1], 30)
    if family:
        reads[n_reads // 2] = unit + rand_seq(rng, 40) + unit
        kinds[n_reads // 2] = "family"
    sc = types.SimpleNamespace(mode=mode, reads=reads, kinds=kinds, w=w, k=k, hpc=hpc, par=P.preset(chain), min_cnt=3, opt=P.post_preset(post),
                               hash_=rng.integers(0, 1 << 32, size=n_reads, dtype=np.uint64).astype(np.uint32),
                               max_occ=2000 if family else 12)
    if ava:
        sc.targets, sc.flag = reads, P.MM_F_NO_DIAG | P.MM_F_NO_DUAL | P.MM_F_NO_LJOIN | P.MM_F_ALL_CHAINS
        sc.bid = (np.arange(n_reads, dtype=np.uint32) | np.uint32(AVA_BID)).astype(np.uint32)
    else:
        sc.targets, sc.flag = genome, flag
        sc.bid = rng.integers(0, 1 << 10, size=n_reads, dtype=np.uint32)     # (not read without NO_DIAG / NO_DUAL)
    sc.ref_len = np.array([len(t) for t in sc.targets], np.int32)
    cache = []

    def image():
        if not cache:
            cache.append(index_image.build_image(index_image.index_entries(sc.targets, w, k, hpc)))
        return cache[0]
    sc.image = image
    return sc


def model_of(sc, img=None, sel=None):
    """model_map on a scenario (sel: the places of the reads to map, in that order; the index stays the whole scenario's)."""
    sel = range(len(sc.reads)) if sel is None else sel
    return model_map(img if img is not None else sc.image(), sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt,
                     [sc.reads[i] for i in sel], sc.bid[list(sel)], sc.hash_[list(sel)], sc.ref_len)


# the batches of tests/test_e2e_model.py (what they exercise) and tests/test_gpu_e2e.py (mapped on the device)
SCENARIOS = {
    "map-ont": dict(mode="map-ont", n_reads=2000, seed=1),
    "map-pb": dict(mode="map-pb", n_reads=2000, seed=1),
    "ava-ont": dict(mode="ava-ont", n_reads=2000, seed=1),
    "ava-pb": dict(mode="ava-pb", n_reads=2000, seed=1),
    "family": dict(mode="map-ont", n_reads=300, seed=1, family=True),
    "large": dict(mode="map-ont", n_reads=8000, seed=2),                     # GPU tier only: >= 5,000 reads and >= 2 M anchors
}


@functools.lru_cache(maxsize=None)
def named(name):
    """(scenario, its model) of one of SCENARIOS, made once per process."""
    sc = scenario(**SCENARIOS[name])
    return sc, model_of(sc)
