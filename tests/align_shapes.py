"""Inputs of the mm_align1 tests: named cases, each at the smallest size that reaches its branch, and a seeded fuzz batch.

A scene is dict(name, opt, targets [str], reads [dict(name, seq str, a uint64[n, 2], regs REG_DTYPE[m])]) -- one call of chaindp_align1.
Targets are 1-4 kb; reads are 150-1500 bases, mutated copies of a target stretch (substitutions, indels, N runs, an inverted stretch, a
large deletion); anchors are exact k-mer matches on the true path, x / y packed as the reference packs them (x = strand << 63 |
rid << 32 | last target base, y = flags | span << 32 | last base on the mapped strand of the read).  min_ksw_len and bw are small, so
that a short read still has many fills and the band still binds."""
import numpy as np

import align_model as A

REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")]
                     + [("bits", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("reserved", "<u4", (2,))])
EXTRA_DTYPE = np.dtype([(k, "<i4") for k in A.EXTRA_FIELDS])

# map-ont scoring with the small band and fill length of this tier; hpc: map-pb's k = 19 on homopolymer-compressed minimizers
OPT = dict(a=2, b=4, q=4, e=2, q2=24, e2=1, bw=40, zdrop=400, zdrop_inv=200, end_bonus=-1, min_cnt=3, min_chain_score=40, min_dp_max=80,
           min_ksw_len=40, max_gap=5000, flag=0, k=15, is_hpc=0)
OPTS = {"ont": OPT, "hpc": dict(OPT, k=19, is_hpc=1), "bonus": dict(OPT, end_bonus=100), "asm": dict(OPT, a=1, b=9, q=16, e=2, q2=41, e2=1, zdrop=200, zdrop_inv=200, min_dp_max=200),
        "lowz": dict(OPT, zdrop=120, zdrop_inv=60), "cnt2": dict(OPT, zdrop=120, zdrop_inv=60, min_cnt=2), "gap600": dict(OPT, max_gap=600)}
ACGT = "ACGT"


def rand_seq(rng, n):
    return "".join(ACGT[i] for i in rng.integers(0, 4, n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def mutate(rng, tseq, t0, t1, sub=0.03, indel=0.02, edits=()):
    """A read of target[t0:t1] on the forward strand: random substitutions and 1-3 base indels, and the given edits
    (tpos, kind, len): "ins" random bases before tpos, "del" of target bases, "n" an N run in the read, "tn" nothing (the target has
    the Ns), "inv" the stretch reverse-complemented, "junk" the stretch replaced by random bases.  Returns (read, path) with
    path[i] = the target position read base i copies exactly, or -1."""
    ed = {e[0]: e for e in edits}
    out, path = [], []
    t = t0
    while t < t1:
        if t in ed:
            _, kind, ln = ed.pop(t)
            if kind == "ins":
                out.append(rand_seq(rng, ln)); path += [-1] * ln
            elif kind == "del":
                t += ln
                continue
            elif kind in ("n", "junk", "inv"):
                s = "N" * ln if kind == "n" else rand_seq(rng, ln) if kind == "junk" else rc(tseq[t:t + ln])
                out.append(s); path += [-1] * ln
                t += ln
                continue
        u = rng.random()
        if u < sub:
            out.append(ACGT[(ACGT.index(tseq[t]) + int(rng.integers(1, 4))) % 4] if tseq[t] in ACGT else "A"); path.append(-1)
        elif u < sub + indel / 2:
            ln = int(rng.integers(1, 4))
            out.append(rand_seq(rng, ln)); path += [-1] * ln
            continue
        elif u < sub + indel:
            t += int(rng.integers(1, 4))
            continue
        else:
            out.append(tseq[t]); path.append(t if tseq[t] in ACGT else -1)
        t += 1
    return "".join(out), path


def anchors_of(path, k, rid, rev, step, rng=None):
    """Exact k-mer matches on the true path, every `step` bases or so: the k bases ending at read position i copy k consecutive target bases."""
    a, run, last = [], 0, -10 ** 9
    for i, t in enumerate(path):
        run = 0 if t < 0 else run + 1 if i > 0 and path[i - 1] == t - 1 else 1
        if run >= k and i - last >= step:
            a.append((rev << 63 | rid << 32 | t, k << 32 | i))
            last = i + (int(rng.integers(0, step // 2 + 1)) if rng is not None else 0)
    return np.array(a, np.uint64).reshape(-1, 2)


def region(a, qlen, as_, cnt, rid=None, bits=0, id_=0, parent=0):
    r = dict(zip(A.REG_FIELDS, (0,) * len(A.REG_FIELDS)))
    r.update({"id": id_, "parent": parent, "as": as_, "cnt": cnt, "bits": bits})
    if cnt:
        ax, ay = [int(v) for v in a[:, 0]], [int(v) for v in a[:, 1]]
        A.set_coor(r, qlen, ax, ay)
        r["bits"] |= bits
        r["score"] = r["score0"] = int(r["mlen"])
    return r


def regs_array(rs):
    out = np.zeros(len(rs), REG_DTYPE)
    for i, r in enumerate(rs):
        for k in A.REG_FIELDS:
            if k != "div":
                out[k][i] = r[k] if k not in ("bits", "hash") else r[k] & 0xffffffff
    return out


def reg_dict(row):
    return {k: (float(row[k]) if k == "div" else int(row[k])) for k in A.REG_FIELDS}


def read_of(rng, name, targets, rid, t0, t1, rev=0, k=15, step=30, jitter=True, whole=True, **mut):
    seq, path = mutate(rng, targets[rid], t0, t1, **mut)
    a = anchors_of(path, k, rid, rev, step, rng if jitter else None)
    rd = dict(name=name, seq=rc(seq) if rev else seq, a=a, regs=[])
    if whole:
        rd["regs"] = [region(a, len(seq), 0, len(a))]
    return rd


def _finish(scene):
    for rd in scene["reads"]:
        rd["regs"] = regs_array(rd["regs"])
    return scene


def named_scenes():
    rng = np.random.default_rng(20240611)
    T = [rand_seq(rng, 3000), rand_seq(rng, 1500)]
    T[1] = T[1][:700] + "NNNNNN" + T[1][706:]                    # N in a target
    unit = "ACGT"
    T.append(rand_seq(rng, 300) + unit * 3 + rand_seq(rng, 900))   # a duplicated unit: a deletion that shifts by the whole M before it
    T.append("".join(c * int(n) for c, n in zip(rand_seq(rng, 700), rng.integers(1, 5, 700))))      # homopolymer runs, for HPC
    scenes = []

    def scene(name, opt, reads):
        scenes.append(_finish(dict(name=name, opt=dict(OPTS[opt]), targets=T, reads=reads)))

    # plain reads, both strands, N in query and target, two lengths and a cnt == 0 region in one batch
    plain = read_of(rng, "fwd", T, 0, 200, 900)
    rev = read_of(rng, "rev", T, 0, 1000, 1600, rev=1)
    short = read_of(rng, "n_query", T, 0, 1700, 1950, edits=[(1800, "n", 12)])
    tn = read_of(rng, "n_target", T, 1, 500, 1000)
    empty = read_of(rng, "cnt0", T, 0, 2000, 2300)
    empty["regs"] = [region(empty["a"], len(empty["seq"]), 0, 0)] + empty["regs"]
    scene("plain", "ont", [plain, rev, short, tn, empty])
    # cnt = 1, 2, 3 and regions with neighbour anchors on both sides (min_cnt + 1 of them tighten the bounds)
    few = []
    for cnt in (1, 2, 3):
        rd = read_of(rng, f"cnt{cnt}", T, 0, 300, 800)
        rd["regs"] = [region(rd["a"], len(rd["seq"]), len(rd["a"]) // 2, cnt)]
        few.append(rd)
    nb = read_of(rng, "neighbours", T, 0, 1200, 2400, step=40)
    n = len(nb["a"])
    nb["regs"] = [region(nb["a"], len(nb["seq"]), 6, n - 12), region(nb["a"], len(nb["seq"]), 2, 5, id_=1, parent=1)]
    scene("few_and_neighbours", "ont", few + [nb])
    # read end, target end, read start (a short first anchor: qs == 0) and target start (rs == 0)
    ends = [read_of(rng, "target_end", T, 1, 900, 1500), read_of(rng, "read_end", T, 0, 100, 600, sub=0, indel=0, step=15, jitter=False)]
    for nm, t0 in (("qs0", 400), ("rs0", 0)):
        rd = read_of(rng, nm, T, 0, t0, t0 + 400, sub=0, indel=0, jitter=False, edits=[(0, "ins", 20)])     # rs0: 20 bases ahead of the target's start
        first = np.array([[t0 + 7, 8 << 32 | 7]], np.uint64) if nm == "qs0" else np.array([[7, 8 << 32 | 27]], np.uint64)
        rd["a"] = np.concatenate([first, rd["a"][1:]])
        rd["regs"] = [region(rd["a"], len(rd["seq"]), 0, len(rd["a"]))]
        ends.append(rd)
    scene("ends", "ont", ends)
    # mm_fix_bad_ends: an indel above half the first / last anchor's span right behind / before it
    scene("bad_ends", "ont", [read_of(rng, "bad_start", T, 0, 300, 900, sub=0, indel=0, jitter=False, edits=[(333, "ins", 12)]),
                              read_of(rng, "bad_end", T, 0, 300, 900, sub=0, indel=0, jitter=False, edits=[(860, "del", 12)])])
    # mm_filter_bad_seeds: one gap (n <= 1), an insertion and a deletion of 25 close together (one run), two such pairs (two runs)
    scene("bad_seeds", "ont", [read_of(rng, "one_gap", T, 0, 300, 900, sub=0, indel=0, edits=[(600, "ins", 25)]),
                               read_of(rng, "one_run", T, 0, 300, 1000, sub=0, indel=0, edits=[(600, "ins", 25), (660, "del", 25)]),
                               ])
    # ... two such pairs further apart than max_gap / 2 (two runs)
    scene("bad_seeds_two_runs", "gap600", [read_of(rng, "two_runs", T, 0, 300, 1500, sub=0, indel=0, edits=[(600, "ins", 25), (660, "del", 25), (1100, "del", 30), (1160, "ins", 30)])])
    # seed flags: SELF on the first anchor, LONG_JOIN and TANDEM on an inner and on the last one; split_inv on input
    flags = []
    for nm, bit, where in (("self", A.SEED_SELF, 0), ("long_join_inner", A.SEED_LONG_JOIN, 4), ("long_join_last", A.SEED_LONG_JOIN, -1),
                           ("tandem_inner", A.SEED_TANDEM, 4), ("tandem_last", A.SEED_TANDEM, -1)):
        rd = read_of(rng, nm, T, 0, 500, 1100)
        rd["a"][where, 1] |= np.uint64(bit)
        if nm == "self":
            rd["regs"][0]["qs"] += 3
        flags.append(rd)
    inv_in = read_of(rng, "split_inv_in", T, 0, 1500, 2000)
    inv_in["regs"][0]["bits"] |= A.BIT_SPLIT_INV
    scene("seed_flags", "ont", flags + [inv_in])
    # mm_test_zdrop: a junk stretch (code 1) and an inverted one (code 2), each with many and with few anchors behind the drop
    scene("zdrop", "lowz", [read_of(rng, "junk_mid", T, 0, 200, 1400, edits=[(700, "junk", 150)]),
                            read_of(rng, "junk_late", T, 0, 200, 1000, edits=[(780, "junk", 150)], step=35),
                            read_of(rng, "inv_mid", T, 0, 1400, 2600, edits=[(1900, "inv", 160)]),
                            read_of(rng, "large_del", T, 0, 100, 1500, edits=[(700, "del", 300)])])
    scene("zdrop_min_cnt", "cnt2", [read_of(rng, "junk_late2", T, 0, 200, 1000, edits=[(760, "junk", 150)], step=40, jitter=False)])
    # mm_fix_cigar: junk at the read's start, no target ahead of the first anchor and a large end bonus (leading I); a duplicated unit at the alignment's start (leading D, and
    # an indel shifted by the whole M before it); equal ops at a stitch boundary come with every fill
    scene("leading_i", "bonus", [read_of(rng, "junk_start", T, 0, 0, 400, sub=0, indel=0, jitter=False, edits=[(0, "ins", 40)])])
    dup = read_of(rng, "dup_unit", T, 2, 304, 800, sub=0, indel=0, jitter=False)
    dup["a"] = np.concatenate([np.array([[2 << 32 | 307, 8 << 32 | 7]], np.uint64), dup["a"]])
    dup["regs"] = [region(dup["a"], len(dup["seq"]), 0, len(dup["a"]))]
    # a fill boundary inside a homopolymer run that is 4 shorter in the read, 2 inserted bases just ahead of the run: "2I 11M" meets "4D ..."
    flank_l, flank_r = rand_seq(rng, 199) + "G", "C" + rand_seq(rng, 299)
    T.append(flank_l + "A" * 30 + flank_r)
    seq = T[4][50:200] + "CC" + "A" * 26 + T[4][230:480]
    hp = [(4 << 32 | (50 + i), 15 << 32 | i) for i in (40, 80, 120)] + [(4 << 32 | 218, 15 << 32 | 170)] + [(4 << 32 | (i + 52), 15 << 32 | i) for i in (230, 270, 310, 350, 390)]
    hp = dict(name="shift_whole_m", seq=seq, a=np.array(hp, np.uint64))
    hp["regs"] = [region(hp["a"], len(seq), 0, len(hp["a"]))]
    scene("leading_d", "ont", [dup, hp])
    # HPC: k = 19, homopolymer runs in target and read
    scene("hpc", "hpc", [read_of(rng, "hpc_fwd", T, 3, 100, 900, k=19), read_of(rng, "hpc_rev", T, 3, 600, 1500, k=19, rev=1)])
    # another scoring set (asm20's) on the plain reads
    scene("asm", "asm", [read_of(rng, "asm_fwd", T, 0, 200, 900, sub=0.01, indel=0.005), read_of(rng, "asm_rev", T, 1, 100, 900, rev=1, sub=0.01, indel=0.005)])
    return scenes


def fuzz_scene(seed=7, n_reads=24):
    rng = np.random.default_rng(seed)
    T = [rand_seq(rng, int(n)) for n in rng.integers(1000, 4000, 3)]
    reads = []
    for i in range(n_reads):
        rid = int(rng.integers(0, len(T)))
        ln = int(rng.integers(150, 1500))
        ln = min(ln, len(T[rid]) - 20)
        t0 = int(rng.integers(0, len(T[rid]) - ln))
        edits = []
        if ln > 600 and rng.random() < 0.5:
            pos = t0 + int(rng.integers(200, ln - 300))
            edits.append((pos, ["junk", "inv", "del", "n", "ins"][int(rng.integers(0, 5))], int(rng.integers(20, 200))))
        rd = read_of(rng, f"fuzz{i}", T, rid, t0, t0 + ln, rev=int(rng.integers(0, 2)), step=int(rng.integers(20, 60)), sub=0.04, indel=0.03, edits=edits)
        n = len(rd["a"])
        if n >= 12 and rng.random() < 0.4:           # two regions of one read, with neighbours
            cut = int(rng.integers(4, n - 4))
            rd["regs"] = [region(rd["a"], len(rd["seq"]), 0, cut), region(rd["a"], len(rd["seq"]), cut, n - cut, id_=1, parent=1)]
        if n == 0:
            rd["regs"] = []
        reads.append(rd)
    return _finish(dict(name="fuzz", opt=dict(OPTS["lowz"]), targets=T, reads=reads))


def pack(scene):
    """The flat arrays chaindp_align1 takes."""
    reads = scene["reads"]
    seq = "".join(rd["seq"] for rd in reads)
    tseq = "".join(scene["targets"])
    return dict(opt=np.array([scene["opt"][k] for k in A.OPT_FIELDS], np.int32),
                tseq=np.frombuffer(tseq.encode(), np.uint8), tseq_off=np.concatenate([[0], np.cumsum([len(t) for t in scene["targets"]])]).astype(np.int64),
                seq=np.frombuffer(seq.encode(), np.uint8), seq_off=np.concatenate([[0], np.cumsum([len(rd["seq"]) for rd in reads])]).astype(np.int64),
                a=np.concatenate([rd["a"].reshape(-1, 2) for rd in reads]).astype(np.uint64) if reads else np.zeros((0, 2), np.uint64),
                a_off=np.concatenate([[0], np.cumsum([len(rd["a"]) for rd in reads])]).astype(np.int64),
                regs=np.concatenate([rd["regs"] for rd in reads]) if reads else np.zeros(0, REG_DTYPE),
                regs_off=np.concatenate([[0], np.cumsum([len(rd["regs"]) for rd in reads])]).astype(np.int64),
                read_name=np.array([rd["name"] for rd in reads]))


def model_scene(p):
    """align_model.align1 over the packed scene p (pack()'s dict or a loaded golden): (a, regs, regs2, extra, cigar_off, cigar) as
    chaindp_align1 returns them."""
    opt = dict(zip(A.OPT_FIELDS, (int(v) for v in p["opt"])))
    tcodes = [A.nt4(bytes(p["tseq"][p["tseq_off"][i]:p["tseq_off"][i + 1]])) for i in range(len(p["tseq_off"]) - 1)]
    a, regs = p["a"].copy(), p["regs"].copy()
    regs2, extra = np.zeros(len(regs), REG_DTYPE), np.zeros(len(regs), EXTRA_DTYPE)
    cigs = []
    for rd in range(len(p["seq_off"]) - 1):
        qf = A.nt4(bytes(p["seq"][p["seq_off"][rd]:p["seq_off"][rd + 1]]))
        a0, a1 = int(p["a_off"][rd]), int(p["a_off"][rd + 1])
        ax, ay = [int(v) for v in a[a0:a1, 0]], [int(v) for v in a[a0:a1, 1]]
        for i in range(int(p["regs_off"][rd]), int(p["regs_off"][rd + 1])):
            r = reg_dict(regs[i])
            r2, ex, cig = A.align1(opt, tcodes, qf, ax, ay, r)
            for k in A.REG_FIELDS:
                if k != "div":
                    regs[k][i] = r[k] & 0xffffffff if k in ("bits", "hash") else r[k]
                    if r2["cnt"]:
                        regs2[k][i] = r2[k] & 0xffffffff if k in ("bits", "hash") else r2[k]
            if r2["cnt"]:
                regs2["div"][i] = regs["div"][i]
            for k in A.EXTRA_FIELDS:
                extra[k][i] = ex[k]
            cigs.append(cig)
        a[a0:a1, 0], a[a0:a1, 1] = np.array(ax, np.uint64), np.array(ay, np.uint64)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.int64)
    return a, regs, regs2, extra, off, np.concatenate(cigs).astype(np.uint32) if len(cigs) and off[-1] else np.zeros(0, np.uint32)
