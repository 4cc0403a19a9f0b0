"""Inputs of the mm_align1_inv tests: named scenes, each at the smallest size at which its property can go wrong, and a seeded fuzz.

A scene is dict(name, opt, targets [str], reads [dict(seq str, regs [dict])]) -- one call of chaindp_align1_inv.  A read is
A + revcomp(X') + B against a target A + X + B (or its reverse complement, for regions on the reverse strand), with the regions of A
and B written by hand as mm_align1 and mm_split_reg would leave them: the call reads only their fields.  max_gap is small (200) where a
scene sits on it; the flanks are longer than the seven bases the start of the extension can lie before the stretch, so that no scene
falls into unspecified behaviour (the generator asserts it)."""
import zlib

import numpy as np

import align_model as A
import inv_model as M
from align_shapes import ACGT, EXTRA_DTYPE, REG_DTYPE, rand_seq, rc, reg_dict, regs_array

OPT = dict(a=2, b=4, q=4, e=2, q2=24, e2=1, bw=40, zdrop=400, zdrop_inv=200, end_bonus=-1, min_cnt=3, min_chain_score=40, min_dp_max=80,
           min_ksw_len=40, max_gap=200, flag=0, k=15, is_hpc=0)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def other(rng, s):
    """s with every base replaced by another one: nothing of it aligns base for base."""
    return "".join(ACGT[(ACGT.index(c) + int(rng.integers(1, 4))) % 4] if c in ACGT else c for c in s)


def noisy(rng, s, sub=0.05):
    return "".join(ACGT[(ACGT.index(c) + int(rng.integers(1, 4))) % 4] if c in ACGT and rng.random() < sub else c for c in s)


def reg(qs, qe, rs, re, rev, bits, rid=0, id_=0, parent=0):
    r = M.zero_reg()
    r.update({"id": id_, "parent": parent, "rid": rid, "qs": qs, "qe": qe, "rs": rs, "re": re, "cnt": 3, "score": 40, "score0": 40,
              "mlen": qe - qs, "blen": qe - qs, "bits": bits | (M.BIT_REV if rev else 0)})
    return r


def chain(rng, flanks, stretches, rev=0, rid=0, t_pre=""):
    """A target t_pre + F0 + X1 + F1 + X2 + F2 ... and its read: stretches = [(x_t, x_q)], x_q being what the read carries on the strand
    opposite to the regions' in the place of x_t.  Returns (target, read, regions): region i covers flank i; every region but the last
    has split & 1, every one but the first split & 2, split_inv and parent MM_PARENT_TMP_PRI."""
    fl = [rand_seq(rng, n) if isinstance(n, int) else n for n in flanks]
    target, frag, tpos, fpos = t_pre, "", [], []
    for i, f in enumerate(fl):
        tpos.append((len(target), len(target) + len(f))); fpos.append((len(frag), len(frag) + len(f)))
        target += f; frag += f
        if i < len(stretches):
            target += stretches[i][0]; frag += rc(stretches[i][1])
    read, qlen, regs = (rc(frag) if rev else frag), len(frag), []
    for i, ((t0, t1), (f0, f1)) in enumerate(zip(tpos, fpos)):
        bits = (M.BIT_SPLIT1 if i < len(fl) - 1 else 0) | ((M.BIT_SPLIT2 | M.BIT_SPLIT_INV) if i > 0 else 0)
        qs, qe = (qlen - f1, qlen - f0) if rev else (f0, f1)
        regs.append(reg(qs, qe, t0, t1, rev, bits, rid, id_=0 if i == 0 else -1, parent=0 if i == 0 else M.PARENT_TMP_PRI))
    return target, read, regs


def one(name, x_t, x_q, rev=0, opt=None, la=30, lb=30, edit=None):
    """A scene of one read with one pair.  edit(r1, r2) may change the regions."""
    rng = _rng(name + "/flanks")
    target, read, regs = chain(rng, (la, lb), [(x_t, x_q)], rev)
    if edit:
        edit(regs[0], regs[1])
    return dict(name=name, opt=dict(OPT, **(opt or {})), targets=[target], reads=[dict(seq=read, regs=regs)])


def merge(name, scenes, opt=None):
    """The reads of several one-target scenes of the same opt in one scene, each with its own target."""
    out = dict(name=name, opt=dict(scenes[0]["opt"], **(opt or {})), targets=[], reads=[])
    for sc in scenes:
        assert len(sc["targets"]) == 1
        for rd in sc["reads"]:
            regs = [dict(r, rid=len(out["targets"])) for r in rd["regs"]]
            out["reads"].append(dict(seq=rd["seq"], regs=regs))
        out["targets"].append(sc["targets"][0])
    return out


def related(rng, n, n_t=None, sub=0.04):
    """(x_t, x_q): x_q a noisy copy of x_t's middle, both with unrelated ends so that the best local alignment reaches neither end."""
    core = rand_seq(rng, n - 16)
    x_t = rand_seq(rng, 8 + ((n_t or n) - n if (n_t or n) > n else 0)) + core + rand_seq(rng, 8)
    x_q = rand_seq(rng, 8) + noisy(rng, core, sub) + rand_seq(rng, 8)
    if n_t is not None and n_t < n:
        x_t = x_t[:4] + x_t[4 + n - n_t:]
    return x_t, x_q


def early_scene():
    """Every early return on its own, both ways round; one read per case."""
    rng = _rng("early")
    cases = []

    def case(nm, lq=60, lt=60, edit=None, rev=0):
        x_t, x_q = related(rng, max(lq, 20), None)
        x_t, x_q = (x_t * 20)[:lt], (x_q * 20)[:lq]
        cases.append(one("early/" + nm, x_t, x_q, rev, edit=edit))

    def setbits(which, clear):
        def f(r1, r2):
            (r1 if which == 1 else r2)["bits"] &= ~clear
        return f

    def setf(which, **kw):
        def f(r1, r2):
            (r1 if which == 1 else r2).update(kw)
        return f
    case("eligible")
    case("eligible_rev", rev=1)
    case("split1_unset", edit=setbits(1, M.BIT_SPLIT1))
    case("split2_unset", edit=setbits(2, M.BIT_SPLIT2))
    case("split1_has_only_bit2", edit=lambda r1, r2: r1.update(bits=(r1["bits"] & ~M.BIT_SPLIT1) | M.BIT_SPLIT2))
    case("split2_has_only_bit1", edit=lambda r1, r2: r2.update(bits=(r2["bits"] & ~M.BIT_SPLIT2) | M.BIT_SPLIT1))
    case("split_inv_unset", edit=setbits(2, M.BIT_SPLIT_INV))
    case("parent1_is_id", edit=setf(1, id=5, parent=5))
    case("parent1_tmp_pri", edit=setf(1, id=5, parent=M.PARENT_TMP_PRI))
    case("parent1_other", edit=setf(1, id=5, parent=2))
    case("parent1_unset", edit=setf(1, id=5, parent=M.PARENT_UNSET))
    case("parent2_is_id", edit=setf(2, id=7, parent=7))
    case("parent2_other", edit=setf(2, id=7, parent=0))
    case("parent2_unset", edit=setf(2, id=-1, parent=-3))
    case("rev_differs", edit=lambda r1, r2: r2.update(bits=r2["bits"] ^ M.BIT_REV))
    mcs, mg = OPT["min_chain_score"], OPT["max_gap"]
    for nm, v in (("low", mcs - 1), ("at_min", mcs), ("at_max_gap", mg), ("high", mg + 1)):
        case("ql_" + nm, lq=v, lt=90)
        case("tl_" + nm, lq=90, lt=v)
    sc = merge("early_returns", cases)
    # a pair on two targets (rid differs), a read of one region, a read of none
    r1, r2 = (dict(r) for r in sc["reads"][0]["regs"])
    r2["rid"] = 1
    sc["reads"].append(dict(seq=sc["reads"][0]["seq"], regs=[r1, r2]))
    sc["reads"].append(dict(seq=sc["reads"][0]["seq"], regs=[dict(sc["reads"][0]["regs"][0])]))
    sc["reads"].append(dict(seq=rand_seq(rng, 50), regs=[]))
    return sc


def padding_scenes():
    """qe in the padding: the inverted stretch matches from the query stretch's first base on, the target stretch has bases before it."""
    out = []
    for rev in (0, 1):
        cases = []
        for ql in (49, 52, 55, 56):
            rng = _rng("pad%d/%d" % (ql, rev))
            core = rand_seq(rng, ql - 6)
            x_q = core + rand_seq(rng, 6)
            x_t = rand_seq(rng, 19) + core + other(rng, x_q[-6:]) + rand_seq(rng, 5)
            cases.append(one("pad/%d/%d" % (ql, rev), x_t, x_q, rev))
        # an N directly behind the best cell inside the stretch: te and qe move by one, not into the padding
        rng = _rng("padn/%d" % rev)
        core = rand_seq(rng, 44)
        cases.append(one("pad/n/%d" % rev, rand_seq(rng, 12) + "C" + core + rand_seq(rng, 9), rand_seq(rng, 10) + "N" + core + rand_seq(rng, 9), rev))
        out.append(merge("padding_strand%d" % rev, cases))
    return out


def tie_scenes():
    out = []
    # te: the unit twice in the target, once in the query: the same maximum in two columns, the last one (the earlier copy) wins
    rng = _rng("te_tie")
    u = rand_seq(rng, 45)
    out.append(one("te_tie", rand_seq(rng, 6) + "AAA" + u + "AAA" + rand_seq(rng, 5) + "AAA" + u + "AAA" + rand_seq(rng, 7),
                   rand_seq(rng, 9) + "CCC" + u + "CCC" + rand_seq(rng, 10)))
    # qe: the unit three times in the query, once in the target: one column, three rows; the striped order picks the middle one.  The
    # spacers are searched for, the model's counter (qe_tie_middle) is the proof.
    rng = _rng("qe_tie")
    u = rand_seq(rng, 42)
    mat = A.simple_mat(OPT["a"], OPT["b"])
    for s1, s2 in ((s1, s2) for s1 in range(3, 30) for s2 in range(3, 20)):
        x_q = "T" * 5 + u + "G" * s1 + u + "A" * s2 + u + "C" * 6
        x_t = rand_seq(_rng("qe_tie_t"), 6) + "CCCC" + u + rand_seq(_rng("qe_tie_t2"), 10)
        q, t = A.nt4(x_q)[::-1], A.nt4(x_t)[::-1]
        full = M.ll_ends(q, t, mat, OPT["q"], OPT["e"])
        if full != M.ll_ends(q, t, mat, OPT["q"], OPT["e"], tie="first") and full != M.ll_ends(q, t, mat, OPT["q"], OPT["e"], tie="last") and full[1] < len(q):
            out.append(one("qe_tie", x_t, x_q))
            break
    else:
        raise AssertionError("no qe tie found")
    return out


def edge_scene():
    """ql and tl on the lane and stripe edges of the local-score kernel and on the 8-row edges of the padding, ql < tl and ql > tl."""
    cases = []
    for n in (63, 64, 65, 127, 128, 129):
        for ql, tl in ((n, n + 5), (n + 5, n)):
            rng = _rng("edge%d/%d" % (ql, tl))
            x_t, x_q = related(rng, ql, tl)
            assert len(x_q) == ql and len(x_t) == tl, (ql, tl, len(x_q), len(x_t))
            cases.append(one("edge/%d/%d" % (ql, tl), x_t, x_q, rev=n & 1))
    return merge("stripe_edges", cases)


def route_scene(name, n, opt):
    rng = _rng(name)
    x_t, x_q = related(rng, n, n + 24, sub=0.06)
    x_q = x_q[:n // 3] + x_q[n // 3 + 3:2 * n // 3] + "GA" + x_q[2 * n // 3:]          # a deletion and an insertion on the way
    return one(name, x_t, x_q, opt=opt, la=40, lb=40)


def named_scenes():
    sc = [early_scene()] + padding_scenes() + tie_scenes() + [edge_scene()]
    # score == min_dp_max and min_dp_max - 1: the same pair under two thresholds around the model's score of it
    rng = _rng("score")
    core = rand_seq(rng, 43)
    x_t, x_q = rand_seq(rng, 9) + core + rand_seq(rng, 9), other(rng, rand_seq(rng, 8)) + core + rand_seq(rng, 7)
    score = M.ll_ends(A.nt4(x_q)[::-1], A.nt4(x_t)[::-1], A.simple_mat(OPT["a"], OPT["b"]), OPT["q"], OPT["e"])[0]
    sc.append(one("score_at_min_dp_max", x_t, x_q, opt=dict(min_dp_max=score)))
    sc.append(one("score_below_min_dp_max", x_t, x_q, opt=dict(min_dp_max=score + 1)))
    # saturation at 32767: a = 127 over 270 matching bases
    rng = _rng("sat")
    core = rand_seq(rng, 270)
    sc.append(one("saturation", rand_seq(rng, 11) + core + rand_seq(rng, 9), rand_seq(rng, 8) + core + rand_seq(rng, 12), opt=dict(a=127, max_gap=400, zdrop=30000)))
    # the extension on the DP's three routes; bw = 500 as the long-read presets have it (a band of 750)
    sc.append(route_scene("route_wide", 700, dict(bw=500, max_gap=5000)))
    sc.append(route_scene("route_global", 5560, dict(bw=500, max_gap=6000)))
    # a Z-dropped extension: the inverted stretch ends and unrelated bases follow
    rng = _rng("zdrop")
    core = rand_seq(rng, 80)
    sc.append(one("ext_zdrop", rand_seq(rng, 8) + core + rand_seq(rng, 100), rand_seq(rng, 9) + core + rand_seq(rng, 100), opt=dict(zdrop=40)))
    # a leading I and a leading D that mm_fix_cigar removes, on each strand.  A local alignment never starts with a gap; the extension
    # does where it starts in the padding: seven bases before the stretch (ql % 8 == 1), which here are the target's seven shifted by one
    lead = []
    for rev in (0, 1):
        for kind in "ID":
            rng = _rng("lead%s%d" % (kind, rev))
            core, P = rand_seq(rng, 43), rand_seq(rng, 7)
            z = P[1:] + other(rng, P[:1]) if kind == "I" else other(rng, P[-1:]) + P[:-1]
            x_q = core + rand_seq(rng, 6)
            x_t = rand_seq(rng, 12) + z + core + other(rng, x_q[-6:]) + rand_seq(rng, 5)
            target, read, regs = chain(_rng("lead/flanks%s%d" % (kind, rev)), (30, rc(P) + rand_seq(rng, 23)), [(x_t, x_q)], rev)
            lead.append(dict(name="lead", opt=dict(OPT), targets=[target], reads=[dict(seq=read, regs=regs)]))
    sc.append(merge("leading_gap", lead))
    # N on both sides inside the inverted stretch
    amb = []
    for rev in (0, 1):
        rng = _rng("ambi%d" % rev)
        core = rand_seq(rng, 70)
        amb.append(one("ambi/%d" % rev, rand_seq(rng, 9) + core[:20] + "N" + core[21:] + rand_seq(rng, 9),
                       rand_seq(rng, 9) + core[:40] + "NN" + core[42:] + rand_seq(rng, 9), rev))
    sc.append(merge("n_both_sides", amb))
    # the extension gives no CIGAR: b > 2 (q + e) is ksw_extd2_sse's early return
    rng = _rng("nocigar")
    x_t, x_q = related(rng, 70)
    sc.append(one("no_cigar", x_t, x_q, opt=dict(b=13)))
    # three regions, both pairs eligible: the second is never tested; with the first failing min_dp_max the second is made
    for nm, first_related in (("three_regions_skip", True), ("three_regions_first_fails", False)):
        reads = []
        targets = []
        for rev in (0, 1):
            rng = _rng(nm + str(rev))
            s1, s2 = related(rng, 70), related(rng, 66)
            if not first_related:
                s1 = (s1[0], other(rng, s1[0]))
            t, rd, regs = chain(rng, (30, 35, 30), [s1, s2], rev, rid=len(targets))
            targets.append(t); reads.append(dict(seq=rd, regs=regs))
        sc.append(dict(name=nm, opt=dict(OPT), targets=targets, reads=reads))
    # a query stretch of 19 996 bases under max_gap = 20 000: 79 984 bytes for the local-score kernel's edge, past the 64 KB a launch
    # gets without asking.  The copy lies at the stretch's end, so the extension is short; the target stretch is two stripes.
    rng = _rng("lds")
    core = rand_seq(rng, 60)
    sc.append(one("ll_lds_above_64k", rand_seq(rng, 8) + core + rand_seq(rng, 8), rand_seq(rng, 19926) + core + rand_seq(rng, 10), rev=1,
                  opt=dict(max_gap=20000)))
    return sc


def fuzz_scene(seed=20240917, n_pairs=200):
    """About 200 pairs, both strands, one to three stretches per read; some stretches unrelated, some with Ns, some copied from the
    stretch's very start (the padding) or with the target stretch starting right at the copy."""
    rng = np.random.default_rng(seed)
    targets, reads, n = [], [], 0
    while n < n_pairs:
        k = int(rng.integers(1, 4))
        st = []
        for _ in range(k):
            ql = int(rng.integers(40, 181))
            kind = int(rng.integers(0, 6))
            core = rand_seq(rng, max(ql - int(rng.integers(0, 30)), 30))
            x_q = noisy(rng, core, 0.08 * rng.random()) + rand_seq(rng, ql - len(core))
            if kind == 0:
                x_t = rand_seq(rng, int(rng.integers(40, 181)))
            else:
                x_t = rand_seq(rng, int(rng.integers(0, 25))) + core + rand_seq(rng, int(rng.integers(0, 25)))
            if kind == 1:
                i = int(rng.integers(0, len(x_q)))
                x_q = x_q[:i] + "N" + x_q[i + 1:]
            if kind == 2:
                x_q = rand_seq(rng, int(rng.integers(1, 12))) + x_q
            st.append((x_t[:200], x_q[:200]))
        t, rd, regs = chain(rng, [int(rng.integers(12, 40)) for _ in range(k + 1)], st, int(rng.integers(0, 2)), rid=len(targets))
        targets.append(t); reads.append(dict(seq=rd, regs=regs))
        n += k
    return dict(name="fuzz", opt=dict(OPT), targets=targets, reads=reads)


def pack(scene):
    """The flat arrays of a scene: what the golden files keep and what the C call takes."""
    t_off = np.concatenate([[0], np.cumsum([len(t) for t in scene["targets"]])]).astype(np.int64)
    s_off = np.concatenate([[0], np.cumsum([len(r["seq"]) for r in scene["reads"]])]).astype(np.int64)
    r_off = np.concatenate([[0], np.cumsum([len(r["regs"]) for r in scene["reads"]])]).astype(np.int64)
    regs = regs_array([r for rd in scene["reads"] for r in rd["regs"]])
    return dict(opt=np.array([scene["opt"][k] for k in A.OPT_FIELDS], np.int32), tseq_off=t_off,
                tseq=np.frombuffer("".join(scene["targets"]).encode(), np.uint8), seq_off=s_off,
                seq=np.frombuffer("".join(r["seq"] for r in scene["reads"]).encode(), np.uint8), regs_off=r_off, regs=regs)


def model_scene(p):
    """inv_model over a packed scene: (made, r_inv, extra, cigar_off, cigar, ll int32[n_candidates, 3], prob int32[n_survivors, 3])."""
    opt = dict(zip(A.OPT_FIELDS, (int(v) for v in p["opt"])))
    tcodes = [A.nt4(bytes(p["tseq"][p["tseq_off"][i]:p["tseq_off"][i + 1]])) for i in range(len(p["tseq_off"]) - 1)]
    n = len(p["regs"])
    made, r_inv, extra = np.zeros(n, np.int32), np.zeros(n, REG_DTYPE), np.zeros(n, EXTRA_DTYPE)
    cigs, lls = [], []
    n0 = len(M.problems)
    for rd in range(len(p["seq_off"]) - 1):
        qf = A.nt4(bytes(p["seq"][p["seq_off"][rd]:p["seq_off"][rd + 1]]))
        g0, g1 = int(p["regs_off"][rd]), int(p["regs_off"][rd + 1])
        res = M.read_pairs(opt, tcodes, qf, [reg_dict(p["regs"][g]) for g in range(g0, g1)])
        for g, (code, r, ex, cig, ll) in zip(range(g0, g1), res):
            made[g] = code
            for k in A.REG_FIELDS:
                r_inv[k][g] = r[k] & 0xffffffff if k in ("bits", "hash") else r[k]
            for k in A.EXTRA_FIELDS:
                extra[k][g] = ex[k]
            cigs.append(cig)
            if ll is not None:
                lls.append(ll)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.int64)
    cigar = np.concatenate(cigs).astype(np.uint32) if len(cigs) and off[-1] else np.zeros(0, np.uint32)
    return (made, r_inv, extra, off, cigar, np.array(lls, np.int32).reshape(-1, 3), np.array(M.problems[n0:], np.int32).reshape(-1, 3))
