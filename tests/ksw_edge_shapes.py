"""Inputs of the edge tier of the extension alignment (chaindp_ksw_extd): scenes that reach what the named and fuzz batches of ksw_shapes
never do -- scoring sets from the corners of the accepted domain 0..127, every flag path and both ways out of the diagonal loop on the
global route, one- and two-base sides on the wide route, and `interleave`, one call whose order by falling work puts unlike problems
next to each other for the workgroup that takes them one after another (Device.ksw_set_grid_cap).

A scene is a list of problems in the dict shape of ksw_shapes (name, query, target, scoring as a tuple, w, zdrop, end_bonus, flag) with
one scoring set: one call.  scenes() gives {file name: problems}; tests/golden/make_ksw_edge_golden.py records the reference's answers
under tests/golden/ksw_edges/, tests/test_ksw_edges_cpu.py and tests/test_gpu_ksw_edges.py read them.  Every problem draws from a
generator seeded by its own name, so adding or dropping one changes no other."""
import numpy as np

import ksw_model as M
import ksw_shapes as S
from ksw_shapes import ROUTE_GLOBAL, ROUTE_LDS, ROUTE_NONE, ROUTE_WIDE, _rng, expected_route, fit, groups, mutate, pack, pair, rand_seq, state_bytes  # noqa: F401

DEFAULT = S.SCORING["default"]
FLAGS6 = (0, 0x02, 0x40, 0xc2, 0x08, 0x09)
FLAGS8 = (0, 0x01, 0x02, 0x08, 0x09, 0x40, 0xc2, 0x80)


def early(sc):
    a, b, q, e, q2, e2 = sc
    return b > 2 * min(q + e, q2 + e2)


def swapped(sc):
    """q, e, q2, e2 as the DP uses them: the cheaper first cost first (no swap on a tie)."""
    a, b, q, e, q2, e2 = sc
    return (q2, e2, q, e) if q2 + e2 < q + e else (q, e, q2, e2)


def _random_sets(n=12, seed=20241020):
    """Seeded sets uniform over 0..127; a draw that returns early is drawn again (the early return has sets of its own)."""
    rng, out = np.random.default_rng(seed), []
    while len(out) < n:
        sc = tuple(int(v) for v in rng.integers(0, 128, 6))
        if not early(sc):
            out.append(sc)
    return out


# class -> a, b, q, e, q2, e2
SCORING = {
    "splice": (1, 2, 2, 1, 32, 0),              # the reference's splice preset: e2 == 0, the wildcard scores 0, Z-drop ignores the gap
    "e_eq_e2": (2, 4, 4, 2, 24, 2),             # long_thres 0
    "identical": (2, 4, 4, 2, 4, 2),            # one gap model twice
    "e_lt_e2": (2, 4, 4, 1, 6, 3),              # a negative quotient in long_thres
    "e_zero": (2, 4, 10, 0, 3, 2),              # swapped; e2 == 0 after the swap
    "q_zero": (2, 4, 0, 3, 20, 0),
    "tie_sum": (2, 4, 5, 1, 4, 2),              # q + e == q2 + e2: no swap
    "tie_sum_rev": (2, 4, 4, 2, 5, 1),
    "a_zero": (0, 4, 4, 2, 24, 1),
    "b_zero": (2, 0, 4, 2, 24, 1),
    "b_on_edge": (2, 12, 4, 2, 24, 1),          # b == 2 (q + e): computed
    "b_past_edge": (2, 13, 4, 2, 24, 1),        # one more: the early return
    "b_past_edge_swapped": (2, 13, 24, 1, 4, 2),    # ... decided on the cheaper cost, which is the second one here
    "all_zero": (0, 0, 0, 0, 0, 0),
    "all_127": (127, 127, 127, 127, 127, 127),
    "big_gaps": (2, 4, 100, 100, 100, 100),     # both sums wrap int8
    "wrap_mixed": (3, 5, 60, 70, 120, 127),
    "second_wraps": (2, 4, 4, 2, 100, 60),      # only q2 + e2 above 127
}
SCORING.update({f"rand_{k:02d}": sc for k, sc in enumerate(_random_sets())})
EARLY = tuple(k for k, sc in SCORING.items() if early(sc))


def case(name, q, t, scoring=DEFAULT, w=-1, zdrop=-1, end_bonus=-1, flag=0):
    return dict(name=name, query=np.asarray(q, np.uint8), target=np.asarray(t, np.uint8), scoring=tuple(scoring), w=w, zdrop=zdrop, end_bonus=end_bonus,
                flag=flag)


def with_wildcards(rng, seq, n):
    out = seq.copy()
    out[rng.integers(0, len(seq), n)] = 4
    return out


def scoring_cases(cls):
    """About ten LDS problems under SCORING[cls]: zdrop alternates between 100 and none, so half of them cannot Z-drop on the first
    diagonals where the set's sums wrap."""
    sc = SCORING[cls]
    q_, e, q2, e2 = swapped(sc)
    lt, _ = M.long_gap(q_, e, q2, e2)
    out = []

    def add(tag, q, t, flag, **kw):
        out.append(case(f"{cls}_{tag}", q, t, sc, zdrop=-1 if len(out) & 1 else 100, flag=flag, **kw))
    pairs = [pair(f"edge_{cls}_{k}", 90, 97, max_indel=30) for k in range(2)]
    for k, flag in enumerate(FLAGS6):
        add(f"rel_f{flag:02x}", *pairs[k // 3], flag, end_bonus=10 if flag & 0x40 else -1)
    rng = _rng(f"edge_{cls}_wild")
    q, t = pair(f"edge_{cls}_wild", 80, 84)
    add("wild", with_wildcards(rng, q, 6), with_wildcards(rng, t, 8), 0x40, end_bonus=5)
    add("homo", np.zeros(40), np.zeros(44), 0)
    if 0 < lt <= 54:                             # a deletion one past long_thres and an insertion one short of it (at least 1) in one pair
        rng = _rng(f"edge_{cls}_long")
        core = rand_seq(rng, 75)
        tgt = np.concatenate([core[:25], rand_seq(rng, lt + 1), core[25:]])
        qry = np.concatenate([core[:50], rand_seq(rng, max(lt - 1, 1)), core[50:]])
        add(f"long_{lt}", qry, tgt, 0)
        add(f"long_{lt}_right", qry, tgt, 0x02)
    return out


def head_tail(name, head, q_tail, tlen, sub=0.08):
    """A related head, then unrelated tails: query head + q_tail bases, target of tlen."""
    rng = _rng(name)
    h = rand_seq(rng, head)
    return np.concatenate([h, rand_seq(rng, q_tail)]), fit(rng, mutate(rng, h, sub=sub), tlen)


def global_flags():
    """About 25 problems on the global route in one call; the targets run from 5 460 to 5 700, so every slice is sized for the largest."""
    out = []
    for k, flag in enumerate(FLAGS8):            # Z-drop in the tails; the approximate maximum cannot Z-drop: its band runs out
        q, t = head_tail(f"glob_head_{flag:02x}", 200, 100 - k, 5460 + 30 * k)
        out.append(case(f"glob_head_f{flag:02x}", q, t, w=60, zdrop=50, end_bonus=10, flag=flag))
    for k, flag in enumerate(FLAGS8):            # no Z-drop: every one leaves by the band
        q, t = head_tail(f"glob_band_{flag:02x}", 60, 20 + 3 * k, 5700 - 16 * k)
        out.append(case(f"glob_band_f{flag:02x}", q, t, w=17 + 5 * k, zdrop=-1, end_bonus=-1, flag=flag))
    q, t = head_tail("glob_band_out", 100, 0, 5480)
    out.append(case("glob_band_out", q, t, w=30))
    out.append(case("glob_tie_homo", np.zeros(64), np.zeros(5470), w=70, zdrop=100, flag=0x40))
    out.append(case("glob_tie_two", np.tile([0, 1], 40), np.tile([0, 1], 2740), w=33, zdrop=100, flag=0))
    # unrelated two-letter sequences under a small Z-drop: equal maxima on a diagonal decide where (and whether) the loop breaks; without
    # a band the break is Z-drop's beyond doubt (the band of the problems above would run out later anyway)
    for k, w, zd, flag in ((4, -1, 10, 0), (20, 40, 10, 0x40), (5, 40, 5, 0xc2)):
        rng = _rng(f"glob_zdrop_tie_{k}")
        out.append(case(f"glob_zdrop_tie_{k}", rand_seq(rng, 60, 2), rand_seq(rng, 5470, 2), w=w, zdrop=zd, end_bonus=10, flag=flag))
    q, t = head_tail("glob_zdrop_no_band", 200, 100, 5600)
    out.append(case("glob_zdrop_no_band", q, t, zdrop=50, end_bonus=10, flag=0x40))
    rng = _rng("glob_wild")
    q, t = head_tail("glob_wild", 250, 0, 5520, sub=0.03)
    out.append(case("glob_wild", with_wildcards(rng, q, 20), with_wildcards(rng, t, 400), w=80, zdrop=50, end_bonus=10, flag=0x40))
    rng = _rng("glob_one")
    out.append(case("glob_1x5500", rand_seq(rng, 1), rand_seq(rng, 5500)))
    out.append(case("glob_1x5500_ext", rand_seq(rng, 1), rand_seq(rng, 5500), zdrop=100, end_bonus=10, flag=0x40))
    out.append(case("glob_2x5470_score", rand_seq(rng, 2), rand_seq(rng, 5470), flag=0x01))
    q, t = pair("glob_long_query", 3000, 5500, sub=0.05, indel=0.02)
    out.append(case("glob_long_query_3000x5500", q, t, w=100, zdrop=400, end_bonus=10, flag=0x40))
    # the query's end is reached only where the band never runs out: no band, a short query against the whole target
    rng = _rng("glob_reach")
    t = rand_seq(rng, 5460)
    out.append(case("glob_reach_end", mutate(rng, t[:120], sub=0.03, indel=0.0)[:120], t, zdrop=-1, end_bonus=10, flag=0x40))
    out.append(case("glob_no_reach_end", np.concatenate([t[:100], (t[100:120] + 1) % 4]), t, zdrop=-1, end_bonus=10, flag=0x40))
    # a complete alignment at a narrow band needs sides of nearly one length: the second long query of the scene
    q, t = pair("glob_complete", 5480, 5500, sub=0.03, indel=0.01, max_indel=2)
    out.append(case("glob_complete_5480x5500_w20", q, t, w=20))
    return out


# 700 x 17 keeps its state in one wave's LDS (1 104 bytes); the nearest query against 17 target bases that passes WIDE_BYTES is this long
WIDE_SHORT_TARGET = (7793, 17)


def wide_small_sides():
    rng = _rng("wide_small")
    out = [case("wide_1x700", rand_seq(rng, 1), rand_seq(rng, 700)), case("wide_1x700_ext", rand_seq(rng, 1), rand_seq(rng, 700), zdrop=100, end_bonus=10, flag=0x40),
           case("wide_2x690", rand_seq(rng, 2), rand_seq(rng, 690)), case("wide_2x690_right", rand_seq(rng, 2), rand_seq(rng, 690), flag=0x02)]
    q, t = pair("wide_short_target", *WIDE_SHORT_TARGET)
    out.append(case("wide_%dx%d" % WIDE_SHORT_TARGET, q, t))
    out.append(case("wide_%dx%d_w5" % WIDE_SHORT_TARGET, q, t, w=5, flag=0x40, zdrop=100))
    q, t = pair("wide_small_flags", 690, 700)
    out.append(case("wide_score_only", q, t, w=50, zdrop=400, flag=0x01))
    out.append(case("wide_approx_max", q, t, w=50, zdrop=400, flag=0x08))
    out.append(case("wide_approx_score_only", q, t, w=50, zdrop=400, flag=0x09))
    return out


# ---- interleave: the order a single workgroup takes the problems in
def work(c):
    """n_diag * n_col of the plan (chaindp_ksw_plan.h): 0 for a problem that returns early."""
    ql, tl = len(c["query"]), len(c["target"])
    if expected_route(ql, tl, c["scoring"]) == ROUTE_NONE:
        return 0
    return (ql + tl - 1) * M.geometry(ql, tl, min(c["w"], max(ql, tl)))[3]


def route(c):
    return expected_route(len(c["query"]), len(c["target"]), c["scoring"])


def plan_order(cases):
    """The plan's order: the one-wave launch (early returns, LDS, global) and then the several-wave launch, each by falling work, equal
    work in the call's order.  Returns (order of launch 0, order of launch 1) as indices into cases."""
    idx = sorted(range(len(cases)), key=lambda i: (route(cases[i]) == ROUTE_WIDE, -work(cases[i])))
    n0 = sum(route(c) != ROUTE_WIDE for c in cases)
    return idx[:n0], idx[n0:]


def band_runs_out(c):
    ql, tl = len(c["query"]), len(c["target"])
    w = c["w"] if c["w"] >= 0 else max(ql, tl)
    return any(max(0, r - ql + 1, (r - w + 1) >> 1) > min(tl - 1, r, (r + w) >> 1) for r in range(ql + tl - 1))


ADJACENCIES = ("small_after_large", "large_after_small", "cigar_after_score_only", "after_zdropped", "after_band_dropped", "empty_after_computed",
               "empty_after_empty", "global_after_lds", "lds_after_global", "wide_after_wide_other_T")


def adjacencies(cases, zdropped=None):
    """{class of ADJACENCIES: [(name before, name after)]} over the neighbours in plan_order(cases).  zdropped[i]: the recorded
    ez.zdropped of problem i; without it the model's, for the problems of at most 130 bases a side (the others count as not dropped).  A computed problem never follows an empty one: the plan gives an early return the work 0 and
    every computed problem at least 32, so the early returns close the one-wave launch -- what can stand between two problems is the
    hand-over to an early return and on from it, which the last two classes of the one-wave launch hold."""
    if zdropped is None:
        zdropped = [max(len(c["query"]), len(c["target"])) <= 130 and model_zdropped([c])[0] for c in cases]
    out = {k: [] for k in ADJACENCIES}
    for launch in plan_order(cases):
        for i, j in zip(launch, launch[1:]):
            a, b = cases[i], cases[j]
            ra, rb = route(a), route(b)
            sa, sb = (state_bytes(len(c["query"]), len(c["target"])) for c in (a, b))
            names = (a["name"], b["name"])

            def hit(k):
                out[k].append(names)
            if ra == ROUTE_NONE or rb == ROUTE_NONE:
                if rb == ROUTE_NONE:
                    hit("empty_after_empty" if ra == ROUTE_NONE else "empty_after_computed")
                continue
            if ra == rb == ROUTE_LDS and sa >= 4 * sb:
                hit("small_after_large")
            if ra == rb == ROUTE_LDS and sb >= 4 * sa and M.geometry(len(b["query"]), len(b["target"]), b["w"])[3] <= 32:
                hit("large_after_small")
            if a["flag"] & 1 and not b["flag"] & 1:
                hit("cigar_after_score_only")
            if zdropped[i]:
                hit("after_band_dropped" if band_runs_out(a) else "after_zdropped")
            if ra == ROUTE_LDS and rb == ROUTE_GLOBAL:
                hit("global_after_lds")
            if ra == ROUTE_GLOBAL and rb == ROUTE_LDS:
                hit("lds_after_global")
            if ra == rb == ROUTE_WIDE and (len(a["target"]) + 15) // 16 != (len(b["target"]) + 15) // 16:
                hit("wide_after_wide_other_T")
    return out


def interleave():
    """About 60 problems of the default scoring set from every route.  The hand-made ones are sized so that the order by falling work
    alternates routes, state sizes and flags; seeded small ones fill the gaps between them."""
    out = []

    def rel(name, ql, tl, **kw):
        q, t = pair("il_" + name, ql, tl)
        out.append(case("il_" + name, q, t, **kw))

    def unrel(name, head, q_tail, tl, **kw):
        q, t = head_tail("il_" + name, head, q_tail, tl)
        out.append(case("il_" + name, q, t, **kw))
    # one-wave launch, by falling work: LDS 748 176, global 354 496, LDS 191 680, global 176 000, LDS ...
    rel("lds_600x600", 600, 600, flag=0x40, zdrop=400)
    unrel("glob_40x5500", 40, 0, 5500)
    rel("lds_300x300_score", 300, 300, flag=0x01)
    rng = _rng("il_one")
    out.append(case("il_glob_1x5500", rand_seq(rng, 1), rand_seq(rng, 5500)))
    unrel("glob_zdrop_80x5470_w30", 60, 20, 5470, w=30, zdrop=20, flag=0x40)      # 266 352
    rel("lds_280x290", 280, 290, flag=0xc2, zdrop=200)
    unrel("glob_score_30x5460_w3", 30, 0, 5460, w=3, flag=0x01)                    # 175 648
    rel("lds_270x280_w200", 270, 280, w=200, flag=0x02)
    # small and large states around one another: 130 x 130 (41 440), 600 x 600 at w = 2 (38 368), 128 x 128 (36 720)
    rel("lds_130x130", 130, 130)
    rel("lds_600x600_w2", 600, 600, w=2)
    rel("lds_128x128_score", 128, 128, flag=0x01)
    rel("lds_600x610_w1_ext", 600, 610, w=1, flag=0x40, zdrop=100)                 # 38 688: between 130 x 130 and 600 x 600
    rel("lds_20x20", 20, 20)
    rel("lds_640x20", 640, 20, w=4)                                                # 659 * 32 = 21 088: a tall state among the small ones
    rel("lds_100x100", 100, 100, flag=0x08)
    # both ways out of the loop, each followed by a problem with a CIGAR
    unrel("zdrop_a", 40, 60, 110, zdrop=5, flag=0x40, w=100)
    unrel("zdrop_b", 50, 50, 105, zdrop=10, w=100)
    unrel("zdrop_c_score", 30, 70, 100, zdrop=5, flag=0x01, w=100)
    rel("band_out_a", 60, 120, w=3)
    rel("band_out_b", 110, 50, w=1, flag=0x40, zdrop=100)
    rel("band_out_c_score", 40, 125, w=5, flag=0x09)
    # early returns: the plan puts them behind every computed problem of the one-wave launch
    q, t = pair("il_empty", 30, 30)
    out += [case("il_empty_q", np.zeros(0), t), case("il_empty_t", q, np.zeros(0)), case("il_empty_both", np.zeros(0), np.zeros(0))]
    # several-wave launch: T differs between neighbours
    rel("wide_700x705", 700, 705, zdrop=400, flag=0x40)
    rel("wide_690x720_score", 690, 720, w=300, flag=0x01)
    rel("wide_100x1500", 100, 1500, w=60, zdrop=50, flag=0x40)
    out.append(case("il_wide_1x700", rand_seq(rng, 1), rand_seq(rng, 700)))
    rel("wide_3000x640_w8", 3000, 640, w=8, flag=0xc2, zdrop=100)
    rel("wide_2x690", 2, 690, flag=0x02)
    # seeded fill: small LDS problems with every flag of the fuzz batch, some dropped
    rng = np.random.default_rng(20241021)
    for k in range(60 - len(out)):
        ql, tl = int(rng.integers(1, 130)), int(rng.integers(1, 130))
        q = rand_seq(rng, ql)
        t = fit(rng, mutate(rng, q, max_indel=int(rng.integers(1, 20))), tl) if k % 3 else rand_seq(rng, tl)
        out.append(case(f"il_fill_{k:02d}", q, t, w=int(rng.choice(S.FUZZ_W)), zdrop=int(rng.choice(S.FUZZ_ZDROP)), end_bonus=int(rng.choice((-1, 0, 10))),
                        flag=int(rng.choice(S.FUZZ_FLAGS))))
    missing = [k for k, v in adjacencies(out).items() if not v]
    assert not missing, missing
    return out


def scenes():
    """{file name: problems of one call}."""
    out = {f"scoring_{cls}": scoring_cases(cls) for cls in SCORING}
    out["global_flags"] = global_flags()
    out["wide_small_sides"] = wide_small_sides()
    out["interleave"] = interleave()
    return out


# the routes each scene was built for
SCENE_ROUTES = {"global_flags": {ROUTE_GLOBAL}, "wide_small_sides": {ROUTE_WIDE}, "interleave": {ROUTE_NONE, ROUTE_LDS, ROUTE_GLOBAL, ROUTE_WIDE}}


def scene_routes(name):
    if name.startswith("scoring_"):
        return {ROUTE_NONE} if name[len("scoring_"):] in EARLY else {ROUTE_LDS}
    return SCENE_ROUTES[name]


def model_zdropped(cases):
    return [int(M.ksw_extd(c["query"], c["target"], *c["scoring"], c["w"], c["zdrop"], c["end_bonus"], c["flag"])[0][1]) for c in cases]


# ---- the class table: what the tier says it reaches, computed from the recorded inputs and answers
def _dropped_by(g, i):
    """"" (not dropped), "band" or "zdrop": a dropped problem that still drops without Z-drop left by its band (as make_ksw_golden.py tells)."""
    if not g["ez"][i, 1]:
        return ""
    if g["zdrop"][i] < 0:
        return "band"
    q = g["bases"][g["q_beg"][i]:g["q_beg"][i] + g["q_len"][i]]
    t = g["bases"][g["t_beg"][i]:g["t_beg"][i] + g["t_len"][i]]
    nz, _ = M.ksw_extd(q, t, *(int(x) for x in g["scoring"]), int(g["w"][i]), -1, int(g["end_bonus"][i]), int(g["flag"][i]))
    return "band" if nz[1] else "zdrop"


def class_table(files):
    """{class: [witnesses]} from {scene: the arrays of its golden file}.  A scoring class counts where the scene has a problem that ran to
    its last diagonal and one with a CIGAR (the early return: where every record is the reset one); a global or wide class where a
    problem of that route has the property."""
    out = {}

    def hit(k, name):
        out.setdefault(k, [])
        if name is not None:
            out[k].append(str(name))
    sc_classes = {
        "e2_zero": lambda a, b, q, e, q2, e2: e2 == 0,
        "long_thres_zero_e_eq_e2": lambda a, b, q, e, q2, e2: e == e2 and q != q2,
        "identical_gap_models": lambda a, b, q, e, q2, e2: (q, e) == (q2, e2),
        "e_lt_e2_negative_quotient": lambda a, b, q, e, q2, e2: e < e2 and q2 > q,
        "e_zero": lambda a, b, q, e, q2, e2: e == 0 or e2 == 0 and q2 + e2 >= q + e and 0 in (e, e2),
        "q_zero": lambda a, b, q, e, q2, e2: q == 0,
        "a_zero": lambda a, b, q, e, q2, e2: a == 0 and b > 0,
        "b_zero": lambda a, b, q, e, q2, e2: b == 0 and a > 0,
        "b_on_edge": lambda a, b, q, e, q2, e2: b == 2 * (q + e),
        "all_zero": lambda *v: max(v) == 0,
        "all_127": lambda *v: min(v) == 127,
        "first_sum_wraps": lambda a, b, q, e, q2, e2: q + e > 127,
        "only_second_sum_wraps": lambda a, b, q, e, q2, e2: q + e <= 127 < q2 + e2,
    }
    for k in list(sc_classes) + ["swap", "tie_sum_no_swap_first_cheaper_e", "tie_sum_no_swap_second_cheaper_e", "early_return_one_past_edge",
                                 "early_return_on_swapped_cost"]:
        hit(k, None)
    for scene, g in files.items():
        sc = tuple(int(x) for x in g["scoring"])
        routes = np.array([expected_route(int(q), int(t), sc) for q, t in zip(g["q_len"], g["t_len"])])
        if scene.startswith("scoring_"):
            a, b = sc[:2]
            q, e, q2, e2 = swapped(sc)
            if early(sc):
                if (g["ez"] == M.reset_ez().astype(np.int32)).all() and not g["cigar_off"][-1]:
                    if b == 2 * (q + e) + 1:
                        hit("early_return_one_past_edge", scene)
                    if (q, e) != sc[2:4]:
                        hit("early_return_on_swapped_cost", scene)
                continue
            if not ((g["ez"][:, 1] == 0).any() and (np.diff(g["cigar_off"]) > 0).any()):
                continue
            for k, f in sc_classes.items():
                if f(a, b, q, e, q2, e2):
                    hit(k, scene)
            if (q, e) != sc[2:4]:
                hit("swap", scene)
            if q + e == q2 + e2 and (q, e) != (q2, e2):
                hit("tie_sum_no_swap_first_cheaper_e" if e < e2 else "tie_sum_no_swap_second_cheaper_e", scene)
            continue
        for i, name in enumerate(g["name"]):
            ql, tl, flag, ez = int(g["q_len"][i]), int(g["t_len"][i]), int(g["flag"][i]), g["ez"][i]
            wild = 4 in g["bases"][g["q_beg"][i]:g["q_beg"][i] + ql] and 4 in g["bases"][g["t_beg"][i]:g["t_beg"][i] + tl]
            if routes[i] == ROUTE_GLOBAL and scene == "global_flags":
                hit(f"global_flag_{flag:02x}", name)
                by = _dropped_by(g, i)
                for k, yes in (("global_score_only", flag & 1), ("global_approx_max", flag & 8), ("global_right_alone", flag == 2),
                               ("global_zdrop_break", by == "zdrop"), ("global_band_runs_out", by == "band"), ("global_wildcards_both_sides", wild),
                               ("global_tie_first_differs", g["first_differs"][i]), ("global_long_query", ql >= 1000), ("global_one_base", ql == 1),
                               ("global_reach_end_1", not flag & 1 and ez[9] == 1), ("global_reach_end_0", flag & 0x40 and not flag & 1 and ez[9] == 0),
                               ("global_complete_narrow_band", not flag & 0x41 and not ez[1] and 0 <= g["w"][i] <= 100 and ez[8] > M.NEG_INF)):
                    hit(k, name if yes else None)
            if routes[i] == ROUTE_WIDE and scene == "wide_small_sides":
                for k, yes in (("wide_one_base", ql == 1), ("wide_two_bases", ql == 2), ("wide_short_target", tl <= 32), ("wide_score_only", flag & 1),
                               ("wide_approx_max", flag & 8)):
                    hit(k, name if yes else None)
        if scene == "global_flags":
            sizes = {state_bytes(int(q), int(t)) for q, t, r in zip(g["q_len"], g["t_len"], routes) if r == ROUTE_GLOBAL}
            hit("global_mixed_state_sizes_in_one_call", f"{len(sizes)} sizes" if len(sizes) > 2 and (routes == ROUTE_GLOBAL).sum() > 2 else None)
    return out
