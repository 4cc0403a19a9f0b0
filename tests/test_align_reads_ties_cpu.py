"""CPU proof of the tie tier of Device.align_reads: the order radix_sort_128x gives equal keys as tests/skeleton_model.py restates it
(sort_pairs) against the oracle's and the reference's; the tie goldens tests/golden/align_reads/ties_*.npz load, are the scenes of
tests/align_reads_shapes.py, reach every tie class and are reproduced by the loop over the CPU models.  Then what k_reads_finish and
k_reads_tied (csrc/reads/chaindp_reads.hip) compute per read -- the placed rank, the marks, the early return for at most one kept
record, the final rank -- restated in numpy and proved equal to every align_reads golden; and, rule by rule, a subtly wrong
restatement that gives the reference's words on the tie-free scenes and other words on a tie scene named beside it."""
import functools

import numpy as np
import pytest

import align_reads_shapes as RS
import oracle_lib as ol
import skeleton_model as K
import skeleton_shapes as SS
from test_skeleton_cpu import same

FILTERED, SOFT_DELETED, LIVE = 0, 1, 2                                     # a record's mark, as the kernel's RD_*


# ---------------------------------------------------------------- the order of equal keys

def test_sort_pairs_is_the_oracles_and_the_references_radix_sort():
    rng = np.random.default_rng(7)
    sizes = list(range(2, 70)) + [100, 129, 130, 131, 200, 257, 300]
    for n in sizes:
        for kind in ("bytes", "dp_max", "one_key"):
            if kind == "bytes":                                           # few distinct keys at a random byte
                x = rng.integers(0, 6, n).astype(np.uint64) << np.uint64(8 * int(rng.integers(0, 8)))
            elif kind == "dp_max":                                        # dp_max << 32 | hash, one hash: the upper passes fill one bucket
                x = (rng.integers(180, 180 + max(2, n // 8), n).astype(np.uint64) << np.uint64(32)) | np.uint64(0x1234567)
            else:
                x = np.full(n, 200 << 32 | 99, np.uint64)
            a = np.stack([x, np.arange(n, dtype=np.uint64)], 1).copy()    # y carries the index: the order of equal keys shows
            mine = np.array(K.sort_pairs([(int(k), int(i)) for k, i in a]), np.uint64).reshape(n, 2)
            b = a.copy()
            ol.oracle().co_radix_sort_128x(b.ctypes.data, b.ctypes.data + b.nbytes)
            assert np.array_equal(mine, b), (n, kind)
            if ol.have_ref():
                c = a.copy()
                ol.ref_cap().radix_sort_128x(c.ctypes.data, c.ctypes.data + c.nbytes)
                assert np.array_equal(mine, c), (n, kind)
            assert (len(set(x.tolist())) < n or n < 12) and mine[:, 0].tolist() == sorted(x.tolist())


def test_up_to_64_pairs_equal_keys_keep_their_order_and_past_64_they_need_not():
    pairs = [(5, i) for i in range(64)]
    assert K.sort_pairs(pairs) == pairs
    x = [(3 - i % 3) << 32 for i in range(130)]
    got = K.sort_pairs(list(zip(x, range(130))))
    assert [k for k, _ in got] == sorted(x) and any([i for k, i in got if k == key] != sorted(i for k, i in got if k == key) for key in set(x))


# ---------------------------------------------------------------- the goldens

def test_shapes_are_what_was_recorded():
    scenes = {s["name"]: RS.pack(s) for s in RS.tie_scenes()}
    assert sorted(scenes) == sorted(RS.TIE_NAMES)
    for name, p in scenes.items():
        g = RS.load(name)
        assert SS.squeezed(p), name
        for k, v in p.items():
            assert same(np.asarray(v), g[k]), (name, k)


def test_every_tie_class_is_reached_and_the_old_scenes_have_no_tie():
    reached = sum((RS.tie_classes(RS.load(n)) for n in RS.TIE_NAMES), start=RS.collections.Counter())
    assert not [k for k in RS.TIE_CLASSES + (RS.UNAIDED,) if not reached[k]], dict(reached)
    assert all(sum(RS.tie_classes(RS.load(n)).values()) == 0 for n in RS.NAMES)
    for n in RS.TIE_NAMES:
        RS.classes(RS.load(n))                                            # its assertion: the keys of a list past 64 do not rise
    g = RS.load("ties_unaided")                                           # no help: every input region's hash is its own
    assert all(len(set(g["regs"]["hash"][int(a):int(b)].tolist())) == b - a for a, b in zip(g["regs_off"], g["regs_off"][1:]))
    caps = {n: int(RS.load(n)["lds_cap"]) for n in RS.TIE_NAMES}
    assert caps == dict(ties_small=RS.RD_LDS_CAP, ties_64=RS.RD_LDS_CAP, ties_130=RS.RD_LDS_CAP, ties_cap=RS.SCENE_CAP, ties_unaided=RS.RD_LDS_CAP)


@functools.lru_cache(maxsize=None)
def model_of(name):
    """The loop over the CPU models on a golden's inputs, once a session."""
    g = RS.load(name)
    trace = []
    got = SS.check(g, trace)
    return g, got, len(trace)


@pytest.mark.parametrize("name", RS.TIE_NAMES)
def test_models_reproduce_the_reference(name):
    g, got, n_calls = model_of(name)
    for k in K.OUTPUTS:
        assert same(got[k], g[k + "_out"]), (name, k)
    assert n_calls == int(g["n_calls"])


# ---------------------------------------------------------------- the kernels' rule

def pool_of(placed):
    """A read's placed list as the host hands it to k_reads_finish: the records in pool order (round by round, then the inversion
    slots) with their place keys origin << 32 | born << 1 | is_inv (chaindp_reads_plan.h).  Returns (pool order as placed positions, keys)."""
    origin, born, keys = -1, 0, []
    for r in placed:
        inv, split_off = bool(int(r["bits"]) & K.BIT_INV), bool(int(r["bits"]) >> 9 & 1)
        if not inv:
            origin, born = (origin, born + 1) if split_off else (origin + 1, 0)
        keys.append((origin << 32 | born << 1 | int(inv), int(inv), born))
    order = sorted(range(len(placed)), key=lambda i: (keys[i][1], keys[i][2], i))
    return order, [keys[i][0] for i in order]


def marks(opt, qlen, regs, extra):
    out = []
    for r, x in zip(regs, extra):
        bits, cnt = int(r["bits"]), int(r["cnt"])
        flt = not bits & K.BIT_INV and not bits & K.BIT_SEG_SPLIT and cnt < opt["min_cnt"]
        if x["has_extra"]:
            clip = np.float32(qlen) * np.float32(1.0)
            if int(r["mlen"]) < opt["min_chain_score"] or int(x["dp_max"]) < opt["min_dp_max"]:
                flt = True
            elif np.float32(int(r["qs"])) > clip and np.float32(qlen - int(r["qe"])) > clip:
                flt = True
        out.append(FILTERED if flt else LIVE if bits & K.BIT_INV or cnt > 0 else SOFT_DELETED)
    return out


def by_counting(k2, at, first):
    """The ranks by counting over the places `at`: a record stands behind those with a larger key and, of those with its own, behind the
    ones first(q, p) names."""
    rank = {p: sum(k2[q] > k2[p] or (k2[q] == k2[p] and first(q, p)) for q in at) for p in at}
    out = [None] * len(at)
    for p, r in rank.items():
        out[r] = p
    return out


def by_radix(k2, at, top=64):
    return [p for _, p in K.sort_pairs([(k2[p], p) for p in at], top)][::-1]


def final_places(k2, mk, rule):
    """The places of a read's final regions, in final order."""
    n = len(k2)
    kept = sum(m != FILTERED for m in mk)
    live_from = SOFT_DELETED if kept <= 1 else LIVE                       # mm_hit_sort_by_dp returns at once when n <= 1
    at = [p for p in range(n) if mk[p] >= live_from]
    tied = len({k2[p] for p in at}) < len(at)
    later, earlier = (lambda q, p: q > p), (lambda q, p: q < p)
    if rule == "kernel":                                                  # k_reads_finish, and k_reads_tied for what it flags
        return by_radix(k2, at) if len(at) > 64 and tied else by_counting(k2, at, later)
    if rule == "ties_in_placed_order":                                    # the rule before this tier
        return by_counting(k2, at, earlier)
    if rule == "threshold_on_the_placed_length":
        return by_radix(k2, at, top=1) if n > 64 and tied else by_counting(k2, at, later)        # the byte passes over 64 records or fewer
    if rule == "stable_sort_past_64":                                     # a stable sort by falling key: placed order
        return by_counting(k2, at, earlier if len(at) > 64 else later)
    if rule == "reverse_placed_order_past_64":                            # the insertion sort's order at every length
        return by_counting(k2, at, later)
    if rule == "ties_ordered_before_the_squeeze":                         # the procedure over every placed record, the dropped ones taken out behind it
        if len(at) > 64 and tied:
            return [p for p in by_radix(k2, list(range(n))) if mk[p] >= live_from]
        return by_counting(k2, at, later)
    raise KeyError(rule)


def finish(name, rule="kernel"):
    """What the kernels make of a golden's reads under the rule: (placed, regs_off, regs) as the golden records them."""
    g, model, _ = model_of(name)
    opt = K.opt_dict(g["opt"])
    placed_all, final_all = [], []
    for rd in range(len(g["seq_off"]) - 1):
        p0, p1 = int(model["placed_off"][rd]), int(model["placed_off"][rd + 1])
        regs, extra = model["placed"][p0:p1], model["placed_extra"][p0:p1]
        order, keys = pool_of(regs)
        # the placed order by rank of the place key, over the records in pool order
        rank = [sum(kj < ki for kj in keys) for ki in keys]
        it = [None] * len(keys)
        for i, r in enumerate(rank):
            it[r] = order[i]
        assert sorted(it) == list(range(len(keys)))
        regs, extra = regs[it], extra[it]
        placed_all.append(regs)
        k2 = [int(x["dp_max"]) << 32 | int(r["hash"]) for r, x in zip(regs, extra)]
        mk = marks(opt, int(g["seq_off"][rd + 1] - g["seq_off"][rd]), regs, extra)
        final_all.append(regs[final_places(k2, mk, rule)] if len(regs) else regs)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, K.REG_DTYPE)
    return cat(placed_all), K.offsets([len(x) for x in final_all]), cat(final_all)


def equals_golden(name, rule):
    g = RS.load(name)
    placed, off, regs = finish(name, rule)
    assert same(placed, g["placed_out"]), (name, "placed")
    return same(off, g["regs_off_out"]) and same(regs, g["regs_out"])


@pytest.mark.parametrize("name", RS.NAMES + RS.TIE_NAMES)
def test_the_kernels_rule_gives_every_golden(name):
    assert equals_golden(name, "kernel")


WRONG = dict(ties_in_placed_order=RS.TIE_NAMES,                            # every tie scene shows it
             stable_sort_past_64=("ties_64", "ties_130", "ties_cap"),
             reverse_placed_order_past_64=("ties_130",),
             ties_ordered_before_the_squeeze=("ties_cap",))               # 70 live records of 73


@pytest.mark.parametrize("rule", sorted(WRONG))
def test_a_wrong_rule_gives_the_tie_free_goldens_and_misses_a_tie_scene(rule):
    for name in RS.NAMES:
        assert equals_golden(name, rule), (rule, name)
    for name in WRONG[rule]:
        assert not equals_golden(name, rule), (rule, name)


def test_what_some_wrong_rules_cannot_be_told_by():
    """Lists of up to 64 live records do not tell the rules past 64 apart, and a list past 64 whose keys are all equal is left where it
    stands by the in-place procedure: reversed, that is the insertion sort's order.  The threshold taken on the placed length cannot
    be told from the one on the live count by any list: the byte passes over up to 64 live records (67 and 66 placed in ties_64 and
    ties_cap) find them all in one bucket of the top byte, move none and sort that bucket by insertion."""
    for rule in ("stable_sort_past_64", "reverse_placed_order_past_64", "ties_ordered_before_the_squeeze"):
        assert equals_golden("ties_small", rule) and equals_golden("ties_unaided", rule), rule
    assert all(equals_golden(name, "threshold_on_the_placed_length") for name in RS.NAMES + RS.TIE_NAMES)
    rng = np.random.default_rng(3)
    for n in (2, 33, 63, 64):
        pairs = [(int(v) << 32 | 7, i) for i, v in enumerate(rng.integers(180, 190, n))]
        assert K.sort_pairs(pairs, top=1) == K.sort_pairs(pairs)
    pairs = [(int(v) << 32 | 7, i) for i, v in enumerate(rng.integers(180, 190, 65))]
    assert K.sort_pairs(pairs) != K.sort_pairs(pairs, top=65)            # one more, and the passes show
    g, model, _ = model_of("ties_64")
    rd = [str(n) for n in g["read_name"]].index("all_equal_70")
    f0, f1 = int(g["regs_off_out"][rd]), int(g["regs_off_out"][rd + 1])
    groups, pos = RS.tie_groups(g, rd)
    assert f1 - f0 == 70 and len(groups) == 1 and pos == list(range(70))[::-1]
