"""CPU tier: every input of tests/seed_edge_shapes.py sits on the edge it claims.  Each case goes through the restatement of
collect_seed_hits (oracle/seed_oracle.cpp, ol.SeedIndex.collect_seeds) and its `props` are checked against the anchors with a short
restatement of the ROUTING of csrc/chaindp_seed.hip only (route_model below: which kernel and layout takes a read, how many words a
thread of the radix sort holds, whether equal x are found, the bucket sizes of every pass, the small ranges a round produces, the
work items of k_seed_sort_huge, the width of the packed key) -- no sorting is restated.  Where oracle/_ref is built the anchors also
equal the unmodified reference's radix_sort_128x over the unsorted anchors, byte for byte.

The limits are the ones a 160 KB LDS gives (8192 / 13248, derived below from the kernel's own LDS formula, not measured) and the
turned-down settings of the GPU tier; tests/test_gpu_seed_edges.py reads the real ones from the device."""
import collections
import functools
import glob
import os

import numpy as np
import pytest

import oracle_lib as ol
import seed_edge_shapes as ss

needs_ref = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (build container only)")
LDS_LIMIT = 160 * 1024
TPB = 1024


# ---------------------------------------------------------------- the limits, from the formulas of chaindp_seed.hip / chaindp_abi_seed.cpp

def table_waves(workers):
    return 16 if workers >= 32 else 4


def small_slots(workers):
    return 1024 if workers >= 32 else 256


def sort_lds_bytes(max_n, workers):
    """seed_sort_lds_bytes"""
    return ((max_n * 10 + 7) & ~7) + table_waves(workers) * (768 * 2 + 256 * 4) + 2 * (max_n // 65 + 2 + small_slots(workers)) * 8 + 16 + ((max_n + 7) & ~7)


def limits_for(lds_limit, max_n_env=None, lab_cap_env=None):
    """What a context settles on when it first collects seeds (collect_seeds_impl)."""
    m, m2, cap = 8192, 65024, (lds_limit - 8192) & ~15
    if max_n_env:
        parts = max_n_env.split(",")
        m = min(m, int(parts[0]))
        if len(parts) > 1:
            m2 = int(parts[1])
    if lab_cap_env:
        cap = int(lab_cap_env) & ~15 if int(lab_cap_env) < cap else cap
    m, cap = max(m, 64), max(cap, 256)
    while m > 0 and sort_lds_bytes(m, 32) > lds_limit:
        m -= 512
    while m2 > m and sort_lds_bytes(m2, 4) > lds_limit:
        m2 -= 64
    return ss.Limits(m, m2, cap)


SETTINGS = {"default": (None, None), "pair": ("64,512", None), "huge": ("128,128", "1024")}          # CHAINDP_SEED_MAX_N, CHAINDP_SEED_LAB_CAP
LIMITS = {k: limits_for(LDS_LIMIT, *v) for k, v in SETTINGS.items()}


def radix_fits(L, n):
    """The condition under which k_seed_sort's first attempt is the radix sort: its tables fit behind the keys of the read's layout."""
    cap_n = L.max_n if n <= L.max_n else L.max_n2
    return -(-n // TPB) <= 13 and cap_n * 2 + table_waves(32 if n <= L.max_n else 4) * (1536 + 1024) >= 2 * 16 * TPB + 512


# ---------------------------------------------------------------- the routing, restated

def bit_length(v):
    return int(v).bit_length()


def kbits_of(x):
    """strand | id | position, as many bits as the read's largest id and position need (k_seed_sort's packed key)."""
    x = np.asarray(x, np.uint64)
    if not len(x):
        return 1
    return 1 + bit_length(np.bitwise_or.reduce(x >> np.uint64(32) & np.uint64(0x7fffffff))) + bit_length(np.bitwise_or.reduce(x & np.uint64(0xffffffff)))


def has_equal(x):
    return len(np.unique(x)) < len(x)


def buckets_of(x, sh):
    d = (x >> np.uint64(sh) & np.uint64(0xff)).astype(np.int64)
    vals, cnt = np.unique(d, return_counts=True)
    return d, vals.tolist(), cnt.tolist()


def lds_procedure(x, shift0, out):
    """The rounds of the reference's procedure in k_seed_sort over the multiset x (which element stands where does not matter for
    the sizes): per round the ranges of more than 64 anchors are split by their digit, buckets above 64 go round again, buckets of
    2..64 are the round's small ranges."""
    big = [(np.asarray(x, np.uint64), shift0)]
    while big:
        nxt, small = [], 0
        for arr, sh in big:
            if len(arr) <= 64:
                out["whole_isort"] += 1
                continue
            d, vals, cnt = buckets_of(arr, sh)
            out["levels"].append((sh, len(arr), len(vals)))
            nx = sh - 8 if sh > 8 else 0
            if len(vals) == 1:
                if sh:
                    nxt.append((arr, nx))
                continue
            out["buckets"][sh] += cnt
            if sh:
                for v, c in zip(vals, cnt):
                    if c > 64:
                        nxt.append((arr[d == v], nx))
                    elif c > 1:
                        small += 1
        out["small_per_round"].append(small)
        big = nxt


def route_model(x, L):
    """x: a read's anchors' x in the order of generation.  -> what the kernels do with it, as far as sizes decide."""
    x = np.asarray(x, np.uint64)
    n = len(x)
    out = dict(route=ss.lds_route(L, n), n=n, radix_items=-(-n // TPB), kbits=kbits_of(x), tied=has_equal(x), items=0, tied_units=0, levels=[],
               buckets=collections.defaultdict(list), small_per_round=[], whole_isort=0, global_ranges=0, restores=0, two_bucket_global=0,
               huge_levels=[], huge_buckets=collections.defaultdict(list), thread_sorted=[], item_sizes=[])
    if out["route"] in ("lds16", "lds4"):
        out["tied_units"] = int(out["tied"])
        if out["tied"]:
            lds_procedure(x, 56, out)
        if n and (x >> np.uint64(63)).min() != (x >> np.uint64(63)).max():                 # two strands: the closed form on the whole read
            mid = int((x >> np.uint64(63) == 0).sum())
            out["cycles"] = int((x[:mid] >> np.uint64(63)).sum())
            out["a_at_mid"], out["a_at_end"] = int(x[mid] >> np.uint64(63) == 0), int(x[-1] >> np.uint64(63) == 0)
    elif out["route"] == "huge":
        min_n, stack = ss.cap_of(L), [(x, 56)]
        while stack:
            arr, sh = stack.pop()
            g = len(arr) > L.lab_cap
            d, vals, cnt = buckets_of(arr, sh)
            nx = sh - 8 if sh > 8 else 0
            out["global_ranges"] += g
            out["huge_levels"].append((sh, len(arr), len(vals), g))
            if len(vals) == 1:
                out["restores"] += g
                if sh:
                    stack.append((arr, nx))
                continue
            out["two_bucket_global"] += int(g and len(vals) == 2)
            out["huge_buckets"][sh] += cnt
            if sh:
                for v, c in zip(vals, cnt):
                    if c > min_n:
                        stack.append((arr[d == v], nx))
                    elif c > 64:
                        out["items"] += 1
                        out["item_sizes"].append(c)
                        out["tied_units"] += int(has_equal(arr[d == v]))
                    elif c > 1:
                        out["thread_sorted"].append(c)
    return out


# ---------------------------------------------------------------- expected values, shared and never changed

def _offsets(parts):
    return np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)


def _cat(parts, empty):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else empty


@functools.lru_cache(maxsize=None)
def built(setting, name, *args):
    return getattr(ss, name)(LIMITS[setting] if isinstance(setting, str) else setting, *args)


def expect(case):
    """collect_seed_hits of every read by the restatement -> what the GPU must return for the batch."""
    n_reads = len(case.bid)
    with ol.SeedIndex(case.image) as oix:
        per = [oix.collect_seeds(case.flag, case.max_occ, int(case.bid[r]), int(case.qlen[r]), case.mini[case.mini_off[r]:case.mini_off[r + 1]])
               for r in range(n_reads)]
    a = [p[0] for p in per]
    mp = [p[2] for p in per]
    return dict(per=per, a_off=_offsets(a), anchors=_cat(a, np.zeros((0, 2), np.uint64)), rep_len=np.array([p[1] for p in per], np.int32),
                mp_off=_offsets(mp), mini_pos=_cat(mp, np.zeros(0, np.uint64)))


@functools.lru_cache(maxsize=None)
def expected(setting, name, *args):
    case, props = built(setting, name, *args)
    e = expect(case)
    e.update(case=case, props=props, L=LIMITS[setting] if isinstance(setting, str) else setting)
    return e


def _id(t):
    return "-".join(str(x) for x in t)


def sort_cases(setting):
    """(constructor, args) of the cases whose point is the sort, per limit setting."""
    if setting == "default":
        c = [("sorted_read", n, tie) for n in ss.RADIX_SIZES for tie in ss.TIES if tie is None or ss.tie_place(n, tie) is not None]
        c += [("layout_read", which, plus, tie) for which in ("max_n", "max_n2") for plus in (0, 1) for tie in (None, "end")]
        c += [("level_bucket", sh, size) for sh in (48, 40, 32, 16, 8, 0) for size in (64, 65)]
        c += [("whole_small_read", n) for n in (2, 64, 65)] + [("top_digits", k) for k in (1, 2, 3)]
        c += [("closed_form", 0), ("closed_form", 1), ("closed_form", 1, "mid"), ("closed_form", 1, "end"), ("closed_form", 64), ("closed_form", 65),
              ("closed_form", 65, "mid"), ("closed_form", 65, "end")]
        c += [("slot_overflow16", p) for p in (1024, 1025, 1030)] + [("slot_overflow4",), ("many_small", 2100)]
        return c + [("combined", "default")]
    if setting == "pair":
        return [("sorted_read", n, tie) for n in ss.PAIR_SIZES for tie in (None, "end")] + [("combined", "pair")]
    return ([("sorted_read", 129, None), ("sorted_read", 129, "end"), ("huge_level48", False), ("huge_level48", True)]
            + [("huge_range", plus, 2, tie) for plus in (0, 1, 2, 8) for tie in (False, True)] + [("huge_range", 1, 1, False), ("huge_range", 1, 1, True), ("huge_range", 0, 0, True), ("huge_range", 1, 0, True)]
            + [("huge_edge", 0, None), ("huge_edge", 0, "end"), ("huge_edge", 1, None), ("combined", "huge")])


SORT_CASES = [(s,) + c for s in SETTINGS for c in sort_cases(s)]
PROBE_CASES = ([("read_blocks", n) for n in sorted(ss.BLOCK_LAYOUTS)] + [("tandem_boundary", True), ("tandem_boundary", False), ("occ_edges",), ("rep_len_chunks",),
               ("scan_minis", 1024), ("scan_minis", 1025)] + [("skip_seed", f) for f in ss.SKIP_FLAGS])
SCAN_LARGE = 1024 * 1024 + 1


def models_of(e):
    """The routing of every read: from its anchors in the order of generation where the case records them, else from the restatement's
    (the sizes do not depend on the order)."""
    un = e["props"].get("unsorted", {})
    return [route_model(un[r][:, 0] if r in un else e["per"][r][0][:, 0], e["L"]) for r in range(len(e["case"].bid))]


# ---------------------------------------------------------------- the limits

def test_limits_of_a_160_kb_lds():
    d = LIMITS["default"]
    assert d == ss.Limits(8192, 13248, LDS_LIMIT - 8192)
    assert sort_lds_bytes(d.max_n2, 4) <= LDS_LIMIT < sort_lds_bytes(d.max_n2 + 64, 4)
    assert d.max_n <= d.max_n2 <= 13312 < 16384                 # the 14-bit place field; "no field passes 13 312" in seed_radix_words
    assert LIMITS["pair"][:2] == (64, 512) and LIMITS["huge"] == ss.Limits(128, 128, 1024)
    # every read of the default setting is radix-sorted; under 64,512 the tables do not fit behind the keys of the four-wave layout
    assert all(radix_fits(d, n) for n in (1, 8192, 8193, 13248))
    p = LIMITS["pair"]
    assert radix_fits(p, 64) and not any(radix_fits(p, n) for n in ss.PAIR_SIZES)
    assert all(p.max_n < n <= p.max_n2 for n in ss.PAIR_SIZES)


# ---------------------------------------------------------------- the sort's cases: one check per constructor
# check(m, claims, L, args, x): m = route_model of the constructor's (first) read, claims = what the constructor said beside n and
# tied_pairs, x = the read's sorted x.  The same checks run on the case alone and on its reads inside the combined batch.

def check_sorted_read(m, claims, L, args, x):
    n, tie = args[0], args[1] if len(args) > 1 else None
    assert claims["route"] == m["route"] and claims["radix_items"] == m["radix_items"] == -(-n // TPB) and m["n"] == n
    tp = ss.tie_place(n, tie)
    assert tp is None or x[tp] == x[tp + 1]
    if m["route"] in ("lds16", "lds4"):
        assert radix_fits(L, n) == (L.max_n2 >= 8192 or n <= L.max_n)           # the pair network takes the four-wave reads of a small max_n2
    if ss.cap_of(L) == 128 and n == 129:                                         # 65 forward (an item), 64 reverse (sorted by their thread)
        assert m["huge_buckets"][56] == [65, 64] and m["items"] == 1 and m["thread_sorted"] == [64]


def check_layout_read(m, claims, L, args, x):
    which, plus = args[:2]
    check_sorted_read(m, claims, L, (getattr(L, which) + plus,) + tuple(args[2:]), x)
    assert m["route"] == {("max_n", 0): "lds16", ("max_n", 1): "lds4", ("max_n2", 0): "lds4", ("max_n2", 1): "huge"}[(which, plus)]
    assert (m["items"] >= 1 and max(m["item_sizes"]) > 64) if m["route"] == "huge" else m["items"] == 0


def check_huge_edge(m, claims, L, args, x):
    check_sorted_read(m, claims, L, (ss.HUGE_STACK * ss.cap_of(L) + args[0],) + tuple(args[1:]), x)
    assert m["route"] == ("huge", "big")[args[0]]


def check_level_bucket(m, claims, L, args, x):
    sh, size = args
    assert m["buckets"][sh].count(size) == 1 and max(m["buckets"][sh]) == size
    assert all(lv[2] == 1 for lv in m["levels"] if lv[0] > sh) and m["levels"][0][:2] == (56, 200)
    down = [lv for lv in m["levels"] if lv[1] == size and lv[0] < sh]                 # the bucket as a range of the levels below
    assert (len(down) > 0 and down[0][0] == (sh - 8 if sh > 8 else 0)) == (size == 65 and sh > 0) and (down == [] or size == 65)
    inside = x[(x >> np.uint64(sh)) == (np.uint64(ss.anchor_x(0x050505, 0x050505)) >> np.uint64(sh))] if sh else x[x == np.uint64(ss.anchor_x(0x050505, 0x050505))]
    assert len(inside) == size and has_equal(inside)                                  # the ties are inside the bucket


def check_whole_small_read(m, claims, L, args, x):
    assert m["whole_isort"] == (1 if args[0] <= 64 else 0) and m["tied"]


def check_top_digits(m, claims, L, args, x):
    first = [lv for lv in m["levels"] if lv[2] > 1][0]
    assert first[2] == {1: 9, 2: 2, 3: 3}[args[0]] and first[0] == {1: 8, 2: 56, 3: 48}[args[0]]


def check_closed_form(m, claims, L, args, x):
    assert m["levels"][0] == (56, 200, 2)
    assert (m["cycles"], m["a_at_mid"], m["a_at_end"]) == (claims["cycles"], claims["a_at_mid"], claims["a_at_end"])


def check_slot_overflow(m, claims, L, args, x):
    assert m["route"] == ("lds16" if claims["slots"] == 1024 else "lds4") and small_slots(32 if m["route"] == "lds16" else 4) == claims["slots"]
    assert max(m["small_per_round"]) == claims["small_ranges_in_a_round"] and sorted(m["small_per_round"])[-2] == 0      # no other round has any
    if claims["slots"] == 1024:
        assert len(m["buckets"][40]) == 5 and min(m["buckets"][40]) > 64


def check_huge_level48(m, claims, L, args, x):
    cap = ss.cap_of(L)
    assert m["huge_buckets"][48] == [64, 65, cap, cap + 1] and m["huge_buckets"][40] == [cap - 64, 65]
    assert m["items"] == claims["items"] == 3 and sorted(m["item_sizes"]) == [65, 65, cap] and m["tied_units"] == claims["tied_units"]
    assert sorted(m["thread_sorted"]) == [64, cap - 64] and m["global_ranges"] == 0


def check_huge_range(m, claims, L, args, x):
    plus, strands, tie = args
    assert m["n"] == L.lab_cap + plus and bool(m["global_ranges"]) == bool(claims["global_digits"]) == (plus > 0)
    if strands == 0:                                                             # all eight levels are one bucket; nothing is handed on
        assert m["restores"] == (8 if plus > 0 else 0) and [lv[2] for lv in m["huge_levels"]] == [1] * 8 and m["items"] == 0 and m["thread_sorted"] == []
    elif strands == 1:                                                           # every level from the strand to byte 2 is one bucket over global digits
        assert m["restores"] == 6 and [lv[2] for lv in m["huge_levels"][:7]] == [1] * 6 + [13 - int(tie)]
    elif plus > 0:
        assert m["two_bucket_global"] == 1 and m["huge_levels"][0][2] == 2 and m["restores"] == 0


def check_nothing_more(m, claims, L, args, x):
    pass


CHECKS = dict(sorted_read=check_sorted_read, layout_read=check_layout_read, huge_edge=check_huge_edge, level_bucket=check_level_bucket,
              whole_small_read=check_whole_small_read, top_digits=check_top_digits, closed_form=check_closed_form, slot_overflow16=check_slot_overflow,
              slot_overflow4=check_slot_overflow, huge_level48=check_huge_level48, huge_range=check_huge_range, many_small=check_nothing_more)
GRID, GRID_TIED = 256 * 8, 256                                                   # workgroups of k_seed_sort's first and second launch


def check_every_read(e, models):
    """n, neighbour ties, the multiset before the sort, tied or not, the key width: for every read that claims them."""
    props = e["props"]
    assert [n for n in props["n"] if n is not None] == [m["n"] for m, n in zip(models, props["n"]) if n is not None]
    assert np.diff(e["a_off"]).tolist() == [m["n"] for m in models]
    for r, (a, rl, mp) in enumerate(e["per"]):
        x = a[:, 0]
        assert len(x) < 2 or (x[1:] >= x[:-1]).all()
        assert models[r]["kbits"] <= 43
        if props["tied_pairs"][r] is None:
            continue
        assert int((x[1:] == x[:-1]).sum()) == props["tied_pairs"][r], (r, "neighbour ties")
        u = props["unsorted"][r]                                                 # the same anchors, before the sort
        assert np.array_equal(u[np.lexsort((u[:, 1], u[:, 0]))], a[np.lexsort((a[:, 1], a[:, 0]))]), (r, "multiset")
        assert len(np.unique(a, axis=0)) == len(a), (r, "equal x are told apart by y")
        assert models[r]["tied"] == (props["tied_pairs"][r] > 0)


@pytest.mark.parametrize("shape", SORT_CASES, ids=_id)
def test_sort_case_sits_on_its_edge(shape):
    e = expected(*shape)
    props, L, name, args = e["props"], e["L"], shape[1], shape[2:]
    models = models_of(e)
    check_every_read(e, models)
    if name != "combined":
        CHECKS[name](models[0], props, L, args, e["per"][0][0][:, 0])
        if name == "many_small":
            assert len(models) > GRID and sum(m["tied_units"] for m in models) > 4 * GRID_TIED
        return
    # the combined batch: every constructor's claim holds for its reads where they stand now
    assert [(p[0],) + p[1] for p in props["parts"]] == ss.small_cases(L, args[0]) and sum(p[3] for p in props["parts"]) == len(models)
    for pname, pargs, first, count, claims in props["parts"]:
        if pname in CHECKS:
            CHECKS[pname](models[first], claims, L, pargs, e["per"][first][0][:, 0])
    tied = [r for r, m in enumerate(models) if m["tied"]]
    assert tied[0] == 0 and tied[-1] == len(models) - 1
    flips = sum(1 for r in range(1, len(models)) if models[r]["tied"] != models[r - 1]["tied"])
    assert flips >= 20                                                           # tied and tie-free reads alternate
    units, tied_units = len(models) + sum(m["items"] for m in models), sum(m["tied_units"] for m in models)
    assert tied_units > 20
    if args[0] == "default":
        assert units > GRID and tied_units > GRID_TIED                           # workgroups of both launches go on to further units
        part = {p[0]: p for p in props["parts"]}
        assert (int(e["case"].mini_off[part["tandem_boundary"][2] + 1])) % 256 == 0      # its read boundary is still on a block edge
        assert int(e["a_off"][-1]) < 1 << 16 and any(m["n"] == 0 for m in models)            # reads without anchors among them
    if args[0] == "huge":
        assert sum(1 for m in models if m["items"]) >= 10                        # work items from many reads in one list


@needs_ref
@pytest.mark.parametrize("shape", SORT_CASES, ids=_id)
def test_sort_case_expected_values_are_the_references(shape):
    e = expected(*shape)
    for r, u in e["props"]["unsorted"].items():
        b = np.ascontiguousarray(u).copy()
        ol.ref_cap().radix_sort_128x(b.ctypes.data, b.ctypes.data + b.nbytes)
        assert b.tobytes() == np.ascontiguousarray(e["per"][r][0]).tobytes(), (shape, r)


# ---------------------------------------------------------------- probe, expand and reads kernels

def test_read_blocks():
    for n in ss.BLOCK_LAYOUTS:
        e = expected("default", "read_blocks", n)
        c = e["case"]
        per = np.diff(c.mini_off).tolist()
        assert per == e["props"]["per_read"] and c.mini_off[-1] == n and len(c.bid) > 0
        assert per[0] == 0 and per[-1] == 0
        if n >= 256:
            assert 256 in c.mini_off.tolist() and per[1] == 256
        if n == 600:
            assert 512 in c.mini_off.tolist() and max(np.diff(np.flatnonzero(np.diff(c.mini_off)))) >= 7        # seven empty reads inside one block
        assert (e["a_off"][-1] > 0) == (n > 0) and np.array_equal(e["mp_off"], c.mini_off)                    # every minimizer is used


def tandem_anchors(e):
    return int((e["anchors"][:, 1] & np.uint64(ss.TANDEM_BIT) != 0).sum())


def tandem_minimizers(case, across_reads):
    """The minimizers equal to a neighbour -- of the same read, or (wrong) of the batch."""
    m = case.mini[:, 0] >> np.uint64(8)
    out = []
    for r in range(len(case.bid)):
        lo, hi = (0, len(m)) if across_reads else (int(case.mini_off[r]), int(case.mini_off[r + 1]))
        out += [i for i in range(int(case.mini_off[r]), int(case.mini_off[r + 1])) if (i > lo and m[i] == m[i - 1]) or (i + 1 < hi and m[i] == m[i + 1])]
    return out


def tandem_count(e, across_reads):
    """Anchors that get the tandem bit: the hits of those minimizers (counted by looking each up alone)."""
    case = e["case"]
    with ol.SeedIndex(case.image) as oix:
        return sum(len(oix.collect_seeds(0, 64, 0, 9000, case.mini[i:i + 1])[0]) for i in tandem_minimizers(case, across_reads))


def test_tandem_boundary():
    for across in (True, False):
        e = expected("default", "tandem_boundary", across)
        c = e["case"]
        assert (256 in c.mini_off.tolist()) == across and c.mini[255, 0] >> np.uint64(8) == c.mini[256, 0] >> np.uint64(8)
        assert len(tandem_minimizers(c, False)) == e["props"]["tandem_minis"] and len(tandem_minimizers(c, True)) == 4
        assert tandem_anchors(e) == tandem_count(e, False) > 0


def test_occ_edges():
    e = expected("default", "occ_edges")
    c, props = e["case"], e["props"]
    assert props["collisions"] == [0, 1, 2] and c.max_occ == 8
    used = [h for h in props["hits"] if h < 8]
    assert sorted(set(props["hits"])) == [0, 1, 2, 3, 7, 8, 9]
    assert len(e["per"][0][0]) == sum(used) and len(e["per"][0][2]) == len(used)          # t == 7 is used, t == 8 is not; t == 0 has a mini_pos entry
    assert e["rep_len"][0] > 0


def test_rep_len_chunks():
    e = expected("default", "rep_len_chunks")
    c, props = e["case"], e["props"]
    r = props["read"]
    b0 = int(c.mini_off[r])
    assert b0 == 10 and b0 % 64 != 0
    sk = props["skipped"]
    lanes = sorted((i // 64, i % 64) for i in sk)
    assert {(0, 63), (1, 0), (6, 63), (7, 0), (0, 0)} <= set(lanes) and not any(ch in (2, 3, 5) for ch, _ in lanes)
    assert sk[0][0] < 0 and sk[65][0] == sk[64][1] and sk[66][0] == sk[65][1] + 1 and sk[64][0] > sk[63][1]
    want, en_prev = 0, 0
    for i in sorted(sk):                                                         # map.c:127-133 as one term per skipped minimizer
        st, en = sk[i]
        want += en - st if st > en_prev else en - en_prev
        en_prev = en
    assert e["rep_len"][r] == want and e["rep_len"][r - 1] == 0 and e["rep_len"][r + 1] == 0
    assert len(e["per"][r][2]) == int(c.mini_off[r + 1]) - b0 - len(sk)


def test_scan_minis():
    for n in (1024, 1025):
        e = expected("default", "scan_minis", n)
        assert e["case"].mini_off[-1] == n and e["props"]["tiles"] == -(-n // 1024) == (1, 2)[n - 1024]
        assert e["a_off"][-1] > n                                                # more than one anchor a minimizer: both scans carry across the tile
    case, props = built("default", "scan_minis", SCAN_LARGE)
    tiles = -(-SCAN_LARGE // 1024)
    assert props["tiles"] == tiles == 1025 and -(-tiles // 1024) == 2 and -(-(tiles - 1) // 1024) == 1     # k_scan_l2's tiles per thread
    assert case.mini.nbytes == 16 * SCAN_LARGE and np.diff(case.mini_off).max() == 4096 and case.mini_off[-1] == SCAN_LARGE
    assert (case.mini[:, 0] >> np.uint64(8)).min() >= ss.ABSENT


def test_skip_seed():
    seen = {}
    for flag in ss.SKIP_FLAGS:
        e = expected("default", "skip_seed", flag)
        c = e["case"]
        seen[flag] = np.diff(e["a_off"]).tolist()
        n_self = int((e["anchors"][:, 1] & np.uint64(ss.SELF_BIT) != 0).sum())
        assert (n_self > 0) == bool(flag & ss.F_NO_DIAG)
        assert e["props"]["block_opens"] == bool(flag & 1)
        y = e["per"][-1][0][:, 1] & np.uint64(0xffffffff)                          # the read of 5 bases: the reverse-strand positions wrapped
        if not flag & ss.F_FOR_ONLY:
            assert (y > np.uint64(1 << 31)).any()
    full = 25
    assert seen[ss.F_NO_DUAL] == [full] * 6 + [12]                               # flag 2 alone: the block opens on bit 0 only, nothing is skipped
    assert seen[ss.F_NO_DIAG][0] == full and seen[ss.F_NO_DIAG][1] < full        # equal id needs bit 31 to count as the same sequence
    d = seen[ss.F_NO_DIAG | ss.F_NO_DUAL]
    assert len(set(d[:6])) >= 4                                                  # bid below / equal / above the hit's id, with and without bit 31
    assert seen[ss.F_FOR_ONLY][0] < full and seen[ss.F_REV_ONLY][0] < full and seen[ss.F_FOR_ONLY][0] + seen[ss.F_REV_ONLY][0] == full


@pytest.mark.parametrize("shape", PROBE_CASES, ids=_id)
def test_probe_case_offsets(shape):
    e = expected("default", *shape)
    assert len(e["a_off"]) == len(e["case"].bid) + 1 == len(e["mp_off"]) and len(e["rep_len"]) == len(e["case"].bid)


# ---------------------------------------------------------------- the key width

def test_packed_key_is_never_wider_than_43_bits():
    """k_seed_expand builds x from a 21-bit id and a 21-bit position (and the strand), so the key of k_seed_sort's first attempt has
    kbits = 1 + rbits + pbits <= 43 and kbits + 14 > 64 is never true: with try_network set, packed_state 2 cannot be reached, and the
    16-bit-index bitonic network under `packed_state == 2 && try_network` runs for no image.  Checked over every case of this tier
    and the recorded fixtures."""
    widest = 0
    for shape in SORT_CASES:
        widest = max([widest] + [m["kbits"] for m in models_of(expected(*shape))])
    for shape in PROBE_CASES:
        e = expected("default", *shape)
        widest = max([widest] + [kbits_of(p[0][:, 0]) for p in e["per"]])
    paths = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seeds", "*.npz")))
    assert len(paths) == 8
    for path in paths:
        g = np.load(path, allow_pickle=False)
        off = g["a_off"]
        widest = max([widest] + [kbits_of(g["anchors"][off[r]:off[r + 1], 0]) for r in range(len(off) - 1)])
    assert 24 <= widest <= 43
    assert kbits_of(np.array([ss.anchor_x((1 << 21) - 1, (1 << 21) - 1, 1)], np.uint64)) == 43       # the widest an image can give


# ---------------------------------------------------------------- restatements that are wrong only above an edge

def verdict(edge, lower_same, upper_differs):
    assert lower_same, (edge, "the wrong restatement differs below the edge")
    assert upper_differs, (edge, "the case above the edge does not tell the wrong restatement from the right one")


def stable_sort(u):
    """The insertion sort of ksort.h:107-117 on a whole read: stable."""
    return u[np.argsort(u[:, 0], kind="stable")]


def test_insertion_sort_wrong_at_65():
    res = {}
    for n in (64, 65):
        e = expected("default", "whole_small_read", n)
        res[n] = np.array_equal(stable_sort(e["props"]["unsorted"][0]), e["per"][0][0])
    verdict("a whole read of 64 / 65 anchors: insertion sort / radix passes", res[64], not res[65])


def test_unstable_order_wrong_with_ties():
    res = {}
    for tie in (None, "mid"):
        e = expected("default", "sorted_read", 1025, tie)
        u = e["props"]["unsorted"][0]
        res[tie] = np.array_equal(u[np.lexsort((-u[:, 1].astype(np.int64), u[:, 0]))], e["per"][0][0])       # equal x by descending y
    verdict("no tie / one tie at places (1023, 1024): any order of equal x", res[None], not res["mid"])


def test_tandem_wrong_across_a_read_boundary():
    res = {}
    for across in (False, True):
        e = expected("default", "tandem_boundary", across)
        res[across] = tandem_count(e, True) == tandem_anchors(e)
    verdict("equal minimizers inside a read / on both sides of a read boundary: tandem", res[False], not res[True])
