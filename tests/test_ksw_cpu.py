"""CPU tier of the alignment (chaindp_ksw_extd): the numpy restatement tests/ksw_model.py against the reference's recorded answers
(tests/golden/ksw/*.npz), the two traps proven by the model's variants, the fixtures against tests/ksw_shapes.py, the header through
_cabi.py, the routing constants, and the table of argument refusals."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import ksw_model as M
import ksw_shapes as S
from conftest import GOLDEN_DIR, ROOT

KSW_DIR = os.path.join(GOLDEN_DIR, "ksw")
FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(KSW_DIR, "*.npz")))


def load(name):
    z = np.load(os.path.join(KSW_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def problem(g, i):
    q = g["bases"][g["q_beg"][i]:g["q_beg"][i] + g["q_len"][i]]
    t = g["bases"][g["t_beg"][i]:g["t_beg"][i] + g["t_len"][i]]
    return (q, t, *(int(x) for x in g["scoring"]), int(g["w"][i]), int(g["zdrop"][i]), int(g["end_bonus"][i]), int(g["flag"][i]))


def answer(g, i):
    return g["ez"][i], g["cigar"][g["cigar_off"][i]:g["cigar_off"][i + 1]]


def test_fixtures_are_there():
    assert FILES == sorted([f"named_{k}" for k in S.SCORING] + [f"fuzz_{k}" for k in M.SCORING]), FILES
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(KSW_DIR, "*.npz"))) < 1 << 20


@pytest.mark.parametrize("name", FILES)
def test_model_equals_every_golden_record(name):
    g = load(name)
    for i in range(len(g["name"])):
        ez, cig = M.ksw_extd(*problem(g, i))
        wez, wcig = answer(g, i)
        assert np.array_equal(ez, wez) and np.array_equal(cig, wcig), (str(g["name"][i]), ez.tolist(), wez.tolist())


@pytest.mark.parametrize("variant", ("clean", "first"))
def test_variant_differs_where_the_generator_said(variant):
    """Out-of-band cells reset ("clean") and the first maximum as max_t ("first") are not what the reference computes."""
    n_differ = 0
    for name in FILES:
        g = load(name)
        marked = np.flatnonzero(g[variant + "_differs"])
        for i in marked:
            ez, cig = M.ksw_extd(*problem(g, i), variant=variant)
            wez, wcig = answer(g, i)
            assert not (np.array_equal(ez, wez) and np.array_equal(cig, wcig)), (variant, str(g["name"][i]))
        n_differ += len(marked)
        for i in np.flatnonzero(~g[variant + "_differs"])[:20]:           # ... and a sample of the others agrees
            ez, cig = M.ksw_extd(*problem(g, i), variant=variant)
            wez, wcig = answer(g, i)
            assert np.array_equal(ez, wez) and np.array_equal(cig, wcig), (variant, str(g["name"][i]))
    assert n_differ >= 1


def test_fixtures_hold_the_named_shapes():
    for sc, group in S.groups(S.named_cases()).items():
        g, p = load(f"named_{sc}"), S.pack(group)
        assert [str(x) for x in g["name"]] == [c["name"] for c in group]
        assert tuple(int(x) for x in g["scoring"]) == S.SCORING[sc]
        for k, v in p.items():
            assert np.array_equal(g[k], v), (sc, k)


def test_fixtures_hold_the_fuzz_batch():
    for sc, group in S.groups(S.fuzz_cases()).items():
        g, p = load(f"fuzz_{sc}"), S.pack(group)
        for k, v in p.items():
            assert np.array_equal(g[k], v), (sc, k)


def test_fixtures_cover_what_the_issue_lists():
    flags, reach, zdropped, routes = set(), set(), 0, set()
    for name in FILES:
        g = load(name)
        sc = tuple(int(x) for x in g["scoring"])
        r = np.array([S.expected_route(int(q), int(t), sc) for q, t in zip(g["q_len"], g["t_len"])])
        flags |= set(g["flag"][r != S.ROUTE_NONE].tolist())
        reach |= set(g["ez"][(r != S.ROUTE_NONE) & (g["flag"] & 1 == 0), 9].tolist())
        zdropped += int(g["ez"][:, 1].sum())
        routes |= set(r.tolist())
    assert flags >= set(S.FLAG_COMBOS) and reach == {0, 1} and zdropped > 0
    assert routes == {S.ROUTE_NONE, S.ROUTE_LDS, S.ROUTE_GLOBAL, S.ROUTE_WIDE}


def test_header_binds_through_cabi():
    from minimap2_chaindp_amd import _cabi, chaindp
    protos = _cabi.prototypes("chaindp_ksw.h")
    assert list(protos) == ["chaindp_ksw_extd", "chaindp_ksw_debug_routing", "chaindp_ksw_debug_route", "chaindp_ksw_debug_set_grid_cap",
                            "chaindp_ksw_debug_launch", "chaindp_ksw_debug_ms"]
    assert chaindp.KSW_SYMBOLS == tuple(protos)
    restype, argtypes = protos["chaindp_ksw_extd"]
    assert restype is C.c_int and len(argtypes) == 21
    assert argtypes[1] is C.c_int64 and argtypes[-1] is C.c_int64 and argtypes[7:13] == [C.c_int] * 6
    assert all(t is C.c_void_p for k, t in enumerate(argtypes) if k not in (1, 7, 8, 9, 10, 11, 12, 20))
    with open(os.path.join(ROOT, "include", "chaindp.h")) as f:
        assert '#include "chaindp_ksw.h"' in f.read()                     # chaindp.h brings it along, as it does chaindp_gaps.h
    fn = chaindp.lib().chaindp_ksw_extd                                       # exported, and bound with that prototype
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert chaindp.lib().chaindp_ksw_extd(None, 0, *([None] * 5), 2, 4, 4, 2, 24, 1, *([None] * 7), 0) == S.ERR_ARG      # no context


def test_routing_constants_are_the_librarys():
    from minimap2_chaindp_amd import chaindp
    assert chaindp.ksw_routing() == dict(lds_budget=S.LDS_BUDGET, per_target=S.PER_TARGET, per_query=S.PER_QUERY, fixed=S.FIXED,
                                         wide_bytes=S.WIDE_BYTES, wide_waves=S.WIDE_WAVES)
    names = [c["name"] for c in S.named_cases()]
    for what, limit in (("wide", S.WIDE_BYTES), ("lds", S.LDS_BUDGET)):        # a problem on, below and above each constant
        sizes = {tag: next(n for n in names if n.startswith(f"route_{what}_{tag}_")).rsplit("_", 1)[1].split("x") for tag in ("below", "on", "above")}
        need = {tag: S.state_bytes(int(q), int(t)) for tag, (q, t) in sizes.items()}
        assert need["below"] == limit - 16 and need["on"] == limit and need["above"] == limit + 16, (what, need)


def test_refusal_table():
    """Every row changes a valid call into one the C call refuses with CHAINDP_ERR_ARG (tests/test_gpu_ksw.py makes the calls); the flag
    rows carry a bit outside the accepted ones, which the model refuses too."""
    base = S.refusal_base_call()
    assert len({r[0] for r in S.REFUSALS}) == len(S.REFUSALS) >= 15
    for name, change, code in S.REFUSALS:
        assert code == S.ERR_ARG and set(change) <= set(base), name
        if "flag" in change:
            assert any(f & ~M.ACCEPTED_FLAGS for f in change["flag"]), name
            bad = next(f for f in change["flag"] if f & ~M.ACCEPTED_FLAGS)
            with pytest.raises(AssertionError):
                M.ksw_extd(base["bases"][:10], base["bases"][10:20], *base["scoring"], -1, 400, -1, bad)
        if "scoring" in change:
            assert any(not 0 <= v <= 127 for v in change["scoring"]), name
        if "bases" in change:
            assert change["bases"](base["bases"]).max() > 4, name
    assert M.ACCEPTED_FLAGS == 0xcb
