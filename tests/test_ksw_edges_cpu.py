"""CPU tier of the extension alignment's edge scenes (tests/ksw_edge_shapes.py): the model against the reference's recorded answers
(tests/golden/ksw_edges/*.npz, made by tests/golden/make_ksw_edge_golden.py from the unmodified reference), the scenes against the recorded
inputs, the routes each scene was built for, the table of classes computed from inputs and answers, the neighbours of `interleave` in
the plan's order, and the two test hooks through _cabi."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import ksw_edge_shapes as E
import ksw_model as M
import ksw_shapes as S
from conftest import GOLDEN_DIR
from test_ksw_cpu import answer, problem

EDGE_DIR = os.path.join(GOLDEN_DIR, "ksw_edges")
FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(EDGE_DIR, "*.npz")))
SCENES = sorted([f"scoring_{k}" for k in E.SCORING] + ["global_flags", "wide_small_sides", "interleave"])
# every class the tier names; class_table() fills each from the recorded inputs and answers
CLASSES = ("e2_zero", "long_thres_zero_e_eq_e2", "identical_gap_models", "e_lt_e2_negative_quotient", "e_zero", "q_zero", "a_zero", "b_zero", "b_on_edge",
           "all_zero", "all_127", "first_sum_wraps", "only_second_sum_wraps", "swap", "tie_sum_no_swap_first_cheaper_e", "tie_sum_no_swap_second_cheaper_e",
           "early_return_one_past_edge", "early_return_on_swapped_cost",
           *(f"global_flag_{f:02x}" for f in E.FLAGS8), "global_score_only", "global_approx_max", "global_right_alone", "global_zdrop_break",
           "global_band_runs_out", "global_wildcards_both_sides", "global_tie_first_differs", "global_long_query", "global_one_base", "global_reach_end_1",
           "global_reach_end_0", "global_complete_narrow_band", "global_mixed_state_sizes_in_one_call",
           "wide_one_base", "wide_two_bases", "wide_short_target", "wide_score_only", "wide_approx_max")


def load(name):
    z = np.load(os.path.join(EDGE_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def files():
    return {name: load(name) for name in FILES}


def test_fixtures_are_there_and_small():
    assert FILES == SCENES
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(EDGE_DIR, "*"))) < 1 << 20


@pytest.mark.parametrize("name", SCENES)
def test_model_equals_every_record(files, name):
    g = files[name]
    for i in range(len(g["name"])):
        ez, cig = M.ksw_extd(*problem(g, i))
        wez, wcig = answer(g, i)
        assert np.array_equal(ez, wez) and np.array_equal(cig, wcig), (str(g["name"][i]), ez.tolist(), wez.tolist())


def test_shapes_are_what_was_recorded(files):
    """The goldens' inputs are the scenes of ksw_edge_shapes (seeded): a change there needs the goldens made again."""
    scenes = E.scenes()
    assert sorted(scenes) == SCENES
    for name, cases in scenes.items():
        g = files[name]
        assert [str(x) for x in g["name"]] == [c["name"] for c in cases], name
        assert all(c["scoring"] == tuple(int(x) for x in g["scoring"]) for c in cases), name
        for k, v in E.pack(cases).items():
            assert np.array_equal(g[k], v), (name, k)


def test_scoring_sets_the_issue_names():
    sets = set(E.SCORING.values())
    assert {(1, 2, 2, 1, 32, 0), (2, 4, 4, 2, 4, 2), (2, 4, 4, 1, 6, 3), (2, 4, 10, 0, 3, 2), (2, 4, 0, 3, 20, 0), (2, 4, 5, 1, 4, 2), (2, 4, 4, 2, 5, 1),
            (0,) * 6, (127,) * 6, (2, 4, 100, 100, 100, 100), (3, 5, 60, 70, 120, 127)} <= sets
    assert sum(k.startswith("rand_") for k in E.SCORING) == 12 and len(sets) == len(E.SCORING)
    assert all(0 <= v <= 127 for sc in sets for v in sc)
    assert set(E.EARLY) == {"b_past_edge", "b_past_edge_swapped"}
    flags = {c["flag"] for c in E.scoring_cases("splice")}
    assert flags >= set(E.FLAGS6) and {c["zdrop"] for c in E.scoring_cases("splice")} == {100, -1}
    for cls, sc in E.SCORING.items():
        q, e, q2, e2 = E.swapped(sc)
        cases = E.scoring_cases(cls)
        assert max(max(len(c["query"]), len(c["target"])) for c in cases) <= 131, cls
        if max(q + e, q2 + e2) > 127:                        # where a sum wraps, half the problems cannot Z-drop
            assert sum(c["zdrop"] == -1 for c in cases) * 2 >= len(cases), cls


def test_expected_routes(files):
    for name in SCENES:
        g = files[name]
        sc = tuple(int(x) for x in g["scoring"])
        routes = {S.expected_route(int(q), int(t), sc) for q, t in zip(g["q_len"], g["t_len"])}
        assert routes == E.scene_routes(name), (name, routes)
    assert S.expected_route(700, 17, E.DEFAULT) == S.ROUTE_LDS                      # why wide_small_sides has a longer query against 17 bases
    ql, tl = E.WIDE_SHORT_TARGET
    assert S.state_bytes(ql, tl) == S.WIDE_BYTES + 16 and S.state_bytes(ql - 1, tl) == S.WIDE_BYTES


def test_class_table(files):
    table = E.class_table(files)
    assert set(table) == set(CLASSES), set(table) ^ set(CLASSES)
    missing = [k for k in CLASSES if not table[k]]
    assert not missing, missing


def test_scoring_scenes_run_to_the_end(files):
    for cls in E.SCORING:
        g = files[f"scoring_{cls}"]
        if cls in E.EARLY:
            assert (g["ez"] == M.reset_ez().astype(np.int32)).all() and g["cigar_off"][-1] == 0
        else:
            assert (g["ez"][:, 1] == 0).any() and (np.diff(g["cigar_off"]) > 0).any(), cls


def test_interleave_adjacencies(files):
    """The neighbours in the plan's order (by falling n_diag * n_col, the several-wave problems apart), with the recorded zdropped."""
    g, cases = files["interleave"], E.interleave()
    assert 55 <= len(cases) <= 65
    adj = E.adjacencies(cases, g["ez"][:, 1])
    assert set(adj) == set(E.ADJACENCIES) and all(adj.values()), {k: v for k, v in adj.items() if not v}
    # the work formula is the plan's: n_col from the model's geometry (ksw2_extd2_sse.c:82-86), routes from the library's constants
    from minimap2_chaindp_amd import chaindp
    assert chaindp.ksw_routing() == dict(lds_budget=S.LDS_BUDGET, per_target=S.PER_TARGET, per_query=S.PER_QUERY, fixed=S.FIXED,
                                         wide_bytes=S.WIDE_BYTES, wide_waves=S.WIDE_WAVES)
    l0, l1 = E.plan_order(cases)
    assert sorted(l0 + l1) == list(range(len(cases)))
    assert all(E.route(cases[i]) == S.ROUTE_WIDE for i in l1) and all(E.route(cases[i]) != S.ROUTE_WIDE for i in l0)
    for launch in (l0, l1):
        works = [E.work(cases[i]) for i in launch]
        assert works == sorted(works, reverse=True)
    # an early return has work 0 and every computed problem at least 32: no computed problem can follow an early return in a launch
    assert all((E.work(c) == 0) == (E.route(c) == S.ROUTE_NONE) for c in cases)
    assert {E.route(cases[i]) for i in l0[-3:]} == {S.ROUTE_NONE}


def test_hooks_bind_through_cabi():
    from minimap2_chaindp_amd import _cabi, chaindp
    protos = _cabi.prototypes("chaindp_ksw.h")
    assert protos["chaindp_ksw_debug_set_grid_cap"] == (C.c_int, [C.c_void_p, C.c_int])
    assert protos["chaindp_ksw_debug_launch"] == (C.c_int, [C.c_void_p, C.c_void_p])
    lib = chaindp.lib()
    assert lib.chaindp_ksw_debug_set_grid_cap(None, 1) == S.ERR_ARG and lib.chaindp_ksw_debug_launch(None, None) == S.ERR_ARG      # no context
    assert callable(chaindp.Device.ksw_set_grid_cap) and callable(chaindp.Device.ksw_launch)
