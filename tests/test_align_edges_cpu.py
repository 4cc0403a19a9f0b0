"""CPU tier of the region alignment's edge scenes (tests/align_edge_shapes.py): the model against the reference's recorded answers
(tests/golden/align_edges/*.npz, made by tests/golden/make_align_edge_golden.py from the unmodified reference), the scenes against the
recorded inputs, and -- by running the model here, not by reading a file -- that every edge the scenes were built for is still reached."""
import collections
import glob
import os

import numpy as np
import pytest

import align_edge_shapes as E
import align_model as A
import align_shapes as S
from conftest import GOLDEN_DIR
from test_align_cpu import _check, words

EDGE_DIR = os.path.join(GOLDEN_DIR, "align_edges")
SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(EDGE_DIR, "*.npz")))
NAMES = ("clamp_edges", "exact_runs", "global_left", "inv_skipped", "inversions", "long_join_wide", "many_anchors", "slots_full", "tiny", "wide_ext",
         "wide_fill_two_pass")


def load(name):
    z = np.load(os.path.join(EDGE_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def modelled():
    """{scene: (the model's outputs, its counters, its DP calls, its inversion stretches)}: the model runs once for the whole file."""
    out = {}
    for name in SCENES:
        A.cover.clear(); del A.problems[:]; del A.inv_seen[:]
        got = S.model_scene(load(name))
        out[name] = (got, collections.Counter(A.cover), list(A.problems), list(A.inv_seen))
    return out


def test_fixtures_are_there_and_small():
    assert tuple(SCENES) == NAMES
    assert all(os.path.getsize(os.path.join(EDGE_DIR, n + ".npz")) < 1 << 20 for n in SCENES)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference(modelled, name):
    g = load(name)
    for label, x, want in zip(("a", "regs", "regs2", "extra", "cigar_off", "cigar"), modelled[name][0], (g[k] for k in ("a_out", "regs_out", "regs2", "extra", "cigar_off", "cigar"))):
        assert np.array_equal(words(x), words(want)), (name, label)


def test_shapes_are_what_was_recorded():
    """The goldens' inputs are the scenes of align_edge_shapes (seeded): a change there needs the goldens made again."""
    scenes = {s["name"]: S.pack(s) for s in E.scenes()}
    assert sorted(scenes) == SCENES
    for name, p in scenes.items():
        g = load(name)
        for k, v in p.items():
            assert np.array_equal(words(np.asarray(v)), words(g[k])), (name, k)
    tseq = {bytes(load(n)["tseq"]) for n in SCENES}
    assert len(tseq) == 1                                       # one target list: scenes of one opt concatenate into one call


def test_every_edge_is_reached(modelled):
    total = collections.Counter()
    for name in SCENES:
        total.update(modelled[name][1])
    print({k: total[k] for k in E.COUNTERS})
    assert not [k for k in E.COUNTERS if total[k] <= 0]
    # ... and in the scene built for it
    where = {"wide_ext": ("route_wide_ext_left", "route_wide_ext_right"), "wide_fill_two_pass": ("route_wide_fill_pass1", "route_wide_fill_pass2", "split_both_sides_gt_64"),
             "long_join_wide": ("route_wide_long_join",), "global_left": ("route_global", "route_wide_fill_pass1", "route_wide_fill_pass2", "route_lds"),
             "many_anchors": ("cnt1_gt_64", "cnt1_gt_128", "long_gaps_only_past_64"), "exact_runs": ("m_run_64", "m_run_65", "m_run_128", "m_run_129"),
             "clamp_edges": ("extra_clamp_at_63", "extra_clamp_at_0", "extra_max_at_63", "extra_max_at_0", "extra_clamp_then_max_later_block", "extra_gap_clamps", "n_ambi_in_gap"),
             "inversions": ("inv_t_le_64", "inv_t_65_128", "inv_t_gt_128", "inv_t_mod64_0", "inv_t_mod64_1", "inv_q_gt_t", "inv_q_lt_t", "inv_below_threshold"),
             "inv_skipped": ("inv_skipped_max_gap",), "slots_full": ("slots_full",)}
    for name, keys in where.items():
        assert not [k for k in keys if modelled[name][1][k] <= 0], name
    # both strands of the wide left extension (it is gathered reversed), and the wide second pass of global_left without a global problem in it
    g = load("wide_ext")
    assert {int(g["a"][g["a_off"][i], 0] >> np.uint64(63)) for i in (0, 1)} == {0, 1} and modelled["wide_ext"][1]["route_wide_ext_left"] == 2
    second = [p for p in modelled["global_left"][2] if p[5] == 2]
    assert second and all(A.KS.expected_route(p[1], p[2], "default") == A.KS.ROUTE_WIDE for p in second)
    # the regions of exactly 64, 65 and 129 anchors, the exact M runs, the inversion that splits with more than 64 anchors on both sides
    assert {64, 65, 129} <= set(load("many_anchors")["regs"]["cnt"].tolist())
    g = load("exact_runs")
    assert [int(c) for c in g["cigar"]] == [n << 4 for n in (64, 65, 127, 128, 129, 193)]
    g = load("wide_fill_two_pass")
    assert ((g["regs_out"]["cnt"] > 64) & (g["regs2"]["cnt"] > 64)).all() and (g["regs2"]["bits"] & A.BIT_SPLIT_INV != 0).sum() == 1
    # one code 1 after the inversion test ran, in `inversions`
    g = load("inversions")
    i = list(np.repeat(g["read_name"], np.diff(g["regs_off"]))).index("inv_diverged")
    assert g["regs2"]["cnt"][i] > 0 and not g["regs2"]["bits"][i] & A.BIT_SPLIT_INV
    # tiny: a region without anchors, a read without a region, both strands, cnt 1 and 2 only
    g = load("tiny")
    assert (np.diff(g["regs_off"]) == 0).sum() == 1 and (g["regs"]["cnt"] == 0).sum() == 1 and set(g["regs"]["cnt"].tolist()) == {0, 1, 2}
    assert len(set((g["a"][:, 0] >> np.uint64(63)).tolist())) == 2 and np.diff(g["seq_off"]).max() <= 60
    # slots_full: the full region lies between other reads' regions
    g = load("slots_full")
    assert len(g["regs"]) == 3 and list(g["read_name"]) == ["before", "full", "after"]


def test_planner_accepts_the_scenes_and_counts_their_slots():
    for name in SCENES:
        g = load(name)
        cnt = g["regs"]["cnt"].astype(np.int64)
        assert _check(g["opt"], g) == (0, len(cnt), int((cnt + (cnt > 0)).sum())), name


def test_concatenation_and_reordering_keep_every_word(modelled):
    """The helpers of the GPU tier's mixed batch and reversed order, against the model: the concatenated (reordered) inputs give the
    concatenated (reordered) recordings."""
    group = [load(n) for n in SCENES if np.array_equal(load(n)["opt"], load("inversions")["opt"])]
    assert len(group) >= 2
    both = E.concat(group)
    rev = E.reorder(both, range(len(both["seq_off"]) - 2, -1, -1))
    for g in (both, rev):
        for label, x, want in zip(("a", "regs", "regs2", "extra", "cigar_off", "cigar"), S.model_scene(g), (g[k] for k in ("a_out", "regs_out", "regs2", "extra", "cigar_off", "cigar"))):
            assert np.array_equal(words(x), words(want)), label
    assert list(rev["read_name"]) == list(both["read_name"])[::-1]


def test_many_anchors_tells_a_one_stride_count_from_the_full_one():
    """k_align_plan counts the long gaps of a region 64 anchors a stride.  Here a count over the first stride alone finds at most one, the
    full count two: mm_filter_bad_seeds marks anchors MM_SEED_IGNORE only if the second stride is counted."""
    g = load("many_anchors")
    for rd, name in enumerate(g["read_name"][:2]):
        a = g["a"][g["a_off"][rd]:g["a_off"][rd + 1]].astype(np.int64)
        gap = np.diff(a[:, 1] & 0xffffffff) - np.diff(a[:, 0] & 0xffffffff)        # gap[i - 1] lies ahead of anchor i
        long_at = np.flatnonzero(np.abs(gap) > 10) + 1
        assert (long_at < 64).sum() <= 1 and (long_at <= 64).sum() <= 1 and len(long_at) >= 2, name
        out = g["a_out"][g["a_off"][rd]:g["a_off"][rd + 1]]
        assert (out[:, 1] & np.uint64(A.SEED_IGNORE)).any() and not (g["a"][:, 1] & np.uint64(A.SEED_IGNORE)).any(), name
    first = g["a"][:int(g["a_off"][1])].astype(np.int64)
    assert (np.flatnonzero(np.abs(np.diff(first[:, 1] & 0xffffffff) - np.diff(first[:, 0] & 0xffffffff)) > 10) + 1).min() >= 64


def test_clamp_edges_tell_a_per_block_score_from_the_running_one():
    """k_align_extra carries s and the maximum over the 64-base blocks of an M run.  Here dp_max with s reset at every 64th base of an M
    run differs from the recorded one on the reads built for it."""
    g = load("clamp_edges")
    opt = dict(zip(A.OPT_FIELDS, (int(v) for v in g["opt"])))
    mat = A.simple_mat(opt["a"], opt["b"])
    tcodes = [A.nt4(bytes(g["tseq"][g["tseq_off"][i]:g["tseq_off"][i + 1]])) for i in range(len(g["tseq_off"]) - 1)]
    differs = {}
    for rd, name in enumerate(g["read_name"]):
        (i,) = range(int(g["regs_off"][rd]), int(g["regs_off"][rd + 1]))
        r = g["regs_out"][i]
        qf = A.nt4(bytes(g["seq"][g["seq_off"][rd]:g["seq_off"][rd + 1]]))
        q = (A.revcomp(qf) if r["bits"] & A.BIT_REV else qf)[(len(qf) - r["qe"]) if r["bits"] & A.BIT_REV else r["qs"]:]
        t = tcodes[r["rid"]][r["rs"]:r["re"]]
        toff = qoff = 0
        s = [0, 0]
        mx = [0, 0]                                             # [as mm_update_extra has it, with s reset at every 64th base of an M run]
        for c in g["cigar"][g["cigar_off"][i]:g["cigar_off"][i + 1]]:
            op, ln = int(c) & 0xf, int(c) >> 4
            if op == 0:
                for l in range(ln):
                    if l and l % 64 == 0:
                        s[1] = 0
                    for k in (0, 1):
                        s[k] = max(s[k] + int(mat[t[toff + l], q[qoff + l]]), 0)
                        mx[k] = max(mx[k], s[k])
                toff += ln; qoff += ln
            else:
                s = [max(v - (opt["q"] + opt["e"] * ln), 0) for v in s]
                if op == 1:
                    qoff += ln
                else:
                    toff += ln
        assert mx[0] == g["extra"]["dp_max"][i], name
        differs[str(name)] = mx[1] != mx[0]
    assert differs["clamp_at_63"] and differs["clamp_at_64"] and differs["max_at_64"], differs
