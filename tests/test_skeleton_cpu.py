"""CPU tier of the alignment loop: the batched composition tests/skeleton_model.py over the CPU models of the stages against the
reference's recorded mm_align_skeleton, tests/golden/skeleton/*.npz (tests/golden/make_skeleton_golden.py wrote them from the
unmodified reference and proved the composition equal to it there), the loop cases the scenes reach, and the host planners of
chaindp_align1 and chaindp_align1_inv on the inputs of every round through their no-GPU hooks."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import skeleton_model as K
import skeleton_shapes as SS
from conftest import GOLDEN_DIR

SKEL_DIR = os.path.join(GOLDEN_DIR, "skeleton")
SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SKEL_DIR, "*.npz")))
NAMES = ("asm", "filters", "fuzz", "inv_edges", "rounds", "zdrop_to_the_end")
TRACED = dict(align1=("regs_off", "regs_in", "a", "regs", "regs2", "extra", "cigar_off", "cigar"),
              align1_inv=("regs_off", "regs_in", "made", "r_inv", "extra", "cigar_off", "cigar"))
words = K.words


def load(name):
    z = np.load(os.path.join(SKEL_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(words(x), words(y))


def calls_of(g):
    """The stage calls the fixture records, in order: [(stage, dict of its traced arrays)]; the last one is the inversion call."""
    n = int(g["n_calls"])
    return [("align1" if i < n - 1 else "align1_inv", {k: g["t%d_%s" % (i, k)] for k in TRACED["align1" if i < n - 1 else "align1_inv"]}) for i in range(n)]


def test_fixtures_are_there_and_small():
    assert SCENES == sorted(NAMES)
    assert all(os.path.getsize(os.path.join(SKEL_DIR, n + ".npz")) < 1 << 20 for n in SCENES)


def test_shapes_are_what_was_recorded():
    scenes = {s["name"]: SS.pack(s) for s in SS.all_scenes()}
    assert sorted(scenes) == SCENES
    for name, p in scenes.items():
        g = load(name)
        assert SS.squeezed(p), name
        for k, v in p.items():
            assert same(np.asarray(v), g[k]), (name, k)


@pytest.fixture(scope="module")
def modelled():
    """Every scene through the loop over the CPU models once: {name: (outputs, trace)}, and the class counters of the whole run."""
    K.cover.clear()
    out = {}
    for name in SCENES:
        trace = []
        out[name] = (SS.check(load(name), trace), trace)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_composition_equals_the_reference(modelled, name):
    g = load(name)
    got, trace = modelled[name]
    for k in K.OUTPUTS:
        assert same(got[k], g[k + "_out"]), (name, k)
    assert not g["regs_out"]["reserved"].any()
    several = np.repeat(np.diff(g["regs_off_out"]) > 1, np.diff(g["regs_off_out"]))
    assert (g["extra_out"]["has_extra"][several] == 1).all()                   # the sort asserts an alignment on every region it orders


@pytest.mark.parametrize("name", NAMES)
def test_stage_calls_are_what_was_recorded(modelled, name):
    g = load(name)
    trace = modelled[name][1]
    rec = calls_of(g)
    assert [t["stage"] for t in trace] == [stage for stage, _ in rec]
    for i, (t, (stage, want)) in enumerate(zip(trace, rec)):
        for k, v in want.items():
            assert same(t[k], v), (name, "call", i, stage, k)


def test_every_class_is_reached(modelled):
    assert not [k for k in K.COVER if not K.cover[k]], dict(K.cover)
    assert not K.cover["inv_no_cigar"]            # no scoring gives the loop a pair without a CIGAR
    codes = np.concatenate([calls_of(load(n))[-1][1]["made"] for n in SCENES])
    assert set(codes.tolist()) == {0, 1, 2, 3}
    assert max(int(load(n)["n_calls"]) - 1 for n in SCENES) >= 3


def test_round_two_needs_the_anchors_round_one_returned():
    """The scene whose first round marks seeds: with the scene's own anchors fed to every round in their place, the marks the first round
    left in the parent's range are missing in the returned anchors.  The regions come out the same: mm_filter_bad_seeds of the later
    round finds the marks of the split-off region's own range again, so a[] is the word that tells the two loops apart."""
    g = load("rounds")
    align1, inv = K.cpu_stages(g["opt"], g["tseq_off"], g["tseq"])
    got = K.run(K.opt_dict(g["opt"]), K.reads_of(g), lambda so, s, ao, a, ro, r: align1(so, s, ao, g["a"], ro, r), inv)
    assert not same(got["a"], g["a_out"])
    rd = int(np.flatnonzero(g["read_name"] == "marks_behind_drop")[0])
    a0, a1 = int(g["a_off"][rd]), int(g["a_off"][rd + 1])
    assert (got["a"][a0:a1, 1] != g["a_out"][a0:a1, 1]).any() and same(got["regs"], g["regs_out"])


# ---- the host's part of every call, without a GPU

def _check(fn, opt, n_reads, arrs, t_off):
    from minimap2_chaindp_amd import chaindp, params
    o = params.AlignOpt(*(int(v) for v in opt))
    t_off = np.ascontiguousarray(t_off, np.int64)
    out = (C.c_int64 * 2)()
    arrs = [np.ascontiguousarray(x) for x in arrs]
    rc = getattr(chaindp.lib(), fn)(C.byref(o), n_reads, *(x.ctypes.data for x in arrs), len(t_off) - 1, t_off.ctypes.data, out)
    return rc, int(out[0]), int(out[1])


@pytest.mark.parametrize("name", NAMES)
def test_planners_accept_the_inputs_of_every_round_and_of_the_inversion_call(name):
    g = load(name)
    a, empty_reads, n_reads = g["a"], 0, len(g["seq_off"]) - 1
    for i, (stage, t) in enumerate(calls_of(g)):
        n_regs = len(t["regs_in"])
        assert len(t["regs_off"]) == len(g["seq_off"]) and int(t["regs_off"][-1]) == n_regs
        empty_reads += int((np.diff(t["regs_off"]) == 0).sum())
        if stage == "align1":
            cnt = t["regs_in"]["cnt"].astype(np.int64)
            got = _check("chaindp_align_debug_check", g["opt"], n_reads, [g["seq_off"], g["a_off"], a, t["regs_off"], t["regs_in"]], g["tseq_off"])
            assert got == (0, n_regs, int((cnt + (cnt > 0)).sum())), (name, "round", i, got)
            a = t["a"]
        else:
            got = _check("chaindp_align_inv_debug_check", g["opt"], n_reads, [g["seq_off"], t["regs_off"], t["regs_in"]], g["tseq_off"])
            assert got[:2] == (0, n_regs) and got[2] == int((t["made"] != 0).sum()), (name, "inversion call", got)
    assert empty_reads or name == "inv_edges"              # a read without a region in a round: every scene but one has such a round
