"""GPU tier of the region alignment's edge scenes: chaindp_align1 against the reference's recorded answers, tests/golden/align_edges/*.npz
(inputs: tests/align_edge_shapes.py) -- the DP's wide and global routes driven from device-made records, a second 64-lane stride in every
bookkeeping kernel, full slots, and batches that mix all of it, turn it around, follow one another on one context and pass 65 536 regions.
Every comparison is of every word."""
import glob
import os
import time

import numpy as np
import pytest

import align_edge_shapes as E
from conftest import GOLDEN_DIR
from test_gpu_align import call, check, dev  # noqa: F401  (dev: the module's context fixture)

pytestmark = pytest.mark.gpu

EDGE_DIR = os.path.join(GOLDEN_DIR, "align_edges")
SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(EDGE_DIR, "*.npz")))
NAMES = ("clamp_edges", "exact_runs", "global_left", "inv_skipped", "inversions", "long_join_wide", "many_anchors", "slots_full", "tiny", "wide_ext",
         "wide_fill_two_pass")


def load(name):
    z = np.load(os.path.join(EDGE_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def groups():
    """{opt words: the scenes' names} of every opt that more than one scene has, plus global_left's (all three routes in its first pass)."""
    by = {}
    for name in NAMES:
        by.setdefault(tuple(int(v) for v in load(name)["opt"]), []).append(name)
    return {"+".join(v): v for v in by.values() if len(v) > 1 or v == ["global_left"]}


GROUPS = groups()


def test_fixtures_are_there():
    assert tuple(SCENES) == NAMES
    assert sorted(len(v) for v in GROUPS.values()) == [1, 2, 6]


@pytest.mark.parametrize("name", NAMES)
def test_scene_in_one_call(dev, name):
    g = load(name)
    check(g, call(dev, g))


@pytest.mark.parametrize("names", list(GROUPS.values()), ids=list(GROUPS))
def test_mixed_batch(dev, names):
    """The scenes of one opt as one call: one-wave, four-wave and global problems in one DP batch, a second pass with a mix of its own, the
    region with full slots between other reads' regions."""
    g = E.concat([load(n) for n in names])
    check(g, call(dev, g))


@pytest.mark.parametrize("names", list(GROUPS.values()), ids=list(GROUPS))
def test_reads_in_reverse_order(dev, names):
    """The DP takes problems by falling work through a counter and reuses state, path slices and exchange words from one problem to the
    next: no read's answer may depend on where it stands in the call."""
    g = E.concat([load(n) for n in names])
    rev = E.reorder(g, range(len(g["seq_off"]) - 2, -1, -1))
    check(rev, call(dev, rev))


def test_a_smaller_call_follows_a_larger_on_one_context(dev):
    import test_gpu_ksw as T
    big = E.concat([load(n) for n in max(GROUPS.values(), key=len)])
    glob_, tiny = load("global_left"), load("tiny")
    check(big, call(dev, big))
    check(tiny, call(dev, tiny))
    check(glob_, call(dev, glob_))
    k = T.load(T.NAMED[0])
    ez, off, cig = T.call(dev, k)
    T.check(k, ez, off, cig)
    assert np.array_equal(dev.ksw_route(len(ez)), T.expected_routes(k))
    check(tiny, call(dev, tiny))
    check(big, call(dev, big))
    check(glob_, call(dev, glob_))


def tiled(g, times):
    out = dict(opt=g["opt"], tseq=g["tseq"], tseq_off=g["tseq_off"])
    for k in ("seq", "a", "regs", "a_out", "regs_out", "regs2", "extra", "cigar", "read_name"):
        out[k] = np.concatenate([g[k]] * times)
    for k in ("seq_off", "a_off", "regs_off", "cigar_off"):
        out[k] = np.concatenate([[0], np.cumsum(np.tile(np.diff(g[k]), times))]).astype(np.int64)
    return out


def test_tiled_batch_past_65536_regions(dev):
    """`tiny` repeated until there are more than 65 536 regions (and twice as many DP problems): al_grid's 65 536 workgroups take a second
    grid stride in k_align_plan, _gather, _zdrop, _stitch, _extra and _pack, and the DP's work counter runs far past its grid.  The expected
    output is the recording repeated, cigar_off accumulated."""
    tiny = load("tiny")
    times = 65536 // len(tiny["regs"]) + 1
    g = tiled(tiny, times)
    assert len(g["regs"]) > 65536 and int((g["regs"]["cnt"] + (g["regs"]["cnt"] > 0)).sum()) > 2 * 65536
    assert g["cigar_off"][-1] == times * tiny["cigar_off"][-1] and len(g["cigar"]) == g["cigar_off"][-1]
    t0 = time.perf_counter()
    got = call(dev, g)
    print(f"tiled call: {len(g['regs'])} regions, {time.perf_counter() - t0:.2f} s")
    check(g, got)
