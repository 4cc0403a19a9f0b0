"""CPU tier of Device.align_reads (chaindp_align_reads): the edge goldens tests/golden/align_reads/*.npz (made by
tests/golden/make_align_reads_golden.py from the unmodified reference's mm_align_skeleton) load, are the scenes of
tests/align_reads_shapes.py, reach every edge class and are reproduced by the loop over the CPU models; the call's prototypes bind
through its header, its _CAPS rows retry by the fetch call, and the planner's no-GPU hook accepts the scenes and makes the refusals."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import align_reads_shapes as RS
import skeleton_model as K
import skeleton_shapes as SS
from test_skeleton_cpu import NAMES as SKELETON_NAMES, load as load_skeleton, same

FUNCTIONS = ("chaindp_align_reads", "chaindp_align_reads_fetch", "chaindp_align_reads_debug_check", "chaindp_align_reads_debug_placed",
             "chaindp_align_reads_debug_rounds", "chaindp_align_reads_debug_ms", "chaindp_align_reads_debug_set_lds_cap")


def test_fixtures_are_there_and_small():
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(RS.GOLDEN, "*.npz")))
    assert files == sorted(RS.NAMES + RS.TIE_NAMES)
    assert all(os.path.getsize(os.path.join(RS.GOLDEN, n + ".npz")) < 1 << 20 for n in files)


def test_shapes_are_what_was_recorded():
    scenes = {s["name"]: RS.pack(s) for s in RS.all_scenes()}
    assert sorted(scenes) == sorted(RS.NAMES)
    for name, p in scenes.items():
        g = RS.load(name)
        assert SS.squeezed(p), name
        for k, v in p.items():
            assert same(np.asarray(v), g[k]), (name, k)


def test_every_edge_class_is_reached():
    reached = sum((RS.classes(RS.load(n)) for n in RS.NAMES), start=RS.collections.Counter())
    assert not [k for k in RS.CLASSES if not reached[k]], dict(reached)
    caps = {n: int(RS.load(n)["lds_cap"]) for n in RS.NAMES}
    assert caps == {"trips": RS.RD_LDS_CAP, "lds_cap": RS.SCENE_CAP} and 2 < RS.SCENE_CAP < 64 < RS.RD_LDS_CAP


@pytest.mark.parametrize("name", RS.NAMES)
def test_models_reproduce_the_reference(name):
    g = RS.load(name)
    trace = []
    got = SS.check(g, trace)
    for k in K.OUTPUTS:
        assert same(got[k], g[k + "_out"]), (name, k)
    assert len(trace) == int(g["n_calls"])


def test_the_header_binds():
    from minimap2_chaindp_amd import _cabi, chaindp
    assert chaindp.ALIGN_READS_SYMBOLS == FUNCTIONS
    lib = chaindp.lib()
    protos = _cabi.prototypes("chaindp_align_reads.h")
    for name in FUNCTIONS:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == protos[name][1], name
    assert len(protos["chaindp_align_reads"][1]) == 17 and len(protos["chaindp_align_reads_fetch"][1]) == 10
    with open(os.path.join(_cabi.INCLUDE, "chaindp.h")) as f:
        includes = re.findall(r'#include "(chaindp_\w+\.h)"', f.read())
    assert includes.index("chaindp_align_reads.h") == includes.index("chaindp_align_inv.h") + 1
    with open(os.path.join(_cabi.INCLUDE, "chaindp_align_reads.h")) as f:
        text = f.read()
    stable, hooks = text.split("NOT part of the stable ABI")
    assert all(("int %s(" % n in hooks) == ("_debug_" in n) and ("int %s(" % n in stable) == ("_debug_" not in n) for n in FUNCTIONS)


def test_caps_rows_retry_by_the_fetch_call():
    from minimap2_chaindp_amd import chaindp
    for row in ("align_reads", "align_reads_cigar"):
        assert chaindp._CAPS[row].retry == "align_reads_fetch" and chaindp._CAPS[row].explicit == "raise"
    assert "chaindp_" + chaindp._CAPS["align_reads"].retry in FUNCTIONS
    for m in ("align_reads", "align_reads_placed", "align_reads_rounds", "align_reads_ms"):
        assert callable(getattr(chaindp.Device, m))


def _check(g, opt=None, t_off=None, caps=(0, 0), **arrays):
    from minimap2_chaindp_amd import chaindp, params
    o = params.AlignOpt(*(int(v) for v in g["opt"]))
    for k, v in (opt or {}).items():
        setattr(o, k, v)
    t_off = np.ascontiguousarray(g["tseq_off"] if t_off is None else t_off, np.int64)
    arrs = [np.ascontiguousarray(arrays.get(k, g[k])) for k in ("seq_off", "a_off", "a", "regs_off", "regs")]
    out = (C.c_int64 * 2)()
    rc = chaindp.lib().chaindp_align_reads_debug_check(C.byref(o), len(arrs[0]) - 1, *(x.ctypes.data for x in arrs), len(t_off) - 1, t_off.ctypes.data,
                                                       caps[0], caps[1], out)
    return rc, int(out[0]), int(out[1])


def test_planner_accepts_the_scenes():
    for g in [RS.load(n) for n in RS.NAMES] + [load_skeleton(n) for n in SKELETON_NAMES]:
        assert _check(g) == (0, len(g["regs"]), len(g["seq_off"]) - 1)


def test_planner_refusals():
    g = load_skeleton("fuzz")
    assert _check(g, caps=(5, 7))[0] == 0
    for opt in (dict(flag=0x1000), dict(flag=0x80), dict(q2=int(g["opt"][2]), e2=int(g["opt"][3])), dict(a=128), dict(max_gap=20001), dict(bw=-1)):
        assert _check(g, opt=opt)[0] == -1, opt
    assert _check(g, t_off=np.zeros(1, np.int64))[0] == -1                      # no targets
    assert _check(g, caps=(-1, 0))[0] == -1 and _check(g, caps=(0, -1))[0] == -1
    off = g["regs_off"].copy(); off[1] = off[2] + 1
    assert _check(g, regs_off=off)[0] == -1                                      # falling offsets
    a = g["a"].copy(); a[0, 0] |= np.uint64(0x7fffffff << 32)
    assert _check(g, a=a)[0] == -1                                               # an anchor of no target
    regs = g["regs"].copy(); regs["cnt"][0] = len(g["a"]) + 1
    assert _check(g, regs=regs)[0] == -1                                         # a region past its read's anchors
