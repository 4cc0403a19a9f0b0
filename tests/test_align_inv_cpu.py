"""CPU tier: the model of mm_align1_inv (tests/inv_model.py) against the reference's recorded answers, tests/golden/align_inv/*.npz
(tests/golden/make_align_inv_golden.py wrote them from the unmodified reference and proved the model equal to it there); that the
scenes tell a wrong local-score kernel from a right one; and the host's part of chaindp_align1_inv through its no-GPU hook."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import align_model as A
import inv_model as M
import inv_shapes as S
from conftest import GOLDEN_DIR

INV_DIR = os.path.join(GOLDEN_DIR, "align_inv")
SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(INV_DIR, "*.npz")))
OUTPUTS = ("made", "r_inv", "extra", "cigar_off", "cigar", "ll", "prob")


def load(name):
    z = np.load(os.path.join(INV_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def words(x):
    return x.view(np.uint32) if x.dtype.fields else x


def stretches(g):
    """(reversed query codes, reversed target codes, ql) of every candidate pair of a scene, in slot order."""
    opt = dict(zip(A.OPT_FIELDS, (int(v) for v in g["opt"])))
    out = []
    for rd in range(len(g["seq_off"]) - 1):
        qf = A.nt4(bytes(g["seq"][g["seq_off"][rd]:g["seq_off"][rd + 1]]))
        for i in range(int(g["regs_off"][rd]) + 1, int(g["regs_off"][rd + 1])):
            r1, r2 = S.reg_dict(g["regs"][i - 1]), S.reg_dict(g["regs"][i])
            why, lens = M.early_return(opt, r1, r2)
            if why:
                continue
            rev1 = bool(r1["bits"] & M.BIT_REV)
            strand, qb = (qf, r2["qe"]) if rev1 else (A.revcomp(qf), len(qf) - r2["qs"])
            t = A.nt4(bytes(g["tseq"][g["tseq_off"][r1["rid"]]:g["tseq_off"][r1["rid"] + 1]]))
            out.append((strand[qb:qb + lens[0]][::-1], t[r1["re"]:r2["rs"]][::-1], lens[0]))
    return opt, out


def test_fixtures_are_there():
    assert SCENES == sorted(NAMES)
    assert len(SCENES) == 19 and "fuzz" in SCENES, SCENES
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(INV_DIR, "*.npz"))) < 200 << 10
    assert SCENES == sorted(sc["name"] for sc in S.named_scenes() + [S.fuzz_scene()])


@pytest.fixture(scope="module")
def modelled():
    """Every scene through the model once: {name: outputs}, and the class counters of the whole run."""
    M.cover.clear()
    return {name: S.model_scene(load(name)) for name in SCENES}


@pytest.mark.parametrize("name", SCENES)
def test_scenes_are_what_the_generator_packed(name):
    g = load(name)
    (sc,) = [s for s in S.named_scenes() + [S.fuzz_scene()] if s["name"] == name] if name != "fuzz" else [S.fuzz_scene()]
    for k, v in S.pack(sc).items():
        assert np.array_equal(words(v), words(g[k])), k


@pytest.mark.parametrize("name", SCENES)
def test_model_reproduces_the_reference(modelled, name):
    g = load(name)
    for k, got in zip(OUTPUTS, modelled[name]):
        assert got.shape == g[k].shape and np.array_equal(words(got), words(g[k])), k
    assert not words(g["r_inv"]).reshape(len(g["made"]), -1)[g["made"] != M.MADE].any() and not g["r_inv"]["reserved"].any()
    assert (g["extra"]["has_extra"] == (g["made"] == M.MADE)).all()


def test_every_class_is_reached(modelled):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_align_inv_golden", os.path.join(GOLDEN_DIR, "make_align_inv_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert not [k for k in gen.COVER if not M.cover[k]]
    made = np.concatenate([load(n)["made"] for n in SCENES])
    assert set(made.tolist()) == {0, 1, 2, 3, 4}


def test_no_fuzz_pair_is_left_out():
    g = load("fuzz")
    assert len(g["ll"]) >= 190 and (g["made"] == M.MADE).sum() >= 100           # model_scene raises where a pair is unspecified: none did


@pytest.mark.parametrize("name", ["padding_strand0", "padding_strand1"])
def test_padding_scenes_tell_an_unpadded_kernel(name):
    g = load(name)
    opt, st = stretches(g)
    mat = A.simple_mat(opt["a"], opt["b"])
    wrong = 0
    for (q, t, ql), want in zip(st, g["ll"]):
        assert M.ll_ends(q, t, mat, opt["q"], opt["e"]) == tuple(want)
        if want[1] >= ql:
            assert M.ll_ends(q, t, mat, opt["q"], opt["e"], pad=False) != tuple(want)
            wrong += 1
    assert wrong == 3 and sorted(ql - (int(w[1]) + 1) for (_, _, ql), w in zip(st, g["ll"]) if w[0] >= opt["min_dp_max"]) == [-7, -4, -1, 0, 10]          # 10: the N in front of the copy, not the copy's first base at 11


def test_qe_tie_scene_tells_first_and_last_row_from_the_striped_order():
    g = load("qe_tie")
    opt, ((q, t, ql),) = stretches(g)
    mat = A.simple_mat(opt["a"], opt["b"])
    want = tuple(g["ll"][0])
    assert M.ll_ends(q, t, mat, opt["q"], opt["e"]) == want and want[1] < ql
    assert M.ll_ends(q, t, mat, opt["q"], opt["e"], tie="first") != want and M.ll_ends(q, t, mat, opt["q"], opt["e"], tie="last") != want


def test_te_tie_scene_takes_the_last_column():
    g = load("te_tie")
    opt, ((q, t, ql),) = stretches(g)
    mat = A.simple_mat(opt["a"], opt["b"])
    score, qe, te = (int(v) for v in g["ll"][0])
    assert (score, te) == (90, 110)
    assert M.ll_ends(q, t[:te], mat, opt["q"], opt["e"])[::2] == (score, 54)   # the same maximum 56 columns earlier: the later column wins


# ---- the host's part of the call, without a GPU

def _check(opt, p, t_off=None):
    from minimap2_chaindp_amd import chaindp, params
    o = params.AlignOpt(*(int(v) for v in opt))
    t_off = np.ascontiguousarray(p["tseq_off"] if t_off is None else t_off, np.int64)
    out = (C.c_int64 * 2)()
    arrs = [np.ascontiguousarray(p[k]) for k in ("seq_off", "regs_off", "regs")]
    rc = chaindp.lib().chaindp_align_inv_debug_check(C.byref(o), len(p["seq_off"]) - 1, *(x.ctypes.data for x in arrs), len(t_off) - 1, t_off.ctypes.data, out)
    return rc, int(out[0]), int(out[1])


NAMES = ("early_returns", "padding_strand0", "padding_strand1", "te_tie", "qe_tie", "stripe_edges", "score_at_min_dp_max", "score_below_min_dp_max",
         "saturation", "route_wide", "route_global", "ext_zdrop", "leading_gap", "n_both_sides", "no_cigar", "three_regions_skip",
         "three_regions_first_fails", "ll_lds_above_64k", "fuzz")


@pytest.mark.parametrize("name", NAMES)
def test_planner_counts_the_candidates_of_every_scene(name):
    g = load(name)
    assert _check(g["opt"], g) == (0, len(g["regs"]), len(g["ll"])) and (name != "fuzz" or len(g["ll"]) == 198)


def test_the_edge_of_the_longest_stretch_needs_more_lds_than_a_launch_gets_unasked():
    g = load("ll_lds_above_64k")
    ((q, t, ql),) = stretches(g)[1]
    assert (ql + 7) // 8 * 8 * 4 > 65536 and ql <= 20000 and g["made"].tolist() == [0, 1]


def test_planner_refusals():
    g = load("padding_strand0")
    opt = {k: int(v) for k, v in zip(A.OPT_FIELDS, g["opt"])}

    def refused(change=None, **arrays):
        o = dict(opt, **(change or {}))
        return _check([o[k] for k in A.OPT_FIELDS], dict(g, **arrays))[0] == -1

    assert not refused()
    assert refused(dict(flag=A.F_SR)) and refused(dict(flag=A.F_SPLICE)) and not refused(dict(flag=A.F_FOR_ONLY))
    assert refused(dict(q2=opt["q"], e2=opt["e"]))
    for k in ("a", "b", "q", "e", "q2", "e2"):
        assert refused({k: 128}) and refused({k: -1}), k
    assert refused(dict(max_gap=20001)) and not refused(dict(max_gap=20000))
    assert refused(tseq_off=g["tseq_off"][:1])                                  # no targets
    regs = g["regs"].copy(); regs["rid"][:2] = len(g["tseq_off"]) - 1
    assert refused(regs=regs)                                                    # a candidate's rid is no target
    regs = g["regs"].copy(); regs["rs"][1] += 100000; regs["re"][0] += 100000
    assert refused(regs=regs)                                                    # its target stretch lies outside the sequence
    regs = g["regs"].copy(); regs["rid"][:2] = 99; regs["bits"][1] &= ~np.uint32(M.BIT_SPLIT_INV)
    assert not refused(regs=regs)                                                # a pair that returns early is never looked at
    off = g["regs_off"].copy(); off[1] = off[2] + 1
    assert refused(regs_off=off)


def test_prototypes_bind_through_the_header():
    from minimap2_chaindp_amd import _cabi, chaindp, params
    protos = _cabi.prototypes("chaindp_align_inv.h")
    assert list(protos) == ["chaindp_align1_inv", "chaindp_align_inv_debug_check", "chaindp_align_inv_debug_ll", "chaindp_align_inv_debug_ms"]
    assert chaindp.ALIGN_INV_SYMBOLS == tuple(protos)
    restype, argtypes = protos["chaindp_align1_inv"]
    assert restype is C.c_int and len(argtypes) == 13 and argtypes[1] is C.POINTER(params.AlignOpt) and argtypes[2] is C.c_int64 and argtypes[-1] is C.c_int64
    with open(os.path.join(_cabi.INCLUDE, "chaindp.h")) as f:
        assert '#include "chaindp_align_inv.h"' in f.read()
    fn = chaindp.lib().chaindp_align1_inv
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert chaindp.lib().chaindp_align1_inv(None, None, 0, *([None] * 9), 0) == -1              # no context
    assert "align1_inv" in chaindp._CAPS
