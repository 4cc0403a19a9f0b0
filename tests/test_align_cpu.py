"""CPU tier of the region alignment (chaindp_align1): the Python restatement tests/align_model.py against the reference's recorded
answers (tests/golden/align/*.npz, made by tests/golden/make_align_golden.py from the unmodified reference), the refusals of the host
planner through its no-GPU hook, and the header's prototypes as the front end binds them."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import align_model as A
import align_shapes as S
from conftest import GOLDEN_DIR

ALIGN_DIR = os.path.join(GOLDEN_DIR, "align")
SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ALIGN_DIR, "*.npz")))


def load(name):
    z = np.load(os.path.join(ALIGN_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def words(x):
    return x.view(np.uint32) if x.dtype.fields else x


def test_fixtures_are_there_and_small():
    assert len(SCENES) == 14 and "fuzz" in SCENES, SCENES
    assert all(os.path.getsize(os.path.join(ALIGN_DIR, n + ".npz")) < 1 << 20 for n in SCENES)


@pytest.mark.parametrize("name", SCENES)
def test_model_equals_the_reference(name):
    g = load(name)
    got = S.model_scene(g)
    for label, x, want in zip(("a", "regs", "regs2", "extra", "cigar_off", "cigar"), got, (g[k] for k in ("a_out", "regs_out", "regs2", "extra", "cigar_off", "cigar"))):
        assert np.array_equal(words(x), words(want)), (name, label)


def test_shapes_are_what_was_recorded():
    """The goldens' inputs are the scenes of align_shapes (seeded): a change there needs the goldens made again."""
    scenes = {s["name"]: S.pack(s) for s in S.named_scenes() + [S.fuzz_scene()]}
    assert sorted(scenes) == SCENES
    for name, p in scenes.items():
        g = load(name)
        for k, v in p.items():
            assert np.array_equal(words(np.asarray(v)), words(g[k])), (name, k)


def test_local_score_model_on_small_cases():
    mat = A.simple_mat(2, 4)
    q = A.nt4("ACGTACGTAC")
    assert A.ll_score(q, q, mat, 4, 2) == 20                                     # ten matches
    assert A.ll_score(q, A.nt4("TTTT" + "ACGTACGTAC" + "GG"), mat, 4, 2) == 20   # local: the flanks cost nothing
    assert A.ll_score(q, A.nt4("ACGTAGCGTAC"), mat, 4, 2) == 20 - 6              # one inserted target base: q + e
    assert A.ll_score(A.nt4("NNNN"), A.nt4("ACGT"), mat, 4, 2) == 0 and A.ll_score(q[:0], q, mat, 4, 2) == 0


def _check(opt, p, t_off=None):
    from minimap2_chaindp_amd import chaindp, params
    o = params.AlignOpt(*(int(v) for v in opt))
    t_off = np.ascontiguousarray(p["tseq_off"] if t_off is None else t_off, np.int64)
    out = (C.c_int64 * 2)()
    arrs = [np.ascontiguousarray(p[k]) for k in ("seq_off", "a_off", "a", "regs_off", "regs")]
    rc = chaindp.lib().chaindp_align_debug_check(C.byref(o), len(p["seq_off"]) - 1, *(x.ctypes.data for x in arrs), len(t_off) - 1, t_off.ctypes.data, out)
    return rc, int(out[0]), int(out[1])


def test_planner_accepts_the_scenes_and_counts_their_slots():
    for name in SCENES:
        g = load(name)
        cnt = g["regs"]["cnt"].astype(np.int64)
        assert _check(g["opt"], g) == (0, len(cnt), int((cnt + (cnt > 0)).sum())), name


def test_planner_refusals():
    g = load("plain")
    opt = {k: int(v) for k, v in zip(A.OPT_FIELDS, g["opt"])}

    def refused(change=None, **arrays):
        o = dict(opt, **(change or {}))
        return _check([o[k] for k in A.OPT_FIELDS], dict(g, **arrays))[0] == -1

    assert not refused()
    assert refused(dict(flag=A.F_SR)) and refused(dict(flag=A.F_SPLICE)) and not refused(dict(flag=A.F_FOR_ONLY))
    assert refused(dict(q2=opt["q"], e2=opt["e"]))                                # ksw_extz2_sse is not built
    for k in ("a", "b", "q", "e", "q2", "e2"):
        assert refused({k: 128}) and refused({k: -1}), k
    a = g["a"].copy(); a[1, 0] ^= np.uint64(1 << 63)
    assert refused(a=a)                                                          # another strand inside a region
    a = g["a"].copy(); a[1, 0] += np.uint64(1 << 32)
    assert refused(a=a)                                                          # another rid inside a region
    a = g["a"].copy(); a[:, 0] += np.uint64(64 << 32)
    assert refused(a=a)                                                          # a rid that is no target
    a = g["a"].copy(); a[0, 0] = (a[0, 0] & np.uint64(0xffffffff00000000)) | np.uint64(int(g["tseq_off"][1]))
    assert refused(a=a)                                                          # a position at its target's length
    a = g["a"].copy(); a[0, 1] = (a[0, 1] & np.uint64(0xffffffff00000000)) | np.uint64(int(g["seq_off"][1]))
    assert refused(a=a)                                                          # ... at its read's length
    regs = g["regs"].copy(); regs["cnt"][0] = len(g["a"]) + 1
    assert refused(regs=regs)
    assert _check(g["opt"], g, t_off=[0])[0] == -1                               # no targets set


def test_prototypes_bind_through_the_header():
    from minimap2_chaindp_amd import _cabi, chaindp, params
    protos = _cabi.prototypes("chaindp_align.h")
    assert list(protos) == ["chaindp_align_set_targets", "chaindp_align_clear_targets", "chaindp_align1", "chaindp_align_debug_check", "chaindp_align_debug_ms"]
    assert chaindp.ALIGN_SYMBOLS == tuple(protos)
    restype, argtypes = protos["chaindp_align1"]
    assert restype is C.c_int and len(argtypes) == 14 and argtypes[1] is C.POINTER(params.AlignOpt) and argtypes[2] is C.c_int64 and argtypes[-1] is C.c_int64
    with open(os.path.join(_cabi.INCLUDE, "chaindp.h")) as f:
        assert '#include "chaindp_align.h"' in f.read()
    fn = chaindp.lib().chaindp_align1
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert C.sizeof(params.AlignOpt) == 18 * 4 and [k for k, _ in params.AlignOpt._fields_] == list(A.OPT_FIELDS)
    assert chaindp.lib().chaindp_align1(None, None, 0, *([None] * 10), 0) == -1              # no context
    o = params.align_opt("map-pb")
    assert (o.k, o.is_hpc, o.min_ksw_len, o.q2, o.zdrop_inv) == (19, 1, 200, 24, 200) and params.align_opt("asm10", bw=100).bw == 100
    assert "align1" in chaindp._CAPS
