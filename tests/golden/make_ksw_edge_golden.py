#!/usr/bin/env python3
"""Generates tests/golden/ksw_edges/*.npz: what the UNMODIFIED reference's ksw_extd2_sse makes of the scenes of tests/ksw_edge_shapes.py
(build container only: it needs the reference's sources and a C compiler).  The reference is compiled where it lies into a temporary
directory outside the repository, by make_ksw_golden.py's build(); nothing of it is copied.  One file per call, in the format of
tests/golden/ksw/*.npz (scoring[6], the flat inputs of pack(), name[n], ez[n, 10], cigar_off[n + 1], cigar) and first_differs[n]: where
the model's "first" variant (the first maximum as max_t) does not give the reference's answer.

Asserts on the way: the model equals the reference on every problem; every scoring_* set that does not return early has a problem that
reaches its last diagonal and a non-empty CIGAR; global_flags holds both reach_end values, zdropped by Z-drop and by the band, a
score-only and an approximate-maximum record and one where "first" differs; the adjacencies of interleave hold with the recorded
zdropped; the class table of ksw_edge_shapes is complete; the directory stays below 1 MiB."""
import ctypes as C
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import ksw_edge_shapes as E  # noqa: E402
import ksw_model as M  # noqa: E402
from make_ksw_golden import Ez, build, simple_mat  # noqa: E402

OUT = os.path.join(HERE, "ksw_edges")


def ref_call(lib, free, c):
    a, b, q, e, q2, e2 = c["scoring"]
    mat = simple_mat(a, b)
    qs, ts = np.ascontiguousarray(c["query"]), np.ascontiguousarray(c["target"])
    ez = Ez()
    lib.ksw_extd2_sse(None, len(qs), qs.ctypes.data, len(ts), ts.ctypes.data, 5, mat.ctypes.data, q, e, q2, e2, c["w"], c["zdrop"], c["end_bonus"],
                      c["flag"], C.byref(ez))
    out = np.array([ez.max_zdropped & 0x7fffffff, ez.max_zdropped >> 31, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score,
                    ez.reach_end], np.int64).astype(np.int32)
    cig = np.array([ez.cigar[k] for k in range(ez.n_cigar)], np.uint32)
    if ez.cigar:
        free(ez.cigar)
    return out, cig


def main():
    tmp = tempfile.mkdtemp(prefix="ksw_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib, free = build(tmp)
        free.argtypes = [C.c_void_p]
        os.makedirs(OUT, exist_ok=True)
        files = {}
        for scene, cases in E.scenes().items():
            sc = cases[0]["scoring"]
            assert all(c["scoring"] == sc for c in cases)
            ezs, cigs, first = [], [], []
            for c in cases:
                ez, cig = ref_call(lib, free, c)
                args = (c["query"], c["target"], *sc, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
                mez, mcig = M.ksw_extd(*args)
                assert np.array_equal(mez, ez) and np.array_equal(mcig, cig), (c["name"], mez, ez, mcig, cig)
                vez, vcig = M.ksw_extd(*args, variant="first")
                first.append(not (np.array_equal(vez, ez) and np.array_equal(vcig, cig)))
                ezs.append(ez); cigs.append(cig)
            off = np.concatenate([[0], np.cumsum([len(x) for x in cigs])]).astype(np.int64)
            g = dict(scoring=np.array(sc, np.int32), name=np.array([c["name"] for c in cases]), ez=np.array(ezs, np.int32).reshape(-1, 10), cigar_off=off,
                     cigar=np.concatenate(cigs).astype(np.uint32) if off[-1] else np.zeros(0, np.uint32), first_differs=np.array(first, bool), **E.pack(cases))
            np.savez_compressed(os.path.join(OUT, scene + ".npz"), **g)
            files[scene] = g
            print(f"{scene}.npz: {len(cases)} problems, {off[-1]} CIGAR words, zdropped {int(g['ez'][:, 1].sum())}, first differs on {sum(first)}, "
                  f"{os.path.getsize(os.path.join(OUT, scene + '.npz'))} bytes")
            if scene.startswith("scoring_") and scene[len("scoring_"):] not in E.EARLY:
                assert (g["ez"][:, 1] == 0).any() and (np.diff(off) > 0).any(), scene
        table = E.class_table(files)
        for k, v in table.items():
            print(f"  {k}: {', '.join(v[:3])}{' ...' if len(v) > 3 else ''}")
        missing = [k for k, v in table.items() if not v]
        assert not missing, missing
        il = E.scenes()["interleave"]
        adj = E.adjacencies(il, files["interleave"]["ez"][:, 1])
        assert all(adj.values()), adj
        total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
        assert total < 1 << 20, total
        print(f"{sum(len(g['name']) for g in files.values())} problems in {len(files)} files, {total} bytes; the model equals the reference on all")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
