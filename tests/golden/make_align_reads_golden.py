#!/usr/bin/env python3
"""Generates tests/golden/align_reads/*.npz: what the UNMODIFIED reference's mm_align_skeleton makes of the edge scenes of
tests/align_reads_shapes.py (build container only: it needs the reference's sources and a C compiler).  The driver is
tests/golden/make_skeleton_golden.py's (its build and ref_scene), compiled in a temporary directory outside the repository; nothing of
the reference is copied.  One file per scene: the flat inputs of align_reads_shapes.pack() with the scene's LDS cap, the reference's
outputs (placed_off_out, placed_out, regs_off_out, regs_out, extra_out, cigar_off_out, cigar_out, a_out) and n_calls, the stage calls
the batched composition made (the rounds and the inversion call).

Asserts on the way: the batched composition over the CPU models (tests/skeleton_model.py) equals the reference in every word; no
scene is refused; every class of align_reads_shapes.CLASSES occurred."""
import collections
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import align_reads_shapes as RS  # noqa: E402
import skeleton_model as K  # noqa: E402
import skeleton_shapes as SS  # noqa: E402
from make_skeleton_golden import build, ref_scene  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="align_reads_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(RS.GOLDEN, exist_ok=True)
        reached = collections.Counter()
        for sc in RS.all_scenes():
            p = RS.pack(sc)
            trace = []
            model = SS.check(p, trace)                 # raises where the scene is refused: none may be
            ref = ref_scene(lib, p)
            for k in K.OUTPUTS:
                u, v = model[k], ref[k]
                assert u.shape == v.shape and np.array_equal(K.words(u), K.words(v)), (sc["name"], k)
            g = dict(p, n_calls=np.int64(len(trace)), **{k + "_out": ref[k] for k in K.OUTPUTS})
            path = os.path.join(RS.GOLDEN, sc["name"] + ".npz")
            np.savez_compressed(path, **g)
            assert os.path.getsize(path) < 1 << 20
            c = RS.classes(g)
            reached.update(c)
            print(f"{sc['name']}.npz: LDS cap {int(p['lds_cap'])}, {len(p['seq_off']) - 1} reads, regions in {np.diff(p['regs_off']).tolist()}, "
                  f"placed {np.diff(ref['placed_off']).tolist()}, out {np.diff(ref['regs_off']).tolist()}, {len(trace) - 1} rounds, "
                  f"{ref['cigar_off'][-1]} CIGAR words, {os.path.getsize(path)} bytes")
        print("classes:", {k: reached[k] for k in RS.CLASSES})
        missing = [k for k in RS.CLASSES if not reached[k]]
        assert not missing, missing
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
