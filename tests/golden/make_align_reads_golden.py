#!/usr/bin/env python3
"""Generates tests/golden/align_reads/*.npz: what the UNMODIFIED reference's mm_align_skeleton makes of the edge scenes of
tests/align_reads_shapes.py (build container only: it needs the reference's sources and a C compiler).  The driver is
tests/golden/make_skeleton_golden.py's (its build and ref_scene), compiled in a temporary directory outside the repository; nothing of
the reference is copied.  One file per scene: the flat inputs of align_reads_shapes.pack() with the scene's LDS cap, the reference's
outputs (placed_off_out, placed_out, regs_off_out, regs_out, extra_out, cigar_off_out, cigar_out, a_out) and n_calls, the stage calls
the batched composition made (the rounds and the inversion call).

The tie scenes (align_reads_shapes.TIE_NAMES) come the same way.  Where a scene's class depends on piece lengths or on a seed, the
search runs here, over the reference alone: seeds 0, 1, ... up to align_reads_shapes.SEARCH, the first whose recorded outputs reach the
class; it must be the seed committed in TIE_SEEDS, and a class that no seed reaches raises.  The one exception is the tie that arises
without help, which is wanted and may be missing: then TIE_SEEDS names no seed for it and no file is written.

Asserts on the way: the batched composition over the CPU models (tests/skeleton_model.py) equals the reference in every word; no
scene is refused; every class of align_reads_shapes.CLASSES and TIE_CLASSES occurred."""
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


def recorded(p, ref, n_calls=0):
    return dict(p, n_calls=np.int64(n_calls), **{k + "_out": ref[k] for k in K.OUTPUTS})


def search(lib, name, make, cls):
    """The first seed below RS.SEARCH at which the reference's outputs of make(seed) reach the class (every class of a tuple), or None."""
    for seed in range(RS.SEARCH):
        p = RS.pack(make(seed))
        c = RS.tie_classes(recorded(p, ref_scene(lib, p)))
        if all(c[k] for k in ([cls] if isinstance(cls, str) else cls)):
            print(f"{name}: seed {seed} reaches {cls}")
            return seed
    return None


def write(lib, sc, reached, classes):
    p = RS.pack(sc)
    trace = []
    model = SS.check(p, trace)                 # raises where the scene is refused: none may be
    ref = ref_scene(lib, p)
    for k in K.OUTPUTS:
        u, v = model[k], ref[k]
        assert u.shape == v.shape and np.array_equal(K.words(u), K.words(v)), (sc["name"], k)
    g = recorded(p, ref, len(trace))
    path = os.path.join(RS.GOLDEN, sc["name"] + ".npz")
    np.savez_compressed(path, **g)
    assert os.path.getsize(path) < 1 << 20
    reached.update(classes(g))
    print(f"{sc['name']}.npz: LDS cap {int(p['lds_cap'])}, {len(p['seq_off']) - 1} reads, regions in {np.diff(p['regs_off']).tolist()}, "
          f"placed {np.diff(ref['placed_off']).tolist()}, out {np.diff(ref['regs_off']).tolist()}, {len(trace) - 1} rounds, "
          f"{ref['cigar_off'][-1]} CIGAR words, {os.path.getsize(path)} bytes")


def main():
    tmp = tempfile.mkdtemp(prefix="align_reads_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(RS.GOLDEN, exist_ok=True)
        reached = collections.Counter()
        for sc in RS.all_scenes():
            write(lib, sc, reached, RS.classes)
        print("classes:", {k: reached[k] for k in RS.CLASSES})
        missing = [k for k in RS.CLASSES if not reached[k]]
        assert not missing, missing
        found = dict(ties_small=search(lib, "ties_small", lambda seed: RS.tie_scene("ties_small", seed),
                                       ("final_len_2_keys_equal", "final_len_3_one_tied_pair", "filtered_and_inversion_between_tied")),
                     ties_64=search(lib, "ties_64", lambda seed: RS.tie_scene("ties_64", seed), "final_past_64_all_keys_equal"),
                     ties_130=search(lib, "ties_130", lambda seed: RS.tie_scene("ties_130", seed), "final_len_130_plus_group_in_neither_order"),
                     ties_unaided=search(lib, "ties_unaided", RS.unaided_scene, RS.UNAIDED))
        assert None not in (found["ties_small"], found["ties_64"], found["ties_130"]), found
        if found["ties_unaided"] is None:
            print(f"no tie without help among {RS.SEARCH} seeds: ties_unaided is not written")
        assert found == RS.TIE_SEEDS, ("align_reads_shapes.TIE_SEEDS is to be", found)
        reached = collections.Counter()
        for sc in RS.tie_scenes():
            write(lib, sc, reached, RS.tie_classes)
        print("tie classes:", {k: reached[k] for k in RS.TIE_CLASSES + (RS.UNAIDED,)})
        missing = [k for k in RS.TIE_CLASSES if not reached[k]]
        assert not missing, missing
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
