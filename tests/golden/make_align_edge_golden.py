#!/usr/bin/env python3
"""Generates tests/golden/align_edges/*.npz: what the UNMODIFIED reference's mm_align1 makes of the scenes of tests/align_edge_shapes.py
(build container only: it needs the reference's sources and a C compiler).  The driver, its build and the per-scene run are
make_align_golden.py's; the files have the same format as tests/golden/align/*.npz.

Asserts on the way: the model (tests/align_model.py) equals the reference on every output of every scene; every class of
align_edge_shapes.COUNTERS was reached, counted by the model; every file is below 1 MiB.  Prints the figures DESIGN.md quotes."""
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
import align_edge_shapes as E  # noqa: E402
import align_model as A  # noqa: E402
import align_shapes as S  # noqa: E402
from make_align_golden import build, ref_scene, same  # noqa: E402

OUT = os.path.join(HERE, "align_edges")
LABELS = ("a", "regs", "regs2", "extra", "cigar_off", "cigar")


def main():
    tmp = tempfile.mkdtemp(prefix="align_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(OUT, exist_ok=True)
        A.cover.clear(); del A.problems[:]; del A.inv_seen[:]
        total = collections.Counter()
        for sc in E.scenes():
            p = S.pack(sc)
            n0 = len(A.problems)
            ref = ref_scene(lib, p)
            model = S.model_scene(p)
            for nm, u, v in zip(LABELS, model, ref):
                if not same([u], [v]):
                    bad = np.nonzero(u != v)[0][:4] if u.shape == v.shape else (u.shape, v.shape)
                    raise AssertionError((sc["name"], nm, bad, u[bad] if u.shape == v.shape else None, v[bad] if u.shape == v.shape else None))
            a, regs, regs2, extra, off, cig = ref
            path = os.path.join(OUT, sc["name"] + ".npz")
            np.savez_compressed(path, a_out=a, regs_out=regs, regs2=regs2, extra=extra, cigar_off=off, cigar=cig, **p)
            assert os.path.getsize(path) < 1 << 20
            total["regions"] += len(regs); total["problems"] += len(A.problems) - n0
            total["max_cnt"] = max(total["max_cnt"], int(p["regs"]["cnt"].max()))
            print(f"{sc['name']}.npz: {len(p['seq_off']) - 1} reads, {len(regs)} regions, {len(A.problems) - n0} DP problems, "
                  f"{int((regs2['cnt'] > 0).sum())} split, {off[-1]} CIGAR words, {os.path.getsize(path)} bytes")
        missing = [k for k in E.COUNTERS if not A.cover[k]]
        print("counters:", {k: A.cover[k] for k in E.COUNTERS})
        assert not missing, missing
        print(f"{total['regions']} regions, {total['problems']} DP problems: " + ", ".join(f"{A.cover['route_' + k]} {k}" for k in ("lds", "wide", "global", "none"))
              + f"; largest cnt {total['max_cnt']}; longest extension {max(max(p[1], p[2]) for p in A.problems if p[0] != 'fill')}, "
              f"longest fill {max(max(p[1], p[2]) for p in A.problems if p[0] == 'fill')}")
        print("inversion stretches (q_len, t_len):", sorted((q, t) for q, t, _ in A.inv_seen))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
