"""Writes tests/golden/sketch_edges/ref_digests.json: for every case of tests/sketch_edge_shapes.py the SHA-256 over mini_off and
mini as the unmodified reference's mm_sketch returned them (tests/sketch_ref.py, oracle/_ref/libmm2sketch_ref.so) and the minimizer
count.  Needs oracle/_ref (make -C oracle ref).  The inputs are not stored: the constructors are seeded and deterministic.  Every
case must be present and the CPU model must agree with the reference before anything is written.

    python tests/golden/make_sketch_edge_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import sketch_edge_shapes as se  # noqa: E402
import sketch_ref as sr  # noqa: E402


def main():
    assert sr.have(), "oracle/_ref/libmm2sketch_ref.so is not built (make -C oracle ref)"
    rec = {}
    for name in se.CASES:
        c = se.case(name)
        seq, seq_off = se.batch(c.seqs)
        off, mini = sr.sketch_batch(seq, seq_off, c.w, c.k, c.is_hpc, n_segs_per_read=c.n_segs)
        m_off, m_mini = se.expected(name)
        assert np.array_equal(off, m_off) and mini.tobytes() == m_mini.tobytes(), f"{name}: the model differs from the reference"
        rec[name] = sr.digest(off, mini)
    assert set(rec) == set(se.CASES)
    os.makedirs(os.path.dirname(sr.DIGESTS), exist_ok=True)
    with open(sr.DIGESTS, "w") as fh:
        json.dump(dict(sorted(rec.items())), fh, indent=0)
        fh.write("\n")
    print(f"{len(rec)} cases, {sum(r['n'] for r in rec.values())} minimizers -> {os.path.relpath(sr.DIGESTS)}")


if __name__ == "__main__":
    main()
