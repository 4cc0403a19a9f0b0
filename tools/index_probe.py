"""The index build on the device, stage by stage: seeded random reads of 10 kb (the all-vs-all case: the reads are the target), ava-ont
parameters (w = 5, k = 15, b = 14), chaindp_index_build repeated; per stage the median milliseconds (the sketch with its uploads by the
host's clock, the sort, the grouping and the tables by events on the device's stream), the whole call by the host's clock, bases/s.
With --ref the reference's own mm_idx_gen on the CPU instead (one thread, through oracle/_ref/mt_dump, which prints the reference's
stage times on stderr) for a target of the same recipe.  One JSON line.
   python3 tools/index_probe.py [bases=200000000] [repeats=5]
   python3 tools/index_probe.py --ref [bases=20000000]"""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN, W, K, B = 10000, 5, 15, 14


def reads(bases, seed=1):
    """uint8 codes 0..3 (bases as the sketch takes them), all reads concatenated, and their offsets"""
    n = max(1, bases // READ_LEN)
    return np.random.RandomState(seed).randint(0, 4, n * READ_LEN).astype(np.uint8), np.arange(n + 1, dtype=np.int64) * READ_LEN


def device(bases, repeats):
    from minimap2_chaindp_amd import chaindp
    seq, seq_off = reads(bases)
    n = len(seq_off) - 1
    out = {"probe": "index_probe", "reads": n, "bases": int(len(seq)), "w": W, "k": K, "b": B, "repeats": repeats}
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=n + 1) as d:
        lib = chaindp.lib()

        def once():
            t0 = time.perf_counter()
            ix = d.build_index(W, K, 0, seq, seq_off, b=B)
            wall = (time.perf_counter() - t0) * 1e3
            ms, route = d.index_stage_ms(ix), d.index_route(ix)
            d._indexes.remove(ix); lib.chaindp_index_destroy(ix)
            return wall, ms, route
        once()                                                              # warm-up: buffers grown, code objects loaded
        runs = [once() for _ in range(repeats)]
        d.set_profiling(True)                                               # the sketch kernels alone (no uploads), one more build
        d.sketch_ms(reset=True)
        once()
        sk_ms, sk_calls = d.sketch_ms(reset=True)
    med = lambda xs: statistics.median(xs)  # noqa: E731
    stage = [med([r[1][i] for r in runs]) for i in range(4)]
    wall = med([r[0] for r in runs])
    out.update(route=runs[0][2], wall_ms=wall, wall_ms_min_max=[min(r[0] for r in runs), max(r[0] for r in runs)],
               stage_ms=dict(zip(("sketch_with_uploads", "sort", "group", "tables"), stage)), sketch_kernels_ms=sk_ms,
               tables_share_of_device_stages=stage[3] / max(sk_ms + stage[1] + stage[2] + stage[3], 1e-9),
               bases_per_s=len(seq) / (wall / 1e3), sort_minimizers_per_s=runs[0][2]["minimizers"] / max(stage[1] / 1e3, 1e-12))
    return out


def reference(bases):
    dump = os.path.join(ROOT, "oracle", "_ref", "mt_dump")
    seq, seq_off = reads(bases)
    with tempfile.TemporaryDirectory() as tmp:
        fa, q = os.path.join(tmp, "t.fa"), os.path.join(tmp, "q.fa")
        txt = np.frombuffer(b"ACGT", np.uint8)[seq]
        with open(fa, "wb") as f:
            for i in range(len(seq_off) - 1):
                f.write(b">r%07d\n" % i + txt[seq_off[i]:seq_off[i + 1]].tobytes() + b"\n")
        with open(q, "wb") as f:
            f.write(b">q\n" + txt[:500].tobytes() + b"\n")
        t0 = time.perf_counter()
        r = subprocess.run([dump, "ava-ont", fa, q, os.path.join(tmp, "a.bin")], capture_output=True, text=True, check=True)
        wall = time.perf_counter() - t0
    ms = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"(mm_idx_gen \d|create idx time):\s*([0-9.]+)", r.stderr)}
    total = sum(ms.values())
    return {"probe": "index_probe --ref", "reads": len(seq_off) - 1, "bases": int(len(seq)), "threads": 1, "reference_ms": ms,
            "mm_idx_gen_ms": total, "bases_per_s": len(seq) / max(total / 1e3, 1e-12), "process_wall_s": wall}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--ref"]
    if "--ref" in sys.argv:
        print(json.dumps(reference(int(args[0]) if args else 20_000_000)))
    else:
        print(json.dumps(device(int(args[0]) if args else 200_000_000, int(args[1]) if len(args) > 1 else 5)))
