#!/usr/bin/env python3
"""What finishing aligned reads on the device costs, on one GPU (DESIGN.md 8 N11 has an MI355X's figures).

The seeded 3000-read batch of tools/align_reads_probe.py.  After a warm-up of both, eleven times in turn, alternating in one process:
  (a) one Device.align_reads_post call (mm_align_skeleton's loop, then the tail of align_regs and mm_set_mapq; only the finished
      result comes down), by the host clock around it -- the call ends in a synchronise;
  (b) one Device.align_reads call alone, the same way.
The output of (a) is first compared word for word with Device.align_reads followed by the resident Device.align_post, and with
tests/apost_model.py run over what (b) returns.  Reported: the medians and spreads (max - min) of both, their difference, the bytes
that cross the call boundary each way, the regions and CIGAR words the tail drops, and the stage's device milliseconds from its hook
(k_apost_read with the scans; the gathers) of calls made with profiling on, with the number of launches the stage makes.  Writes
profiles/align_post_probe.json.

  python tools/align_post_probe.py [--reads 3000] [--out profiles/align_post_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import apost_model as M  # noqa: E402
import apost_shapes as PS  # noqa: E402
import skeleton_model as K  # noqa: E402
import skeleton_shapes as SS  # noqa: E402
from minimap2_chaindp_amd import chaindp, params  # noqa: E402

REPEATS = 11


def nbytes(*arrays):
    return int(sum(np.asarray(x).nbytes for x in arrays))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_post_probe.json"))
    args = ap.parse_args()
    g = SS.pack(SS.fuzz_scene(seed=11, n_reads=args.reads))
    opt = params.AlignOpt(*(int(v) for v in g["opt"]))
    popt_d = PS.real_opt(g["opt"])
    popt = PS.post_opt(PS.opt_row(popt_d))
    n_reads = len(g["seq_off"]) - 1
    rng = np.random.default_rng(5)
    rep_len = np.where(rng.integers(0, 3, n_reads) == 0, 0, rng.integers(1, 401, n_reads)).astype(np.int32)
    import torch
    prop = torch.cuda.get_device_properties(0)
    res = {"device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count},
           "batch": {"reads": n_reads, "bases": len(g["seq"]), "anchors": len(g["a"]), "regions": len(g["regs"])}}
    print("device:", res["device"], "batch:", res["batch"])
    ins = (g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"])
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 12) as dev:
        dev.align_set_targets(g["tseq_off"], g["tseq"])

        def one_call():
            t0 = time.perf_counter()
            out = dev.align_reads_post(opt, popt, *ins, rep_len)
            return time.perf_counter() - t0, out

        def reads_alone():
            t0 = time.perf_counter()
            out = dev.align_reads(opt, *ins)
            return time.perf_counter() - t0, out
        # warm-up, and the outputs word for word
        _, got = one_call()
        _, plain = reads_alone()
        resident = dev.align_post(popt, rep_len)
        model = M.run(popt_d, rep_len, *plain[1:])
        for k, x, y in zip(M.OUTPUTS, got[1:], resident):
            assert x.shape == y.shape == model[k].shape and np.array_equal(K.words(x), K.words(y)) and np.array_equal(K.words(x), K.words(model[k])), k
        assert np.array_equal(got[0], plain[0])
        one_call(); reads_alone()
        ta, tb = [], []
        for _ in range(REPEATS):
            ta.append(one_call()[0])
            tb.append(reads_alone()[0])
        dev.set_profiling(True)
        stage = []
        for _ in range(5):
            one_call()
            stage.append(dev.align_post_ms())
        dev.set_profiling(False)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    spread_a, spread_b = max(ta) - min(ta), max(tb) - min(tb)
    ms = {k: statistics.median(s[k] for s in stage) for k in stage[0]}
    # k_apost_read; two scans of one tile each (two kernels a scan while the reads fit one tile of 1024, three above); the two gathers
    launches = 1 + 2 * (2 if n_reads <= 1024 else 3) + 2
    res.update(regions_in=len(plain[2]), cigar_words_in=len(plain[5]), final_regions=len(got[2]), cigar_words=len(got[6]),
               one_call_ms={"median": med_a * 1e3, "spread": spread_a * 1e3, "all": [t * 1e3 for t in ta],
                            "bytes": {"up": nbytes(*ins, rep_len), "down": nbytes(*got)}},
               align_reads_alone_ms={"median": med_b * 1e3, "spread": spread_b * 1e3, "all": [t * 1e3 for t in tb],
                                     "bytes": {"up": nbytes(*ins), "down": nbytes(*plain)}},
               difference_ms=(med_a - med_b) * 1e3, stage_device_ms=ms, stage_device_ms_all=stage, stage_launches=launches)
    print(f"{res['regions_in']} regions and {res['cigar_words_in']} CIGAR words after the loop, {res['final_regions']} and {res['cigar_words']} after the tail")
    print(f"(a) one align_reads_post call: median {med_a * 1e3:.2f} ms, spread {spread_a * 1e3:.2f} ms, {res['one_call_ms']['bytes']}")
    print(f"(b) align_reads alone:         median {med_b * 1e3:.2f} ms, spread {spread_b * 1e3:.2f} ms, {res['align_reads_alone_ms']['bytes']}")
    print(f"difference of the medians {(med_a - med_b) * 1e3:+.2f} ms; the stage's device ms {ms} over {launches} launches")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
