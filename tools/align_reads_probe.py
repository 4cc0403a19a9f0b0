#!/usr/bin/env python3
"""Device.align_reads against the only way there was before it, on one GPU (DESIGN.md 8 N10 has an MI355X's figures).

A seeded batch of a few thousand reads in the style of tests/skeleton_shapes.fuzz_scene (both strands, up to three inverted, junk or
deleted stretches a read, some reads as two regions; map-ont scoring with the low Z-drops of the test tiers).  After a warm-up of
both, five times in turn:
  (a) one Device.align_reads call, by the host clock around it;
  (b) the same rounds through Device.align1 and Device.align1_inv (tests/skeleton_model.run with the device's stages): only the wall
      time inside those calls is counted, each of which ends in a synchronise; the loop's host code between them is not.
The outputs of (a) and (b) are compared word for word first.  Reported: the medians, the spread (max - min) of each, the bytes that
cross the call boundary each way (bases, anchors, region records, CIGAR words and offsets as the caller passes and receives them; what
a stage moves for its own planning is the same in both), the rounds, and the device milliseconds per stage of one more call made
with profiling on.  Accepted when median(a) <= median(b) + spread(b).  Writes profiles/align_reads_probe.json.

  python tools/align_reads_probe.py [--reads 3000] [--out profiles/align_reads_probe.json]"""
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
import skeleton_model as K  # noqa: E402
import skeleton_shapes as SS  # noqa: E402
from minimap2_chaindp_amd import chaindp, params  # noqa: E402


def nbytes(*arrays):
    return int(sum(np.asarray(x).nbytes for x in arrays))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_reads_probe.json"))
    args = ap.parse_args()
    g = SS.pack(SS.fuzz_scene(seed=11, n_reads=args.reads))
    opt = params.AlignOpt(*(int(v) for v in g["opt"]))
    import torch
    prop = torch.cuda.get_device_properties(0)
    res = {"device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count},
           "batch": {"reads": len(g["seq_off"]) - 1, "bases": len(g["seq"]), "anchors": len(g["a"]), "regions": len(g["regs"])}}
    print("device:", res["device"], "batch:", res["batch"])
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 12) as dev:
        dev.align_set_targets(g["tseq_off"], g["tseq"])
        inside, moved = [0.0], [0, 0]

        def align1_batch(*x):
            t0 = time.perf_counter()
            out = dev.align1(opt, *x)
            inside[0] += time.perf_counter() - t0
            moved[0] += nbytes(*x); moved[1] += nbytes(*out)
            return out

        def inv_batch(*x):
            t0 = time.perf_counter()
            out = dev.align1_inv(opt, *x)
            inside[0] += time.perf_counter() - t0
            moved[0] += nbytes(*x); moved[1] += nbytes(*out)
            return out

        def one_call():
            t0 = time.perf_counter()
            out = dev.align_reads(opt, g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"])
            return time.perf_counter() - t0, out

        def stage_calls():
            inside[0], moved[0], moved[1] = 0.0, 0, 0
            out = K.run(K.opt_dict(g["opt"]), K.reads_of(g), align1_batch, inv_batch)
            return inside[0], out
        # warm-up, and the outputs word for word
        _, got = one_call()
        _, want = stage_calls()
        for k, x in zip(("a", "regs_off", "regs", "extra", "cigar_off", "cigar"), got):
            assert x.shape == want[k].shape and np.array_equal(K.words(x), K.words(want[k])), k
        _, got = one_call()
        placed_off, placed = dev.align_reads_placed()
        assert np.array_equal(placed_off, want["placed_off"]) and np.array_equal(K.words(placed), K.words(want["placed"]))
        rounds = [int(x) for x in dev.align_reads_rounds()]
        bytes_a = {"up": nbytes(g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"]), "down": nbytes(*got)}
        bytes_b = {"up": moved[0], "down": moved[1]}
        ta, tb = [], []
        for _ in range(5):
            ta.append(one_call()[0])
            tb.append(stage_calls()[0])
        dev.set_profiling(True)
        one_call()
        ms = dev.align_reads_ms()
        dev.set_profiling(False)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    spread_a, spread_b = max(ta) - min(ta), max(tb) - min(tb)
    res.update(rounds=rounds, final_regions=len(got[2]), cigar_words=len(got[5]),
               one_call_ms={"median": med_a * 1e3, "spread": spread_a * 1e3, "all": [t * 1e3 for t in ta], "bytes": bytes_a},
               stage_calls_ms={"median": med_b * 1e3, "spread": spread_b * 1e3, "all": [t * 1e3 for t in tb], "bytes": bytes_b},
               device_ms=ms, accepted=bool(med_a <= med_b + spread_b))
    print(f"rounds {rounds}, {res['final_regions']} final regions, {res['cigar_words']} CIGAR words")
    print(f"(a) one align_reads call:        median {med_a * 1e3:.2f} ms, spread {spread_a * 1e3:.2f} ms, {bytes_a['up']} bytes up, {bytes_a['down']} down")
    print(f"(b) align1 / align1_inv calls:   median {med_b * 1e3:.2f} ms, spread {spread_b * 1e3:.2f} ms, {bytes_b['up']} bytes up, {bytes_b['down']} down")
    print("device ms of one call:", {k: round(v, 3) for k, v in ms.items()})
    print("accepted" if res["accepted"] else "NOT accepted", f"(median(a) {'<=' if res['accepted'] else '>'} median(b) + spread(b))")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
