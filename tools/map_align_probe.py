#!/usr/bin/env python3
"""What mapping with base alignment costs in one call against the same work composed from the calls there were before, on one GPU
(DESIGN.md 8 N12 has an MI355X's figures).

A seeded map-ont batch (tests/e2e_model.scenario, reads of up to 3000 bases on three targets of about 30 kb).  After a warm-up of
both, eleven times in turn, alternating in one process, by the host clock around each (both end in a synchronise):
  (A) one Device.map_align_seqs call;
  (B) Device.sketch, collect_seeds + run_full + backtrack + gen_regs (the stages of map_batch, on the sketch's resident minimizers),
      chain_post(MM_F_CIGAR, want_anchors=True), mm_squeeze_a in numpy, Device.align_reads_post.
The outputs are first compared byte for byte.  Reported: the medians and spreads (max - min) of both and their difference, the spread
of (B) being the yardstick for it; the bytes (B) moves that (A) does not (the bases once more, the anchors down and up); (B)'s numpy
squeeze alone; and the device milliseconds of (A)'s stages from its hook, from calls made with profiling on.  Writes
profiles/map_align_probe.json.

  python tools/map_align_probe.py [--reads 3000] [--out profiles/map_align_probe.json]"""
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
import e2e_model as em  # noqa: E402
import map_align_shapes as S  # noqa: E402
from minimap2_chaindp_amd import chaindp, params as P  # noqa: E402

REPEATS = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_align_probe.json"))
    args = ap.parse_args()
    sc = em.scenario("map-ont", n_reads=args.reads, seed=21, max_len=3000, genome_len=30000)
    opt = P.PostOpt(**dict(sc.opt.asdict(), flag=sc.opt.flag | P.MM_F_CIGAR))
    aopt = P.align_opt("map-ont")
    tseq, tseq_off = em.batch(sc.targets)
    seq, seq_off = em.batch(sc.reads)
    qlen = np.diff(seq_off).astype(np.int32)
    import torch
    prop = torch.cuda.get_device_properties(0)
    res = {"device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count},
           "batch": {"reads": len(sc.reads), "bases": len(seq)}}
    with chaindp.Device(0, max_anchors=1 << 24, max_reads=1 << 14) as dev:
        ix = dev.load_index(sc.image())
        dev.align_set_targets(tseq_off, tseq)
        moved = {}

        def one():
            return dev.map_align_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, opt, aopt, seq, seq_off, sc.bid, sc.hash_, sc.ref_len)

        def composed():
            dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off)
            _, _, rep, _, _ = dev.collect_seeds(ix, sc.flag, sc.max_occ, None, None, sc.bid, None)
            dev.run_full(sc.par)
            coff, _, _, _ = dev.backtrack(sc.par, sc.min_cnt)
            dev.gen_regs(sc.hash_, qlen, int(coff[-1]))
            roff, regs, aoff, a = dev.chain_post(opt, sc.ref_len, want_anchors=True)
            t0 = time.perf_counter()
            regs2, aoff2, a2 = S.squeeze(roff, regs, aoff, a)
            moved["squeeze_ms"] = (time.perf_counter() - t0) * 1e3
            moved["anchors_down"], moved["anchors_up"], moved["regions"] = len(a), len(a2), len(regs)
            return dev.align_reads_post(aopt, opt, seq_off, seq, aoff2, a2, roff, regs2, rep)[1:]

        A, B = one(), composed()                                           # warm-up, and the comparison
        for k, (x, y) in enumerate(zip(A[:6], B)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), ("the two paths differ", k)
        res["batch"].update(regions_before_alignment=moved["regions"], final_regions=len(A[1]), cigar_words=len(A[5]), anchors=A[7],
                            chain_anchors=moved["anchors_down"], squeezed_anchors=moved["anchors_up"])
        ta, tb, sq = [], [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter(); one(); ta.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); composed(); tb.append((time.perf_counter() - t0) * 1e3)
            sq.append(moved["squeeze_ms"])
        dev.set_profiling(True)
        stages = []
        for _ in range(3):
            one()
            stages.append(dev.map_align_ms())
        dev.set_profiling(False)
    med = statistics.median
    res["one_call_ms"] = {"median": med(ta), "spread": max(ta) - min(ta), "runs": ta}
    res["composed_ms"] = {"median": med(tb), "spread": max(tb) - min(tb), "runs": tb, "numpy_squeeze_median": med(sq)}
    res["one_call_minus_composed_ms"] = med(ta) - med(tb)
    res["not_slower_than_composed_by_more_than_its_spread"] = bool(med(ta) - med(tb) <= max(tb) - min(tb))
    # (the one call brings the squeezed anchors down once, for the stages' host planner; the composed path brings every chain anchor
    # down, sends the squeezed ones up and gets them back with their marks)
    res["bytes_the_composed_path_moves_and_the_one_call_does_not"] = {
        "bases_up_again": int(len(seq)), "chain_anchors_down_beyond_the_squeezed": int((moved["anchors_down"] - moved["anchors_up"]) * 16),
        "squeezed_anchors_up": int(moved["anchors_up"] * 16), "anchors_down_again_with_marks": int(moved["anchors_up"] * 16)}
    res["one_call_stage_device_ms"] = {k: med([s[k] for s in stages]) for k in stages[0]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "device"}, indent=1))


if __name__ == "__main__":
    main()
