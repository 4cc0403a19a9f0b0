#!/usr/bin/env python3
"""Rates of chaindp_align1_inv on one GPU (DESIGN.md 8 has an MI355X's) for inverted stretches of 100, 1 000 and 10 000 bases: pairs per second by the host clock
around the whole synchronous call, and local-DP cells per second of k_inv_ll (rows of the padded query x target bases, by device
events with profiling on).  Every read is A + revcomp(X') + B against a target A + X + B, X' a copy of X with 4 % substitutions, the
two regions written as mm_align1 and mm_split_reg leave them; map-ont's options with max_gap 20 000.  One warm-up call, then the
median of five.

Beside it, k_align_zdrop's score-only DP (the inversion test inside chaindp_align1) on stretches of the same size: the same reads
given to chaindp_align1 as ONE region whose anchors lie in A and B, so that the gap fill across the inversion Z-drops and the
inversion is scored; the `zdrop` share of chaindp_align_debug_ms over the cells of the fills that came back as potential inversions.
Writes profiles/inv_probe.json and prints the lines of DESIGN.md 8.

  python tools/inv_probe.py [--out profiles/inv_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minimap2_chaindp_amd import chaindp, params  # noqa: E402

K, FLANK, STEP = 15, 300, 30
ACGT = np.frombuffer(b"ACGT", np.uint8)
BIT_SPLIT1, BIT_SPLIT2, BIT_SPLIT_INV = 1 << 8, 1 << 9, 1 << 24


def batch(rng, n, pairs):
    """pairs reads with an inverted stretch of n bases, each with its own target: the flat arrays of both calls."""
    tl = 2 * FLANK + n
    t = rng.integers(0, 4, (pairs, tl)).astype(np.uint8)
    x = t[:, FLANK:FLANK + n].copy()
    sub = rng.random(x.shape) < 0.04
    x[sub] = (x[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    q = t.copy()
    q[:, FLANK:FLANK + n] = 3 - x[:, ::-1]
    regs = np.zeros(2 * pairs, chaindp.REG_DTYPE)
    rid = np.arange(pairs)
    for i, (s, e, bits, id_, parent) in enumerate(((0, FLANK, BIT_SPLIT1, 0, 0), (FLANK + n, tl, BIT_SPLIT2 | BIT_SPLIT_INV, -1, -2))):
        r = regs[i::2]
        r["id"], r["parent"], r["rid"], r["qs"], r["qe"], r["rs"], r["re"], r["bits"], r["cnt"] = id_, parent, rid, s, e, s, e, bits, 3
    # one region per read for chaindp_align1: exact 15-mers every 30 bases of both flanks
    pos = np.concatenate([np.arange(K - 1, FLANK, STEP), np.arange(FLANK + n + K - 1, tl, STEP)]).astype(np.uint64)
    a = np.zeros((pairs, len(pos), 2), np.uint64)
    a[:, :, 0] = (rid.astype(np.uint64)[:, None] << np.uint64(32)) | pos[None, :]
    a[:, :, 1] = (np.uint64(K) << np.uint64(32)) | pos[None, :]
    whole = np.zeros(pairs, chaindp.REG_DTYPE)
    whole["cnt"], whole["rid"], whole["qs"], whole["rs"], whole["qe"], whole["re"] = len(pos), rid, 0, 0, int(pos[-1]) + 1, int(pos[-1]) + 1
    whole["mlen"] = whole["blen"] = whole["score"] = whole["score0"] = K * len(pos)
    off = np.arange(pairs + 1, dtype=np.int64)
    return dict(t_off=off * tl, tseq=ACGT[t].ravel(), seq_off=off * tl, seq=ACGT[q].ravel(), regs_off=off * 2, regs=regs,
                a_off=off * len(pos), a=a.reshape(-1, 2), whole=whole, whole_off=off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inv_probe.json"))
    args = ap.parse_args()
    opt = params.align_opt("map-ont", max_gap=20000)
    rng = np.random.default_rng(3)
    import torch
    prop = torch.cuda.get_device_properties(0)       # what the runtime says of the device: its marketing name is not always known to it
    res = {"device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                      "memory_gib": round(prop.total_memory / 2 ** 30)}, "options": "map-ont, max_gap 20000", "sizes": {}}
    print("device:", res["device"])
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as dev:
        dev.set_profiling(True)
        for n, pairs in ((100, 16384), (1000, 2048), (10000, 256)):
            b = batch(rng, n, pairs)
            dev.align_set_targets(b["t_off"], b["tseq"])
            times, ll_ms, made = [], [], None
            for it in range(6):
                t0 = time.perf_counter()
                made, r_inv, extra, off, cig = dev.align1_inv(opt, b["seq_off"], b["seq"], b["regs_off"], b["regs"])
                dt = time.perf_counter() - t0
                if it:
                    times.append(dt); ll_ms.append(dev.align_inv_ms())
            ms = {k: statistics.median(m[k] for m in ll_ms) for k in ll_ms[0]}
            cells = pairs * ((n + 7) // 8 * 8) * n
            row = {"pairs": pairs, "made": int((made == 1).sum()), "call_ms": statistics.median(times) * 1e3,
                   "pairs_per_s": pairs / statistics.median(times), "device_ms": ms, "ll_cells": cells, "ll_gcells_per_s": cells / ms["ll"] / 1e6}
            # the inversion test of chaindp_align1 on the same stretches
            zp = min(pairs, 512 if n < 10000 else 32)
            zo = np.arange(zp + 1, dtype=np.int64)
            na = int(b["a_off"][1])
            tlen = int(b["seq_off"][1])
            zd = []
            for it in range(3):
                _, regs, regs2, _, _, _ = dev.align1(opt, zo * tlen, b["seq"][:zp * tlen], zo * na, b["a"][:zp * na], zo, b["whole"][:zp])
                if it:
                    zd.append(dev.align_ms()["zdrop"])
            n_inv = int(((regs2["cnt"] > 0) & ((regs2["bits"] & BIT_SPLIT_INV) != 0)).sum())
            row["zdrop"] = {"reads": zp, "came_back_as_inversion": n_inv, "zdrop_ms": statistics.median(zd),
                            "gcells_per_s_if_every_stretch_was_scored": zp * n * n / statistics.median(zd) / 1e6 if n_inv else None}
            res["sizes"][str(n)] = row
            z = row["zdrop"]
            print(f"{n:>6} bases: {pairs} pairs, {row['made']} made, call {row['call_ms']:.2f} ms = {row['pairs_per_s']:.0f} pairs / s; k_inv_ll {ms['ll']:.3f} ms = "
                  f"{row['ll_gcells_per_s']:.2f} G cells / s; DP {ms['dp']:.3f} ms, finish {ms['finish']:.3f} ms, pack {ms['pack']:.3f} ms | k_align_zdrop on {zp} "
                  f"such fills: {z['zdrop_ms']:.3f} ms, {n_inv} potential inversions" + (f", about {z['gcells_per_s_if_every_stretch_was_scored']:.3f} G cells / s" if n_inv else ""))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
