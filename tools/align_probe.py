#!/usr/bin/env python3
"""Rates of chaindp_align1 on one MI355X: regions per second and aligned read bases per second over a seeded batch -- by default 2 000
reads of 2..10 kb, mutated copies of stretches of twenty 200 kb targets (4 % substitutions, an indel of 1..3 bases every 60 bases or
so, both strands), anchors on exact 15-mers every 60 bases or so, one region per read, map-ont's options with its min_ksw_len of 200
-- and where the device time goes: plan (with the gathers), DP (both passes: this is what chaindp_ksw_extd alone takes on the same
problems), zdrop, stitch, extra (with the pack), by device events with profiling on.  One warm-up call, then the median of five by
the host clock around the whole synchronous call (checks, copies over PCIe both ways, the host's part between the kernels).  The gap
between the call and its DP share is the cost of the bookkeeping.  Writes profiles/align_probe.json and prints the lines of DESIGN.md 8.

  python tools/align_probe.py [--reads 2000] [--out profiles/align_probe.json]"""
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

K = 15
COMP = np.array([3, 2, 1, 0], np.uint8)


def make_read(rng, target, rid, lo, hi):
    """(read codes on its own forward strand, anchors uint64[n, 2]) of a mutated copy of a stretch of `target` (codes 0..3)."""
    ln = int(rng.integers(lo, hi + 1))
    t0 = int(rng.integers(0, len(target) - ln))
    pieces, tpos = [], []
    t = t0
    while t < t0 + ln:
        seg = int(min(rng.integers(30, 90), t0 + ln - t))
        pieces.append(target[t:t + seg]); tpos.append(np.arange(t, t + seg))
        t += seg
        u = rng.random()
        if u < 0.5:
            n = int(rng.integers(1, 4))
            pieces.append(rng.integers(0, 4, n).astype(np.uint8)); tpos.append(np.full(n, -1))
        else:
            t += int(rng.integers(1, 4))
    q, path = np.concatenate(pieces), np.concatenate(tpos)
    sub = rng.random(len(q)) < 0.04
    q[sub] = (q[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    path[sub] = -1
    # the length of the exact diagonal run ending at every base
    cont = np.concatenate([[False], (path[1:] == path[:-1] + 1) & (path[:-1] >= 0)]) & (path >= 0)
    idx = np.arange(len(q))
    start = np.maximum.accumulate(np.where(cont, 0, idx))
    run = np.where(path >= 0, idx - start + 1, 0)
    cand = np.flatnonzero(run >= K)
    keep, last = [], -10 ** 9
    for i in cand:
        if i - last >= 60:
            keep.append(i); last = i
    keep = np.array(keep, np.int64)
    rev = int(rng.integers(0, 2))
    a = np.zeros((len(keep), 2), np.uint64)
    a[:, 0] = (np.uint64(rev) << np.uint64(63)) | (np.uint64(rid) << np.uint64(32)) | path[keep].astype(np.uint64)
    a[:, 1] = (np.uint64(K) << np.uint64(32)) | keep.astype(np.uint64)
    return (COMP[q][::-1] if rev else q), a


def region_of(a, qlen):
    r = np.zeros(1, chaindp.REG_DTYPE)
    n = len(a)
    x, y = (a[:, 0] & np.uint64(0xffffffff)).astype(np.int64), (a[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    rev = int(a[0, 0] >> np.uint64(63))
    r["cnt"], r["as"], r["rid"] = n, 0, int((a[0, 0] >> np.uint64(32)) & np.uint64(0x7fffffff))
    r["rs"], r["re"] = x[0] + 1 - K, x[-1] + 1
    r["qs"], r["qe"] = (qlen - (y[-1] + 1), qlen - (y[0] + 1 - K)) if rev else (y[0] + 1 - K, y[-1] + 1)
    r["mlen"] = r["blen"] = r["score"] = r["score0"] = K + int(np.minimum(np.diff(x), K).sum())
    r["bits"] = rev << 10
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_probe.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    targets = [rng.integers(0, 4, 200_000).astype(np.uint8) for _ in range(20)]
    seqs, anchors, regs = [], [], []
    while len(seqs) < args.reads:
        rid = int(rng.integers(0, len(targets)))
        q, a = make_read(rng, targets[rid], rid, 2000, 10000)
        if len(a) < 3:
            continue
        seqs.append(q); anchors.append(a); regs.append(region_of(a, len(q)))
    letters = np.frombuffer(b"ACGT", np.uint8)
    seq = letters[np.concatenate(seqs)]
    tseq = letters[np.concatenate(targets)]
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    a_off = np.concatenate([[0], np.cumsum([len(a) for a in anchors])]).astype(np.int64)
    t_off = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
    a, regs = np.concatenate(anchors), np.concatenate(regs)
    regs_off = np.arange(len(seqs) + 1, dtype=np.int64)
    opt = params.align_opt("map-ont")
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as dev:
        dev.align_set_targets(t_off, tseq)
        dev.set_profiling(True)
        walls, parts = [], []
        for it in range(6):
            t0 = time.perf_counter()
            out = dev.align1(opt, seq_off, seq, a_off, a, regs_off, regs, cigar_cap=int(seq_off[-1]))
            if it:
                walls.append((time.perf_counter() - t0) * 1e3); parts.append(dev.align_ms())
    _, r_out, r2, extra, coff, cig = out
    wall = statistics.median(walls)
    ms = {k: statistics.median(p[k] for p in parts) for k in parts[0]}
    dev_ms = sum(ms.values())
    aligned = int((r_out["qe"] - r_out["qs"])[extra["has_extra"] == 1].sum())
    res = dict(probe="align_probe", reads=len(seqs), regions=len(regs), read_bases=int(seq_off[-1]), anchors=int(a_off[-1]), aligned_read_bases=aligned,
               split=int((r2["cnt"] > 0).sum()), cigar_words=int(coff[-1]), wall_ms_per_call=wall, regions_per_s=len(regs) / wall * 1e3,
               aligned_bases_per_s=aligned / wall * 1e3, device_ms=ms, device_ms_total=dev_ms,
               device_share={k: v / dev_ms for k, v in ms.items()}, bookkeeping_ms=wall - ms["dp"],
               reference_one_thread=dict(regions_per_s=6397, aligned_bases_per_s=3.63e6,
                                         note="tests/golden/make_align_golden.py over its own small scenes (reads of 150..1500 bases, min_ksw_len 40)"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{len(regs)} regions, {seq_off[-1]} read bases, {aligned} aligned: {wall:.1f} ms per call, {res['regions_per_s']:.0f} regions / s, "
          f"{res['aligned_bases_per_s'] / 1e6:.1f} M aligned bases / s")
    print("device ms: " + ", ".join(f"{k} {v:.2f} ({v / dev_ms * 100:.0f} %)" for k, v in ms.items()) + f"; the call minus its DP: {wall - ms['dp']:.1f} ms")


if __name__ == "__main__":
    main()
