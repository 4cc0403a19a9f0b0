#!/usr/bin/env python3
"""Rates of chaindp_ksw_extd on one MI355X: cell updates per second (cells inside the band [st0, en0] of every diagonal, as the
reference counts its work) for three batches --
  gap_fills   20 000 problems of 50..400 bases a side, w = 751 (map-ont's bw * 1.5 + 1: no band at these sizes), exact maximum;
  extensions   2 000 problems of 1..3 kb a side at w = 500, KSW_EZ_EXTZ_ONLY, zdrop 400;
  mix          both in one call --
each with CIGAR and score-only.  One warm-up call, then the median of five.  Per call: the host clock around the whole synchronous
call (checks, planning, copies over PCIe both ways, kernels) and the DP kernel alone (device events), so the copies and the host's
share show as the difference.  Writes profiles/ksw_probe.json and prints the table of DESIGN.md 8.

  python tools/ksw_probe.py [--scale 1.0] [--out profiles/ksw_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minimap2_chaindp_amd import chaindp  # noqa: E402

SCORING = (2, 4, 4, 2, 24, 1)           # map-ont


def relative(rng, q, tlen):
    """A target of tlen related to q: 8 % substitutions, a few bases dropped or added."""
    t = q.copy()
    hit = rng.random(len(t)) < 0.08
    t[hit] = (t[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    t = np.delete(t, rng.integers(0, len(t), max(1, len(t) // 50)))
    t = np.insert(t, rng.integers(0, len(t), max(1, len(t) // 50)), rng.integers(0, 4, max(1, len(t) // 50)))
    return np.concatenate([t[:tlen], rng.integers(0, 4, max(0, tlen - len(t)))]).astype(np.uint8)


def batch(rng, n, lo, hi, w, zdrop, flag):
    ql, tl = rng.integers(lo, hi + 1, n), rng.integers(lo, hi + 1, n)
    seqs = []
    for i in range(n):
        q = rng.integers(0, 4, int(ql[i])).astype(np.uint8)
        seqs += [q, relative(rng, q, int(tl[i]))]
    lens = np.array([len(s) for s in seqs], np.int64)
    beg = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return dict(bases=np.concatenate(seqs), q_beg=beg[0::2], q_len=ql.astype(np.int32), t_beg=beg[1::2], t_len=tl.astype(np.int32),
                w=np.full(n, w, np.int32), zdrop=np.full(n, zdrop, np.int32), end_bonus=np.full(n, -1, np.int32), flag=np.full(n, flag, np.int32))


def merge(a, b):
    out = {k: np.concatenate([a[k], b[k]]) for k in a if k != "bases"}
    out["bases"] = np.concatenate([a["bases"], b["bases"]])
    out["q_beg"][len(a["q_beg"]):] += len(a["bases"])
    out["t_beg"][len(a["t_beg"]):] += len(a["bases"])
    return out


def cells(b):
    """Cells inside the band over all diagonals of all problems."""
    total = 0
    for ql, tl, w in zip(b["q_len"].tolist(), b["t_len"].tolist(), b["w"].tolist()):
        w = max(ql, tl) if w < 0 else w
        r = np.arange(ql + tl - 1)
        st = np.maximum(np.maximum(0, r - ql + 1), (r - w + 1) >> 1)
        en = np.minimum(np.minimum(tl - 1, r), (r + w) >> 1)
        total += int(np.maximum(0, en - st + 1).sum())
    return total


def measure(dev, b, score_only, reps):
    flag = b["flag"] | (1 if score_only else 0)
    args = (b["bases"], b["q_beg"], b["q_len"], b["t_beg"], b["t_len"], SCORING, b["w"], b["zdrop"], b["end_bonus"], flag)
    ez, off, _ = dev.ksw_extd(*args)                       # warm-up
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev.ksw_extd(*args)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(dev.ksw_ms())
    routes = np.bincount(dev.ksw_route(len(ez)), minlength=3).tolist()
    return dict(call_ms=[round(x, 3) for x in wall], kernel_ms=[round(x, 3) for x in kern], call_median_ms=round(statistics.median(wall), 3),
                kernel_median_ms=round(statistics.median(kern), 3), cigar_words=int(off[-1]), zdropped=int(ez[:, 1].sum()),
                routes=dict(zip(("none", "lds", "global"), routes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the problem counts (rehearsals)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksw_probe.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    fills = batch(rng, max(1, int(20000 * a.scale)), 50, 400, 751, 400, 0)
    exts = batch(rng, max(1, int(2000 * a.scale)), 1000, 3000, 500, 400, 0x40)
    batches = {"gap_fills": fills, "extensions": exts, "mix": merge(fills, exts)}
    res = dict(probe="ksw_probe", lib=os.path.basename(chaindp.LIB_PATH), scoring=list(SCORING), repetitions=a.reps, batches={})
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as dev:
        dev.set_profiling(True)
        for name, b in batches.items():
            n_cells = cells(b)
            rec = dict(problems=len(b["q_len"]), bases=int(len(b["bases"])), cells=n_cells)
            for mode, so in (("cigar", False), ("score_only", True)):
                m = measure(dev, b, so, a.reps)
                m["kernel_gcups"] = round(n_cells / m["kernel_median_ms"] / 1e6, 2)
                m["call_gcups"] = round(n_cells / m["call_median_ms"] / 1e6, 2)
                m["copies_and_host_ms"] = round(m["call_median_ms"] - m["kernel_median_ms"], 3)
                rec[mode] = m
            rec["device_bytes"] = dev.device_bytes()
            res["batches"][name] = rec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| batch | problems | cells | mode | call ms | kernel ms | copies + host ms | kernel G cells/s | call G cells/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, rec in res["batches"].items():
        for mode in ("cigar", "score_only"):
            m = rec[mode]
            print(f"| {name} | {rec['problems']} | {rec['cells']} | {mode} | {m['call_median_ms']} | {m['kernel_median_ms']} | {m['copies_and_host_ms']} | "
                  f"{m['kernel_gcups']} | {m['call_gcups']} |")


if __name__ == "__main__":
    main()
