#!/usr/bin/env python3
"""What chain_post + mm_est_err + mm_set_mapq cost on the GPU (chaindp_chain_post, csrc/chaindp_post.hip), against what they save (the
80 B/hit download of chaindp_gen_regs) and against the reference's hit.c steps on one host core.

  1. map-ont generator preset at BASELINE configs[2] size (9 400 reads, as bench.py's map-ont job): upload -> DP -> backtrack -> gen_regs
     resident, then chaindp_gen_regs with its download and chaindp_chain_post timed, each over `calls` calls
  2. the reference's all-vs-all dump repeated as tools/map_batch_probe.py does: chaindp_map_reads against chaindp_map_batch
  3. the reference's mm_set_parent / mm_select_sub / mm_join_long / mm_set_mapq (oracle/_ref, where it is built) over the hits of (1),
     one read at a time from Python on one core (ctypes overhead included), for comparison
Kernel times come from one `rocprofv3 --kernel-trace --stats -- python tools/post_probe.py` run.
  python tools/post_probe.py [calls] [n_reads]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from minimap2_chaindp_amd import anchorgen, chaindp, params  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 9400


def timed(fn, n):
    fn()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    return (time.perf_counter() - t0) / n, out


# 1. generator preset
par = params.preset("map-ont")
opt = params.post_preset("map-ont")
off, a = anchorgen.generate("map-ont", n_reads=n_reads, seed=11)
qlen = np.full(n_reads, 10000, np.int32)
hash_ = (np.arange(n_reads, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
rep = np.zeros(n_reads, np.int32)
with chaindp.Device(0, max_anchors=len(a) + 1024, max_reads=n_reads + 1) as d:
    d.upload(off, a)
    d.run_full(par)
    coff, u, boff, b = d.backtrack(par, 3)
    n_hits = int(coff[-1])
    regs_in = d.gen_regs(hash_, qlen, n_hits)
    ref_len = np.full(int(regs_in["rid"].max()) + 1 if n_hits else 1, 1 << 30, np.int32)
    t_gen, _ = timed(lambda: d.gen_regs(hash_, qlen, n_hits), calls)
    # without mini_pos (the generator has none): chain_post + mm_set_mapq, mm_est_err skipped (is_sr = 1 skips it, the rest is the same)
    opt_nodiv = params.post_preset("map-ont", is_sr=1)
    t_post, (roff, regs) = timed(lambda: d.chain_post(opt_nodiv, ref_len, qlen=qlen, rep_len=rep), calls)
print(f"map-ont generator: {n_reads} reads, {len(a)} anchors, {n_hits} hits in, {int(roff[-1])} out")
print(f"  chaindp_gen_regs (kernels + {n_hits * 80 / 1e6:.1f} MB download): {t_gen * 1e3:.2f} ms")
print(f"  chaindp_chain_post (kernels + download of {int(roff[-1]) * 80 / 1e6:.1f} MB): {t_post * 1e3:.2f} ms, "
      f"{n_hits / t_post / 1e6:.1f} M hits/s")

# 1b. a repeat-rich read on k_post_read's global-memory path where mm_set_parent's union costs the most: 1 000 short primaries (5 anchors,
# 80 bp apart on the query) and 2 000 weaker long hits (4 anchors 4.9 kb apart) laid over them, each overlapping ~190 primaries
import post_shapes  # noqa: E402
rng = np.random.default_rng(5)
tiles = [post_shapes._chain(int(t), 1000, 100 + 80 * t, 5) for t in range(1000)]
longs = [post_shapes._chain(2000 + h, 1000, 100 + int(rng.integers(0, 60000)), 4, step=4900) for h in range(2000)]
ta, tq, tmp, _ = post_shapes._read(tiles + longs, 90000)
toff = np.array([0, len(ta)], np.int64)
with chaindp.Device(0, max_anchors=len(ta) + 1024, max_reads=2) as d:
    d.upload(toff, ta)
    d.run_full(par)
    tco, _, _, _ = d.backtrack(par, 3)
    d.gen_regs(np.zeros(1, np.uint32), np.array([tq], np.int32), int(tco[-1]))
    trl = np.full(4096, 1 << 30, np.int32)
    t_tiles, (troff, _) = timed(lambda: d.chain_post(opt_nodiv, trl, qlen=np.array([tq], np.int32), rep_len=np.zeros(1, np.int32)), calls)
print(f"one read of {int(tco[-1])} hits (1 000 tiles + 2 000 long hits over them): chaindp_chain_post {t_tiles * 1e3:.2f} ms, "
      f"{int(troff[-1])} hits out")

# 2. all-vs-all dump, as tools/map_batch_probe.py
big = os.path.join(ROOT, "tests", "golden", "_big", "big_avaont.npz")
path = big if os.path.exists(big) else os.path.join(ROOT, "tests", "golden", "seeds", "syn_repeats_avaont.npz")
g = np.load(path, allow_pickle=False)
pv = [int(x) for x in g["params"]]
par2 = params.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
mult = max(1, int(24_000_000 // max(len(g["anchors"]), 1)))
mini_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(g["mini_off"]), mult))]).astype(np.int64)
mini, bid, ql2 = np.tile(g["mini"], (mult, 1)), np.tile(g["bid"], mult), np.tile(g["qlen"], mult)
R2 = len(bid)
h2 = (np.arange(R2, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
cap_a = len(g["anchors"]) * mult + 1024
with chaindp.Device(0, max_anchors=cap_a, max_reads=R2 + 1) as d:
    ix = d.load_index([g["img_B"], g["img_H"], g["img_V"], g["img_P"]])
    rl2 = np.full(1 << 16, 1 << 30, np.int32)
    t_mb, (mroff, _, _, na) = timed(lambda: d.map_batch(ix, int(g["flag"]), int(g["mid_occ"]), par2, pv[7], mini_off, mini, bid, ql2, h2,
                                                        regs_cap=cap_a // 8), calls)
    t_mr, (rroff, _, _, _) = timed(lambda: d.map_reads(ix, int(g["flag"]), int(g["mid_occ"]), par2, pv[7], params.post_preset("ava-ont"), mini_off,
                                                       mini, bid, ql2, h2, rl2, regs_cap=cap_a // 8), calls)
print(f"{os.path.basename(path)} x{mult}: {R2} reads, {na} anchors, {int(mroff[-1])} hits")
print(f"  chaindp_map_batch: {t_mb * 1e3:.2f} ms;  chaindp_map_reads (ava-ont): {t_mr * 1e3:.2f} ms")

# 3. the reference's hit.c steps on one core, over the hits of (1)
try:
    import oracle_lib as ol
    import post_oracle as po
    have = ol.have_ref()
except Exception:                                                         # noqa: BLE001
    have = False
if have:
    od = po.opt_dict(opt_nodiv)
    t0 = time.perf_counter()
    for r in range(n_reads):
        po.ref_post_read(od, int(qlen[r]), 0, ref_len, regs_in[coff[r]:coff[r + 1]], b[boff[r]:boff[r + 1]], np.zeros(0, np.uint64))
    t_ref = time.perf_counter() - t0
    print(f"  reference hit.c steps, one host core through ctypes: {t_ref * 1e3:.1f} ms ({n_hits / t_ref / 1e6:.2f} M hits/s)")
else:
    print("  reference hit.c steps: oracle/_ref not built, not measured")
