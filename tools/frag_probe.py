#!/usr/bin/env python3
"""What the paired-read path costs on the GPU (chaindp_map_frag_seqs: sketch, seed collection, chain DP, backtrack, mm_gen_regs and the
fragment post steps of csrc/chaindp_frag.hip) on the shape it is built for: a seeded `sr` batch of about a million 2 x 150 bp
fragments (5 % orphans) drawn from the targets of tests/frag_model.py's scenario, mates reverse-complemented as a sequencer reports
them, mapped with pe_ori = 1.

Prints the wall time of a call, the hits, how many fragments had more hits than the kernels' LDS fast path keeps (FRAG_LDS_CAP), and
the bytes per fragment that cross PCIe on the way back now (offsets, 80 B per final hit, rep_len) against before (80 B per
mm_gen_regs hit plus 16 B per chain anchor, for the host's pe.c / hit.c).  Per-kernel times come from one
  rocprofv3 --kernel-trace --stats -- python tools/frag_probe.py
run; give it before = 0, so that the call's own kernels are the only ones in the trace (the "before" figure downloads the resident
chains through chaindp_backtrack).  The last line printed is the same record as JSON.
  python tools/frag_probe.py [n_frags=1000000] [calls=2] [before=1]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frag_model as fm  # noqa: E402
from minimap2_chaindp_amd import chaindp  # noqa: E402

n_frags = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
want_before = int(sys.argv[3]) if len(sys.argv) > 3 else 1
L, LDS_CAP = 150, 64

sc = fm.scenario(n_frags=16, seed=1)                                  # its targets, index and parameters
rng = np.random.default_rng(20261017)
comp = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    comp[a] = b
tgt = [np.frombuffer(t, np.uint8) for t in sc.targets]
which = rng.integers(0, len(tgt), n_frags)
ins = rng.integers(L, 500, n_frags)
orphan = rng.random(n_frags) < 0.05
m1 = np.empty((n_frags, L), np.uint8)
m2 = np.empty((n_frags, L), np.uint8)
col = np.arange(L)
for t, g in enumerate(tgt):
    sel = np.nonzero(which == t)[0]
    s0 = rng.integers(0, len(g) - 600, len(sel))
    m1[sel] = g[s0[:, None] + col]
    m2[sel] = comp[g[(s0 + ins[sel] - L)[:, None] + col]][:, ::-1]    # the right end, reverse-complemented
for m in (m1, m2):                                                    # 2 % substitutions
    hit = rng.random(m.shape) < 0.02
    m[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
swap = rng.random(n_frags) < 0.5                                      # half the fragments from the other strand
m1[swap], m2[swap] = m2[swap].copy(), m1[swap].copy()
ns = np.where(orphan, 1, 2).astype(np.int32)
rows = np.stack([m1, m2], 1).reshape(-1, L)[np.stack([np.ones(n_frags, bool), ~orphan], 1).reshape(-1)]
seq = np.ascontiguousarray(rows).reshape(-1)
seq_off = (np.arange(len(rows) + 1, dtype=np.int64) * L)
bid = rng.integers(0, 1 << 10, size=n_frags, dtype=np.uint32)
hash_ = rng.integers(0, 1 << 32, size=n_frags, dtype=np.uint64).astype(np.uint32)
print(f"{n_frags} fragments, {len(rows)} segments, {len(seq)} bases")

with chaindp.Device(0, max_anchors=max(1 << 22, n_frags * 160), max_reads=n_frags + 16) as dev:
    ix = dev.load_index(sc.image())

    def call():
        return dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, bid, hash_, sc.ref_len,
                                 pe_ori=1, regs_cap=6 * n_frags)

    soff, regs, rep, n_anchors = call()                               # warm-up: buffers grow, code objects load
    t0 = time.perf_counter()
    for _ in range(calls):
        soff, regs, rep, n_anchors = call()
    wall = (time.perf_counter() - t0) / calls
    now = 8 * len(soff) + 80 * len(regs) + 4 * n_frags
    out = {"probe": "frag_probe", "fragments": n_frags, "segments": len(rows), "bases": len(seq), "calls": calls, "wall_ms_per_call": wall * 1e3,
           "fragments_per_s": n_frags / wall, "anchors": int(n_anchors), "final_hits": len(regs), "lds_cap": LDS_CAP,
           "bytes_back_per_fragment_now": now / n_frags}
    print(f"map_frag_seqs: {wall * 1e3:.1f} ms per call ({n_frags / wall / 1e6:.2f} M fragments/s), {n_anchors} anchors, {len(regs)} final per-segment hits")
    if want_before:
        coff, u, boff, b = dev.backtrack(sc.par, sc.min_cnt)          # the resident chains of the last call: what went back before
        n_hits0 = np.diff(coff)
        before = 8 * len(coff) + 80 * int(coff[-1]) + 8 * len(boff) + 16 * int(boff[-1])
        out.update({"hits_before_post": int(coff[-1]), "chain_anchors": int(boff[-1]), "fragments_above_lds_cap": int((n_hits0 > LDS_CAP).sum()),
                    "most_hits_on_a_fragment": int(n_hits0.max()), "bytes_back_per_fragment_before": before / n_frags})
        print(f"{int(coff[-1])} hits and {int(boff[-1])} chain anchors before the post steps")
        print(f"fragments above the LDS cap of {LDS_CAP} hits: {int((n_hits0 > LDS_CAP).sum())} of {n_frags} (most hits on one fragment: {int(n_hits0.max())})")
        print(f"bytes back over PCIe per fragment: {now / n_frags:.1f} now, {before / n_frags:.1f} before ({before / now:.1f}x)")
    print(json.dumps(out))
