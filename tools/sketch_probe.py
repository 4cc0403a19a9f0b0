"""Bases in, hits out against minimizers in, hits out: chaindp_map_seqs (the GPU sketches) and chaindp_map_reads given the
reference's minimizers ready-made in host memory (the caller sketched, which is not charged), on the same batch, alternating, from
pageable and from pinned input.  The batches are the syn_repeats_avaont / syn_repeats_mapont reads tiled to about the 24 M anchors
tools/map_probe.py uses, with the same index images.  Also the sketch alone: device time of its kernels, bases/s, and bytes/s
against the algorithmic 1 B + 16 B x minimizers per base.  One JSON line.
   python3 tools/sketch_probe.py [repeats=9] [target_anchors=24000000]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minimap2_chaindp_amd import chaindp, params  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
target = int(sys.argv[2]) if len(sys.argv) > 2 else 24_000_000
GOLD = os.path.join(ROOT, "tests", "golden")


def stats(ts):
    """spread_s = max - min; trimmed_spread_s leaves out the single slowest repeat (one stall of a shared host must not widen the
    margin the comparison is judged by)."""
    srt = sorted(ts)
    return {"median_s": statistics.median(ts), "min_s": srt[0], "max_s": srt[-1], "spread_s": srt[-1] - srt[0],
            "trimmed_spread_s": (srt[-2] if len(srt) > 2 else srt[-1]) - srt[0], "n": len(ts)}


def pin(keep, x):
    pa = chaindp.PinnedArray(x.shape, x.dtype); pa.array[...] = x; keep.append(pa)
    return pa.array


def probe(name, preset):
    g = np.load(os.path.join(GOLD, "seeds", name + ".npz"), allow_pickle=False)
    z = np.load(os.path.join(GOLD, "sketch", name + ".npz"), allow_pickle=False)
    R0 = len(g["qlen"])
    first = len(z["seq_off"]) - 1 - R0                                   # the reads are the last sequences of the sketch fixture
    seq0 = z["seq"][z["seq_off"][first]:]
    assert np.array_equal(np.diff(z["seq_off"][first:]), g["qlen"])
    w, k, hpc = int(z["w"]), int(z["k"]), int(z["is_hpc"])
    pv = [int(x) for x in g["params"]]
    par = params.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    opt = params.post_preset(preset)
    mult = max(1, target // max(len(g["anchors"]), 1))
    mini_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(g["mini_off"]), mult))]).astype(np.int64)
    mini = np.ascontiguousarray(np.tile(g["mini"], (mult, 1)), np.uint64)
    bid, qlen = np.tile(g["bid"], mult).astype(np.uint32), np.tile(g["qlen"], mult).astype(np.int32)
    seq = np.tile(seq0, mult)
    seq_off = np.concatenate([[0], np.cumsum(qlen.astype(np.int64))])
    n_reads = len(bid)
    hash_ = (np.arange(n_reads, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    ref_len = np.full(1 << 16, 1 << 20, np.int32)
    cap_a = len(g["anchors"]) * mult + 1024
    n_chunks = int(((qlen.astype(np.int64) + 255) // 256).sum())
    out = {"batch": name, "w": w, "k": k, "reads": n_reads, "bases": int(len(seq)), "minimizers": int(mini_off[-1]),
           "minimizers_per_base": float(mini_off[-1]) / len(seq),
           "upload_bytes_per_read": {"map_reads": (16 * int(mini_off[-1]) + n_reads * (8 + 4 + 4 + 4)) / n_reads,
                                     "map_seqs": (len(seq) + n_reads * (8 + 4 + 4 + 4 + 8) + 4 * n_chunks) / n_reads}}
    with chaindp.Device(0, max_anchors=cap_a, max_reads=n_reads + 1) as d:
        ix = d.load_index([g["img_B"], g["img_H"], g["img_V"], g["img_P"]])
        for pinned in (0, 1):
            keep = []
            if pinned:
                a_mini_off, a_mini, a_bid, a_qlen, a_seq, a_seq_off = (pin(keep, x) for x in (mini_off, mini, bid, qlen, seq, seq_off))
            else:
                a_mini_off, a_mini, a_bid, a_qlen, a_seq, a_seq_off = mini_off, mini, bid, qlen, seq, seq_off
            reads = lambda: d.map_reads(ix, int(g["flag"]), int(g["mid_occ"]), par, pv[7], opt, a_mini_off, a_mini, a_bid, a_qlen, hash_, ref_len, regs_cap=cap_a // 8)  # noqa: E731
            seqs = lambda: d.map_seqs(ix, w, k, hpc, int(g["flag"]), int(g["mid_occ"]), par, pv[7], opt, a_seq, a_seq_off, a_bid, hash_, ref_len, regs_cap=cap_a // 8)  # noqa: E731
            want, got = reads(), seqs()                                     # warm-up, and the two paths must agree
            assert np.array_equal(want[0], got[0]) and want[1].tobytes() == got[1].tobytes() and want[3] == got[3]
            reads(); seqs()
            tr, ts = [], []
            for _ in range(repeats):                                        # alternating: both see the same machine
                t0 = time.perf_counter(); reads(); tr.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); seqs(); ts.append(time.perf_counter() - t0)
            sr, ss = stats(tr), stats(ts)
            out["pinned" if pinned else "pageable"] = {
                "anchors": int(want[3]), "hits": int(want[0][-1]), "map_reads": sr, "map_seqs": ss,
                "map_seqs_minus_map_reads_s": ss["median_s"] - sr["median_s"],
                "not_slower_beyond_map_reads_spread": bool(ss["median_s"] - sr["median_s"] <= sr["trimmed_spread_s"])}
            for pa in keep:
                pa.free()
        # the sketch alone (pageable input): wall time of the call, device time of its kernels and scans
        d.set_profiling(True)
        d.sketch(w, k, hpc, seq, seq_off); d.sketch_ms(reset=True)
        tw = []
        for _ in range(repeats):
            t0 = time.perf_counter(); d.sketch(w, k, hpc, seq, seq_off); tw.append(time.perf_counter() - t0)
        ms, calls = d.sketch_ms(reset=True)
        d.set_profiling(False)
        # one verdict per batch, from the input whose map_reads measurement is the tighter one
        tight = min(("pageable", "pinned"), key=lambda m: out[m]["map_reads"]["trimmed_spread_s"])
        out["not_slower_beyond_map_reads_spread"] = out[tight]["not_slower_beyond_map_reads_spread"]
        kern_s = ms / calls / 1e3
        out["sketch"] = {"call": stats(tw), "kernels_ms": ms / calls, "bases_per_s": len(seq) / kern_s,
                         "algorithmic_bytes_per_s": (len(seq) + 16 * int(mini_off[-1])) / kern_s}
    return out


if __name__ == "__main__":
    print(json.dumps({"probe": "sketch_probe", "repeats": repeats,
                      "batches": [probe("syn_repeats_avaont", "ava-ont"), probe("syn_repeats_mapont", "map-ont")]}))
