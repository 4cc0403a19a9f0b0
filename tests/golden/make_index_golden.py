#!/usr/bin/env python3
"""Generates tests/golden/index/*.npz: targets and the index image the UNMODIFIED reference builds for them (mm_idx_gen, worker_post
and the FPGA image of index.c:603-720), through oracle/_ref/mt_dump (`make -C oracle ref-dump`), in the canonical form of
tests/index_build_model.py (key and value of empty slots zeroed: the reference writes heap garbage there).  Only the build container
can run this; the tests read the committed files.

Each fixture: seq (uint8, all targets concatenated), seq_off[n + 1], rank[n] (rank of each target's name in strcmp order), w, k, is_hpc,
img_B/H/V/P (canonical), mid_occ (the reference's, after mm_mapopt_update) and min_mid_occ (the preset's clamp, 0 where it has none).

  dense_mapont   24 x 5 kb random targets, names t168 ... so that rank != number; a 400-base unit in several targets on both strands and a
                 short tandem repeat (P holds words of several targets); more than 500 buckets whose table is expanded while it is built
  dense_avapb    the same smaller, homopolymer-compressed (k = 19, w = 5), with homopolymer runs; a unit occurs with stretched runs, so
                 that a group holds minimizers of different span
  heavy_buckets  tables larger than random input of committable size reaches: minimizers picked from a 2 Mb random sequence so that
                 buckets get 12, 13, 25, 26, 49 and 50 keys (the last size without and the first with an expansion, for 16, 32 and 64
                 slots), each emitted as a short target of its own (the minimizer's window with flanks)"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import index_build_model as ibm          # noqa: E402
import sketch_model as sm                # noqa: E402
from make_seed_golden import read_seed_dump   # noqa: E402

DUMP = os.path.join(ROOT, "oracle", "_ref", "mt_dump")
OUT = os.path.join(HERE, "index")
PRESETS = {"map-ont": (10, 15, 0, 0), "ava-ont": (5, 15, 0, 0), "ava-pb": (5, 19, 1, 0)}     # w, k, is_hpc, min_mid_occ (options.c:84-96)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s[::-1].translate(COMP)


def rand_seq(rs, n):
    return bytes(b"ACGT"[i] for i in rs.randint(0, 4, n))


def ranks(names):
    order = sorted(range(len(names)), key=lambda i: names[i].encode())
    rank = np.zeros(len(names), np.uint32)
    rank[order] = np.arange(len(names))
    return rank


def reference_image(name, preset, names, seqs):
    tgt, qry = f"/tmp/ixgold_{name}_t.fa", f"/tmp/ixgold_{name}_q.fa"
    with open(tgt, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + s + b"\n")
    with open(qry, "wb") as f:
        f.write(b">q0\n" + max(seqs, key=len)[:400] + b"\n")
    a_path, s_path = f"/tmp/ixgold_{name}.dump", f"/tmp/ixgold_{name}.seed"
    subprocess.run([DUMP, preset, tgt, qry, a_path, s_path], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    _, mid_occ, img, _ = read_seed_dump(s_path)
    return mid_occ, img


def key_counts(img):
    """{bucket: keys} of an image, and the buckets whose table was expanded while it was built (n_keys > upper of the first size)."""
    occ = ibm.occupied(img)
    out, grown = {}, 0
    for bk, N, h0, _ in ibm._tables(img):
        out[bk] = int(occ[h0:h0 + N].sum())
        grown += out[bk] > ibm.upper(ibm.first_size(out[bk]))
    return out, grown


def save(name, preset, names, seqs, check):
    w, k, is_hpc, min_mid_occ = PRESETS[preset]
    mid_occ, raw = reference_image(name, preset, names, seqs)
    img = ibm.canonical(raw)
    garbage = sum(int((np.asarray(a) != np.asarray(c)).sum()) for a, c in zip(raw, img))
    keys, grown = key_counts(img)
    check(img, keys, grown)
    seq_off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), seq=np.frombuffer(b"".join(seqs), np.uint8), seq_off=seq_off, rank=ranks(names),
                        w=np.int32(w), k=np.int32(k), is_hpc=np.int32(is_hpc), img_B=img[0], img_H=img[1], img_V=img[2], img_P=img[3],
                        mid_occ=np.int32(mid_occ), min_mid_occ=np.int32(min_mid_occ))
    print(f"{name}: {len(seqs)} targets, {int(seq_off[-1])} bases, {sum(keys.values())} distinct minimizers, {grown} buckets expanded, "
          f"most keys {max(keys.values())}, P words {len(img[3]) // 8}, mid_occ {mid_occ}, bytes changed by canonicalising {garbage}, "
          f"{os.path.getsize(os.path.join(OUT, name + '.npz')) >> 10} KB")


def p_rids(img):
    return np.unique(np.asarray(img[3], np.uint8).view(np.uint64) >> np.uint64(43))


def dense(name, preset, seed, n_seqs, length, hpc_runs):
    rs = np.random.RandomState(seed)
    unit, tand = rand_seq(rs, 400), rand_seq(rs, 37)
    if hpc_runs:                                    # homopolymer runs all over, and a second copy of the unit with its runs stretched
        def runs(s, lo, hi):
            return b"".join(bytes([c]) * int(rs.randint(lo, hi)) for c in s)
        unit2 = runs(unit, 1, 4)
        unit = runs(unit, 1, 3)
    seqs = []
    for i in range(n_seqs):
        s = bytearray(rand_seq(rs, length) if not hpc_runs else runs(rand_seq(rs, length // 2), 1, 4)[:length])
        if i % 4 == 0:
            at = int(rs.randint(0, len(s) - 900))
            u = unit if i % 8 == 0 else rc(unit)
            if hpc_runs and i % 3 == 0:
                u = unit2
            s[at:at + len(u)] = u
        if i == 5:
            s[1000:1000 + 37 * 12] = tand * 12
        seqs.append(bytes(s))
    names = ["t%d" % ((i * 23 + 168) % 211) for i in range(n_seqs)]
    assert len(set(names)) == n_seqs and (ranks(names) != np.arange(n_seqs)).any()

    def check(img, keys, grown):
        assert len(p_rids(img)) > 1, "P must hold words of more than one target"
        if not hpc_runs:
            assert grown >= 500, grown
        else:
            w, k, is_hpc, _ = PRESETS[preset]
            mini = ibm.minimizers(seqs, w, k, is_hpc)
            m, span = mini[:, 0] >> np.uint64(8), mini[:, 0] & np.uint64(255)
            o = np.argsort(m, kind="stable")
            m, span = m[o], span[o]
            assert ((m[1:] == m[:-1]) & (span[1:] != span[:-1])).any(), "no group with minimizers of different span"
    save(name, preset, names, seqs, check)


def heavy(name="heavy_buckets", preset="ava-ont", seed=31, wanted=(12, 13, 25, 26, 49, 50), per_count=3):
    w, k, is_hpc, _ = PRESETS[preset]
    rs = np.random.RandomState(seed)
    genome = rand_seq(rs, 2_000_000)
    x, y = sm.sketch(genome, w, k, is_hpc)
    m, pos = x >> np.uint64(8), (y & np.uint64(0xFFFFFFFF)) >> np.uint64(1)
    _, first = np.unique(m, return_index=True)                 # one occurrence of every distinct minimizer
    m, pos = m[first], pos[first].astype(np.int64)
    bucket = (m & np.uint64((1 << 14) - 1)).astype(np.int64)
    have = np.bincount(bucket, minlength=1 << 14)
    flank = 2 * (w + k)
    while True:
        taken, picks = set(), []
        for want in wanted:
            for bk in [b for b in np.argsort(-have).tolist() if have[b] >= want and b not in taken][:per_count]:
                taken.add(bk)
                picks += np.nonzero(bucket == bk)[0][:want].tolist()
        seqs = [genome[max(0, pos[i] - k + 1 - flank):pos[i] + 1 + flank] for i in picks]
        names = ["h%d" % ((i * 7 + 3) % (len(seqs) + 1)) for i in range(len(seqs))]
        if len(set(names)) != len(seqs):
            names = ["h%d" % (len(seqs) - i) for i in range(len(seqs))]
        _, img = reference_image(name, preset, names, seqs)
        keys, _ = key_counts(ibm.canonical(img))
        if set(wanted) <= set(keys.values()):
            break
        flank += w
        assert flank < 400, "the chosen minimizers do not survive in their excerpts"

    def check(img, keys, grown):
        assert set(wanted) <= set(keys.values()), sorted(set(keys.values()))
    save(name, preset, names, seqs, check)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    dense("dense_mapont", "map-ont", 7, 24, 5000, False)
    dense("dense_avapb", "ava-pb", 9, 12, 4000, True)
    heavy()
