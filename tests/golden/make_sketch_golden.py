#!/usr/bin/env python3
"""Generates tests/golden/sketch/*.npz: sequences and the minimizers the UNMODIFIED reference's collect_minimizers (map.c:87-99,
mm_sketch of sketch.c:77-143) makes of them, through oracle/_ref/mt_dump (`make -C oracle ref-dump`; build container only).  The
GPU box and the CPU test tier only read the committed .npz files.

Each file: seq uint8[*] (the bases as the reference's reader holds them, concatenated), seq_off int64[R+1], w, k, is_hpc,
mini_off int64[R+1], mini uint64[*,2].  mt_dump skips a read without minimizers, so such a read is recognised by the model
having none either and the reference's dump then not containing it (the read count and every qlen must still line up).

Inputs: the four FASTA under tests/golden/fa/, the seeded synthetic genome and 12 reads of make_seed_golden.synthetic_fasta()
(their minimizers are asserted equal to tests/golden/seeds/syn_repeats_*.npz), and a seeded trap set: ambiguous runs of 1..3 at every
phase within w+k of a 256-base tile boundary of the kernels, lower case and other letters, homopolymers above 255 bases, tandem repeats
with a period below w, the short lengths around k and w+k-1, sequences without any valid k-mer.
The generator asserts that the CPU model (tests/sketch_model.py) equals the reference on every read and that every emission
site / quirk the model reports fired in some file."""
import os
import random
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_seed_golden as msg          # noqa: E402
import sketch_model as sm               # noqa: E402

OUT = os.path.join(HERE, "sketch")
FA = os.path.join(HERE, "fa")
PRESETS = {"map-ont": (10, 15, 0), "ava-ont": (5, 15, 0), "map-pb": (10, 19, 1), "ava-pb": (5, 19, 1), "asm5": (19, 19, 0), "sr": (11, 21, 0)}
TILE = 256


def read_fasta(path):
    seqs = []
    for ln in open(path):
        if ln.startswith(">"):
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return ["".join(s).encode() for s in seqs]


def trap_fasta(path):
    rnd = random.Random(20261)

    def dna(n):
        return "".join(rnd.choice("ACGT") for _ in range(n))

    reads = []
    reach = max(w + k for w, k, _ in PRESETS.values())       # how far back the window / l of a slot look (38: asm5)
    for run in (1, 2, 3):                                     # ambiguous runs at every phase around a tile boundary, near it in reads of their own ...
        for ph in range(-4, 5):
            s = list(dna(420))
            s[TILE + ph:TILE + ph + run] = "N" * run
            reads.append("".join(s))
    for run in (1, 2, 3):                                     # ... and at every phase within the look-back's reach, one boundary after the other
        phases = list(range(-reach, reach + 1, 1 if run == 1 else 6))
        s = list(dna(TILE * (len(phases) + 1)))
        for i, ph in enumerate(phases):
            at = TILE * (i + 1) + ph
            s[at:at + run] = "N" * run
        reads.append("".join(s))
    for n_after in (0, 1, 2, 4, 9, 16, 22, 30):               # the sequence ends soon after an ambiguous base: the last minimum is a stale one
        reads.append(dna(70) + "N" + dna(n_after))
    reads.append("".join(c.lower() if rnd.random() < .5 else c for c in dna(300)))
    reads.append("".join(rnd.choice("NnRYKMSWryXx*-.") if rnd.random() < .04 else c for c in dna(500)).replace("T", "U", 20))
    for base, n in (("A", 256), ("C", 300), ("g", 700)):      # homopolymers above 255 bases (span >= 256 under compression)
        reads.append(dna(120) + base * n + dna(120))
    reads.append(dna(40) + "".join(c * rnd.randrange(1, 40) for c in dna(60)) + dna(40))
    for period, copies in ((1, 60), (2, 50), (3, 40), (5, 30), (7, 20), (9, 14)):   # identical k-mers inside one window
        reads.append(dna(60) + dna(period) * copies + dna(60))
    for period in (2, 3, 4, 5):                               # ... and inside the first window of a sequence / after an ambiguous base
        reads += [dna(period) * 24 + dna(50), dna(50) + "N" + dna(period) * 24 + dna(30)]
    lens = {1, 2}
    for w, k, _ in PRESETS.values():
        lens |= {k - 1, k, k + 1, w + k - 2, w + k - 1, w + k, w + k + 1}
    for n in sorted(lens):
        reads += [dna(n), dna(n)]
    reads += ["N" * 50, "N", (dna(9) + "N") * 12, "n" * 3 + dna(14) + "*" + dna(14)]          # no valid k-mer at all
    open(path, "w").write("".join(">t%03d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    return path


def make(name, preset, query, traps, check_seed_fixture=None, target=None):
    w, k, hpc = PRESETS[preset]
    a_path, s_path = f"/tmp/sketchgold_{name}.dump", f"/tmp/sketchgold_{name}.seed"
    subprocess.run([msg.DUMP, preset, target or os.path.join(FA, "MT-human.fa"), query, a_path, s_path], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    _, _, _, dumped = msg.read_seed_dump(s_path)
    seqs = read_fasta(query)
    seq = np.frombuffer(b"".join(seqs), np.uint8)
    seq_off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    minis, it, n_empty = [], iter(dumped), 0
    for s in seqs:
        x, y = sm.sketch(s, w, k, hpc, TILE, traps)
        if len(x) == 0:                                       # the reference's dump has no record of such a read
            minis.append(np.zeros((0, 2), np.uint64)); n_empty += 1
            traps["no_minimizer_read"] = traps.get("no_minimizer_read", 0) + 1
            continue
        _, qlen, mv, _, _, _ = next(it)
        assert qlen == len(s), (name, qlen, len(s))
        assert np.array_equal(np.stack((x, y), 1), mv), f"{name}: the model differs from the reference on a read of {len(s)} bases"
        minis.append(mv)
    assert next(it, None) is None, f"{name}: the reference has minimizers for a read the model has none for"
    mini_off, mini = msg.cat(minis, 2)
    if check_seed_fixture:
        fx = np.load(os.path.join(HERE, "seeds", check_seed_fixture + ".npz"))
        n = len(fx["mini_off"]) - 1
        assert np.array_equal(mini_off[-n - 1:] - mini_off[-n - 1], fx["mini_off"]) and np.array_equal(mini[mini_off[-n - 1]:], fx["mini"]), check_seed_fixture
    np.savez_compressed(os.path.join(OUT, name + ".npz"), seq=seq, seq_off=seq_off, w=np.int32(w), k=np.int32(k), is_hpc=np.int32(hpc),
                        mini_off=mini_off, mini=mini)
    print(f"{name}: {preset} w={w} k={k} hpc={hpc} reads={len(seqs)} (without minimizers {n_empty}) bases={len(seq)} minimizers={len(mini)}")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    traps = {}
    make("mt_human_mapont", "map-ont", f"{FA}/MT-human.fa", traps)
    make("mt_human_avaont", "ava-ont", f"{FA}/MT-human.fa", traps)
    make("mt_orang_mappb", "map-pb", f"{FA}/MT-orang.fa", traps)
    make("q_inv_sr", "sr", f"{FA}/q-inv.fa", traps)
    make("q_inv_asm5", "asm5", f"{FA}/q-inv.fa", traps)
    make("t_inv_avapb", "ava-pb", f"{FA}/t-inv.fa", traps)
    tgt, reads = msg.synthetic_fasta()
    both = "/tmp/sketchgold_syn_all.fa"                       # the genome, then the 12 reads: the reads are the fixture's last 12 sequences
    open(both, "w").write(open(tgt).read() + open(reads).read())
    make("syn_repeats_mapont", "map-ont", both, traps, "syn_repeats_mapont", target=tgt)
    make("syn_repeats_avaont", "ava-ont", reads, traps, "syn_repeats_avaont", target=reads)
    make("syn_repeats_avapb", "ava-pb", reads, traps, "syn_repeats_avapb", target=reads)
    tf = trap_fasta("/tmp/sketchgold_traps.fa")
    for preset in PRESETS:
        make("traps_" + preset.replace("-", ""), preset, tf, traps)
    print(traps)
    # every site and quirk must have occurred somewhere, against the reference (final_stale_beats_fresh needs w >= k + 2, which no
    # preset has: the restatement tier of tests/test_sketch_cpu.py covers it)
    need = ("first_window_tie", "old_min_on_new_min", "min_left_window", "rescan_tie", "final", "pending_min_dropped", "final_is_stale",
            "span_ge_256_slot", "no_minimizer_read")
    missing = [n for n in need if traps.get(n, 0) == 0]
    assert not missing, missing
