"""CPU tier of the sketch: the model of csrc/chaindp_sketch.hip (tests/sketch_model.py) against what the reference emits.

Two tiers, and they are not worth the same:
  * preset tier -- pinned to the reference: every tests/golden/sketch/*.npz (written by tests/golden/make_sketch_golden.py from the
    unmodified reference's collect_minimizers) and the `mini` arrays of the older seed fixtures, sketched here from tests/golden/fa/.
  * restatement tier -- even k, w up to 255, w >= k + 2, the bytes 0..3 and multi-segment reads cannot be produced by the reference's
    dumper (its presets do not reach them).  There the model is held to `loop_sketch` below, a per-base loop with a ring of w
    entries written for this test from the loop's semantics: restatement against restatement, which shows that the parallel
    formulation equals the sequential one.  The reference's mm_sketch itself takes w, k and is_hpc as arguments, so where
    oracle/_ref/libmm2sketch_ref.so is built (tests/sketch_ref.py) the same inputs are also held to the unmodified reference,
    minimizer for minimizer.  Where it is not built, this tier is tied to the reference through the recorded results of the edge
    cases (tests/test_sketch_edge_shapes_cpu.py), which sit in the same region.
The model's tiled scans are also run with every tile size: the cut between tiles must never show."""
import glob
import os
import random

import numpy as np
import pytest

import sketch_model as sm
import sketch_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
SKETCH = sorted(glob.glob(os.path.join(HERE, "golden", "sketch", "*.npz")))
M64 = (1 << 64) - 1


def read_fasta(path):
    seqs = []
    for ln in open(path):
        if ln.startswith(">"):
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return ["".join(s).encode() for s in seqs]


def loop_sketch(seq, w, k, is_hpc):
    """One base at a time, a ring of the last w window entries, the current minimum and where it sits."""
    codes = [int(sm.NT4[b]) for b in bytes(seq)]
    n, mask, top = len(codes), (1 << 2 * k) - 1, 2 * (k - 1)
    ring = [(M64, M64)] * w
    cur, cur_at, at = (M64, M64), 0, 0
    fwd = rev = 0
    good = 0                       # window entries since the last ambiguous base
    runs = []                      # lengths of the last <= k runs (homopolymer compression)
    out = []
    i = 0
    while i < n:
        c, entry, take = codes[i], (M64, M64), True
        if c < 4:
            if is_hpc:
                j = i
                while j + 1 < n and codes[j + 1] == c:
                    j += 1
                runs.append(j - i + 1); runs = runs[-k:]
                span, i = sum(runs), j
            else:
                span = min(good + 1, k)
            fwd = ((fwd << 2) | c) & mask
            rev = (rev >> 2) | ((3 - c) << top)
            if fwd == rev:
                take = False           # no strand: no window entry, the ring does not advance
            else:
                good += 1
                if good >= k and span < 256:
                    strand = 0 if fwd < rev else 1
                    h = int(sm.hash64(np.array([rev if strand else fwd], np.uint64), mask)[0])
                    entry = ((h << 8 | span) & M64, i << 1 | strand)
        else:
            good, runs = 0, []
        if take:
            ring[at] = entry
            order = [(at + 1 + d) % w for d in range(w)]          # oldest .. newest (= at)
            if good == w + k - 1 and cur[0] != M64:
                out += [ring[j] for j in order[:-1] if ring[j][0] == cur[0] and ring[j][1] != cur[1]]
            if entry[0] <= cur[0]:
                if good >= w + k and cur[0] != M64:
                    out.append(cur)
                cur, cur_at = entry, at
            elif at == cur_at:
                if good >= w + k - 1 and cur[0] != M64:
                    out.append(cur)
                cur = (M64, M64)
                for j in order:
                    if ring[j][0] <= cur[0]:
                        cur, cur_at = ring[j], j
                if good >= w + k - 1 and cur[0] != M64:
                    out += [ring[j] for j in order if ring[j][0] == cur[0] and ring[j][1] != cur[1]]
            at = (at + 1) % w
        i += 1
    if cur[0] != M64:
        out.append(cur)
    a = np.array(out, np.uint64).reshape(-1, 2)
    return a[:, 0], a[:, 1]


def fuzz_seq(rnd, max_exp=3.3, alphabet="ACGT"):
    n = int(10 ** rnd.uniform(0, max_exp))
    long_runs = rnd.random() < .3
    s = []
    while len(s) < n:
        r = rnd.random()
        if r < 0.05:
            s += "N" * rnd.randrange(1, 4)
        elif r < 0.12:
            s += rnd.choice(alphabet) * rnd.randrange(2, 300 if long_runs else 9)
        elif r < 0.2:
            s += [rnd.choice(alphabet) for _ in range(rnd.randrange(1, 7))] * rnd.randrange(2, 30)
        elif r < 0.25:
            s += rnd.choice("acgtuURYn*\x00\x01\x02\x03")
        else:
            s += [rnd.choice(alphabet) for _ in range(rnd.randrange(1, 60))]
    return "".join(s[:n]).encode("latin1")


def test_fixtures_exist():
    assert len(SKETCH) >= 15
    assert {(int(z["w"]), int(z["k"]), int(z["is_hpc"])) for z in map(np.load, SKETCH)} == {(10, 15, 0), (5, 15, 0), (10, 19, 1), (5, 19, 1), (19, 19, 0), (11, 21, 0)}


@pytest.mark.parametrize("path", SKETCH, ids=lambda p: os.path.basename(p)[:-4])
def test_model_equals_reference_fixture(path):
    z = np.load(path)
    off, mini = sm.sketch_batch(z["seq"], z["seq_off"], int(z["w"]), int(z["k"]), int(z["is_hpc"]))
    assert np.array_equal(off, z["mini_off"])
    assert np.array_equal(mini, z["mini"])


@pytest.mark.parametrize("fixture,fa,w,k", [("mt_orang_vs_human_mapont", "MT-orang.fa", 10, 15), ("mt_human_self_avaont", "MT-human.fa", 5, 15),
                                            ("mt_human_vs_orang_avaont", "MT-human.fa", 5, 15), ("inv_mapont", "q-inv.fa", 10, 15), ("inv_sr", "q-inv.fa", 11, 21)])
def test_model_equals_seed_fixture_minimizers(fixture, fa, w, k):
    fx = np.load(os.path.join(HERE, "golden", "seeds", fixture + ".npz"))
    seqs = read_fasta(os.path.join(HERE, "golden", "fa", fa))
    seq = np.frombuffer(b"".join(seqs), np.uint8)
    off, mini = sm.sketch_batch(seq, np.cumsum([0] + [len(s) for s in seqs]), w, k, 0)
    assert np.array_equal(off, fx["mini_off"]) and np.array_equal(mini, fx["mini"])


@pytest.mark.parametrize("tile", [64, 128, 256, 512, 1024])
def test_tile_cut_never_shows(tile):
    for path in SKETCH:
        if "traps" not in path and "t_inv" not in path:
            continue
        z = np.load(path)
        off, mini = sm.sketch_batch(z["seq"], z["seq_off"], int(z["w"]), int(z["k"]), int(z["is_hpc"]), tile=tile)
        assert np.array_equal(off, z["mini_off"]) and np.array_equal(mini, z["mini"]), (path, tile)


def test_quirks_occur_in_the_fixtures():
    traps = {}
    for path in SKETCH:
        z = np.load(path)
        sm.sketch_batch(z["seq"], z["seq_off"], int(z["w"]), int(z["k"]), int(z["is_hpc"]), traps=traps)
        lens = np.diff(z["seq_off"]); w, k = int(z["w"]), int(z["k"])
        if "traps" in path:
            assert {k - 1, w + k - 2, w + k - 1, w + k} <= set(lens.tolist()), path
            assert (np.diff(z["mini_off"]) == 0).any(), path                       # a read without any minimizer
    for name in ("first_window_tie", "old_min_on_new_min", "min_left_window", "rescan_tie", "final", "pending_min_dropped", "final_is_stale", "span_ge_256_slot"):
        assert traps.get(name, 0) > 0, (name, traps)


def test_restatement_tier_model_equals_per_base_loop():
    rnd = random.Random(3)
    traps = {}
    for it in range(400):
        s = fuzz_seq(rnd)
        w = rnd.choice([1, 2, 3, 5, 10, 19, 40, 255]); k = rnd.choice([1, 2, 3, 4, 6, 8, 15, 16, 19, 28]); hpc = rnd.random() < .5
        x, y = sm.sketch(s, w, k, hpc, tile=rnd.choice([64, 256, 1024]), traps=traps)
        lx, ly = loop_sketch(s, w, k, hpc)
        assert np.array_equal(x, lx) and np.array_equal(y, ly), (it, len(s), w, k, hpc)
        if sr.have():
            assert np.stack((x, y), 1).tobytes() == sr.sketch(s, w, k, hpc).tobytes(), (it, len(s), w, k, hpc)
    for name in ("symmetric_skipped", "final_stale_beats_fresh", "span_ge_256_slot", "first_window_tie", "rescan_tie"):
        assert traps.get(name, 0) > 0, (name, traps)


def test_restatement_tier_multi_segment_reads():
    rnd = random.Random(8)
    seqs = [fuzz_seq(rnd, 2.6) for _ in range(9)]
    segs = [2, 1, 3, 1, 2]
    seq = np.frombuffer(b"".join(seqs), np.uint8); seq_off = np.cumsum([0] + [len(s) for s in seqs])
    off, mini = sm.sketch_batch(seq, seq_off, 5, 15, 0, n_segs_per_read=segs)
    want, q = [], 0
    for ns in segs:
        shift = 0
        for rid in range(ns):
            x, y = loop_sketch(seqs[q], 5, 15, 0)
            want.append(np.stack((x, y + np.uint64((rid << 32) + (shift << 1))), 1)); shift += len(seqs[q]); q += 1
    assert np.array_equal(mini, np.concatenate(want)) and off[-1] == len(mini) and len(off) == len(segs) + 1
    if sr.have():
        r_off, r_mini = sr.sketch_batch(seq, seq_off, 5, 15, 0, n_segs_per_read=segs)
        assert np.array_equal(off, r_off) and mini.tobytes() == r_mini.tobytes()
