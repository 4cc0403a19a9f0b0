"""GPU tier: mm_sketch on the GPU (csrc/chaindp_sketch.hip; chaindp_sketch, chaindp_download_minimizers, chaindp_map_seqs).
(a) every tests/golden/sketch fixture (the unmodified reference's minimizers) byte for byte, one batch per file and one per
(w, k, hpc); (b) seeded fuzz against the CPU model, even k and w up to 255 included; (c) bases in, hits out equals minimizers in,
hits out on the seed fixtures, and the resident minimizers feed chaindp_collect_seeds; (d) a refused batch leaves the context
usable; (e) a sketch drops the batch that was resident: its downloads are refused, never answered with the new batch's data."""
import glob
import os
import random

import numpy as np
import pytest

import sketch_model as sm
from minimap2_chaindp_amd import chaindp, params as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SKETCH = sorted(glob.glob(os.path.join(HERE, "golden", "sketch", "*.npz")))
SEEDS = os.path.join(HERE, "golden", "seeds")
FA = os.path.join(HERE, "golden", "fa")


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 22, max_reads=1 << 13) as d:
        yield d


def read_fasta(path):
    seqs = []
    for ln in open(path):
        if ln.startswith(">"):
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return ["".join(s).encode() for s in seqs]


def batch(seqs):
    return np.frombuffer(b"".join(seqs), np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)


# ---- (a) the reference's minimizers

@pytest.mark.parametrize("path", SKETCH, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_byte_for_byte(dev, path):
    z = np.load(path)
    off = dev.sketch(int(z["w"]), int(z["k"]), int(z["is_hpc"]), z["seq"], z["seq_off"])
    assert np.array_equal(off, z["mini_off"])
    assert dev.download_minimizers().tobytes() == np.ascontiguousarray(z["mini"]).tobytes()


def test_fixtures_of_one_parameter_set_in_one_batch(dev):
    groups = {}
    for path in SKETCH:
        z = np.load(path)
        groups.setdefault((int(z["w"]), int(z["k"]), int(z["is_hpc"])), []).append(z)
    assert len(groups) == 6
    for (w, k, hpc), zs in groups.items():
        seq = np.concatenate([z["seq"] for z in zs])
        seq_off = np.concatenate([[0]] + [z["seq_off"][1:] + b for z, b in zip(zs, np.cumsum([0] + [len(z["seq"]) for z in zs]))])
        want_off = np.concatenate([[0]] + [z["mini_off"][1:] + b for z, b in zip(zs, np.cumsum([0] + [len(z["mini"]) for z in zs]))])
        off = dev.sketch(w, k, hpc, seq, seq_off)
        assert np.array_equal(off, want_off), (w, k, hpc)
        assert dev.download_minimizers().tobytes() == np.concatenate([z["mini"] for z in zs]).tobytes(), (w, k, hpc)


# ---- (b) fuzz against the CPU model

def fuzz_read(rnd, n):
    long_runs, s = rnd.random() < .2, []
    while len(s) < n:
        r = rnd.random()
        if r < 0.02:
            s += "N" * rnd.randrange(1, 4)
        elif r < 0.07:
            s += rnd.choice("ACGT") * rnd.randrange(2, 400 if long_runs else 9)
        elif r < 0.12:
            s += [rnd.choice("ACGT") for _ in range(rnd.randrange(1, 7))] * rnd.randrange(2, 30)
        elif r < 0.14:
            s += rnd.choice("acgtuURYn*\x00\x01\x02\x03")
        else:
            s += [rnd.choice("ACGT") for _ in range(rnd.randrange(1, 200))]
    return "".join(s[:n]).encode("latin1")


@pytest.mark.parametrize("w,k,hpc,n_reads,max_exp", [(10, 15, 0, 1500, 5.0), (5, 19, 1, 700, 5.0), (19, 19, 0, 300, 4.5), (11, 21, 0, 300, 4.0),
                                                      (7, 14, 0, 300, 4.5), (4, 6, 1, 200, 4.0), (3, 2, 0, 100, 3.5), (50, 28, 1, 100, 4.5),
                                                      (255, 16, 0, 60, 4.0), (255, 1, 1, 40, 3.5), (1, 1, 0, 40, 3.5), (1, 28, 0, 40, 3.5)])
def test_fuzz_against_cpu_model(dev, w, k, hpc, n_reads, max_exp):
    rnd = random.Random(w * 1000 + k * 10 + hpc)
    seqs = [fuzz_read(rnd, int(10 ** rnd.uniform(0, max_exp))) for _ in range(n_reads)]
    seqs[n_reads // 2] = b""                                              # an empty sequence in the middle and at the end
    seqs.append(b"")
    seq, seq_off = batch(seqs)
    off = dev.sketch(w, k, hpc, seq, seq_off)
    mini = dev.download_minimizers()
    want_off, want = sm.sketch_batch(seq, seq_off, w, k, hpc)
    assert np.array_equal(off, want_off)
    assert mini.tobytes() == want.tobytes()


def test_multi_segment_reads_against_cpu_model(dev):
    rnd = random.Random(77)
    segs = [rnd.choice([1, 1, 2, 2, 3]) for _ in range(200)]
    seqs = [fuzz_read(rnd, int(10 ** rnd.uniform(0.5, 3.5))) for _ in range(sum(segs))]
    seq, seq_off = batch(seqs)
    off = dev.sketch(11, 21, 0, seq, seq_off, n_segs=segs)
    want_off, want = sm.sketch_batch(seq, seq_off, 11, 21, 0, n_segs_per_read=segs)
    assert np.array_equal(off, want_off) and dev.download_minimizers().tobytes() == want.tobytes()


def test_bad_arguments_are_refused(dev):
    seq, seq_off = batch([b"ACGT" * 20])
    for w, k in ((0, 15), (256, 15), (10, 0), (10, 29)):
        with pytest.raises(chaindp.ChainDPError):
            dev.sketch(w, k, 0, seq, seq_off)
    with pytest.raises(chaindp.ChainDPError):
        dev.sketch(10, 15, 0, seq, np.array([0, 50, 40], np.int64))
    with pytest.raises(chaindp.ChainDPError):
        dev.sketch(10, 15, 0, seq, seq_off, n_segs=[2])


# ---- (c) bases in, hits out

def _case(name):
    g = np.load(os.path.join(SEEDS, name + ".npz"), allow_pickle=False)
    if name.startswith("syn_repeats"):
        z = np.load(os.path.join(HERE, "golden", "sketch", name + ".npz"))
        n = len(g["qlen"])
        first = len(z["seq_off"]) - 1 - n                                  # the reads are the fixture's last sequences (after the genome)
        seqs = [z["seq"][z["seq_off"][q]:z["seq_off"][q + 1]].tobytes() for q in range(first, first + n)]
        w, k, hpc = int(z["w"]), int(z["k"]), int(z["is_hpc"])
        preset = {"syn_repeats_avaont": "ava-ont", "syn_repeats_avapb": "ava-pb", "syn_repeats_mapont": "map-ont"}[name]
    else:
        seqs, (w, k, hpc), preset = read_fasta(os.path.join(FA, "MT-orang.fa")), (10, 15, 0), "map-ont"
    assert [len(s) for s in seqs] == list(g["qlen"])
    return g, seqs, w, k, hpc, preset


@pytest.mark.parametrize("name", ["syn_repeats_mapont", "syn_repeats_avaont", "syn_repeats_avapb", "mt_orang_vs_human_mapont"])
def test_map_seqs_equals_map_reads_on_the_reference_minimizers(dev, name):
    g, seqs, w, k, hpc, preset = _case(name)
    pv = [int(x) for x in g["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    R = len(g["qlen"])
    hash_ = (np.arange(R, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    ref_len = np.full(1 << 16, 1 << 20, np.int32)
    opt = P.post_preset(preset)
    ix = dev.load_index([g["img_B"], g["img_H"], g["img_V"], g["img_P"]])
    want = dev.map_reads(ix, int(g["flag"]), int(g["mid_occ"]), par, pv[7], opt, g["mini_off"], g["mini"], g["bid"], g["qlen"], hash_, ref_len)
    seq, seq_off = batch(seqs)
    got = dev.map_seqs(ix, w, k, hpc, int(g["flag"]), int(g["mid_occ"]), par, pv[7], opt, seq, seq_off, g["bid"], hash_, ref_len)
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    assert np.array_equal(got[2], want[2]) and got[3] == want[3]
    assert len(got[1]) > 0
    # the separate calls: the sketch's minimizers are the fixture's, and they feed the seed collection from where they are
    off = dev.sketch(w, k, hpc, seq, seq_off)
    assert np.array_equal(off, g["mini_off"]) and dev.download_minimizers().tobytes() == np.ascontiguousarray(g["mini"]).tobytes()
    a_off, a, rep, mpo, mp = dev.collect_seeds(ix, int(g["flag"]), int(g["mid_occ"]), None, None, g["bid"], None)
    assert np.array_equal(a_off, g["a_off"]) and a.tobytes() == np.ascontiguousarray(g["anchors"]).tobytes()
    assert np.array_equal(rep, g["rep_len"]) and np.array_equal(mpo, g["mp_off"]) and np.array_equal(mp, g["mini_pos"])
    again = dev.map_reads(ix, int(g["flag"]), int(g["mid_occ"]), par, pv[7], opt, None, None, g["bid"], None, hash_, ref_len)
    assert np.array_equal(again[0], want[0]) and again[1].tobytes() == want[1].tobytes()


def test_resident_minimizers_need_a_sketch_of_the_same_reads(dev):
    g, seqs, w, k, hpc, _ = _case("syn_repeats_avaont")
    ix = dev.load_index([g["img_B"], g["img_H"], g["img_V"], g["img_P"]])
    seq, seq_off = batch(seqs)
    dev.sketch(w, k, hpc, seq, seq_off)
    with pytest.raises(chaindp.ChainDPError):
        dev.collect_seeds(ix, int(g["flag"]), int(g["mid_occ"]), None, None, g["bid"][:-1], None)          # another read count
    dev.collect_seeds(ix, int(g["flag"]), int(g["mid_occ"]), g["mini_off"], g["mini"], g["bid"], g["qlen"])     # uploads minimizers of its own
    with pytest.raises(chaindp.ChainDPError):
        dev.collect_seeds(ix, int(g["flag"]), int(g["mid_occ"]), None, None, g["bid"], None)               # ... which replaced the sketch's
    with pytest.raises(chaindp.ChainDPError):
        dev.download_minimizers()


# ---- (d) capacity

def test_capacity_refusal_leaves_the_context_usable(monkeypatch):
    """The refusals that can be provoked without harm: more bases than one call takes (through the CHAINDP_SKETCH_MAX_BASES test
    switch) and more reads than the context was created for.  The third one, the device having no room for the buffers (the
    all-or-nothing release in sketch_reserve / seed_reserve after a failed hipMalloc), is NOT exercised: that would mean exhausting
    the HBM of a machine other people's work runs on."""
    z = np.load(os.path.join(HERE, "golden", "sketch", "traps_mapont.npz"))
    monkeypatch.setenv("CHAINDP_SKETCH_MAX_BASES", "5000")                  # read once, when the context is created
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=64) as d:
        n = 40
        seq, seq_off = z["seq"][:z["seq_off"][n]], z["seq_off"][:n + 1]
        assert len(seq) > 5000
        with pytest.raises(chaindp.ChainDPError, match="bases"):
            d.sketch(10, 15, 0, seq, seq_off)
        with pytest.raises(chaindp.ChainDPError, match="read capacity"):
            d.sketch(10, 15, 0, z["seq"][:z["seq_off"][70]][:4000], np.minimum(z["seq_off"][:71], 4000))   # 70 reads in a context made for 64
        m = 10
        assert z["seq_off"][m] <= 5000
        off = d.sketch(10, 15, 0, z["seq"][:z["seq_off"][m]], z["seq_off"][:m + 1])
        assert np.array_equal(off, z["mini_off"][:m + 1])
        assert d.download_minimizers().tobytes() == np.ascontiguousarray(z["mini"][:z["mini_off"][m]]).tobytes()


# ---- (e) a sketch starts a new batch

def test_sketch_drops_the_resident_batch_instead_of_corrupting_it(dev):
    from minimap2_chaindp_amd import anchorgen
    par = P.preset("ava-ont")
    off, a = anchorgen.generate("ava-ont", n_reads=32, seed=5)
    f, p, v = dev.chain_batch(par, off, a)
    dev.upload(off, a)
    dev.run_full(par)
    z = np.load(os.path.join(HERE, "golden", "sketch", "mt_human_avaont.npz"))
    dev.sketch(5, 15, 0, z["seq"], z["seq_off"])
    with pytest.raises(chaindp.ChainDPError):                               # refused, not answered with something else
        dev.download()
    with pytest.raises(chaindp.ChainDPError):
        dev.backtrack(par, 3)
    assert dev.download_minimizers().tobytes() == np.ascontiguousarray(z["mini"]).tobytes()
    f2, p2, v2 = dev.chain_batch(par, off, a)                               # and the context goes on working
    assert np.array_equal(f, f2) and np.array_equal(p, p2) and np.array_equal(v, v2)
