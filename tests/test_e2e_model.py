"""CPU tier of the end-to-end tests: pins the checker of tests/test_gpu_e2e.py and shows that its inputs exercise what they are meant
to.  (a) the index-image builder (tests/index_image.py) against all eight seed fixtures: opened by the seed oracle, its image gives
the anchors, rep_len and mini_pos the reference recorded for its own image; (b) the composed model (tests/e2e_model.py), from the
bases alone, against the reference's final hits in tests/golden/post; (c) what every seeded batch of the GPU tier contains, counted
from the model's intermediates and asserted, so that a change to the generator cannot silently empty a case."""
import os

import numpy as np
import pytest

import e2e_model as em
import index_image
import oracle_lib as ol
from minimap2_chaindp_amd import params as P
from test_gpu_post import post_opt, same_records

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def read_fasta(name):
    seqs = []
    for ln in open(os.path.join(GOLDEN, "fa", name)):
        if ln.startswith(">"):
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return ["".join(s).encode() for s in seqs]


def sketch_seqs(name, lo, hi=None):
    z = np.load(os.path.join(GOLDEN, "sketch", name + ".npz"))
    off = z["seq_off"]
    return [z["seq"][off[q]:off[q + 1]].tobytes() for q in range(lo, len(off) - 1 if hi is None else hi)]


# fixture -> (targets, reads, w, k, hpc): the sequences the reference was run on when the seed / regs / post fixtures were made
CASES = {
    "inv_mapont": (lambda: read_fasta("t-inv.fa"), lambda: read_fasta("q-inv.fa"), 10, 15, 0),
    "inv_sr": (lambda: read_fasta("t-inv.fa"), lambda: read_fasta("q-inv.fa"), 11, 21, 0),
    "mt_human_self_avaont": (lambda: read_fasta("MT-human.fa"), lambda: read_fasta("MT-human.fa"), 5, 15, 0),
    "mt_human_vs_orang_avaont": (lambda: read_fasta("MT-orang.fa"), lambda: read_fasta("MT-human.fa"), 5, 15, 0),
    "mt_orang_vs_human_mapont": (lambda: read_fasta("MT-human.fa"), lambda: read_fasta("MT-orang.fa"), 10, 15, 0),
    "syn_repeats_mapont": (lambda: sketch_seqs("syn_repeats_mapont", 0, 1), lambda: sketch_seqs("syn_repeats_mapont", 1), 10, 15, 0),
    "syn_repeats_avaont": (lambda: sketch_seqs("syn_repeats_avaont", 0), lambda: sketch_seqs("syn_repeats_avaont", 0), 5, 15, 0),
    "syn_repeats_avapb": (lambda: sketch_seqs("syn_repeats_avapb", 0), lambda: sketch_seqs("syn_repeats_avapb", 0), 5, 19, 1),
}


def image_of(name):
    targets, _, w, k, hpc = CASES[name]
    return index_image.build_image(index_image.index_entries(targets(), w, k, hpc))


# ---- (a) the builder

@pytest.mark.parametrize("name", sorted(CASES))
def test_built_image_gives_the_reference_images_seeds(name):
    g = np.load(os.path.join(GOLDEN, "seeds", name + ".npz"), allow_pickle=False)
    img = image_of(name)
    assert [len(b) % 8 for b in img] == [0, 0, 0, 0] and len(img[0]) == len(g["img_B"]) and len(img[3]) == len(g["img_P"])
    with ol.SeedIndex(img) as ix:
        for r in range(len(g["qlen"])):
            a, rep, mp = ix.collect_seeds(int(g["flag"]), int(g["mid_occ"]), int(g["bid"][r]), int(g["qlen"][r]), g["mini"][g["mini_off"][r]:g["mini_off"][r + 1]])
            assert np.array_equal(a, g["anchors"][g["a_off"][r]:g["a_off"][r + 1]]), (r, "anchors, order of equal x included")
            assert rep == g["rep_len"][r] and np.array_equal(mp, g["mini_pos"][g["mp_off"][r]:g["mp_off"][r + 1]]), r


def test_builder_asserts_the_formats_limits():
    with pytest.raises(AssertionError, match="2\\^21"):
        index_image.index_entries([b"A" * (1 << 21)], 10, 15, 0)
    with pytest.raises(AssertionError):
        index_image.index_entries([b"ACGT"], 10, 15, 0, rank=[1 << 21])
    assert [len(b) for b in index_image.build_image({})] == [16 << 14, 0, 0, 0]


# ---- (b) the composed model, from the bases

@pytest.mark.parametrize("name", ["syn_repeats_mapont", "syn_repeats_avaont", "syn_repeats_avapb", "mt_orang_vs_human_mapont", "mt_human_vs_orang_avaont",
                                  "inv_mapont"])
def test_model_from_bases_gives_the_references_final_hits(name):
    g = np.load(os.path.join(GOLDEN, "seeds", name + ".npz"), allow_pickle=False)
    z = np.load(os.path.join(GOLDEN, "post", name + ".npz"), allow_pickle=False)
    _, reads, w, k, hpc = CASES[name]
    reads = reads()
    assert [len(s) for s in reads] == list(g["qlen"]) == list(z["qlen"])
    pv = [int(x) for x in g["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    sets = [c[:-4] for c in z.files if c.endswith("_opt") and np.array_equal(z[c[:-4] + "_rep_len"], g["rep_len"])]   # rep_len as collected
    assert "mapont" in sets and "avaont" in sets and len(sets) >= 6
    with ol.SeedIndex(image_of(name)) as ix:
        for cname in sets:
            m = em.model_map(ix, w, k, hpc, int(g["flag"]), int(g["mid_occ"]), par, pv[7], post_opt(z, cname), reads, g["bid"], z["hash"], z["ref_len"])
            assert np.array_equal(m.mini_off, g["mini_off"]) and m.mini.tobytes() == np.ascontiguousarray(g["mini"]).tobytes()
            assert np.array_equal(m.a_off, g["a_off"]) and np.array_equal(m.anchors, g["anchors"]) and np.array_equal(m.mini_pos, g["mini_pos"])
            assert np.array_equal(m.chains_off, z["chains_off"]) and m.regs_in.tobytes() == z["regs_in"].tobytes()
            assert np.array_equal(m.rep_len, g["rep_len"]) and m.n_anchors == len(g["anchors"])
            assert np.array_equal(m.regs_off, z[cname + "_regs_off"]), cname
            same_records(m.regs, z[cname + "_regs"].copy().view(ol.REG_DTYPE).reshape(-1), (name, cname))


# ---- (c) what the GPU tier's batches contain

def _counts(name):
    sc, m = em.named(name)
    c = em.coverage(m, sc.par)
    print(f"\n{name}: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    return sc, c


@pytest.mark.parametrize("name", ["map-ont", "map-pb", "ava-ont", "ava-pb", "family"])
def test_scenario_contains_what_it_is_meant_to(name):
    sc, c = _counts(name)
    assert c["reads"] >= (300 if name == "family" else 2000)
    kinds = set(sc.kinds)
    assert kinds >= {n for n, _ in em.KINDS}, "every kind of read"
    assert min(len(s) for s in sc.reads) == 0 and max(len(s) for s in sc.reads) >= 29000 and any(0 < len(s) < sc.k for s in sc.reads)
    assert any(len(s) > 0 and set(s) == {ord("N")} for s in sc.reads) and any(any(ch in s for ch in b"acgt") for s in sc.reads)
    for what in ("no_minimizers", "no_anchors", "no_chains", "multi_hit", "mapq0", "reverse", "x_ties"):
        assert c[what] > 0, (name, what, c)
    assert c["max_unit"] > 64 and c["max_anchors"] > 4096, c
    if sc.mode.startswith("map"):
        # (the ava presets carry MM_F_ALL_CHAINS and MM_F_NO_LJOIN: no mm_set_parent, mm_select_sub or mm_join_long there, every hit
        # keeps mapq 0; what is left of the post steps on those batches is mm_est_err and mm_set_mapq's zero)
        for what in ("secondary", "dropped", "joined", "mapq60"):
            assert c[what] > 0, (name, what, c)
    if name != "family":                                                     # (its max_occ lets every minimizer through)
        assert c["rep_len"] > 0, c
    else:
        assert c["max_chains"] > 256, c                                      # beyond k_post_read's LDS path
        assert "family" in kinds
    if sc.hpc:
        assert c["mixed_q_span"] > 0, c


def test_scenarios_are_seeded():
    a, b = em.scenario("map-ont", 60, seed=5), em.scenario("map-ont", 60, seed=5)
    assert a.reads == b.reads and a.targets == b.targets and np.array_equal(a.hash_, b.hash_) and np.array_equal(a.bid, b.bid)
    assert em.scenario("map-ont", 60, seed=6).reads != a.reads
    ava = em.scenario("ava-pb", 60, seed=5)
    g = np.load(os.path.join(GOLDEN, "seeds", "syn_repeats_avapb.npz"), allow_pickle=False)
    assert ava.targets is ava.reads and ava.flag == int(g["flag"]) and np.array_equal(ava.bid[:12], g["bid"])
    assert (ava.w, ava.k, ava.hpc) == (5, 19, 1) and list(ava.ref_len) == [len(s) for s in ava.reads]
