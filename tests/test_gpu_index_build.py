"""GPU tier: chaindp_index_build (target bases in, the index image resident) against the images the unmodified reference built, in
canonical form (tests/index_fixtures.py): (a) the downloaded blobs byte for byte and the route's expansions against the model's;
(b) mm_idx_cal_max_occ on built and on loaded indexes; (c) forced sketch sub-batches; (d) the built index is interchangeable with a
loaded one for chaindp_collect_seeds and chaindp_map_seqs; (e) chaindp_sketch is what it was; (f) the refusals."""
import os

import numpy as np
import pytest

import index_build_model as ibm
import index_fixtures as fx
from minimap2_chaindp_amd import chaindp
from minimap2_chaindp_amd import params as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BLOBS = "BHVP"


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 22, max_reads=1 << 13) as d:
        yield d


def build(dev, c, **kw):
    return dev.build_index(c["w"], c["k"], c["is_hpc"], c["seq"], c["seq_off"], rank=c["rank"], **kw)


def same_blobs(got, want, what):
    for n, g, w in zip(BLOBS, got, want):
        assert g.shape == w.shape, (what, n, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert not len(bad), (what, n, f"{len(bad)} bytes differ, first at {int(bad[0])}")


# ---- (a), (b)

@pytest.mark.parametrize("name", fx.CASES)
def test_built_image_is_the_reference_image(dev, name):
    c = fx.case(name)
    ix = build(dev, c)
    same_blobs(dev.index_blobs(ix), c["img"], name)
    route, want = dev.index_route(ix), fx.model(name)[1]
    print(f"\n[index route] {name}: {route}")
    assert route["sub_batches"] == 1
    for key in ("minimizers", "distinct", "buckets", "expanded", "max_keys", "passes_run", "passes_skipped"):
        assert route[key] == want[key], (key, route, want)
    # mm_idx_cal_max_occ: the built index, the reference's own image loaded (its empty slots hold heap garbage), the model
    loaded = dev.load_index(c["raw"])
    for f in (fx.MID_OCC_FRAC, 0.01, 0.5, 1.0):
        want_occ = ibm.cal_max_occ(c["img"], f)
        assert dev.index_max_occ(ix, f) == want_occ and dev.index_max_occ(loaded, f) == want_occ, f
    assert dev.index_max_occ(ix, 0.0) == 0x7FFFFFFF and dev.index_max_occ(loaded, -1.0) == 0x7FFFFFFF
    if c["mid_occ"] is not None:
        assert max(dev.index_max_occ(ix, fx.MID_OCC_FRAC), c["min_mid_occ"]) == c["mid_occ"]
    same_blobs(dev.index_blobs(loaded), [np.asarray(x) for x in c["raw"]], name + " (loaded: what was uploaded)")


# ---- (c)

def test_forced_sub_batches_give_the_same_image(dev):
    c = fx.case("dense_mapont")
    dev.set_index_chunk_bases(int(c["seq_off"][-1]) // 5)
    try:
        ix = build(dev, c)
    finally:
        dev.set_index_chunk_bases(0)
    assert dev.index_route(ix)["sub_batches"] > 1
    same_blobs(dev.index_blobs(ix), c["img"], "dense_mapont in sub-batches")
    dev.set_index_chunk_bases(1)                                         # one sequence per sub-batch
    try:
        ix = build(dev, c)
    finally:
        dev.set_index_chunk_bases(0)
    assert dev.index_route(ix)["sub_batches"] == len(c["seqs"])
    same_blobs(dev.index_blobs(ix), c["img"], "dense_mapont, a sequence per sub-batch")


def test_other_bucket_bits_and_the_empty_input(dev):
    c = fx.case("inv_mapont")
    mini = ibm.minimizers(c["seqs"], c["w"], c["k"], c["is_hpc"])
    for b in (1, 6, 17):
        ix = build(dev, c, b=b)
        same_blobs(dev.index_blobs(ix), ibm.build(mini, c["rank"], b)[0], f"b = {b}")
    for seq, seq_off in ((b"", [0]), (b"", [0, 0, 0]), (b"ACGTN" * 2, [0, 4, 10])):      # nothing, empty sequences, no k-mer
        ix = dev.build_index(10, 15, 0, seq, seq_off, b=6)
        blobs = dev.index_blobs(ix)
        assert [len(x) for x in blobs] == [16 << 6, 0, 0, 0] and not blobs[0].any()
        assert dev.index_route(ix)["minimizers"] == 0
        with pytest.raises(chaindp.ChainDPError):
            dev.index_max_occ(ix, 0.5)


# ---- (d)

@pytest.mark.parametrize("name", list(fx.SEED_CASES))
def test_collect_seeds_over_the_built_index(dev, name):
    c = fx.case(name)
    g = c["seeds"]
    built, loaded = build(dev, c), dev.load_index(c["raw"])
    res = [dev.collect_seeds(ix, int(g["flag"]), int(g["mid_occ"]), g["mini_off"], g["mini"], g["bid"], g["qlen"]) for ix in (built, loaded)]
    for x, y in zip(*res):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert np.array_equal(res[0][0], g["a_off"]) and res[0][1].tobytes() == np.ascontiguousarray(g["anchors"]).tobytes()


def test_map_seqs_of_the_synthetic_reads_against_their_own_built_index(dev):
    g = np.load(os.path.join(HERE, "golden", "seeds", "syn_repeats_avaont.npz"), allow_pickle=False)
    z = np.load(os.path.join(HERE, "golden", "sketch", "syn_repeats_avaont.npz"))
    n = len(g["qlen"])
    first = len(z["seq_off"]) - 1 - n                                     # the reads are the sketch fixture's last sequences
    seqs = [z["seq"][z["seq_off"][q]:z["seq_off"][q + 1]].tobytes() for q in range(first, first + n)]
    assert n == 12 and [len(s) for s in seqs] == list(g["qlen"])
    w, k, hpc = int(z["w"]), int(z["k"]), int(z["is_hpc"])
    seq, seq_off = np.frombuffer(b"".join(seqs), np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    raw = [g["img_B"], g["img_H"], g["img_V"], g["img_P"]]
    built = dev.build_index(w, k, hpc, seq, seq_off)                       # the reads are named r00 .. r11: rank = number
    same_blobs(dev.index_blobs(built), ibm.canonical(raw), "syn_repeats_avaont")
    mid_occ = dev.index_max_occ(built, fx.MID_OCC_FRAC)
    assert mid_occ == int(g["mid_occ"])
    pv = [int(x) for x in g["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    hash_ = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    ref_len, opt = np.array([len(s) for s in seqs], np.int32), P.post_preset("ava-ont")
    res = [dev.map_seqs(ix, w, k, hpc, int(g["flag"]), mid_occ, par, pv[7], opt, seq, seq_off, g["bid"], hash_, ref_len)
           for ix in (built, dev.load_index(raw))]
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1].tobytes() == res[1][1].tobytes()
    assert np.array_equal(res[0][2], res[1][2]) and res[0][3] == res[1][3] and len(res[0][1]) > 0


# ---- (e)

def test_sketch_after_a_build_is_what_it_was(dev):
    build(dev, fx.case("dense_avapb"))
    with pytest.raises(chaindp.ChainDPError):                              # the build leaves no minimizers for the mapping calls
        dev.download_minimizers()
    for name in ("traps_avapb", "mt_human_mapont", "syn_repeats_avaont"):
        z = np.load(os.path.join(HERE, "golden", "sketch", name + ".npz"))
        off = dev.sketch(int(z["w"]), int(z["k"]), int(z["is_hpc"]), z["seq"], z["seq_off"])
        assert np.array_equal(off, z["mini_off"]) and dev.download_minimizers().tobytes() == np.ascontiguousarray(z["mini"]).tobytes(), name


# ---- (f)

def test_refusals_leave_the_context_usable(dev):
    c = fx.case("inv_mapont")
    lib, ctx = chaindp.lib(), dev._ctx
    arg = {"code": -1}

    def refused(**kw):
        a = dict(w=c["w"], k=c["k"], is_hpc=0, seq=c["seq"], seq_off=c["seq_off"], rank=c["rank"], b=14)
        a.update(kw)
        with pytest.raises(chaindp.ChainDPError, match=r"chaindp error -1: \S"):
            dev.build_index(a["w"], a["k"], a["is_hpc"], a["seq"], a["seq_off"], rank=a["rank"], b=a["b"])
        assert lib.chaindp_index_build_status(ctx) == arg["code"]
        same_blobs(dev.index_blobs(build(dev, c)), c["img"], f"after the refusal of {kw.keys()}")      # the next call works

    for b in (0, 25, -3):
        refused(b=b)
    for w, k in ((0, 15), (256, 15), (10, 0), (10, 29)):
        refused(w=w, k=k)
    n = len(c["seq_off"]) - 1
    refused(rank=np.full(n, 1 << 21, np.uint32))
    long_ = np.random.RandomState(1).randint(0, 4, 1 << 21).astype(np.uint8)   # 2^21 bases (the bytes 0..3): one more than a position holds
    refused(seq=long_, seq_off=np.array([0, 1 << 21], np.int64), rank=None)
    many = (1 << 21) + 1
    refused(seq=np.zeros(0, np.uint8), seq_off=np.zeros(many + 1, np.int64), rank=None)
    ok = dev.build_index(10, 15, 0, long_[:(1 << 21) - 1], np.array([0, (1 << 21) - 1], np.int64))          # the longest sequence there is
    assert dev.index_route(ok)["minimizers"] > 0
