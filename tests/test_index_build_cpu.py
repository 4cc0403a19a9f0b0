"""CPU tier: tests/index_build_model.py (the checker of the device's index build) against the images the unmodified reference built:
the fixtures of tests/golden/index and the seed fixtures whose targets lie in tests/golden/fa, in canonical form.  Nothing of the
product runs here."""
import numpy as np
import pytest

import index_build_model as ibm
import index_fixtures as fx
import oracle_lib as ol

BLOBS = "BHVP"


@pytest.mark.parametrize("name", fx.CASES)
def test_model_image_equals_the_reference(name):
    c = fx.case(name)
    blobs, route = fx.model(name)
    for n, ours, ref in zip(BLOBS, blobs, c["img"]):
        assert ours.shape == ref.shape and np.array_equal(ours, ref), (name, n)
    assert route["distinct"] == int(ibm.occupied(c["img"]).sum())


@pytest.mark.parametrize("name", fx.CASES)
def test_canonical_form_touches_only_empty_slots(name):
    c = fx.case(name)
    occ = ibm.occupied(c["raw"])
    for k in (0, 3):
        assert np.array_equal(c["raw"][k], c["img"][k]), BLOBS[k]
    raw_h, can_h = np.asarray(c["raw"][1]).reshape(-1, 64), c["img"][1].reshape(-1, 64)
    assert np.array_equal(raw_h[:, :4], can_h[:, :4]) and np.array_equal(raw_h[:, 52:], can_h[:, 52:])
    assert not can_h[:, 52:].any()
    assert np.array_equal(raw_h[:, 4:52].reshape(-1, 6)[occ], can_h[:, 4:52].reshape(-1, 6)[occ])
    assert np.array_equal(np.asarray(c["raw"][2]).view(np.uint64)[occ], c["img"][2].view(np.uint64)[occ])
    assert not c["img"][2].view(np.uint64)[~occ].any()


@pytest.mark.parametrize("name", [n for n in fx.CASES if fx.case(n)["mid_occ"] is not None])
def test_model_mid_occ_equals_the_reference(name):
    c = fx.case(name)
    got = ibm.cal_max_occ(fx.model(name)[0], fx.MID_OCC_FRAC)
    assert max(got, c["min_mid_occ"]) == c["mid_occ"]
    assert ibm.cal_max_occ(c["raw"], fx.MID_OCC_FRAC) == got
    assert ibm.cal_max_occ(c["raw"], 0.0) == 0x7FFFFFFF


def test_fixtures_hold_what_they_are_for():
    r = fx.model("dense_mapont")[1]
    assert r["expanded"] >= 500 and (fx.case("dense_mapont")["rank"] != np.arange(24)).any()
    assert len(np.unique(fx.case("dense_mapont")["img"][3].view(np.uint64) >> np.uint64(43))) > 1
    c = fx.case("dense_avapb")
    mini = ibm.minimizers(c["seqs"], c["w"], c["k"], c["is_hpc"])
    o = np.argsort(mini[:, 0] >> np.uint64(8), kind="stable")
    m, span = (mini[:, 0] >> np.uint64(8))[o], (mini[:, 0] & np.uint64(255))[o]
    assert ((m[1:] == m[:-1]) & (span[1:] != span[:-1])).any()
    img = fx.case("heavy_buckets")["img"]
    occ = ibm.occupied(img)
    keys = {int(occ[h0:h0 + N].sum()) for _, N, h0, _ in ibm._tables(img)}
    assert {12, 13, 25, 26, 49, 50} <= keys


@pytest.mark.parametrize("name", list(fx.SEED_CASES))
def test_model_image_gives_the_recorded_anchors(name):
    g = fx.case(name)["seeds"]
    with ol.SeedIndex(fx.model(name)[0]) as ix:
        for r in range(len(g["bid"])):
            mini = g["mini"][g["mini_off"][r]:g["mini_off"][r + 1]]
            a, rep_len, mini_pos = ix.collect_seeds(int(g["flag"]), int(g["mid_occ"]), g["bid"][r], g["qlen"][r], mini)
            assert np.array_equal(a, g["anchors"][g["a_off"][r]:g["a_off"][r + 1]]), (name, r)
            assert rep_len == int(g["rep_len"][r])
            assert np.array_equal(mini_pos, g["mini_pos"][g["mp_off"][r]:g["mp_off"][r + 1]])
