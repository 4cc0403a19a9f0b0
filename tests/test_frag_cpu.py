"""CPU tier: the restatement of the reference's post steps for reads of several segments (tests/frag_oracle.py) against what the unmodified
reference produced (tests/golden/frag, written by tests/golden/make_frag_golden.py), the traps those fixtures must hold, and the
composed CPU model of tests/frag_model.py on a small seeded paired batch."""
import glob
import os

import numpy as np
import pytest

import frag_model as fm
import frag_oracle as fo
import oracle_lib as ol
import post_oracle as po
from minimap2_chaindp_amd import params as P

HERE = os.path.dirname(os.path.abspath(__file__))
FRAG = sorted(glob.glob(os.path.join(HERE, "golden", "frag", "*.npz")))
POST_MAX = max(os.path.getsize(p) for p in glob.glob(os.path.join(HERE, "golden", "post", "*.npz")))
OPT_KEYS = [k for k, _ in P.PostOpt._fields_]


def _opt(z, cname):
    return {k: (float(np.float32(v)) if k in ("mask_level", "pri_ratio") else int(v)) for k, v in zip(OPT_KEYS, z[cname + "_opt"])}


def _reads(z):
    regs = z["regs_in"].copy().view(ol.REG_DTYPE).reshape(-1)
    first = np.concatenate([[0], np.cumsum(z["n_segs"])])
    for r in range(len(z["qlen"])):
        yield (r, regs[z["chains_off"][r]:z["chains_off"][r + 1]], z["b"][z["b_off"][r]:z["b_off"][r + 1]], z["seg_len"][first[r]:first[r + 1]],
               z["mini_pos"][z["mini_pos_off"][r]:z["mini_pos_off"][r + 1]], first[r])


def test_fixtures_are_there_and_small():
    assert len(FRAG) >= 4
    for p in FRAG:
        assert os.path.getsize(p) <= POST_MAX, p


@pytest.mark.parametrize("path", FRAG, ids=[os.path.basename(p)[:-4] for p in FRAG])
def test_restatement_equals_every_fixture_bit_for_bit(path):
    z = np.load(path, allow_pickle=False)
    max_gap_ref = int(z["params"][0])
    for cname in sorted(k[:-4] for k in z.files if k.endswith("_opt")):
        od = _opt(z, cname)
        soff, exp = z[cname + "_seg_regs_off"], z[cname + "_regs"].copy().view(ol.REG_DTYPE).reshape(-1)
        for r, regs, b, qlens, mp, q0 in _reads(z):
            segs = fo.frag_read(od, max_gap_ref, int(z["hash"][r]), qlens, int(z[cname + "_rep_len"][r]), z["ref_len"], regs, b, mp)
            assert len(segs) == len(qlens)
            for s, (got, sa) in enumerate(segs):
                q = q0 + s
                assert got.tobytes() == exp[soff[q]:soff[q + 1]].tobytes(), (cname, r, s)
                if len(qlens) > 1:
                    assert (got["div"].view(np.uint32) == np.float32(-1.0).view(np.uint32)).all()
                if cname + "_seg_a" in z.files:
                    ao = z[cname + "_seg_a_off"]
                    assert sa.tobytes() == z[cname + "_seg_a"][ao[q]:ao[q + 1]].tobytes(), (cname, r, s)


def test_every_recorded_trap_is_set():
    seen = {}
    for p in FRAG:
        z = np.load(p, allow_pickle=False)
        for k, v in zip(z["trap_names"], z["trap_seen"]):
            seen[str(k)] = seen.get(str(k), False) or bool(v)
    want = [b + "_" + o for b in fo.BRANCHES for o in ("no", "yes")] + [
        "best_n_cut", "sync_after_drop", "slot_overwritten", "squeezed_zero", "empty_segment", "reverse_hit", "three_segments", "above_lds_cap",
        "seg_gen_regs_over_64_or_equal_keys", "one_segment_read", "pri1_float_matters", "chi_both_matters"]
    assert sorted(seen) == sorted(want)
    assert all(seen.values()), [k for k, v in seen.items() if not v]


def test_one_segment_path_equals_post_read():
    z = np.load(os.path.join(HERE, "golden", "frag", "syn_frag.npz"), allow_pickle=False)
    n = 0
    for cname in ("sr", "nonsr", "cigar"):
        od = _opt(z, cname)
        for r, regs, b, qlens, mp, _ in _reads(z):
            if len(qlens) != 1:
                continue
            got, ga = fo.frag_read(od, int(z["params"][0]), int(z["hash"][r]), qlens, int(z[cname + "_rep_len"][r]), z["ref_len"], regs, b, mp)[0]
            exp, ea = po.post_read(od, int(qlens[0]), int(z[cname + "_rep_len"][r]), z["ref_len"], regs, b, mp)
            assert got.tobytes() == exp.tobytes() and ga.tobytes() == ea.tobytes()
            n += 1
    assert n > 0


def test_the_variants_differ_where_the_reference_made_a_choice():
    """the float product of pe.c:20 and `is_chi_both ||` of pe.c:25, on the fragments built for them"""
    for frag, variant in ((fm.pri1_frag(), "pri1_double"), (fm.chi_both_frag(), "no_chi_both")):
        sh = fm._pack([frag])
        par = P.preset("sr")
        f, p, v, _ = ol.oracle_fpv(par, sh["anchors"])
        u, b = ol.oracle_bottom(2, par.min_sc, ol.oracle_compact(par, sh["anchors"], f.copy(), p.copy(), v.copy()))
        regs = ol.oracle_gen_regs(1, int(sh["qlen"][0]), u, b.reshape(-1, 2))
        od = po.opt_dict(P.post_preset("sr"))
        args = (od, par.max_dist_x, 1, sh["seg_len"], 0, np.full(8, 1 << 20, np.int32), regs, b.reshape(-1, 2), sh["mini_pos"])
        a, c = fo.frag_read(*args), fo.frag_read(*args, variant=variant)
        assert any(x[0].tobytes() != y[0].tobytes() for x, y in zip(a, c)), variant


def test_sr_post_preset():
    o = P.post_preset("sr")
    assert (o.flag, o.best_n, o.min_cnt, o.min_chain_score, o.match_sc, o.sub_diff, o.min_diff, o.is_sr) == (P.MM_F_SR, 20, 2, 25, 2, 12, 42, 1)
    assert o.pri_ratio == 0.5
    assert set(P.POST_PRESETS) == {"map-ont", "map-pb", "ava-ont", "ava-pb", "sr"}
    assert P.POST_PRESETS["map-ont"] == dict(min_diff=30) and P.POST_PRESETS["map-pb"] == dict(min_diff=38)   # existing entries unchanged


def test_composed_model_on_a_small_paired_batch_is_deterministic():
    sc = fm.scenario(n_frags=120, seed=5)
    img = sc.image()
    m1, m2 = fm.model_of(sc, img, pe_ori=1), fm.model_of(fm.scenario(n_frags=120, seed=5), img, pe_ori=1)
    assert m1.regs.tobytes() == m2.regs.tobytes() and np.array_equal(m1.seg_regs_off, m2.seg_regs_off)
    assert len(m1.seg_regs_off) == int(m1.n_segs.sum()) + 1
    cov = fm.coverage(m1)
    assert cov["both_segments"] > 0 and cov["one_segment"] > 0 and cov["reverse"] > 0 and cov["final_hits"] > 0, cov
    split = np.repeat(np.repeat(m1.n_segs > 1, m1.n_segs), np.diff(m1.seg_regs_off))
    assert (m1.regs["div"][split] == np.float32(-1.0)).all() and (m1.regs["bits"][split] >> 15 & 1).all()
    # without pe_ori the mates lie on opposite strands and no chain spans both segments; with it the flip changes strand and coordinates
    m0 = fm.model_of(sc, img, pe_ori=-1)
    assert m0.regs.tobytes() != m1.regs.tobytes()
