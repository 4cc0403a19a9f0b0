"""chain_post + mm_est_err + mm_set_mapq (map.c:870-877), CPU tier: the restatement (tests/post_oracle.py) against the reference's
fixtures (tests/golden/post, written by tests/golden/make_post_golden.py) and, where oracle/_ref is built, against the live reference on
freshly seeded shapes; the new ABI symbols; the options mirror; the host half of the logf patch list."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import oracle_lib as ol
import post_oracle as po
import post_shapes
from minimap2_chaindp_amd import chaindp, params as P

HERE = os.path.dirname(os.path.abspath(__file__))
POST = sorted(glob.glob(os.path.join(HERE, "golden", "post", "*.npz")))
OPT_KEYS = [k for k, _ in P.PostOpt._fields_]
NEW_SYMBOLS = ("chaindp_chain_post", "chaindp_map_reads", "chaindp_post_logf_selftest", "chaindp_post_logf_patches")


def configs(z):
    return sorted(k[:-4] for k in z.files if k.endswith("_opt"))


def opt_of(z, cname):
    d = dict(zip(OPT_KEYS, (float(v) for v in z[cname + "_opt"])))
    return {k: (v if k in ("mask_level", "pri_ratio") else int(v)) for k, v in d.items()}


def reads_of(z):
    regs = z["regs_in"].copy().view(ol.REG_DTYPE).reshape(-1)
    for r in range(len(z["qlen"])):
        c0, c1 = z["chains_off"][r], z["chains_off"][r + 1]
        yield (regs[c0:c1], z["b"][z["b_off"][r]:z["b_off"][r + 1]], int(z["qlen"][r]),
               z["mini_pos"][z["mini_pos_off"][r]:z["mini_pos_off"][r + 1]])


def test_post_fixtures_present():
    assert len(POST) >= 9
    assert all(os.path.getsize(p) < (1 << 20) for p in POST)


@pytest.mark.parametrize("path", POST, ids=[os.path.basename(p)[:-4] for p in POST])
def test_restatement_equals_golden(path):
    z = np.load(path, allow_pickle=False)
    for cname in configs(z):
        od = opt_of(z, cname)
        rep = z[cname + "_rep_len"]
        got, ga = [], []
        for r, (regs, b, qlen, mp) in enumerate(reads_of(z)):
            out, a = po.post_read(od, qlen, int(rep[r]), z["ref_len"], regs, b, mp)
            got.append(out); ga.append(a.reshape(-1, 2))
        got = np.concatenate(got)
        want = z[cname + "_regs"].copy().view(ol.REG_DTYPE).reshape(-1)
        assert len(got) == len(want), cname
        assert got.tobytes() == want.tobytes(), cname
        if cname + "_a" in z.files:
            assert np.concatenate(ga).tobytes() == z[cname + "_a"].tobytes(), cname


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (build container only)")
@pytest.mark.parametrize("seed", [101, 202])
def test_restatement_equals_live_reference(seed):
    sh = post_shapes.shapes(seed=seed, n_random=4)
    par = P.preset("map-ont")
    ref_len = np.full(8192, 1 << 28, np.int32)
    grid = [P.post_preset("map-ont"), P.post_preset("map-ont", pri_ratio=0.5, best_n=2), P.post_preset("map-ont", flag=P.MM_F_NO_LJOIN),
            P.post_preset("map-ont", mask_level=0.2, min_join_flank_sc=200)]
    n_reads = 0
    for r in range(len(sh["qlen"])):
        a = np.ascontiguousarray(sh["anchors"][sh["off"][r]:sh["off"][r + 1]])
        _, _, _, seeds = ol.ref_fpv_seeds(par, a)
        u, b = ol.ref_bottom(3, par.min_sc, 1, seeds)
        b = b.reshape(-1, 2)
        regs = ol.ref_gen_regs(r * 7919, int(sh["qlen"][r]), u, b)
        mp = sh["mini_pos"][sh["mini_pos_off"][r]:sh["mini_pos_off"][r + 1]]
        for opt in grid:
            od = po.opt_dict(opt)
            want, wa = po.ref_post_read(od, int(sh["qlen"][r]), int(sh["rep_len"][r]), ref_len, regs, b, mp)
            got, ga = po.post_read(od, int(sh["qlen"][r]), int(sh["rep_len"][r]), ref_len, regs, b, mp)
            assert got.tobytes() == want.tobytes() and ga.tobytes() == wa.tobytes(), (seed, r, opt)
        n_reads += 1
    assert n_reads == len(sh["qlen"])


def test_new_symbols_exported_and_bound():
    L = chaindp.lib()
    for name in NEW_SYMBOLS:
        assert name in chaindp.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None, name


def test_post_opt_mirror():
    assert C.sizeof(P.PostOpt) == 13 * 4
    assert [k for k, _ in P.PostOpt._fields_] == ["flag", "mask_level", "pri_ratio", "best_n", "min_diff", "sub_diff", "max_join_long",
                                                 "max_join_short", "min_join_flank_sc", "min_cnt", "min_chain_score", "match_sc", "is_sr"]
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "chaindp.h")).read()
    body = hdr[hdr.index("typedef struct {\n\tint32_t flag;"):hdr.index("} chaindp_post_opt_t;")]
    assert [ln.split()[1].rstrip(";") for ln in body.splitlines()[1:] if ln.strip()] == [k for k, _ in P.PostOpt._fields_]


def test_post_presets():
    m = P.post_preset("map-ont")
    assert (m.flag, m.min_diff, m.sub_diff, m.best_n, m.min_chain_score, m.match_sc) == (0, 30, 8, 5, 40, 2)
    assert abs(m.mask_level - 0.5) < 1e-7 and abs(m.pri_ratio - 0.8) < 1e-7
    a = P.post_preset("ava-pb")
    assert a.flag & P.MM_F_ALL_CHAINS and a.flag & P.MM_F_NO_LJOIN and a.pri_ratio == 0 and a.min_chain_score == 100 and a.min_diff == 38
    assert P.post_preset("map-ont", best_n=1).best_n == 1


def test_logf_patch_list_reproduces_host_logf():
    """(float)log((double)k), patched at the listed integers, is the host's logf((float)k) for every k in [1, 2^24]."""
    k, v = chaindp.post_logf_patches()
    assert len(k) > 0 and np.all(np.diff(k.astype(np.int64)) > 0) and k[0] >= 1 and k[-1] <= (1 << 24)
    for kk, vv in zip(k.tolist(), v.tolist()):                        # the listed values are the host's
        assert po.host_logf(kk) == np.float32(vv)
    ks = np.arange(1, (1 << 24) + 1, dtype=np.float64)
    cr = np.log(ks).astype(np.float32)
    cr[k.astype(np.int64) - 1] = v
    # the host's logf at every integer, libm's through ctypes (numpy's own float32 log is not libm's)
    libm = po._libm
    host = np.empty(len(ks), np.float32)
    fn = libm.logf
    step = 1 << 16
    for s in range(0, len(ks), step):
        host[s:s + step] = [fn(x) for x in ks[s:s + step].tolist()]
    bad = np.flatnonzero(host.view(np.uint32) != cr.view(np.uint32))
    assert bad.size == 0, f"{bad.size} mismatches, first k = {bad[:5] + 1}"
