"""GPU tier: chain_post + mm_est_err + mm_set_mapq on the GPU (csrc/chaindp_post.hip, chaindp_chain_post / chaindp_map_reads) against
the unmodified reference's results (tests/golden/post, make_post_golden.py) and the restatement (tests/post_oracle.py).  Every byte of
every record is compared except div, which keeps the 2e-6 relative tolerance of chaindp_est_err (the device's logf of a non-integer)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import post_oracle as po
import post_shapes
from minimap2_chaindp_amd import chaindp, params as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POST = sorted(glob.glob(os.path.join(HERE, "golden", "post", "*.npz")))
SEEDS = os.path.join(HERE, "golden", "seeds")
PROG = os.path.join(ROOT, "oracle", "_ref", "minimap2_chaindp")
FA = os.path.join(HERE, "golden", "fa")
OPT_KEYS = [k for k, _ in P.PostOpt._fields_]
DIV_RTOL = 2e-6
LDS_CAP = 256


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 22, max_reads=1 << 12) as d:
        yield d


def post_opt(z, cname):
    return P.PostOpt(**{k: (float(v) if k in ("mask_level", "pri_ratio") else int(v)) for k, v in zip(OPT_KEYS, z[cname + "_opt"])})


def same_records(got, exp, where):
    got = np.ascontiguousarray(got, ol.REG_DTYPE); exp = np.ascontiguousarray(exp, ol.REG_DTYPE)
    assert len(got) == len(exp), (where, len(got), len(exp))
    g2, e2 = got.copy(), exp.copy()
    g2["div"] = 0; e2["div"] = 0
    for i in range(len(got)):
        assert g2[i].tobytes() == e2[i].tobytes(), (where, i, got[i], exp[i])
    unset = exp["div"] < 0
    assert np.array_equal(got["div"] < 0, unset), (where, "div set / unset")
    assert np.array_equal(got["div"][unset], exp["div"][unset]), where
    assert np.allclose(got["div"][~unset], exp["div"][~unset], rtol=DIV_RTOL, atol=0), (where, "div")


def resident_hits(dev, z):
    """upload -> DP -> compaction -> mm_chain_dp_bottom -> mm_gen_regs on the device; checked against the fixture's input hits."""
    pv = [int(x) for x in z["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    dev.upload(z["off"], z["anchors"])
    dev.run_full(par)
    coff, u, boff, b = dev.backtrack(par, pv[7])
    assert np.array_equal(coff, z["chains_off"]) and np.array_equal(boff, z["b_off"])
    regs = dev.gen_regs(z["hash"], z["qlen"], coff[-1])
    assert regs.tobytes() == z["regs_in"].tobytes()
    return par, pv[7], regs


@pytest.mark.parametrize("path", POST, ids=[os.path.basename(p)[:-4] for p in POST])
def test_chain_post_equals_reference(dev, path):
    z = np.load(path, allow_pickle=False)
    resident_hits(dev, z)
    for cname in sorted(k[:-4] for k in z.files if k.endswith("_opt")):
        opt = post_opt(z, cname)
        roff, regs, aoff, a = dev.chain_post(opt, z["ref_len"], qlen=z["qlen"], rep_len=z[cname + "_rep_len"], mini_pos_off=z["mini_pos_off"],
                                             mini_pos=z["mini_pos"], want_anchors=True)
        assert np.array_equal(roff, z[cname + "_regs_off"]), cname
        same_records(regs, z[cname + "_regs"].copy().view(ol.REG_DTYPE).reshape(-1), cname)
        assert np.array_equal(aoff, z["b_off"])
        if cname + "_a" in z.files:
            assert a.tobytes() == z[cname + "_a"].tobytes(), cname


def test_global_memory_path_is_reached_and_exact(dev):
    z = np.load(os.path.join(HERE, "golden", "post", "syn_post.npz"), allow_pickle=False)
    n_hits = np.diff(z["chains_off"])
    assert n_hits.max() > LDS_CAP                                        # one read goes to k_post_read's global-memory path
    resident_hits(dev, z)
    for cname in ("mapont", "pri05_best1", "mask03"):
        roff, regs = dev.chain_post(post_opt(z, cname), z["ref_len"], qlen=z["qlen"], rep_len=z[cname + "_rep_len"], mini_pos_off=z["mini_pos_off"],
                                    mini_pos=z["mini_pos"])
        r = int(np.argmax(n_hits))
        exp = z[cname + "_regs"].copy().view(ol.REG_DTYPE).reshape(-1)
        eoff = z[cname + "_regs_off"]
        same_records(regs[roff[r]:roff[r + 1]], exp[eoff[r]:eoff[r + 1]], (cname, "big read"))


@pytest.mark.parametrize("seed", [3, 17, 29])
def test_fuzz_against_restatement(dev, seed):
    rng = np.random.default_rng(seed)
    sh = post_shapes.shapes(seed=seed, n_random=6)
    par = P.preset("map-ont")
    R = len(sh["qlen"])
    hash_ = rng.integers(0, 1 << 32, size=R, dtype=np.uint64).astype(np.uint32)
    dev.upload(sh["off"], sh["anchors"])
    dev.run_full(par)
    coff, u, boff, b = dev.backtrack(par, 3)
    regs_in = dev.gen_regs(hash_, sh["qlen"], coff[-1])
    ref_len = np.full(int(regs_in["rid"].max()) + 1, 1 << 27, np.int32)
    for _ in range(4):
        opt = P.post_preset("map-ont", mask_level=float(rng.choice([0.2, 0.5, 0.8])), pri_ratio=float(rng.choice([0.0, 0.5, 0.8, 0.95])),
                            best_n=int(rng.integers(1, 8)), max_join_long=int(rng.choice([2000, 20000])), min_join_flank_sc=int(rng.choice([200, 1000])),
                            flag=int(rng.choice([0, 0, P.MM_F_NO_LJOIN, P.MM_F_CIGAR])), min_chain_score=int(rng.choice([40, 100])))
        rep = rng.integers(0, 5000, size=R).astype(np.int32)
        roff, regs = dev.chain_post(opt, ref_len, qlen=sh["qlen"], rep_len=rep, mini_pos_off=sh["mini_pos_off"], mini_pos=sh["mini_pos"])
        od = po.opt_dict(opt)
        for r in range(R):
            mp = sh["mini_pos"][sh["mini_pos_off"][r]:sh["mini_pos_off"][r + 1]]
            exp, _ = po.post_read(od, int(sh["qlen"][r]), int(rep[r]), ref_len, regs_in[coff[r]:coff[r + 1]], b[boff[r]:boff[r + 1]], mp)
            same_records(regs[roff[r]:roff[r + 1]], exp, (seed, r, od))


def _seed_fixture(name):
    return np.load(os.path.join(SEEDS, name + ".npz"), allow_pickle=False)


@pytest.mark.parametrize("name", ["mt_orang_vs_human_mapont", "inv_mapont", "syn_repeats_mapont"])
def test_map_reads_equals_map_batch_then_chain_post(dev, name):
    g = _seed_fixture(name)
    pv = [int(x) for x in g["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    R = len(g["qlen"])
    hash_ = (np.arange(R, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    ref_len = np.full(1 << 16, 1 << 20, np.int32)
    opt = P.post_preset("map-ont")
    ix = dev.load_index([g["img_B"], g["img_H"], g["img_V"], g["img_P"]])
    roff, regs, rep, na = dev.map_reads(ix, int(g["flag"]), int(g["mid_occ"]), par, pv[7], opt, g["mini_off"], g["mini"], g["bid"], g["qlen"], hash_, ref_len)
    boff, bregs, brep, bna = dev.map_batch(ix, int(g["flag"]), int(g["mid_occ"]), par, pv[7], g["mini_off"], g["mini"], g["bid"], g["qlen"], hash_)
    assert np.array_equal(rep, brep) and na == bna
    roff2, regs2 = dev.chain_post(opt, ref_len)                          # qlen, rep_len, mini_pos resident
    assert np.array_equal(roff, roff2) and regs.tobytes() == regs2.tobytes()
    # and the restatement on what map_batch returned
    coff, u, bo, b = dev.backtrack(par, pv[7])
    for r in range(R):
        mp = g["mini_pos"][g["mp_off"][r]:g["mp_off"][r + 1]]
        exp, _ = po.post_read(po.opt_dict(opt), int(g["qlen"][r]), int(rep[r]), ref_len, bregs[boff[r]:boff[r + 1]], b[bo[r]:bo[r + 1]], mp)
        same_records(regs[roff[r]:roff[r + 1]], exp, (name, r))


def test_device_logf_equals_host_logf(dev):
    assert dev.post_logf_selftest(1 << 24) == 0


def test_capacity_leaves_regs_off_valid(dev):
    z = np.load(os.path.join(HERE, "golden", "post", "syn_post.npz"), allow_pickle=False)
    resident_hits(dev, z)
    opt = post_opt(z, "mapont")
    with pytest.raises(chaindp.ChainDPError, match="-2"):
        dev.chain_post(opt, z["ref_len"], qlen=z["qlen"], rep_len=z["mapont_rep_len"], mini_pos_off=z["mini_pos_off"], mini_pos=z["mini_pos"], regs_cap=3)
    roff = np.zeros(len(z["qlen"]) + 1, np.int64)
    regs = np.zeros(3, ol.REG_DTYPE)
    rc = dev._lib.chaindp_chain_post(dev._ctx, chaindp.C.byref(opt), chaindp._ptr(np.ascontiguousarray(z["qlen"], np.int32)),
                                     chaindp._ptr(np.ascontiguousarray(z["mapont_rep_len"], np.int32)), chaindp._ptr(z["ref_len"]), len(z["ref_len"]),
                                     chaindp._ptr(z["mini_pos_off"]), chaindp._ptr(z["mini_pos"]), chaindp._ptr(roff), chaindp._ptr(regs), 3, None, None)
    assert rc == -2 and np.array_equal(roff, z["mapont_regs_off"])


def test_refusals(dev):
    z = np.load(os.path.join(HERE, "golden", "post", "syn_repeats_mapont.npz"), allow_pickle=False)
    opt = post_opt(z, "mapont")
    kw = dict(qlen=z["qlen"], rep_len=z["mapont_rep_len"], mini_pos_off=z["mini_pos_off"], mini_pos=z["mini_pos"])
    pv = [int(x) for x in z["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    # no gen_regs on this batch
    dev.upload(z["off"], z["anchors"]); dev.run_full(par); dev.backtrack(par, pv[7])
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.chain_post(opt, z["ref_len"], **kw)
    # an est_err upload in between
    regs = dev.gen_regs(z["hash"], z["qlen"], int(z["chains_off"][-1]))
    dev.chain_post(opt, z["ref_len"], **kw)
    dev.est_err(z["chains_off"], regs, z["qlen"], z["ref_len"], z["mini_pos_off"], z["mini_pos"])
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.chain_post(opt, z["ref_len"], **kw)
    # a read with n_segs > 1
    ns = np.ones(len(z["qlen"]), np.int32); ns[-1] = 2
    dev.upload(z["off"], z["anchors"], n_segs=ns); dev.run_full(par)
    coff, _, _, _ = dev.backtrack(par, pv[7])
    dev.gen_regs(z["hash"], z["qlen"], int(coff[-1]))
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.chain_post(opt, z["ref_len"], **kw)


def test_existing_calls_unchanged_after_chain_post(dev):
    """chain_post writes to buffers of its own: est_err on the gen_regs hits afterwards still gives the regs fixture's result."""
    rg = np.load(os.path.join(HERE, "golden", "regs", "syn_repeats_mapont.npz"), allow_pickle=False)
    z = np.load(os.path.join(HERE, "golden", "post", "syn_repeats_mapont.npz"), allow_pickle=False)
    _, _, regs = resident_hits(dev, z)
    dev.chain_post(post_opt(z, "mapont"), z["ref_len"], qlen=z["qlen"], rep_len=z["mapont_rep_len"], mini_pos_off=z["mini_pos_off"],
                   mini_pos=z["mini_pos"])
    regs2 = dev.gen_regs(z["hash"], z["qlen"], int(z["chains_off"][-1]))       # (re-made; equal to the first)
    assert regs2.tobytes() == regs.tobytes()
    got, _, _ = dev.est_err(rg["chains_off"], regs, rg["qlen"], rg["ref_len"], z["mini_pos_off"], z["mini_pos"])
    exp = rg["regs_div"].copy().view(ol.REG_DTYPE).reshape(-1)
    same_records(got, exp, "est_err after chain_post")


# ---- end to end: the reference program's PAF lines ---------------------------------------------------------------------------------

def _fasta(path):
    names, lens, cur = [], [], None
    for ln in open(path):
        if ln.startswith(">"):
            names.append(ln[1:].split()[0]); lens.append(0)
        else:
            lens[-1] += len(ln.strip())
    return names, lens


def _wang(key):
    m = 0xffffffff
    key = (key + (~(key << 15) & m)) & m
    key ^= key >> 10
    key = (key + (key << 3)) & m
    key ^= key >> 6
    key = (key + (~(key << 11) & m)) & m
    key ^= key >> 16
    return key


def _read_hash(name, qlen, seed=11):                                    # map.c:345-347
    h = ord(name[0])
    for ch in name[1:]:
        h = ((h << 5) - h + ord(ch)) & 0xffffffff
    h ^= (_wang(qlen) + _wang(seed)) & 0xffffffff
    return _wang(h)


@pytest.mark.skipif(not os.path.exists(PROG), reason="reference program not built (needs /root/reference: make -C oracle ref-prog)")
@pytest.mark.parametrize("name,target,query", [("mt_orang_vs_human_mapont", "MT-human.fa", "MT-orang.fa"), ("inv_mapont", "t-inv.fa", "q-inv.fa")])
def test_map_reads_reproduces_reference_program_paf(dev, name, target, query):
    r = subprocess.run([PROG, "-x", "map-ont", "-t", "12", os.path.join(FA, target), os.path.join(FA, query)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    paf = [ln.split("\t") for ln in r.stdout.splitlines() if ln.strip()]
    g = _seed_fixture(name)
    qnames, qlens = _fasta(os.path.join(FA, query))
    tnames, tlens = _fasta(os.path.join(FA, target))
    assert list(g["qlen"]) == qlens
    pv = [int(x) for x in g["params"]]
    par = P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=1)
    hash_ = np.array([_read_hash(n, l) for n, l in zip(qnames, qlens)], np.uint32)
    ix = dev.load_index([g["img_B"], g["img_H"], g["img_V"], g["img_P"]])
    roff, regs, _, _ = dev.map_reads(ix, int(g["flag"]), int(g["mid_occ"]), par, pv[7], P.post_preset("map-ont"), g["mini_off"], g["mini"], g["bid"],
                                     g["qlen"], hash_, np.array(tlens, np.int32))
    mine = []
    for q in range(len(qnames)):
        for x in regs[roff[q]:roff[q + 1]]:
            mine.append((qnames[q], x))
    assert len(mine) == len(paf), (len(mine), len(paf), r.stdout)
    for (qn, x), p in zip(mine, paf):
        tags = dict((t.split(":", 2)[0], t.split(":", 2)[2]) for t in p[12:])
        primary = x["parent"] == x["id"]
        assert p[0] == qn and p[5] == tnames[x["rid"]]
        assert (int(p[2]), int(p[3]), p[4], int(p[7]), int(p[8])) == (x["qs"], x["qe"], "+-"[int(x["bits"]) >> 10 & 1], x["rs"], x["re"]), (p, x)
        assert int(p[11]) == int(x["bits"]) & 0xff, (p, x)
        assert tags["tp"] == ("P" if primary else "S") and int(tags["cm"]) == x["cnt"] and int(tags["s1"]) == x["score"]
        if primary:
            assert int(tags["s2"]) == x["subsc"]
        if "dv" in tags:
            d = float(x["div"])
            lo, hi = d * (1 - DIV_RTOL), d * (1 + DIV_RTOL)
            assert tags["dv"] in {("0" if v == 0 else "%.4f" % np.float32(v)) for v in (d, lo, hi)}, (tags["dv"], d)
        else:
            assert not (0.0 <= float(x["div"]) <= 1.0)
