"""GPU tier: reads of several segments on the GPU (csrc/chaindp_frag.hip; chaindp_frag_post / chaindp_map_frags / chaindp_map_frag_seqs)
against the unmodified reference's results (tests/golden/frag, make_frag_golden.py), the restatement (tests/frag_oracle.py) and the
composed CPU model (tests/frag_model.py).  Every byte of every record, offset and anchor is compared; the one exception is div of the hits
of one-segment reads, which keeps the 2e-6 relative tolerance of chaindp_est_err.  div of a split hit must be exactly -1.0f."""
import glob
import os

import numpy as np
import pytest

import e2e_model as em
import frag_model as fm
import frag_oracle as fo
import oracle_lib as ol
from minimap2_chaindp_amd import chaindp, params as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FRAG = sorted(glob.glob(os.path.join(HERE, "golden", "frag", "*.npz")))
OPT_KEYS = [k for k, _ in P.PostOpt._fields_]
DIV_RTOL = 2e-6
LDS_CAP = 64


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 22, max_reads=1 << 13) as d:
        yield d


def post_opt(z, cname):
    return P.PostOpt(**{k: (float(v) if k in ("mask_level", "pri_ratio") else int(v)) for k, v in zip(OPT_KEYS, z[cname + "_opt"])})


def same_hits(got_off, got, exp_off, exp, n_segs, where):
    """Offsets equal; every record byte-equal -- div of one-segment reads within DIV_RTOL, div of split hits exactly -1."""
    assert np.array_equal(got_off, exp_off), where
    got = np.ascontiguousarray(got, ol.REG_DTYPE); exp = np.ascontiguousarray(exp, ol.REG_DTYPE)
    assert len(got) == len(exp) == int(exp_off[-1]), (where, len(got), len(exp))
    single = np.repeat(np.repeat(np.asarray(n_segs) == 1, n_segs), np.diff(exp_off))
    g2, e2 = got.copy(), exp.copy()
    g2["div"][single] = 0; e2["div"][single] = 0
    if g2.tobytes() != e2.tobytes():
        i = int(np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(g2, e2)])[0][0])
        raise AssertionError((where, i, got[i], exp[i]))
    assert (got["div"][~single].view(np.uint32) == np.float32(-1.0).view(np.uint32)).all(), (where, "div of a split hit")
    gs, es = got["div"][single], exp["div"][single]
    unset = es < 0
    assert np.array_equal(gs < 0, unset) and np.array_equal(gs[unset], es[unset]), (where, "div set / unset")
    assert np.allclose(gs[~unset], es[~unset], rtol=DIV_RTOL, atol=0), (where, "div")


def chain_par(z):
    pv = [int(x) for x in z["params"]]
    return P.ChainParams(max_dist_x=pv[0], max_dist_y=pv[1], bw=pv[2], max_skip=pv[3], min_sc=pv[4], is_cdna=pv[5], n_segs=pv[6]), pv[7]


def resident_hits(dev, z):
    """upload -> DP -> compaction -> mm_chain_dp_bottom -> mm_gen_regs on the device; checked against the fixture's input hits."""
    par, min_cnt = chain_par(z)
    dev.upload(z["off"], z["anchors"], n_segs=z["n_segs"])
    dev.run_full(par)
    coff, u, boff, b = dev.backtrack(par, min_cnt)
    assert np.array_equal(coff, z["chains_off"]) and np.array_equal(boff, z["b_off"]) and b.tobytes() == z["b"].tobytes()
    regs = dev.gen_regs(z["hash"], z["qlen"], coff[-1])
    assert regs.tobytes() == z["regs_in"].tobytes()
    return par, min_cnt, regs, u, b


@pytest.mark.parametrize("cap", [LDS_CAP, 0], ids=["lds", "scratch"])
@pytest.mark.parametrize("path", FRAG, ids=[os.path.basename(p)[:-4] for p in FRAG])
def test_frag_post_equals_reference(dev, path, cap):
    """Every fixture and option set; cap 0 sends every fragment and segment through the global-scratch path."""
    z = np.load(path, allow_pickle=False)
    resident_hits(dev, z)
    dev.set_frag_lds_cap(cap)
    try:
        for cname in sorted(k[:-4] for k in z.files if k.endswith("_opt")):
            soff, regs, aoff, a = dev.frag_post(post_opt(z, cname), z["ref_len"], z["n_segs"], seg_len=z["seg_len"], rep_len=z[cname + "_rep_len"],
                                                mini_pos_off=z["mini_pos_off"], mini_pos=z["mini_pos"], want_anchors=True)
            same_hits(soff, regs, z[cname + "_seg_regs_off"], z[cname + "_regs"].copy().view(ol.REG_DTYPE).reshape(-1), z["n_segs"], (path, cname, cap))
            if cname + "_seg_a" in z.files:
                assert np.array_equal(aoff, z[cname + "_seg_a_off"]), cname
                assert a.tobytes() == z[cname + "_seg_a"].tobytes(), cname
    finally:
        dev.set_frag_lds_cap(LDS_CAP)


def test_a_fragment_above_the_lds_cap_is_in_the_fixtures():
    z = np.load(os.path.join(HERE, "golden", "frag", "syn_frag.npz"), allow_pickle=False)
    assert np.diff(z["chains_off"]).max() > LDS_CAP and np.diff(z["allchains_seg_regs_off"]).max() > LDS_CAP


@pytest.mark.parametrize("seed", [3, 17])
def test_fuzz_against_restatement(dev, seed):
    rng = np.random.default_rng(seed)
    sh = fm.shapes(seed=seed, n_random=10)
    par = P.preset("sr")
    R = len(sh["qlen"])
    hash_ = rng.integers(0, 1 << 32, size=R, dtype=np.uint64).astype(np.uint32)
    dev.upload(sh["off"], sh["anchors"], n_segs=sh["n_segs"])
    dev.run_full(par)
    coff, u, boff, b = dev.backtrack(par, 2)
    regs_in = dev.gen_regs(hash_, sh["qlen"], coff[-1])
    ref_len = np.full(int(regs_in["rid"].max()) + 1, 1 << 27, np.int32)
    first = np.concatenate([[0], np.cumsum(sh["n_segs"])])
    for _ in range(4):
        opt = P.post_preset("sr", mask_level=float(rng.choice([0.2, 0.5, 0.8])), pri_ratio=float(rng.choice([0.0, 0.3, 0.5, 0.8, 0.95])),
                            best_n=int(rng.integers(1, 8)), flag=int(rng.choice([P.MM_F_SR, 0, P.MM_F_SR | P.MM_F_CIGAR])), max_join_long=400,
                            min_join_flank_sc=40, is_sr=int(rng.integers(0, 2)))
        rep = rng.integers(0, 300, size=R).astype(np.int32)
        soff, regs = dev.frag_post(opt, ref_len, sh["n_segs"], seg_len=sh["seg_len"], rep_len=rep, mini_pos_off=sh["mini_pos_off"], mini_pos=sh["mini_pos"])
        od = fm.po.opt_dict(opt)
        exp = []
        for r in range(R):
            mp = sh["mini_pos"][sh["mini_pos_off"][r]:sh["mini_pos_off"][r + 1]]
            exp += [x for x, _ in fo.frag_read(od, par.max_dist_x, int(hash_[r]), sh["seg_len"][first[r]:first[r + 1]], int(rep[r]), ref_len,
                                               regs_in[coff[r]:coff[r + 1]], b[boff[r]:boff[r + 1]], mp)]
        same_hits(soff, regs, em._offsets(exp), em._cat(exp, np.zeros(0, ol.REG_DTYPE)), sh["n_segs"], (seed, od))


# ---- bases in: the seeded sr batch ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    sc = fm.scenario(n_frags=400, seed=3)
    return sc, sc.image()


def _seqs(frags):
    return fm.batch(frags)


def _resident(dev, n_c, n_b):
    """What chaindp_gen_regs / chaindp_backtrack left in HBM, as it lies there: (hits, u, chain anchors)."""
    out = (np.zeros(max(n_c, 1), ol.REG_DTYPE), np.zeros(max(n_c, 1), np.uint64), np.zeros((max(n_b, 1), 2), np.uint64))
    fn = chaindp.lib().chaindp_debug_bottom
    for which, arr, n, size in ((7, out[0], n_c, 80), (8, out[1], n_c, 8), (9, out[2], n_b, 16)):
        if n:
            assert fn(dev._ctx, which, chaindp._ptr(arr), n * size) == 0
    return out[0][:n_c], out[1][:n_c], out[2][:n_b]


def test_map_frag_seqs_without_pe_ori_equals_the_model(dev, small):
    sc, img = small
    ix = dev.load_index(img)
    seq, seq_off, ns = _seqs(sc.frags)
    soff, regs, rep, na = dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid, sc.hash_,
                                            sc.ref_len, pe_ori=-1)
    m = fm.model_of(sc, img, pe_ori=-1)
    same_hits(soff, regs, m.seg_regs_off, m.regs, ns, "pe_ori -1")
    assert np.array_equal(rep, m.rep_len) and na == m.n_anchors


def test_map_frags_equals_stages_and_map_frag_seqs_equals_sketch_then_map_frags(dev, small):
    sc, img = small
    ix = dev.load_index(img)
    seq, seq_off, ns = _seqs(sc.frags)
    seg_len = np.diff(seq_off).astype(np.int32)
    # stage by stage
    mini_off = dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off, n_segs=ns)
    mini = dev.download_minimizers()
    qlen = np.add.reduceat(seg_len, np.concatenate([[0], np.cumsum(ns)[:-1]])).astype(np.int32)
    off, a, rep, mpo, mp = dev.collect_seeds(ix, sc.flag, sc.max_occ, mini_off, mini, sc.bid, qlen, n_segs=ns)
    dev.run_full(sc.par)
    coff, u, boff, b = dev.backtrack(sc.par, sc.min_cnt)
    before = dev.gen_regs(sc.hash_, qlen, coff[-1])
    err1 = dev.est_err(coff, before, qlen, sc.ref_len)[0]                 # reads the resident chain anchors and mini_pos
    assert dev.gen_regs(sc.hash_, qlen, coff[-1]).tobytes() == before.tobytes()
    res1 = _resident(dev, int(coff[-1]), int(boff[-1]))
    assert res1[0].tobytes() == before.tobytes() and res1[1].tobytes() == u.tobytes() and res1[2].tobytes() == b.tobytes()
    soff, regs, aoff, sa = dev.frag_post(sc.opt, sc.ref_len, ns, seg_len=seg_len, want_anchors=True)
    assert soff[-1] > 0
    res2 = _resident(dev, int(coff[-1]), int(boff[-1]))                   # the resident hits, u[] and chain anchors themselves, downloaded
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res1, res2))
    # what backtrack / gen_regs left resident is byte-identical afterwards: gen_regs reads the chains, est_err the anchors and mini_pos
    assert dev.gen_regs(sc.hash_, qlen, coff[-1]).tobytes() == before.tobytes()
    assert dev.est_err(coff, before, qlen, sc.ref_len)[0].tobytes() == err1.tobytes()
    # one call, minimizers in
    soff2, regs2, rep2, na2 = dev.map_frags(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, mini_off, mini, sc.bid, qlen, sc.hash_, ns, seg_len, sc.ref_len)
    assert np.array_equal(soff, soff2) and regs.tobytes() == regs2.tobytes() and np.array_equal(rep, rep2) and na2 == int(off[-1])
    # sketch, then map_frags on the resident minimizers; and bases in
    dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off, n_segs=ns)
    soff3, regs3, _, _ = dev.map_frags(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, None, None, sc.bid, None, sc.hash_, ns, None, sc.ref_len)
    soff4, regs4, rep4, na4 = dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid, sc.hash_, sc.ref_len)
    assert np.array_equal(soff, soff3) and regs.tobytes() == regs3.tobytes()
    assert np.array_equal(soff, soff4) and regs.tobytes() == regs4.tobytes() and np.array_equal(rep, rep4) and na4 == na2


def test_map_batch_then_frag_post_on_a_uniform_paired_batch(dev, small):
    sc, img = small
    ix = dev.load_index(img)
    sel = [i for i, f in enumerate(sc.frags) if len(f) == 2]
    frags = [sc.frags[i] for i in sel]
    seq, seq_off, ns = _seqs(frags)
    seg_len = np.diff(seq_off).astype(np.int32)
    qlen = (seg_len[0::2] + seg_len[1::2]).astype(np.int32)
    mini_off = dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off, n_segs=ns)
    mini = dev.download_minimizers()
    dev.map_batch(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, mini_off, mini, sc.bid[sel], qlen, sc.hash_[sel])   # par.n_segs = 2 for every read
    soff, regs = dev.frag_post(sc.opt, sc.ref_len, ns, seg_len=seg_len)
    soff2, regs2, _, _ = dev.map_frags(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, mini_off, mini, sc.bid[sel], qlen, sc.hash_[sel], ns, seg_len, sc.ref_len)
    assert soff[-1] > 0 and np.array_equal(soff, soff2) and regs.tobytes() == regs2.tobytes()


def _flip(frags, soff, regs, pe_ori):
    """map.c:620-631 restated: the hits of the segments worker_for turned round, back on the read's strand."""
    regs = regs.copy()
    q = 0
    for f in frags:
        for j, s in enumerate(f):
            if len(f) == 2 and ((j == 0 and pe_ori >> 1 & 1) or (j == 1 and pe_ori & 1)):
                for k in range(soff[q], soff[q + 1]):
                    t = int(regs[k]["qs"])
                    regs[k]["qs"] = len(s) - int(regs[k]["qe"])
                    regs[k]["qe"] = len(s) - t
                    regs[k]["bits"] = int(regs[k]["bits"]) ^ (1 << 10)
            q += 1
    return regs


@pytest.mark.parametrize("pe_ori", [1, 2, 3])
def test_pe_ori(dev, small, pe_ori):
    sc, img = small
    ix = dev.load_index(img)
    args = (ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt)
    seq, seq_off, ns = _seqs(sc.frags)
    soff, regs, rep, na = dev.map_frag_seqs(*args, seq, seq_off, ns, sc.bid, sc.hash_, sc.ref_len, pe_ori=pe_ori)
    # the same reads with those segments reverse-complemented by the test, mapped as they are, then flipped back
    turned = [[em.revcomp(s) if len(f) == 2 and ((j == 0 and pe_ori >> 1 & 1) or (j == 1 and pe_ori & 1)) else s for j, s in enumerate(f)] for f in sc.frags]
    seq2, seq_off2, _ = _seqs(turned)
    soff2, regs2, rep2, na2 = dev.map_frag_seqs(*args, seq2, seq_off2, ns, sc.bid, sc.hash_, sc.ref_len, pe_ori=-1)
    assert np.array_equal(soff, soff2) and np.array_equal(rep, rep2) and na == na2
    assert regs.tobytes() == _flip(sc.frags, soff2, regs2, pe_ori).tobytes()
    # and the model
    m = fm.model_of(sc, img, pe_ori=pe_ori)
    same_hits(soff, regs, m.seg_regs_off, m.regs, ns, ("pe_ori", pe_ori))
    assert np.array_equal(rep, m.rep_len) and na == m.n_anchors
    # one-segment reads are untouched by any pe_ori
    plain = dev.map_frag_seqs(*args, seq, seq_off, ns, sc.bid, sc.hash_, sc.ref_len, pe_ori=-1)
    first = np.concatenate([[0], np.cumsum(ns)])
    n1 = 0
    for r in np.nonzero(ns == 1)[0]:
        q = first[r]
        assert regs[soff[q]:soff[q + 1]].tobytes() == plain[1][plain[0][q]:plain[0][q + 1]].tobytes()
        n1 += 1
    assert n1 > 0


def test_end_to_end_equals_the_composed_model(dev):
    """Several thousand 2 x 150 bp fragments, fragment by fragment against the model, mapped as the sr preset maps them (pe_ori = 1)."""
    sc = fm.scenario(n_frags=3000, seed=1)
    img = sc.image()
    m = fm.model_of(sc, img, pe_ori=1)
    cov = fm.coverage(m)
    print(cov)
    assert cov["both_segments"] > 0 and cov["multi_dropped"] > 0 and cov["reverse"] > 0 and cov["one_segment"] > 0 and cov["secondary"] > 0
    assert cov["empty_segments"] > 0
    ix = dev.load_index(img)
    seq, seq_off, ns = _seqs(sc.frags)
    soff, regs, rep, na = dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid, sc.hash_,
                                            sc.ref_len, pe_ori=1)
    assert np.array_equal(rep, m.rep_len) and na == m.n_anchors
    same_hits(soff, regs, m.seg_regs_off, m.regs, ns, "e2e")


# ---- contracts -----------------------------------------------------------------------------------------------------------------------

def test_contracts(dev):
    z = np.load(os.path.join(HERE, "golden", "frag", "syn_frag.npz"), allow_pickle=False)
    opt = post_opt(z, "sr")
    kw = dict(seg_len=z["seg_len"], rep_len=z["sr_rep_len"], mini_pos_off=z["mini_pos_off"], mini_pos=z["mini_pos"])
    par, min_cnt = chain_par(z)
    # no gen_regs on this batch
    dev.upload(z["off"], z["anchors"], n_segs=z["n_segs"]); dev.run_full(par); dev.backtrack(par, min_cnt)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.frag_post(opt, z["ref_len"], z["n_segs"], **kw)
    regs_in = dev.gen_regs(z["hash"], z["qlen"], int(z["chains_off"][-1]))
    # regs_cap too small: CHAINDP_ERR_CAPACITY with the offsets filled
    with pytest.raises(chaindp.ChainDPError, match="-2"):
        dev.frag_post(opt, z["ref_len"], z["n_segs"], regs_cap=3, **kw)
    S = int(z["n_segs"].sum())
    soff = np.zeros(S + 1, np.int64)
    regs = np.zeros(3, ol.REG_DTYPE)
    ptr = chaindp._ptr
    ns, sl, rl = (np.ascontiguousarray(z[k], np.int32) for k in ("n_segs", "seg_len", "sr_rep_len"))
    rc = dev._lib.chaindp_frag_post(dev._ctx, chaindp.C.byref(opt), S, ptr(ns), ptr(sl), ptr(rl), ptr(z["ref_len"]), len(z["ref_len"]), ptr(z["mini_pos_off"]),
                                    ptr(z["mini_pos"]), ptr(soff), ptr(regs), 3, None, None)
    assert rc == -2 and np.array_equal(soff, z["sr_seg_regs_off"])
    # seg_len that does not add up to the batch's qlen; segments that do not add up
    bad = z["seg_len"].copy(); bad[0] += 1
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.frag_post(opt, z["ref_len"], z["n_segs"], **dict(kw, seg_len=bad))
    ns3 = z["n_segs"].copy(); ns3[0] += 1
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.frag_post(opt, z["ref_len"], ns3, **dict(kw, seg_len=np.concatenate([[0], z["seg_len"]])))
    # the single-segment calls still refuse the batch
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.chain_post(opt, z["ref_len"], qlen=z["qlen"], rep_len=z["sr_rep_len"], mini_pos_off=z["mini_pos_off"], mini_pos=z["mini_pos"])
    # the context is usable afterwards, and what was resident is as it was
    soff2, regs2 = dev.frag_post(opt, z["ref_len"], z["n_segs"], **kw)
    same_hits(soff2, regs2, z["sr_seg_regs_off"], z["sr_regs"].copy().view(ol.REG_DTYPE).reshape(-1), z["n_segs"], "after refusals")
    assert dev.gen_regs(z["hash"], z["qlen"], int(z["chains_off"][-1])).tobytes() == regs_in.tobytes()
    # an est_err upload replaces the resident hits: refused
    nonsr = post_opt(z, "nonsr")
    dev.est_err(z["chains_off"], regs_in, z["qlen"], z["ref_len"], z["mini_pos_off"], z["mini_pos"])
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.frag_post(nonsr, z["ref_len"], z["n_segs"], **kw)


def test_map_reads_and_map_seqs_still_refuse_several_segments(dev, small):
    sc, img = small
    ix = dev.load_index(img)
    sel = [i for i, f in enumerate(sc.frags) if len(f) == 2][:8]
    seq, seq_off, ns = _seqs([sc.frags[i] for i in sel])
    one_off = seq_off[::2].copy()                                         # every pair as one sequence
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.map_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, one_off, sc.bid[sel], sc.hash_[sel], sc.ref_len)
    mini_off = dev.sketch(sc.w, sc.k, sc.hpc, seq, one_off)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.map_reads(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, mini_off, dev.download_minimizers(), sc.bid[sel], np.diff(one_off).astype(np.int32),
                      sc.hash_[sel], sc.ref_len)
