"""GPU tier: per-read chaining gaps (chaindp_set_read_gaps; the gap instantiations of k_prepass and k_chain_units, k_frag_read's per-read
max_gap_ref).  Every shape of tests/gap_shapes.py against the oracle read by read, the trimmed pairs of tests/gap_model.py in one
call against the existing call once per gap group and against the composed model.  Bit-exact: integers with array_equal, records by
bytes (div of one-segment reads keeps chaindp_est_err's 2e-6)."""
import numpy as np
import pytest

import frag_model as fm
import gap_model as gm
import gap_shapes as gs
import oracle_lib as ol
from conftest import load_golden, params_from
from minimap2_chaindp_amd import chaindp, params as P
from test_gpu_frag import same_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 12) as d:
        yield d


@pytest.fixture(autouse=True)
def _defaults(dev):
    dev.set_ring(128); dev.set_variant(0); dev.clear_read_gaps()
    yield
    dev.set_ring(128); dev.set_variant(0); dev.clear_read_gaps()


@pytest.mark.parametrize("ring,variant", [(128, 0), (256, 0), (512, 0), (128, 1), (256, 1), (512, 1)])
@pytest.mark.parametrize("name", gs.NAMES)
def test_gap_shapes_equal_the_oracle_read_by_read(dev, name, ring, variant):
    sh, (ef, ep, ev, esoff, eseeds) = gs.shape_with_expected(name)
    dev.set_ring(ring); dev.set_variant(variant)
    dev.upload(sh.off, sh.a, sh.n_segs)
    dev.set_read_gaps(sh.gap_ref, sh.gap_qry)
    dev.run(sh.par)
    f, p, v = dev.download()
    soff, seeds = dev.compact(sh.par)
    for what, x, y in (("f", f, ef), ("p", p, ep), ("v", v, ev)):
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, what, "anchor", int(bad[0]), int(x[bad[0]]), int(y[bad[0]]), "read", int(np.searchsorted(sh.off, bad[0], side="right") - 1))
    assert np.array_equal(soff, esoff), (name, "new_i")
    assert seeds.tobytes() == eseeds.tobytes(), (name, "new_seed[] bytes")
    # the same through the one-call paths
    f2, p2, v2 = dev.chain_batch(sh.par, sh.off, sh.a, sh.n_segs, gaps=(sh.gap_ref, sh.gap_qry))
    assert np.array_equal(f2, ef) and np.array_equal(p2, ep) and np.array_equal(v2, ev)
    dev.upload(sh.off, sh.a, sh.n_segs)
    dev.run_full(sh.par, gaps=(sh.gap_ref, sh.gap_qry))
    soff3, seeds3 = dev.compact(sh.par)
    assert np.array_equal(soff3, esoff) and seeds3.tobytes() == eseeds.tobytes()


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", ["syn_paired_sr", "syn_ties_tinygap"])
def test_equal_gaps_equal_the_plain_run(dev, name, variant):
    """Every read with par's own gaps: the bytes of the plain run (which goes through k_chain_twin and the batch kernels)."""
    g = load_golden(name)
    par = params_from(g["params"])
    dev.set_variant(variant)
    f, p, v = dev.chain_batch(par, g["off"], g["anchors"])
    soff, seeds = dev.compact(par)
    assert np.array_equal(f, g["f"]) and np.array_equal(p, g["p"]) and np.array_equal(v, g["v"])
    n = len(g["off"]) - 1
    other = P.ChainParams(*par.astuple())
    other.max_dist_x, other.max_dist_y = 1, 1                        # ignored while gaps are in force
    f2, p2, v2 = dev.chain_batch(other, g["off"], g["anchors"], gaps=(np.full(n, par.max_dist_x), np.full(n, par.max_dist_y)))
    soff2, seeds2 = dev.compact(other)
    assert f2.tobytes() == f.tobytes() and p2.tobytes() == p.tobytes() and v2.tobytes() == v.tobytes()
    assert np.array_equal(soff2, soff) and seeds2.tobytes() == seeds.tobytes()


@pytest.fixture(scope="module")
def pairs():
    sc, m = gm.scenario_with_model()
    seq, seq_off, ns = fm.batch(sc.frags)
    return sc, m, seq, seq_off, ns


def _map(dev, ix, sc, frags, sel, par, **kw):
    seq, seq_off, ns = fm.batch(frags)
    sel = list(sel)
    return dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid[sel], sc.hash_[sel], sc.ref_len,
                             pe_ori=sc.pe_ori, **kw)


def test_trimmed_pairs_in_one_call_equal_one_call_per_gap_group_and_the_model(dev, pairs):
    sc, m, seq, seq_off, ns = pairs
    ix = dev.load_index(sc.image())
    soff, regs, rep, na = _map(dev, ix, sc, sc.frags, range(len(sc.frags)), sc.par, gaps=sc.gaps)
    assert np.array_equal(rep, m.rep_len) and na == m.n_anchors
    same_hits(soff, regs, m.seg_regs_off, m.regs, ns, "one call with gaps")
    first = np.concatenate(([0], np.cumsum(ns)))
    grp = gm.groups(sc)
    assert len(grp) >= 100
    n_hits = 0
    for (gr, gq), sel in grp:                                        # as a caller had to: the existing call, one per gap group
        par = P.ChainParams(*sc.par.astuple())
        par.max_dist_x, par.max_dist_y = gr, gq
        s2, r2, rep2, _ = _map(dev, ix, sc, [sc.frags[r] for r in sel], sel, par)
        q = 0
        for r in sel:
            for j in range(ns[r]):
                mine = regs[soff[first[r] + j]:soff[first[r] + j + 1]]
                assert mine.tobytes() == r2[s2[q]:s2[q + 1]].tobytes(), ("read", r, "segment", j, (gr, gq))
                n_hits += len(mine); q += 1
        assert np.array_equal(rep2, rep[sel])
    assert n_hits == soff[-1] > 0


def test_map_frags_and_the_stages_with_gaps_equal_the_one_call(dev, pairs):
    sc, m, seq, seq_off, ns = pairs
    ix = dev.load_index(sc.image())
    soff, regs, rep, na = _map(dev, ix, sc, sc.frags, range(len(sc.frags)), sc.par, gaps=sc.gaps)
    # pe_ori is map_frag_seqs' alone: compare the other paths without it
    soff0, regs0, _, _ = dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid, sc.hash_,
                                           sc.ref_len, pe_ori=-1, gaps=sc.gaps)
    dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off, n_segs=ns)
    soff1, regs1, _, _ = dev.map_frags(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, None, None, sc.bid, None, sc.hash_, ns, None, sc.ref_len,
                                       gaps=sc.gaps)
    assert np.array_equal(soff0, soff1) and regs0.tobytes() == regs1.tobytes()
    # map_batch with gaps, the gaps cleared, then frag_post: the run's own copy of the gaps is what mm_select_sub_multi gets
    seg_len = np.diff(seq_off).astype(np.int32)
    mini_off = dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off, n_segs=ns)
    mini = dev.download_minimizers()
    off, a, _, _, _ = dev.collect_seeds(ix, sc.flag, sc.max_occ, mini_off, mini, sc.bid, sc.qlen_sum, n_segs=ns)
    dev.run_full(sc.par, gaps=sc.gaps)
    coff, u, boff, b = dev.backtrack(sc.par, sc.min_cnt)
    dev.gen_regs(sc.hash_, sc.qlen_sum, coff[-1])
    dev.set_read_gaps(*gm.uniform(sc, 1, 1))                         # set and cleared behind the run: neither reaches frag_post
    dev.clear_read_gaps()
    soff2, regs2 = dev.frag_post(sc.opt, sc.ref_len, ns, seg_len=seg_len)
    assert np.array_equal(soff0, soff2) and regs0.tobytes() == regs2.tobytes()


def test_frag_post_takes_the_runs_gap_ref_and_a_rerun_without_gaps_is_uniform(dev):
    """Two-segment reads whose secondary hit lies within ql0 + ql1 + gap_ref of its parent under one gap_ref and beyond it under another
    (pe.c:15-31 through tests/frag_model.py's branches_frag): frag_post behind a gap run follows the run's gap_ref per read, also after
    the gaps were cleared; a rerun without gaps equals the uniform result."""
    import frag_oracle as fo
    import post_oracle as po
    reads = [fm.branches_frag(), fm.branches_frag(rev=True), fm.pri1_frag(), fm.branches_frag()]
    z = fm._pack(reads)
    par, opt = P.preset("sr"), P.post_preset("sr")
    n = len(reads)
    gap_ref = np.array([500, 60, 500, 60], np.int32)                 # chaining itself is the same under both: every step is 10
    gap_qry = np.full(n, 300, np.int32)
    hash_ = np.arange(1, n + 1, dtype=np.uint32) * np.uint32(2654435761)
    ref_len = np.full(8, 1 << 20, np.int32)

    def run(gaps, clear_before_post):
        dev.upload(z["off"], z["anchors"], z["n_segs"])
        if gaps is not None:
            dev.set_read_gaps(*gaps)
        dev.run_full(par)
        coff, u, boff, b = dev.backtrack(par, 2)
        regs_in = dev.gen_regs(hash_, z["qlen"], coff[-1])
        if clear_before_post:
            dev.clear_read_gaps()
        out = dev.frag_post(opt, ref_len, z["n_segs"], seg_len=z["seg_len"], rep_len=z["rep_len"], mini_pos_off=z["mini_pos_off"], mini_pos=z["mini_pos"])
        dev.clear_read_gaps()
        return out, (coff, u, boff, b, regs_in)

    (soff, regs), res_g = run((gap_ref, gap_qry), True)
    (soff_u, regs_u), res_u = run(None, False)                       # par's 500 for every read
    (soff_k, regs_k), _ = run((gap_ref, gap_qry), False)
    assert np.array_equal(soff, soff_k) and regs.tobytes() == regs_k.tobytes()
    # the restatement, read by read, from the hits each run's own chaining left on the device
    od = po.opt_dict(opt)
    first = np.concatenate(([0], np.cumsum(z["n_segs"])))
    for label, so, rg, mgr, (coff, u, boff, b, regs_in) in (("gaps", soff, regs, gap_ref, res_g), ("uniform", soff_u, regs_u, np.full(n, par.max_dist_x), res_u)):
        for r in range(n):
            ql = z["seg_len"][first[r]:first[r + 1]].tolist()
            segs = fo.frag_read(od, int(mgr[r]), int(hash_[r]), ql, int(z["rep_len"][r]), ref_len, regs_in[coff[r]:coff[r + 1]].copy(),
                                b[boff[r]:boff[r + 1]], z["mini_pos"][z["mini_pos_off"][r]:z["mini_pos_off"][r + 1]])
            for j, (exp, _) in enumerate(segs):
                got = rg[so[first[r] + j]:so[first[r] + j + 1]]
                assert got.tobytes() == np.ascontiguousarray(exp, ol.REG_DTYPE).tobytes(), (label, r, j)
    differ = [r for r in range(n) if not np.array_equal(np.diff(soff[first[r]:first[r + 1] + 1]), np.diff(soff_u[first[r]:first[r + 1] + 1]))
              or regs[soff[first[r]]:soff[first[r + 1]]].tobytes() != regs_u[soff_u[first[r]]:soff_u[first[r + 1]]].tobytes()]
    assert differ and set(differ) <= {1, 3}, differ                  # only the reads with another gap_ref, and at least one of them


def test_refusals_leave_the_context_usable(dev):
    sh, (ef, ep, ev, _, _) = gs.shape_with_expected("singletons")
    n = len(sh.off) - 1
    gaps = (sh.gap_ref, sh.gap_qry)
    # a negative gap, a NULL array, more reads than the context has
    bad = sh.gap_ref.copy(); bad[2] = -1
    for args in ((bad, sh.gap_qry), (sh.gap_ref, bad)):
        with pytest.raises(chaindp.ChainDPError, match="-1"):
            dev.set_read_gaps(*args)
    L = chaindp.lib()
    assert L.chaindp_set_read_gaps(dev._ctx, n, None, chaindp._ptr(sh.gap_qry)) == -1
    assert L.chaindp_set_read_gaps(dev._ctx, dev.max_reads + 1, chaindp._ptr(sh.gap_ref), chaindp._ptr(sh.gap_qry)) == -1
    # none of those left gaps in force
    f, p, v = dev.chain_batch(sh.par, sh.off, sh.a)
    uni = gs.expected(sh, np.full(n, sh.par.max_dist_x), np.full(n, sh.par.max_dist_y))
    assert np.array_equal(f, uni[0]) and np.array_equal(p, uni[1])
    # a batch of another read count: refused at entry, before anything is launched or uploaded
    dev.upload(sh.off, sh.a)
    dev.set_read_gaps(sh.gap_ref[:-1], sh.gap_qry[:-1])
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.run(sh.par)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.run_full(sh.par)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.chain_batch(sh.par, sh.off, sh.a)
    sc = fm.scenario(n_frags=8, seed=3)
    ix = dev.load_index(sc.image())
    seq, seq_off, ns = fm.batch(sc.frags)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.map_frag_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid, sc.hash_, sc.ref_len)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.download()                                               # nothing ran: the refused calls launched nothing on the uploaded batch
    # run_device while gaps are in force (refused before it looks at a pointer's target)
    with pytest.raises(chaindp.ChainDPError, match="-1"):
        dev.run_device(sh.par, n, int(sh.off[-1]), 0x1000, 0x1000, 0, 0x1000, 0x1000, 0x1000)
    # and the context is usable: the right count runs, cleared gaps give the uniform result
    dev.set_read_gaps(*gaps)
    dev.run(sh.par)
    f, p, v = dev.download()
    assert np.array_equal(f, ef) and np.array_equal(p, ep) and np.array_equal(v, ev)
    dev.clear_read_gaps()
    dev.run(sh.par)
    f, p, v = dev.download()
    assert np.array_equal(f, uni[0]) and np.array_equal(p, uni[1]) and np.array_equal(v, uni[2])
    assert not (np.array_equal(ef, uni[0]) and np.array_equal(ep, uni[1]))


def test_device_memory_is_constant_over_set_run_clear_rounds(dev):
    sh, (ef, ep, ev, _, _) = gs.shape_with_expected("geometry")
    sizes = []
    for _ in range(4):
        dev.upload(sh.off, sh.a)
        dev.set_read_gaps(sh.gap_ref, sh.gap_qry)
        dev.run_full(sh.par)
        dev.sync()
        dev.clear_read_gaps()
        sizes.append(dev.device_bytes())
    assert len(set(sizes[1:])) == 1 and sizes[0] == sizes[1], sizes
    f, p, v = dev.download()
    assert np.array_equal(f, ef) and np.array_equal(p, ep) and np.array_equal(v, ev)
