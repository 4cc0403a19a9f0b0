"""GPU tier of mapping with base alignment in one call (Device.map_align_seqs / Device.align_resident, chaindp_map_align.h) against the
reference's recorded results of a run with MM_F_CIGAR (tests/golden/map_align/, made by tests/golden/make_map_align_golden.py): every
word of the final regions, of what r->p held, dp_max2, every CIGAR word, a[] with its marks, and the regions and anchors as the
skeleton's mm_squeeze_a left them.  div is judged by same_records / DIV_RTOL of test_gpu_post.py (the device's logf in mm_est_err).
(a) the one call equals every golden; (b) the staged path -- sketch, collect_seeds + run_full + backtrack + gen_regs (map_batch's stages),
chain_post(MM_F_CIGAR, want_anchors), the numpy squeeze, align_reads_post -- equals (a) byte for byte; (c) align_resident after
map_seqs(MM_F_CIGAR) equals (a), and what it hands over equals the golden's tap; (d) every scene and the hand-made lists under LDS caps
1 and 5; (e) a scene tiled over the scan's tile edges; (f) the capacities and the fetch; (g) two presets on one context; (h) every
refusal; (i) no reads, and reads without regions."""
import numpy as np
import pytest

import map_align_shapes as S
from minimap2_chaindp_amd import chaindp, params as P
from test_gpu_post import same_records
from test_map_align_cpu import load

pytestmark = pytest.mark.gpu
OUT = ("regs_off", "regs", "extra", "dp_max2", "cigar_off", "cigar")


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 21, max_reads=1 << 12) as d:
        yield d


_loaded = {}


def index_of(dev, name):
    if (id(dev), name) not in _loaded:
        _loaded[id(dev), name] = dev.load_index(S.scene(name).image())
    return _loaded[id(dev), name]


def one_call(dev, name, t=None, **kw):
    """map_align_seqs on a scene (t: a tiling of its reads), the targets set first."""
    sc = S.scene(name)
    t = t or sc
    dev.align_set_targets(sc.tseq_off, sc.tseq)
    return dev.map_align_seqs(index_of(dev, name), sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, sc.aopt, t.seq, t.seq_off, t.bid, t.hash_,
                              sc.ref_len, **kw)


def staged(dev, name):
    """The same work composed from the calls there were before: ((a, regs_off, regs, extra, dp_max2, cigar_off, cigar), rep_len, n_anchors)."""
    sc = S.scene(name)
    ix = index_of(dev, name)
    dev.align_set_targets(sc.tseq_off, sc.tseq)
    qlen = np.diff(sc.seq_off).astype(np.int32)
    dev.sketch(sc.w, sc.k, sc.hpc, sc.seq, sc.seq_off)
    a_off, _, rep, _, _ = dev.collect_seeds(ix, sc.flag, sc.max_occ, None, None, sc.bid, None)
    dev.run_full(sc.par)
    coff, _, _, _ = dev.backtrack(sc.par, sc.min_cnt)
    dev.gen_regs(sc.hash_, qlen, int(coff[-1]))
    roff, regs, aoff, a = dev.chain_post(sc.opt, sc.ref_len, want_anchors=True)
    regs2, aoff2, a2 = S.squeeze(roff, regs, aoff, a)
    return dev.align_reads_post(sc.aopt, sc.opt, sc.seq_off, sc.seq, aoff2, a2, roff, regs2, rep), rep, int(a_off[-1])


def equals_golden(got, g, where, rows=None):
    """got: (regs_off, regs, extra, dp_max2, cigar_off, cigar, ...) of a call; g: a golden, or with rows the golden tiled to those reads."""
    want = {k: g[k + "_out"] for k in OUT} if rows is None else tile_golden(g, rows)
    assert np.array_equal(got[0], want["regs_off"]), (where, "regs_off")
    same_records(got[1], want["regs"].view(chaindp.REG_DTYPE) if want["regs"].dtype != chaindp.REG_DTYPE else want["regs"], where)
    for k, x in zip(OUT[2:], got[2:6]):
        assert x.shape == want[k].shape and x.tobytes() == want[k].tobytes(), (where, k)


def tile_golden(g, rows):
    ro, co = g["regs_off_out"], g["cigar_off_out"]
    pick = np.concatenate([np.arange(ro[r], ro[r + 1]) for r in rows]).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
    cigs = [g["cigar_out"][co[i]:co[i + 1]] for i in pick]
    off = lambda lens: np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return dict(regs_off=off([ro[r + 1] - ro[r] for r in rows]), regs=g["regs_out"][pick], extra=g["extra_out"][pick], dp_max2=g["dp_max2_out"][pick],
                cigar_off=off([len(c) for c in cigs]), cigar=np.concatenate(cigs).astype(np.uint32) if cigs else np.zeros(0, np.uint32))


def same_bytes(x, y, where):
    for i, (u, v) in enumerate(zip(x, y)):
        u, v = np.asarray(u), np.asarray(v)
        assert u.shape == v.shape and u.tobytes() == v.tobytes(), (where, i)


# ---- (a) (b) (c)

@pytest.mark.parametrize("name", list(S.SCENES))
def test_a_the_one_call_equals_the_golden(dev, name):
    g = load(name)
    got = one_call(dev, name, want_anchors=True)
    equals_golden(got, g, name)
    assert np.array_equal(got[6], g["rep_len"]) and got[7] == int(g["n_anchors"])
    assert np.array_equal(got[8], g["a_off_out"]) and got[9].tobytes() == g["a_out"].tobytes(), (name, "a[] with its marks")


@pytest.mark.parametrize("name", list(S.SCENES))
def test_b_the_staged_path_equals_the_one_call_byte_for_byte(dev, name):
    A = one_call(dev, name, want_anchors=True)
    (a, *B), rep, n_anchors = staged(dev, name)
    same_bytes(A[:6], B, name)
    assert a.tobytes() == A[9].tobytes() and np.array_equal(rep, A[6]) and n_anchors == A[7]


@pytest.mark.parametrize("name", list(S.SCENES))
def test_c_align_resident_after_map_seqs_equals_the_one_call_and_hands_over_what_the_reference_squeezed(dev, name):
    sc, g = S.scene(name), load(name)
    A = one_call(dev, name, want_anchors=True)
    pre = dev.map_seqs(index_of(dev, name), sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, sc.seq, sc.seq_off, sc.bid, sc.hash_, sc.ref_len)
    C = dev.align_resident(sc.aopt, sc.opt, want_anchors=True)
    same_bytes(A[:6], C[:6], name)
    assert np.array_equal(C[6], A[8]) and C[7].tobytes() == A[9].tobytes()
    roff, regs, aoff = dev.map_align_handoff()
    assert np.array_equal(roff, pre[0]) and np.array_equal(roff, g["sq_regs_off_out"]) and np.array_equal(aoff, g["sq_a_off_out"])
    same_records(regs, g["sq_regs_out"].view(chaindp.REG_DTYPE), name + ": the regions handed over")
    assert np.array_equal(regs["as"], g["sq_regs_out"]["as"])
    # the anchors handed over are the tap's: the alignment only adds marks
    assert (C[7] & ~np.array([0, int(S.SEED_IGNORE)], np.uint64)).tobytes() == (g["sq_a_out"] & ~np.array([0, int(S.SEED_IGNORE)], np.uint64)).tobytes()
    again = dev.align_resident(sc.aopt, sc.opt)                               # chain_post's result is still what it was
    same_bytes(A[:6], again, name + " again")


# ---- (d) the LDS caps

@pytest.mark.parametrize("cap", [1, S.SCENE_CAP])
def test_d_every_scene_under_lowered_lds_caps(dev, cap):
    assert dev.map_align_set_lds_cap(cap) == S.HO_LDS_CAP
    try:
        for name in S.SCENES:
            got = one_call(dev, name, want_anchors=True)
            g = load(name)
            equals_golden(got, g, (name, cap))
            assert got[9].tobytes() == g["a_out"].tobytes()
    finally:
        dev.map_align_set_lds_cap(0)


@pytest.mark.parametrize("cap", [0, 1, S.SCENE_CAP, 64, 65])
def test_d_the_hand_made_lists_on_both_routes(dev, cap):
    """cnt_65 / cnt_257 (anchors across a lane stride and more), regs_64 / regs_65 / regs_129 (ranking in strides), lists on both sides of
    the lowered and the built-in cap, equal `as`: the hand-off alone against mm_squeeze_a."""
    ro, r, bo, b = S.synthetic()
    want = S.squeeze(ro, r, bo, b)
    dev.map_align_set_lds_cap(cap)
    try:
        got = dev.map_align_run_handoff(ro, r, bo, b)
    finally:
        dev.map_align_set_lds_cap(0)
    same_bytes(want, got, cap)


# ---- (e) the scan's tile edges

@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_e_a_scene_tiled_over_the_scans_tile_edges(dev, n):
    sc, g = S.scene("map-ont"), load("map-ont")
    t = S.tiled(sc, n)
    got = one_call(dev, "map-ont", t)
    equals_golden(got, g, n, rows=t.at)


# ---- (f) capacities

def test_f_short_capacities_and_the_fetch(dev):
    name = "no-ljoin"
    ample = one_call(dev, name)
    n, m = len(ample[1]), len(ample[5])
    for caps in (dict(regs_cap=n, cigar_cap=m), dict(regs_cap=n + 7, cigar_cap=m + 9)):
        same_bytes(ample[:6], one_call(dev, name, **caps)[:6], caps)
    for caps in (dict(regs_cap=0, cigar_cap=0), dict(regs_cap=n - 1, cigar_cap=m), dict(regs_cap=n, cigar_cap=m - 1)):
        with pytest.raises(chaindp.ChainDPError) as e:
            one_call(dev, name, **caps)
        assert list(e.value.need) == [n, m] and np.array_equal(e.value.regs_off, ample[0]), caps
        # the result is resident: the fetch delivers it without computing anything again
        off, need = np.zeros(len(ample[0]), np.int64), np.zeros(2, np.int64)
        regs, extra, dp2 = np.zeros(n, chaindp.REG_DTYPE), np.zeros(n, chaindp.ALIGN_EXTRA_DTYPE), np.zeros(n, np.int32)
        coff, cig = np.zeros(n + 1, np.int64), np.zeros(m, np.uint32)
        p = lambda x: x.ctypes.data
        assert dev._lib.chaindp_align_post_fetch(dev._ctx, len(off) - 1, p(off), p(regs), p(extra), p(dp2), n, p(coff), p(cig), m, p(need)) == 0
        same_bytes(ample[:6], (off, regs, extra, dp2, coff, cig), ("fetch", caps))


# ---- (g) two presets on one context

def test_g_batches_of_different_preset_one_after_the_other():
    with chaindp.Device(0, max_anchors=1 << 21, max_reads=1 << 12) as d:
        for name in ("map-pb", "ava-ont", "map-pb", "asm5"):
            equals_golden(one_call(d, name), load(name), name)


# ---- (h) refusals

def test_h_every_refusal_is_err_arg_and_a_valid_call_follows(dev):
    name = "map-ont"
    sc = S.scene(name)
    ix = index_of(dev, name)
    ample = one_call(dev, name)

    def resident(opt=None, n_reads=None, aopt=None):
        """chaindp_align_resident with ample room: its return code."""
        n = len(sc.reads) if n_reads is None else n_reads
        off, need = np.zeros(max(n, 0) + 1, np.int64), np.zeros(2, np.int64)
        regs, extra, dp2 = np.zeros(1024, chaindp.REG_DTYPE), np.zeros(1024, chaindp.ALIGN_EXTRA_DTYPE), np.zeros(1024, np.int32)
        coff, cig = np.zeros(1025, np.int64), np.zeros(1 << 16, np.uint32)
        p = lambda x: x.ctypes.data
        import ctypes as C
        return dev._lib.chaindp_align_resident(dev._ctx, C.byref(aopt or sc.aopt), C.byref(opt or sc.opt), n, p(off), p(regs), p(extra), p(dp2), 1024, p(coff), p(cig),
                                               1 << 16, p(need), None, None)

    def map_seqs(opt=None):
        return dev.map_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, opt or sc.opt, sc.seq, sc.seq_off, sc.bid, sc.hash_, sc.ref_len)

    no_cigar = P.PostOpt(**dict(sc.opt.asdict(), flag=sc.opt.flag & ~P.MM_F_CIGAR))
    dev.align_set_targets(sc.tseq_off, sc.tseq)
    map_seqs()
    assert resident() == 0
    assert resident(opt=no_cigar) == -1                                      # popt->flag lacks MM_F_CIGAR
    assert resident(n_reads=len(sc.reads) - 1) == -1 and resident(n_reads=-1) == -1   # n_reads is not theirs
    assert resident(opt=P.PostOpt(**dict(sc.opt.asdict(), match_sc=0))) == -1            # what the post stage refuses
    assert resident(aopt=P.align_opt("map-ont", bw=-1)) == -1                             # what the alignment stage refuses
    assert resident() == 0                                                   # the batch is still there
    map_seqs(no_cigar)
    assert resident() == -1                                                  # chain_post ran without MM_F_CIGAR
    map_seqs()
    dev.align_clear_targets()
    assert resident() == -1                                                  # no targets
    dev.align_set_targets(sc.tseq_off[:-1], sc.tseq[:sc.tseq_off[-2]])
    assert resident() == -1                                                  # not the n_ref chain_post was given
    short = sc.tseq_off.copy()
    short[-1] -= 1
    dev.align_set_targets(short, sc.tseq[:-1])
    assert resident() == -1                                                  # not the ref_len chain_post was given
    dev.align_set_targets(sc.tseq_off, sc.tseq)
    assert resident() == 0
    # a chaindp_est_err upload replaces the hits
    roff, regs = map_seqs()[:2]
    dev.est_err(roff, regs, np.diff(sc.seq_off).astype(np.int32), sc.ref_len)
    assert resident() == -1
    # a new sketch replaces the bases (and the batch)
    map_seqs()
    dev.sketch(sc.w, sc.k, sc.hpc, sc.seq, sc.seq_off)
    assert resident() == -1
    # minimizers of the caller's own: the resident bases are not this batch's
    mini_off = dev.sketch(sc.w, sc.k, sc.hpc, sc.seq, sc.seq_off)
    mini = dev.download_minimizers()
    dev.map_reads(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, mini_off, mini, sc.bid, np.diff(sc.seq_off).astype(np.int32), sc.hash_, sc.ref_len)
    assert resident() == -1
    # ... while the sketch's own minimizers through map_reads are
    dev.sketch(sc.w, sc.k, sc.hpc, sc.seq, sc.seq_off)
    dev.map_reads(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, None, None, sc.bid, None, sc.hash_, sc.ref_len)
    assert resident() == 0
    # reads of several segments: the one call refuses the parameters at its entry and leaves the resident batch alone ...
    par2 = P.preset("map-ont", n_segs=2)
    with pytest.raises(chaindp.ChainDPError) as e:
        dev.map_align_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, par2, sc.min_cnt, sc.opt, sc.aopt, sc.seq, sc.seq_off, sc.bid, sc.hash_, sc.ref_len)
    assert "chaindp error -1" in str(e.value)
    assert resident() == 0
    same_bytes(ample[:6], one_call(dev, name)[:6], "after the refused n_segs")
    # ... a batch of pairs is refused by chain_post, so none is resident for align_resident ...
    pairs = 8
    ns = np.full(pairs, 2, np.int32)
    pseq, pseq_off = sc.seq[:sc.seq_off[2 * pairs]], sc.seq_off[:2 * pairs + 1]
    plen = (pseq_off[2::2] - pseq_off[:-1:2]).astype(np.int32)
    dev.sketch(sc.w, sc.k, sc.hpc, pseq, pseq_off, n_segs=ns)
    dev.collect_seeds(ix, sc.flag, sc.max_occ, None, None, sc.bid[:pairs], None, n_segs=ns)
    dev.run_full(par2)
    coff = dev.backtrack(par2, sc.min_cnt)[0]
    dev.gen_regs(sc.hash_[:pairs], plen, int(coff[-1]))
    with pytest.raises(chaindp.ChainDPError) as e:
        dev.chain_post(sc.opt, sc.ref_len)
    assert "chaindp error -1" in str(e.value) and "single-segment" in str(e.value)
    assert resident(n_reads=pairs) == -1 and resident() == -1
    same_bytes(ample[:6], one_call(dev, name)[:6], "after the batch of pairs")
    # ... and chaindp_frag_post on a batch takes the buffers chain_post's result lay in
    map_seqs()
    assert resident() == 0
    dev.frag_post(sc.opt, sc.ref_len, np.ones(len(sc.reads), np.int32))
    assert resident() == -1
    same_bytes(ample[:6], one_call(dev, name)[:6], "after frag_post")
    # no batch at all on a fresh context; the one call without targets
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 8) as d:
        with pytest.raises(chaindp.ChainDPError):
            d.align_resident(sc.aopt, sc.opt)
        with pytest.raises(chaindp.ChainDPError):
            d.map_align_seqs(d.load_index(sc.image()), sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, sc.aopt, sc.seq, sc.seq_off, sc.bid,
                             sc.hash_, sc.ref_len)
    same_bytes(ample[:6], one_call(dev, name)[:6], "a valid call on the same context afterwards")


# ---- (i) nothing to do

def test_i_no_reads_and_reads_without_regions(dev):
    sc = S.scene("map-ont")
    none = S.tiled(sc, 0)
    got = one_call(dev, "map-ont", none, want_anchors=True)
    assert list(got[0]) == [0] and len(got[1]) == 0 and len(got[5]) == 0 and list(got[4]) == [0] and got[7] == 0 and list(got[8]) == [0]
    g = load("map-ont")
    bare = [r for r in range(len(sc.reads)) if g["regs_off_out"][r] == g["regs_off_out"][r + 1] and g["sq_regs_off_out"][r] == g["sq_regs_off_out"][r + 1]]
    assert len(bare) >= 20 and any(len(sc.reads[r]) == 0 for r in bare)
    at = np.array(bare)
    t = S.tiled(sc, 0)
    t.at, t.reads, t.bid, t.hash_ = at, [sc.reads[i] for i in at], sc.bid[at], sc.hash_[at]
    import e2e_model as em
    t.seq, t.seq_off = em.batch(t.reads)
    got = one_call(dev, "map-ont", t, want_anchors=True)
    assert not got[0].any() and len(got[0]) == len(bare) + 1 and len(got[1]) == 0 and len(got[5]) == 0 and not got[8].any() and len(got[9]) == 0
