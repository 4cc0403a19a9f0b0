"""GPU tier, end to end: chaindp_map_seqs (bases in, final hits out, every stage resident) against the composed CPU restatements
(tests/e2e_model.py, pinned to the reference by tests/test_e2e_model.py) on seeded batches of thousands of reads of every kind --
empty, shorter than k, N only, unrelated, chimeric, inverted, inside a tandem repeat, with hundreds of chains -- in the four presets.
Every read of every batch is compared: regs_off, rep_len and n_anchors equal, the records by same_records (every byte; div within
DIV_RTOL of test_gpu_post.py).  (a) map_seqs equals the model; (b) the stages called one by one equal map_seqs and the model, and
on a mismatch anywhere the same helper names the first stage, read and element that differ; (c) map_reads on the model's minimizers
equals map_seqs; (d) batches of different shape one after the other on one context; (e) the regs_cap retry; (f) partition and order
invariance on a batch of more than 2 M anchors; (g) the DP kernels each batch took are printed.

Tried against deliberately wrong builds of the library: mini_pos offsets shifted by one read where chaindp_chain_post hands them to
launch_est_err fail twelve tests here (the stages name chain_post); chaindp_gen_regs keeping the lengths of the context's first batch
in d_rqlen fails ten (the stages name gen_regs); k_chain_twin's take_tile without its first_child store fails
test_staged_calls_on_one_context_batch_after_batch at "compact new_seed[]" on the second batch -- the staged calls stop there, which is
why that build was run on that test alone: a wrong p in new_seed[] is an index that the backtrack would follow."""
import time

import numpy as np
import pytest

import e2e_model as em
import oracle_lib as ol
from minimap2_chaindp_amd import chaindp
from test_gpu_post import DIV_RTOL, same_records

pytestmark = pytest.mark.gpu
MAX_ANCHORS, MAX_READS = 1 << 23, 1 << 14


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as d:
        yield d


_loaded = {}


def index_of(dev, name):
    """The scenario's index image on the device, loaded once per context."""
    if (id(dev), name) not in _loaded:
        _loaded[id(dev), name] = dev.load_index(em.named(name)[0].image())
    return _loaded[id(dev), name]


def _ids(sc, sel):
    return np.arange(len(sc.reads)) if sel is None else np.asarray(sel, np.int64).reshape(-1)


def _sel(sc, sel):
    sel = _ids(sc, sel)
    return [sc.reads[i] for i in sel], sc.bid[sel], sc.hash_[sel]


def map_seqs(dev, ix, sc, sel=None, regs_cap=None):
    reads, bid, hash_ = _sel(sc, sel)
    seq, seq_off = em.batch(reads)
    return dev.map_seqs(ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, seq, seq_off, bid, hash_, sc.ref_len, regs_cap=regs_cap)


def map_reads(dev, ix, sc, m, sel=None):
    """map_reads fed the model's minimizers and lengths."""
    _, bid, hash_ = _sel(sc, sel)
    sel = _ids(sc, sel)
    mini = [m.mini[m.mini_off[i]:m.mini_off[i + 1]] for i in sel]
    mini_off = np.concatenate(([0], np.cumsum([len(x) for x in mini]))).astype(np.int64)
    mini = np.concatenate(mini) if len(mini) and mini_off[-1] else np.zeros((0, 2), np.uint64)
    return dev.map_reads(ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt, sc.opt, mini_off, mini, bid, m.qlen[sel], hash_, sc.ref_len)


def subset(m, sel):
    """The model's result for the reads `sel`, in that order (reads are mapped independently of their batch)."""
    sel = np.asarray(sel, np.int64).reshape(-1)
    regs = [m.regs[m.regs_off[i]:m.regs_off[i + 1]] for i in sel]
    roff = np.concatenate(([0], np.cumsum([len(x) for x in regs]))).astype(np.int64)
    regs = np.concatenate(regs) if len(regs) and roff[-1] else np.zeros(0, ol.REG_DTYPE)
    return roff, regs, m.rep_len[sel], int(np.diff(m.a_off)[sel].sum())


def routes(dev, what):
    print(f"\n[routes] {what}: twin_tables {dev.twin_tables()}, leftover_units {dev.leftover_units()}, deep_units {dev.deep_units()}")


# ---- (b) the stages one by one

def _first(stage, got_off, got, exp_off, exp):
    """None, or where `got` first differs from `exp` (arrays with one row per element, read r owning off[r]:off[r + 1])."""
    got_off, exp_off = np.asarray(got_off, np.int64), np.asarray(exp_off, np.int64)
    if len(got_off) != len(exp_off):
        return f"{stage}: {len(got_off) - 1} reads, the model has {len(exp_off) - 1}"
    bad = np.nonzero(got_off != exp_off)[0]
    if len(bad):
        r = int(bad[0]) - 1
        return f"{stage}: read {r} has {int(got_off[r + 1] - got_off[r])} elements, the model has {int(exp_off[r + 1] - exp_off[r])}"
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), -1) if len(got) else np.zeros((0, 1), np.uint8)
    e = np.ascontiguousarray(exp).view(np.uint8).reshape(len(exp), -1) if len(exp) else np.zeros((0, 1), np.uint8)
    if len(g) != len(e):
        return f"{stage}: {len(g)} elements, the model has {len(e)}"
    rows = np.nonzero((g != e).any(1))[0] if len(g) else []
    if len(rows):
        i = int(rows[0])
        r = int(np.searchsorted(exp_off, i, side="right")) - 1
        return f"{stage}: read {r}, element {i - int(exp_off[r])}: device {got[i]!r}, model {exp[i]!r}"
    return None


def staged(dev, ix, sc, m, sel=None):
    """sketch + download_minimizers, collect_seeds, run + download, compact, backtrack, gen_regs, chain_post on this context, each
    compared with the model's intermediates.  Returns (first difference or None, the final result or None): the calls stop at the
    first stage that differs, whose output the later ones would only carry along."""
    reads, bid, hash_ = _sel(sc, sel)
    if sel is not None:
        m = em.model_of(sc, sel=sel)
    seq, seq_off = em.batch(reads)
    off = dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off)
    d = _first("sketch", off, dev.download_minimizers(), m.mini_off, m.mini)
    if d:
        return d, None
    a_off, a, rep, mpo, mp = dev.collect_seeds(ix, sc.flag, sc.max_occ, None, None, bid, None)
    d = (_first("collect_seeds anchors", a_off, a, m.a_off, m.anchors) or _first("collect_seeds mini_pos", mpo, mp, m.mp_off, m.mini_pos)
         or _first("collect_seeds rep_len", np.arange(len(rep) + 1), rep, np.arange(len(m.rep_len) + 1), m.rep_len))
    if d:
        return d, None
    dev.run(sc.par)
    f, p, v = dev.download()
    d = _first("chain DP f", a_off, f, m.a_off, m.f) or _first("chain DP p", a_off, p, m.a_off, m.p) or _first("chain DP v", a_off, v, m.a_off, m.v)
    if d:
        return d, None
    soff, seeds = dev.compact(sc.par)
    d = _first("compact new_seed[]", soff, seeds, m.seeds_off, m.seeds)
    if d:
        return d, None
    coff, u, boff, b = dev.backtrack(sc.par, sc.min_cnt)
    d = _first("backtrack u", coff, u, m.chains_off, m.u) or _first("backtrack b", boff, b, m.b_off, m.b)
    if d:
        return d, None
    regs_in = dev.gen_regs(hash_, m.qlen, int(coff[-1]))
    d = _first("gen_regs", coff, regs_in, m.chains_off, m.regs_in)
    if d:
        return d, None
    roff, regs = dev.chain_post(sc.opt, sc.ref_len)                       # qlen, rep_len and mini_pos: the resident ones
    g0, e0 = regs.copy(), m.regs.copy()
    close = len(g0) == len(e0) and np.allclose(g0["div"], e0["div"], rtol=DIV_RTOL, atol=0)
    if close:
        g0["div"] = e0["div"]                                               # (div has its tolerance: same_records is the judge of it)
    d = _first("chain_post", roff, g0, m.regs_off, e0)
    return d, (roff, regs, rep, int(a_off[-1]))


def check(dev, ix, sc, m, got, where, sel=None):
    """got (a map_seqs / map_reads result) equals the model for every read; if not, the stages say where it first goes wrong."""
    exp = m.result if sel is None else subset(m, sel)
    try:
        assert np.array_equal(got[0], exp[0]), (where, "regs_off")
        assert np.array_equal(got[2], exp[2]), (where, "rep_len")
        assert got[3] == exp[3], (where, "n_anchors", got[3], exp[3])
        same_records(got[1], exp[1], where)
    except AssertionError as e:
        first, _ = staged(dev, ix, sc, m, sel)
        raise AssertionError(f"{where}: map_seqs differs from the model ({e}); stage by stage: {first or 'every stage equals the model'}") from e


# ---- (a) map_seqs equals the model, (c) map_reads equals map_seqs, (g) routes

@pytest.mark.parametrize("name", ["map-ont", "map-pb", "ava-ont", "ava-pb", "family"])
def test_map_seqs_equals_the_model(dev, name):
    sc, m = em.named(name)
    ix = index_of(dev, name)
    t0 = time.time()
    got = map_seqs(dev, ix, sc)
    dt = time.time() - t0
    routes(dev, name)
    print(f"[{name}] {len(sc.reads)} reads, {int(m.qlen.sum())} bases, {len(m.mini)} minimizers, {got[3]} anchors, {int(m.chains_off[-1])} chains, "
          f"{len(got[1])} final hits; map_seqs {dt * 1e3:.0f} ms with transfers")
    assert len(sc.reads) >= (300 if name == "family" else 2000)
    if name == "family":
        assert np.diff(m.chains_off).max() > 256 and sc.max_occ >= 2000
    check(dev, ix, sc, m, got, name)
    again = map_reads(dev, ix, sc, m)
    check(dev, ix, sc, m, again, name + " map_reads")
    assert np.array_equal(again[0], got[0]) and again[1].tobytes() == got[1].tobytes() and np.array_equal(again[2], got[2]) and again[3] == got[3]


@pytest.mark.parametrize("name", ["map-pb", "ava-ont"])
def test_staged_calls_equal_map_seqs_and_the_model(dev, name):
    sc, m = em.named(name)
    ix = index_of(dev, name)
    whole = map_seqs(dev, ix, sc)
    first, res = staged(dev, ix, sc, m)
    assert first is None, first
    check(dev, ix, sc, m, res, name + " staged")
    assert np.array_equal(res[0], whole[0]) and res[1].tobytes() == whole[1].tobytes() and np.array_equal(res[2], whole[2]) and res[3] == whole[3]


def test_staged_calls_on_one_context_batch_after_batch():
    """The separate calls keep the same state between stages and between batches as map_seqs does: three batches of different shape
    and preset, one after the other on a context of their own, every stage of each equal to the model."""
    with chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as d:
        for name in ("ava-pb", "map-ont", "map-pb"):
            sc, m = em.named(name)
            first, res = staged(d, d.load_index(sc.image()), sc, m)
            assert first is None, (name, first)
            same_records(res[1], m.regs, name)


def test_the_stage_helper_names_a_difference():
    """_first on arrays that differ in one place: the report names the stage, the read and the element."""
    off = np.array([0, 2, 2, 5], np.int64)
    a = np.arange(10, dtype=np.uint64).reshape(5, 2)
    b = a.copy(); b[3, 1] = 99
    assert _first("x", off, a, off, a) is None
    assert _first("stage", off, a, off, b).startswith("stage: read 2, element 1:")
    assert _first("stage", np.array([0, 2, 3, 5]), a, off, a).startswith("stage: read 1 has 1 elements, the model has 0")


# ---- (d) one context, many batches

@pytest.mark.parametrize("interleave", [False, True], ids=["map_seqs", "map_reads_interleaved"])
def test_one_context_many_batches(interleave):
    big, mb = em.named("map-ont")
    ava, ma = em.named("ava-pb")
    has_hit = np.nonzero(np.diff(mb.regs_off) > 0)[0]
    no_chain = [int(i) for i in np.nonzero(np.diff(mb.chains_off) == 0)[0]]
    assert len(no_chain) > 100 and (np.diff(mb.a_off)[no_chain] > 0).any() and (np.diff(mb.mini_off)[no_chain] == 0).any()
    with chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as d:
        ixb = d.load_index(big.image())
        steps = [("large", big, mb, ixb, None), ("one read", big, mb, ixb, [int(has_hit[len(has_hit) // 2])]), ("no reads", big, mb, ixb, []),
                 ("no chains", big, mb, ixb, no_chain), ("ava-pb", ava, ma, None, None), ("large again", big, mb, ixb, None)]
        results = {}
        for what, sc, m, ix, sel in steps:
            if ix is None:
                ix = d.load_index(sc.image())                               # the second index, beside the first
            got = map_seqs(d, ix, sc, sel)
            routes(d, what)
            check(d, ix, sc, m, got, what, sel)
            results[what] = got
            if interleave:
                other = map_reads(d, ix, sc, m, sel)
                check(d, ix, sc, m, other, what + " map_reads", sel)
                assert other[1].tobytes() == got[1].tobytes(), what
        first, last = results["large"], results["large again"]
        assert np.array_equal(first[0], last[0]) and first[1].tobytes() == last[1].tobytes(), "byte for byte, div included"
        assert np.array_equal(first[2], last[2]) and first[3] == last[3]
        assert len(results["no chains"][1]) == 0 and len(results["one read"][1]) > 0 and list(results["no reads"][0]) == [0]


# ---- (e) the regs_cap retry

def test_regs_cap_retry_gives_the_same_records(dev):
    sc, m = em.named("map-ont")
    ix = index_of(dev, "map-ont")
    n = int(m.regs_off[-1])
    ample = map_seqs(dev, ix, sc, regs_cap=n + 100)
    check(dev, ix, sc, m, ample, "ample regs_cap")
    for cap in (1, n - 1):
        got = map_seqs(dev, ix, sc, regs_cap=cap)
        assert np.array_equal(got[0], ample[0]) and got[1].tobytes() == ample[1].tobytes(), cap
        assert np.array_equal(got[2], ample[2]) and got[3] == ample[3]
    exact = map_seqs(dev, ix, sc, regs_cap=n)
    assert exact[1].tobytes() == ample[1].tobytes()


# ---- (f) partition and order invariance at size

def test_partition_and_order_invariance_at_size(dev):
    sc, m = em.named("large")
    ix = index_of(dev, "large")
    R = len(sc.reads)
    whole = map_seqs(dev, ix, sc)
    routes(dev, "large batch")
    print(f"[large] {R} reads, {int(m.qlen.sum())} bases, {len(m.mini)} minimizers, {whole[3]} anchors, {int(m.chains_off[-1])} chains, {len(whole[1])} final hits")
    assert R >= 5000 and whole[3] >= 2_000_000
    check(dev, ix, sc, m, whole, "large batch")

    def per_read(res, r):
        return res[1][res[0][r]:res[0][r + 1]].tobytes(), int(res[2][r])

    at = 0
    for part in ([0], list(range(1, 8)), list(range(8, R))):
        got = map_seqs(dev, ix, sc, part)
        assert got[3] == int(np.diff(m.a_off)[part].sum())
        for j, r in enumerate(part):
            assert per_read(got, j) == per_read(whole, r), ("part", len(part), "read", r)
        at += len(part)
    assert at == R
    perm = [int(i) for i in np.random.default_rng(20260117).permutation(R)]
    got = map_seqs(dev, ix, sc, perm)
    assert got[3] == whole[3]
    for j, r in enumerate(perm):
        assert per_read(got, j) == per_read(whole, r), ("permuted", "read", r)
