"""GPU tier: the device memory of a context reaches a steady state.  Every device buffer of a context is an entry of one pool
(csrc/chaindp_devmem.h) and Device.device_bytes() is the sum of its live entries, so these are equalities of the pool's own accounting,
nothing measured: (a) map_seqs on the same batch again and again owns the same bytes after the second call as after the twelfth (a
chaindp_sketch used to make the next compaction allocate its scratch anew, over the live pointers); (b) the same for the staged calls;
(c) a larger and a smaller batch in turn: the bytes never go down and stay put after the first large batch (the buffers only grow);
(d) two fresh contexts of the same capacities own the same bytes, and a context that has been through map_seqs and the fragment path
closes without error."""
import numpy as np
import pytest

import e2e_model as em
import frag_model as fm
from minimap2_chaindp_amd import chaindp
from test_gpu_e2e import map_seqs, staged
from test_gpu_post import same_records

pytestmark = pytest.mark.gpu
MAX_ANCHORS, MAX_READS = 1 << 20, 1 << 10


@pytest.fixture(scope="module")
def batch():
    sc = em.scenario("map-ont", n_reads=64, max_len=3000)
    return sc, em.model_of(sc)


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as d:
        yield d


def same_result(got, exp, where):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[2]) and got[3] == exp[3], where
    same_records(got[1], exp[1], where)


def test_repeated_map_seqs_owns_the_same_bytes(dev, batch):
    sc, _ = batch
    ix = dev.load_index(sc.image())
    results, owned = [], []
    for _ in range(12):
        results.append(map_seqs(dev, ix, sc))
        owned.append(dev.device_bytes())
    print(f"\n[ctx memory] map_seqs x 12: {owned}")
    assert len(results[0][1]) > 0 and owned[0] > 0
    assert owned[1] == owned[11], owned
    same_result(results[11], results[0], "twelfth map_seqs against the first")


def test_repeated_staged_calls_own_the_same_bytes(dev, batch):
    sc, m = batch
    ix = dev.load_index(sc.image())
    results, owned = [], []
    for _ in range(6):
        first, res = staged(dev, ix, sc, m)
        assert first is None, first
        results.append(res)
        owned.append(dev.device_bytes())
    print(f"\n[ctx memory] staged calls x 6: {owned}")
    assert owned[1] == owned[5], owned
    same_result(results[5], results[1], "sixth round of staged calls against the second")


def test_batches_of_two_sizes_never_shrink_and_settle(batch):
    sc, _ = batch
    with chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as d:
        ix = d.load_index(sc.image())
        owned = [d.device_bytes()]
        for _ in range(6):
            for sel in (range(64), range(8)):
                got = map_seqs(d, ix, sc, list(sel))
                assert len(got[0]) == len(sel) + 1
                owned.append(d.device_bytes())
        print(f"\n[ctx memory] 64 and 8 reads in turn: {owned}")
        assert all(b >= a for a, b in zip(owned, owned[1:])), owned
        assert owned[1] > owned[0] and all(b == owned[1] for b in owned[1:]), owned


def test_context_lifetime(batch):
    sc, _ = batch
    with chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as a, chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS) as b:
        fresh = a.device_bytes()
        assert fresh > 0 and fresh == b.device_bytes()
    d = chaindp.Device(0, max_anchors=MAX_ANCHORS, max_reads=MAX_READS)
    try:
        assert d.device_bytes() == fresh
        got = map_seqs(d, d.load_index(sc.image()), sc)
        assert len(got[1]) > 0
        fs = fm.scenario(n_frags=400, seed=3)
        pairs = [i for i, f in enumerate(fs.frags) if len(f) == 2][:32]
        seq, seq_off, ns = fm.batch([fs.frags[i] for i in pairs])
        soff, regs, _, na = d.map_frag_seqs(d.load_index(fs.image()), fs.w, fs.k, fs.hpc, fs.flag, fs.max_occ, fs.par, fs.min_cnt, fs.opt, seq, seq_off, ns,
                                            fs.bid[pairs], fs.hash_[pairs], fs.ref_len)
        assert len(ns) == 32 and (ns == 2).all() and len(soff) == 65 and na > 0 and len(regs) > 0
        assert d.device_bytes() > fresh
    finally:
        d.close()                                                    # (chaindp_destroy returns nothing: what this shows is one release_all without a crash)
    assert d._ctx is None
