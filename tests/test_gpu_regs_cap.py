"""GPU tier: what the calls that return hits do about the room for them, through the public methods only.  For every one of
map_batch, chain_post, map_reads, map_seqs (the map-ont batch of tests/e2e_model.py) and frag_post, map_frags, map_frag_seqs (the
smallest paired batch of tests/frag_model.py with two final hits), with n the hits of a call with ample room:
  regs_cap = n and n + 100        the ample call's bytes
  regs_cap = 1 and n - 1          the same bytes again (map_batch, map_reads, map_seqs fetch what did not fit) or ChainDPError with
                                  CHAINDP_ERR_CAPACITY (-2) (chain_post, frag_post, map_frags, map_frag_seqs)
  regs_cap = None, floor of 1     the ample call's bytes, whatever the guess came to
With the floor at 1 the guess is short of the hits only on the paired batch, for map_frags and map_frag_seqs (22 hits from two
segments of 150 bases: fewer than half as many minimizers, 300 // 16 bases).  The map-ont batch has 1409 hits for 1.46 M minimizers
and 7.9 M bases, and the paired batch 454 anchors (frag_post guesses a quarter of them): for the other five methods the last case
pins only that the result does not depend on the guess."""
import types

import numpy as np
import pytest

import e2e_model as em
import frag_model as fm
from minimap2_chaindp_amd import chaindp

pytestmark = pytest.mark.gpu
AMPLE = 1 << 15
N_FRAGS = 1                       # the fewest fragments whose model has two final hits (asserted below)
RETRIED = ("map_batch", "map_reads", "map_seqs")
RAISES = ("chain_post", "frag_post", "map_frags", "map_frag_seqs")


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 23, max_reads=1 << 14) as d:
        yield d


@pytest.fixture(scope="module")
def single(dev):
    sc, m = em.named("map-ont")
    seq, seq_off = em.batch(sc.reads)
    return types.SimpleNamespace(sc=sc, ix=dev.load_index(sc.image()), seq=seq, seq_off=seq_off, mini_off=m.mini_off, mini=m.mini, qlen=m.qlen)


@pytest.fixture(scope="module")
def paired(dev):
    sc = fm.scenario(n_frags=N_FRAGS)
    seq, seq_off, ns = fm.batch(sc.frags)
    seg_len = np.diff(seq_off).astype(np.int32)
    qlen = np.add.reduceat(seg_len, np.concatenate([[0], np.cumsum(ns)[:-1]])).astype(np.int32)
    mini_off = dev.sketch(sc.w, sc.k, sc.hpc, seq, seq_off, n_segs=ns)
    return types.SimpleNamespace(sc=sc, ix=dev.load_index(sc.image()), seq=seq, seq_off=seq_off, ns=ns, seg_len=seg_len, qlen=qlen, mini_off=mini_off,
                                 mini=dev.download_minimizers())


def test_the_paired_batch_is_the_smallest_with_two_final_hits():
    assert N_FRAGS == 1 and int(fm.model_of(fm.scenario(n_frags=N_FRAGS)).seg_regs_off[-1]) >= 2        # no fragment, no hit


def call(dev, S, P, name, cap):
    """The method `name` on its batch with regs_cap = cap; the post steps after a map_batch with ample room."""
    B = P if name in ("frag_post", "map_frags", "map_frag_seqs") else S
    sc = B.sc
    head = (B.ix, sc.flag, sc.max_occ, sc.par, sc.min_cnt)
    if name in ("map_batch", "chain_post", "frag_post"):
        hits = dev.map_batch(*head, B.mini_off, B.mini, sc.bid, B.qlen, sc.hash_, regs_cap=cap if name == "map_batch" else AMPLE)
        if name == "map_batch":
            return hits
        assert int(hits[0][-1]) < AMPLE
        if name == "chain_post":
            return dev.chain_post(sc.opt, sc.ref_len, regs_cap=cap)
        return dev.frag_post(sc.opt, sc.ref_len, B.ns, seg_len=B.seg_len, regs_cap=cap)
    if name == "map_reads":
        return dev.map_reads(*head, sc.opt, B.mini_off, B.mini, sc.bid, B.qlen, sc.hash_, sc.ref_len, regs_cap=cap)
    if name == "map_seqs":
        return dev.map_seqs(B.ix, sc.w, sc.k, sc.hpc, *head[1:], sc.opt, B.seq, B.seq_off, sc.bid, sc.hash_, sc.ref_len, regs_cap=cap)
    if name == "map_frags":
        return dev.map_frags(*head, sc.opt, B.mini_off, B.mini, sc.bid, B.qlen, sc.hash_, B.ns, B.seg_len, sc.ref_len, regs_cap=cap)
    return dev.map_frag_seqs(B.ix, sc.w, sc.k, sc.hpc, *head[1:], sc.opt, B.seq, B.seq_off, B.ns, sc.bid, sc.hash_, sc.ref_len, pe_ori=1, regs_cap=cap)


def same(got, exp):
    return len(got) == len(exp) and all(x == y if isinstance(y, int) else (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())
                                        for x, y in zip(got, exp))


@pytest.mark.parametrize("name", RETRIED + RAISES)
def test_regs_cap(dev, single, paired, monkeypatch, name):
    ample = call(dev, single, paired, name, AMPLE)
    n = int(ample[0][-1])
    print(f"\n[regs_cap] {name}: {n} hits, {len(ample[0]) - 1} offsets")
    assert 2 <= n < AMPLE and len(ample[1]) == n
    for cap in (n, n + 100):
        assert same(call(dev, single, paired, name, cap), ample), cap
    for cap in (1, n - 1):
        if name in RETRIED:
            assert same(call(dev, single, paired, name, cap), ample), cap
        else:
            with pytest.raises(chaindp.ChainDPError, match="chaindp error -2"):
                call(dev, single, paired, name, cap)
    monkeypatch.setattr(chaindp, "REGS_CAP_FLOOR", 1)
    assert same(call(dev, single, paired, name, None), ample)
