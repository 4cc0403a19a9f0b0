"""GPU tier: every kernel that flushes tiles (the v[] loop with its early exit) on the inputs of test_flush_rounds_model.py -- the five
seeded batches and the hand-built units that need rounds 4 to 6 and the count -- plus the small dense batch: k_chain_twin with one
cost table per wave and with one per half, its hand-over modes (1: every unit to k_chain_units untouched, 2: after its first tile),
and k_chain_dense / dense1 / dense16 behind k_chain_units (all three flush through fast_flush_tile).  f, p and v are
compared element for element with the oracle, new_seed[] byte for byte with the oracle's compaction."""
import numpy as np
import pytest

import flush_model as fm
import oracle_lib as ol
from minimap2_chaindp_amd import anchorgen as ag, chaindp, params as P

pytestmark = pytest.mark.gpu

DENSE = len(fm.SEEDED) + 1


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 23, max_reads=1 << 16) as d:
        d.set_ring(128)
        d.set_variant(0)
        yield d


@pytest.fixture(scope="module")
def inputs():
    """[(name, par, off, a, f, p, v, expected seeds per read)]: 0-4 seeded, 5 built, 6 dense.  Computed once, never written to."""
    batches = [(str(fm.SEEDED[i]),) + fm.seeded(i) for i in range(len(fm.SEEDED))] + [("built",) + fm.built()]
    batches.append(("dense", P.preset("ava-ont")) + ag.generate("dense", n_reads=6, seed=fm.SEED, read_len=3000, n_hits=12))
    out = []
    for name, par, off, a in batches:
        f, p, v, _ = ol.oracle_batch(par, off, a, threads=8)
        seeds = []
        for r in range(len(off) - 1):
            lo, hi = int(off[r]), int(off[r + 1])
            seeds.append(ol.oracle_compact(par, np.ascontiguousarray(a[lo:hi]), f[lo:hi].copy(), p[lo:hi].copy(), v[lo:hi].copy()).tobytes())
        for x in (off, a, f, p, v):
            x.setflags(write=False)
        out.append((name, par, off, a, f, p, v, seeds))
    assert 3_500_000 < sum(int(b[2][-1]) for b in out) < 5_000_000
    return out


def _check(dev, batch, route):
    name, par, off, a, of, op, ov, exp_seeds = batch
    f, p, v = dev.chain_batch(par, off, a)
    soff, seeds = dev.compact(par)
    for what, x, y in (("f", f, of), ("p", p, op), ("v", v, ov)):
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, route, what, "first mismatch at anchor", int(bad[0]), int(x[bad[0]]), int(y[bad[0]]))
    assert int(soff[-1]) == len(seeds)
    for r, exp in enumerate(exp_seeds):
        assert seeds[int(soff[r]):int(soff[r + 1])].tobytes() == exp, (name, route, "new_seed[] of read", r)


@pytest.mark.parametrize("handover", [0, 1, 2])
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
def test_twin_layouts_and_handovers(dev, inputs, two, handover):
    """One-key batches go to the one-table layout unless the hook keeps them on the other; hand-over 1 sends every unit to
    k_chain_units (fast_flush_tile flushes all tiles), 2 after the first tile (both loops in one unit)."""
    dev.set_twin_tables(two)
    dev.set_twin_handover(handover)
    try:
        for i, batch in enumerate(inputs[:DENSE]):
            _check(dev, batch, ("two" if two else "one", handover))
            if i in (0, 1, 2):                                                 # one avg_qspan: one table key
                assert dev.twin_tables() == (2 if two else 1), (batch[0], dev.twin_tables())
    finally:
        dev.set_twin_tables(False)
        dev.set_twin_handover(0)


@pytest.mark.parametrize("deep", [False, True, 2, 3, 4], ids=["k_chain_units_to_the_end", "device_decides", "dense", "dense1", "dense16"])
def test_dense_route(dev, inputs, deep):
    """The dense batch is k_chain_units' (long units): it keeps them to the end, or hands them to k_chain_dense, dense1 or dense16,
    which redo them; with the hook the map-ont batch's units with deep scans take that road too."""
    dev.set_deep_handover(deep)
    try:
        _check(dev, inputs[DENSE], ("deep", deep))
        assert dev.twin_tables() == 0
        if deep is not False:
            assert dev.deep_units() > 0
        _check(dev, inputs[3], ("deep", deep))
    finally:
        dev.set_deep_handover(True)
