"""GPU tier: k_chain_twin's two LDS layouts -- one cost table per wave (batches whose units share one table key) and one per half
(mixed keys, or kept there by the test hook) -- against the golden vectors and the oracle, element for element, through every
hand-over mode of the kernel.  Each case also checks which layout took the batch.  (The per-anchor flags the DP kernels write are
what the compaction reads: new_seed[] checks them.)"""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import golden_names, load_golden, params_from
from minimap2_chaindp_amd import anchorgen as ag, chaindp, params as P

pytestmark = pytest.mark.gpu

ONE, TWO = 1, 2          # Device.twin_tables(): the layout that ran the last batch (0: k_chain_twin declined it as a whole)
NONE = 0

# the layout that takes each fixture when the device decides: ONE where every unit the kernel may take has the same table key, TWO
# where the keys differ or no unit qualifies (segment ids, n_segs > 1), NONE where the batch is one of long units (map-ont shape,
# dense repeats, cDNA / splice: k_chain_units takes it whole)
GOLDEN_LAYOUT = {
    "edge_cases_mapont": ONE, "edge_cases_minsc0": ONE, "inv_mapont": ONE, "mt_orang_human_avaont_params": ONE,
    "mt_orang_human_mapont": ONE, "q2_t2_mapont": NONE, "syn_ava_ont": ONE, "syn_dense_ava": NONE, "syn_map_ont": NONE,
    "syn_paired_cdna_nsegs2": NONE, "syn_paired_nsegs2_mapont": TWO, "syn_paired_sr": TWO, "syn_ties_mapont": NONE,
    "syn_ties_skip0": NONE, "syn_ties_skip3_bw40": NONE, "syn_ties_splice": NONE, "syn_ties_tinygap": TWO,
}


def _expected(layout, two):
    return TWO if two and layout != NONE else layout


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 23, max_reads=1 << 16) as d:
        d.set_ring(128)
        d.set_variant(0)
        yield d


def _run(dev, par, off, a, two, handover, n_segs=None):
    dev.set_twin_tables(two)
    dev.set_twin_handover(handover)
    try:
        f, p, v = dev.chain_batch(par, off, a, n_segs=n_segs)
        took = dev.twin_tables()
        soff, seeds = dev.compact(par)
    finally:
        dev.set_twin_tables(False)
        dev.set_twin_handover(0)
    return f, p, v, soff, seeds, took


@pytest.mark.parametrize("handover", [0, 1, 2])
@pytest.mark.parametrize("two", [False, True], ids=["device_decides", "two_tables"])
@pytest.mark.parametrize("name", golden_names())
def test_golden_fixtures_on_both_layouts(dev, name, two, handover):
    g = load_golden(name)
    par = params_from(g["params"])
    f, p, v, soff, seeds, took = _run(dev, par, g["off"], g["anchors"], two, handover)
    assert took == _expected(GOLDEN_LAYOUT[name], two), (name, took)
    assert np.array_equal(f, g["f"]), (name, "f")
    assert np.array_equal(p, g["p"]), (name, "p")
    assert np.array_equal(v, g["v"]), (name, "v")
    assert np.array_equal(soff, g["seeds_off"]), (name, "new_i")
    assert seeds.tobytes() == g["seeds"].tobytes(), (name, "new_seed[] bytes")


CASES = [  # generator, generator overrides, DP preset, DP overrides, reads, per-read n_segs?, layout when the device decides
    ("ava-ont", {}, "ava-ont", {}, 300, False, ONE),                         # one q_span: one avg_qspan
    ("ava-ont", dict(span_jitter=4), "ava-ont", {}, 200, False, TWO),          # reads of different avg_qspan
    ("ava-ont", dict(noise_pct=40, tie_pct=20), "ava-ont", {}, 120, False, ONE),
    ("ava-ont", dict(q_span=255, span_jitter=0), "ava-ont", {}, 40, False, TWO),   # costs do not fit int8: no unit qualifies
    ("skew", dict(skew_max=30000), "ava-ont", {}, 100, False, ONE),
    ("map-ont", {}, "map-ont", {}, 200, False, NONE),                        # long units
    ("ties", {}, "map-ont", {}, 200, False, TWO),                            # span jitter
    ("ties", {}, "ava-pb", {}, 100, False, TWO),
    ("paired", {}, "sr", {}, 2000, False, TWO),                              # n_segs = 2: no unit qualifies
    ("paired", {}, "map-ont", dict(n_segs=2), 500, True, TWO),
    ("dense", dict(read_len=3000, n_hits=12), "ava-ont", {}, 6, False, NONE),
    ("ties", {}, "map-ont", dict(max_skip=0), 50, False, TWO),
    ("ties", {}, "map-ont", dict(max_skip=2, bw=30), 50, False, TWO),
    ("ava-ont", {}, "ava-ont", dict(max_dist_y=2000), 100, False, ONE),     # max_dist_y < max_dist_x: the other instantiation
]


@pytest.mark.parametrize("handover", [0, 1, 2])
@pytest.mark.parametrize("two", [False, True], ids=["device_decides", "two_tables"])
@pytest.mark.parametrize("gen,gen_over,preset,par_over,n_reads,per_read,layout", CASES)
def test_seeded_batches_on_both_layouts(dev, gen, gen_over, preset, par_over, n_reads, per_read, layout, two, handover):
    par = P.preset(preset, **par_over)
    off, a = ag.generate(gen, n_reads=n_reads, seed=4321, **gen_over)
    n_segs = (np.arange(n_reads) % 2 + 1).astype(np.int32) if per_read else None
    f, p, v, soff, seeds, took = _run(dev, par, off, a, two, handover, n_segs=n_segs)
    assert took == _expected(layout, two), (gen, gen_over, par_over, took)
    of, op, ov, _ = ol.oracle_batch(par, off, a, n_segs=n_segs, threads=8)
    for name, x, y in (("f", f, of), ("p", p, op), ("v", v, ov)):
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (gen, two, handover, name, "first mismatch at anchor", int(bad[0]), int(x[bad[0]]), int(y[bad[0]]))
    assert int(soff[-1]) == len(seeds)
    for r in range(n_reads):
        lo, hi = int(off[r]), int(off[r + 1])
        rp = P.preset(preset, **par_over)
        if n_segs is not None:
            rp.n_segs = int(n_segs[r])
        exp = ol.oracle_compact(rp, np.ascontiguousarray(a[lo:hi]), of[lo:hi].copy(), op[lo:hi].copy(), ov[lo:hi].copy())
        assert seeds[int(soff[r]):int(soff[r + 1])].tobytes() == exp.tobytes(), (gen, two, handover, r)


def test_one_key_batch_takes_one_table_and_both_layouts_agree(dev):
    """The flagship shape (one q_span, so one avg_qspan) goes to the one-table layout; kept on the two-table layout by the hook it
    gives the same bytes."""
    par = P.preset("ava-ont")
    off, a = ag.generate("ava-ont", n_reads=400, seed=11)
    r1 = _run(dev, par, off, a, False, 0)
    r2 = _run(dev, par, off, a, True, 0)
    assert r1[-1] == ONE and r2[-1] == TWO
    for x, y in zip(r1[:-1], r2[:-1]):
        assert x.tobytes() == y.tobytes()


def test_mixed_keys_take_two_tables(dev):
    """Reads with different avg_qspan (span jitter) need a table per half: the one-table layout must leave such a batch alone."""
    par = P.preset("ava-ont")
    off, a = ag.generate("ava-ont", n_reads=150, seed=12, span_jitter=6)
    f, p, v, _, _, took = _run(dev, par, off, a, False, 0)
    assert took == TWO
    of, op, ov, _ = ol.oracle_batch(par, off, a, threads=8)
    assert np.array_equal(f, of) and np.array_equal(p, op) and np.array_equal(v, ov)
