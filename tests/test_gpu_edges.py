"""GPU tier: the inputs of tests/edge_shapes.py, each exactly on a constant that routes a read or a unit to one kernel or
another (tests/test_edge_shapes_cpu.py proves that they sit there).  Bit for bit, as the rest of the tier: f, p, v element for
element with the oracle, new_seed[] of every read byte for byte with oracle_compact, and for the backtracker cases coff, u,
boff, b with oracle_bottom (and the reference's mm_chain_dp_bottom where it is built).  What the hooks tell about the route
taken (leftover_units, deep_units, twin_tables, stats) is asserted beside the parity."""
import functools

import numpy as np
import pytest

import edge_shapes as es
import oracle_lib as ol
from minimap2_chaindp_amd import chaindp
from test_edge_shapes_cpu import oracle_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 15) as d:
        yield d


def reset(dev):
    dev.set_ring(128)
    dev.set_variant(0)
    dev.set_twin_handover(0)
    dev.set_twin_tables(False)
    dev.set_deep_handover(True)


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(batch, props, oracle results) of a constructor of edge_shapes that makes one batch, built once for the module."""
    made = getattr(es, name)(*args)
    return made + (oracle_results(*made[0]),)


@functools.lru_cache(maxsize=None)
def cases(name):
    """{key: (batch, props, oracle results)} of a constructor that makes several batches."""
    return {k: m + (oracle_results(*m[0]),) for k, m in getattr(es, name)().items()}


def observed(edge, **values):
    """The route the hooks report, printed before it is asserted (pytest -s shows it)."""
    print("edge:", edge, " ".join(f"{k}={v}" for k, v in values.items()))


def read_of(off, i):
    return int(np.searchsorted(off, i, side="right") - 1)


def check_fpv(edge, off, got, exp):
    for name, x in zip("fpv", got):
        bad = np.flatnonzero(x != exp[name])
        assert bad.size == 0, (edge, name, "read", read_of(off, bad[0]), "anchor", int(bad[0]), "got", int(x[bad[0]]), "expected", int(exp[name][bad[0]]))


def check_seeds(edge, dev, par, exp):
    soff, seeds = dev.compact(par)
    assert np.array_equal(soff, exp["soff"]), (edge, "soff", "read", int(np.flatnonzero(soff != exp["soff"])[0]) - 1)
    want = np.concatenate(exp["seeds"]) if len(exp["seeds"]) else seeds[:0]
    if seeds.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(seeds != want)[0])
        raise AssertionError((edge, "new_seed[]", "read", read_of(soff, bad), "record", bad - int(soff[read_of(soff, bad)]), seeds[bad], want[bad]))
    return soff, seeds


def check_chains(edge, dev, par, min_cnt, exp, bottoms=None):
    """coff, u, boff, b whole (the offsets of reads without chains included)."""
    u_exp, b_exp = (exp["u"], exp["b"]) if bottoms is None else bottoms
    coff, u, boff, b = dev.backtrack(par, min_cnt)
    want = dict(coff=np.concatenate(([0], np.cumsum([len(x) for x in u_exp]))), boff=np.concatenate(([0], np.cumsum([len(x) for x in b_exp]))),
                u=np.concatenate(u_exp + [np.zeros(0, np.uint64)]), b=np.concatenate(b_exp + [np.zeros((0, 2), np.uint64)]))
    for name, x in (("coff", coff), ("boff", boff)):
        assert np.array_equal(x, want[name]), (edge, name, "read", int(np.flatnonzero(x != want[name])[0]) - 1)
    bad = np.flatnonzero(u != want["u"])
    assert bad.size == 0, (edge, "u", "read", read_of(coff, bad[0]), "chain", int(bad[0]) - int(coff[read_of(coff, bad[0])]), hex(int(u[bad[0]])), hex(int(want["u"][bad[0]])))
    bad = np.flatnonzero((b != want["b"]).any(1))
    assert bad.size == 0, (edge, "b", "read", read_of(boff, bad[0]), "anchor", int(bad[0]) - int(boff[read_of(boff, bad[0])]))
    if ol.have_ref():
        for r, s in enumerate(exp["seeds"]):
            ru, rb = ol.ref_bottom(min_cnt, par.min_sc, 1, s)
            assert np.array_equal(u[int(coff[r]):int(coff[r + 1])], ru) and np.array_equal(b[int(boff[r]):int(boff[r + 1])], rb.reshape(-1, 2)), (edge, "reference", r)
    return coff, u, boff, b


def run(edge, dev, par, off, a, exp, seeds=True):
    got = dev.chain_batch(par, off, a)
    check_fpv(edge, off, got, exp)
    if seeds:
        check_seeds(edge, dev, par, exp)


def bottoms_for(exp, par, min_cnt):
    out = [ol.oracle_bottom(min_cnt, par.min_sc, s) for s in exp["seeds"]]
    return [u for u, _ in out], [b.reshape(-1, 2) for _, b in out]


# ---------------------------------------------------------------- backtracker

@functools.lru_cache(maxsize=None)
def bt_singles():
    return [m + (oracle_results(*m[0]),) for m in es.bt_single_reads()]


@pytest.mark.parametrize("i", range(len(es.BT_EDGES)), ids=["rec%d_ends%d_kept%d" % e for e in es.BT_EDGES])
def test_backtracker_edge_read_alone(dev, i):
    """A read with exactly BT_LDS_RECS / + 1 / BT_LDS_RECS_MAX / + 1 records, 64 / 65 kept chains (insertion order against the
    reference's radix sort, several chains sharing their first x) and 256 / 257 / 1024 / 1025 chain ends (k_bt_rank's rounds
    and tiles), with a chain that stopped at an older one and one that min_sc drops."""
    reset(dev)
    (par, off, a, min_cnt), props, exp = bt_singles()[i]
    edge = ("backtracker", es.BT_EDGES[i])
    run(edge, dev, par, off, a, exp)
    coff, u, boff, b = check_chains(edge, dev, par, min_cnt, exp)
    assert len(u) == props["kept"] and len(exp["seeds"][0]) == props["records"]


def test_backtracker_all_regimes_in_one_call(dev):
    """Every edge read in one call, so that the three record regimes run side by side on the scratch arrays they share
    (pdense / b_tmp, blk / c_src, chain_read / key, end_read / c_dst), among reads without anchors (first, two in the middle,
    two last: the ends_off back-fill and k_bt_close_offsets), a read without records, and a 1024-record block over three reads
    and an empty one.  The same call again after another batch on the same context (stale scratch), and every read's chains
    against those of the same read run alone."""
    reset(dev)
    (par, off, a, min_cnt), props, exp = case("bt_combined")
    edge = "backtracker, combined batch"
    run(edge, dev, par, off, a, exp)
    first = check_chains(edge, dev, par, min_cnt, exp)
    alone = {}
    for i, ((spar, soff_, sa, smin), _, sexp) in enumerate(bt_singles()):
        dev.chain_batch(spar, soff_, sa)
        dev.compact(spar)
        alone[i] = dev.backtrack(spar, smin)
    (opar, ooff, oa, omin), _, oexp = case("bt_other_batch")
    run("backtracker, other batch", dev, opar, ooff, oa, oexp)
    check_chains("backtracker, other batch", dev, opar, omin, oexp)
    run(edge + " again", dev, par, off, a, exp)
    again = check_chains(edge + " again", dev, par, min_cnt, exp)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    coff, u, boff, b = again
    for r, i in props["edge_at"].items():
        _, su, _, sb = alone[i]
        assert np.array_equal(u[int(coff[r]):int(coff[r + 1])], su), (edge, "read", r, es.BT_EDGES[i], "u differs from the read run alone")
        assert np.array_equal(b[int(boff[r]):int(boff[r + 1])], sb), (edge, "read", r, es.BT_EDGES[i], "b differs from the read run alone")


# ---------------------------------------------------------------- DP routing

@pytest.mark.parametrize("two_tables", [False, True], ids=["one_table_layout", "table_per_half"])
def test_int8_fit_of_the_cost_table(dev, two_tables):
    """bw = 500: the table's last entry is -128 for a read of spans 25 (k_chain_twin keeps the table as bytes) and -129 with
    every fifth span 26 (SUMQ_LUT16_FLAG in k_build_lut, lut16 in k_unit_scatter: the unit goes to k_chain_units)."""
    reset(dev)
    try:
        dev.set_twin_tables(two_tables)
        for name in ("fit", "nofit", "mixed"):
            (par, off, a), props, exp = cases("int8_batches")[name]
            edge = ("int8 fit", name, "twin_tables", two_tables)
            dev.set_variant(0)
            got = dev.chain_batch(par, off, a)
            left, tables, units = dev.leftover_units(), dev.twin_tables(), dev.stats()["units"]
            observed(edge, leftover_units=left, twin_tables=tables, units=units)
            check_fpv(edge, off, got, exp)
            check_seeds(edge, dev, par, exp)
            assert units == sum(props["units"]), (edge, units)
            assert left == props["units_nofit"], (edge, "leftover_units", left, props["units_nofit"])
            if name == "fit":
                assert tables == (2 if two_tables else 1), (edge, "twin_tables", tables)
            dev.set_variant(2)
            run(edge + ("variant 2",), dev, par, off, a, exp)
    finally:
        reset(dev)


@pytest.mark.parametrize("bw", [511, 512])
def test_bw_at_the_twin_kernels_table_size(dev, bw):
    """k_chain_twin holds bw + 1 <= 512 table bytes: bw 511 stays, bw 512 hands every unit over.  One pair with |dr - dq| = bw
    chains and one with bw + 1 does not (the oracle's p, asserted on the CPU tier)."""
    reset(dev)
    try:
        (par, off, a), props, exp = case("bw_batch", bw, 15, 20)
        for variant in (0, 2):
            dev.set_variant(variant)
            edge = ("bw", bw, "variant", variant)
            got = dev.chain_batch(par, off, a)
            left, units = dev.leftover_units(), dev.stats()["units"]
            observed(edge, leftover_units=left, units=units)
            check_fpv(edge, off, got, exp)
            check_seeds(edge, dev, par, exp)
            assert units == props["units"]
            if variant == 0:
                assert left == (0 if bw == 511 else units), (edge, "leftover_units", left, units)
    finally:
        reset(dev)


@pytest.mark.parametrize("bw", [4095, 4096])
def test_bw_at_the_cost_tables_limit(dev, bw):
    """bw 4095 is the widest cost table (entries of spans 255 still fit 16 bits), bw 4096 takes the general 64-bit variant.  No
    hook tells the table-driven from the general variant of k_chain_units: parity alone, under variants 0 and 2 and rings 128
    and 512, with a pair at |dr - dq| = bw that chains and one at bw + 1 that does not."""
    reset(dev)
    try:
        (par, off, a), props, exp = case("bw_batch", bw, 255, 60)
        for variant in (0, 2):
            for ring in (128, 512):
                dev.set_variant(variant); dev.set_ring(ring)
                run(("bw", bw, "variant", variant, "ring", ring), dev, par, off, a, exp)
    finally:
        reset(dev)


@pytest.mark.parametrize("above", [0, 1], ids=["M", "M_plus_1"])
def test_max_dist_x_at_the_twin_kernels_bound(dev, above):
    """129 * (max_dist_x + 1) < 2^31 holds at M and fails at M + 1: there every unit is handed over.  The unit has gaps of
    exactly max_dist_x and pairs that chain across them."""
    reset(dev)
    try:
        mdx = es.largest_mdx(129, 31) + above
        (par, off, a), props, exp = case("mdx_twin_batch", mdx)
        for variant in (0, 2):
            dev.set_variant(variant)
            edge = ("max_dist_x, twin bound", mdx, "variant", variant)
            got = dev.chain_batch(par, off, a)
            left, units = dev.leftover_units(), dev.stats()["units"]
            observed(edge, leftover_units=left, units=units)
            check_fpv(edge, off, got, exp)
            check_seeds(edge, dev, par, exp)
            assert units == props["units"]
            if variant == 0:
                assert left == (units if above else 0), (edge, "leftover_units", left, units)
    finally:
        reset(dev)


@pytest.mark.parametrize("above", [0, 1], ids=["M", "M_plus_1"])
@pytest.mark.parametrize("ring", [128, 256, 512])
def test_max_dist_x_at_the_ring_bounds(dev, ring, above):
    """(max_dist_x + 1) * (ring + 1) < 2^32: the table-driven variant of k_chain_units keeps 32-bit differences at M and the
    general variant takes over at M + 1.  ring + 8 anchors at gaps of exactly max_dist_x, x running past 2^32."""
    reset(dev)
    try:
        mdx = es.largest_mdx(ring + 1, 32) + above
        (par, off, a), props, exp = case("mdx_ring_batch", mdx, ring, 0)
        dev.set_ring(ring); dev.set_variant(2)
        run(("max_dist_x, ring bound", ring, mdx), dev, par, off, a, exp)
        assert dev.stats()["units"] == props["units"]
    finally:
        reset(dev)


@pytest.mark.parametrize("above", [0, 1], ids=["M", "M_plus_1"])
@pytest.mark.parametrize("ring,mode", [(512, 2), (1024, 4)], ids=["dense_513", "dense16_1025"])
def test_max_dist_x_at_the_dense_kernels_bounds(dev, ring, mode, above):
    """The dense hand-over keeps 32-bit differences over 512 anchors (k_chain_dense: (max_dist_x + 1) * 513 < 2^32, or nothing is
    handed over) and over 1024 (k_chain_dense16: * 1025).  The unit starts with 1500 anchors whose scans run deep, then has
    ring + 8 anchors at gaps of exactly max_dist_x."""
    reset(dev)
    try:
        mdx = es.largest_mdx(ring + 1, 32) + above
        (par, off, a), props, exp = case("mdx_ring_batch", mdx, ring, 1500)
        for variant in (0, 2):
            dev.set_variant(variant); dev.set_deep_handover(mode)
            edge = ("max_dist_x, dense bound", ring + 1, mdx, "variant", variant)
            got = dev.chain_batch(par, off, a)
            deep = dev.deep_units()
            observed(edge, deep_units=deep)
            check_fpv(edge, off, got, exp)
            check_seeds(edge, dev, par, exp)
            if ring == 512:
                assert deep == (0 if above else 1), (edge, "deep_units", deep)
            else:
                assert deep == 1, (edge, "deep_units", deep)
    finally:
        reset(dev)


def test_short_units_average(dev):
    """k_chain_twin takes the batch while (total - singletons) <= 512 * units: at equality it runs (twin_tables() != 0), one
    anchor above it leaves everything to k_chain_units."""
    reset(dev)
    try:
        for name in ("equal", "above"):
            (par, off, a), props, exp = cases("short_units_batches")[name]
            got = dev.chain_batch(par, off, a)
            tables, st = dev.twin_tables(), dev.stats()
            observed(("short_units", name), twin_tables=tables, **st)
            check_fpv(("short_units", name), off, got, exp)
            check_seeds(("short_units", name), dev, par, exp)
            assert st["units"] == props["units"] and st["singletons"] == props["singletons"]
            assert (tables != 0) == (name == "equal"), ("short_units", name, "twin_tables", tables)
    finally:
        reset(dev)


@pytest.mark.parametrize("n", [es.DENSE_BITCAP, es.DENSE_BITCAP + 1])
def test_dense_unit_at_the_mark_bitmaps_size(dev, n):
    """Default settings: a unit of 65536 anchors is handed to the dense kernel (room <= CHAINDP_DENSE_BITCAP), one of 65537
    stays with k_chain_units."""
    reset(dev)
    try:
        (par, off, a), props, exp = case("dense_bitmap_batch", n)
        for variant in (0, 2):
            dev.set_variant(variant)
            edge = ("dense bitmap", n, "variant", variant)
            got = dev.chain_batch(par, off, a)
            deep = dev.deep_units()
            observed(edge, deep_units=deep)
            check_fpv(edge, off, got, exp)
            check_seeds(edge, dev, par, exp)
            assert deep == (1 if n <= es.DENSE_BITCAP else 0), (edge, "deep_units", deep)
    finally:
        reset(dev)


def test_hand_over_cap(dev):
    """2200 units that all qualify: k_chain_dense and k_chain_dense16 take CHAINDP_DENSE_UNITS of them (the check and the count's
    atomicAdd are apart, so a few more), the rest stays with k_chain_units and must match as well; k_chain_dense1 has no cap."""
    reset(dev)
    try:
        (par, off, a), props, exp = case("dense_units_batch", 2200, 320, 11)
        for variant in (0, 2):
            for mode in (2, 4, 3):
                dev.set_variant(variant); dev.set_deep_handover(mode)
                edge = ("hand-over cap", "mode", mode, "variant", variant)
                got = dev.chain_batch(par, off, a)
                deep = dev.deep_units()
                observed(edge, deep_units=deep)
                check_fpv(edge, off, got, exp)
                if mode == 3:
                    assert es.DENSE_UNITS < deep <= props["units"], (edge, "deep_units", deep)
                else:
                    assert es.DENSE_UNITS <= deep < props["units"], (edge, "deep_units", deep)
                if variant == 0:
                    check_seeds(edge, dev, par, exp)
    finally:
        reset(dev)


@pytest.mark.parametrize("n_units", [es.DENSE16_MAX_UNITS, es.DENSE16_MAX_UNITS + 1])
def test_dense_kernel_by_the_batchs_own_decision(dev, n_units):
    """Default hand-over (units of 2400 anchors, above CHAINDP_DEEP_HANDOVER_LEFT): 256 handed-over units go to k_chain_dense16,
    257 to the eight-wave k_chain_dense, without the forcing hook."""
    reset(dev)
    try:
        (par, off, a), props, exp = case("dense_units_batch", n_units, 2400, 8)
        got = dev.chain_batch(par, off, a)
        deep = dev.deep_units()
        edge = ("dense16 / dense", n_units)
        observed(edge, deep_units=deep)
        check_fpv(edge, off, got, exp)
        check_seeds(edge, dev, par, exp)
        assert deep == n_units, (edge, "deep_units", deep)
    finally:
        reset(dev)


# ---------------------------------------------------------------- alignment

ALIGN = {"confetti": ("confetti_batch", False), "confetti_block_multiple": ("confetti_batch", True), "adjacent_reads": ("adjacent_reads_batch",),
         "unit_lengths": ("unit_lengths_batch",)}


@pytest.mark.parametrize("name", list(ALIGN))
def test_alignment_batches(dev, name):
    """Read and unit boundaries on lanes 0, 1 and 63 of the prepass' 64-anchor tiles and on the first and last anchor of its
    1024-anchor blocks, dozens of boundaries in a tile, runs of empty reads, a last tile of one anchor; units of 1 .. 129
    anchors starting on lanes 0 and 63.  soff, coff and boff are compared whole: the offsets of empty reads count."""
    reset(dev)
    try:
        (par, off, a, min_cnt), props, exp = case(*ALIGN[name])
        for variant in (0, 2):
            for handover in (0, 2):
                if variant == 2 and handover:
                    continue
                dev.set_variant(variant); dev.set_twin_handover(handover)
                edge = (name, "variant", variant, "twin_handover", handover)
                run(edge, dev, par, off, a, exp)
                check_chains(edge, dev, par, 1, exp)
                check_chains(edge, dev, par, 3, exp, bottoms_for(exp, par, 3))
    finally:
        reset(dev)
