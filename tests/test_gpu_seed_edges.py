"""GPU tier: the inputs of tests/seed_edge_shapes.py (proved to sit on their edges by tests/test_seed_edge_shapes_cpu.py) through seed
collection on the GPU, each alone and the small ones of every limit setting as one batch over one image (combined: more units than
the sort has workgroups, work items from many reads, the reference's procedure for hundreds of units in one launch): a_off, anchors,
rep_len, mp_off and mini_pos bit for bit against the restatement of collect_seed_hits, and beside the parity the ROUTE the device
reports (Device.seed_route(): the limits the context settled on, the work items k_seed_sort_huge made, the units with equal x)
against the routing restated on the CPU tier.  The cases are built relative to the limits read from the device.  Each limit setting
(the device's own; CHAINDP_SEED_MAX_N=64,512 for the pair network; 128,128 with CHAINDP_SEED_LAB_CAP=1024 for k_seed_sort_huge and the
one-thread kernel) has a context of its own: the switches are read when a context first collects seeds.  A failure names the edge,
the read and the place."""
import time

import numpy as np
import pytest

import seed_edge_shapes as ss
from minimap2_chaindp_amd import chaindp
from test_seed_edge_shapes_cpu import PROBE_CASES, SCAN_LARGE, SETTINGS, _id, expected, models_of, radix_fits, sort_cases

pytestmark = pytest.mark.gpu


def observed(edge, **values):
    """The route the hook reports, printed before it is asserted (pytest -s shows it)."""
    print("edge:", edge, " ".join(f"{k}={v}" for k, v in values.items()))


def _context(setting, max_anchors, max_reads=1 << 12):
    """A context that has settled on the limits of `setting`: yields (device, Limits as the device reports them)."""
    env_n, env_cap = SETTINGS[setting]
    with chaindp.Device(0, max_anchors=max_anchors, max_reads=max_reads) as d:
        assert d.seed_route() == dict(max_n=-1, max_n2=-1, lab_cap=0, items=0, tied=0)       # nothing collected yet
        with pytest.MonkeyPatch.context() as mp:
            for k, v in (("CHAINDP_SEED_MAX_N", env_n), ("CHAINDP_SEED_LAB_CAP", env_cap)):
                if v is None:
                    mp.delenv(k, raising=False)
                else:
                    mp.setenv(k, v)
            c, _ = ss.sorted_read(ss.Limits(64, 64, 256), 2, "front")
            d.collect_seeds(d.load_index(c.image), c.flag, c.max_occ, c.mini_off, c.mini, c.bid, c.qlen)
        r = d.seed_route()
        assert r["tied"] == 1 and r["items"] == 0
        yield d, ss.Limits(r["max_n"], r["max_n2"], r["lab_cap"])


@pytest.fixture(scope="module")
def dev_default():
    yield from _context("default", 1 << 16)


@pytest.fixture(scope="module")
def dev_pair():
    yield from _context("pair", 1 << 14)


@pytest.fixture(scope="module")
def dev_huge():
    yield from _context("huge", 1 << 16)


def collect(dev, case):
    ix = dev.load_index(case.image)
    t0 = time.time()
    got = dev.collect_seeds(ix, case.flag, case.max_occ, case.mini_off, case.mini, case.bid, case.qlen)
    return got, dev.seed_route(), time.time() - t0


def same_seeds(edge, got, e):
    """a_off, anchors, rep_len, mp_off, mini_pos against the restatement; the first difference named."""
    off, a, rep, mpo, mp = got
    n_reads = len(e["case"].bid)
    bad = np.flatnonzero(off != e["a_off"])
    assert bad.size == 0, f"{edge}: a_off: read {int(bad[0]) - 1 if bad.size else -1}: {np.diff(off).tolist()[:16]}, expected {np.diff(e['a_off']).tolist()[:16]}"
    bad = np.flatnonzero((a != e["anchors"]).any(axis=1))
    if bad.size:
        i = int(bad[0])
        r = int(np.searchsorted(off, i, side="right") - 1)
        raise AssertionError(f"{edge}: anchors: read {r} ({int(off[r + 1] - off[r])} anchors), place {i - int(off[r])}: got {a[i, 0]:#x} {a[i, 1]:#x}, "
                             f"expected {e['anchors'][i, 0]:#x} {e['anchors'][i, 1]:#x}; {bad.size} places differ")
    bad = np.flatnonzero(rep[:n_reads] != e["rep_len"])
    assert bad.size == 0, f"{edge}: rep_len: read {int(bad[0]) if bad.size else -1}: got {rep[bad[:1]]}, expected {e['rep_len'][bad[:1]]}"
    bad = np.flatnonzero(mpo != e["mp_off"])
    assert bad.size == 0, f"{edge}: mp_off: read {int(bad[0]) - 1 if bad.size else -1}"
    bad = np.flatnonzero(mp != e["mini_pos"])
    assert bad.size == 0, f"{edge}: mini_pos: entry {int(bad[0]) if bad.size else -1} of {len(mp)}"


def check_sort_case(dev, L, setting, shape):
    edge = _id((setting,) + shape)
    e = expected(L, *shape)
    got, route, dt = collect(dev, e["case"])
    models = models_of(e)
    want_items, want_tied = sum(m["items"] for m in models), sum(m["tied_units"] for m in models)
    observed(edge, reads=len(models), n=e["props"]["n"][:16], routes=sorted({m["route"] for m in models}), items=route["items"], tied=route["tied"], want_items=want_items, want_tied=want_tied,
             ms=round(dt * 1e3, 1), **{k: route[k] for k in ("max_n", "max_n2", "lab_cap")})
    same_seeds(edge, got, e)
    assert (route["max_n"], route["max_n2"], route["lab_cap"]) == tuple(L), (edge, "the limits moved")
    assert route["tied"] == want_tied, f"{edge}: {route['tied']} units took the reference's procedure, {want_tied} have equal x"
    if all(m["route"] in ("lds16", "lds4") for m in models):                    # whole reads only: the tied units are the reads with ties
        assert want_tied == sum(1 for r, m in enumerate(models) if (e["per"][r][0][1:, 0] == e["per"][r][0][:-1, 0]).any()) and want_items == 0
    assert route["items"] == want_items, f"{edge}: k_seed_sort_huge made {route['items']} work items, expected {want_items}"
    if "items" in e["props"]:
        assert route["items"] == e["props"]["items"] and route["tied"] == e["props"]["tied_units"]
    return e, route, dt


def test_limits_of_this_device(dev_default, dev_pair, dev_huge):
    (_, d), (_, p), (_, h) = dev_default, dev_pair, dev_huge
    observed("limits", default=tuple(d), pair=tuple(p), huge=tuple(h))
    assert d.max_n2 <= 13312, "the 14-bit place field and the 16-bit halves of seed_radix_words' counts"
    assert 0 < d.max_n <= d.max_n2 and d.lab_cap >= 256
    assert tuple(p)[:2] == (64, 512) and tuple(h) == (128, 128, 1024)
    # the pair network is what sorts the reads of the second setting; everything of the first is radix-sorted
    assert not any(radix_fits(p, n) for n in ss.PAIR_SIZES) and radix_fits(d, d.max_n) and radix_fits(d, d.max_n2)


@pytest.mark.parametrize("shape", sort_cases("default"), ids=_id)
def test_sort_edges(dev_default, shape):
    dev, L = dev_default
    e, route, _ = check_sort_case(dev, L, "default", shape)
    if shape[0] == "layout_read":
        m = models_of(e)[0]
        if shape[1:3] == ("max_n2", 0):
            assert route["items"] == 0                                           # still sorted in LDS
        if shape[1:3] == ("max_n2", 1):
            assert m["route"] == "huge" and max(m["item_sizes"]) > 64 and route["items"] >= 1


@pytest.mark.parametrize("shape", sort_cases("pair"), ids=_id)
def test_pair_network_edges(dev_pair, shape):
    dev, L = dev_pair
    check_sort_case(dev, L, "pair", shape)


@pytest.mark.parametrize("shape", sort_cases("huge"), ids=_id)
def test_huge_and_big_edges(dev_huge, shape):
    dev, L = dev_huge
    e, route, dt = check_sort_case(dev, L, "huge", shape)
    if shape[0] == "huge_edge":
        print(f"\n{e['props']['n'][0]} anchors by {'k_seed_sort_huge' if shape[1] == 0 else 'the one-thread kernel'}: {dt * 1e3:.0f} ms with transfers")


@pytest.mark.parametrize("shape", PROBE_CASES, ids=_id)
def test_probe_expand_reads_edges(dev_default, shape):
    dev, L = dev_default
    e = expected(L, *shape)
    got, route, dt = collect(dev, e["case"])
    observed(_id(shape), reads=len(e["case"].bid), minimizers=len(e["case"].mini), anchors=int(e["a_off"][-1]), items=route["items"], tied=route["tied"], ms=round(dt * 1e3, 1))
    same_seeds(_id(shape), got, e)
    assert route["items"] == 0
    if shape == ("read_blocks", 0):                                             # reads, but no minimizer and no anchor: the sort is launched and finds nothing
        assert route["tied"] == 0


def test_route_counts_after_a_collection_without_reads(dev_default):
    """The hook's counts are the last collection's: zero after one without reads, whatever the one before left."""
    dev, L = dev_default
    e = expected(L, "whole_small_read", 65)
    got, route, _ = collect(dev, e["case"])
    assert route["tied"] == 1
    ix = dev.load_index(e["case"].image)
    dev.collect_seeds(ix, 0, 64, np.zeros(1, np.int64), np.zeros((0, 2), np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.int32))
    assert dev.seed_route() == dict(max_n=L.max_n, max_n2=L.max_n2, lab_cap=L.lab_cap, items=0, tied=0)


def test_scan_over_a_million_minimizers():
    """1024 * 1024 + 1 absent minimizers: 1025 scan tiles, two per thread of the second level; no anchors, a mini_pos entry each."""
    e = expected("default", "scan_minis", SCAN_LARGE)
    case = e["case"]
    with chaindp.Device(0, max_anchors=1 << 10, max_reads=len(case.bid) + 1) as dev:
        got, route, dt = collect(dev, case)
    print(f"\n{SCAN_LARGE} minimizers, {len(case.bid)} reads: {dt * 1e3:.0f} ms with transfers")
    same_seeds("scan-1048577", got, e)
    assert len(got[4]) == SCAN_LARGE and got[0][-1] == 0
