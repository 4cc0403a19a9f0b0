"""GPU tier of the extension alignment's edge scenes: chaindp_ksw_extd (k_ksw_extd) against the reference's recorded answers,
tests/golden/ksw_edges/*.npz (inputs: tests/ksw_edge_shapes.py) -- scoring sets from the corners of 0..127, the global route under every
flag and both ways out of its loop, one-base sides on the wide route; then the same recordings with the launches capped at one, two and
three workgroups (Device.ksw_set_grid_cap), so that a workgroup takes unlike problems one after another, and tiled until the natural
grid is passed.  Every comparison is of every word: the ten ez fields, cigar_off, every CIGAR word, the route."""
import time

import numpy as np
import pytest

import ksw_edge_shapes as E
import test_gpu_ksw as T
from test_gpu_ksw import call, check, dev, expected_routes  # noqa: F401  (dev: the module's context fixture)
from test_ksw_edges_cpu import SCENES, load

pytestmark = pytest.mark.gpu

SCORING_SCENES = [n for n in SCENES if n.startswith("scoring_")]
PER_PROBLEM = ("q_beg", "q_len", "t_beg", "t_len", "w", "zdrop", "end_bonus", "flag")
INT_MAX, INT_MIN = 2**31 - 1, -2**31


@pytest.fixture
def cap(dev):
    """Sets the grid cap; back to 0 (the plan's own grid) whatever the test does."""
    try:
        yield dev.ksw_set_grid_cap
    finally:
        dev.ksw_set_grid_cap(0)


def recorded(name):
    return load(name) if name in SCENES else T.load(name)


@pytest.mark.parametrize("name", SCENES)
def test_scene_in_one_call(dev, name):
    g = load(name)
    ez, off, cig = call(dev, g)
    check(g, ez, off, cig)
    assert np.array_equal(dev.ksw_route(len(ez)), expected_routes(g))


@pytest.mark.parametrize("name", SCORING_SCENES)
def test_scoring_in_calls_of_one(dev, name):
    g = load(name)
    want_route = expected_routes(g)
    for i in range(len(g["name"])):
        ez, off, cig = call(dev, g, sel=slice(i, i + 1))
        lo, hi = int(g["cigar_off"][i]), int(g["cigar_off"][i + 1])
        assert np.array_equal(ez[0], g["ez"][i]), (str(g["name"][i]), ez[0].tolist(), g["ez"][i].tolist())
        assert off.tolist() == [0, hi - lo] and np.array_equal(cig, g["cigar"][lo:hi]), str(g["name"][i])
        assert dev.ksw_route(1)[0] == want_route[i], str(g["name"][i])


@pytest.mark.parametrize("name", ["interleave", "global_flags", "named_default"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_grid_cap(dev, cap, n, name):
    """One, two or three workgroups take the whole launch: every problem but the first few follows another one in the same LDS or global
    state, path slice and exchange words.  named_default: 204 problems of all four routes, the large_* ones included."""
    g = recorded(name)
    cap(n)
    t0 = time.perf_counter()
    ez, off, cig = call(dev, g)
    dt = time.perf_counter() - t0
    launch = dev.ksw_launch()
    print(f"cap {n}, {name}: {launch}, {dt:.2f} s")
    check(g, ez, off, cig)
    assert np.array_equal(dev.ksw_route(len(ez)), expected_routes(g))
    routes = expected_routes(g)
    assert launch["count"] == (int((routes != E.ROUTE_WIDE).sum()), int((routes == E.ROUTE_WIDE).sum()))
    for c in range(2):
        assert launch["grid"][c] <= n
        assert launch["count"][c] == 0 or launch["count"][c] > launch["grid"][c] > 0, launch
    assert launch["count"][0] > n


def unit_of(parts):
    """Problems of several recordings of one scoring set as one call's arrays over shared bases: parts = [(g, mask)]."""
    out = {k: [] for k in PER_PROBLEM + ("bases", "ez", "cigs")}
    base = 0
    for g, mask in parts:
        assert tuple(g["scoring"]) == tuple(parts[0][0]["scoring"])
        idx = np.flatnonzero(mask)
        for k in PER_PROBLEM:
            out[k].append(g[k][idx] + (base if k.endswith("_beg") else 0))
        out["bases"].append(g["bases"]); base += len(g["bases"])
        out["ez"].append(g["ez"][idx])
        out["cigs"] += [g["cigar"][g["cigar_off"][i]:g["cigar_off"][i + 1]] for i in idx]
    unit = {k: np.concatenate(out[k]) for k in PER_PROBLEM + ("bases", "ez")}
    unit["cigs"], unit["scoring"] = out["cigs"], parts[0][0]["scoring"]
    return unit


def tiled(unit, times, seed):
    """The unit's problems `times` times over the same bases, in a seeded order; the recorded answers the same way."""
    n = len(unit["ez"])
    perm = np.random.default_rng(seed).permutation(n * times)
    g = {k: np.tile(unit[k], times)[perm] for k in PER_PROBLEM}
    g["bases"], g["scoring"] = unit["bases"], unit["scoring"]
    g["ez"] = np.tile(unit["ez"], (times, 1))[perm]
    cigs = [unit["cigs"][i % n] for i in perm]
    g["cigar_off"] = np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.int64)
    g["cigar"] = np.concatenate(cigs).astype(np.uint32)
    g["name"] = np.array([f"tile_{i}" for i in perm])
    return g


def routes_of(g):
    return expected_routes(g)


def run_past_the_grid(dev, unit, c, enough):
    """Tiles the unit until enough(launch) holds for the very call made, and compares that call."""
    times = 4
    while True:
        g = tiled(unit, times, seed=20241022 + times)
        t0 = time.perf_counter()
        ez, off, cig = call(dev, g)
        dt = time.perf_counter() - t0
        launch = dev.ksw_launch()
        print(f"launch {c}: x{times}, {launch}, {dt:.2f} s")
        if enough(launch):
            break
        assert times < 1024 and launch["count"][c] == times * len(unit["ez"])
        times *= 2
    check(g, ez, off, cig)
    assert np.array_equal(dev.ksw_route(len(ez)), routes_of(g))
    return launch


def test_one_wave_launch_past_its_natural_grid(dev):
    """No cap: the fuzz batch and every LDS and global problem of named_default and global_flags, repeated over shared bases until the
    plan's own grid is a quarter short of the problems and k_ksw_pack's 4 096 workgroups take a second stride."""
    parts = [(T.load("fuzz_default"), None), (T.load("named_default"), None), (load("global_flags"), None)]
    parts = [(g, routes_of(g) != E.ROUTE_WIDE) for g, _ in parts]
    launch = run_past_the_grid(dev, unit_of(parts), 0, lambda la: la["count"][0] >= 1.25 * la["grid"][0] and la["count"][0] > 4096)
    assert launch["count"][1] == 0 and launch["grid"][0] > 64


def test_wide_launch_past_its_natural_grid(dev):
    parts = [(g, routes_of(g) == E.ROUTE_WIDE) for g in (T.load("named_default"), load("wide_small_sides"), load("interleave"))]
    launch = run_past_the_grid(dev, unit_of(parts), 1, lambda la: la["count"][1] > la["grid"][1])
    assert launch["count"][0] == 0 and launch["grid"][1] > 64


@pytest.mark.parametrize("w", [INT_MAX, INT_MIN])
def test_band_at_the_ends_of_int32(dev, w):
    """w = 2^31 - 1 is the band of w = max(qlen, tlen) (the plan clamps it: r + w cannot overflow), w = -2^31 is no band: both are the
    recorded w = -1 answers."""
    g = T.load("named_default")
    names = np.array([str(x) for x in g["name"]])
    sel = np.flatnonzero([(n.startswith("size_") or n.startswith("band_")) and g["w"][i] == -1 for i, n in enumerate(names)])
    assert len(sel) == 54
    h = dict(g, w=np.where(np.isin(np.arange(len(names)), sel), w, g["w"]).astype(np.int32))
    ez, off, cig = call(dev, h, sel=sel)
    want = unit_of([(g, np.isin(np.arange(len(names)), sel))])
    assert np.array_equal(ez, want["ez"])
    assert np.array_equal(np.diff(off), [len(c) for c in want["cigs"]]) and np.array_equal(cig, np.concatenate(want["cigs"]))


def test_region_alignment_under_cap_1(dev, cap):
    """chaindp_align1 plans its DP through the same route: the scene with one-wave, several-wave and global problems in its first pass."""
    import test_gpu_align as A
    import test_gpu_align_edges as AE
    g = AE.load("global_left")
    cap(1)
    got = A.call(dev, g)
    launch = dev.ksw_launch()
    A.check(g, got)
    assert max(launch["grid"]) <= 1, launch


@pytest.mark.parametrize("name", ["route_wide", "route_global"])
def test_inversion_alignment_under_cap_1(dev, cap, name):
    import test_gpu_align_inv as I
    g = I.load(name)
    cap(1)
    got = I.call(dev, g)
    launch = dev.ksw_launch()
    I.check(dev, g, got)
    assert max(launch["grid"]) == 1, launch


def test_afterwards_the_context_is_as_before(dev):
    """Cap 0 again: named_sr takes the plan's own grid (a workgroup per problem), and a repeat allocates nothing."""
    g = T.load("named_sr")
    ez, off, cig = call(dev, g)
    check(g, ez, off, cig)
    launch = dev.ksw_launch()
    assert launch["grid"] == launch["count"], launch
    first = dev.device_bytes()
    ez, off, cig = call(dev, g)
    check(g, ez, off, cig)
    assert dev.device_bytes() == first and dev.ksw_launch() == launch
    with pytest.raises(Exception, match="chaindp error -1"):
        dev.ksw_set_grid_cap(-1)
    assert dev.ksw_launch() == launch
