"""GPU tier: chaindp_ksw_extd (k_ksw_extd) against the reference's recorded answers, tests/golden/ksw/*.npz -- every field of
ksw_extz_t and every CIGAR word of every problem, and the route the device reports for it."""
import glob
import os

import numpy as np
import pytest

import ksw_shapes as S
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

KSW_DIR = os.path.join(GOLDEN_DIR, "ksw")
NAMED = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(KSW_DIR, "named_*.npz")))
FUZZ = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(KSW_DIR, "fuzz_*.npz")))
INPUTS = ("bases", "q_beg", "q_len", "t_beg", "t_len")
PER_PROBLEM = ("w", "zdrop", "end_bonus", "flag")


def load(name):
    z = np.load(os.path.join(KSW_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def call(dev, g, sel=None, **kw):
    a = {k: g[k] for k in INPUTS + PER_PROBLEM}
    if sel is not None:
        for k in a:
            if k != "bases":
                a[k] = a[k][sel]
    return dev.ksw_extd(*(a[k] for k in INPUTS), tuple(int(x) for x in g["scoring"]), *(a[k] for k in PER_PROBLEM), **kw)


def expected_routes(g):
    sc = tuple(int(x) for x in g["scoring"])
    return np.array([S.expected_route(int(q), int(t), sc) for q, t in zip(g["q_len"], g["t_len"])], np.int32)


def check(g, ez, off, cig, names=None):
    names = g["name"] if names is None else names
    bad = np.flatnonzero((ez != g["ez"]).any(axis=1))
    assert not len(bad), [(str(names[i]), ez[i].tolist(), g["ez"][i].tolist()) for i in bad[:5]]
    assert np.array_equal(off, g["cigar_off"]), [str(names[i]) for i in np.flatnonzero(np.diff(off) != np.diff(g["cigar_off"]))[:5]]
    assert np.array_equal(cig, g["cigar"])


def test_fixtures_are_there():
    assert len(NAMED) == 7 and len(FUZZ) == 5, (NAMED, FUZZ)


@pytest.mark.parametrize("name", NAMED + FUZZ)
def test_batch_in_one_call(dev, name):
    g = load(name)
    ez, off, cig = call(dev, g)
    check(g, ez, off, cig)
    assert np.array_equal(dev.ksw_route(len(ez)), expected_routes(g))


def test_every_route_is_taken():
    routes = np.concatenate([expected_routes(load(n)) for n in NAMED])
    assert set(routes.tolist()) == {S.ROUTE_NONE, S.ROUTE_LDS, S.ROUTE_GLOBAL, S.ROUTE_WIDE}


@pytest.mark.parametrize("name", NAMED)
def test_named_in_calls_of_one(dev, name):
    g = load(name)
    want_route = expected_routes(g)
    for i in range(len(g["name"])):
        ez, off, cig = call(dev, g, sel=slice(i, i + 1))
        lo, hi = int(g["cigar_off"][i]), int(g["cigar_off"][i + 1])
        assert np.array_equal(ez[0], g["ez"][i]), (str(g["name"][i]), ez[0].tolist(), g["ez"][i].tolist())
        assert off.tolist() == [0, hi - lo] and np.array_equal(cig, g["cigar"][lo:hi]), str(g["name"][i])
        assert dev.ksw_route(1)[0] == want_route[i], str(g["name"][i])


def test_short_cigar_cap_then_exact(dev):
    from minimap2_chaindp_amd import chaindp
    g = load("named_sr")
    need = int(g["cigar_off"][-1])
    assert need > 1
    with pytest.raises(chaindp.ChainDPError, match="chaindp error -2") as ei:
        call(dev, g, cigar_cap=need - 1)
    assert np.array_equal(ei.value.cigar_off, g["cigar_off"]) and np.array_equal(ei.value.ez, g["ez"])
    ez, off, cig = call(dev, g, cigar_cap=int(ei.value.cigar_off[-1]))
    check(g, ez, off, cig)
    with pytest.raises(chaindp.ChainDPError, match="chaindp error -2"):
        call(dev, g, cigar_cap=0)


def test_empty_call(dev):
    g = load("named_default")
    before = dev.device_bytes()
    ez, off, cig = dev.ksw_extd(np.zeros(0, np.uint8), [], [], [], [], S.SCORING["default"], [], [], [], [])
    assert ez.shape == (0, 10) and off.tolist() == [0] and len(cig) == 0
    assert dev.device_bytes() == before
    ez, off, cig = call(dev, g)
    check(g, ez, off, cig)


@pytest.mark.parametrize("name,change,code", S.REFUSALS, ids=[r[0] for r in S.REFUSALS])
def test_refusals(dev, name, change, code):
    from minimap2_chaindp_amd import chaindp
    base = S.refusal_base_call()
    order = ("bases", "q_beg", "q_len", "t_beg", "t_len", "scoring", "w", "zdrop", "end_bonus", "flag")
    good = dev.ksw_extd(*(base[k] for k in order))
    bad = dict(base)
    for k, v in change.items():
        bad[k] = v(base[k]) if callable(v) else v
    with pytest.raises(chaindp.ChainDPError, match=f"chaindp error {code}:"):
        dev.ksw_extd(*(bad[k] for k in order))
    again = dev.ksw_extd(*(base[k] for k in order))           # the context is still usable, and gives the same
    assert all(np.array_equal(x, y) for x, y in zip(good, again))


def test_device_bytes_constant_over_a_repeated_batch(dev):
    g = load("fuzz_asm10")
    call(dev, g)
    first = dev.device_bytes()
    for _ in range(3):
        ez, off, cig = call(dev, g)
        assert dev.device_bytes() == first
    check(g, ez, off, cig)
    dev.ksw_extd(np.zeros(0, np.uint8), [], [], [], [], S.SCORING["asm10"], [], [], [], [])
    assert dev.device_bytes() == first


def test_a_context_without_alignment_allocates_nothing_for_it():
    from minimap2_chaindp_amd import chaindp
    g = load("named_early")
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as a, chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as b:
        assert a.device_bytes() == b.device_bytes()
        call(a, g)
        assert a.device_bytes() > b.device_bytes()


def test_map_seqs_before_and_after_gives_the_same_bytes():
    """The alignment shares the context with the mapping stages and disturbs none of them."""
    import e2e_model as em
    from minimap2_chaindp_amd import chaindp
    from test_gpu_e2e import map_seqs
    sc = em.scenario("map-ont", n_reads=16, max_len=2000)
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 10) as d:
        ix = d.load_index(sc.image())
        first = map_seqs(d, ix, sc)
        g = load("fuzz_default")
        ez, off, cig = call(d, g)
        check(g, ez, off, cig)
        second = map_seqs(d, ix, sc)
    assert len(first[1]) > 0 and len(first) == len(second)
    for x, y in zip(first, second):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
