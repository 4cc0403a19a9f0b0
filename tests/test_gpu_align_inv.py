"""GPU tier: chaindp_align1_inv (mm_align1_inv on the device: k_inv_ll, the extension through k_ksw_extd, k_inv_finish, the loop's rule)
against the reference's recorded answers, tests/golden/align_inv/*.npz -- every word of made, r_inv, extra, cigar_off and cigar, the
local scores with their end positions through the debug hook, and the route every extension took."""
import numpy as np
import pytest

import ksw_shapes as KS
from test_align_inv_cpu import SCENES, load, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def opt_of(g):
    from minimap2_chaindp_amd import params
    return params.AlignOpt(*(int(v) for v in g["opt"]))


def blocks(g):
    """A scene read by read: dicts of the read's inputs and of the outputs of its slots (ll: of its candidates)."""
    out = []
    cand_before = np.concatenate([[0], np.cumsum(g["made"] != 0)])
    for rd in range(len(g["seq_off"]) - 1):
        s0, s1, r0, r1 = (int(g[k][i]) for k in ("seq_off", "regs_off") for i in (rd, rd + 1))
        c0, c1 = int(g["cigar_off"][r0]), int(g["cigar_off"][r1])
        out.append(dict(seq=g["seq"][s0:s1], regs=g["regs"][r0:r1], made=g["made"][r0:r1], r_inv=g["r_inv"][r0:r1], extra=g["extra"][r0:r1],
                        cigar=g["cigar"][c0:c1], ll=g["ll"][cand_before[r0]:cand_before[r1]]))
    return out


def join(parts):
    """Scenes of one opt as one call: parts = [(scene, its blocks in the order wanted)].  The targets of every scene are kept, rid shifted."""
    g0 = parts[0][0]
    tseq, t_off, bl = [], [0], []
    for g, bs in parts:
        shift = len(t_off) - 1
        tseq.append(g["tseq"]); t_off += [t_off[-1] + int(v) for v in g["tseq_off"][1:]]
        for b in bs:
            regs, r_inv = b["regs"].copy(), b["r_inv"].copy()
            regs["rid"] += shift; r_inv["rid"][b["made"] == 1] += shift
            bl.append(dict(b, regs=regs, r_inv=r_inv))
    cat = lambda k, dt=None: np.concatenate([b[k] for b in bl]) if bl else np.zeros(0, dt)
    off = lambda k: np.concatenate([[0], np.cumsum([len(b[k]) for b in bl])]).astype(np.int64)
    extra = cat("extra")
    return dict(opt=g0["opt"], tseq=np.concatenate(tseq), tseq_off=np.array(t_off, np.int64), seq=cat("seq"), seq_off=off("seq"), regs=cat("regs"),
                regs_off=off("regs"), made=cat("made"), r_inv=cat("r_inv"), extra=extra, cigar=cat("cigar"), ll=cat("ll").reshape(-1, 3),
                cigar_off=np.concatenate([[0], np.cumsum(extra["n_cigar"])]).astype(np.int64))


def call(dev, g, **kw):
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    return dev.align1_inv(opt_of(g), g["seq_off"], g["seq"], g["regs_off"], g["regs"], **kw)


def check(dev, g, got):
    made, r_inv, extra, off, cig = got
    assert np.array_equal(made, g["made"]), (made.tolist()[:40], g["made"].tolist()[:40])
    for label, x, want in (("r_inv", r_inv, g["r_inv"]), ("extra", extra, g["extra"])):
        bad = np.flatnonzero((words(x).reshape(len(x), -1) != words(want).reshape(len(want), -1)).any(axis=1))
        assert not len(bad), [(label, int(i), x[i], want[i]) for i in bad[:4]]
    assert np.array_equal(off, g["cigar_off"]) and np.array_equal(cig, g["cigar"])
    assert np.array_equal(dev.align_inv_ll(len(g["ll"])), g["ll"])


def test_fixtures_are_there():
    assert len(SCENES) == 19


@pytest.mark.parametrize("name", SCENES)
def test_scene_in_one_call(dev, name):
    g = load(name)
    check(dev, g, call(dev, g))
    if len(g["prob"]):          # the extensions, in candidate order: the route the device took is the one the sizes ask for
        sc = tuple(int(v) for v in g["opt"][:6])
        assert dev.ksw_route(len(g["prob"])).tolist() == [KS.expected_route(int(q), int(t), sc) for q, t, _ in g["prob"]]


def test_extension_routes_are_all_taken(dev):
    seen = set()
    for name in ("stripe_edges", "route_wide", "route_global", "no_cigar"):
        g = load(name)
        call(dev, g)
        seen |= set(dev.ksw_route(len(g["prob"])).tolist())
    assert seen == {KS.ROUTE_NONE, KS.ROUTE_LDS, KS.ROUTE_WIDE, KS.ROUTE_GLOBAL}


def by_opt():
    groups = {}
    for name in SCENES:
        g = load(name)
        groups.setdefault(tuple(int(v) for v in g["opt"]), []).append(g)
    return list(groups.values())


def test_scenes_of_one_opt_in_one_call_and_in_reverse_order(dev):
    groups = by_opt()
    assert max(len(gs) for gs in groups) >= 8
    for gs in groups:
        g = join([(x, blocks(x)) for x in gs])
        check(dev, g, call(dev, g))
        g = join([(x, blocks(x)[::-1]) for x in gs[::-1]])
        check(dev, g, call(dev, g))


@pytest.mark.parametrize("name", ["fuzz", "early_returns"])
def test_scene_split_into_two_calls(dev, name):
    g = load(name)
    bs = blocks(g)
    for part in (bs[:len(bs) // 2], bs[len(bs) // 2:]):
        h = join([(g, part)])
        check(dev, h, call(dev, h))


def test_no_reads_no_regions_and_no_candidates(dev):
    from minimap2_chaindp_amd import chaindp
    g = load("fuzz")
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    z64 = np.zeros(1, np.int64)
    made, r_inv, extra, off, cig = dev.align1_inv(opt_of(g), z64, b"", z64, np.zeros(0, chaindp.REG_DTYPE))
    assert len(made) == 0 and off.tolist() == [0] and len(cig) == 0
    n = len(g["seq_off"]) - 1
    got = dev.align1_inv(opt_of(g), g["seq_off"], g["seq"], np.zeros(n + 1, np.int64), np.zeros(0, chaindp.REG_DTYPE))
    assert got[3].tolist() == [0]
    regs = g["regs"].copy(); regs["bits"] &= ~np.uint32(1 << 24)                # split_inv nowhere: every slot 0, nothing launched
    made, r_inv, extra, off, cig = dev.align1_inv(opt_of(g), g["seq_off"], g["seq"], g["regs_off"], regs)
    assert not made.any() and not words(r_inv).any() and not words(extra).any() and not off.any() and len(cig) == 0
    assert len(dev.align_inv_ll(0)) == 0


def test_small_cigar_cap_is_capacity_with_the_rest_filled(dev):
    from minimap2_chaindp_amd import chaindp
    g = load("fuzz")
    total = int(g["cigar_off"][-1])
    with pytest.raises(chaindp.ChainDPError, match="CIGAR words") as e:
        call(dev, g, cigar_cap=total - 1)
    err = e.value
    assert np.array_equal(err.cigar_off, g["cigar_off"]) and np.array_equal(err.made, g["made"])
    assert np.array_equal(words(err.r_inv), words(g["r_inv"])) and np.array_equal(words(err.extra), words(g["extra"]))
    with pytest.raises(chaindp.ChainDPError, match="CIGAR words"):
        call(dev, g, cigar_cap=0)                                  # cigar NULL with cigar_cap 0
    check(dev, g, call(dev, g, cigar_cap=total))                   # the exact room is enough, and the context is usable
    check(dev, g, call(dev, g))


def test_align1_and_ksw_extd_still_pass_around_it_on_one_context(dev):
    import test_gpu_align as TA
    import test_gpu_ksw as T

    def others():
        a = TA.load("fuzz")
        TA.check(a, TA.call(dev, a))
        for name in T.NAMED[:2] + T.FUZZ[:1]:
            k = T.load(name)
            ez, off, cig = T.call(dev, k)
            T.check(k, ez, off, cig)
            assert np.array_equal(dev.ksw_route(len(ez)), T.expected_routes(k))
    others()
    for name in ("fuzz", "route_wide", "three_regions_skip"):
        g = load(name)
        check(dev, g, call(dev, g))
    others()


def test_tiny_scene_tiled_past_65536_slots(dev):
    g = load("padding_strand0")
    n = 2 * 65536 // len(g["regs"]) + 50                           # more candidates than the widest grid too
    bs = blocks(g)
    tiled = join([(g, bs)])
    rep = lambda x: np.concatenate([x] * n)
    reps_off = lambda o: np.concatenate([[0]] + [o[1:] + k * o[-1] for k in range(n)]).astype(np.int64)
    big = dict(tiled, seq=rep(tiled["seq"]), seq_off=reps_off(tiled["seq_off"]), regs=rep(tiled["regs"]), regs_off=reps_off(tiled["regs_off"]),
               made=rep(tiled["made"]), r_inv=rep(tiled["r_inv"]), extra=rep(tiled["extra"]), cigar=rep(tiled["cigar"]), ll=rep(tiled["ll"]),
               cigar_off=reps_off(tiled["cigar_off"]))
    assert len(big["regs"]) > 2 * 65536 and len(big["ll"]) > 65536
    check(dev, big, call(dev, big))


def test_refusals_leave_the_context_usable(dev):
    from minimap2_chaindp_amd import chaindp, params
    g = load("padding_strand1")

    def refused(o=None, **arrays):
        h = dict(g, **arrays)
        with pytest.raises(chaindp.ChainDPError):
            dev.align1_inv(o or opt_of(g), h["seq_off"], h["seq"], h["regs_off"], h["regs"])
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    for change in (dict(flag=params.MM_F_SR), dict(flag=params.MM_F_SPLICE), dict(q2=4, e2=2), dict(a=128), dict(max_gap=20001)):
        o = opt_of(g)
        for k, v in change.items():
            setattr(o, k, v)
        refused(o)
    regs = g["regs"].copy(); regs["rid"][:2] = len(g["tseq_off"]) - 1
    refused(regs=regs)                                             # a candidate pair whose rid is no target
    regs = g["regs"].copy(); regs["rs"][1] += 100000; regs["re"][0] += 100000
    refused(regs=regs)                                             # ... whose target stretch lies outside its sequence
    dev.align_clear_targets()
    with pytest.raises(chaindp.ChainDPError, match="target"):
        dev.align1_inv(opt_of(g), g["seq_off"], g["seq"], g["regs_off"], g["regs"])
    check(dev, g, call(dev, g))


# ---- the three alignment stages on one context: what they share on the host (the packed-CIGAR buffer, the stage events)
def stage_calls(dev):
    """name -> a function that makes one call of the stage on `scene` and checks every word of its result."""
    import test_gpu_align as TA
    import test_gpu_ksw as T

    def ksw(scene):
        k = T.load(scene)
        T.check(k, *T.call(dev, k))

    def align(scene):
        a = TA.load(scene)
        TA.check(a, TA.call(dev, a))

    def inv(scene):
        g = load(scene)
        check(dev, g, call(dev, g))
    return dict(ksw_extd=ksw, align1=align, align1_inv=inv)


@pytest.fixture()
def fresh():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def test_one_packed_cigar_buffer_serves_the_three_stages_in_any_order(fresh):
    """Small after large, large after small (the buffer grows) and a call that packs nothing after one that did."""
    run = stage_calls(fresh)
    order = [("ksw_extd", "fuzz_asm10"), ("align1_inv", "no_cigar"), ("align1", "fuzz"), ("align1_inv", "fuzz"), ("ksw_extd", "named_early")]
    assert int(load("no_cigar")["cigar_off"][-1]) == 0
    for stage, scene in order + order[::-1]:
        run[stage](scene)


def test_alignment_stages_hold_their_memory_steady(fresh):
    run = stage_calls(fresh)
    held = []
    for _ in range(4):
        run["ksw_extd"]("fuzz_asm10"); run["align1"]("fuzz"); run["align1_inv"]("fuzz")
        held.append(fresh.device_bytes())
    print("device_bytes after each round of ksw_extd, align1, align1_inv:", held)
    assert held[1] == held[3], held


def test_stage_ms_hooks_follow_the_profiling_switch(fresh):
    run = stage_calls(fresh)
    scenes = dict(ksw_extd="fuzz_asm10", align1="fuzz", align1_inv="fuzz")
    ms = lambda: dict(ksw_extd=[fresh.ksw_ms()], align1=list(fresh.align_ms().values()), align1_inv=list(fresh.align_inv_ms().values()))
    before = ms()
    assert [len(v) for v in before.values()] == [1, 5, 4] and all(x == -1 for v in before.values() for x in v), before
    fresh.set_profiling(True)
    for stage, scene in scenes.items():
        run[stage](scene)
        after = ms()
        assert all(np.isfinite(x) and x >= 0 for x in after[stage]), (stage, after)
        assert all(after[s] == before[s] for s in scenes if s != stage), (stage, before, after)
        before = after
    fresh.set_profiling(False)
    for stage, scene in scenes.items():
        run[stage](scene)
    assert ms() == before
