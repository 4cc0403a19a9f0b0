"""GPU tier: chaindp_align1 (mm_align1 on the device around k_ksw_extd) against the reference's recorded answers,
tests/golden/align/*.npz -- every word of the updated regions, of what was split off, of the extras, every CIGAR word and the returned
anchors."""
import glob
import os

import numpy as np
import pytest

import align_shapes as S
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

ALIGN_DIR = os.path.join(GOLDEN_DIR, "align")
SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ALIGN_DIR, "*.npz")))
OUTPUTS = ("a_out", "regs_out", "regs2", "extra", "cigar_off", "cigar")


def load(name):
    z = np.load(os.path.join(ALIGN_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def opt_of(g):
    from minimap2_chaindp_amd import params
    return params.AlignOpt(*(int(v) for v in g["opt"]))


def call(dev, g, reads=None, **kw):
    """align1 over the scene, or over its reads [reads[0], reads[1]) alone."""
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    lo, hi = (0, len(g["seq_off"]) - 1) if reads is None else reads
    part = {k: g[k + "_off"][lo:hi + 1] - g[k + "_off"][lo] for k in ("seq", "a", "regs")}
    cut = {k: g[k][g[k + "_off"][lo]:g[k + "_off"][hi]] for k in ("seq", "a", "regs")}
    return dev.align1(opt_of(g), part["seq"], cut["seq"], part["a"], cut["a"], part["regs"], cut["regs"], **kw)


def words(x):
    return x.view(np.uint32) if x.dtype.fields else x


def check(g, got, reads=None):
    lo, hi = (0, len(g["seq_off"]) - 1) if reads is None else reads
    r0, r1, a0, a1 = (int(g[k][i]) for k in ("regs_off", "a_off") for i in (lo, hi))
    a, regs, regs2, extra, off, cig = got
    names = g["read_name"]
    which = np.repeat(np.arange(len(names)), np.diff(g["regs_off"]))[r0:r1]
    assert np.array_equal(a, g["a_out"][a0:a1])
    for label, x, want in (("regs", regs, g["regs_out"][r0:r1]), ("regs2", regs2, g["regs2"][r0:r1]), ("extra", extra, g["extra"][r0:r1])):
        bad = np.flatnonzero((words(x).reshape(len(x), -1) != words(want).reshape(len(want), -1)).any(axis=1))
        assert not len(bad), [(label, str(names[which[i]]), x[i], want[i]) for i in bad[:4]]
    c0, c1 = int(g["cigar_off"][r0]), int(g["cigar_off"][r1])
    assert np.array_equal(off, g["cigar_off"][r0:r1 + 1] - c0)
    assert np.array_equal(cig, g["cigar"][c0:c1])


def test_fixtures_are_there():
    assert len(SCENES) == 14 and "fuzz" in SCENES, SCENES


@pytest.mark.parametrize("name", SCENES)
def test_scene_in_one_call(dev, name):
    g = load(name)
    check(g, call(dev, g))


@pytest.mark.parametrize("name", ["plain", "zdrop", "fuzz"])
def test_scene_split_into_two_calls(dev, name):
    g = load(name)
    n = len(g["seq_off"]) - 1
    for part in ((0, n // 2), (n // 2, n)):
        check(g, call(dev, g, part), part)


def test_no_reads_and_no_regions(dev):
    g = load("plain")
    from minimap2_chaindp_amd import chaindp
    z64 = np.zeros(1, np.int64)
    a, regs, regs2, extra, off, cig = dev.align1(opt_of(g), z64, b"", z64, np.zeros((0, 2), np.uint64), z64, np.zeros(0, chaindp.REG_DTYPE))
    assert len(regs) == 0 and off.tolist() == [0] and len(cig) == 0
    # reads without regions
    n = len(g["seq_off"]) - 1
    got = dev.align1(opt_of(g), g["seq_off"], g["seq"], g["a_off"], g["a"], np.zeros(n + 1, np.int64), np.zeros(0, chaindp.REG_DTYPE))
    assert got[4].tolist() == [0] and np.array_equal(got[0], g["a"])


def test_cnt0_region_is_left_alone(dev):
    g = load("plain")
    (i,) = np.flatnonzero(g["regs"]["cnt"] == 0)
    regs2 = np.zeros(len(g["regs"]), S.REG_DTYPE)
    regs2["score"] = 77; regs2["cnt"] = 5                      # only cnt is written where nothing is split off
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    a, regs, r2, extra, off, cig = dev.align1(opt_of(g), g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"], regs2=regs2)
    assert regs[i] == g["regs"][i] and r2["cnt"][i] == 0 and r2["score"][i] == 77 and extra[i].tolist() == (0, 0, 0, 0, 0)
    assert (r2["cnt"] == 0).all() and (r2["score"] == 77).all()


def test_small_cigar_cap_is_capacity_with_the_rest_filled(dev):
    from minimap2_chaindp_amd import chaindp
    g = load("zdrop")
    total = int(g["cigar_off"][-1])
    with pytest.raises(chaindp.ChainDPError, match="CIGAR words") as e:
        call(dev, g, cigar_cap=total - 1)
    err = e.value
    assert np.array_equal(err.cigar_off, g["cigar_off"]) and np.array_equal(err.a, g["a_out"])
    for x, want in ((err.regs, g["regs_out"]), (err.regs2, g["regs2"]), (err.extra, g["extra"])):
        assert np.array_equal(words(x), words(want))
    check(g, call(dev, g, cigar_cap=total))                    # the exact room is enough, and the context is usable
    check(g, call(dev, g))                                     # ... and so is the front end's guess, with its retry


def test_refusals_leave_the_context_usable(dev):
    from minimap2_chaindp_amd import chaindp, params
    g = load("plain")
    for change in (dict(flag=params.MM_F_SR), dict(flag=params.MM_F_SPLICE), dict(q2=4, e2=2), dict(a=128)):
        o = opt_of(g)
        for k, v in change.items():
            setattr(o, k, v)
        dev.align_set_targets(g["tseq_off"], g["tseq"])
        with pytest.raises(chaindp.ChainDPError):
            dev.align1(o, g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"])
    dev.align_clear_targets()
    with pytest.raises(chaindp.ChainDPError, match="target"):
        dev.align1(opt_of(g), g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"])
    check(g, call(dev, g))


def test_ksw_extd_still_passes_on_the_same_context(dev):
    import test_gpu_ksw as T
    g = load("fuzz")
    check(g, call(dev, g))
    for name in T.NAMED[:2] + T.FUZZ[:1]:
        k = T.load(name)
        ez, off, cig = T.call(dev, k)
        T.check(k, ez, off, cig)
        assert np.array_equal(dev.ksw_route(len(ez)), T.expected_routes(k))
    check(g, call(dev, g))
