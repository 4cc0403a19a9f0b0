"""CPU tier: the per-read-gap shapes (tests/gap_shapes.py) and scenario (tests/gap_model.py) do what they claim, and chaindp_read_gaps
equals map.c:358-366.  No GPU: the oracle, the compiled reference where it is built, and the library's host-only helper."""
import numpy as np
import pytest

import gap_model as gm
import gap_shapes as gs
import oracle_lib as ol
from minimap2_chaindp_amd import params as P


@pytest.mark.parametrize("name", gs.NAMES)
def test_shape_bites_either_way(name):
    """Every read taking the gaps of the read behind it, or of the read before it, changes f, p or v of at least one read: a GPU pass
    cannot come from a wrong index.  With one pair for all reads the per-read loop is the batch oracle."""
    sh, exp = gs.shape_with_expected(name)
    assert len(sh.gap_ref) == len(sh.off) - 1 and sh.off[-1] == len(sh.a) <= 4000
    for k in (1, -1):
        other = gs.expected(sh, *gs.neighbours(sh, k))
        changed = [r for r in range(len(sh.off) - 1)
                   if any(not np.array_equal(x[sh.off[r]:sh.off[r + 1]], y[sh.off[r]:sh.off[r + 1]]) for x, y in zip(exp[:3], other[:3]))]
        assert changed, (name, k)
    uni = P.ChainParams(*sh.par.astuple())
    uni.max_dist_x, uni.max_dist_y = 300, 400
    n = len(sh.off) - 1
    f, p, v, _ = ol.oracle_batch(uni, sh.off, sh.a, sh.n_segs)
    e = gs.expected(sh, np.full(n, 300), np.full(n, 400))
    assert np.array_equal(f, e[0]) and np.array_equal(p, e[1]) and np.array_equal(v, e[2])


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref is not built")
@pytest.mark.parametrize("name", gs.NAMES)
def test_shape_expectations_equal_the_compiled_reference(name):
    sh, exp = gs.shape_with_expected(name)
    ref = gs.expected(sh, use_ref=True)
    for x, y in zip(exp[:4], ref[:4]):
        assert np.array_equal(x, y), name
    assert exp[4].tobytes() == ref[4].tobytes(), name


def test_cut_edge_cuts_where_it_says():
    sh, (f, p, v, soff, seeds) = gs.shape_with_expected("cut_edge")
    for i, g in enumerate(gs.CUT_GAPS):
        for j, own in enumerate((g, g + 1, g - 1, g + 1, g)):
            r = 5 * i + j
            pr = p[sh.off[r]:sh.off[r + 1]]
            steps = np.array([g, g + 1, g, g + 1, g, g, g + 1])
            assert np.array_equal(pr[1:] >= 0, steps <= own), (g, own, pr)


def test_singletons_and_emitted_singletons_depend_on_the_gap():
    sh, (f, p, v, soff, seeds) = gs.shape_with_expected("singletons")
    lone_alone, lone_unit = p[sh.off[0]:sh.off[1]], p[sh.off[1]:sh.off[2]]
    assert (lone_alone == -1).all() and (lone_unit[1:] >= 0).all()
    assert soff[1] - soff[0] == 5                                    # alone: only the anchors with q_span 30 >= min_sc are emitted
    assert sh.off[6] == sh.off[5]                                    # the empty read


def test_the_deep_unit_scans_past_the_ring():
    sh, (f, p, v, soff, seeds) = gs.shape_with_expected("variants")
    r = 4
    pr = p[sh.off[r]:sh.off[r + 1]]
    i = np.arange(gs.DEEP_LEN)
    assert len(pr) == gs.DEEP_LEN and (pr[:200] == -1).all() and (pr[300:] >= 0).all()
    assert ((i - pr)[pr >= 0] >= 200).all() and ((i - pr)[pr >= 0] <= 300).all()      # every predecessor lies beyond a ring of 128


def test_the_gap_header_is_part_of_the_abi():
    """include/chaindp_gaps.h declares exactly the two gap functions, chaindp.h includes it, the library exports both and the front end
    binds them with the header's parameter counts."""
    import os
    import subprocess
    from minimap2_chaindp_amd import _cabi, chaindp
    assert chaindp.GAPS_SYMBOLS == ("chaindp_read_gaps", "chaindp_set_read_gaps")
    with open(os.path.join(_cabi.INCLUDE, "chaindp.h")) as fh:
        assert '#include "chaindp_gaps.h"' in fh.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", chaindp.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    L = chaindp.lib()
    for name, n in zip(chaindp.GAPS_SYMBOLS, (8, 4)):
        assert f" T {name}\n" in nm and len(getattr(L, name).argtypes) == n
    assert L.chaindp_read_gaps.restype is None


def test_read_gaps_equals_the_reference_lines():
    """map.c:358-366 restated in Python against chaindp_read_gaps: qlen_sum around max_gap, max_frag_len - qlen_sum around max_gap,
    max_gap_ref set, max_frag_len = 0, is_sr = 0."""
    mg, mfl = 100, 800
    q = np.array([1, mg - 1, mg, mg + 1, 300, mfl - mg - 1, mfl - mg, mfl - mg + 1, mfl, mfl + 50, 60, 299], np.int32)
    for max_gap, max_gap_ref, max_frag_len, is_sr in ((mg, -1, mfl, 1), (mg, 0, mfl, 1), (mg, 650, mfl, 1), (mg, -1, 0, 1), (mg, -1, mfl, 0),
                                                      (mg, 650, 0, 0), (5000, -1, 0, 0), (mg, 1, mfl, 1)):
        gr, gq = P.read_gaps(max_gap, max_gap_ref, max_frag_len, is_sr, q)
        er, eq = gm.gaps_py(max_gap, max_gap_ref, max_frag_len, is_sr, q)
        assert np.array_equal(gr, er) and np.array_equal(gq, eq), (max_gap, max_gap_ref, max_frag_len, is_sr)
    gr, gq = P.read_gaps(mg, -1, mfl, 1, q)
    assert gq[1:4].tolist() == [mg, mg, mg + 1] and gr[5:8].tolist() == [mg + 1, mg, mg]
    gr, gq = P.read_gaps(mg, -1, mfl, 1, np.zeros(0, np.int32))
    assert len(gr) == len(gq) == 0


def test_scenario_has_many_gap_pairs_and_depends_on_them():
    """What makes the end-to-end GPU test bite: at least 300 pairs-or-orphans with at least 100 distinct gap pairs, and at least a
    tenth of the reads end with other hits under each of three uniform settings (500 / 300, the batch's largest pair, its smallest)."""
    sc, m = gm.scenario_with_model()
    n = len(sc.frags)
    assert n >= 300 and len(gm.groups(sc)) >= 100
    lens = [len(s) for f in sc.frags for s in f if len(s)]
    assert min(lens) >= 30 and max(lens) <= 150
    assert any(len(f) == 1 for f in sc.frags) and any(len(f) == 2 and not len(f[1]) for f in sc.frags)
    assert m.seg_regs_off[-1] > n // 2
    img = sc.image()
    ix = ol.SeedIndex(img)
    try:
        for gr, gq in ((500, 300), (int(sc.gaps[0].max()), int(sc.gaps[1].max())), (int(sc.gaps[0].min()), int(sc.gaps[1].min()))):
            d = gm.reads_that_differ(m, gm.model_of(sc, gm.uniform(sc, gr, gq), img=ix))
            print(f"uniform {gr}/{gq}: {len(d)} of {n} reads differ")
            assert len(d) * 10 >= n, (gr, gq, len(d))
    finally:
        ix.close()
