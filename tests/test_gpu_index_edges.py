"""GPU tier: the index build behind its sketch (chaindp_debug_index_from_minimizers) on the minimizer lists of
tests/index_edge_shapes.py -- every table size around an expansion bound, one home slot for all keys, a kick-out chain, groups of 1, 2
and 257 occurrences, 1, 6 and 14 bucket bits, the empty input, and the sort's tile edges -- against tests/index_build_model.py: the
four blobs byte for byte and the route number for number."""
import numpy as np
import pytest

import index_build_model as ibm
import index_edge_shapes as ies
from minimap2_chaindp_amd import chaindp

pytestmark = pytest.mark.gpu
SHAPES = ies.shapes()


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 10) as d:
        yield d


@pytest.mark.parametrize("shape", SHAPES, ids=[s["name"] for s in SHAPES])
def test_shape_equals_the_model(dev, shape):
    want, route = ibm.build(shape["mini"], shape["rank"], shape["b"])
    assert ies.shape_hits(shape, route) == [], route
    ix = dev.index_from_minimizers(shape["b"], shape["mini"], n_seqs=8, rank=shape["rank"])
    got = dev.index_blobs(ix)
    for n, g, w in zip("BHVP", got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (shape["name"], n)
    got_route = dev.index_route(ix)
    assert got_route["sub_batches"] == 0
    for key in ibm.ROUTE[1:]:
        assert got_route[key] == route[key], (key, got_route, route)
    if route["distinct"]:
        for f in (2e-4, 0.3, 1.0):
            assert dev.index_max_occ(ix, f) == ibm.cal_max_occ(want, f)


def test_input_order_does_not_matter(dev):
    shape = next(s for s in SHAPES if s["name"] == "key_counts_b6")
    want = ibm.build(shape["mini"], shape["rank"], 6)[0]
    for mini in (shape["mini"][::-1], shape["mini"][np.lexsort((shape["mini"][:, 1], shape["mini"][:, 0]))]):
        got = dev.index_blobs(dev.index_from_minimizers(6, mini, rank=shape["rank"]))
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
