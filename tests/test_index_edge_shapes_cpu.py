"""CPU tier: every shape of tests/index_edge_shapes.py is what its name says, judged by the model's route, and the model's image of
it is a well-formed one (every minimizer is found where the format says it lives)."""
import numpy as np
import pytest

import index_build_model as ibm
import index_edge_shapes as ies

SHAPES = ies.shapes()


def test_the_shapes_cover_the_edges():
    names = {s["name"] for s in SHAPES}
    assert {"key_counts_b1", "key_counts_b6", "key_counts_b14", "kick_out_chain", "groups_1_2_257", "empty", "sort_one_digit"} <= names
    assert {f"sort_{n}" for n in (1, ies.TILE - 1, ies.TILE, ies.TILE + 1, 2 * ies.TILE + 1)} <= names
    assert ies.KEY_COUNTS == (1, 3, 4, 6, 7, 12, 13, 16, 17, 25, 26)


@pytest.mark.parametrize("shape", SHAPES, ids=[s["name"] for s in SHAPES])
def test_shape_hits_what_it_names(shape):
    blobs, route = ibm.build(shape["mini"], shape["rank"], shape["b"])
    assert ies.shape_hits(shape, route) == [], route
    assert len(blobs[0]) == 16 << shape["b"]
    # every minimizer is where a lookup goes: home slot, then steps of 1, 2, 3, ...
    occ = ibm.occupied(blobs)
    assert int(occ.sum()) == route["distinct"]
    H, V, P = blobs[1].reshape(-1, 64), blobs[2].view(np.uint64), blobs[3].view(np.uint64)
    tables = {bk: (N, h0, p0) for bk, N, h0, p0 in ibm._tables(blobs)}
    b = shape["b"]
    m_all, cnt = np.unique(shape["mini"][:, 0] >> np.uint64(8), return_counts=True)
    for m, c in zip(m_all.tolist(), cnt.tolist()):
        N, h0, p0 = tables[m & ((1 << b) - 1)]
        i, step = (m >> b) & 0xFFFFFFFF & (N - 1), 0
        while True:
            assert occ[h0 + i]
            key = int.from_bytes(H[(h0 + i) >> 3, 4 + 6 * ((h0 + i) & 7):10 + 6 * ((h0 + i) & 7)].tobytes(), "little")
            if key >> 1 == (m >> b) & ((1 << 47) - 1):
                break
            step += 1
            i = (i + step) & (N - 1)
        assert key & 1 == (c == 1)
        if c > 1:
            assert int(V[h0 + i]) & 0xFFFFFFFF == c and p0 + (int(V[h0 + i]) >> 32) + c <= len(P)
