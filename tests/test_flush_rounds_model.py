"""CPU tier: the tile flush's v[] loop with its early exit (tests/flush_model.py) against the oracle's v, tile by tile, on the five
seeded batches whose round counts motivated the exit and on hand-built units that need the late rounds.  The kernels' loops
(chaindp_twin.hip, fast_flush_tile in chaindp_fast.h) are this loop; test_gpu_flush_early_exit.py runs the same
inputs through them.

What the data say (units of two anchors and more: a single anchor is settled without a flush), tiles by rounds started 0 .. 5:

    ava-ont, 200 reads                     246, 21 189,   830,     1,  0, 0    of 22 266 tiles
    ava-ont noise 40 %, ties 20 %        2 498,  8 535, 6 666,    23,  0, 0    of 17 722
    skew up to 30 000                      197, 10 676,   407,     0,  0, 0    of 11 280
    map-ont, 60 reads                        7,  1 206, 2 581,   346, 14, 0    of  4 154
    ties, map-ont parameters               126,    983, 6 576, 2 313, 79, 1    of 10 078

against 5.6, 4.9, 5.6, 5.9 and 4.3 rounds a tile when the loop stops only once every pointer has left the tile."""
import numpy as np
import pytest

import flush_model as fm
import oracle_lib as ol

TABLE = [  # tiles by rounds started 0 .. 6 (units of >= 2 anchors), per seeded batch
    [246, 21189, 830, 1, 0, 0, 0],
    [2498, 8535, 6666, 23, 0, 0, 0],
    [197, 10676, 407, 0, 0, 0, 0],
    [7, 1206, 2581, 346, 14, 0, 0],
    [126, 983, 6576, 2313, 79, 1, 0],
]


def _run(par, off, a):
    f, p, v, _ = ol.oracle_batch(par, off, a, threads=8)
    mv, st = fm.flush_v(par, off, a, f, p)
    return f, p, v, mv, st


@pytest.fixture(scope="module")
def results():
    return [_run(*fm.seeded(i)) for i in range(len(fm.SEEDED))] + [_run(*fm.built())]


def _rounds_without_exit(par, off, a, p, st):
    """Rounds per tile of the loop that stops only when no pointer is inside the tile: the r-th round runs while some lane has an
    r-th... 2^(r-1)-th ancestor inside the tile, so a tile runs 1 + floor(log2(longest in-tile ancestor path)) rounds."""
    n = int(off[-1])
    idx = np.arange(n, dtype=np.int64)
    read_of = np.searchsorted(off, idx, side="right") - 1
    gp = np.where(p >= 0, p.astype(np.int64) + off[read_of], -1)
    first_lane = np.flatnonzero(np.r_[True, st["tile_of"][1:] != st["tile_of"][:-1]])
    tstart = first_lane[st["tile_of"]]
    depth = np.zeros(n, np.int64)                                         # ancestors inside the tile
    for i in range(fm.TILE):                                              # lane by lane in tile order: the predecessor's depth is final
        lanes = first_lane + i
        lanes = lanes[(lanes < n)]
        lanes = lanes[st["tile_of"][lanes] == st["tile_of"][lanes - i]]
        inside = gp[lanes] >= tstart[lanes]
        depth[lanes[inside]] = depth[gp[lanes[inside]]] + 1
    deepest = np.zeros(len(first_lane), np.int64)
    np.maximum.at(deepest, st["tile_of"], depth)
    return np.where(deepest > 0, 1 + np.floor(np.log2(np.maximum(deepest, 1))).astype(np.int64), 0)


@pytest.mark.parametrize("i", range(len(fm.SEEDED) + 1), ids=[s[0] + "-" + s[2] + "-" + str(s[3]) for s in fm.SEEDED] + ["built"])
def test_v_with_the_exit_is_the_oracles_v(results, i):
    _, _, v, mv, st = results[i]
    bad = np.flatnonzero(mv != v)
    assert bad.size == 0, ("first wrong anchor", int(bad[0]), "tile", int(st["tile_of"][bad[0]]), int(mv[bad[0]]), int(v[bad[0]]))


@pytest.mark.parametrize("i", range(len(fm.SEEDED)))
def test_rounds_of_the_seeded_batches(results, i):
    """The round counts the change rests on: nearly every tile of the flagship's shape is quiet in its first round."""
    f, p, _, _, st = results[i]
    keep = st["unit_len"] >= 2
    assert np.bincount(st["rounds"][keep], minlength=7).tolist() == TABLE[i]
    par, off, a = fm.seeded(i)
    before = _rounds_without_exit(par, off, a, p, st)[keep]
    print(f"{fm.SEEDED[i]}: {int(keep.sum())} tiles, {before.mean():.2f} rounds a tile without the exit, {st['rounds'][keep].mean():.2f} with it")
    assert (before >= st["rounds"][keep] - 1).all()                         # the exit costs at most the round that finds it
    assert before.mean() > 4.2 and st["rounds"][keep].mean() < 2.2


def test_inputs_reach_what_can_go_wrong(results):
    rounds = np.concatenate([r[4]["rounds"] for r in results])
    way = np.concatenate([r[4]["way"] for r in results])
    anchors = np.concatenate([r[4]["anchors"] for r in results])
    ext_above = np.concatenate([r[4]["ext_above"] for r in results])
    for r in range(1, 7):
        assert ((way == "quiet") & (rounds == r)).any(), f"no tile leaves by the new exit in round {r}"
    assert ((way == "none") & (rounds == 0)).any()                          # no pointer inside the tile at all
    assert ((way == "none") & (rounds > 0)).any()                           # ... the last of them left after a round
    assert ((way == "count") & (rounds == 6)).any()                         # the sixth round still raised a value
    assert ext_above.any()                                                  # a predecessor in an earlier tile whose v exceeds the lane's f
    assert (ext_above & (rounds > 0)).any()
    assert (anchors < fm.TILE).any() and (anchors == fm.TILE).any()
    assert set(way) == {"none", "quiet", "count"}


def test_built_units_need_the_late_rounds(results):
    """Rounds 4 to 6 are rare in the seeded batches (93 tiles, 1 tile, none): the built units supply them, and the oracle confirms
    the construction: one chain per read, f falls once behind the peak, every anchor behind the peak has the peak's f as its v."""
    par, off, a = fm.built()
    f, p, v, mv, st = results[-1]
    quiet = {int(r) for r, w in zip(st["rounds"], st["way"]) if w == "quiet"}
    assert {4, 5, 6} <= quiet, quiet
    assert ((st["way"] == "count") & (st["rounds"] == 6)).sum() >= 2
    assert st["ext_above"].sum() >= 2
    for r in range(len(off) - 1):
        lo, hi = int(off[r]), int(off[r + 1])
        assert p[lo] == -1 and (p[lo + 1:hi] == np.arange(hi - lo - 1)).all()      # one chain, each anchor on the one before it
        peak = lo + int(np.argmax(f[lo:hi]))
        assert (np.diff(f[lo:peak + 1]) == 15).all() and f[peak + 1] < f[peak] - 50 and (np.diff(f[peak + 1:hi]) == 1).all()
        assert f[hi - 1] < f[peak] and (v[peak:hi] == f[peak]).all() and (v[lo:peak] == f[lo:peak]).all()
