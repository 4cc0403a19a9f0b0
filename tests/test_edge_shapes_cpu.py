"""CPU tier: every input of tests/edge_shapes.py sits on the edge it claims -- proved with the oracle (records, chain ends and
kept chains per read, the cost table's last entry, which pairs chain, unit counts and lengths, tile and block positions), and
for the table-driven single-segment cases the wave model (ring 128) equals the oracle.  No edge is skipped: a constructor that
cannot reach its edge raises.  The only have_ref() branch compares the oracle's chains with the reference's where it is built."""
import numpy as np
import pytest

import edge_shapes as es
import oracle_lib as ol


def oracle_results(par, off, a, min_cnt=None):
    """What the GPU path must return for the batch: f, p, v; per read new_seed[] (seeds, soff); with min_cnt the chains too
    (u, b per read and their offsets coff, boff)."""
    f, p, v, _ = ol.oracle_batch(par, off, a, threads=8)
    n = len(off) - 1
    seeds, u, b = [], [], []
    for r in range(n):
        lo, hi = int(off[r]), int(off[r + 1])
        s = ol.oracle_compact(par, np.ascontiguousarray(a[lo:hi]), f[lo:hi].copy(), p[lo:hi].copy(), v[lo:hi].copy())
        seeds.append(s)
        if min_cnt is not None:
            uu, bb = ol.oracle_bottom(min_cnt, par.min_sc, s)
            u.append(uu); b.append(bb.reshape(-1, 2))
    out = dict(f=f, p=p, v=v, seeds=seeds, soff=np.concatenate(([0], np.cumsum([len(s) for s in seeds]))).astype(np.int64))
    if min_cnt is not None:
        out.update(u=u, b=b, coff=np.concatenate(([0], np.cumsum([len(x) for x in u]))).astype(np.int64),
                   boff=np.concatenate(([0], np.cumsum([len(x) for x in b]))).astype(np.int64))
    return out


def chain_ends(seeds):
    """chain.c:346-354: records with the v >= min_sc flag that no record points at."""
    has = np.zeros(len(seeds), bool)
    pp = seeds["p"]
    has[pp[pp >= 0] >> 2] = True
    return int(((pp & 1) == 1)[~has].sum())


def assert_model_equals_oracle(par, off, a, exp, what):
    mf, mp, mv, st = ol.wave_model_batch(par, off, a, ring=128)
    for name, x, y in (("f", mf, exp["f"]), ("p", mp, exp["p"]), ("v", mv, exp["v"])):
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (what, name, int(bad[0]))
    return st


def assert_bt_read(a, seeds, u, b, props, par, min_cnt, what):
    assert len(seeds) == len(a) == props["records"], (what, "every anchor is a record")
    assert chain_ends(seeds) == props["ends"], (what, "ends", chain_ends(seeds))
    assert len(u) == props["kept"], (what, "kept", len(u))
    # a kept chain that stopped at an older one scores its peak's f minus the f of the record it stopped at
    first = np.concatenate(([0], np.cumsum((u & np.uint64(0xffffffff)).astype(np.int64))))
    key = {(int(s["x"]), int(s["y"])): int(s["f"]) for s in seeds}
    below = [i for i in range(len(u)) if int(u[i] >> np.uint64(32)) < key[tuple(int(t) for t in b[first[i + 1] - 1])]]
    assert len(below) >= 1, (what, "no kept chain stopped at an older one")
    u_all, _ = ol.oracle_bottom(min_cnt, -(1 << 30), seeds)
    assert len(u_all) - len(u) == 1, (what, "chains dropped by the min_sc rule", len(u_all) - len(u))
    x_first = b[first[:-1], 0]
    assert np.bincount(np.unique(x_first, return_inverse=True)[1]).max() >= props["shared_first_x"] >= 2, (what, "kept chains sharing their first x")
    if ol.have_ref():
        ru, rb = ol.ref_bottom(min_cnt, par.min_sc, 1, seeds)
        assert np.array_equal(u, ru) and np.array_equal(b, rb.reshape(-1, 2)), (what, "reference")


# ---------------------------------------------------------------- backtracker

def test_backtracker_edges_cover_every_regime():
    regimes = {(lo, k): 0 for lo in (0, 1, 2) for k in (64, 65)}
    for rec, ends, kept in es.BT_EDGES:
        regimes[(0 if rec <= es.BT_LDS_RECS else 1 if rec <= es.BT_LDS_RECS_MAX else 2, kept)] += 1
    assert all(regimes.values()), regimes
    assert {256, 257, 1024, 1025} <= {e for _, e, _ in es.BT_EDGES}
    assert {es.BT_LDS_RECS, es.BT_LDS_RECS + 1, es.BT_LDS_RECS_MAX, es.BT_LDS_RECS_MAX + 1} <= {r for r, _, _ in es.BT_EDGES}
    assert es.BT_INSERTION_MAX == 64
    # (records, ends, kept) on both sides of each constant at once; the read without one-anchor runs has 65 ends, not 64: the
    # fork's dropped branch is an end too
    assert {(10112, 256, 64), (10113, 257, 65), (20000, 1025, 64), (20001, 1025, 65), (20001, 65, 64), (700, 256, 65)} <= set(es.BT_EDGES)


def test_backtracker_single_reads():
    for (par, off, a, min_cnt), props in es.bt_single_reads():
        exp = oracle_results(par, off, a, min_cnt)
        assert_bt_read(a, exp["seeds"][0], exp["u"][0], exp["b"][0], props, par, min_cnt, props)


def test_fork_chains():
    """The forks by themselves: chains (501, 55) and (19, 25); the second branch of 8 anchors is dropped."""
    par = es.bt_par()
    for n_branch, chains in ((es.FORK_KEPT, [(501, 55), (19, 25)]), (es.FORK_DROPPED, [(501, 55)])):
        a = es.sort_read(es._fork(1000, 1000, n_branch))
        exp = oracle_results(par, np.array([0, len(a)], np.int64), a, es.BT_MIN_CNT)
        got = sorted(((int(x >> np.uint64(32)), int(x & np.uint64(0xffffffff))) for x in exp["u"][0]), reverse=True)
        assert got == chains, (n_branch, got)
        assert chain_ends(exp["seeds"][0]) == 2


def test_backtracker_combined_batch():
    (par, off, a, min_cnt), props = es.bt_combined()
    exp = oracle_results(par, off, a, min_cnt)
    n = len(off) - 1
    rec = np.diff(exp["soff"])
    assert list(rec) == props["records"]
    assert off[1] == 0 and rec[0] == 0, "an empty read first"
    i, j = props["empty_middle"]
    assert j == i + 1 and off[i] == off[i + 1] == off[j + 1] and 0 < i < n - 3, "two empty reads in the middle"
    nr = props["norec_read"]
    assert off[nr + 1] - off[nr] > 0 and rec[nr] == 0, "anchors without a record"
    assert off[n - 2] == off[n - 1] == off[n] and rec[n - 1] == 0 and rec[n - 2] == 0, "two empty reads last"
    ar = props["aligned_read"]
    assert exp["soff"][ar] % es.BLOCK == 0 and exp["soff"][ar] > 0 and rec[ar] > 0, "a read whose first record opens a block"
    blk = int(exp["soff"][ar]) // es.BLOCK
    inside = [r for r in range(n) if exp["soff"][r] // es.BLOCK == blk and exp["soff"][r] < (blk + 1) * es.BLOCK and r >= ar]
    assert len([r for r in inside if rec[r] > 0]) >= 3 and any(rec[r] == 0 for r in inside[:-1]), "a block over three reads and an empty one"
    assert len(props["edge_at"]) == len(es.BT_EDGES)
    for r, e in props["edge_at"].items():
        records, ends, kept = es.BT_EDGES[e]
        assert rec[r] == records and chain_ends(exp["seeds"][r]) == ends and len(exp["u"][r]) == kept, (r, es.BT_EDGES[e])
    regimes = {0 if m <= es.BT_LDS_RECS else 1 if m <= es.BT_LDS_RECS_MAX else 2 for m in rec if m}
    assert regimes == {0, 1, 2}, "all three record regimes in one call"


# ---------------------------------------------------------------- DP routing

def test_int8_fit_batches():
    for name, ((par, off, a), props) in es.int8_batches().items():
        assert par.bw == 500
        for r, fit in enumerate(props["fits"]):
            spans = (a[int(off[r]):int(off[r + 1]), 1] >> np.uint64(32)).astype(np.int64)
            assert es.lut_last_entry(par.bw, spans) == props["last_entry"][r] == (-128 if fit else -129), (name, r)
            assert (spans.mean() == 25.0) == fit
        lens, _ = es.unit_lengths(par, off, a)
        assert (lens >= 2).all() and (lens <= 60).all() and len(lens) == sum(props["units"])
        exp = oracle_results(par, off, a)
        st = assert_model_equals_oracle(par, off, a, exp, name)
        assert st["units"] == sum(props["units"]) and st["singletons"] == 0 and st["deep_chunks"] == 0
    b = es.int8_batches()
    assert b["fit"][1]["units_nofit"] == 0 and b["nofit"][1]["units_nofit"] == sum(b["nofit"][1]["units"])
    assert 0 < b["mixed"][1]["units_nofit"] < sum(b["mixed"][1]["units"])


BW_CASES = [(511, 15, 20), (512, 15, 20), (4095, 255, 60), (4096, 255, 60)]


@pytest.mark.parametrize("bw,span,run", BW_CASES)
def test_bw_pairs_chain_at_bw_and_not_above(bw, span, run):
    (par, off, a), props = es.bw_batch(bw, span, run)
    assert par.bw == bw and {511, 512} == {es.TWIN_LUT_BYTES - 1, es.TWIN_LUT_BYTES} and {4095, 4096} == {es.LUT_MAX_BW, es.LUT_MAX_BW + 1}
    exp = oracle_results(par, off, a)
    for j in props["jumps"]:
        i, pr = j["anchor"], j["pred"]
        dr = int(a[i, 0]) - int(a[pr, 0])
        dq = int(a[i, 1] & np.uint64(0xffffffff)) - int(a[pr, 1] & np.uint64(0xffffffff))
        assert abs(dr - dq) == j["dd"] and j["dd"] in (bw, bw + 1)
        assert exp["p"][i] == (pr if j["dd"] == bw else -1), (bw, j, int(exp["p"][i]))
    if bw >= 4095:
        assert int((a[:, 1] >> np.uint64(32)).max()) == 255
    if bw <= es.LUT_MAX_BW:
        st = assert_model_equals_oracle(par, off, a, exp, bw)
        assert st["units"] - st["singletons"] == props["units"]


def test_max_dist_x_bounds_are_computed():
    for factor, bits in ((129, 31), (129, 32), (257, 32), (513, 32), (1025, 32)):
        m = es.largest_mdx(factor, bits)
        assert (m + 1) * factor < (1 << bits) <= (m + 2) * factor, (factor, bits)
    assert es.largest_mdx(129, 31) == 16647159                      # (2^31 - 1) // 129 - 1


@pytest.mark.parametrize("above", [0, 1])
def test_twin_max_dist_x_batch(above):
    mdx = es.largest_mdx(129, 31) + above
    (par, off, a), props = es.mdx_twin_batch(mdx)
    assert ((par.max_dist_x + 1) * 129 < (1 << 31)) == (above == 0)
    lens, pos = es.unit_lengths(par, off, a)
    assert list(lens[:2]) == props["first_units"] and int((lens >= 2).sum()) == props["units"]
    gaps = np.diff(a[:lens[0], 0].astype(np.int64))
    assert (gaps == mdx).sum() >= 20 and (gaps == mdx - 1).sum() >= 20 and (gaps < 10).sum() >= 20 and gaps.max() == mdx
    assert int(a[lens[0], 0]) - int(a[lens[0] - 1, 0]) == mdx + 1
    exp = oracle_results(par, off, a)
    big = np.flatnonzero(gaps >= mdx - 1) + 1
    assert (exp["p"][big] == big - 1).all(), "pairs chain across the large gaps"
    assert exp["p"][lens[0]] == -1
    assert_model_equals_oracle(par, off, a, exp, mdx)


@pytest.mark.parametrize("above", [0, 1])
@pytest.mark.parametrize("ring,dense_head", [(128, 0), (256, 0), (512, 0), (512, 1500), (1024, 1500)])
def test_ring_max_dist_x_batch(ring, dense_head, above):
    mdx = es.largest_mdx(ring + 1, 32) + above
    (par, off, a), props = es.mdx_ring_batch(mdx, ring, dense_head)
    assert ((par.max_dist_x + 1) * (ring + 1) < (1 << 32)) == (above == 0)
    lens, _ = es.unit_lengths(par, off, a)
    assert list(lens) == props["unit_lens"]
    gaps = np.diff(a[:lens[0], 0].astype(np.int64))
    run = max(len(s) for s in "".join("g" if g >= mdx - 1 else " " for g in gaps).split())
    assert run >= ring + 7 and gaps.max() == mdx and (gaps == mdx - 1).any(), "the ring spans ring + 1 gaps of max_dist_x"
    assert int(a[lens[0], 0]) - int(a[lens[0] - 1, 0]) == mdx + 1
    assert a[0, 0] < (1 << 32) <= a[lens[0] - 1, 0]
    exp = oracle_results(par, off, a)
    assert (exp["p"][dense_head:] >= 0).sum() > 100, "the clusters chain inside"
    _, _, _, st = ol.wave_model_batch(par, off, a, ring=128)
    assert st["deep_chunks"] >= 20 * bool(dense_head), "the head's scans run past the ring"


def test_short_units_batches():
    b = es.short_units_batches()
    for name, ((par, off, a), props) in b.items():
        lens, _ = es.unit_lengths(par, off, a)
        assert int((lens >= 2).sum()) == props["units"] and int((lens == 1).sum()) == props["singletons"]
        st = assert_model_equals_oracle(par, off, a, oracle_results(par, off, a), name)
        assert st["units"] - st["singletons"] == props["units"] and st["singletons"] == props["singletons"]
        assert len(a) - props["singletons"] == es.SHORT_UNIT_AVG * props["units"] + (name == "above")


@pytest.mark.parametrize("n", [es.DENSE_BITCAP, es.DENSE_BITCAP + 1])
def test_dense_bitmap_units(n):
    (par, off, a), props = es.dense_bitmap_batch(n)
    assert props["unit_lens"] == [n] and par.max_dist_x == 1000
    x = a[:, 0].astype(np.int64)
    window = np.arange(n) - np.searchsorted(x, x - par.max_dist_x, side="left")
    assert np.median(window) >= 150 and (window > 128).sum() > n - 1000
    exp = oracle_results(par, off, a)
    assert 12 <= (exp["p"] < 0).sum() < 20, "all but the first anchors of the twelve q offsets chain"
    _, _, _, st = ol.wave_model_batch(par, off, a, ring=128)
    assert st["deep_chunks"] > n // 2 and st["units"] == 1


@pytest.mark.parametrize("n_units,unit_len,per_read", [(2200, 320, 11), (es.DENSE16_MAX_UNITS, 2400, 8), (es.DENSE16_MAX_UNITS + 1, 2400, 8)])
def test_dense_unit_batches(n_units, unit_len, per_read):
    (par, off, a), props = es.dense_units_batch(n_units, unit_len, per_read)
    assert n_units > es.DENSE_UNITS or unit_len > es.DEEP_HANDOVER_LEFT
    lens, _ = es.unit_lengths(par, off, a)
    assert len(lens) == n_units and (lens == unit_len).all()
    k = 2 * per_read                                            # the model on the first two reads: every unit has deep scans
    _, _, _, st = ol.wave_model_batch(par, off[:3], a[:int(off[2])], ring=128)
    assert st["units"] == k and st["deep_chunks"] >= k * (unit_len // 64 - 3)


# ---------------------------------------------------------------- alignment

@pytest.mark.parametrize("block_multiple", [False, True])
def test_confetti_batches(block_multiple):
    (par, off, a, min_cnt), props = es.confetti_batch(block_multiple)
    ln = np.diff(off)
    assert props["n_reads"] == len(ln) >= 3000 and (ln <= 3).sum() >= 3000
    assert all(c > 0 for c in props["starts_lane"].values()) and all(c > 0 for c in props["starts_block"].values()), props
    assert all(c > 0 for c in props["one_anchor"].values()), props["one_anchor"]
    assert props["max_boundaries_in_tile"] >= 20 and props["max_reads_in_block"] >= 300 and props["longest_empty_run"] >= 70
    assert props["mid_reads"] >= 2 and props["long_reads"] >= 2
    if block_multiple:
        assert off[-1] % es.BLOCK == 0
    else:
        assert off[-1] % es.TILE == 1 and ln[-1] == 1
    # the places, again from off[] alone
    st = off[:-1]
    for m in (0, 1, 63):
        assert ((st % es.TILE == m) & (ln > 0)).any()
    assert ((st % es.BLOCK == 0) & (ln == 1)).any() and ((st % es.BLOCK == es.BLOCK - 1) & (ln == 1)).any()
    assert ((st % es.TILE == 0) & (ln == 1)).any() and ((st % es.TILE == 63) & (ln == 1)).any()
    exp = oracle_results(par, off, a, min_cnt)
    stt = assert_model_equals_oracle(par, off, a, exp, "confetti")
    assert stt["singletons"] > 500 and stt["units"] - stt["singletons"] > 500
    assert (np.diff(exp["soff"]) == 0).sum() >= 70 and exp["coff"][-1] > 1000


def test_adjacent_reads_batch():
    (par, off, a, min_cnt), props = es.adjacent_reads_batch()
    lens, pos = es.unit_lengths(par, off, a)
    assert list(lens) == props["unit_lens"] and list(pos) == [0, 40, 70, 140]
    assert 0 < int(a[off[1], 0]) - int(a[off[1] - 1, 0]) <= par.max_dist_x
    assert a[off[2], 0] < a[off[2] - 1, 0]
    assert 0 < int(a[off[4], 0]) - int(a[off[4] - 1, 0]) <= par.max_dist_x and off[3] == off[4]
    exp = oracle_results(par, off, a, min_cnt)
    assert all(exp["p"][off[r]] == -1 for r in (0, 1, 2, 4))
    whole = ol.oracle_fpv(par, np.ascontiguousarray(a[:70]))[1]
    assert whole[40] == 39, "reads 0 and 1 would chain as one read"
    assert_model_equals_oracle(par, off, a, exp, "adjacent")


def test_unit_lengths_batch():
    (par, off, a, min_cnt), props = es.unit_lengths_batch()
    lens, pos = es.unit_lengths(par, off, a)
    at = dict(zip(pos.tolist(), lens.tolist()))
    seen = set()
    for g, L in props["placed"]:
        assert at.get(g) == L, (g, L)
        seen.add((L, g % es.TILE))
    assert seen == {(L, lane) for L in es.UNIT_LENGTHS for lane in (0, 63)}
    assert_model_equals_oracle(par, off, a, oracle_results(par, off, a), "unit lengths")
