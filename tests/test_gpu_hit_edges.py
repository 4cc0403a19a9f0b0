"""GPU tier: the inputs of tests/hit_edge_shapes.py (proved to sit on their edges by tests/test_hit_edge_shapes_cpu.py) through the
stages after the chains on the GPU.  A single-segment batch goes through upload, run_full, backtrack and gen_regs (byte for byte
against oracle_gen_regs), est_err (n_match and n_tot exact, div within the project's 2e-6 relative tolerance, unset div exact) and
chain_post with want_anchors (same_records of test_gpu_post.py: every byte but div; the anchors byte for byte).  A fragment batch goes
through frag_post (same_hits of test_gpu_frag.py).  No debug switch: the inputs reach the edges by themselves, alone and concatenated
into one batch so that neighbours of different routes share a launch.  A failure names the edge, the read, the hit and the field."""
import numpy as np
import pytest

import hit_edge_shapes as hs
import oracle_lib as ol
from minimap2_chaindp_amd import chaindp
from test_gpu_frag import same_hits
from test_gpu_post import DIV_RTOL, same_records
from test_hit_edge_shapes_cpu import FRAGS, REF_LEN, SINGLE, _cat, _id, expected_frag, expected_single

pytestmark = pytest.mark.gpu
SINGLE_BATCHES = SINGLE + [("regs_all",), ("post_all",)] + [("post_overlap_all", f) for f in hs.OVERLAP_FLAVOURS]
FRAG_BATCHES = FRAGS + [("frag_all",)]
NO_REGS = np.zeros(0, ol.REG_DTYPE)
NO_ANCHORS = np.zeros((0, 2), np.uint64)


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 22, max_reads=1 << 13) as d:
        yield d


def name_the_field(got, exp, edge, stage, r):
    """The first difference outside div, named: edge, stage, read, hit, field."""
    assert len(got) == len(exp), f"{edge}: {stage}: read {r}: {len(got)} hits, expected {len(exp)}"
    for i in range(len(exp)):
        for k in ol.REG_DTYPE.names:
            if k != "div" and not np.array_equal(got[i][k], exp[i][k]):
                raise AssertionError(f"{edge}: {stage}: read {r}, hit {i}, field {k}: got {got[i][k]}, expected {exp[i][k]}")


def resident_chains(dev, e, n_segs=None):
    sh = e["sh"]
    dev.upload(sh["off"], sh["anchors"], n_segs=n_segs)
    dev.run_full(e["par"])
    coff, u, boff, b = dev.backtrack(e["par"], hs.MIN_CNT if n_segs is None else hs.FRAG_MIN_CNT)
    return coff, u, boff, b


@pytest.mark.parametrize("shape", SINGLE_BATCHES, ids=_id)
def test_single_segment_stages(dev, shape):
    edge = _id(shape)
    e = expected_single(*shape)
    sh = e["sh"]
    n = len(sh["qlen"])
    coff, u, boff, b = resident_chains(dev, e)
    assert np.array_equal(coff, e["coff"]) and np.array_equal(boff, e["boff"]), (edge, "chains per read", np.diff(coff), np.diff(e["coff"]))
    assert np.array_equal(u, _cat(e["u"], np.zeros(0, np.uint64))) and np.array_equal(b, _cat(e["b"], NO_ANCHORS)), (edge, "chains")
    # mm_gen_regs
    regs = dev.gen_regs(e["hash"], sh["qlen"], coff[-1])
    for r in range(n):
        got = regs[coff[r]:coff[r + 1]]
        name_the_field(got, e["regs"][r], edge, "gen_regs", r)
        assert got.tobytes() == e["regs"][r].tobytes(), (edge, "gen_regs", r)
    # mm_est_err on those hits
    got, n_match, n_tot = dev.est_err(coff, regs, sh["qlen"], REF_LEN, sh["mini_pos_off"], sh["mini_pos"])
    for r in range(n):
        s = slice(int(coff[r]), int(coff[r + 1]))
        exp = e["err"][r]
        name_the_field(got[s], exp, edge, "est_err", r)
        for k, g, x in (("n_match", n_match[s], e["n_match"][r]), ("n_tot", n_tot[s], e["n_tot"][r])):
            bad = np.flatnonzero(g != x)
            assert bad.size == 0, f"{edge}: est_err: read {r}, hit {int(bad[0])}, {k}: got {g[bad[0]]}, expected {x[bad[0]]}"
        unset = exp["div"] < 0
        bad = np.flatnonzero(((got[s]["div"] < 0) != unset) | (unset & (got[s]["div"].view(np.uint32) != exp["div"].view(np.uint32))))
        assert bad.size == 0, f"{edge}: est_err: read {r}, hit {int(bad[0]) if bad.size else -1}, field div (unset): got {got[s]['div'][bad[:1]]}"
        bad = np.flatnonzero(~unset & ~np.isclose(got[s]["div"], exp["div"], rtol=DIV_RTOL, atol=0))
        assert bad.size == 0, f"{edge}: est_err: read {r}, hit {int(bad[0]) if bad.size else -1}, field div: got {got[s]['div'][bad[:1]]}, expected {exp['div'][bad[:1]]}"
    # chain_post + mm_est_err + mm_set_mapq (est_err's upload replaced the resident hits: gen_regs puts them back)
    assert dev.gen_regs(e["hash"], sh["qlen"], coff[-1]).tobytes() == regs.tobytes(), (edge, "gen_regs, second call")
    roff, out, aoff, a = dev.chain_post(e["opt"], REF_LEN, qlen=sh["qlen"], rep_len=sh["rep_len"], mini_pos_off=sh["mini_pos_off"],
                                        mini_pos=sh["mini_pos"], want_anchors=True)
    assert np.array_equal(roff, e["roff"]), (edge, "chain_post: final hits per read", np.diff(roff), np.diff(e["roff"]))
    assert np.array_equal(aoff, e["boff"]), (edge, "chain_post: anchor offsets")
    for r in range(n):
        got_r = out[roff[r]:roff[r + 1]]
        name_the_field(got_r, e["post"][r], edge, "chain_post", r)
        same_records(got_r, e["post"][r], (edge, "chain_post", "read", r))
        ga, ea = a[aoff[r]:aoff[r + 1]], e["post_a"][r].reshape(-1, 2)
        bad = np.flatnonzero((ga != ea).any(axis=1))
        assert bad.size == 0, f"{edge}: chain_post: read {r}, anchor {int(bad[0]) if bad.size else -1} of {len(ea)} as chain_post leaves them"


@pytest.mark.parametrize("shape", FRAG_BATCHES, ids=_id)
def test_fragment_stages(dev, shape):
    edge = _id(shape)
    e = expected_frag(*shape)
    sh = e["sh"]
    n = len(sh["qlen"])
    coff, u, boff, b = resident_chains(dev, e, n_segs=sh["n_segs"])
    assert np.array_equal(coff, e["coff"]) and np.array_equal(boff, e["boff"]), (edge, "chains per read", np.diff(coff), np.diff(e["coff"]))
    assert np.array_equal(u, _cat(e["u"], np.zeros(0, np.uint64))) and np.array_equal(b, _cat(e["b"], NO_ANCHORS)), (edge, "chains")
    regs = dev.gen_regs(e["hash"], sh["qlen"], coff[-1])
    for r in range(n):
        got = regs[coff[r]:coff[r + 1]]
        name_the_field(got, e["regs"][r], edge, "gen_regs", r)
        assert got.tobytes() == e["regs"][r].tobytes(), (edge, "gen_regs", r)
    soff, out, aoff, a = dev.frag_post(e["opt"], REF_LEN, sh["n_segs"], seg_len=sh["seg_len"], rep_len=sh["rep_len"], mini_pos_off=sh["mini_pos_off"],
                                       mini_pos=sh["mini_pos"], want_anchors=True)
    assert np.array_equal(soff, e["soff"]), (edge, "frag_post: final hits per segment", np.flatnonzero(np.diff(soff) != np.diff(e["soff"]))[:8])
    first = e["first"]
    for r in range(n):
        for q in range(first[r], first[r + 1]):
            name_the_field(out[soff[q]:soff[q + 1]], e["segs"][q], edge, f"frag_post, segment {q - first[r]}", r)
    same_hits(soff, out, e["soff"], _cat(e["segs"], NO_REGS), sh["n_segs"], (edge, "frag_post"))
    ea = [x for x in e["seg_a"]]
    assert np.array_equal(aoff, np.concatenate(([0], np.cumsum([len(x) for x in ea])))), (edge, "frag_post: anchors per segment")
    for q in range(len(ea)):
        bad = np.flatnonzero((a[aoff[q]:aoff[q + 1]] != ea[q]).any(axis=1))
        assert bad.size == 0, f"{edge}: frag_post: sequence {q}, anchor {int(bad[0]) if bad.size else -1} of {len(ea[q])}"
