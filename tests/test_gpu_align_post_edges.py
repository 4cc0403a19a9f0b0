"""GPU tier of the align-post edges: the scenes of tests/apost_edge_shapes.py (proved to sit on their edges by
tests/test_align_post_edges_cpu.py) through Device.align_post from the host, against the reference's recorded words
(tests/golden/align_post_edges/): every word of the final regions, of what r->p held, dp_max2 and every CIGAR word, exactly.  Each scene
on both routes (the built-in LDS cap and lowered caps), the scenes of one option row in one launch and in reverse order, batches on
both sides of the scan's tile and of the gathers' grid cap, the logf self-test for the match_sc that are no powers of two, and the error
word: what it must refuse, the exact caps it must accept, and what it must not refuse."""
import numpy as np
import pytest

import apost_edge_shapes as E
import apost_model as M
import apost_shapes as PS
import skeleton_model as K
from apost_shapes import BIT_INV, reg
from test_align_post_cpu import inputs, same
from test_gpu_align_post import check, from_host, joined, run_joined, synthetic_blocks

pytestmark = pytest.mark.gpu
GRID_CAP = 65536                        # blocks of k_apost_gather and k_apost_gather_cig
SCAN_TILE = 1024                        # items per tile of the scans


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 17) as d:
        yield d


@pytest.mark.parametrize("name", E.SCENES)
def test_edge_scene_from_the_host_on_both_routes(dev, name):
    # the built-in cap, then caps 1 and 5: every list of at most 48 regions changes its route, the longer ones are on the global route anyway
    for cap in (0, 1, PS.SCENE_CAP):
        assert dev.align_post_set_lds_cap(cap) == PS.AP_LDS_CAP
        try:
            check(*from_host(dev, name), "%s under cap %d" % (name, cap))
        finally:
            dev.align_post_set_lds_cap(0)


def test_scenes_of_one_option_row_in_one_batch_and_in_reverse_order(dev):
    rows = {}
    for name in E.SCENES:
        rows.setdefault(E.load(name)["opt"].tobytes(), []).append(name)
    assert max(len(v) for v in rows.values()) >= 8 and sum(len(v) for v in rows.values()) == len(E.SCENES)
    for names in rows.values():
        opt_row = E.load(names[0])["opt"]
        bs = [b for n in names for b in synthetic_blocks(n)]
        check(joined(bs), run_joined(dev, opt_row, joined(bs)), "joined: " + " ".join(names))
        check(joined(bs[::-1]), run_joined(dev, opt_row, joined(bs[::-1])), "reversed: " + " ".join(names))


def tiled(name, n_reads):
    """The reads of a scene repeated up to n_reads reads, with their recorded outputs: what joined() makes of that many blocks."""
    g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
    whole, rest = divmod(n_reads, len(rep_len))
    tail = joined(synthetic_blocks(name)[:rest]) if rest else None
    full = dict(rep_len=rep_len, regs=regs, extra=extra, cigar=cigar, **{k: g[k] for k in ("regs_out", "extra_out", "dp_max2_out", "cigar_out")})
    out = {k: np.concatenate([np.tile(x, whole)] + ([tail[k]] if rest else [])) for k, x in full.items()}
    for k, off in (("regs_off", regs_off), ("regs_off_out", g["regs_off_out"])):
        out[k] = K.offsets(np.concatenate([np.tile(np.diff(off), whole)] + ([np.diff(tail[k])] if rest else [])))
    out["cigar_off"], out["cigar_off_out"] = K.offsets(out["extra"]["n_cigar"]), K.offsets(out["extra_out"]["n_cigar"])
    return out


@pytest.mark.parametrize("n_reads", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1, GRID_CAP, GRID_CAP + 1])
def test_batches_across_the_scan_tile_and_the_grid_cap(dev, n_reads):
    j = tiled("structure", n_reads)
    assert len(j["rep_len"]) == n_reads == len(j["regs_off"]) - 1 and j["regs_off"][-1] == len(j["regs"]) and j["cigar_off"][-1] == len(j["cigar"])
    if n_reads > GRID_CAP:
        assert len(j["regs"]) > GRID_CAP and len(j["regs_out"]) > GRID_CAP        # both gathers go round their grid-stride loops
    check(j, run_joined(dev, PS.load("structure")["opt"], j), "%d reads" % n_reads)


def test_tiled_is_joined():
    bs = synthetic_blocks("structure")
    want, got = joined((bs * 3)[:len(bs) * 2 + 4]), tiled("structure", len(bs) * 2 + 4)
    assert set(want) == set(got) and all(same(want[k], got[k]) for k in want)


@pytest.mark.parametrize("match_sc", [3, 5, 6])
def test_logf_selftest_where_the_division_is_inexact(dev, match_sc):
    assert dev.apost_logf_selftest(match_sc, 1 << 24) == 0


# ---------------------------------------------------------------- the error word

CAP = 1 << 24
REFUSED = dict(score=lambda: [reg(0, 1000, CAP + 1, has_extra=0)], n_sub=lambda: [reg(0, 1000, 1000, n_sub=CAP)], dp_max=lambda: [reg(0, 1000, 1000, dp_max=CAP + 1)])
ACCEPTED = dict(score=lambda: [reg(0, 1000, CAP, has_extra=0)], n_sub=lambda: [reg(0, 1000, 1000, n_sub=CAP - 1)], dp_max=lambda: [reg(0, 1000, 1000, dp_max=CAP)],
                secondary=lambda: [reg(0, 1000, 1000, dp_max=1000), reg(10, 990, 900, dp_max=CAP + 1)],
                secondary_score=lambda: [reg(0, 1000, 1000, has_extra=0), reg(10, 990, CAP + 1, has_extra=0, cnt=5)],
                inversion=lambda: [reg(0, 1000, 500), reg(1100, 2000, 80, as_=30, cnt=5), reg(1000, 1100, CAP + 1, dp_max=CAP + 1, cnt=0, as_=10, n_sub=CAP, bits=BIT_INV)],
                score_with_p=lambda: [reg(0, 1000, 1 << 30, dp_max=1000)])


def one_read(records):
    return PS.pack(dict(opt=PS.OPT, lds_cap=PS.AP_LDS_CAP, reads=[(0, []), (3, records()), (0, [])]))


def call(d, p):
    return d.align_post(PS.post_opt(p["opt"]), p["rep_len"], p["regs_off"], p["regs"], p["extra"], p["cigar_off"], p["cigar"])


def test_error_word_refuses_accepts_and_lets_pass():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 12, max_reads=1 << 6) as d:
        g = PS.load("structure")
        off, need = np.zeros(4, np.int64), np.zeros(2, np.int64)
        for what, records in REFUSED.items():
            p = one_read(records)
            with pytest.raises(chaindp.ChainDPError) as e:
                call(d, p)
            assert "-2" in str(e.value).split(":")[0] and "2^24" in str(e.value), what
            assert d._lib.chaindp_align_post_fetch(d._ctx, 3, off.ctypes.data, None, None, None, 0, None, None, 0, need.ctypes.data) == -1, what     # nothing resident
            check(*from_host(d, "structure"), "after the refusal of " + what)
        for what, records in ACCEPTED.items():
            p = one_read(records)
            want = M.run(PS.opt_of(p["opt"]), p["rep_len"], p["regs_off"], p["regs"], p["extra"], p["cigar_off"], p["cigar"])
            check(want, call(d, p), what)
            if what == "secondary":
                assert want["dp_max2"][0] == CAP + 1 and want["regs"]["parent"].tolist() == [0, 0]
            if what == "inversion":
                assert want["regs"]["bits"][2] & BIT_INV and int(want["regs"]["bits"][2]) & 0xff > 0
