"""CPU tier: the fast loop of k_chain_twin<true, true> (one cost table, max_dist_y >= max_dist_x: the flagship instantiation), read
off the gfx950 listing (tests/kernel_listing.py walks the loop's common path from its header round to it).  The path decides whether
to go on with ONE scalar compare and ONE conditional branch: the interleave test, the B-lane counts of both halves and the pass
counter are folded into that compare, and everything rare (general pass, lane-31 window test, tile end) is out of line behind the
loop.  Also the instruction budget of the pass, its VALU instructions classified by issue rate (what was cut
from the pass: DESIGN.md section 5; what bounds it: section 6), and no SGPR spill traffic inside the loop."""
import pytest

from kernel_listing import classify, fast_loop, function, mangled

# the pass before the VALU cut: 27 half-rate + 15 full-rate VALU (~149 cycles at 4.2 and 2.4 cycles), 23 SALU (branches included),
# 8 LDS.  After it 18 + 15 (~112 cycles), and 22 SALU since the loop has one exit
HALF_RATE_MAX, FULL_RATE_MAX, SALU_MAX, LDS = 18, 15, 22, 8


@pytest.fixture(scope="module")
def loop():
    return fast_loop(function("chaindp_twin", mangled("k_chain_twin", True, True)))


def test_classifier():
    assert classify("v_max_i32_dpp", ["v4", "v20", "v20", "row_shr:1"]) == "half"
    assert classify("v_xad_u32", ["v3", "v24", "-1", "v26"]) == "half"
    assert classify("v_cmp_gt_u32_e64", ["s[0:1]", "s70", "v24"]) == "half"
    assert classify("v_cndmask_b32_e32", ["v24", "-4", "v24", "vcc"]) == "half"
    assert classify("v_and_b32_e32", ["v4", "0x7f8", "v3"]) == "full"
    assert classify("v_add_u32_e32", ["v2", "4", "v2"]) == "full"
    assert classify("s_add_i32", ["s12", "s12", "-1"]) is None


def test_one_conditional_branch(loop):
    """One conditional branch on the common path, decided by one scalar compare: either it is the back edge and the loop is left
    where it is not taken, or it leaves the loop and an s_branch is the back edge.  No flag registers of a merged exit."""
    path, branches, header = loop
    assert len(branches) == 1, branches
    mn, target = branches[0]
    assert mn in ("s_cbranch_scc0", "s_cbranch_scc1"), branches
    back_edges = [ops[0] for m, ops in path if m == "s_branch"]
    assert target == header or back_edges == [header], (branches, back_edges)
    compares = [m for m, _ in path if m.startswith("s_cmp")]
    assert len(compares) == 1, compares
    assert not any(m in ("s_cselect_b64",) or (m in ("s_and_b64", "s_andn2_b64") and ops[:2] == ["vcc", "exec"]) for m, ops in path), path


def test_budget_and_no_spill_traffic(loop):
    path = loop[0]
    c = {"half": 0, "full": 0, "salu": 0, "lds": 0}
    for mn, ops in path:
        k = classify(mn, ops)
        if k:
            c[k] += 1
        elif mn.startswith("s_") and mn != "s_nop" and not mn.startswith("s_waitcnt"):
            c["salu"] += 1
        elif mn.startswith("ds_"):
            c["lds"] += 1
    assert c["half"] <= HALF_RATE_MAX and c["full"] <= FULL_RATE_MAX, c
    assert c["salu"] <= SALU_MAX, c
    assert c["lds"] == LDS, c                      # 4 reads of the rings, the mark round trip, the table, the PF write
    assert not any(mn.startswith(("v_readlane", "v_writelane", "scratch_", "buffer_")) for mn, _ in path), path
