"""CPU tier: what k_chain_twin's per-tile service costs in SGPR spill traffic.  The kernel's scalar registers are spilled into
lanes of a vector register and taken back with v_writelane / v_readlane: VALU instructions at half rate (tools/issue_calib.hip,
profiles/r07_issue_calib.json) that contribute nothing to the result.  With the by-value TwinArgs held in scalar registers through
the pass loops, the service took its pointers back a sixteen-register tuple at a time; it now reads them from the kernel-argument
segment where it uses them (TW_KARGS).  Cross-compiles chaindp_twin.hip for gfx950 as test_twin_pass_budget.py does and counts, per
instantiation, the lane moves behind the fast loop's first row_bcast:15 -- the main loop's service, general pass and slow tail --
and in the fast pass of the flagship instantiation itself (none)."""
import os
import subprocess

import pytest

from test_twin_pass_budget import CSRC, HIPCC, fast_pass, parse_function_raw

KERNEL = "_ZN7chaindp12k_chain_twinILb{}ELb{}EEEvNS_8TwinArgsE"

# (max_dist_y >= max_dist_x, one table per wave) -> lane moves behind the fast loop.  Before the change: 484, 209, 213, 216.
# BOUND: half of the flagship's count before, and what is left of the others once the arguments are read where they are used
# (they have the scalar registers of six and seven waves per SIMD).  LANDED: what the build reaches, held as the pass budget is.
BOUND = {(True, True): 242, (False, True): 32, (True, False): 32, (False, False): 32}
LANDED = {(True, True): 111, (False, True): 30, (True, False): 26, (False, False): 26}


def is_lane_move(line):
    return line.startswith(("v_readlane_b32", "v_writelane_b32"))


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("twin_spills") / "twin.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), os.path.join(CSRC, "chaindp_twin.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out.read_text()


def lane_moves_behind_fast_loop(asm, samegap, one):
    raw = parse_function_raw(asm, KERNEL.format(int(samegap), int(one)))
    code = [r.partition(";")[0].strip() for r in raw]
    code = [c for c in code if c and not c.endswith(":") and not c.startswith(".")]
    bcast = next(i for i, c in enumerate(code) if "row_bcast:15" in c)
    return sum(1 for c in code[bcast:] if is_lane_move(c))


def test_counter():
    assert is_lane_move("v_readlane_b32 s14, v58, 0")
    assert is_lane_move("v_writelane_b32 v58, s12, 0")
    assert not is_lane_move("v_readfirstlane_b32 s4, v2")
    assert not is_lane_move("s_load_dwordx2 s[4:5], s[0:1], 0x48")


@pytest.mark.parametrize("samegap,one", sorted(BOUND), ids=lambda x: str(x))
def test_lane_moves_behind_the_fast_loop(listing, samegap, one):
    n = lane_moves_behind_fast_loop(listing, samegap, one)
    print(f"k_chain_twin<{samegap}, {one}>: {n} lane moves behind the fast loop")
    assert n <= BOUND[(samegap, one)], n
    assert n <= LANDED[(samegap, one)], n


def test_fast_pass_has_no_lane_moves(listing):
    path = fast_pass(parse_function_raw(listing, KERNEL.format(1, 1)))
    assert len(path) > 40, len(path)                    # (the pass itself: 33 VALU, 20 SALU, 8 LDS)
    assert not [mn for mn, _ in path if mn.startswith(("v_readlane", "v_writelane"))]
