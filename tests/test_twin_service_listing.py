"""CPU tier: what k_chain_twin's per-tile service no longer does, read off the gfx950 listing (tests/kernel_listing.py).

* Unit lengths are exact (k_emit_units takes a unit's end from start_mask | single_mask), so take_tile() tests no gap: no
  wave_shr:1 DPP move (the neighbour's x) and no 64-bit vector compare is left in any of the four instantiations.
* Whether the launch's parameters are the kernel's is decided once, when the kernel starts, and kept in the halves' cold state:
  par.is_cdna and par.n_segs, which nothing else reads, are loaded from the kernel-argument segment at most once per function
  and not through the service's own argument pointers, and at most one single-dword load of par.max_dist_y is left (the
  first sixteen bytes of par, max_dist_y among them, are also loaded as one where the kernel reads max_dist_x and bw).
* The flagship instantiation's way from the fast loop's exit to the flush's flag store is shorter than it was in the parent
  commit (static instructions in layout order).
* SGPR spill traffic.  The kernel's scalar registers are spilled into lanes of a vector register and taken back with v_writelane /
  v_readlane: VALU instructions at half rate (tools/issue_calib.hip, profiles/r07_issue_calib.json) that contribute nothing to the
  result.  With the by-value TwinArgs held in scalar registers through the pass loops, the service took its pointers back a
  sixteen-register tuple at a time; it now reads them from the kernel-argument segment where it uses them (TW_KARGS).  Counted per
  instantiation: the lane moves behind the fast loop's first row_bcast:15 -- the main loop's service, general pass and slow tail.
  (That the fast pass itself has none is test_twin_single_exit.py's.)"""
import re

import pytest

from kernel_listing import code_lines, function, mangled
from minimap2_chaindp_amd.params import ChainParams

INSTANCES = [(1, 1), (0, 1), (1, 0), (0, 0)]


def twin(samegap, one):
    return function("chaindp_twin", mangled("k_chain_twin", bool(samegap), bool(one)))


# static instructions from the first label behind the fast loop (the first block in layout order that is not one of the loop's)
# to the first global_store_byte behind it, in k_chain_twin<true, true>: counted by service_head() below on the listing of
# commit cf9c2f9 (the parent of the change that made unit lengths exact), same compiler flags
PARENT_COMMIT, PARENT_SERVICE_HEAD = "cf9c2f9", 677


def service_head(raw):
    lines = code_lines(raw)
    bcast = next(i for i, (c, _) in enumerate(lines) if "row_bcast:15" in c)
    header = next(i for i in range(bcast, -1, -1) if lines[i][0].endswith(":") and "Inner Loop Header" in lines[i][1])
    name = lines[header][0][1:-1]                          # ".LBB0_191:" -> "LBB0_191"; its blocks are marked "in Loop: Header=BB0_191"
    first = next(i for i in range(bcast, len(lines)) if lines[i][0].endswith(":") and f"Header={name[1:]} " not in lines[i][1] + " ")
    store = next(i for i in range(first, len(lines)) if lines[i][0].startswith("global_store_byte"))
    return sum(1 for c, _ in lines[first:store] if not c.endswith(":"))


LOAD = re.compile(r"^s_load_dword(x2|x4|x8|x16)?\s+\S+,\s*(s\[\d+:\d+\]),\s*(0x[0-9a-f]+|\d+)")


def kernarg_loads(raw, field_offset):
    """(base pair, offset, bytes) of the scalar loads that cover byte `field_offset` of the kernel-argument segment: through
    s[0:1], the segment's pointer at entry, or through a pair it is copied into (TW_KARGS)."""
    lines = [c for c, _ in code_lines(raw)]
    bases = {"s[0:1]"} | {m.group(1) for c in lines for m in [re.match(r"^s_mov_b64\s+(s\[\d+:\d+\]),\s*s\[0:1\]$", c)] if m}
    out = []
    for c in lines:
        m = LOAD.match(c)
        if m and m.group(2) in bases:
            size, off = 4 * int((m.group(1) or "x1")[1:]), int(m.group(3), 0)
            if off <= field_offset < off + size:
                out.append((m.group(2), off, size))
    return out


# (max_dist_y >= max_dist_x, one table per wave) -> lane moves behind the fast loop.  Before the change: 484, 209, 213, 216.
# BOUND: half of the flagship's count before, and what is left of the others once the arguments are read where they are used
# (they have the scalar registers of six and seven waves per SIMD).  LANDED: what the build reaches, held as the pass budget is.
BOUND = {(True, True): 242, (False, True): 32, (True, False): 32, (False, False): 32}
LANDED = {(True, True): 111, (False, True): 30, (True, False): 26, (False, False): 26}


def is_lane_move(line):
    return line.startswith(("v_readlane_b32", "v_writelane_b32"))


def lane_moves_behind_fast_loop(raw):
    code = [c for c, _ in code_lines(raw) if not c.endswith(":")]
    bcast = next(i for i, c in enumerate(code) if "row_bcast:15" in c)
    return sum(1 for c in code[bcast:] if is_lane_move(c))


def test_parsers():
    raw = ["\ts_mov_b64 s[26:27], s[0:1]", "\ts_load_dwordx2 s[10:11], s[0:1], 0x14", "\ts_load_dword s4, s[26:27], 0x4 ; x",
           "\ts_load_dwordx4 s[8:11], s[12:13], 0x0", "\ts_load_dwordx4 s[28:31], s[0:1], 0x0"]
    assert kernarg_loads(raw, 20) == [("s[0:1]", 0x14, 8)] and kernarg_loads(raw, 24) == [("s[0:1]", 0x14, 8)]
    assert kernarg_loads(raw, 4) == [("s[26:27]", 4, 4), ("s[0:1]", 0, 16)]
    assert (ChainParams.max_dist_y.offset, ChainParams.is_cdna.offset, ChainParams.n_segs.offset) == (4, 20, 24)   # par is TwinArgs' first member


@pytest.mark.parametrize("samegap,one", INSTANCES, ids=lambda x: str(x))
def test_no_gap_test_is_left(samegap, one):
    code = [c for c, _ in code_lines(twin(samegap, one))]
    assert len(code) > 2000
    assert not [c for c in code if "wave_shr:1" in c]
    assert not [c for c in code if re.match(r"v_cmp\w*_u64", c)]


@pytest.mark.parametrize("samegap,one", INSTANCES, ids=lambda x: str(x))
def test_parameters_are_judged_once(samegap, one):
    raw = twin(samegap, one)
    cdna, segs, mdy = (kernarg_loads(raw, f.offset) for f in (ChainParams.is_cdna, ChainParams.n_segs, ChainParams.max_dist_y))
    print(f"k_chain_twin<{samegap}, {one}>: is_cdna {cdna}, n_segs {segs}, max_dist_y {mdy}")
    assert len(cdna) <= 1 and len(segs) <= 1, (cdna, segs)
    assert len([l for l in mdy if l[2] == 4]) <= 1, mdy
    assert all(base == "s[0:1]" for base, _, _ in cdna + segs), (cdna, segs)   # none through a service's TW_KARGS copy


def test_service_head_is_shorter_than_the_parents():
    n = service_head(twin(1, 1))
    print(f"k_chain_twin<1, 1>: {n} instructions from the fast loop's exit to the flush's flag store ({PARENT_COMMIT}: {PARENT_SERVICE_HEAD})")
    assert n < PARENT_SERVICE_HEAD, n


def test_counter():
    assert is_lane_move("v_readlane_b32 s14, v58, 0")
    assert is_lane_move("v_writelane_b32 v58, s12, 0")
    assert not is_lane_move("v_readfirstlane_b32 s4, v2")
    assert not is_lane_move("s_load_dwordx2 s[4:5], s[0:1], 0x48")


@pytest.mark.parametrize("samegap,one", sorted(BOUND), ids=lambda x: str(x))
def test_lane_moves_behind_the_fast_loop(samegap, one):
    n = lane_moves_behind_fast_loop(twin(samegap, one))
    print(f"k_chain_twin<{samegap}, {one}>: {n} lane moves behind the fast loop")
    assert n <= BOUND[(samegap, one)], n
    assert n <= LANDED[(samegap, one)], n
