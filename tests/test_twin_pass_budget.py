"""CPU tier: the instruction budget of k_chain_twin's fast pass.  Cross-compiles chaindp_twin.hip for gfx950, finds the fast loop of
k_chain_twin<true, true> (one cost table, max_dist_y >= max_dist_x: the flagship instantiation) -- the innermost loop around the
scan's row_bcast:15, its header as the compiler's listing marks it ("Inner Loop Header") --, walks its common path round to that
header, and classifies the VALU instructions by issue rate as tools/issue_calib.hip measured them on MI355X: DPP, compares,
v_cndmask, v_mbcnt, three-source and SGPR-operand instructions at half rate (~4.2 cycles), plain two-source ones at full rate
(~2.4 cycles).  The common path: exit branches not taken; a branch whose condition is a flag register that the path itself has
just set (the compiler's merge of the loop's exits: s_and_b64 vcc, exec, s[..] after s_mov_b64 s[..], 0 or -1) goes the way that
flag says.  The counts hold what was cut from the pass; what bounds the pass is in section 6."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL = "_ZN7chaindp12k_chain_twinILb1ELb1EEEvNS_8TwinArgsE"

# the pass before this change: 27 half-rate + 15 full-rate VALU (~149 cycles), 23 SALU (branches included), 8 LDS.  After it: 18 + 15
# (~112 cycles), 30 SALU: the VALU cut holds, and the SALU it costs may not grow further
HALF_RATE_MAX, FULL_RATE_MAX, SALU_MAX = 18, 15, 30
CYCLES_MAX = 112.0                       # 18 * 4.2 + 15 * 2.4
HALF, FULL = 4.2, 2.4

SREG = re.compile(r"^(s\d+|s\[\d+:\d+\]|vcc|vcc_lo|vcc_hi|exec|exec_lo|exec_hi|m0)$")


def classify(mnemonic, operands):
    """'half', 'full' or None (not VALU)."""
    if not mnemonic.startswith("v_"):
        return None
    if "dpp" in mnemonic or any(o.startswith(("row_", "quad_perm", "wave_")) for o in operands):
        return "half"
    if mnemonic.startswith(("v_cmp", "v_cndmask", "v_mbcnt", "v_readlane", "v_writelane", "v_readfirstlane")):
        return "half"
    srcs = [o for o in operands[1:] if not o.startswith(("offset", "row_mask", "bank_mask", "bound_ctrl", "clamp"))]
    if len(srcs) >= 3 or any(SREG.match(o) for o in srcs):
        return "half"
    return "full"


def parse_function_raw(asm, name):
    start = asm.index(f"\n{name}:")
    end = asm.index(".Lfunc_end", start)
    return asm[start:end].splitlines()[1:]


def fast_pass(raw):
    """Instructions of the fast loop's common path, from its header round to it again.  raw: the function's listing lines, with
    the compiler's comments."""
    lines, notes = [], []                          # instruction / label lines, and the comments that belong to each
    for r in raw:
        code, _, comment = r.partition(";")
        code = code.strip()
        if code:
            lines.append(code)
            notes.append(comment)
        elif lines and comment.strip():
            notes[-1] += " " + comment
    bcast = next(i for i, l in enumerate(lines) if "row_bcast:15" in l)
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    header = next(i for i in range(bcast, -1, -1) if lines[i].endswith(":") and "Inner Loop Header" in notes[i])
    path, i, seen, flags = [], header + 1, 0, {}
    while True:
        seen += 1
        assert seen < 2000, "no way back to the loop header"
        if i == header:
            break
        l = lines[i]
        if l.endswith(":") or l.startswith("."):
            i += 1
            continue
        m = l.split(None, 1)
        mn, ops = m[0], [o.strip() for o in m[1].split(",")] if len(m) > 1 else []
        path.append((mn, ops))
        if mn == "s_mov_b64" and ops[1] in ("0", "-1"):
            flags[ops[0]] = int(ops[1]) != 0       # a flag the path sets
        elif mn in ("s_and_b64", "s_andn2_b64") and ops[0] == "vcc" and ops[1] == "exec" and ops[2] in flags:
            flags["vcc"] = flags[ops[2]] if mn == "s_and_b64" else not flags[ops[2]]
        elif ops and ops[0] in flags and not mn.startswith("s_cbranch"):
            del flags[ops[0]]                      # overwritten by something else
        if mn == "s_branch":
            i = labels[ops[0]]
            continue
        if mn.startswith("s_cbranch"):
            target = labels.get(ops[0])
            taken = target == header                               # the back edge
            if mn in ("s_cbranch_vccnz", "s_cbranch_vccz") and "vcc" in flags:
                taken = flags["vcc"] == (mn == "s_cbranch_vccnz")   # decided by a flag set on the path
            if mn.startswith(("s_cbranch_vcc", "s_cbranch_scc")):
                flags.pop("vcc", None)
            if taken:
                i = target
                continue
        i += 1
    return path


@pytest.fixture(scope="module")
def pass_counts(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("twin_budget") / "twin.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), os.path.join(CSRC, "chaindp_twin.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    path = fast_pass(parse_function_raw(out.read_text(), KERNEL))
    counts = {"half": 0, "full": 0, "salu": 0, "lds": 0}
    for mn, ops in path:
        c = classify(mn, ops)
        if c:
            counts[c] += 1
        elif mn.startswith("s_") and mn not in ("s_nop", "s_waitcnt") and not mn.startswith("s_waitcnt"):
            counts["salu"] += 1
        elif mn.startswith("ds_"):
            counts["lds"] += 1
    return counts


def test_classifier():
    assert classify("v_max_i32_dpp", ["v4", "v20", "v20", "row_shr:1"]) == "half"
    assert classify("v_xad_u32", ["v3", "v24", "-1", "v26"]) == "half"
    assert classify("v_cmp_gt_u32_e64", ["s[0:1]", "s70", "v24"]) == "half"
    assert classify("v_cndmask_b32_e32", ["v24", "-4", "v24", "vcc"]) == "half"
    assert classify("v_and_b32_e32", ["v4", "0x7f8", "v3"]) == "full"
    assert classify("v_add_u32_e32", ["v2", "4", "v2"]) == "full"
    assert classify("s_add_i32", ["s12", "s12", "-1"]) is None


def test_fast_pass_within_budget(pass_counts):
    c = pass_counts
    cycles = c["half"] * HALF + c["full"] * FULL
    assert c["half"] <= HALF_RATE_MAX, c
    assert c["full"] <= FULL_RATE_MAX, c
    assert cycles <= CYCLES_MAX + 1e-9, (c, cycles)
    assert c["salu"] <= SALU_MAX, c
    assert c["lds"] == 8, c                        # 4 reads of the rings, the mark round trip, the table, the PF write
