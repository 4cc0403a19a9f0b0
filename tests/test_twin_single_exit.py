"""CPU tier: the fast loop of k_chain_twin<true, true> (one cost table, max_dist_y >= max_dist_x: the flagship instantiation) has
one way out.  Cross-compiles chaindp_twin.hip for gfx950, walks the loop's common path from its header round to it (the walker of
test_twin_pass_budget.py), and checks that the path decides whether to go on with ONE scalar compare and ONE conditional branch: the
interleave test, the B-lane counts of both halves and the pass counter are folded into that compare, and everything rare (general
pass, lane-31 window test, tile end) is out of line behind the loop.  Also the budget that folding buys, and no
SGPR spill traffic inside the loop."""
import os
import subprocess

import pytest

from test_twin_pass_budget import CSRC, HIPCC, KERNEL, classify, parse_function_raw

HALF_RATE_MAX, FULL_RATE_MAX, SALU_MAX, LDS = 18, 15, 22, 8


def _walk(raw):
    """(instructions of the common path, labels the path branches to): the path as test_twin_pass_budget.fast_pass finds it, with
    every conditional branch on it kept for the checks below."""
    lines, notes = [], []
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
    path, branches, i = [], [], header + 1
    for _ in range(2000):
        if i == header:
            return path, branches, lines[header][:-1]
        l = lines[i]
        if l.endswith(":") or l.startswith("."):
            i += 1
            continue
        m = l.split(None, 1)
        mn, ops = m[0], [o.strip() for o in m[1].split(",")] if len(m) > 1 else []
        path.append((mn, ops))
        if mn == "s_branch":
            i = labels[ops[0]]
            continue
        if mn.startswith("s_cbranch"):
            branches.append((mn, ops[0]))
            if labels.get(ops[0]) == header:
                i = header
                continue
        i += 1
    raise AssertionError("no way back to the loop header")


@pytest.fixture(scope="module")
def fast_loop(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("twin_exit") / "twin.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), os.path.join(CSRC, "chaindp_twin.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return _walk(parse_function_raw(out.read_text(), KERNEL))


def test_one_conditional_branch(fast_loop):
    """One conditional branch on the common path, decided by one scalar compare: either it is the back edge and the loop is left
    where it is not taken, or it leaves the loop and an s_branch is the back edge.  No flag registers of a merged exit."""
    path, branches, header = fast_loop
    assert len(branches) == 1, branches
    mn, target = branches[0]
    assert mn in ("s_cbranch_scc0", "s_cbranch_scc1"), branches
    back_edges = [ops[0] for m, ops in path if m == "s_branch"]
    assert target == header or back_edges == [header], (branches, back_edges)
    compares = [m for m, _ in path if m.startswith("s_cmp")]
    assert len(compares) == 1, compares
    assert not any(m in ("s_cselect_b64",) or (m in ("s_and_b64", "s_andn2_b64") and ops[:2] == ["vcc", "exec"]) for m, ops in path), path


def test_budget_and_no_spill_traffic(fast_loop):
    path = fast_loop[0]
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
    assert c["lds"] == LDS, c
    assert not any(mn.startswith(("v_readlane", "v_writelane", "scratch_", "buffer_")) for mn, _ in path), path
