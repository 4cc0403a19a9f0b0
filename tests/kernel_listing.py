"""What the CPU tier knows of the compiled kernels.  `make listings` in csrc/ cross-compiles every .hip of the library for gfx950 with the
flags the library is built with and leaves, per source, the listing (objs/NAME.s) and the compiler's resource remarks
(objs/NAME.remarks); the tests read those, and none compiles anything itself.  make rebuilds only what is out of date.

  python tests/kernel_listing.py --record     rewrites tests/golden/kernel_resources.json from the current tree"""
import functools
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "minimap2_chaindp_amd", "csrc")
TABLE = os.path.join(HERE, "golden", "kernel_resources.json")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIELDS = ("TotalSGPRs", "VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")
# the library's second build of chaindp_dense.hip: listing name -> key in the table
VARIANTS = {"chaindp_dense16": "chaindp_dense.hip -DDN_VARIANT16"}


@functools.lru_cache(maxsize=None)
def _make(target):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    r = subprocess.run(["make", "-s", "-j8", f"HIPCC={HIPCC}", target], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def _made(name, suffix):
    _make("listings")
    if not os.path.exists(os.path.join(CSRC, "objs", name + ".s")):
        _make(f"objs/{name}.s")                    # a source that is not (yet) one of the library's
    with open(os.path.join(CSRC, "objs", name + suffix)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def listing(name):
    """The gfx950 listing of csrc/NAME.hip ("chaindp_dense16": chaindp_dense.hip as the library builds it a second time)."""
    return _made(name, ".s")


@functools.lru_cache(maxsize=None)
def remarks(name):
    """{mangled kernel name: {remark: value}} of csrc/NAME.hip, all of the compiler's resource remarks."""
    kernels, cur = {}, None
    for line in _made(name, ".remarks").splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)\s", line + " ")
        if cur is not None and m:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def mangled(name, *targs):
    """What the mangled name of chaindp::NAME<targs...> begins with (template arguments: bools and ints)."""
    args = "".join(f"L{'b' if isinstance(t, bool) else 'i'}{int(t)}E" for t in targs)
    return f"_ZN7chaindp{len(name)}{name}" + (f"I{args}E" if targs else "") + "E"


def _one(names, pattern):
    hits = [m for m in names if re.match(pattern, m)]
    assert len(hits) == 1, (pattern, sorted(names))
    return hits[0]


def kernel(remarks, pattern):
    """The figures of the one kernel whose mangled name matches."""
    return remarks[_one(remarks, pattern)]


def function(name, pattern):
    """The listing lines of the one kernel of csrc/NAME.hip whose mangled name matches, with the compiler's comments."""
    return parse_function_raw(listing(name), _one(remarks(name), pattern))


def collect():
    """{file[ + defines]: {mangled kernel name: [the FIELDS]}} of every .hip of the library."""
    names = sorted([os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, "*.hip"))] + list(VARIANTS))
    return {VARIANTS.get(n, n + ".hip"): {k: [v[f] for f in FIELDS] for k, v in remarks(n).items()} for n in names}


# ---- reading a listing

SREG = re.compile(r"^(s\d+|s\[\d+:\d+\]|vcc|vcc_lo|vcc_hi|exec|exec_lo|exec_hi|m0)$")


def classify(mnemonic, operands):
    """'half', 'full' or None (not VALU): the issue rate as tools/issue_calib.hip measured it on MI355X.  DPP, compares, v_cndmask,
    v_mbcnt, lane moves, three-source and SGPR-operand instructions at half rate (~4.2 cycles), plain two-source ones at full rate
    (~2.4 cycles)."""
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


def code_lines(raw):
    """(instruction or label, the compiler's comment) for every line of a function's listing that holds code."""
    out = []
    for r in raw:
        code, _, comment = r.partition(";")
        code = code.strip()
        if code and not (code.startswith(".") and not code.endswith(":")):
            out.append((code, comment))
    return out


def fast_loop(raw):
    """(instructions of the common path, conditional branches on it, header label) of k_chain_twin's fast loop: the innermost loop
    around the scan's row_bcast:15, its header as the compiler marks it ("Inner Loop Header").  The common path goes from the header
    round to it again, taking no conditional branch but one back to the header."""
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


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(TABLE, "w") as out:
        json.dump(collect(), out, indent=1, sort_keys=True)
