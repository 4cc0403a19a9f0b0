"""CPU tier: what the alignment kernels cost, and that they cost the existing kernels nothing.  Cross-compiles every .hip of the
library for gfx950 and reads the compiler's resource remarks: k_ksw_extd<1>, k_ksw_extd<4> and k_ksw_pack have no static LDS (all
of theirs is the dynamic block the launch sizes) and no scratch, and every other kernel has the registers, spills, scratch and LDS
recorded in tests/golden/ksw/kernel_resources_parent.json from the commit before the alignment was added.

  python tests/test_ksw_resources.py CSRC_DIR OUT.json     records such a table from a source tree"""
import concurrent.futures
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "minimap2_chaindp_amd", "csrc")
TABLE = os.path.join(HERE, "golden", "ksw", "kernel_resources_parent.json")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIELDS = ("TotalSGPRs", "VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")
KSW_KERNELS = {"k_ksw_extd<1>": r"_ZN7chaindp10k_ksw_extdILi1EEE", "k_ksw_extd<4>": r"_ZN7chaindp10k_ksw_extdILi4EEE", "k_ksw_pack": r"_ZN7chaindp10k_ksw_packE"}


def remarks_of(src, defs=()):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", *defs, "-S", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "out.s"), src], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)\s", line + " ")
        if cur is not None and m:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def collect(csrc):
    """{file[ + defines]: {mangled kernel name: [the FIELDS]}} of every .hip under csrc (chaindp_dense.hip also as the library's second build)."""
    jobs = [(os.path.basename(p), p, ()) for p in sorted(glob.glob(os.path.join(csrc, "*.hip")))]
    jobs.append(("chaindp_dense.hip -DDN_VARIANT16", os.path.join(csrc, "chaindp_dense.hip"), ("-DDN_VARIANT16",)))
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda j: remarks_of(j[1], j[2]), jobs))
    return {j[0]: {k: [v[f] for f in FIELDS] for k, v in r.items()} for j, r in zip(jobs, res)}


@pytest.fixture(scope="module")
def now():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return collect(CSRC)


def test_alignment_kernels_have_no_static_lds_and_no_scratch(now):
    ksw = now["chaindp_ksw.hip"]
    assert len(ksw) == len(KSW_KERNELS), sorted(ksw)
    for name, pattern in KSW_KERNELS.items():
        (k,) = [v for m, v in ksw.items() if re.match(pattern, m)]
        res = dict(zip(FIELDS, k))
        assert res["LDS Size [bytes/block]"] == 0 and res["ScratchSize [bytes/lane]"] == 0 and res["VGPRs Spill"] == 0, (name, res)


def test_existing_kernels_are_what_they_were(now):
    with open(TABLE) as f:
        before = json.load(f)
    assert sorted(before) == sorted(k for k in now if k != "chaindp_ksw.hip")
    for src, kernels in before.items():
        assert now[src] == kernels, (src, {k: (v, now[src].get(k)) for k, v in kernels.items() if now[src].get(k) != v})


if __name__ == "__main__":
    with open(sys.argv[2], "w") as out:
        json.dump(collect(sys.argv[1]), out, indent=1, sort_keys=True)
