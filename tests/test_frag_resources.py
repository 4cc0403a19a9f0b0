"""CPU tier: the fragment kernels' resources.  Cross-compiles chaindp_frag.hip for gfx950 and checks that no kernel uses scratch or spills
registers, and that the fast path is sized for tiny fragments: at most 10 240 B of LDS per one-wave workgroup (1280-byte granule, 160 KB
per CU) and at most 128 VGPRs, so four waves or more per SIMD -- twice what k_post_read gets."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_frag_read", "k_frag_split", "k_frag_seg", "k_frag_revcomp", "k_frag_flip")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("frag") / "frag.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, "chaindp_frag.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN7chaindp\d+(k_frag_[a-z_]+)E", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)\s", line + " ")
        if cur is not None and m:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def test_every_kernel_of_the_file_is_listed(remarks):
    assert sorted(remarks) == sorted(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_resources(remarks, name):
    assert name in remarks, sorted(remarks)
    k = remarks[name]
    assert k["ScratchSize [bytes/lane]"] == 0, k
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["LDS Size [bytes/block]"] <= 10240, k
    assert k["VGPRs"] <= 128, k
    assert k["Occupancy [waves/SIMD]"] >= 4, k
