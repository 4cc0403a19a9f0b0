"""CPU tier: the index-build kernels' resources.  Cross-compiles chaindp_index.hip for gfx950 and checks that no kernel uses scratch or
spills registers, and that the streaming kernels (prepare, the radix passes, grouping, layout) keep eight waves per SIMD.  The table
kernel (one lane per bucket, bound by dependent memory accesses) and the count kernel are exempt from the occupancy rule."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
STREAMING = ("k_ix_prepare", "k_ix_hist", "k_ix_scatter", "k_ix_group", "k_ix_layout", "k_ix_bentries")
KERNELS = STREAMING + ("k_ix_tables", "k_ix_counts")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("index") / "index.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, "chaindp_index.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN7chaindp\d+(k_ix_[a-z_]+)E", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)\s", line + " ")
        if cur is not None and m:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_spills(remarks, name):
    assert name in remarks, sorted(remarks)
    k = remarks[name]
    assert k["ScratchSize [bytes/lane]"] == 0, k
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k


@pytest.mark.parametrize("name", STREAMING)
def test_streaming_kernels_keep_eight_waves(remarks, name):
    k = remarks[name]
    assert k["Occupancy [waves/SIMD]"] == 8, k
    assert k["LDS Size [bytes/block]"] <= 16384, k       # 256 threads per block: eight blocks per CU at eight waves per SIMD, 128 KB
