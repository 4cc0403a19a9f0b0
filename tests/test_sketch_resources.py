"""CPU tier: the sketch kernels' resources.  Cross-compiles chaindp_sketch.hip for gfx950 and checks that no kernel uses scratch or
spills registers, and that each keeps eight waves per SIMD (they are streaming kernels: latency is hidden by occupancy)."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_sk_push_count", "k_sk_push", "k_sk_kmer", "k_sk_slots", "k_sk_value", "k_sk_windowILb0", "k_sk_windowILb1", "k_sk_read_off")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("sketch") / "sketch.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, "chaindp_sketch.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN7chaindp\d+(k_sk_[a-z_]+(?:ILb[01])?)E", line)
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
    assert k["Occupancy [waves/SIMD]"] == 8, k
    assert k["LDS Size [bytes/block]"] <= 8192, k
