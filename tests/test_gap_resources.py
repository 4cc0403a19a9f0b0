"""CPU tier: the kernels with per-read gaps cost the existing kernels nothing.  Cross-compiles chaindp_prepass.hip and chaindp_kernels.hip
for gfx950 and reads the compiler's resource remarks: k_prepass and k_chain_units<128 / 256 / 512> in their existing instantiations
keep the registers, spills, scratch and LDS they had before the gap instantiations were added ("Per-read gaps": the
table is the record), and every gap instantiation uses no more scratch than its counterpart."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIELDS = ("TotalSGPRs", "VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")
# the existing instantiations, as they were before this file's kernels existed: SGPRs, VGPRs, SGPR spills, VGPR spills, scratch, LDS
BEFORE = {
    "k_prepass":          (106, 55, 2, 0, 0, 0),
    "k_chain_units<128>": (78, 60, 142, 0, 0, 0),
    "k_chain_units<256>": (78, 64, 156, 0, 0, 0),
    "k_chain_units<512>": (78, 64, 172, 7, 32, 0),
}
COUNTERPART = {"k_prepass_gaps": "k_prepass", "k_chain_units<128, gaps>": "k_chain_units<128>", "k_chain_units<256, gaps>": "k_chain_units<256>",
               "k_chain_units<512, gaps>": "k_chain_units<512>"}


def _name(mangled):
    m = re.match(r"_ZN7chaindp\d+(k_prepass_gaps|k_prepass)E", mangled)
    if m:
        return m.group(1)
    m = re.match(r"_ZN7chaindp13k_chain_unitsILi(\d+)ELb([01])EEE", mangled)
    if m:
        return f"k_chain_units<{m.group(1)}{', gaps' if m.group(2) == '1' else ''}>"
    return None


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    kernels = {}
    for src in ("chaindp_prepass.hip", "chaindp_kernels.hip"):
        out = tmp_path_factory.mktemp("gap") / (src + ".s")
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, src)],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        cur = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = kernels.setdefault(_name(m.group(1)), {}) if _name(m.group(1)) else None
                continue
            m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)\s", line + " ")
            if cur is not None and m:
                cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def test_every_instantiation_is_there(remarks):
    assert sorted(remarks) == sorted(list(BEFORE) + list(COUNTERPART))


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_existing_instantiations_are_unchanged(remarks, name):
    assert tuple(remarks[name][f] for f in FIELDS) == BEFORE[name], (name, remarks[name])


@pytest.mark.parametrize("name", sorted(COUNTERPART))
def test_gap_instantiations_use_no_more_scratch(remarks, name):
    k, c = remarks[name], remarks[COUNTERPART[name]]
    assert k["ScratchSize [bytes/lane]"] <= c["ScratchSize [bytes/lane]"], (name, k, c)
    assert k["LDS Size [bytes/block]"] == 0, (name, k)             # the DP kernels address LDS from byte 0: no static LDS (chaindp_create checks it too)
    assert k["Occupancy [waves/SIMD]"] >= c["Occupancy [waves/SIMD]"], (name, k, c)
