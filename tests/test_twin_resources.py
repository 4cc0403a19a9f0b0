"""CPU tier: k_chain_twin's occupancy by design.  Cross-compiles chaindp_twin.hip for gfx950 and checks, for every instantiation
(both LDS layouts, both gap variants), that it has no scratch and no VGPR spills and few enough VGPRs for the waves per SIMD its
LDS layout allows; and that the layouts' LDS fits the workgroups per CU the launch asks for."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (max_dist_y >= max_dist_x, one table per wave) -> waves per SIMD.  The two-table layout's LDS allows six (24 workgroups per CU): it
# spends the registers of the other two waves on its tile prefetch.
TARGET_WAVES = {(True, True): 8, (False, True): 7, (True, False): 6, (False, False): 6}
LDS_GRANULE, LDS_PER_CU = 1280, 160 * 1024      # MI355X: LDS per CU and the piece it is handed out in (tools/lds_occupancy_probe.hip)


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("twin") / "twin.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, "chaindp_twin.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN7chaindp12k_chain_twinILb([01])ELb([01])EEEvNS_8TwinArgsE", line)
        if m:
            cur = kernels.setdefault((m.group(1) == "1", m.group(2) == "1"), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?):\s+(\d+)\s", line + " ")
        if cur is not None and m:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("samegap,one", sorted(TARGET_WAVES), ids=lambda x: str(x))
def test_registers_allow_the_target_waves(remarks, samegap, one):
    k = remarks[(samegap, one)]
    waves = TARGET_WAVES[(samegap, one)]
    assert k["ScratchSize [bytes/lane]"] == 0, k
    assert k["VGPRs Spill"] == 0, k
    assert k["VGPRs"] <= 512 // waves, k
    assert k["Occupancy [waves/SIMD]"] >= waves, k
    assert k["LDS Size [bytes/block]"] == 0, k          # LDS is addressed from byte 0 of the dynamic segment


@pytest.fixture(scope="module")
def lib():
    from minimap2_chaindp_amd import chaindp
    if not os.path.exists(chaindp.LIB_PATH):
        pytest.skip("library not built")
    return chaindp.lib()


@pytest.mark.parametrize("samegap,one", sorted(TARGET_WAVES), ids=lambda x: str(x))
def test_launch_asks_for_what_lds_and_registers_allow(lib, remarks, samegap, one):
    """The layout's LDS (from the library itself) and the kernel's registers must both allow the workgroups per CU the launch asks
    for, and the one-table layout must reach 32 (eight waves per SIMD) where its registers do."""
    lds = lib.chaindp_debug_twin_lds_bytes(int(one))
    wg = lib.chaindp_debug_twin_max_wg_per_cu(int(samegap), int(one))
    alloc = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert LDS_PER_CU // alloc >= wg, (lds, alloc, wg)
    assert 4 * remarks[(samegap, one)]["Occupancy [waves/SIMD]"] >= wg
    assert wg == min(4 * TARGET_WAVES[(samegap, one)], LDS_PER_CU // alloc), wg
    if one:
        assert lds <= 5120, lds
