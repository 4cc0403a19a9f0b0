"""CPU tier: k_chain_twin's occupancy by design, from the compiler's resource remarks for gfx950 (tests/kernel_listing.py): every
instantiation (both LDS layouts, both gap variants) has no scratch and no VGPR spills and few enough VGPRs for the waves per SIMD its
LDS layout allows; and the layouts' LDS fits the workgroups per CU the launch asks for."""
import os

import pytest

from kernel_listing import kernel, mangled, remarks

# (max_dist_y >= max_dist_x, one table per wave) -> waves per SIMD.  The two-table layout's LDS allows six (24 workgroups per CU): it
# spends the registers of the other two waves on its tile prefetch.
TARGET_WAVES = {(True, True): 8, (False, True): 7, (True, False): 6, (False, False): 6}
LDS_GRANULE, LDS_PER_CU = 1280, 160 * 1024      # MI355X: LDS per CU and the piece it is handed out in (tools/lds_occupancy_probe.hip)


def twin(samegap, one):
    return kernel(remarks("chaindp_twin"), mangled("k_chain_twin", samegap, one))


@pytest.mark.parametrize("samegap,one", sorted(TARGET_WAVES), ids=lambda x: str(x))
def test_registers_allow_the_target_waves(samegap, one):
    k = twin(samegap, one)
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
def test_launch_asks_for_what_lds_and_registers_allow(lib, samegap, one):
    """The layout's LDS (from the library itself) and the kernel's registers must both allow the workgroups per CU the launch asks
    for, and the one-table layout must reach 32 (eight waves per SIMD) where its registers do."""
    lds = lib.chaindp_debug_twin_lds_bytes(int(one))
    wg = lib.chaindp_debug_twin_max_wg_per_cu(int(samegap), int(one))
    alloc = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert LDS_PER_CU // alloc >= wg, (lds, alloc, wg)
    assert 4 * twin(samegap, one)["Occupancy [waves/SIMD]"] >= wg
    assert wg == min(4 * TARGET_WAVES[(samegap, one)], LDS_PER_CU // alloc), wg
    if one:
        assert lds <= 5120, lds
