"""CPU tier: what the kernels of chaindp_align_post (csrc/apost/chaindp_apost.hip) cost, from the compiler's resource remarks for
gfx950.  tests/golden/kernel_resources_apost.json records them in the form of tests/golden/kernel_resources.json, which holds the
kernels of csrc/*.hip (python tests/test_apost_kernel_resources.py --record rewrites it).  k_apost_read stages a list of up to AP_LDS_CAP
regions in static LDS, AP_NF ints a region: few enough bytes, and few enough registers, for eight one-wave workgroups per SIMD."""
import json
import os
import sys

from kernel_listing import FIELDS, HERE, kernel, mangled, remarks

APOST_TABLE = os.path.join(HERE, "golden", "kernel_resources_apost.json")
APOST_KERNELS = ("k_apost_read", "k_apost_gather", "k_apost_gather_cig", "k_apost_logf_probe")
SOURCE = "apost/chaindp_apost.hip"
AP_LDS_CAP, AP_NF = 48, 24


def collect_apost():
    return {SOURCE: {k: [v[f] for f in FIELDS] for k, v in remarks("chaindp_apost").items()}}


def test_every_apost_kernel_costs_what_its_table_records():
    with open(APOST_TABLE) as f:
        table = json.load(f)
    now = collect_apost()
    assert now == table, {k: (v, now[SOURCE].get(k)) for k, v in table[SOURCE].items() if now[SOURCE].get(k) != v}
    assert len(table[SOURCE]) == len(APOST_KERNELS)


def test_apost_kernels_have_no_scratch_no_spilled_vector_register_and_at_most_64_vgprs():
    r = remarks("chaindp_apost")
    assert len(r) == len(APOST_KERNELS), sorted(r)
    for name in APOST_KERNELS:
        k = kernel(r, mangled(name))
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["VGPRs"] <= 64, (name, k)
    assert kernel(r, mangled("k_apost_read"))["LDS Size [bytes/block]"] == 4 * AP_NF * AP_LDS_CAP
    assert 32 * 4 * AP_NF * AP_LDS_CAP <= 160 << 10                               # eight workgroups per SIMD fit a CU's LDS
    assert kernel(r, mangled("k_apost_read"))["Occupancy [waves/SIMD]"] == 8
    for name in ("k_apost_gather", "k_apost_gather_cig", "k_apost_logf_probe"):
        assert kernel(r, mangled(name))["LDS Size [bytes/block]"] == 0, name


def test_the_tables_of_the_other_kernels_do_not_hold_them():
    for other in ("kernel_resources.json", "kernel_resources_inv.json", "kernel_resources_reads.json"):
        with open(os.path.join(HERE, "golden", other)) as f:
            assert not any("k_apost_" in k for src in json.load(f).values() for k in src), other


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(APOST_TABLE, "w") as f:
        json.dump(collect_apost(), f, indent=1, sort_keys=True)
        f.write("\n")
