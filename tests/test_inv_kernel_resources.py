"""CPU tier: what the kernels of mm_align1_inv (csrc/inv/chaindp_inv.hip) cost, from the compiler's resource remarks for gfx950.
tests/golden/kernel_resources_inv.json records them in the form of tests/golden/kernel_resources.json, which holds the kernels of
csrc/*.hip (python tests/test_inv_kernel_resources.py --record rewrites it).  All of k_inv_ll's LDS is the dynamic block the launch
sizes (the stripe's right edge, four bytes per row of the padded query); its column record, F, the query pipe and the edge registers
live in vector registers, few enough for eight waves per SIMD."""
import json
import os
import sys

from kernel_listing import FIELDS, HERE, kernel, mangled, remarks

INV_TABLE = os.path.join(HERE, "golden", "kernel_resources_inv.json")
INV_KERNELS = ("k_inv_ll", "k_inv_gather", "k_inv_finish", "k_inv_skip", "k_inv_pack")


def collect_inv():
    return {"inv/chaindp_inv.hip": {k: [v[f] for f in FIELDS] for k, v in remarks("chaindp_inv").items()}}


def test_every_inv_kernel_costs_what_its_table_records():
    with open(INV_TABLE) as f:
        table = json.load(f)
    now = collect_inv()
    assert now == table, {k: (v, now["inv/chaindp_inv.hip"].get(k)) for k, v in table["inv/chaindp_inv.hip"].items() if now["inv/chaindp_inv.hip"].get(k) != v}
    assert len(table["inv/chaindp_inv.hip"]) == len(INV_KERNELS)


def test_inv_kernels_have_no_scratch_no_spilled_vector_register_and_no_static_lds():
    r = remarks("chaindp_inv")
    assert len(r) == len(INV_KERNELS), sorted(r)
    for name in INV_KERNELS:
        k = kernel(r, mangled(name))
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["LDS Size [bytes/block]"] == 0, (name, k)
        assert k["VGPRs"] <= 64, (name, k)
    k = kernel(r, mangled("k_inv_ll"))                            # the hot one: nothing spilled at all, eight waves per SIMD
    assert k["SGPRs Spill"] == 0 and k["Occupancy [waves/SIMD]"] >= 8, k


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(INV_TABLE, "w") as f:
        json.dump(collect_inv(), f, indent=1, sort_keys=True)
        f.write("\n")
