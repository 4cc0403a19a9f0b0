"""CPU tier: what the kernels of the hand-off between chain_post and the alignment stages (csrc/handoff/chaindp_handoff.hip) cost, from
the compiler's resource remarks for gfx950.  tests/golden/kernel_resources_handoff.json records them in the form of
tests/golden/kernel_resources.json, which holds the kernels of csrc/*.hip (python tests/test_handoff_kernel_resources.py --record
rewrites it).  k_handoff_move keeps as, cnt and the new as of a list of up to HO_LDS_CAP regions in static LDS, 12 bytes a region, and
is held to the 64 registers that let eight waves share a SIMD; k_handoff_count keeps nothing."""
import json
import os
import sys

from kernel_listing import FIELDS, HERE, kernel, mangled, remarks

TABLE = os.path.join(HERE, "golden", "kernel_resources_handoff.json")
KERNELS = ("k_handoff_count", "k_handoff_move")
SOURCE = "handoff/chaindp_handoff.hip"
HO_LDS_CAP = 256


def collect():
    return {SOURCE: {k: [v[f] for f in FIELDS] for k, v in remarks("chaindp_handoff").items()}}


def test_every_handoff_kernel_costs_what_its_table_records():
    with open(TABLE) as f:
        table = json.load(f)
    now = collect()
    assert now == table, {k: (v, now[SOURCE].get(k)) for k, v in table[SOURCE].items() if now[SOURCE].get(k) != v}
    assert len(table[SOURCE]) == len(KERNELS)


def test_handoff_kernels_have_no_scratch_no_spilled_vector_register_and_at_most_64_vgprs():
    r = remarks("chaindp_handoff")
    assert len(r) == len(KERNELS), sorted(r)
    for name in KERNELS:
        k = kernel(r, mangled(name))
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["VGPRs"] <= 64, (name, k)
    assert kernel(r, mangled("k_handoff_move"))["LDS Size [bytes/block]"] == 12 * HO_LDS_CAP
    assert kernel(r, mangled("k_handoff_count"))["LDS Size [bytes/block]"] == 0


def test_the_tables_of_the_other_kernels_do_not_hold_them():
    for other in ("kernel_resources.json", "kernel_resources_inv.json", "kernel_resources_reads.json", "kernel_resources_apost.json"):
        with open(os.path.join(HERE, "golden", other)) as f:
            assert not any("k_handoff_" in k for src in json.load(f).values() for k in src), other


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(TABLE, "w") as f:
        json.dump(collect(), f, indent=1, sort_keys=True)
        f.write("\n")
