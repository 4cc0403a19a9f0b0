"""CPU tier: what the kernels at the end of chaindp_align_reads (csrc/reads/chaindp_reads.hip) cost, from the compiler's resource
remarks for gfx950.  tests/golden/kernel_resources_reads.json records them in the form of tests/golden/kernel_resources.json, which
holds the kernels of csrc/*.hip (python tests/test_reads_kernel_resources.py --record rewrites it).  k_reads_finish keeps a list of up
to RD_LDS_CAP records in static LDS, 24 bytes a record; k_reads_scan its two running sums of 256 reads; k_reads_tied the two digit
tables of radix_sort_128x, 256 words each, which one lane indexes by a key's byte: in registers they would be scratch."""
import json
import os
import sys

from kernel_listing import FIELDS, HERE, kernel, mangled, remarks

READS_TABLE = os.path.join(HERE, "golden", "kernel_resources_reads.json")
READS_KERNELS = ("k_reads_keep", "k_reads_finish", "k_reads_tied", "k_reads_scan", "k_reads_order", "k_reads_gather", "k_reads_gather_cig")
SOURCE = "reads/chaindp_reads.hip"
RD_LDS_CAP = 1024


def collect_reads():
    return {SOURCE: {k: [v[f] for f in FIELDS] for k, v in remarks("chaindp_reads").items()}}


def test_every_reads_kernel_costs_what_its_table_records():
    with open(READS_TABLE) as f:
        table = json.load(f)
    now = collect_reads()
    assert now == table, {k: (v, now[SOURCE].get(k)) for k, v in table[SOURCE].items() if now[SOURCE].get(k) != v}
    assert len(table[SOURCE]) == len(READS_KERNELS)


def test_reads_kernels_have_no_scratch_no_spilled_vector_register_and_at_most_64_vgprs():
    r = remarks("chaindp_reads")
    assert len(r) == len(READS_KERNELS), sorted(r)
    for name in READS_KERNELS:
        k = kernel(r, mangled(name))
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["VGPRs"] <= 64, (name, k)
    assert kernel(r, mangled("k_reads_finish"))["LDS Size [bytes/block]"] == 24 * RD_LDS_CAP
    assert kernel(r, mangled("k_reads_tied"))["LDS Size [bytes/block]"] == 2 * 256 * 4
    for name in ("k_reads_keep", "k_reads_order", "k_reads_gather", "k_reads_gather_cig"):
        assert kernel(r, mangled(name))["LDS Size [bytes/block]"] == 0, name


def test_the_tables_of_the_other_kernels_do_not_hold_them():
    for other in ("kernel_resources.json", "kernel_resources_inv.json"):
        with open(os.path.join(HERE, "golden", other)) as f:
            assert not any("k_reads_" in k for src in json.load(f).values() for k in src), other


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(READS_TABLE, "w") as f:
        json.dump(collect_reads(), f, indent=1, sort_keys=True)
        f.write("\n")
