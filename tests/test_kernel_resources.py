"""CPU tier: what every kernel of the library costs, from the compiler's resource remarks for gfx950 (tests/kernel_listing.py).
tests/golden/kernel_resources.json records registers, spills, scratch and static LDS of every kernel; a change that adds or changes
a kernel re-records it (python tests/kernel_listing.py --record), and the diff of the table is what the change cost.  Below it, what
each stage's kernels were designed to: the DESIGN.md sections on the stages say why.  (k_chain_twin's occupancy, which is held against
what the library's launch asks for, is tests/test_twin_resources.py's.)"""
import json

import pytest

from kernel_listing import TABLE, collect, kernel, mangled, remarks


def kernels_of(src, names):
    """{name: figures} of `names` ({name: pattern}), which must be exactly the kernels of csrc/SRC.hip."""
    r = remarks(src)
    assert len(r) == len(names), sorted(r)
    return {name: kernel(r, pattern) for name, pattern in names.items()}


def test_every_kernel_costs_what_the_table_records():
    now = collect()
    with open(TABLE) as f:
        table = json.load(f)
    assert {src: sorted(k) for src, k in now.items()} == {src: sorted(k) for src, k in table.items()}
    for src, kernels in table.items():
        assert now[src] == kernels, (src, {k: (v, now[src][k]) for k, v in kernels.items() if now[src][k] != v})


# ---- the alignment DP and its pack (chaindp_ksw.hip): all of their LDS is the dynamic block the launch sizes

KSW_KERNELS = {"k_ksw_extd<1>": mangled("k_ksw_extd", 1), "k_ksw_extd<4>": mangled("k_ksw_extd", 4), "k_ksw_pack": mangled("k_ksw_pack")}


def test_alignment_kernels_have_no_static_lds_and_no_scratch():
    for name, k in kernels_of("chaindp_ksw", KSW_KERNELS).items():
        assert k["LDS Size [bytes/block]"] == 0 and k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)


# ---- mm_align1 around that DP (chaindp_align.hip): no static LDS but k_align_stitch's, whose mm_reg_set_coor fields for a region and
# what is split off it are a few words (the inversion score's state is the dynamic block the launch sizes)

ALIGN_KERNELS = ("k_align_encode", "k_align_plan", "k_align_gather", "k_align_zdrop", "k_align_stitch", "k_align_extra", "k_align_pack")
STITCH_LDS = 2 * 20 * 4          # PF_NF fields of two records


def test_align_kernels_have_no_scratch_and_no_spilled_vector_registers():
    for name, k in kernels_of("chaindp_align", {n: mangled(n) for n in ALIGN_KERNELS}).items():
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["LDS Size [bytes/block]"] <= (STITCH_LDS if name == "k_align_stitch" else 0), (name, k)
        assert k["VGPRs"] <= 64, (name, k)                      # eight waves per SIMD stay possible


# ---- the fragment kernels (chaindp_frag.hip): the fast path is sized for tiny fragments, at most 10 240 B of LDS per one-wave
# workgroup (1280-byte granule, 160 KB per CU) and at most 128 VGPRs, so four waves or more per SIMD -- twice what k_post_read gets

FRAG_KERNELS = ("k_frag_read", "k_frag_split", "k_frag_seg", "k_frag_revcomp", "k_frag_flip")


def test_every_frag_kernel_of_the_file_is_listed():
    kernels_of("chaindp_frag", {n: mangled(n) for n in FRAG_KERNELS})


@pytest.mark.parametrize("name", FRAG_KERNELS)
def test_frag_resources(name):
    k = kernel(remarks("chaindp_frag"), mangled(name))
    assert k["ScratchSize [bytes/lane]"] == 0, k
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["LDS Size [bytes/block]"] <= 10240, k
    assert k["VGPRs"] <= 128, k
    assert k["Occupancy [waves/SIMD]"] >= 4, k


# ---- the sketch kernels (chaindp_sketch.hip): streaming kernels, latency is hidden by occupancy

SKETCH_KERNELS = {"k_sk_push_count": (), "k_sk_push": (), "k_sk_kmer": (), "k_sk_slots": (), "k_sk_value": (), "k_sk_window<false>": (False,),
                  "k_sk_window<true>": (True,), "k_sk_read_off": ()}


@pytest.mark.parametrize("name", SKETCH_KERNELS)
def test_sketch_no_scratch_no_spills(name):
    k = kernel(remarks("chaindp_sketch"), mangled(name.partition("<")[0], *SKETCH_KERNELS[name]))
    assert k["ScratchSize [bytes/lane]"] == 0, k
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["Occupancy [waves/SIMD]"] == 8, k
    assert k["LDS Size [bytes/block]"] <= 8192, k


# ---- the index-build kernels (chaindp_index.hip): the streaming ones (prepare, the radix passes, grouping, layout) keep eight waves
# per SIMD; the table kernel (one lane per bucket, bound by dependent memory accesses) and the count kernel are exempt

INDEX_STREAMING = ("k_ix_prepare", "k_ix_hist", "k_ix_scatter", "k_ix_group", "k_ix_layout", "k_ix_bentries")
INDEX_KERNELS = INDEX_STREAMING + ("k_ix_tables", "k_ix_counts")


@pytest.mark.parametrize("name", INDEX_KERNELS)
def test_index_no_scratch_no_spills(name):
    k = kernel(remarks("chaindp_index"), mangled(name))
    assert k["ScratchSize [bytes/lane]"] == 0, k
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k


@pytest.mark.parametrize("name", INDEX_STREAMING)
def test_index_streaming_kernels_keep_eight_waves(name):
    k = kernel(remarks("chaindp_index"), mangled(name))
    assert k["Occupancy [waves/SIMD]"] == 8, k
    assert k["LDS Size [bytes/block]"] <= 16384, k       # 256 threads per block: eight blocks per CU at eight waves per SIMD, 128 KB


# ---- the kernels with per-read gaps (chaindp_prepass.hip, chaindp_kernels.hip; DESIGN.md 8, "Per-read gaps"): every gap
# instantiation uses no more scratch than its counterpart and keeps its occupancy

GAP_KERNELS = {"k_prepass": ("chaindp_prepass", mangled("k_prepass")), "k_prepass_gaps": ("chaindp_prepass", mangled("k_prepass_gaps"))}
GAP_KERNELS.update({f"k_chain_units<{n}{', gaps' if gaps else ''}>": ("chaindp_kernels", mangled("k_chain_units", n, gaps))
                    for n in (128, 256, 512) for gaps in (False, True)})
COUNTERPART = {"k_prepass_gaps": "k_prepass", "k_chain_units<128, gaps>": "k_chain_units<128>", "k_chain_units<256, gaps>": "k_chain_units<256>",
               "k_chain_units<512, gaps>": "k_chain_units<512>"}


def gap_kernel(name):
    src, pattern = GAP_KERNELS[name]
    return kernel(remarks(src), pattern)


def test_every_gap_instantiation_is_there():
    both = [m for src in ("chaindp_prepass", "chaindp_kernels") for m in remarks(src)]
    stems = tuple(mangled(n)[:-1] for n in ("k_prepass", "k_prepass_gaps", "k_chain_units"))
    assert len([m for m in both if m.startswith(stems)]) == len(GAP_KERNELS), both
    for name in GAP_KERNELS:
        gap_kernel(name)


@pytest.mark.parametrize("name", sorted(COUNTERPART))
def test_gap_instantiations_use_no_more_scratch(name):
    k, c = gap_kernel(name), gap_kernel(COUNTERPART[name])
    assert k["ScratchSize [bytes/lane]"] <= c["ScratchSize [bytes/lane]"], (name, k, c)
    assert k["LDS Size [bytes/block]"] == 0, (name, k)             # the DP kernels address LDS from byte 0: no static LDS (chaindp_create checks it too)
    assert k["Occupancy [waves/SIMD]"] >= c["Occupancy [waves/SIMD]"], (name, k, c)
