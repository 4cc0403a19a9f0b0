"""CPU tier: what the kernels of mm_align1 cost.  Cross-compiles csrc/align/chaindp_align.hip for gfx950 and reads the compiler's
resource remarks, as tests/test_ksw_resources.py does for the DP: none of the seven kernels has scratch or a spilled vector register, and
none has static LDS but k_align_stitch, whose mm_reg_set_coor fields for a region and what is split off it are a few words (the
inversion score's state is the dynamic block the launch sizes).  That the existing kernels cost what they did is
test_ksw_resources.py's own check against tests/golden/ksw/kernel_resources_parent.json; it compiles every .hip directly under csrc/,
which is why these kernels lie in a directory of their own."""
import glob
import os
import re

import pytest

import test_ksw_resources as R

SRC = os.path.join(R.CSRC, "align", "chaindp_align.hip")
KERNELS = ("k_align_encode", "k_align_plan", "k_align_gather", "k_align_zdrop", "k_align_stitch", "k_align_extra", "k_align_pack")
STITCH_LDS = 2 * 20 * 4          # PF_NF fields of two records


@pytest.fixture(scope="module")
def now():
    if not os.path.exists(R.HIPCC):
        pytest.skip("hipcc not found")
    return R.remarks_of(SRC)


def test_align_kernels_have_no_scratch_and_no_spilled_vector_registers(now):
    assert len(now) == len(KERNELS), sorted(now)
    for name in KERNELS:
        (k,) = [v for m, v in now.items() if re.match(r"_ZN7chaindp%d%sE" % (len(name), name), m)]
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["LDS Size [bytes/block]"] <= (STITCH_LDS if name == "k_align_stitch" else 0), (name, k)
        assert k["VGPRs"] <= 64, (name, k)                      # eight waves per SIMD stay possible


def test_the_directory_keeps_the_older_table_whole():
    assert os.path.basename(SRC) not in [os.path.basename(p) for p in glob.glob(os.path.join(R.CSRC, "*.hip"))]
