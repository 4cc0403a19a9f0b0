"""GPU tier of Device.align_reads (chaindp_align_reads) where regions of a read share the sort key dp_max << 32 | hash: the tie scenes
of tests/golden/align_reads/ (align_reads_shapes.TIE_NAMES), recorded from the reference's mm_align_skeleton, whose mm_hit_sort_by_dp
leaves equal keys as radix_sort_128x and the reversal behind it do -- the later placed region first up to 64 live regions, the order
of the in-place byte-wise procedure above.  Every comparison is exact (check_final): each scene under its own LDS cap, the built-in
one and SCENE_CAP, joined with the tie-free scene `trips` and in reversed read order, and through Device.align_reads_post, whose
mm_set_parent, mm_select_sub and mapq consume the order.

The scan and grid edges of the kernels at the end of the call, on tie-free reads: k_reads_scan's trips of 256 reads (255, 256, 257 and
513 reads), reads_grid's cap of 65536 workgroups and k_reads_finish's reuse of its LDS from read to read (65536 and 65537 reads)."""
import numpy as np
import pytest

import align_reads_shapes as RS
import apost_model as M
import apost_shapes as PS
import skeleton_model as K
from test_gpu_align_reads import opt_of, run
from test_gpu_skeleton import blocks, check_final, join
from test_skeleton_cpu import load as load_skeleton, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def under_cap(dev, g, cap, label):
    dev.align_reads_set_lds_cap(cap)
    try:
        check_final(g, run(dev, g), label)
    finally:
        dev.align_reads_set_lds_cap(0)


@pytest.mark.parametrize("name", RS.TIE_NAMES)
def test_tie_scene_under_its_own_cap_the_built_in_cap_and_the_scene_cap(dev, name):
    g = RS.load(name)
    assert sum(RS.tie_classes(g).values()) > 0
    under_cap(dev, g, int(g["lds_cap"]), name)
    check_final(g, run(dev, g), name + ", built-in cap")
    under_cap(dev, g, RS.SCENE_CAP, name + ", every longer list on the global route")


def test_tie_scenes_joined_with_a_tie_free_scene_and_in_reverse_order(dev):
    gs = [RS.load(n) for n in RS.TIE_NAMES + ("trips",)]
    assert len({tuple(int(v) for v in x["opt"]) for x in gs}) == 1
    g = join([(x, blocks(x)) for x in gs])
    check_final(g, run(dev, g), "joined")
    under_cap(dev, g, RS.SCENE_CAP, "joined, every longer list on the global route")
    g = join([(x, blocks(x)[::-1]) for x in gs[::-1]])
    check_final(g, run(dev, g), "reversed")


@pytest.mark.parametrize("name", ("ties_small", "ties_64"))
def test_the_tail_of_align_regs_over_a_tied_order(dev, name):
    """align_reads_post against apost_model over the golden's final lists: parents, subs and mapq of the order the reference left."""
    g = RS.load(name)
    row = PS.opt_row(PS.real_opt(g["opt"]))
    rep_len = (np.arange(len(g["seq_off"]) - 1) % 3 * 150).astype(np.int32)
    want = M.run(PS.opt_of(row), rep_len, g["regs_off_out"], g["regs_out"], g["extra_out"], g["cigar_off_out"], g["cigar_out"])
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    a, *got = dev.align_reads_post(opt_of(g), PS.post_opt(row), g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"], rep_len)
    assert same(a, g["a_out"])
    for k, x in zip(M.OUTPUTS, got):
        assert same(x, want[k]), (name, k, np.flatnonzero(x != want[k])[:4] if x.shape == want[k].shape else (x.shape, want[k].shape))


# ---- the scan's trips and the grid's cap

DATA = ("seq", "a", "regs", "a_out", "regs_out", "placed_out", "extra_out", "cigar_out")
OFFS = dict(seq_off="seq", a_off="a", regs_off="regs", regs_off_out="regs_out", placed_off_out="placed_out")


def tiled(g, bs, n_reads):
    """The reads bs of scene g, again and again, to n_reads reads, with the golden tiled the same way."""
    whole, rest = divmod(n_reads, len(bs))
    full, tail = join([(g, bs)]), join([(g, bs[:rest])]) if rest else None
    out = dict(opt=g["opt"], tseq=g["tseq"], tseq_off=g["tseq_off"])
    for k in DATA:
        out[k] = np.concatenate([np.tile(full[k], (whole,) + (1,) * (full[k].ndim - 1))] + ([tail[k]] if rest else []))
    for k in OFFS:
        out[k] = K.offsets(np.concatenate([np.tile(np.diff(full[k]), whole)] + ([np.diff(tail[k])] if rest else [])))
    out["cigar_off_out"] = K.offsets(out["extra_out"]["n_cigar"])
    return out


@pytest.mark.parametrize("n_reads", (255, 256, 257, 513))
def test_scan_trips_of_256_reads(dev, n_reads):
    g = load_skeleton("rounds")
    bs = blocks(g)
    assert len(bs) == 5 and any(len(b["regs"]) == 0 for b in bs) and len({len(b["regs_out"]) for b in bs}) >= 3
    h = tiled(g, bs, n_reads)
    assert len(h["seq_off"]) - 1 == n_reads
    got = run(dev, h)
    check_final(h, got, "%d reads" % n_reads)                 # regs_off and cigar_off are among the outputs: exact


@pytest.mark.parametrize("n_reads", (65536, 65537))
def test_grid_cap_of_65536_workgroups(n_reads):
    """One recorded read of one region, 65536 and 65537 times: at 65537 reads a workgroup of k_reads_finish and of k_reads_order takes a
    second read.  Measured on an MI355X: 0.07 to 0.09 s a case, the tiling and the comparison included."""
    from minimap2_chaindp_amd import chaindp
    g = RS.load("trips")
    (b,) = [b for b in blocks(g) if len(b["regs"]) == 1]
    assert len(b["seq"]) <= 120 and len(b["regs_out"]) == 1
    h = tiled(g, [b], n_reads)
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 17) as d:
        check_final(h, run(d, h), "%d reads" % n_reads)
