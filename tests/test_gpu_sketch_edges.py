"""GPU tier: the inputs of tests/sketch_edge_shapes.py (proved to sit on their edges and held to the reference by
tests/test_sketch_edge_shapes_cpu.py) through chaindp_sketch on the GPU: mini_off and the downloaded minimizers byte for byte against
tests/sketch_model.py.
  alone      every case as a batch of its own (the multi-segment case through n_segs).
  batched    the single-segment cases of one (w, k, is_hpc) as one batch, in constructor order and reversed: every case moves to other
             chunk, push-word and slot-tile phases, and the expected result is still the concatenation.
  after big  every small case again on a context that has just sketched the 262145-base case, so that stale bytes of a larger batch
             sit in pcode, sn, sx and scnt behind (and inside the padding of) what the case writes.
A failure names the case, the read and the first differing minimizer."""
import numpy as np
import pytest

import sketch_edge_shapes as se
from minimap2_chaindp_amd import chaindp

pytestmark = pytest.mark.gpu

NAMES = list(se.CASES)
SMALL = [n for n in NAMES if not n.startswith("scan_slot_tiles_")]
GROUPS = {}
for _n in NAMES:
    if not se.PARAMS[_n][3]:
        GROUPS.setdefault(se.PARAMS[_n][:3], []).append(_n)
GROUPS = {g: names for g, names in GROUPS.items() if len(names) > 1}


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 13) as d:
        yield d


def same(what, got_off, got, want_off, want, read_names=None):
    """mini_off and the minimizers against the expected ones; the first difference named by read and place."""
    def read_of(r):
        return f"read {r}" + (f" ({read_names(r)})" if read_names else "")
    assert len(got_off) == len(want_off), f"{what}: {len(got_off) - 1} reads returned, {len(want_off) - 1} expected"
    bad = np.flatnonzero(got_off != want_off)
    if bad.size:
        r = max(int(bad[0]) - 1, 0)
        raise AssertionError(f"{what}: mini_off: {read_of(r)} has {int(got_off[r + 1] - got_off[r])} minimizers, expected {int(want_off[r + 1] - want_off[r])}; "
                             f"{bad.size} offsets differ, the first at {int(bad[0])}")
    assert got.shape == want.shape, f"{what}: {len(got)} minimizers downloaded, {len(want)} expected"
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        r = int(np.searchsorted(want_off, i, side="right") - 1)
        raise AssertionError(f"{what}: {read_of(r)}, minimizer {i - int(want_off[r])} of {int(want_off[r + 1] - want_off[r])}: got x={int(got[i, 0]):#x} y={int(got[i, 1]):#x}, "
                             f"expected x={int(want[i, 0]):#x} y={int(want[i, 1]):#x}; {bad.size} minimizers differ")
    assert got.tobytes() == want.tobytes() and np.asarray(got_off, np.int64).tobytes() == np.asarray(want_off, np.int64).tobytes()


def run(dev, name):
    c = se.case(name)
    seq, seq_off = se.batch(c.seqs)
    off = dev.sketch(c.w, c.k, c.is_hpc, seq, seq_off, n_segs=c.n_segs)
    return off, dev.download_minimizers()


@pytest.mark.parametrize("name", NAMES)
def test_case_alone(dev, name):
    off, mini = run(dev, name)
    same(name, off, mini, *se.expected(name))


@pytest.mark.parametrize("order", ["constructor_order", "reversed"])
@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: "w%d_k%d_hpc%d" % g)
def test_cases_of_one_parameter_set_in_one_batch(dev, group, order):
    names = GROUPS[group] if order == "constructor_order" else GROUPS[group][::-1]
    seqs, owner, want_off, want, base = [], [], [np.zeros(1, np.int64)], [], 0
    for n in names:
        c = se.case(n)
        e_off, e_mini = se.expected(n)
        seqs += c.seqs; owner += [n] * len(c.seqs)
        want_off.append(e_off[1:] + base); want.append(e_mini); base += len(e_mini)
    seq, seq_off = se.batch(seqs)
    off = dev.sketch(*group, seq, seq_off)
    same("+".join(names), off, dev.download_minimizers(), np.concatenate(want_off), np.concatenate(want), read_names=lambda r: owner[r])


@pytest.mark.parametrize("name", SMALL)
def test_case_after_the_largest(dev, name):
    big_off, _ = run(dev, se.BIG)
    assert big_off[-1] == se.expected(se.BIG)[0][-1]
    off, mini = run(dev, name)
    same(name + " after " + se.BIG, off, mini, *se.expected(name))


def test_multi_segment_reads_through_n_segs(dev):
    c = se.case("multi_segment")
    assert c.n_segs and sorted(set(c.n_segs)) == [1, 2, 3]
    off, mini = run(dev, "multi_segment")
    assert len(off) == len(c.n_segs) + 1
    same("multi_segment", off, mini, *se.expected("multi_segment"))
    rid = (mini[:, 1] >> np.uint64(32)).astype(np.int64)                     # the segment's number is in y: every segment that has minimizers shows
    assert set(rid.tolist()) == {0, 1, 2}
    # the same sequences as single-segment reads: other mini_off, no rid, no shift
    seq, seq_off = se.batch(c.seqs)
    off1 = dev.sketch(c.w, c.k, c.is_hpc, seq, seq_off)
    import sketch_model as sm
    same("multi_segment as single reads", off1, dev.download_minimizers(), *sm.sketch_batch(seq, seq_off, c.w, c.k, c.is_hpc))
