"""GPU tier: where a unit ends.  The prepass writes exact unit lengths (the next start of a unit OR of a singleton behind the
unit's start, or its read's end) and k_chain_twin takes min(64, len - tile) anchors per tile without testing a gap, so a length
that is one anchor off shows as a wrong f / p / v or a wrong new_seed[] byte.  Hand-built reads put a unit's end on every place
the two masks and the tiles can disagree about: singletons between units (1, 2, 63, 64 of them: inside a mask word, across one,
beyond the 64 mask words one wave of k_emit_units holds, behind a unit of 4200 anchors), units of exactly 64, 65, 127, 128 and
129 anchors, ends and starts on read boundaries (with the next read going on at a close x, so that only the boundary
cuts), a gap of exactly max_dist_x against one more, a cut made by the high word of x alone, reads of nothing but singletons and
two-anchor units back to back.  Every case runs with one q_span (the layout with one cost table per wave) and with a q_span per
read (a table per half), through the default route, the hand-over behind the first tile and one unit per wave, and is compared
element for element with the oracle and byte for byte with the oracle's compaction."""
import numpy as np
import pytest

import oracle_lib as ol
from edge_shapes import anchors, batch, colinear, unit_lengths
from minimap2_chaindp_amd import chaindp, params as P

MDX = 10000                             # ava-ont's max_dist_x
FAR = MDX + 1000                        # a gap that cuts
STEP = 9


class Read:
    """Builds one read: units (colinear runs) and singletons, each a given gap in x behind the anchor before it."""

    def __init__(self, x0=1000, q0=1000, rid=0):
        self.parts, self.x, self.q, self.rid = [], x0, q0, rid

    def unit(self, n, gap=FAR):
        self.x += gap
        self.q += 50
        self.parts.append(colinear(n, (self.rid << 32) + self.x, self.q, STEP))
        self.x += STEP * (n - 1)
        self.q += STEP * (n - 1)
        return self

    def singles(self, k, gap=FAR):
        for i in range(k):
            self.unit(1, gap if i == 0 else FAR)
        return self

    def target(self, rid, x):
        """The anchors that follow lie on another target: the high word of x changes, the low word starts at x."""
        self.rid, self.x = rid, x
        return self

    def done(self):
        return np.concatenate(self.parts)


def _cases():
    c = {}
    for k in (1, 2, 63, 64):
        # (the unit in front is 70 anchors: the singletons start at bit 6 of the second mask word)
        c[f"unit_{k}_singletons_unit"] = [Read().unit(70, 0).singles(k).unit(50).done(),
                                          Read().singles(5, 0).unit(30).singles(k).unit(2).singles(k).unit(90).done()]
    for n in (64, 65, 127, 128, 129):
        c[f"unit_of_{n}_singleton_unit"] = [Read().unit(n, 0).singles(1).unit(40).done(),
                                            Read().singles(3, 0).unit(n).singles(1).unit(n).done()]
    # read boundaries: each read goes on where the one before it stopped (x one step on), so nothing but the boundary cuts
    r1 = Read().unit(100, 0)                              # the unit is the read
    r2 = Read(r1.x + STEP - FAR, r1.q).unit(70)           # starts at the read's first anchor, a singleton behind it
    r2.singles(1)
    r3 = Read(r2.x + STEP - FAR, r2.q).singles(1).unit(70)   # a singleton first, the unit ends with the read
    r4 = Read(r3.x + STEP - FAR, r3.q).unit(64)           # exactly one tile, then the batch's last read
    r5 = Read(r4.x + STEP - FAR, r4.q).unit(129)
    c["units_on_read_boundaries"] = [r.done() for r in (r1, r2, r3, r4, r5)]
    c["gap_of_max_dist_x_and_one_more"] = [Read().unit(40, 0).unit(40, MDX).unit(40, MDX + 1).unit(40, MDX).done(),
                                           Read().unit(64, 0).unit(64, MDX + 1).unit(64, MDX).done()]
    # the low words stay close (the second target's anchors start 9 behind the first's last), only the high word cuts
    t = Read().unit(80, 0)
    t.target(1, t.x + STEP - FAR).unit(80)
    t.target(3, t.x + STEP - FAR).unit(2)
    c["cut_by_the_high_word_of_x"] = [t.done()]
    # a unit whose end lies beyond the 64 mask words a wave of k_emit_units holds: the walk over the following words finds it (and
    # twelve short units, so that the batch stays one of short units on average and k_chain_twin takes it)
    c["end_beyond_the_waves_mask_words"] = [Read().unit(4200, 0).singles(2).unit(40).done(),
                                            np.concatenate([Read(1000 + FAR * 3 * i, 1000 + 100 * i).unit(2, 0).done() for i in range(12)])]
    c["singletons_only"] = [Read().singles(100, 0).done(), Read().singles(1, 0).done(), Read().singles(65, 0).done()]
    c["two_anchor_units_back_to_back"] = [np.concatenate([Read(1000 + FAR * 3 * i, 1000 + 100 * i).unit(2, 0).done() for i in range(150)])]
    return c


def _with_span_per_read(reads):
    """The same anchors with q_span 15, 14, 13, 15, ... by read, and a first read that makes sure two table keys exist."""
    out = []
    for i, r in enumerate([Read().unit(10, 0).done()] + list(reads)):
        r = r.copy()
        r[:, 1] = (r[:, 1] & np.uint64(0xffffffff)) | (np.uint64(15 - i % 3) << np.uint64(32))
        out.append(r)
    return out


@pytest.fixture(scope="module")
def dev():
    with chaindp.Device(0, max_anchors=1 << 20, max_reads=1 << 12) as d:
        d.set_ring(128)
        d.set_variant(0)
        yield d


@pytest.fixture(scope="module")
def inputs():
    """{(case, jitter): (par, off, a, f, p, v, [new_seed[] bytes per read])}: built and scored by the oracle once, never written to."""
    out = {}
    for name, reads in _cases().items():
        for jitter in (False, True):
            par = P.preset("ava-ont")
            off, a = batch(_with_span_per_read(reads) if jitter else reads)
            assert len(a) < 6000
            f, p, v, _ = ol.oracle_batch(par, off, a, threads=4)
            seeds = []
            for r in range(len(off) - 1):
                lo, hi = int(off[r]), int(off[r + 1])
                seeds.append(ol.oracle_compact(par, np.ascontiguousarray(a[lo:hi]), f[lo:hi].copy(), p[lo:hi].copy(), v[lo:hi].copy()).tobytes())
            for x in (off, a, f, p, v):
                x.setflags(write=False)
            out[(name, jitter)] = (par, off, a, f, p, v, seeds)
    return out


def test_the_cases_are_what_they_claim():
    """The unit lengths of the built reads, by the definition of a unit (numpy, no GPU involved in it)."""
    par, c = P.preset("ava-ont"), _cases()

    def lens(name):
        off, a = batch(c[name])
        return [int(x) for x in unit_lengths(par, off, a)[0]]

    for k in (1, 2, 63, 64):
        assert lens(f"unit_{k}_singletons_unit") == [70] + [1] * k + [50] + [1] * 5 + [30] + [1] * k + [2] + [1] * k + [90]
    for n in (64, 65, 127, 128, 129):
        assert lens(f"unit_of_{n}_singleton_unit") == [n, 1, 40, 1, 1, 1, n, 1, n]
    assert lens("units_on_read_boundaries") == [100, 70, 1, 1, 70, 64, 129]
    off, a = batch(c["units_on_read_boundaries"])
    assert all(int(a[o, 0] - a[o - 1, 0]) == STEP for o in off[1:-1])          # only the boundary cuts
    assert lens("gap_of_max_dist_x_and_one_more") == [80, 80, 64, 128]
    assert lens("cut_by_the_high_word_of_x") == [80, 80, 2]
    x = batch(c["cut_by_the_high_word_of_x"])[1][:, 0]
    assert int(x[80] & np.uint64(0xffffffff)) - int(x[79] & np.uint64(0xffffffff)) == STEP and int(x[80] >> np.uint64(32)) == 1
    assert lens("end_beyond_the_waves_mask_words") == [4200, 1, 1, 40] + [2] * 12
    assert lens("singletons_only") == [1] * 166
    assert lens("two_anchor_units_back_to_back") == [2] * 150


ROUTES = ["default", "handover_after_first_tile", "one_unit_per_wave"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("jitter", [False, True], ids=["one_span", "span_per_read"])
@pytest.mark.parametrize("name", sorted(_cases()))
def test_unit_ends(dev, inputs, name, jitter, route):
    par, off, a, of, op, ov, exp_seeds = inputs[(name, jitter)]
    dev.set_variant(2 if route == "one_unit_per_wave" else 0)
    dev.set_twin_handover(2 if route == "handover_after_first_tile" else 0)
    try:
        f, p, v = dev.chain_batch(par, off, a)
        took = dev.twin_tables()
        soff, seeds = dev.compact(par)
    finally:
        dev.set_variant(0)
        dev.set_twin_handover(0)
    if route != "one_unit_per_wave" and name != "singletons_only":
        assert took == (2 if jitter else 1), (name, jitter, route, took)   # k_chain_twin ran it, on the layout the case is for
    for what, x, y in (("f", f, of), ("p", p, op), ("v", v, ov)):
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, jitter, route, what, "first mismatch at anchor", int(bad[0]), int(x[bad[0]]), int(y[bad[0]]))
    assert int(soff[-1]) == len(seeds)
    for r, exp in enumerate(exp_seeds):
        assert seeds[int(soff[r]):int(soff[r + 1])].tobytes() == exp, (name, jitter, route, "new_seed[] of read", r)
