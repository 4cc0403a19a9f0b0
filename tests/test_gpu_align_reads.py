"""GPU tier of Device.align_reads (chaindp_align_reads): whole reads in one call against the reference's recorded mm_align_skeleton --
the six scenes of tests/golden/skeleton/ and the edge scenes of tests/golden/align_reads/ -- every word of the final regions, of what
r->p held, every CIGAR word, the anchors with their marks, and through the hook the list as the loop left it for the filter and the
rounds made.  Batches joined and reversed, read by read, the empty call, the two capacities with the fetch call, the refusals, and
the call between stage calls of other sizes on the same context."""
import numpy as np
import pytest

import align_reads_shapes as RS
import skeleton_model as K
from test_gpu_skeleton import blocks, by_opt, check_final, join
from test_skeleton_cpu import NAMES, load, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def opt_of(g):
    from minimap2_chaindp_amd import params
    return params.AlignOpt(*(int(v) for v in g["opt"]))


def call(dev, g, **caps):
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    return dev.align_reads(opt_of(g), g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"], **caps)


def run(dev, g, **caps):
    """One call and the hook's view of it, under the names of skeleton_model.OUTPUTS."""
    a, regs_off, regs, extra, cigar_off, cigar = call(dev, g, **caps)
    placed_off, placed = dev.align_reads_placed()
    return dict(placed_off=placed_off, placed=placed, regs_off=regs_off, regs=regs, extra=extra, cigar_off=cigar_off, cigar=cigar, a=a)


@pytest.mark.parametrize("name", NAMES)
def test_scene_in_one_call(dev, name):
    g = load(name)
    check_final(g, run(dev, g), name)
    rounds = dev.align_reads_rounds()
    assert len(rounds) == int(g["n_calls"]) - 1                           # the recorded calls but the inversion call
    assert int(rounds[0]) == len(g["regs"]) and (np.diff(rounds) <= 0).all() and (rounds > 0).all()


def test_scenes_of_one_opt_in_one_batch_and_in_reverse_order(dev):
    groups = by_opt()
    assert max(len(gs) for gs in groups) >= 5 and len(groups) >= 2
    for gs in groups:
        g = join([(x, blocks(x)) for x in gs])
        check_final(g, run(dev, g), "joined")
        g = join([(x, blocks(x)[::-1]) for x in gs[::-1]])
        check_final(g, run(dev, g), "reversed")


def test_scene_read_by_read_equals_the_batched_call(dev):
    g = load("rounds")
    batched = run(dev, g)
    check_final(g, batched, "batched")
    bs = blocks(g)
    assert len(bs) == 5 and any(len(b["regs"]) == 0 for b in bs)
    for rd, b in enumerate(bs):
        h = join([(g, [b])])
        got = run(dev, h)
        check_final(h, got, "read %d alone" % rd)
        for k, off in (("regs", "regs_off"), ("extra", "regs_off"), ("placed", "placed_off")):
            r0, r1 = (int(batched[off][i]) for i in (rd, rd + 1))
            assert same(got[k], batched[k][r0:r1]), (rd, k)
        c0, c1 = (int(batched["cigar_off"][int(batched["regs_off"][i])]) for i in (rd, rd + 1))
        assert same(got["cigar"], batched["cigar"][c0:c1]) and same(got["a"], batched["a"][int(g["a_off"][rd]):int(g["a_off"][rd + 1])])


@pytest.mark.parametrize("name", RS.NAMES)
def test_edge_scene(dev, name):
    g = RS.load(name)
    builtin = dev.align_reads_set_lds_cap(int(g["lds_cap"]))
    try:
        assert 0 < int(g["lds_cap"]) <= builtin
        check_final(g, run(dev, g), name)
    finally:
        dev.align_reads_set_lds_cap(0)
    if int(g["lds_cap"]) != builtin:                                      # ... and with every list in LDS the same
        check_final(g, run(dev, g), name + ", built-in cap")
    else:                                                                 # ... and the lists of 64 and 65 through the global work arrays
        dev.align_reads_set_lds_cap(RS.SCENE_CAP)
        try:
            check_final(g, run(dev, g), name + ", every longer list on the global route")
        finally:
            dev.align_reads_set_lds_cap(0)


def test_no_reads(dev):
    g = load("asm")
    e = dict(g, seq_off=np.zeros(1, np.int64), seq=g["seq"][:0], a_off=np.zeros(1, np.int64), a=g["a"][:0], regs_off=np.zeros(1, np.int64), regs=g["regs"][:0])
    got = run(dev, e)
    assert [len(got[k]) for k in K.OUTPUTS] == [1, 0, 1, 0, 0, 1, 0, 0] and len(dev.align_reads_rounds()) == 0


def test_capacities_and_fetch(dev):
    from minimap2_chaindp_amd import chaindp
    g = load("fuzz")
    n_regs, n_words = len(g["regs_out"]), len(g["cigar_out"])
    assert n_regs > 1 and n_words > 1
    for caps in (dict(regs_cap=n_regs - 1, cigar_cap=n_words), dict(regs_cap=n_regs, cigar_cap=n_words - 1)):
        with pytest.raises(chaindp.ChainDPError) as e:                    # a caller's cap raises, with what is exact attached
            call(dev, g, **caps)
        assert "-2" in str(e.value).split(":")[0]
        assert same(e.value.regs_off, g["regs_off_out"]) and same(e.value.a, g["a_out"]) and e.value.need.tolist() == [n_regs, n_words]
        # the result is resident: the fetch call delivers it, nothing is computed again (the rounds are the refused call's)
        off, need = np.zeros(len(g["seq_off"]), np.int64), np.zeros(2, np.int64)
        regs, extra = np.zeros(n_regs, chaindp.REG_DTYPE), np.zeros(n_regs, chaindp.ALIGN_EXTRA_DTYPE)
        coff, cig = np.zeros(n_regs + 1, np.int64), np.zeros(n_words, np.uint32)
        p = lambda x: x.ctypes.data
        rc = dev._lib.chaindp_align_reads_fetch(dev._ctx, len(off) - 1, p(off), p(regs), p(extra), n_regs, p(coff), p(cig), n_words, p(need))
        assert rc == 0 and need.tolist() == [n_regs, n_words]
        for k, x in (("regs_off", off), ("regs", regs), ("extra", extra), ("cigar_off", coff), ("cigar", cig)):
            assert same(x, g[k + "_out"]), (caps, k)
        assert dev._lib.chaindp_align_reads_fetch(dev._ctx, len(off), p(off), p(regs), p(extra), n_regs, p(coff), p(cig), n_words, p(need)) == -1
    # a guess that is short is made good by the fetch call
    rows = {k: chaindp._CAPS[k] for k in ("align_reads", "align_reads_cigar")}
    assert all(r.retry == "align_reads_fetch" for r in rows.values())
    try:
        chaindp._CAPS.update({k: r._replace(divisor=1 << 30, floored=False) for k, r in rows.items()})      # a guess of one region, one word
        check_final(g, run(dev, g), "guessed caps")
    finally:
        chaindp._CAPS.update(rows)


def test_fetch_without_a_result_is_refused_and_the_buffers_are_the_loops_own():
    from minimap2_chaindp_amd import chaindp
    g = load("asm")
    with chaindp.Device(0, max_anchors=1 << 12, max_reads=1 << 6) as d:
        before = d.device_bytes()
        off, need = np.zeros(1, np.int64), np.zeros(2, np.int64)
        assert d._lib.chaindp_align_reads_fetch(d._ctx, 0, off.ctypes.data, None, None, 0, None, None, 0, need.ctypes.data) == -1
        assert d.device_bytes() == before                                 # a context that never calls the loop has none of its buffers
        check_final(g, run(d, g), "a fresh context")
        d.align_clear_targets()
        with_loop = d.device_bytes()
        d.align1(opt_of(g), g["seq_off"][:1], g["seq"][:0], g["a_off"][:1], g["a"][:0], g["regs_off"][:1], g["regs"][:0])
        assert with_loop > before and d.device_bytes() == with_loop       # every buffer of the loop is counted, an empty stage call frees none


def test_refusals_leave_the_context_usable(dev):
    from minimap2_chaindp_amd import chaindp
    g = load("asm")
    dev.align_clear_targets()
    with pytest.raises(chaindp.ChainDPError, match="names no target"):
        dev.align_reads(opt_of(g), g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"])
    dev.align_set_targets(g["tseq_off"], g["tseq"])
    for change, text in ((dict(flag=0x1000), "MM_F_SR"), (dict(q2=int(g["opt"][2]), e2=int(g["opt"][3])), "q == q2")):
        o = opt_of(g)
        for k, v in change.items():
            setattr(o, k, v)
        with pytest.raises(chaindp.ChainDPError, match=text):
            dev.align_reads(o, g["seq_off"], g["seq"], g["a_off"], g["a"], g["regs_off"], g["regs"])
    check_final(g, run(dev, g), "after the refusals")


def test_fuzz_twice_with_stage_calls_of_other_sizes_between(dev):
    """The second call finds the context's buffers as calls of other sizes left them, and the stage calls theirs as the loop left them."""
    import test_gpu_ksw as T
    import test_gpu_skeleton as TS
    g, small = load("fuzz"), load("asm")
    check_final(g, run(dev, g), "first")
    k = T.load(T.FUZZ[0])
    T.check(k, *T.call(dev, k))
    check_final(small, TS.run(dev, small, TS.calls_of(small)), "asm through align1 and align1_inv between")
    check_final(g, run(dev, g), "second")
    check_final(g, TS.run(dev, g, TS.calls_of(g)), "the stage calls afterwards")     # every stage call against its own recorded golden
    T.check(k, *T.call(dev, k))
