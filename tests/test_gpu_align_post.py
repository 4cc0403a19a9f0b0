"""GPU tier of Device.align_post / Device.align_reads_post (chaindp_align_post and its siblings) against the reference's recorded tail of
align_regs and mm_set_mapq (tests/golden/align_post/): every word of the final regions (id, parent, subsc, n_sub, mapq and sam_pri in
the bit-field word), of what r->p held, dp_max2 and every CIGAR word.  The synthetic scenes through the regions-from-the-host form, the
real scenes through align_reads + the resident form and through the one call; batches joined and reversed, read by read, the
capacities with the fetch call, the LDS cap, the refusals, the logf self-tests, steady device memory, other stage calls between."""
import numpy as np
import pytest

import apost_model as M
import apost_shapes as PS
import skeleton_model as K
from test_align_post_cpu import inputs, same
from test_gpu_skeleton import blocks, join

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def check(want, got, label=""):
    """want: dict of M.OUTPUTS (or a golden's *_out); got: the tuple Device.align_post returns."""
    for k, x in zip(M.OUTPUTS, got):
        w = want[k + "_out"] if k + "_out" in want else want[k]
        if not same(x, w):
            bad = np.flatnonzero(x != w)[:4] if x.shape == w.shape else (x.shape, w.shape)
            raise AssertionError((label, k, bad, x[bad] if x.shape == w.shape else None, w[bad] if x.shape == w.shape else None))


def from_host(dev, name, **caps):
    g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
    return g, dev.align_post(PS.post_opt(g["opt"]), rep_len, regs_off, regs, extra, cigar_off, cigar, **caps)


def align_opt(src):
    from minimap2_chaindp_amd import params
    return params.AlignOpt(*(int(v) for v in src["opt"]))


def source(name):
    loader, sub = PS.real_source(name)
    return loader(sub)


@pytest.mark.parametrize("name", PS.SYNTHETIC)
def test_synthetic_scene_from_the_host(dev, name):
    g = PS.load(name)
    builtin = dev.align_post_set_lds_cap(int(g["lds_cap"]))
    try:
        assert 0 < int(g["lds_cap"]) <= builtin == PS.AP_LDS_CAP
        check(*from_host(dev, name), name)
    finally:
        dev.align_post_set_lds_cap(0)


@pytest.mark.parametrize("name", PS.REAL)
def test_real_scene_two_ways(dev, name):
    g, src = PS.load(name), source(name)
    o, po = align_opt(src), PS.post_opt(g["opt"])
    dev.align_set_targets(src["tseq_off"], src["tseq"])
    args = (src["seq_off"], src["seq"], src["a_off"], src["a"], src["regs_off"], src["regs"])
    a, *reads = dev.align_reads(o, *args)
    check(g, dev.align_post(po, g["rep_len"]), name + ": align_reads + the resident align_post")
    # the result of align_reads is still what it was
    off, need = np.zeros(len(src["seq_off"]), np.int64), np.zeros(2, np.int64)
    n, m = len(src["regs_out"]), len(src["cigar_out"])
    from minimap2_chaindp_amd import chaindp
    regs, extra, coff, cig = np.zeros(max(n, 1), chaindp.REG_DTYPE), np.zeros(max(n, 1), chaindp.ALIGN_EXTRA_DTYPE), np.zeros(n + 1, np.int64), np.zeros(max(m, 1), np.uint32)
    p = lambda x: x.ctypes.data
    assert dev._lib.chaindp_align_reads_fetch(dev._ctx, len(off) - 1, p(off), p(regs), p(extra), n, p(coff), p(cig), m, p(need)) == 0
    for k, x in (("regs_off", off), ("regs", regs[:n]), ("extra", extra[:n]), ("cigar_off", coff), ("cigar", cig[:m])):
        assert same(x, src[k + "_out"]) and same(x, reads[("regs_off", "regs", "extra", "cigar_off", "cigar").index(k)]), (name, k)
    a2, *got = dev.align_reads_post(o, po, *args, g["rep_len"])
    check(g, got, name + ": align_reads_post")
    assert same(a2, src["a_out"]) and same(a, src["a_out"])


def synthetic_blocks(name):
    """A synthetic scene read by read: (rep_len, inputs, recorded outputs)."""
    g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
    out = []
    for rd in range(len(rep_len)):
        r0, r1, o0, o1 = (int(x[i]) for x in (regs_off, g["regs_off_out"]) for i in (rd, rd + 1))
        out.append(dict(rep_len=int(rep_len[rd]), regs=regs[r0:r1], extra=extra[r0:r1], cigar=cigar[int(cigar_off[r0]):int(cigar_off[r1])],
                        regs_out=g["regs_out"][o0:o1], extra_out=g["extra_out"][o0:o1], dp_max2_out=g["dp_max2_out"][o0:o1],
                        cigar_out=g["cigar_out"][int(g["cigar_off_out"][o0]):int(g["cigar_off_out"][o1])]))
    return out


def joined(bs):
    cat = lambda k: np.concatenate([b[k] for b in bs])
    return dict(rep_len=np.array([b["rep_len"] for b in bs], np.int32), regs_off=K.offsets([len(b["regs"]) for b in bs]), regs=cat("regs"), extra=cat("extra"),
                cigar_off=K.offsets(cat("extra")["n_cigar"]), cigar=cat("cigar"), regs_off_out=K.offsets([len(b["regs_out"]) for b in bs]), regs_out=cat("regs_out"),
                extra_out=cat("extra_out"), dp_max2_out=cat("dp_max2_out"), cigar_off_out=K.offsets(cat("extra_out")["n_cigar"]), cigar_out=cat("cigar_out"))


def run_joined(dev, opt_row, j, **caps):
    return dev.align_post(PS.post_opt(opt_row), j["rep_len"], j["regs_off"], j["regs"], j["extra"], j["cigar_off"], j["cigar"], **caps)


def test_scenes_of_one_opt_in_one_batch_and_in_reverse_order(dev):
    names = [n for n in PS.SYNTHETIC if same(PS.load(n)["opt"], PS.opt_row(PS.OPT))]
    assert len(names) >= 6
    opt_row = PS.opt_row(PS.OPT)
    bs = [b for n in names for b in synthetic_blocks(n)]
    check(joined(bs), run_joined(dev, opt_row, joined(bs)), "joined")
    check(joined(bs[::-1]), run_joined(dev, opt_row, joined(bs[::-1])), "reversed")


def test_real_scenes_of_one_opt_joined_through_the_one_call(dev):
    groups = {}
    for name in PS.REAL:
        groups.setdefault(tuple(int(v) for v in source(name)["opt"]), []).append(name)
    names = max(groups.values(), key=len)
    assert len(names) >= 5
    for order in (names, names[::-1]):
        parts, rep, want, shift = [], [], [], 0
        for n in order:
            g, src = PS.load(n), source(n)
            bl = blocks(src)
            parts.append((src, bl if order is names else bl[::-1]))
            rds = list(range(len(bl))) if order is names else list(range(len(bl)))[::-1]
            for rd in rds:
                o0, o1 = int(g["regs_off_out"][rd]), int(g["regs_off_out"][rd + 1])
                regs = g["regs_out"][o0:o1].copy(); regs["rid"] += shift
                want.append(dict(rep_len=int(g["rep_len"][rd]), regs=regs[:0], extra=g["extra_out"][:0], cigar=g["cigar_out"][:0], regs_out=regs, extra_out=g["extra_out"][o0:o1],
                                 dp_max2_out=g["dp_max2_out"][o0:o1], cigar_out=g["cigar_out"][int(g["cigar_off_out"][o0]):int(g["cigar_off_out"][o1])]))
            shift += len(src["tseq_off"]) - 1
        j, w = join(parts), joined(want)
        dev.align_set_targets(j["tseq_off"], j["tseq"])
        a, *got = dev.align_reads_post(align_opt(j), PS.post_opt(PS.load(names[0])["opt"]), j["seq_off"], j["seq"], j["a_off"], j["a"], j["regs_off"], j["regs"], w["rep_len"])
        check(w, got, "joined" if order is names else "reversed")
        assert same(a, j["a_out"])


def test_each_read_alone_equals_its_slice_of_the_batched_call(dev):
    for name in ("structure", "inv"):
        g, batched = from_host(dev, name)
        check(g, batched, name)
        for rd, b in enumerate(synthetic_blocks(name)):
            got = run_joined(dev, g["opt"], joined([b]))
            check(joined([b]), got, "%s: read %d alone" % (name, rd))
            o0, o1 = int(batched[0][rd]), int(batched[0][rd + 1])
            assert same(got[1], batched[1][o0:o1]) and same(got[3], batched[3][o0:o1])
            assert same(got[5], batched[5][int(batched[4][o0]):int(batched[4][o1])])


def test_no_reads_and_reads_without_regions(dev):
    from minimap2_chaindp_amd import chaindp
    po = PS.post_opt(PS.opt_row(PS.OPT))
    e = dev.align_post(po, np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, chaindp.REG_DTYPE), np.zeros(0, chaindp.ALIGN_EXTRA_DTYPE), np.zeros(1, np.int64),
                       np.zeros(0, np.uint32))
    assert [len(x) for x in e] == [1, 0, 0, 0, 1, 0]
    e = dev.align_post(po, np.zeros(3, np.int32), np.zeros(4, np.int64), np.zeros(0, chaindp.REG_DTYPE), np.zeros(0, chaindp.ALIGN_EXTRA_DTYPE), np.zeros(1, np.int64),
                       np.zeros(0, np.uint32))
    assert [len(x) for x in e] == [4, 0, 0, 0, 1, 0] and not e[0].any()


def test_capacities_and_fetch(dev):
    from minimap2_chaindp_amd import chaindp
    g = PS.load("structure")
    n_regs, n_words = len(g["regs_out"]), len(g["cigar_out"])
    assert 1 < n_regs < len(g["regs"]) and 1 < n_words < len(g["cigar"])
    for caps in (dict(regs_cap=n_regs - 1, cigar_cap=n_words), dict(regs_cap=n_regs, cigar_cap=n_words - 1), dict(regs_cap=0, cigar_cap=0)):
        with pytest.raises(chaindp.ChainDPError) as e:                    # a caller's cap raises, with what is exact attached
            from_host(dev, "structure", **caps)
        assert "-2" in str(e.value).split(":")[0]
        assert same(e.value.regs_off, g["regs_off_out"]) and e.value.need.tolist() == [n_regs, n_words]
        off, need = np.zeros(len(g["rep_len"]) + 1, np.int64), np.zeros(2, np.int64)
        regs, extra, dp2 = np.zeros(n_regs, chaindp.REG_DTYPE), np.zeros(n_regs, chaindp.ALIGN_EXTRA_DTYPE), np.zeros(n_regs, np.int32)
        coff, cig = np.zeros(n_regs + 1, np.int64), np.zeros(n_words, np.uint32)
        p = lambda x: x.ctypes.data
        rc = dev._lib.chaindp_align_post_fetch(dev._ctx, len(off) - 1, p(off), p(regs), p(extra), p(dp2), n_regs, p(coff), p(cig), n_words, p(need))
        assert rc == 0 and need.tolist() == [n_regs, n_words]
        check(g, (off, regs, extra, dp2, coff, cig), "fetched")
        assert dev._lib.chaindp_align_post_fetch(dev._ctx, len(off), p(off), p(regs), p(extra), p(dp2), n_regs, p(coff), p(cig), n_words, p(need)) == -1
    # a guess that is short is made good by the fetch call
    rows = {k: chaindp._CAPS[k] for k in ("align_post", "align_post_cigar")}
    try:
        chaindp._CAPS.update({k: r._replace(divisor=1 << 30, floored=False) for k, r in rows.items()})      # a guess of one region, one word
        check(*from_host(dev, "structure"), "guessed caps")
    finally:
        chaindp._CAPS.update(rows)


def test_lowered_lds_cap_gives_the_same_words_on_both_routes(dev):
    for name in ("sizes", "lds_cap", "structure"):
        g, at_builtin = from_host(dev, name)
        check(g, at_builtin, name)
        for cap in (1, PS.SCENE_CAP):
            dev.align_post_set_lds_cap(cap)
            try:
                check(g, from_host(dev, name)[1], "%s under cap %d" % (name, cap))
            finally:
                dev.align_post_set_lds_cap(0)


def test_refusals_leave_the_context_usable():
    from minimap2_chaindp_amd import chaindp, params
    with chaindp.Device(0, max_anchors=1 << 12, max_reads=1 << 6) as d:
        before = d.device_bytes()
        g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs("structure")
        po = PS.post_opt(g["opt"])
        with pytest.raises(chaindp.ChainDPError, match="no result of chaindp_align_reads"):
            d.align_post(po, rep_len)                                             # nothing resident
        off, need = np.zeros(1, np.int64), np.zeros(2, np.int64)
        assert d._lib.chaindp_align_post_fetch(d._ctx, 0, off.ctypes.data, None, None, None, 0, None, None, 0, need.ctypes.data) == -1
        assert d.device_bytes() == before
        for change, text in ((dict(flag=0x1000), "MM_F_SR"), (dict(flag=0x80), "MM_F_SPLICE"), (dict(match_sc=0), "match_sc")):
            bad = params.PostOpt(**dict(PS.opt_of(g["opt"]), **change))
            with pytest.raises(chaindp.ChainDPError, match=text):
                d.align_post(bad, rep_len, regs_off, regs, extra, cigar_off, cigar)
        ex = extra.copy(); ex["has_extra"][0] = 3
        with pytest.raises(chaindp.ChainDPError, match="has_extra"):
            d.align_post(po, rep_len, regs_off, regs, ex, cigar_off, cigar)
        ex = extra.copy(); ex["n_cigar"][0] += 1
        with pytest.raises(chaindp.ChainDPError, match="n_cigar"):
            d.align_post(po, rep_len, regs_off, regs, ex, cigar_off, cigar)
        rl = rep_len.copy(); rl[0] = -1
        with pytest.raises(chaindp.ChainDPError, match="rep_len"):
            d.align_post(po, rl, regs_off, regs, extra, cigar_off, cigar)
        assert d.device_bytes() == before                                         # nothing was launched, nothing allocated
        check(g, d.align_post(po, rep_len, regs_off, regs, extra, cigar_off, cigar), "after the refusals")
        # a logf argument beyond the patch range: CHAINDP_ERR_CAPACITY, no result resident, the context usable
        big = extra.copy(); big["dp_max"][0] = (1 << 24) + 1
        with pytest.raises(chaindp.ChainDPError) as e:
            d.align_post(po, rep_len, regs_off, regs, big, cigar_off, cigar)
        assert "-2" in str(e.value).split(":")[0] and "2^24" in str(e.value)
        assert d._lib.chaindp_align_post_fetch(d._ctx, len(rep_len), off.ctypes.data, None, None, None, 0, None, None, 0, need.ctypes.data) == -1
        check(g, d.align_post(po, rep_len, regs_off, regs, extra, cigar_off, cigar), "after the capacity error")
        with pytest.raises(chaindp.ChainDPError, match="not of n_reads"):
            d.align_post(po, rep_len)                                             # still no align_reads result


@pytest.mark.parametrize("match_sc", [1, 2, 4])
def test_logf_selftest(dev, match_sc):
    assert dev.apost_logf_selftest(match_sc, 1 << 24) == 0


def test_device_bytes_are_steady_and_the_ms_hook_reports(dev):
    g, first = from_host(dev, "sizes")
    check(g, first, "sizes")
    steady = dev.device_bytes()
    dev.set_profiling(True)
    try:
        for _ in range(3):
            check(g, from_host(dev, "sizes")[1], "sizes again")
            check(*from_host(dev, "mapq"), "mapq between")
        ms = dev.align_post_ms()
        assert set(ms) == {"read", "gather"} and all(v >= 0 for v in ms.values()), ms
    finally:
        dev.set_profiling(False)
    assert dev.device_bytes() == steady


def test_between_stage_calls_of_other_sizes(dev):
    import test_gpu_ksw as T
    name = "skeleton_fuzz"
    g, src = PS.load(name), source(name)
    o, po = align_opt(src), PS.post_opt(g["opt"])
    args = (src["seq_off"], src["seq"], src["a_off"], src["a"], src["regs_off"], src["regs"])
    dev.align_set_targets(src["tseq_off"], src["tseq"])
    check(g, dev.align_reads_post(o, po, *args, g["rep_len"])[1:], "first")
    k = T.load(T.FUZZ[0])
    T.check(k, *T.call(dev, k))
    check(*from_host(dev, "inv"), "a small batch from the host between")
    dev.align_set_targets(src["tseq_off"], src["tseq"])
    check(g, dev.align_reads_post(o, po, *args, g["rep_len"])[1:], "second")
    T.check(k, *T.call(dev, k))
