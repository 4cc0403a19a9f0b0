"""GPU tier of the alignment loop: tests/skeleton_model.run with Device.align1 and Device.align1_inv as its stages, on one context,
against the reference's recorded mm_align_skeleton (tests/golden/skeleton/*.npz) -- every word of the final regions, of what r->p held,
every CIGAR word, the anchors with their marks and the list as the loop left it for the filter -- and, round by round, against what
the CPU models returned for the same call.  The loop code is the one the CPU tier runs (tests/test_skeleton_cpu.py); only the stage
implementation differs."""
import numpy as np
import pytest

import skeleton_model as K
from test_skeleton_cpu import NAMES, calls_of, load, same, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from minimap2_chaindp_amd import chaindp
    with chaindp.Device(0, max_anchors=1 << 16, max_reads=1 << 10) as d:
        yield d


def read_of_row(off, row):
    return int(np.searchsorted(off, row, side="right")) - 1


def first_difference(got, want, off):
    """(row, read) of the first row in which two arrays differ; off the CSR offsets that say which read a row belongs to."""
    if got.shape != want.shape:
        return "shapes", got.shape, want.shape
    g, w = words(got).reshape(len(got), -1), words(want).reshape(len(want), -1)
    row = int(np.flatnonzero((g != w).any(axis=1))[0])
    return dict(row=row, read=read_of_row(off, row), got=got[row], want=want[row])


def device_stages(dev, g, recorded=None):
    """Device.align1 / Device.align1_inv over the scene's targets.  recorded = calls_of(g): every call is compared, as it returns, with
    what the CPU models returned for it; a mismatch names the round and the read."""
    from minimap2_chaindp_amd import params
    o = params.AlignOpt(*(int(v) for v in g["opt"]))
    n = [0]

    def compare(stage, got, a_off=None):
        if recorded is None:
            return
        i, n[0] = n[0], n[0] + 1
        assert i < len(recorded) and recorded[i][0] == stage, ("call", i, stage, "the models made", [s for s, _ in recorded])
        want = recorded[i][1]
        for k, x in got.items():
            if not same(x, want[k]):
                off = a_off if k == "a" else want["cigar_off"][want["regs_off"]] if k == "cigar" else want["regs_off"]
                raise AssertionError((stage, "round", i, k, first_difference(x, want[k], off)))

    def align1_batch(seq_off, seq, a_off, a, regs_off, regs):
        dev.align_set_targets(g["tseq_off"], g["tseq"])
        got = dev.align1(o, seq_off, seq, a_off, a, regs_off, regs)
        compare("align1", dict(zip(("a", "regs", "regs2", "extra", "cigar_off", "cigar"), got), regs_in=regs, regs_off=regs_off), a_off)
        return got

    def inv_batch(seq_off, seq, regs_off, regs):
        dev.align_set_targets(g["tseq_off"], g["tseq"])
        got = dev.align1_inv(o, seq_off, seq, regs_off, regs)
        compare("align1_inv", dict(zip(("made", "r_inv", "extra", "cigar_off", "cigar"), got), regs_in=regs, regs_off=regs_off))
        return got
    return align1_batch, inv_batch


def check_final(g, got, label=""):
    for k in K.OUTPUTS:
        want = g[k + "_out"]
        if not same(got[k], want):
            off = (g["a_off"] if k == "a" else want if k.endswith("_off") else g["placed_off_out"] if k == "placed"
                   else g["cigar_off_out"][g["regs_off_out"]] if k == "cigar" else g["regs_off_out"])
            raise AssertionError((label, k, first_difference(got[k], want, off)))


def run(dev, g, recorded=None):
    return K.run_scene(g, device_stages(dev, g, recorded))


def test_fixtures_are_there():
    assert len(NAMES) == 6


@pytest.mark.parametrize("name", NAMES)
def test_scene_in_one_go_round_by_round(dev, name):
    g = load(name)
    rec = calls_of(g)
    trace = []
    got = K.run_scene(g, device_stages(dev, g, rec), trace=trace)
    assert len(trace) == len(rec)                            # as many rounds as the models made, and the inversion call
    check_final(g, got, name)


# ---- batches: scenes joined, reads reordered, one call per read

def blocks(g):
    """A scene read by read: the read's inputs and its recorded final outputs."""
    out = []
    for rd in range(len(g["seq_off"]) - 1):
        s0, s1, a0, a1, r0, r1, o0, o1, p0, p1 = (int(g[k][i]) for k in ("seq_off", "a_off", "regs_off", "regs_off_out", "placed_off_out")
                                                  for i in (rd, rd + 1))
        c0, c1 = int(g["cigar_off_out"][o0]), int(g["cigar_off_out"][o1])
        out.append(dict(seq=g["seq"][s0:s1], a=g["a"][a0:a1], regs=g["regs"][r0:r1], a_out=g["a_out"][a0:a1], regs_out=g["regs_out"][o0:o1],
                        placed_out=g["placed_out"][p0:p1], extra_out=g["extra_out"][o0:o1], cigar_out=g["cigar_out"][c0:c1]))
    return out


def join(parts):
    """Scenes of one opt as one batch: parts = [(scene, its blocks in the order wanted)].  The targets of every scene are kept, rid shifted
    in the regions and in the anchors' x."""
    tseq, t_off, bl = [], [0], []
    for g, bs in parts:
        shift = len(t_off) - 1
        tseq.append(g["tseq"]); t_off += [t_off[-1] + int(v) for v in g["tseq_off"][1:]]
        for b in bs:
            b = {k: v.copy() for k, v in b.items()}
            for k in ("regs", "regs_out", "placed_out"):
                b[k]["rid"] += shift
            for k in ("a", "a_out"):
                b[k][:, 0] += np.uint64(shift << 32)
            bl.append(b)
    cat = lambda k: np.concatenate([b[k] for b in bl])
    off = lambda k: K.offsets([len(b[k]) for b in bl])
    extra = cat("extra_out")
    return dict(opt=parts[0][0]["opt"], tseq=np.concatenate(tseq), tseq_off=np.array(t_off, np.int64), seq=cat("seq"), seq_off=off("seq"), a=cat("a"),
                a_off=off("a"), regs=cat("regs"), regs_off=off("regs"), a_out=cat("a_out"), regs_out=cat("regs_out"), regs_off_out=off("regs_out"),
                placed_out=cat("placed_out"), placed_off_out=off("placed_out"), extra_out=extra, cigar_out=cat("cigar_out"),
                cigar_off_out=K.offsets(extra["n_cigar"]))


def by_opt():
    groups = {}
    for name in NAMES:
        g = load(name)
        groups.setdefault(tuple(int(v) for v in g["opt"]), []).append(g)
    return list(groups.values())


def test_scenes_of_one_opt_in_one_batch_and_in_reverse_order(dev):
    groups = by_opt()
    assert max(len(gs) for gs in groups) >= 5 and len(groups) >= 2
    for gs in groups:
        g = join([(x, blocks(x)) for x in gs])
        check_final(g, run(dev, g), "joined")
        g = join([(x, blocks(x)[::-1]) for x in gs[::-1]])
        check_final(g, run(dev, g), "reversed")


def test_scene_read_by_read_equals_the_batched_run(dev):
    g = load("rounds")
    batched = run(dev, g)
    check_final(g, batched, "batched")
    bs = blocks(g)
    assert len(bs) == 5 and any(len(b["regs"]) == 0 for b in bs)
    for rd, b in enumerate(bs):
        h = join([(g, [b])])
        got = run(dev, h)                                       # every round and the inversion call with this read alone
        check_final(h, got, "read %d alone" % rd)
        r0, r1 = (int(batched["regs_off"][i]) for i in (rd, rd + 1))
        assert same(got["regs"], batched["regs"][r0:r1]) and same(got["a"], batched["a"][int(g["a_off"][rd]):int(g["a_off"][rd + 1])])


def test_fuzz_twice_with_other_stage_calls_between(dev):
    """The second run finds the context's buffers as calls of other sizes left them."""
    import test_gpu_ksw as T
    g, small = load("fuzz"), load("asm")
    check_final(g, run(dev, g, calls_of(g)), "first")
    k = T.load(T.FUZZ[0])
    T.check(k, *T.call(dev, k))
    check_final(small, run(dev, small), "asm between")
    check_final(g, run(dev, g, calls_of(g)), "second")
