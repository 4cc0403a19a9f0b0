"""Inputs of the alignment-loop tests (tests/skeleton_model.py): scenes as align_shapes makes them (targets of 1-4 kb, reads of at most
about 1500 bases, anchors on the true path, regions over them), each at the smallest size that reaches its loop case, and a seeded
fuzz.  Every read's anchors are as mm_squeeze_a leaves them: the regions' anchor ranges follow each other from 0 without a hole.

check() refuses a scene that falls into unspecified behaviour of align1 or align1_inv (align_model.Undefined) or in which a surviving
region would reach the sort without an alignment.  Regions of a read that share the sort key are ordered as the reference's sort
leaves them (skeleton_model.sort_pairs); the scenes here have none, the tie scenes of align_reads_shapes.py do."""
import zlib

import numpy as np

import align_shapes as S
import skeleton_model as K
from align_shapes import rand_seq, rc, read_of, region
from inv_shapes import other


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def compose(rng, tseq, t0, pieces):
    """A read written piece by piece from tseq[t0:]: ("copy", n) exact bases, ("other", n) every base replaced by another one, ("junk", n)
    random bases in the place of n target bases, ("inv", n) the stretch reverse-complemented, ("inv", n, positions) with the bases at these
    positions of it replaced by the next letter, ("del", n), ("ins", n).  Returns (read, path) as align_shapes.mutate does."""
    out, path, t = [], [], t0
    for kind, n, *subs in pieces:
        if kind == "copy":
            out.append(tseq[t:t + n]); path += list(range(t, t + n))
        elif kind == "del":
            t += n
            continue
        else:
            out.append({"other": lambda: other(rng, tseq[t:t + n]), "junk": lambda: rand_seq(rng, n), "ins": lambda: rand_seq(rng, n),
                        "inv": lambda: rc(tseq[t:t + n])}[kind]())
            for q in (subs[0] if subs else ()):
                out[-1] = out[-1][:q] + S.ACGT[(S.ACGT.index(out[-1][q]) + 1) % 4] + out[-1][q + 1:]
            path += [-1] * n
            if kind == "ins":
                continue
        t += n
    return "".join(out), path


def composed(rng, name, targets, rid, t0, pieces, rev=0, step=30, k=15):
    seq, path = compose(rng, targets[rid], t0, pieces)
    a = S.anchors_of(path, k, rid, rev, step)
    return dict(name=name, seq=rc(seq) if rev else seq, a=a, regs=[region(a, len(seq), 0, len(a))])


def two_regions(rd, cut, second=(1, 1)):
    """The read's anchors as two regions, [0, cut) and [cut, n): the second with id and parent `second`."""
    n = len(rd["a"])
    rd["regs"] = [region(rd["a"], len(rd["seq"]), 0, cut), region(rd["a"], len(rd["seq"]), cut, n - cut, id_=second[0], parent=second[1])]
    return rd


def chimera(rng, name, targets, fwd, back):
    """One read on two targets and two strands: targets[fwd[0]][fwd[1]:fwd[2]] forward, then a stretch of another target reverse-complemented.
    The anchors of the second part count from the start of the read's reverse complement, which is where that part begins."""
    s0, p0 = S.mutate(rng, targets[fwd[0]], fwd[1], fwd[2])
    s1, p1 = S.mutate(rng, targets[back[0]], back[1], back[2])
    a0, a1 = S.anchors_of(p0, 15, fwd[0], 0, 30, rng), S.anchors_of(p1, 15, back[0], 1, 30, rng)
    a, seq = np.concatenate([a0, a1]), s0 + rc(s1)
    return two_regions(dict(name=name, seq=seq, a=a, regs=[]), len(a0))


def set_hashes(scene):
    """A hash per read, as mm_gen_regs gives every region of a read a hash of its own; here the read's number decides it."""
    for i, rd in enumerate(scene["reads"]):
        for j, r in enumerate(rd["regs"]):
            r["hash"] = zlib.crc32(b"%d/%d" % (i, j)) & 0x7fffffff
    return scene


def named_scenes():
    rng = np.random.default_rng(20241105)
    T = [rand_seq(rng, 3000), rand_seq(rng, 2000)]
    scenes = []

    def scene(name, opt, reads):
        scenes.append(S._finish(set_hashes(dict(name=name, opt=dict(S.OPTS[opt]), targets=T, reads=reads))))

    # rounds: two inverted stretches give a split of a split and, with the first inversion made, a pair the loop never tests; a read that
    # is done after one round beside them; a junk stretch ahead of an insertion and a deletion close together, whose seeds round 0 marks
    # in what becomes the split-off region's range
    scene("rounds", "lowz", [read_of(rng, "two_inv_fwd", T, 0, 150, 1650, edits=[(600, "inv", 160), (1150, "inv", 160)]),
                             read_of(rng, "plain", T, 1, 300, 700),
                             read_of(rng, "two_inv_rev", T, 0, 1400, 2900, rev=1, edits=[(1850, "inv", 150), (2400, "inv", 170)]),
                             read_of(rng, "marks_behind_drop", T, 1, 100, 1500, sub=0, indel=0, edits=[(500, "junk", 150), (900, "ins", 25), (960, "del", 25)]),
                             dict(name="no_regions", seq=rand_seq(rng, 200), a=np.zeros((0, 2), np.uint64), regs=[])])
    # filters: a split-off tail of 36 matching bases (mlen below min_chain_score), one of 45 in three runs with two mismatches between
    # them (dp_max below min_dp_max), a second region of two anchors (min_cnt), a short first region ahead of a long one (the sort)
    secondary = read_of(rng, "secondary_inv", T, 1, 200, 1300, edits=[(700, "inv", 160)])
    secondary["regs"][0].update(id=1, parent=0)
    small = read_of(rng, "min_cnt", T, 0, 2000, 2600)
    scene("filters", "lowz", [composed(rng, "tail_mlen", T, 0, 300, [("copy", 500), ("junk", 150), ("copy", 36)], step=8),
                              composed(rng, "tail_dp_max", T, 1, 200, [("copy", 500), ("junk", 150), ("copy", 15), ("other", 2), ("copy", 15), ("other", 2), ("copy", 15)], step=8),
                              two_regions(small, len(small["a"]) - 2),
                              two_regions(read_of(rng, "short_first", T, 0, 1000, 1900), 4),
                              secondary,
                              chimera(rng, "two_targets", T, (0, 100, 600), (1, 900, 1700))])
    # inversions: a stretch of 49 bases with three substitutions passes mm_test_zdrop's inversion test on the stretch of the Z-drop and
    # fails align1_inv's on the stretch between the two aligned regions (below min_dp_max), or is too short there for a test at all
    # (an early return on regions the first stage made); the inversion behind it is made
    def low(name, subs, rev):
        return composed(rng, name, T, 0, 200, [("copy", 400), ("inv", 49, subs), ("copy", 350), ("inv", 160), ("copy", 300)], rev=rev)
    scene("inv_edges", "lowz", [low("low_then_made_fwd", [16, 18, 40], 0), low("low_then_made_rev", [16, 35, 38], 1), low("early_then_made", [16, 32, 42], 1)])
    # another scoring set (asm20's, min_dp_max 200): an inverted stretch long enough for it, and a read without one
    scene("asm", "asm", [read_of(rng, "asm_inv", T, 0, 400, 1700, sub=0.01, indel=0.005, edits=[(900, "inv", 300)]),
                         read_of(rng, "asm_plain", T, 1, 1000, 1600, rev=1, sub=0.01, indel=0.005)])
    # the committed scene of the first stage whose reads Z-drop at junk, at an inverted stretch and at a large deletion, now taken to the end
    (zdrop,) = [sc for sc in S.named_scenes() if sc["name"] == "zdrop"]
    scenes.append(dict(zdrop, name="zdrop_to_the_end"))
    return scenes


def fuzz_scene(seed=3, n_reads=30):
    """A few dozen reads on both strands with up to three inverted, junk or deleted stretches each, some as two regions."""
    rng = np.random.default_rng(seed)
    T = [rand_seq(rng, int(n)) for n in rng.integers(1500, 4000, 3)]
    reads = []
    for i in range(n_reads):
        rid = int(rng.integers(0, len(T)))
        ln = min(int(rng.integers(300, 1500)), len(T[rid]) - 20)
        t0 = int(rng.integers(0, len(T[rid]) - ln))
        edits, pos = [], t0 + int(rng.integers(120, 300))
        while pos < t0 + ln - 250 and len(edits) < 3:
            n = int(rng.integers(45, 200))
            edits.append((pos, ["inv", "inv", "junk", "del"][int(rng.integers(0, 4))], n))
            pos += n + int(rng.integers(150, 500))
        rd = read_of(rng, f"fuzz{i}", T, rid, t0, t0 + ln, rev=int(rng.integers(0, 2)), step=int(rng.integers(20, 50)), sub=0.03, indel=0.02, edits=edits)
        n = len(rd["a"])
        if n >= 12 and rng.random() < 0.3:
            two_regions(rd, int(rng.integers(4, n - 4)), second=(1, 1) if rng.random() < 0.5 else (1, 0))
        if n == 0:
            rd["regs"] = []
        reads.append(rd)
    return S._finish(set_hashes(dict(name="fuzz", opt=dict(S.OPTS["lowz"]), targets=T, reads=reads)))


def all_scenes():
    return named_scenes() + [fuzz_scene()]


pack = S.pack


def squeezed(p):
    """Whether mm_squeeze_a would leave the scene's anchors where they are: every read's regions, by `as`, follow each other from 0 to the
    read's last anchor."""
    for rd in range(len(p["seq_off"]) - 1):
        regs = p["regs"][int(p["regs_off"][rd]):int(p["regs_off"][rd + 1])]
        at = 0
        for i in np.argsort(regs["as"], kind="stable"):
            if int(regs["as"][i]) != at:
                return False
            at += int(regs["cnt"][i])
        if len(regs) and at != int(p["a_off"][rd + 1] - p["a_off"][rd]):
            return False
    return True


def check(p, trace=None):
    """The scene through the loop over the CPU models: raises where the scene is refused, returns run()'s outputs otherwise."""
    assert squeezed(p), "the anchors are not as mm_squeeze_a leaves them"
    return K.run_scene(p, trace=trace)           # align_model.Undefined passes through
