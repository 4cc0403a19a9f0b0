"""CPU tier of mapping with base alignment in one call: the composition tests/map_align_model.py (e2e_model with MM_F_CIGAR ->
mm_squeeze_a -> skeleton_model -> apost_model) against the reference's recorded results (tests/golden/map_align/*.npz, made and proven
by tests/golden/make_map_align_golden.py), the classes of the cover table, the hand-off's rule restated the way k_handoff_move states
it, three wrong rules that the scenes must tell from the right one, and the host's checks of the new calls, which need no GPU."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import map_align_model as M
import map_align_shapes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_align")
COMPARED = M.OUTPUTS + ("a_off", "a", "sq_regs_off", "sq_regs", "sq_a_off", "sq_a")
_models = {}


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(name):
    """The composition over a scene, once per process (each takes about ten seconds: the DP model is Python)."""
    if name not in _models:
        _models[name] = M.run(S.scene(name))
    return _models[name]


@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_model_equals_the_reference_in_every_word(name):
    g, m = load(name), model(name)
    for k in COMPARED:
        u, v = np.asarray(m[k]), g[k + "_out"]
        assert u.shape == v.shape and u.tobytes() == v.tobytes(), (name, k)
    assert np.array_equal(m["rep_len"], g["rep_len"]) and int(m["n_anchors"]) == int(g["n_anchors"])


def test_every_class_of_the_cover_table_is_reached_and_the_unreachable_one_is_not():
    total = collections.Counter()
    for name in S.SCENES:
        total.update(model(name)["cover"])
    assert not [k for k in M.COVER if not total[k]], dict(total)
    # joined_then_moved: counted like the others, never seen -- after mm_join_long the skeleton's squeeze rewrites no `as`, it only
    # cuts the tail that mm_select_sub's drops left above the packed anchors
    assert total["joined_then_moved"] == 0 and total["joined_tail_cut"] >= 4


def _post_and_tap(name):
    """A scene's regions and anchors as chain_post leaves them (the model's) and as the reference's squeeze left them (the golden's tap)."""
    import e2e_model as em
    sc = S.scene(name)
    roff, regs, aoff, a, _ = M.chain_post(sc, em.model_of(sc))
    return (roff, regs, aoff, a), load(name)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_kernels_rule_equals_the_references_squeeze_on_every_scene(name):
    (roff, regs, aoff, a), g = _post_and_tap(name)
    got = S.squeeze(roff, regs, aoff, a, rule=S.handoff_read)
    assert got[0].tobytes() == g["sq_regs_out"].tobytes() and np.array_equal(got[1], g["sq_a_off_out"]) and got[2].tobytes() == g["sq_a_out"].tobytes()


def test_the_kernels_rule_equals_mm_squeeze_a_on_the_hand_made_lists():
    ro, r, bo, b = S.synthetic()
    want, got = S.squeeze(ro, r, bo, b), S.squeeze(ro, r, bo, b, rule=S.handoff_read)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(want, got))
    names = list(S.SYNTHETIC)
    assert (want[0]["as"] != r["as"]).sum() > 700                         # nearly every region moves
    n = np.diff(ro)
    for k, v in (("regs_64", 64), ("regs_65", 65), ("regs_5", S.SCENE_CAP), ("regs_6", S.SCENE_CAP + 1), ("regs_256", S.HO_LDS_CAP), ("regs_257", S.HO_LDS_CAP + 1), ("none", 0)):
        assert n[names.index(k)] == v
    for k, v in (("cnt_65", 65), ("cnt_257", 257), ("cnt_64", 64)):
        assert v in r["cnt"][ro[names.index(k)]:ro[names.index(k) + 1]]
    t = names.index("cnt_0_tie")
    assert len(set(r["as"][ro[t]:ro[t + 1]][1:])) == 1                    # equal `as`: the slot decides


def _per_read(name, rule):
    """Per read of a scene: (the read's class facts, whether `rule` gives what the reference's squeeze left)."""
    (roff, regs, aoff, a), g = _post_and_tap(name)
    out = []
    for r in range(len(roff) - 1):
        x, y = regs[roff[r]:roff[r + 1]], a[aoff[r]:aoff[r + 1]]
        if not len(x):
            continue
        gr, ga = rule(x, y)
        t0, t1 = int(g["sq_a_off_out"][r]), int(g["sq_a_off_out"][r + 1])
        same = gr.tobytes() == g["sq_regs_out"][roff[r]:roff[r + 1]].tobytes() and np.asarray(ga).tobytes() == g["sq_a_out"][t0:t1].tobytes()
        in_order = list(np.argsort(x["as"], kind="stable")) == list(range(len(x)))
        kept = in_order and int(x["as"][0]) == 0 and int(x["cnt"].sum()) == len(y)     # region order = anchor order, as 0, nothing to cut
        out.append((kept, len(x), int(x["as"].min()), in_order, same))
    return out


# each wrong rule: equal to the right one on the reads the squeeze leaves alone (`kept`), different on a read of a named scene and class
@pytest.mark.parametrize("rule, scene, cls", [("rank_by_slot", "no-ljoin", "order_differs"), ("keep_as", "map-ont", "one_as_gt0"),
                                              ("skip_one_region", "map-ont", "one_as_gt0")])
def test_a_wrong_rule_passes_where_nothing_moves_and_fails_on_its_scene(rule, scene, cls):
    kept = [x for name in ("ava-ont", "map-ont") for x in _per_read(name, S.wrong(rule)) if x[0]]
    assert len(kept) >= 10 and all(x[4] for x in kept), rule
    assert model(scene)["cover"][cls] > 0
    rows = _per_read(scene, S.wrong(rule))
    hit = [x for x in rows if (not x[3] if cls == "order_differs" else x[1] == 1 and x[2] > 0)]
    assert hit and not any(x[4] for x in hit), (rule, scene, cls)
    assert all(x[4] for x in _per_read(scene, S.handoff_read))               # ... which the right rule gets right


def test_a_golden_belongs_to_its_scene():
    import hashlib
    for name in S.SCENES:
        sc = S.scene(name)
        d = hashlib.sha256(bytes(sc.seq) + bytes(sc.tseq) + sc.seq_off.tobytes() + sc.tseq_off.tobytes() + sc.hash_.tobytes() + sc.bid.tobytes()).digest()
        assert bytes(load(name)["digest"]) == d, name


# ---- the library's host side, without a GPU

def test_the_prototypes_come_from_the_header_and_the_calls_refuse_a_null_context():
    from minimap2_chaindp_amd import _cabi, chaindp
    protos = _cabi.prototypes("chaindp_map_align.h")
    assert {"chaindp_align_resident", "chaindp_map_align_seqs", "chaindp_align_resident_anchors", "chaindp_map_align_debug_set_lds_cap", "chaindp_map_align_debug_ms",
            "chaindp_map_align_debug_handoff", "chaindp_map_align_debug_run_handoff"} == set(protos)
    assert len(protos["chaindp_align_resident"][1]) == 15 and len(protos["chaindp_map_align_seqs"][1]) == 31
    L = chaindp.lib()
    assert L.chaindp_align_resident(*([None] * 3), 0, *([None] * 4), 0, None, None, 0, None, None, None) == -1
    assert L.chaindp_map_align_debug_set_lds_cap(None, 0, None) == -1 and L.chaindp_map_align_debug_ms(None, None) == -1
    for row in ("align_resident", "align_resident_cigar", "map_align_seqs", "map_align_seqs_cigar"):
        assert chaindp._CAPS[row].retry == "align_post_fetch"
    assert hasattr(chaindp.Device, "align_resident") and hasattr(chaindp.Device, "map_align_seqs")
    assert C.sizeof(C.c_void_p) == 8
