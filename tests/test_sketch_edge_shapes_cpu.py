"""CPU tier of the sketch's edge cases (tests/sketch_edge_shapes.py; the GPU runs them in tests/test_gpu_sketch_edges.py).

  claims       every entry of every case's `props` is measured again here from the model's intermediate quantities -- push ranks
               modulo 8, slot indices modulo 256, l, the emission sites, the spans, the trap counters -- and a few of them a second
               time by plain loops over the bases that share nothing with the model (what a run, a push, a chunk is).
  sensitivity  for the cases about a sequence boundary: the sequence sketched alone and as the tail of its predecessor + itself
               yield different minimizers, so a kernel that let the predecessor leak in would show.
  reference    every case equals the unmodified reference's mm_sketch: live where oracle/_ref is built (and then the live result
               equals the recorded one), through tests/golden/sketch_edges/ref_digests.json where it is not."""
import numpy as np
import pytest

import sketch_edge_shapes as se
import sketch_model as sm
import sketch_ref as sr

NAMES = list(se.CASES)


def test_the_constants_are_the_kernels():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimap2_chaindp_amd", "csrc")
    sk = open(os.path.join(csrc, "chaindp_sketch.hip")).read()
    assert int(re.search(r"#define SK_TILE (\d+)", sk).group(1)) == se.TILE
    assert "wi = rank >> 3" in sk and "wi = s >> 3" in sk and se.WORD == 1 << 3                 # k_sk_kmer, k_sk_value: eight per load
    assert f"blockIdx.x * {se.SCAN_TILE} + threadIdx.x * 4" in open(os.path.join(csrc, "chaindp_compact.hip")).read()        # k_scan_l1


def test_every_issue_shape_has_a_case():
    assert len(NAMES) == 41 and se.BIG in NAMES
    assert se.case("base_lengths").props["lens"] == [1, 255, 256, 257, 511, 512, 513] == se.case("base_lengths_hpc").props["lens"]
    assert {(c.w, c.k) for c in map(se.case, NAMES) if c.props.get("l_after_ambiguous")} == set(se.L_PARAMS)
    assert {(c.w, c.k) for c in map(se.case, NAMES) if c.props.get("l_from_start")} == set(se.L_PARAMS)
    assert {c.k for c in map(se.case, NAMES) if "push0_mod_word" in c.props} == {1, 2, 7, 8, 9, 28}
    assert [se.case(f"read_counts_{n}").props["n_reads"] for n in (255, 256, 257)] == [255, 256, 257]
    assert [se.case(f"scan_chunks_{n}").props["n_chunks_plus_1"] for n in (1024, 1025)] == [1024, 1025]
    assert [se.case(f"scan_slot_tiles_{n}").props["slot_tiles"] for n in (262144, 262145)] == [1024, 1025]
    assert [len(se.case(f"scan_slot_tiles_{n}").seqs[0]) for n in (262144, 262145)] == [262144, 262145]


@pytest.mark.parametrize("name", NAMES)
def test_claims(name):
    c = se.case(name)
    assert c.props, name
    F = se.facts(c.seqs, c.w, c.k, c.is_hpc, c.n_segs)
    for claim, value in c.props.items():
        assert claim in F, f"{name}: {claim} is not a measured fact"
        assert se.holds(value, F[claim]), f"{name}: {claim}: claimed {value}, measured {F[claim]}"


# ---- the same, restated without the model where a plain loop can say it

def _codes(s):
    return [int(sm.NT4[b]) for b in bytes(s)]


def _runs(codes, is_hpc):
    """(start, end, code) of every push: every unambiguous base, or under compression every run of equal ones."""
    out, i = [], 0
    while i < len(codes):
        j = i
        if codes[i] < 4:
            while is_hpc and j + 1 < len(codes) and codes[j + 1] == codes[i]:
                j += 1
            out.append((i, j, codes[i]))
        i = j + 1
    return out


@pytest.mark.parametrize("name", NAMES)
def test_push_ranks_and_chunks_by_a_plain_loop(name):
    c = se.case(name)
    F = se.facts(c.seqs, c.w, c.k, c.is_hpc, c.n_segs)
    push0, first, n_push, quiet, late, chunks = 0, set(), [], 0, 0, 0
    for s in c.seqs:
        codes = _codes(s)
        runs = _runs(codes, c.is_hpc)
        if runs:
            first.add(push0 % 8)
        push0 += len(runs); n_push.append(len(runs))
        late += sum(1 for a, b, _ in runs if a // 256 < b // 256)
        n = max((len(s) + 255) // 256, 1)
        chunks += n
        busy = {b // 256 for _, b, _ in runs} | {i // 256 for i, x in enumerate(codes) if x >= 4}       # chunks with a push end or an N
        quiet += (n if s else 0) - len(busy)
    assert n_push == F["n_push"] and first == F["push0_mod_word"] and chunks + 1 == F["n_chunks_plus_1"]
    assert late == F["runs_started_in_an_earlier_chunk"]
    if not F["trap_symmetric_skipped"]:                              # no symmetric push: a chunk without a push end or an N has no slot
        assert quiet == F["chunks_without_push_or_slot"]


def test_the_homopolymer_runs_sit_where_they_are_claimed():
    for which, (a, b) in (("255_256", (255, 256)), ("chunk", (256, 511)), ("513", (255, 767))):
        s = se.case("hpc_run_" + which).seqs[0]
        assert len(set(s[a:b + 1])) == 1 and s[a - 1] != s[a] and s[b + 1] != s[b], which
    for kind in ("AAA", "byte0"):
        q = se.case("hpc_boundary_" + kind).seqs
        for s0, s1 in ((q[0], q[1]), (q[2], q[3])):
            assert sm.NT4[s0[-1]] == sm.NT4[s1[0]] == 0 and sm.NT4[s0[-3]] == 0 and sm.NT4[s1[2]] == 0 and sm.NT4[s0[-4]] != 0 and sm.NT4[s1[3]] != 0
            assert (s0.endswith(b"\x00\x00\x00") and s1.startswith(b"aaa")) if kind == "byte0" else (s0.endswith(b"AAA") and s1.startswith(b"AAA"))
        assert [len(_runs(_codes(x), 1)) for x in q[:2]] == [19, 19]                # exactly k pushes: the boundary run is in the only k-mer
    s0, s1 = se.case("kmer_across_sequences").seqs
    assert s0.endswith(b"AC") and s1.startswith(b"GT")
    assert b"ACNGT" in se.case("kmer_over_ambiguous").seqs[0]
    for s, run in zip(se.case("hpc_span").seqs, range(235, 240)):
        r = _runs(_codes(s), 1)
        assert [b - a + 1 for a, b, _ in r[:19]] == [1] * 18 + [run]


def test_l_cases_by_a_plain_loop():
    """Slots counted base by base (no symmetric k-mer occurs in these cases: one slot per base)."""
    for w, k in se.L_PARAMS:
        for kind in ("after_ambiguous", "from_start"):
            c = se.case(f"l_{kind}_w{w}_k{k}")
            assert se.facts(c.seqs, c.w, c.k, 0)["trap_symmetric_skipped"] == 0
            g, seen_n, seen_0 = 0, set(), set()
            for s in c.seqs:
                last = None
                for i, x in enumerate(_codes(s)):
                    if x >= 4:
                        last = i
                    elif i == len(s) - 1 or _codes(s[i + 1:i + 2])[0] >= 4:          # a stretch ends here
                        if last is None:
                            seen_0.add((i + 1, g % 8, (g + i) % 8))
                        else:
                            seen_n.add((i - last, (g + last) % 8, (g + i) % 8))
                g += len(s)
            for d in se._distances(w, k):
                got = seen_n if kind == "after_ambiguous" else seen_0
                assert {a for dd, a, _ in got if dd == d} == set(range(8)), (w, k, kind, d)
                assert {b for dd, _, b in got if dd == d} == set(range(8)), (w, k, kind, d)


# ---- sensitivity

@pytest.mark.parametrize("name,i", se.BOUNDARY_CASES)
def test_a_leaking_predecessor_would_show(name, i):
    c = se.case(name)
    pred, s = c.seqs[i - 1], c.seqs[i]
    assert pred and s
    x, y = sm.sketch(s, c.w, c.k, c.is_hpc)
    jx, jy = sm.sketch(pred + s, c.w, c.k, c.is_hpc)
    tail = (jy >> np.uint64(1)) >= np.uint64(len(pred))                    # what the joined sequence yields at the bases of s
    jy = jy[tail] - np.uint64(len(pred) << 1)
    assert len(x) > 0
    assert not (np.array_equal(x, jx[tail]) and np.array_equal(y, jy)), f"{name}: sequence {i} yields the same alone and behind its predecessor"


# ---- the reference

@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_reference(name):
    c = se.case(name)
    theirs = None
    if sr.have():
        seq, seq_off = se.batch(c.seqs)
        theirs = sr.sketch_batch(seq, seq_off, c.w, c.k, c.is_hpc, n_segs_per_read=c.n_segs)
    sr.check(name, se.expected(name), theirs)


def test_the_record_holds_exactly_the_cases():
    assert set(sr.record()) == set(NAMES)
    assert all(sr.record()[n]["n"] == len(se.expected(n)[1]) for n in NAMES)
