"""Constructive inputs for the sketch (csrc/chaindp_sketch.hip): batches of sequences that put a base, a push, a slot or a read exactly
on an edge of the kernels -- the 256-base chunk, the eight codes / flags one load brings, the 256-slot tile with its look-back of w,
the 1024-item tile of the scans -- and the (w, k, is_hpc) no preset reaches (even k, w = 255, w >= k + 2, the bytes 0..3).

A case is (seqs, w, k, is_hpc, n_segs or None, props).  `props` is what the case claims, in the vocabulary of facts(): a set claims
"these are among the measured ones", ("ge", n) "at least n", ("each_ge", n) "every entry at least n", anything else equality.  A constructor measures its own batch with the
CPU model's intermediate quantities (measure(), facts()) and RAISES when a claim does not hold; it never moves to a nearby size.
tests/test_sketch_edge_shapes_cpu.py proves the claims again and holds every case to the reference, tests/test_gpu_sketch_edges.py
runs the cases on the GPU.  Inputs are seeded and deterministic: nothing but the reference's digests is stored.  numpy only.

Slot indices and push ranks are counted over the whole batch, as the kernels count them.  One thing the kernels' edges cannot have:
a sequence with a push always has a slot, because the first push of a sequence is never symmetric (its reverse word holds 3 - c in
the top digit and zeros below, its forward word c in the bottom digit); the slotless reads are therefore the empty ones."""
import collections
import functools

import numpy as np

import sketch_model as sm

TILE = 256            # SK_TILE (chaindp_sketch.hip:39): bases per chunk, slots per tile, threads per block
WORD = 8              # codes per load in k_sk_kmer (chaindp_sketch.hip:136) and flags per load in k_sk_value (chaindp_sketch.hip:199)
SCAN_TILE = 1024      # items per block of k_scan_l1 (chaindp_compact.hip:58), the first level of launch_scan_u64

Case = collections.namedtuple("Case", "seqs w k is_hpc n_segs props")

PH_FIRST_TIE, PH_MIN, PH_RESCAN_TIE, PH_FINAL = 0, 1, 2, 3          # the emission sites, in the order a slot writes them


class EdgeNotReached(ValueError):
    pass


# ---------------------------------------------------------------- measuring a batch with the model's intermediates

def measure(seqs, w, k, is_hpc):
    """Per sequence: where its chunks, pushes and slots start in the batch, and the model's intermediates (sketch_model.sketch's probe)."""
    out, traps = [], {}
    chunk0 = push0 = slot0 = 0
    for s in seqs:
        s = bytes(s)
        pr = {}
        x, _ = sm.sketch(s, w, k, is_hpc, traps=traps, probe=pr)
        code = sm.NT4[np.frombuffer(s, np.uint8)]
        r = dict(len=len(s), chunk0=chunk0, n_chunks=max((len(s) + TILE - 1) // TILE, 1), push0=push0, n_push=pr["n_push"], slot0=slot0,
                 n_mini=len(x), code=code)
        z = np.zeros(0, np.int64)
        if pr["n_push"] == 0:                      # no push: the slots are the ambiguous bases, none has a value
            spos = np.nonzero(code >= 4)[0]
            r.update(spos=spos, is_n=np.ones(len(spos), bool), l=np.zeros(len(spos), np.int64), em_slot=z, em_phase=z, em_target=z,
                     end=np.zeros(len(s), bool), slot_flag=code >= 4, pend=z, pstart=z, sym=np.zeros(0, bool), span=np.zeros(len(spos), np.int64),
                     has=np.zeros(len(spos), bool), v=np.full(len(spos), sm.NONE, np.uint64))
        else:
            assert "spos" in pr                    # a sequence with a push has a slot
            r.update({n: pr[n] for n in ("spos", "is_n", "l", "em_slot", "em_phase", "em_target", "end", "slot_flag", "pend", "pstart", "sym", "span", "has", "v")})
        r["n_slots"] = len(r["spos"])
        out.append(r)
        chunk0 += r["n_chunks"]; push0 += r["n_push"]; slot0 += r["n_slots"]
    return out, traps


def facts(seqs, w, k, is_hpc, n_segs=None):
    """Everything a case may claim, measured."""
    M, traps = measure(seqs, w, k, is_hpc)
    cap = w + k
    dist = {d for d in (1, cap - 2, cap - 1, cap, cap + 1) if d >= 1}
    F = dict(w=w, k=k, is_hpc=int(bool(is_hpc)), n_seqs=len(M), lens=[r["len"] for r in M], empty_at=[i for i, r in enumerate(M) if r["len"] == 0],
             n_push=[r["n_push"] for r in M], n_slots=[r["n_slots"] for r in M], n_mini=[r["n_mini"] for r in M])
    F["n_chunks_plus_1"] = sum(r["n_chunks"] for r in M) + 1
    F["total_slots"] = sum(F["n_slots"])
    F["slot_tiles"] = (F["total_slots"] + TILE - 1) // TILE
    F["total_mini"] = sum(F["n_mini"])
    for name in ("first_window_tie", "old_min_on_new_min", "min_left_window", "rescan_tie", "final", "pending_min_dropped", "final_is_stale",
                 "final_stale_beats_fresh", "span_ge_256_slot", "symmetric_skipped"):
        F["trap_" + name] = traps.get(name, 0)
    # base chunks
    quiet = late = 0
    runs, same_code = set(), 0
    for i, r in enumerate(M):
        for c in range(r["n_chunks"] if r["len"] else 0):
            sl = slice(c * TILE, (c + 1) * TILE)
            quiet += int(r["end"][sl].sum() == 0 and r["slot_flag"][sl].sum() == 0)
        if is_hpc and r["n_push"]:
            late += int((r["pstart"] // TILE < r["pend"] // TILE).sum())
            runs |= {(i, int(a), int(b)) for a, b in zip(r["pstart"], r["pend"]) if b - a >= 255 or a // TILE != b // TILE}
        if i and r["len"] and M[i - 1]["len"] and r["code"][0] < 4 and r["code"][0] == M[i - 1]["code"][-1]:
            same_code += 1
    F.update(chunks_without_push_or_slot=quiet, runs_started_in_an_earlier_chunk=late, long_runs=runs, same_code_across_a_boundary=same_code)
    # push words
    F["push0_mod_word"] = {r["push0"] % WORD for r in M if r["n_push"]}
    F["seqs_with_fewer_than_k_pushes"] = sum(1 for r in M if r["len"] and r["n_push"] < k)
    pal = inside = 0
    for i, r in enumerate(M):
        if i and r["len"] and M[i - 1]["len"]:
            a = np.concatenate((M[i - 1]["code"][-(k - 1):] if k > 1 else M[i - 1]["code"][:0], r["code"][:k - 1]))
            for j in range(len(a) - k + 1):
                m = a[j:j + k]
                pal += int((m < 4).all() and np.array_equal(m, 3 - m[::-1]))
        for p in np.nonzero(r["sym"])[0]:
            if p >= k - 1:
                inside += int((r["code"][r["pend"][p - k + 1]:r["pend"][p] + 1] >= 4).any())
    F.update(palindromes_across_a_boundary=pal, symmetric_pushes_over_an_ambiguous_base=inside)
    # span
    kept = [r["span"][r["has"]] for r in M if r["n_slots"]]
    allsp = [r["span"][(~r["is_n"]) & (r["l"] >= k)] for r in M if r["n_slots"]]
    F["max_span_kept"] = int(max([a.max() for a in kept if len(a)], default=0))
    F["spans_met"] = set(np.concatenate(allsp).tolist()) if allsp else set()
    # l and the flag words
    after_n, from_start, stretch_n, stretch_0, n_runs = set(), set(), set(), set(), set()
    ends_in_n = all_short = 0
    for r in M:
        S, g0 = r["n_slots"], r["slot0"]
        if not S:
            continue
        idx = np.arange(S)
        last_n = idx - r["l"]                                   # -1: none before
        for s in np.nonzero((~r["is_n"]) & np.isin(r["l"], list(dist)))[0]:
            d = int(r["l"][s])
            if last_n[s] >= 0:
                after_n |= {(d, "n", int(g0 + last_n[s]) % WORD), (d, "s", int(g0 + s) % WORD)}
            else:
                from_start |= {(d, "s0", g0 % WORD), (d, "s", int(g0 + s) % WORD)}
        for s in np.nonzero(~r["is_n"])[0]:                     # the last slot of a stretch: how long the stretch is
            if s == S - 1 or r["is_n"][s + 1]:
                (stretch_n if last_n[s] >= 0 else stretch_0).add(int(r["l"][s]))
        run = 0
        for f in list(r["is_n"]) + [False]:
            if f:
                run += 1
            elif run:
                n_runs.add(run); run = 0
        ends_in_n += int(r["code"][-1] >= 4)
        all_short += int((r["l"] < k).all() and r["n_mini"] == 0)
    # an N of the PREVIOUS sequence in the eight-flag word of a sequence's first slot, not directly before it: a look-back that did
    # not mask the flags before the sequence's first slot would take it for the sequence's own and count a longer l
    g_is_n = np.concatenate([r["is_n"] for r in M]) if M else np.zeros(0, bool)
    foreign = set()
    for r in M:
        S, g0 = r["n_slots"], r["slot0"]
        if S and not r["is_n"][:min(S, cap + 1)].any():
            before = np.nonzero(g_is_n[g0 - g0 % WORD:g0])[0]
            first_stretch = S if not r["is_n"].any() else int(np.nonzero(r["is_n"])[0][0])
            if len(before) and g0 % WORD - int(before[-1]) >= 2:
                foreign.add((first_stretch, g0 % WORD - int(before[-1])))
    F["foreign_ambiguous_in_the_first_word"] = foreign
    F.update(l_after_ambiguous=after_n, l_from_start=from_start, stretches_after_ambiguous=stretch_n, stretches_from_start=stretch_0,
             ambiguous_runs=n_runs, seqs_ending_ambiguous=ends_in_n, seqs_with_every_l_below_k=all_short)
    # window
    first_tie, rescan_tie, d255, multi, fin_prev, short_w = set(), set(), set(), 0, 0, 0
    for r in M:
        g0 = r["slot0"]
        first_tie |= {int(g0 + s) % TILE for s in r["em_slot"][r["em_phase"] == PH_FIRST_TIE]}
        rescan_tie |= {int(g0 + s) % TILE for s in r["em_slot"][r["em_phase"] == PH_RESCAN_TIE]}
        cnt = np.bincount(r["em_slot"], minlength=max(r["n_slots"], 1))
        multi += int((cnt > 1).sum())
        for s, t in zip(r["em_slot"], r["em_target"]):
            if cnt[s] == 1 and s - t == 255:
                d255.add(int(g0 + s) % TILE)
        fin = r["em_phase"] == PH_FINAL
        if fin.any() and (g0 + r["n_slots"] - 1) % TILE == 0 and r["em_target"][fin][0] < r["n_slots"] - 1:
            fin_prev += 1
        short_w += int(0 < r["n_slots"] < w and r["n_mini"] > 0)
    reach = 0
    gv = np.concatenate([r["v"] for r in M]) if M else np.zeros(0, np.uint64)
    for r in M:
        if 0 < r["n_slots"] < w and r["n_mini"] and r["slot0"]:
            last = r["slot0"] + r["n_slots"] - 1
            reach += int(gv[max(last - w, 0):r["slot0"]].min(initial=sm.NONE) < r["v"].min())
    F["smaller_value_in_reach_in_the_sequence_before"] = reach
    F.update(first_window_tie_at=first_tie, rescan_tie_at=rescan_tie, single_push_at_distance_255_at=d255, slots_that_push_several=multi,
             last_slot_opens_a_tile_with_the_minimum_before_it=fin_prev, seqs_with_fewer_than_w_slots_and_minimizers=short_w)
    # reads
    segs = [1] * len(M) if n_segs is None else [int(x) for x in n_segs]
    assert sum(segs) == len(M)
    first = np.cumsum([0] + segs)
    F["n_reads"] = len(segs)
    F["n_segs"] = segs
    F["read_slot0_mod_tile"] = {M[first[i]]["slot0"] % TILE for i in range(len(segs)) if sum(M[q]["n_slots"] for q in range(first[i], first[i + 1]))}
    F["slotless_reads"] = [i for i in range(len(segs)) if not sum(M[q]["n_slots"] for q in range(first[i], first[i + 1]))]
    F["reads_with_an_empty_first_segment"] = sum(1 for i in range(len(segs)) if segs[i] > 1 and M[first[i]]["len"] == 0)
    F["slotless_later_segments"] = sum(1 for i in range(len(segs)) for q in range(first[i] + 1, first[i + 1]) if M[q]["n_slots"] == 0)
    return F


def holds(claim, fact):
    if isinstance(claim, (set, frozenset)):
        return claim <= fact
    if isinstance(claim, tuple) and len(claim) == 2 and claim[0] == "ge":
        return fact >= claim[1]
    if isinstance(claim, tuple) and len(claim) == 2 and claim[0] == "each_ge":
        return all(f >= claim[1] for f in fact)
    return claim == fact


def make(seqs, w, k, is_hpc, props, n_segs=None):
    """The case, or EdgeNotReached with the claim that fails."""
    seqs = [bytes(s) for s in seqs]
    F = facts(seqs, w, k, is_hpc, n_segs)
    for name, claim in props.items():
        if not holds(claim, F[name]):
            raise EdgeNotReached(f"{name}: claimed {claim}, measured {F[name]}")
    return Case(seqs, w, k, int(bool(is_hpc)), None if n_segs is None else list(n_segs), props)


# ---------------------------------------------------------------- bases

def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) if n else b""


def no_repeat(rng, n, before=None, after=None):
    """n bases, no two neighbours equal; the first differs from `before`, the last from `after` (single-base runs under compression)."""
    out, prev = [], before
    for i in range(n):
        ban = {prev} | ({after} if i == n - 1 else set())
        c = int(rng.choice([x for x in b"ACGT" if x not in ban]))
        out.append(c); prev = c
    return bytes(out)


def n_slots_of(seq, w, k, is_hpc):
    return measure([seq], w, k, is_hpc)[0][0]["n_slots"]


class Placer:
    """Appends sequences to a batch and, where asked, a filler sequence in front so that a given slot of the sequence gets a given
    batch-wide slot index modulo `mod`.  The filler is a sequence of its own: it changes nothing in the sequence placed."""

    def __init__(self, rng, w, k, is_hpc):
        self.rng, self.par, self.seqs, self.slots = rng, (w, k, is_hpc), [], 0

    def add(self, seq, local=None, target=None, mod=TILE):
        if local is not None:
            need = (target - self.slots - local) % mod
            if need:
                filler = no_repeat(self.rng, need) if self.par[2] else bases(self.rng, need)
                got = n_slots_of(filler, *self.par)
                if got != need:
                    raise EdgeNotReached(f"a filler of {need} bases has {got} slots")
                self.seqs.append(filler); self.slots += got
        self.seqs.append(bytes(seq)); self.slots += n_slots_of(seq, *self.par)


# ---------------------------------------------------------------- base chunks (sk_base, k_sk_push*)

def base_lengths(is_hpc=0):
    rng = np.random.default_rng(101 + is_hpc)
    lens = [1, 255, 256, 257, 511, 512, 513]
    w, k = (5, 19) if is_hpc else (10, 15)
    return make([bases(rng, n) for n in lens], w, k, is_hpc, dict(lens=lens, total_mini=("ge", 50)))


def base_empties():
    rng = np.random.default_rng(102)
    seqs = [b"", bases(rng, 300), b"", bases(rng, 40), b"", b"", b"", bases(rng, 257), b""]
    return make(seqs, 10, 15, 0, dict(empty_at=[0, 2, 4, 5, 6, 8], slotless_reads=[0, 2, 4, 5, 6, 8], total_mini=("ge", 20)))


def base_only_empties():
    return make([b"", b"", b""], 10, 15, 0, dict(empty_at=[0, 1, 2], n_chunks_plus_1=4, total_slots=0, total_mini=0))


def base_no_sequences():
    return make([], 10, 15, 0, dict(n_seqs=0, n_chunks_plus_1=1, total_mini=0))


def hpc_runs(which):
    """A homopolymer run that starts at base 255 and ends at 256 / is the whole chunk 1 / is 513 long from base 255 (chunk 1 inside it)."""
    rng = np.random.default_rng(103)
    start, end = {"255_256": (255, 256), "chunk": (256, 511), "513": (255, 767)}[which]
    x = ord("G")
    seq = no_repeat(rng, start, after=x) + bytes([x]) * (end - start + 1) + no_repeat(rng, 120, before=x)
    claimed = {"255_256": (0, 255, 256), "chunk": (0, 256, 511), "513": (0, 255, 767)}[which]          # stated apart from the construction
    props = dict(long_runs={claimed}, runs_started_in_an_earlier_chunk=1 if which != "chunk" else 0, chunks_without_push_or_slot=1 if which == "513" else 0,
                 total_mini=("ge", 10))
    if which != "255_256":
        props["trap_span_ge_256_slot"] = ("ge", 1)
    else:
        seq = seq[:300]
        props["lens"] = [300]
    return make([seq], 5, 19, 1, props)


def hpc_boundary(kind):
    """A sequence that ends in a run and the next one that begins with the same base: the run must not join across them.  (A start
    base that took the neighbour's for its own would leave pstart[] unwritten: that shows where the buffer holds an earlier batch's
    values, as it does in the GPU tier's order, not in a fresh context whose memory happens to be zero.)"""
    rng = np.random.default_rng(104)
    tail, head = {"AAA": (b"AAA", b"AAA"), "byte0": (b"\x00\x00\x00", b"aaa")}[kind]
    seqs = []
    for n in (18, 45):                                   # 18: exactly k pushes, one k-mer, and the run at the boundary is part of it
        seqs += [no_repeat(rng, n, after=ord("A")) + tail, head + no_repeat(rng, n, before=ord("A"))]
    return make(seqs, 5, 19, 1, dict(same_code_across_a_boundary=("ge", 2), n_push=[19, 19, 46, 46], n_mini=("each_ge", 1), spans_met={21}))


# ---------------------------------------------------------------- push words (k_sk_kmer)

def push_words(k):
    """The first push rank of a sequence at every residue modulo 8, one sequence with fewer than k pushes among them."""
    rng = np.random.default_rng(200 + k)
    n = 8 * ((k + 10) // 8) + 1
    seqs = [bases(rng, n) for _ in range(5)] + [bases(rng, k - 1) if k > 1 else b"NN"] + [bases(rng, n) for _ in range(8)]
    return make(seqs, 3, k, 0, dict(push0_mod_word=set(range(WORD)), seqs_with_fewer_than_k_pushes=1, total_mini=("ge", 14)))


def kmer_across_sequences():
    """..AC | GT.. at k = 4: a k-mer read past the sequence's first push would be the palindrome ACGT and drop a slot."""
    rng = np.random.default_rng(210)
    seqs = [bases(rng, 30) + b"AC", b"GT" + bases(rng, 30)]
    return make(seqs, 2, 4, 0, dict(palindromes_across_a_boundary=("ge", 1), n_mini=("each_ge", 1)))


def kmer_over_ambiguous():
    """..AC N GT.. in one sequence: the k-mer words are not cleared at N, the push of T is symmetric and takes no slot."""
    rng = np.random.default_rng(211)
    return make([bases(rng, 30) + b"ACNGT" + bases(rng, 30)], 2, 4, 0, dict(symmetric_pushes_over_an_ambiguous_base=("ge", 1), total_mini=("ge", 2)))


def pushes_without_slots():
    """AT x 40 at k = 2: every push but the first is symmetric.  80 pushes, one slot (l = 1 < k), no minimizer."""
    return make([b"AT" * 40], 3, 2, 0, dict(n_push=[80], n_slots=[1], n_mini=[0], trap_symmetric_skipped=79))


# ---------------------------------------------------------------- span (k_sk_slots under compression)

def hpc_span():
    """18 single-base runs and one run of 235..239 bases at k = 19: spans 253..257.  255 is kept, 256 leaves an empty window entry."""
    rng = np.random.default_rng(300)
    x = ord("T")
    seqs = [no_repeat(rng, 18, after=x) + bytes([x]) * run + no_repeat(rng, 70, before=x) for run in range(235, 240)]
    return make(seqs, 5, 19, 1, dict(spans_met={253, 254, 255, 256, 257}, max_span_kept=255, trap_span_ge_256_slot=("ge", 2), n_mini=("each_ge", 1)))


# ---------------------------------------------------------------- l and the flag words (k_sk_value)

L_PARAMS = [(1, 1), (10, 15), (255, 28)]


def _distances(w, k):
    return [d for d in (w + k - 2, w + k - 1, w + k, w + k + 1) if d >= 1]


def l_after_ambiguous(w, k):
    """prefix, a run of 1..3 N, then exactly d slots, d = w+k-2 .. w+k+1: the last N and the last slot at every residue modulo 8.
    And: N directly before a slot, a sequence that ends in N, a sequence whose every slot has l < k."""
    rng = np.random.default_rng(400 + w + k)
    seqs, slots, want = [], 0, set()
    for d in _distances(w, k):
        for r in range(WORD):
            nrun = 1 + (r + d) % 3
            pre = (r - slots - (nrun - 1)) % WORD
            seqs.append(bases(rng, pre) + b"N" * nrun + bases(rng, d))
            slots += pre + nrun + d
            want |= {(d, "n", r), (d, "s", (r + d) % WORD)}
    seqs.append(bases(rng, w + k + 3) + b"N")
    seqs.append((bases(rng, k - 1) + b"N") * 4 + bases(rng, k - 1) if k > 1 else b"NNN")
    want |= {(1, "n", r) for r in range(WORD)} | {(1, "s", r) for r in range(WORD)}          # N directly before a slot
    return make(seqs, w, k, 0, dict(l_after_ambiguous=want, stretches_after_ambiguous=set(_distances(w, k)), ambiguous_runs={1, 2, 3},
                                    seqs_ending_ambiguous=("ge", 1), seqs_with_every_l_below_k=("ge", 1), total_mini=("ge", 8)))


def l_from_start(w, k):
    """Sequences of exactly d slots without N, d = w+k-2 .. w+k+1, first and last slot at every residue modulo 8.  The sequence in
    front of each holds one N, j = 2..7 slots before the sequence's first slot and in the same eight-flag word where the residue
    allows it (r >= 2): a look-back that took it for the sequence's own would count l + j - 1."""
    rng = np.random.default_rng(500 + w + k)
    seqs, slots, want, foreign = [], 0, set(), set()
    for d in _distances(w, k):
        for r in range(WORD):
            j = 2 + (d + r) % (r - 1) if r >= 2 else 1                  # the N sits j slots before the first slot
            q = (r - slots - j) % WORD
            seqs.append(bases(rng, q) + b"N" + bases(rng, j - 1)); slots += q + j
            seqs.append(bases(rng, d)); slots += d
            want |= {(d, "s0", r), (d, "s", (r + d - 1) % WORD)}
            if r >= 2:
                foreign.add((d, j))
    for d in _distances(w, k):
        if len({j for dd, j in foreign if dd == d}) < 2:
            raise EdgeNotReached("the N in front is not at several distances")
    return make(seqs, w, k, 0, dict(l_from_start=want, stretches_from_start=set(_distances(w, k)), foreign_ambiguous_in_the_first_word=foreign,
                                    total_mini=("ge", 8)))


# ---------------------------------------------------------------- window (k_sk_window)

def _tandem(rng, n):
    out = bytearray()
    while len(out) < n:
        r = rng.random()
        if r < 0.5:
            out += bases(rng, int(rng.integers(1, 7))) * int(rng.integers(3, 12))
        else:
            out += bases(rng, int(rng.integers(5, 40)))
    return bytes(out[:n])


def _find(w, k, is_hpc, seed, gen, event, tries=400):
    """The first generated sequence in which `event` (probe -> local slot index or None) happens; deterministic."""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        s = gen(rng)
        pr = {}
        sm.sketch(s, w, k, is_hpc, probe=pr)
        j = event(pr) if "em_slot" in pr else None
        if j is not None:
            return s, int(j)
    raise EdgeNotReached("no sequence with the event in %d tries" % tries)


def _slot_of_phase(ph):
    def event(pr):
        s = pr["em_slot"][pr["em_phase"] == ph]
        return s[0] if len(s) else None
    return event


def window_ties():
    """First-window ties (l == w+k-1, a tandem repeat with a period below w) and rescan ties, each at slot 255 and at slot 0 of a tile:
    slots that push more than one minimizer (the slow path of the emit pass)."""
    w, k = 10, 15
    rng = np.random.default_rng(600)
    unit = None
    for _ in range(50):
        u = bases(rng, 3)
        s = u * 40
        pr = {}
        sm.sketch(s, w, k, 0, probe=pr)
        if (pr["em_phase"] == PH_FIRST_TIE).any():
            unit = s; j_first = int(pr["em_slot"][pr["em_phase"] == PH_FIRST_TIE][0])
            break
    if unit is None or j_first != w + k - 2:
        raise EdgeNotReached("no first-window tie at l == w+k-1 in a repeat of period 3")
    rs, j_rescan = _find(w, k, 0, 601, lambda g: _tandem(g, 200), _slot_of_phase(PH_RESCAN_TIE))
    p = Placer(rng, w, k, 0)
    p.add(unit, j_first, TILE - 1); p.add(unit, j_first, 0)
    p.add(rs, j_rescan, TILE - 1); p.add(rs, j_rescan, 0)
    return make(p.seqs, w, k, 0, dict(first_window_tie_at={TILE - 1, 0}, rescan_tie_at={TILE - 1, 0}, slots_that_push_several=("ge", 4)))


def window_w255():
    """w = 255: a minimum that leaves the window having pushed once, by the slot that opens a tile: distance 255, P in the tile before."""
    w, k = 255, 15

    def event(pr):
        cnt = np.bincount(pr["em_slot"])
        for s, t in zip(pr["em_slot"], pr["em_target"]):
            if cnt[s] == 1 and s - t == 255:
                return s
        return None
    s, j = _find(w, k, 0, 610, lambda g: bases(g, 560), event)
    p = Placer(np.random.default_rng(611), w, k, 0)
    p.add(s, j, 0)
    return make(p.seqs, w, k, 0, dict(single_push_at_distance_255_at={0}, trap_min_left_window=("ge", 1)))


def window_w1():
    """w = 1: every entry is its window's minimum.  The entry before the N is pending when the N comes and is dropped (l == 0 there)."""
    rng = np.random.default_rng(620)
    return make([bases(rng, 150) + b"N" + bases(rng, 150), bases(rng, 15), bases(rng, 16)], 1, 15, 0, dict(w=1, n_mini=[271, 1, 2], trap_pending_min_dropped=1))


def window_short_repeats():
    """The same 17-base sequence five times at (19, 15): fewer than w slots each, the previous sequence's slots hold equal values.
    Equal values cannot show in the final minimum (the rightmost smallest is the sequence's own), so two more sequences follow, the
    first with a smaller value within w slots of the second's last slot: a window that did not stop at the sequence's first slot
    would end on it."""
    rng = np.random.default_rng(630)
    s = bases(rng, 17)
    for _ in range(200):                                 # and a pair where the sequence in front holds the smaller value
        a, b = bases(rng, 17), bases(rng, 17)
        if sm.sketch(a, 19, 15, 0)[0].min() < sm.sketch(b, 19, 15, 0)[0].min():
            break
    return make([s] * 5 + [a, b], 19, 15, 0, dict(seqs_with_fewer_than_w_slots_and_minimizers=7, n_slots=[17] * 7,
                                                  smaller_value_in_reach_in_the_sequence_before=("ge", 1)))


def window_last_slot_opens_tile():
    """The last slot of a sequence at slot 0 of a tile, the current minimum in the tile before it."""
    w, k = 10, 15

    def event(pr):
        fin = pr["em_phase"] == PH_FINAL
        S = len(pr["spos"])
        return S - 1 if fin.any() and pr["em_target"][fin][0] < S - 1 else None
    s, j = _find(w, k, 0, 640, lambda g: bases(g, 120), event)
    p = Placer(np.random.default_rng(641), w, k, 0)
    p.add(s, j, 0)
    p.add(bases(p.rng, 50))
    return make(p.seqs, w, k, 0, dict(last_slot_opens_a_tile_with_the_minimum_before_it=1))


def window_stale_final():
    """w >= k + 2: the final minimum is an entry from before the last N, once with nothing fresh behind it and once beating fresh ones."""
    w, k = 19, 15
    out = []
    for fresh, seed in ((False, 650), (True, 651)):
        rng = np.random.default_rng(seed)
        for _ in range(400):
            s = bases(rng, 60) + b"N" + bases(rng, 16 if fresh else 5)
            tr = {}
            sm.sketch(s, w, k, 0, traps=tr)
            if tr.get("final_is_stale", 0) and bool(tr.get("final_stale_beats_fresh", 0)) == fresh:
                out.append(s)
                break
        else:
            raise EdgeNotReached("no stale final minimum")
    return make(out, w, k, 0, dict(trap_final_is_stale=2, trap_final_stale_beats_fresh=1))


# ---------------------------------------------------------------- read offsets and scans (k_sk_read_off, launch_scan_u64)

def read_first_slots():
    """Reads whose first slot is slot 0, 1 and 255 of a tile."""
    rng = np.random.default_rng(700)
    lens = [1, 254, 300, 213, 40]                        # first slots 0, 1, 255, 555 = 43, 768 = 0
    return make([bases(rng, n) for n in lens], 10, 15, 0, dict(lens=lens, read_slot0_mod_tile={0, 1, TILE - 1}, total_mini=("ge", 50)))


def read_counts(n):
    """n reads of eight bases: the grid of k_sk_read_off is (n + 256) / 256 blocks and thread n writes the total."""
    rng = np.random.default_rng(710 + n)
    return make([bases(rng, 8) for _ in range(n)], 2, 3, 0, dict(n_reads=n, total_mini=("ge", n)))


def scan_chunks(n):
    """n_chunks + 1 == n: the scans over the chunks fill one tile of launch_scan_u64 exactly / need a second one."""
    rng = np.random.default_rng(720 + n)
    return make([bases(rng, 8) for _ in range(n - 1)], 2, 3, 0, dict(n_chunks_plus_1=n, total_mini=("ge", n)))


def scan_slot_tiles(n_bases):
    """One sequence of n_bases bases (an N every 1000th) at (5, 15): one slot per base, n_bases / 256 tiles of slots to scan."""
    rng = np.random.default_rng(730)
    s = np.frombuffer(bases(rng, n_bases), np.uint8).copy()
    s[999::1000] = ord("N")
    tiles = (n_bases + TILE - 1) // TILE
    return make([s.tobytes()], 5, 15, 0, dict(total_slots=n_bases, slot_tiles=tiles, total_mini=("ge", n_bases // 8)))


def multi_segment():
    """Reads of 1..3 segments; one has an empty first segment, one a slotless (empty) later one."""
    rng = np.random.default_rng(740)
    segs = [1, 2, 3, 2, 3, 1, 2]
    lens = [80, 60, 70, 0, 90, 50, 100, 0, 40, 0, 66, 257, 256, 33]
    return make([bases(rng, n) for n in lens], 10, 15, 0, dict(n_segs=segs, n_reads=7, reads_with_an_empty_first_segment=1, slotless_later_segments=2,
                                                              total_mini=("ge", 100)), n_segs=segs)


# ---------------------------------------------------------------- the cases, in constructor order

BIG = "scan_slot_tiles_262145"

CASES = collections.OrderedDict()
PARAMS = {}                            # name -> (w, k, is_hpc, multi-segment): known without building the case


def _reg(name, fn, w, k, is_hpc=0, multi=False):
    CASES[name], PARAMS[name] = fn, (w, k, is_hpc, multi)


_reg("base_lengths", functools.partial(base_lengths, 0), 10, 15)
_reg("base_lengths_hpc", functools.partial(base_lengths, 1), 5, 19, 1)
_reg("base_empties", base_empties, 10, 15)
_reg("base_only_empties", base_only_empties, 10, 15)
_reg("base_no_sequences", base_no_sequences, 10, 15)
for _w in ("255_256", "chunk", "513"):
    _reg("hpc_run_" + _w, functools.partial(hpc_runs, _w), 5, 19, 1)
for _w in ("AAA", "byte0"):
    _reg("hpc_boundary_" + _w, functools.partial(hpc_boundary, _w), 5, 19, 1)
for _k in (1, 2, 7, 8, 9, 28):
    _reg(f"push_words_k{_k}", functools.partial(push_words, _k), 3, _k)
_reg("kmer_across_sequences", kmer_across_sequences, 2, 4)
_reg("kmer_over_ambiguous", kmer_over_ambiguous, 2, 4)
_reg("pushes_without_slots", pushes_without_slots, 3, 2)
_reg("hpc_span", hpc_span, 5, 19, 1)
for _w, _k in L_PARAMS:
    _reg(f"l_after_ambiguous_w{_w}_k{_k}", functools.partial(l_after_ambiguous, _w, _k), _w, _k)
    _reg(f"l_from_start_w{_w}_k{_k}", functools.partial(l_from_start, _w, _k), _w, _k)
_reg("window_ties", window_ties, 10, 15)
_reg("window_w255", window_w255, 255, 15)
_reg("window_w1", window_w1, 1, 15)
_reg("window_short_repeats", window_short_repeats, 19, 15)
_reg("window_last_slot_opens_tile", window_last_slot_opens_tile, 10, 15)
_reg("window_stale_final", window_stale_final, 19, 15)
_reg("read_first_slots", read_first_slots, 10, 15)
for _n in (255, 256, 257):
    _reg(f"read_counts_{_n}", functools.partial(read_counts, _n), 2, 3)
for _n in (SCAN_TILE, SCAN_TILE + 1):
    _reg(f"scan_chunks_{_n}", functools.partial(scan_chunks, _n), 2, 3)
for _n in (SCAN_TILE * TILE, SCAN_TILE * TILE + 1):
    _reg(f"scan_slot_tiles_{_n}", functools.partial(scan_slot_tiles, _n), 5, 15)
_reg("multi_segment", multi_segment, 10, 15, 0, True)
assert BIG in CASES

# the cases whose point is that a predecessor must not leak into a sequence: (case, index of the sequence)
BOUNDARY_CASES = [("hpc_boundary_AAA", 1), ("hpc_boundary_byte0", 1), ("hpc_boundary_AAA", 3), ("hpc_boundary_byte0", 3), ("window_short_repeats", 6), ("kmer_across_sequences", 1), ("window_short_repeats", 1), ("window_short_repeats", 4)]


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    assert (c.w, c.k, c.is_hpc, c.n_segs is not None) == PARAMS[name], name
    return c


def batch(seqs):
    return np.frombuffer(b"".join(seqs), np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def expected(name):
    """mini_off, mini of the case by the CPU model (computed once, shared, never changed: the arrays are read-only)."""
    c = case(name)
    seq, seq_off = batch(c.seqs)
    off, mini = sm.sketch_batch(seq, seq_off, c.w, c.k, c.is_hpc, n_segs_per_read=c.n_segs)
    off.setflags(write=False); mini.setflags(write=False)
    return off, mini
