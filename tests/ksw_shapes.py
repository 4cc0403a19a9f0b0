"""The named problems of the alignment tests (ksw_extd2_sse) and the seeded fuzz batch, as plain inputs.

tests/golden/make_ksw_golden.py runs the reference over them and records inputs and answers under tests/golden/ksw/; the tests read
those files.  A problem is a dict: name, query, target (uint8 codes 0..4), scoring (a key of ksw_model.SCORING or a tuple),
w, zdrop, end_bonus, flag.  groups() sorts them by scoring set, because one call has one scoring set."""
import zlib

import numpy as np

import ksw_model as M

# what the device routes by (chaindp_ksw_debug_routing; tests/test_ksw_cpu.py holds these to the library's): a problem keeps its state
# in LDS while PER_TARGET * T + PER_QUERY * Q + FIXED <= LDS_BUDGET, T and Q the lengths rounded up to 16
# a problem in LDS whose sum is above WIDE_BYTES gets WIDE_WAVES waves instead of one
LDS_BUDGET, PER_TARGET, PER_QUERY, FIXED, WIDE_BYTES, WIDE_WAVES = 65536, 12, 1, 16, 8192, 4
ROUTE_NONE, ROUTE_LDS, ROUTE_GLOBAL, ROUTE_WIDE = 0, 1, 2, 3

SCORING = dict(M.SCORING)
SCORING["swapped"] = (2, 4, 24, 1, 4, 2)        # the default's two gap costs the other way round: :70 swaps them
SCORING["early"] = (1, 19, 4, 2, 24, 1)         # b > 2 (q + e): the reference returns before it computes anything

FLAG_COMBOS = [f for f in range(256) if not f & ~M.ACCEPTED_FLAGS]      # the 32 combinations of the five accepted bits
FUZZ_W = (-1, 0, 1, 2, 3, 5, 8, 15, 16, 17, 31, 40, 500)
FUZZ_ZDROP = (-1, 5, 20, 100, 400)
FUZZ_FLAGS = (0, 0x01, 0x02, 0x08, 0x40, 0xc2)


def state_bytes(qlen, tlen):
    return PER_TARGET * ((tlen + 15) // 16 * 16) + PER_QUERY * ((qlen + 15) // 16 * 16) + FIXED


def expected_route(qlen, tlen, scoring):
    a, b, q, e, q2, e2 = SCORING[scoring] if isinstance(scoring, str) else scoring
    if qlen == 0 or tlen == 0 or b > 2 * min(q + e, q2 + e2):
        return ROUTE_NONE
    need = state_bytes(qlen, tlen)
    return ROUTE_LDS if need <= WIDE_BYTES else ROUTE_WIDE if need <= LDS_BUDGET else ROUTE_GLOBAL


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def rand_seq(rng, n, letters=4):
    return rng.integers(0, letters, n).astype(np.uint8)


def mutate(rng, seq, sub=0.08, indel=0.04, max_indel=3):
    """A relative of seq: substitutions, and insertions / deletions of 1..max_indel bases."""
    out, i = [], 0
    while i < len(seq):
        x = rng.random()
        if x < indel / 2:
            i += int(rng.integers(1, max_indel + 1))
        elif x < indel:
            out.extend(rng.integers(0, 4, int(rng.integers(1, max_indel + 1))))
        elif x < indel + sub:
            out.append((int(seq[i]) + int(rng.integers(1, 4))) % 4); i += 1
        else:
            out.append(int(seq[i])); i += 1
    return np.array(out, np.uint8)


def fit(rng, seq, n):
    """seq cut or padded with random bases to n."""
    return np.concatenate([seq[:n], rand_seq(rng, max(0, n - len(seq)))]).astype(np.uint8)


def pair(name, qlen, tlen, **kw):
    """A query of qlen and a related target of tlen."""
    rng = _rng(name)
    q = rand_seq(rng, qlen)
    return q, fit(rng, mutate(rng, q, **kw), tlen)


def named_cases():
    out = []

    def add(name, q, t, scoring="default", w=-1, zdrop=-1, end_bonus=-1, flag=0):
        out.append(dict(name=name, query=np.asarray(q, np.uint8), target=np.asarray(t, np.uint8), scoring=scoring, w=w, zdrop=zdrop,
                        end_bonus=end_bonus, flag=flag))

    # sizes: the 16-byte word, the wave and two waves, tlen a multiple of 16 against tlen % 16 == 1, qlen - tlen of either sign
    for ql, tl in ((1, 1), (1, 37), (37, 1), (2, 16), (16, 2), (15, 15), (16, 16), (17, 17), (15, 17), (17, 15), (16, 33), (33, 16), (63, 63), (64, 64),
                   (65, 65), (63, 65), (65, 64), (64, 81), (127, 127), (128, 128), (129, 129), (128, 113), (113, 128), (129, 97), (97, 144)):
        q, t = pair(f"size_{ql}x{tl}", ql, tl)
        for flag in (0, 0x40):
            add(f"size_{ql}x{tl}_f{flag:02x}", q, t, flag=flag, zdrop=400 if flag else -1)
    # band: st > en sets zdropped for the narrow ones where the lengths differ
    for ql, tl in ((70, 75), (75, 70), (60, 90), (64, 64)):
        q, t = pair(f"band_{ql}x{tl}", ql, tl)
        for w in (-1, 0, 1, 2, 15, 16, 17, 90, 200):
            add(f"band_{ql}x{tl}_w{w}", q, t, w=w)
    # the scoring sets, the swap among them, and gaps around long_thres under each: the second gap cost takes over
    for sc in ("default", "asm5", "asm10", "asm20", "sr", "swapped"):
        a, b, q_, e, q2, e2 = SCORING[sc]
        if q2 + e2 < q_ + e:
            q_, e, q2, e2 = q2, e2, q_, e
        lt, _ = M.long_gap(q_, e, q2, e2)
        q, t = pair(f"sc_{sc}", 100, 110)
        for flag in (0, 0x02, 0x40):
            add(f"sc_{sc}_f{flag:02x}", q, t, scoring=sc, flag=flag, zdrop=200 if flag else -1, end_bonus=10)
        for L in (lt - 1, lt, lt + 1, lt + 12):
            rng = _rng(f"long_{sc}_{L}")
            core = rand_seq(rng, 90)
            with_gap = np.concatenate([core[:45], rand_seq(rng, L), core[45:]])
            add(f"longdel_{sc}_{L}", core, with_gap, scoring=sc)             # the target has L bases more: a deletion
            add(f"longins_{sc}_{L}", with_gap, core, scoring=sc, flag=0x02)  # the query has: an insertion
    # the wildcard
    q, t = pair("wild", 80, 84)
    qn, tn = q.copy(), t.copy()
    qn[[3, 30, 31, 79]] = 4
    tn[[0, 17, 50, 51, 52, 83]] = 4
    add("wild_query", qn, t); add("wild_target", q, tn); add("wild_both", qn, tn); add("wild_all", np.full(20, 4), np.full(23, 4))
    # ties of H across t mod 4
    for name, q, t in (("homo", np.zeros(40), np.zeros(44)), ("homo_sq", np.ones(48), np.ones(48)), ("two", np.tile([0, 1], 24), np.tile([0, 1], 26)),
                       ("two_shift", np.tile([0, 1], 24), np.tile([1, 0], 25)), ("three", np.tile([0, 0, 1], 20), np.tile([0, 1, 1], 20)),
                       ("homo_vs_other", np.zeros(33), np.ones(35))):
        for w in (-1, 5):
            for flag in (0, 0x40, 0xc2):
                add(f"tie_{name}_w{w}_f{flag:02x}", q, t, w=w, flag=flag, zdrop=100)
        for sc in ("asm20", "sr"):
            add(f"tie_{name}_{sc}", q, t, scoring=sc, flag=0x40, zdrop=50, end_bonus=10)
    # Z-drop in mid-matrix: a related head, then unrelated tails
    for zd, junk in ((5, 40), (20, 80), (100, 320)):
        rng = _rng(f"zdrop_{zd}")
        head = rand_seq(rng, 60)
        q, t = np.concatenate([head, rand_seq(rng, junk)]), np.concatenate([mutate(rng, head), rand_seq(rng, junk + 7)])
        for flag in (0, 0x40, 0xc2):
            add(f"zdrop_{zd}_f{flag:02x}", q, t, zdrop=zd, flag=flag, w=100)
    # end bonus: the extension reaches the query's end (reach_end 1) or stops at the maximum
    for eb in (10, -1):
        rng = _rng(f"endbonus_{eb}")
        head = rand_seq(rng, 70)
        tgt = np.concatenate([mutate(rng, head, sub=0.03, indel=0.0), rand_seq(rng, 20)])
        add(f"endbonus_{eb}_reach", head, tgt, scoring="sr", flag=0x40, end_bonus=eb, zdrop=100)
        bad = head.copy(); bad[-6:] = (bad[-6:] + 1) % 4          # a bad last stretch: the maximum lies before the query's end
        add(f"endbonus_{eb}_short", bad, np.concatenate([head, rand_seq(rng, 20)]), scoring="sr", flag=0x40, end_bonus=eb, zdrop=100)
        bad2 = head.copy(); bad2[-2:] = (bad2[-2:] + 1) % 4       # two mismatches: worth it with the bonus only
        add(f"endbonus_{eb}_edge", bad2, np.concatenate([head, rand_seq(rng, 20)]), scoring="sr", flag=0x40, end_bonus=eb, zdrop=100)
    # flag combinations: all 32 on one input; the gap fill's approximate pass followed by the exact one
    q, t = pair("flags", 50, 55)
    for f in FLAG_COMBOS:
        add(f"flags_{f:02x}", q, t, flag=f, zdrop=400, end_bonus=-1, w=40)
    # early returns: empty problems between full ones; the scoring set that returns early
    q, t = pair("empty", 30, 30)
    add("empty_q", np.zeros(0), t); add("empty_between", q, t); add("empty_t", q, np.zeros(0)); add("empty_both", np.zeros(0), np.zeros(0))
    add("early_a", q, t, scoring="early"); add("early_b", t, q, scoring="early", flag=0x40); add("early_empty", np.zeros(0), t, scoring="early")
    # larger problems: many 64-cell steps per diagonal
    q, t = pair("large_2000x2100", 2000, 2100, sub=0.06, indel=0.04)
    add("large_2000x2100_w500", q, t, w=500, zdrop=400, flag=0x40)
    q, t = pair("large_600x600", 600, 600)
    add("large_600x600", q, t)
    # ... and, past WIDE_BYTES, several waves per diagonal: every flag path, ties, the band running out, Z-drop
    q, t = pair("wide_700x705", 700, 705)
    for flag, w in ((0, -1), (0x02, 100), (0x08, 100), (0x01, 64), (0x09, 64), (0xc2, 300), (0x40, 17), (0, 2)):
        add(f"wide_700x705_f{flag:02x}_w{w}", q, t, flag=flag, w=w, zdrop=400, end_bonus=10)
    add("wide_tie_homo", np.zeros(720), np.zeros(724), w=70, flag=0x40, zdrop=100)
    add("wide_tie_two", np.tile([0, 1], 350), np.tile([0, 1], 352), w=200)
    rng = _rng("wide_zdrop")
    head = rand_seq(rng, 300)
    add("wide_zdrop", np.concatenate([head, rand_seq(rng, 500)]), np.concatenate([mutate(rng, head), rand_seq(rng, 520)]), zdrop=100, flag=0x40, w=400)
    q, t = pair("wide_asm", 690, 720, max_indel=40)
    add("wide_asm5", q, t, scoring="asm5", w=300); add("wide_sr", q, t, scoring="sr", flag=0x40, zdrop=100, end_bonus=10, w=150)
    # routes: exactly on each routing constant, one 16-base step below it and one above; a plainly global one
    for what, limit in (("wide", WIDE_BYTES), ("lds", LDS_BUDGET)):
        tl = (limit - FIXED) // PER_TARGET // 16 * 16 - 16
        q_on = (limit - FIXED - PER_TARGET * tl) // PER_QUERY
        assert q_on % 16 == 0 and q_on >= 32 and state_bytes(q_on, tl) == limit
        for tag, ql in (("below", q_on - 16), ("on", q_on), ("above", q_on + 1)):
            q, t = pair(f"route_{what}_{tag}", ql, tl, sub=0.03, indel=0.01)
            add(f"route_{what}_{tag}_{ql}x{tl}", q, t, w=24 if what == "lds" else -1, flag=0x40 if tag == "above" else 0, zdrop=400)
    q, t = pair("route_global", 40, tl + 61)
    add("route_global_narrow", q, t)
    add("route_global_narrow_rev", q, t, flag=0xc2, zdrop=100)
    q, t = pair("route_global_tall", tl + 33, 48)            # the query is the long one: LDS
    add("route_lds_tall", q, t, w=30)
    return out


def fuzz_cases(n_per_set=300, seed=20240607):
    """About 1 500 problems below 90 x 90 over the five scoring sets of options.c."""
    out = []
    for k, sc in enumerate(("default", "asm5", "asm10", "asm20", "sr")):
        rng = np.random.default_rng(seed + k)
        for i in range(n_per_set):
            ql, tl = int(rng.integers(1, 90)), int(rng.integers(1, 90))
            kind = rng.integers(0, 5)
            if kind == 0:
                q, t = rand_seq(rng, ql), rand_seq(rng, tl)
            elif kind == 1:
                letters = int(rng.integers(1, 3))
                q, t = rand_seq(rng, ql, letters), rand_seq(rng, tl, letters)
            else:
                q = rand_seq(rng, ql)
                t = fit(rng, mutate(rng, q, sub=float(rng.random() * 0.2), indel=float(rng.random() * 0.1), max_indel=int(rng.integers(1, 30))), tl)
            if rng.random() < 0.15:
                q = q.copy(); q[rng.integers(0, ql, max(1, ql // 10))] = 4
            if rng.random() < 0.15:
                t = t.copy(); t[rng.integers(0, tl, max(1, tl // 10))] = 4
            out.append(dict(name=f"fuzz_{sc}_{i}", query=q, target=t, scoring=sc, w=int(rng.choice(FUZZ_W)), zdrop=int(rng.choice(FUZZ_ZDROP)),
                            end_bonus=int(rng.choice((-1, 0, 10))), flag=int(rng.choice(FUZZ_FLAGS))))
    return out


def groups(cases):
    """{scoring key: [cases]} in order of first appearance."""
    out = {}
    for c in cases:
        out.setdefault(c["scoring"], []).append(c)
    return out


def pack(cases):
    """The flat arrays of one call: bases, q_beg, q_len, t_beg, t_len, w, zdrop, end_bonus, flag."""
    seqs, beg = [], 0
    cols = {k: [] for k in ("q_beg", "q_len", "t_beg", "t_len", "w", "zdrop", "end_bonus", "flag")}
    for c in cases:
        cols["q_beg"].append(beg); cols["q_len"].append(len(c["query"])); beg += len(c["query"])
        cols["t_beg"].append(beg); cols["t_len"].append(len(c["target"])); beg += len(c["target"])
        seqs += [c["query"], c["target"]]
        for k in ("w", "zdrop", "end_bonus", "flag"):
            cols[k].append(c[k])
    out = {k: np.array(v, np.int64 if k.endswith("_beg") else np.int32) for k, v in cols.items()}
    out["bases"] = np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)
    return out


# Argument refusals of chaindp_ksw_extd, as a table: (name, what to change of a valid call, the code it returns).  A change names an
# argument of Device.ksw_extd ("flag", "w", ... take a list that replaces the per-problem array; "scoring" a tuple; "bases" a
# function of the array).  -1 is CHAINDP_ERR_ARG; nothing is launched and the context stays usable.
ERR_ARG = -1
REFUSALS = (
    ("flag_generic_sc", dict(flag=[0, 0x04]), ERR_ARG),
    ("flag_approx_drop", dict(flag=[0x10, 0]), ERR_ARG),
    ("flag_approx_drop_with_max", dict(flag=[0x18, 0]), ERR_ARG),
    ("flag_splice_for", dict(flag=[0, 0x100]), ERR_ARG),
    ("flag_splice_rev", dict(flag=[0x200, 0]), ERR_ARG),
    ("flag_splice_flank", dict(flag=[0, 0x400]), ERR_ARG),
    ("flag_bit_5", dict(flag=[0x20, 0]), ERR_ARG),
    ("flag_high_bit", dict(flag=[0, 0x800]), ERR_ARG),
    ("flag_negative", dict(flag=[-1, 0]), ERR_ARG),
    ("scoring_a_128", dict(scoring=(128, 4, 4, 2, 24, 1)), ERR_ARG),
    ("scoring_b_negative", dict(scoring=(2, -4, 4, 2, 24, 1)), ERR_ARG),
    ("scoring_q2_128", dict(scoring=(2, 4, 4, 2, 128, 1)), ERR_ARG),
    ("scoring_e_negative", dict(scoring=(2, 4, 4, -1, 24, 1)), ERR_ARG),
    ("base_5_in_query", dict(bases=lambda b: np.concatenate([[5], b[1:]]).astype(np.uint8)), ERR_ARG),
    ("base_255_in_target", dict(bases=lambda b: np.concatenate([b[:-1], [255]]).astype(np.uint8)), ERR_ARG),
    ("negative_q_len", dict(q_len=[-1, 10]), ERR_ARG),
    ("negative_t_len", dict(t_len=[10, -5]), ERR_ARG),
    ("negative_q_beg", dict(q_beg=[-1, 0]), ERR_ARG),
    ("negative_t_beg", dict(t_beg=[0, -2]), ERR_ARG),
)


def refusal_base_call():
    """A valid call of two problems over 40 bases: query [0, 10) against target [10, 20), query [20, 30) against target [30, 40)."""
    rng = np.random.default_rng(5)
    return dict(bases=rand_seq(rng, 40), q_beg=[0, 20], q_len=[10, 10], t_beg=[10, 30], t_len=[10, 10], scoring=SCORING["default"], w=[-1, 5],
                zdrop=[400, -1], end_bonus=[-1, 10], flag=[0, 0x40])
