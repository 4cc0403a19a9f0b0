"""Inputs that sit exactly on the lane-group (64) and LDS-cap (256 hits, 64 hits of a fragment) edges of the stages after the chains:
mm_gen_regs, mm_est_err, chain_post, mm_set_mapq and the fragment kernels (numpy only).

Every constructor returns (batch, props): the batch in the layout of post_shapes._pack (single-segment reads, map-ont chaining
parameters, min_cnt 3) or frag_model._pack (fragments, sr chaining parameters, min_cnt 2), and a dict of the properties it claims.
props["post"] holds the chain_post options the shape needs besides the preset's (e.g. mask_level).  tests/test_hit_edge_shapes_cpu.py
proves every claim with the restatements, tests/test_gpu_hit_edges.py runs the batches on the GPU.  A constructor that cannot reach its
edge raises: it never falls back to a nearby size.

With span 15 and colinear anchors 20 apart a chain of n anchors scores 15 n (map-ont) and covers 20 (n - 1) + 15 query bases; a step
below 15 adds the step.  With span 21 and anchors 10 apart a chain of n anchors scores 21 + 10 (n - 1) (sr)."""
import numpy as np

import frag_model as fm
import post_shapes as ps
from frag_model import _frag, _place
from post_shapes import _chain, _pack, _read

LANES = 64                       # every group loop of the hit stages
POST_LDS_CAP = 256               # k_post_read: hits of a read kept in LDS
FRAG_LDS_CAP = 64                # k_frag_read / k_frag_seg
REGS_DIV_BLOCK = 256             # k_regs_div: hits per block
MIN_CNT, FRAG_MIN_CNT = 3, 2
PITCH = 150                      # query distance between the disjoint short chains


def _disjoint(n, rid0=0, q0=100, cnts=(4, 5, 6), pitch=PITCH):
    """n colinear chains of cnts[i % len(cnts)] anchors on n distinct targets and disjoint query intervals: n hits, n primaries."""
    return [_chain(rid0 + i, 1000, q0 + pitch * i, cnts[i % len(cnts)]) for i in range(n)]


def _chains_read(n, rid0=0, cnts=(4, 5, 6)):
    """A read of n chains; for n = 0 two anchors that make no chain (fewer than min_cnt, score 30), so that the read is not empty."""
    if n == 0:
        return _read([_chain(rid0, 1000, 100, 2)], 500)
    return _read(_disjoint(n, rid0=rid0, cnts=cnts), _qend(n) + 200)


def _qend(n, q0=100, pitch=PITCH):
    return q0 + pitch * n


def _score_chain(rid, r0, y0, length, score):
    """One diagonal chain that covers `length` query bases (qs = y0 + 1 - 15) and scores `score`: 15 for the first anchor, one step of
    t <= 15 (adds t), m steps of 15 or more (15 each)."""
    m, t = (score - 16) // 15, score - 15 - 15 * ((score - 16) // 15)
    rest = length - 15 - t
    if m < 1 or not 1 <= t <= 15 or rest < 15 * m or rest // m + 1 > 4000:
        raise ValueError(f"no chain of length {length} with score {score}")
    steps = [t] + [rest // m + (1 if i < rest % m else 0) for i in range(m)]
    return ps._steps_chain(rid, r0, y0, steps)


def _single(reads, **props):
    return _pack(reads), props


# ---------------------------------------------------------------- mm_gen_regs

REGS_CHAINS = (0, 1, 64, 65, 128, 129)


def regs_chain_counts(n):
    """One read of n chains (k_regs_keys: the rank by readlane up to 64, the radix procedure above; the carry between groups of 64)."""
    return _single([_chains_read(n)], chains=[n])


def regs_equal_keys(n=130):
    """n >= 130 chains of equal score and count: the keys differ in the scrambled low half only."""
    if n < 130:
        raise ValueError("the equal-key read needs at least 130 chains")
    return _single([_read(_disjoint(n, cnts=(4,)), _qend(n) + 200)], chains=[n], equal_high=True)


REGS_NEIGHBOURS = (1, 65, 130, 0, 66)


def regs_neighbours():
    """Reads of 1, 65, 130, 0 and 66 chains: range stacks side by side at offsets that are no multiples of 64."""
    return _single([_chains_read(n, rid0=200 * i) for i, n in enumerate(REGS_NEIGHBOURS)], chains=list(REGS_NEIGHBOURS))


REGS_LONG = (64, 65, 66, 129)


def regs_long_chain(n_anchors, n_short=5):
    """One chain of n_anchors anchors (n_anchors - 1 fuzzy-length terms) among short ones."""
    long_ = _chain(0, 1000, 100, n_anchors, step=20, qstep=23)        # tl != ql: mlen and blen differ
    q1 = 100 + 23 * n_anchors + 100
    short = _disjoint(n_short, rid0=1, q0=q1)
    return _single([_read([long_] + short, q1 + PITCH * n_short + 200)], chains=[n_short + 1], longest=n_anchors)


def regs_all():
    """Every mm_gen_regs read in one batch."""
    reads, chains, longest = [], [], []
    for n in REGS_CHAINS:
        reads.append(_chains_read(n)); chains.append(n); longest.append(6 if n > 2 else 4 if n else 0)
    reads.append(_read(_disjoint(130, cnts=(4,)), _qend(130) + 200)); chains.append(130); longest.append(4)
    for n in REGS_LONG:
        sh, pr = regs_long_chain(n)
        reads.append((sh["anchors"], int(sh["qlen"][0]), sh["mini_pos"], 0)); chains.append(pr["chains"][0]); longest.append(n)
    for i, n in enumerate(REGS_NEIGHBOURS):
        reads.append(_chains_read(n, rid0=200 * i)); chains.append(n); longest.append(6 if n > 2 else 4 if n else 0)
    return _single(reads, chains=chains, longest=longest)


# ---------------------------------------------------------------- mm_est_err

def _with_mini_pos(read, mp):
    return read[0], read[1], np.asarray(mp, np.uint64), read[3]


def _mp_of(qpos, span=ps.SPAN):
    return np.array([span << 32 | int(q) for q in sorted(set(int(x) for x in qpos))], np.uint64)


def _anchor_qpos(a, qlen):
    """esterr.c:7-14: the forward query position of every anchor."""
    y = (a[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    span = (a[:, 1] >> np.uint64(32) & np.uint64(0xff)).astype(np.int64)
    rev = (a[:, 0] >> np.uint64(63)).astype(bool)
    return np.where(rev, qlen - 1 - (y + 1 - span), y)


def esterr_totals(total):
    """A batch whose hits add up to `total` (256: one block of k_regs_div; 257: a second block of one hit), with reads without hits
    at the front, in the middle and at the end, whose offsets repeat in the binary search (every other one of them has no anchor
    either)."""
    if total < 200:
        raise ValueError("total too small")
    per = [0, 0, 100, 0, 64, 0, total - 164, 0, 0]
    reads = [_read([], 300) if n == 0 and i % 2 else _chains_read(n, rid0=300 * i) for i, n in enumerate(per)]
    return _single(reads, hits=per, total=total)


def esterr_mini_pos(n_reads):
    """n_reads (4: one block of k_regs_span_sum; 5: two) reads: one without minimizer positions (div stays as it came), one with exactly
    64 and one with exactly 65 positions of differing spans, one whose hits' first anchors are missing from mini_pos (a forward and a
    reverse hit), and for 5 reads one plain read."""
    if n_reads not in (4, 5):
        raise ValueError("4 or 5 reads")
    reads, n_mp, absent = [], [], []
    r = _read(_disjoint(3), 1000)
    reads.append(_with_mini_pos(r, np.zeros(0, np.uint64))); n_mp.append(0); absent.append(0)
    for want in (64, 65):
        chains = _disjoint(6, cnts=(5, 6))
        a, qlen = np.concatenate(chains), _qend(6) + 4000
        pos = sorted(set(_anchor_qpos(a, qlen).tolist()))
        extra = [p for p in range(_qend(6) + 50, qlen, 37)][:want - len(pos)]
        pos = sorted(pos + extra)
        if len(pos) != want:
            raise ValueError(f"no read with {want} minimizer positions")
        mp = np.array([(11 + i % 9) << 32 | p for i, p in enumerate(pos)], np.uint64)     # spans 11..19: the last one counts in avg_k
        reads.append(_with_mini_pos(_read(chains, qlen), mp)); n_mp.append(want); absent.append(0)
    qlen = 3000
    fwd, rev = _chain(0, 1000, 100, 8), _chain(1, 1000, 600, 8, rev=True)
    keep = _chain(2, 1000, 1200, 8)
    a = np.concatenate([fwd, rev, keep])
    pos = set(_anchor_qpos(a, qlen).tolist())
    # the search starts from the first anchor of a forward hit and from the last anchor of a reverse hit (esterr.c:46)
    gone = {int(_anchor_qpos(fwd[:1], qlen)[0]), int(_anchor_qpos(rev[-1:], qlen)[0])}
    reads.append(_with_mini_pos(_read([fwd, rev, keep], qlen), _mp_of(pos - gone))); n_mp.append(len(pos - gone)); absent.append(2)
    if n_reads == 5:
        r = _read(_disjoint(7, rid0=10), _qend(7) + 200)
        reads.append(r); n_mp.append(len(r[2])); absent.append(0)
    return _single(reads, n_mini_pos=n_mp, absent_first=absent)


# ---------------------------------------------------------------- chain_post

JOIN_PIECE = 80                  # anchors of each joinable piece: the joined chain has 160


def _join_pair(rid, r0, q0):
    """Two pieces of one alignment cut by a 3000-bp deletion (beyond bw, within max_join_long): mm_join_long joins them."""
    n = JOIN_PIECE
    return [_chain(rid, r0, q0, n), _chain(rid, r0 + 20 * n + 3000, q0 + 20 * n, n)]


def post_lds_cap(n_hits):
    """One read of n_hits hits (256: LDS; 257: global scratch): a joinable pair, a secondary that mm_select_sub drops (so mm_sync_regs
    runs after it and after the join, the squeeze moves anchors and the fix-up has a parent to move) and short disjoint primaries."""
    n_dis = n_hits - 4
    if n_dis < 1:
        raise ValueError("too few hits")
    q0 = 100
    pair = _join_pair(5000, 10000, q0)
    sec = _chain(5001, 500, q0 + 20 * JOIN_PIECE, 70)                  # a secondary of the second piece, kept: its parent moves
    drop = _chain(0, 500, q0, 20)                                      # a secondary of the first piece, dropped
    q1 = q0 + 40 * JOIN_PIECE + 200
    read = _read(pair + [sec, drop] + _disjoint(n_dis, rid0=10, q0=q1), q1 + PITCH * n_dis + 200)   # (the dropped hit's anchors come first)
    return read, dict(hits=n_hits, final=n_hits - 2, joined=1, joined_cnt=2 * JOIN_PIECE)


def post_cap_single(n_hits):
    read, props = post_lds_cap(n_hits)
    return _single([read], **{k: [v] for k, v in props.items()})


def post_cap_neighbours():
    """A 257-hit read (global scratch) between a 256-hit read and a small one (LDS)."""
    out = [post_lds_cap(256), post_lds_cap(257), (_read(_disjoint(7), _qend(7) + 200), dict(hits=7, final=7, joined=0, joined_cnt=0))]
    return _single([r for r, _ in out], **{k: [p[k] for _, p in out] for k in out[0][1]})


def post_primaries(n):
    """n disjoint hits: n primaries (post_set_parent: w[] of 64 is one group, 65 two)."""
    return _single([_read(_disjoint(n), _qend(n) + 200)], hits=[n], primaries=[n])


OVERLAP_FLAVOURS = ("first", "none", "late")


def post_overlap(k, flavour):
    """A last-ranked hit H (4 anchors, score 60) that overlaps exactly k primaries.
      first  k disjoint primaries inside H; mask_level 0.698 lies between the test's value with all k (64: 0.7024, 65: 0.7029) and
             with the first 64 of 65 (0.6931) counted as covered: H passes at the first primary
      none   the same read with mask_level 0.75: H passes nowhere and becomes a primary after ceil(k / 64) ballot rounds
      late   mask_level 0.95; k - 1 primaries of 700 bases, 20 apart (each fails against the ones before it: 680/700 - 20/700), that
             cover at most 630 bases of H's two ends (630/700) and rank before P, which covers H and ranks k-th among the k: H
             passes only at P"""
    if flavour not in OVERLAP_FLAVOURS:
        raise ValueError(flavour)
    if flavour in ("first", "none"):
        q0 = 100
        pri = _disjoint(k, q0=q0, cnts=(5, 6))
        qs, qe = q0 + 1 - 15, q0 + PITCH * (k - 1) + 20 * ((5, 6)[(k - 1) % 2] - 1) + 1
        step = -(-(qe - qs - 15) // 3)
        if step > 4900:
            raise ValueError("H's anchors would lie beyond max_dist")
        h = _chain(9000, 1000, q0, 4, step=step)
        covered = sum(20 * ((5, 6)[i % 2] - 1) + 15 for i in range(k))
        read = _read(pri + [h], q0 + 3 * step + 300)
        return _single([read], post=dict(mask_level=0.698 if flavour == "first" else 0.75), hits=[k + 1], overlapped=[k], h_len=15 + 3 * step,
                       covered=covered, passes_at_rank=[0 if flavour == "first" else -1], primaries=[k if flavour == "first" else k + 1])
    n_right, n_left = 32, k - 1 - 32
    if not 1 <= n_left <= 32:
        raise ValueError("late: 34 <= k <= 65")
    L, d, g, hl = 700, 20, 10, 15 + 3 * 465
    h0 = 2000
    h1 = h0 + hl
    chains = []
    for j in range(n_right):                                            # starts inside H's end, 20 apart; scores 200 - j
        chains.append(_score_chain(j, 1000, h1 - g - d * j + 14, L, 200 - j))
    for j in range(n_left):                                             # ends inside H's start; scores 160 - j
        chains.append(_score_chain(100 + j, 1000, h0 + g + d * j - L + 14, L, 160 - j))
    chains.append(_score_chain(8000, 1000, h0 + 14, hl, 85))            # P: H's interval, score 85 (H is kept: 60 + 30 >= 85)
    chains.append(ps._steps_chain(9000, 1000, h0 + 14, [465] * 3))      # H
    return _single([_read(chains, h1 + L + 300)], post=dict(mask_level=0.95), hits=[k + 1], overlapped=[k], passes_at_rank=[k - 1], primaries=[k])


def post_select_sub_above_64(n_low=30, n_drop=3):
    """More than 64 hits, of which mm_select_sub drops some in the middle of the ranks: the hits behind them (ids above 63) move down
    and mm_sync_regs renumbers them.  A primary of 10 anchors with a dropped secondary of 5 inside it, n_drop times; primaries of 6
    and 5 anchors before and n_low of 4 anchors after."""
    chains, q = [], 100
    for i in range(n_drop):
        chains += [_chain(3000 + i, 1000, q, 10), _chain(i, 1000, q + 20, 5)]                # (the dropped hits' anchors come first)
        q += 300
    n_high = 70 - 2 * n_drop
    chains += _disjoint(n_high, rid0=10, q0=q, cnts=(6, 6, 5))
    q += PITCH * n_high
    chains += _disjoint(n_low, rid0=1000, q0=q, cnts=(4,))
    n = 2 * n_drop + n_high + n_low
    return _single([_read(chains, q + PITCH * n_low + 200)], hits=[n], final=[n - n_drop], dropped=[n_drop])


def post_join_above_64():
    """A join whose joined chain has 160 anchors (post_set_coor: three groups of lanes) in a read of more than 64 hits."""
    pair = _join_pair(5000, 10000, 100)
    q1 = 100 + 40 * JOIN_PIECE + 200
    return _single([_read(pair + _disjoint(68, q0=q1), q1 + PITCH * 68 + 200)], hits=[70], final=[69], joined=[1], joined_cnt=[2 * JOIN_PIECE])


def post_all():
    """Every chain_post read that runs under the preset's options, in one batch."""
    parts = [post_cap_single(256), post_primaries(64), post_cap_single(257), post_primaries(65), post_select_sub_above_64(), post_join_above_64()]
    reads = []
    for sh, _ in parts:
        reads.append((sh["anchors"], int(sh["qlen"][0]), sh["mini_pos"], 0))
    return _single(reads, hits=[p["hits"][0] for _, p in parts])


def post_overlap_all(flavour):
    """Both sides of the 64-primaries edge of one flavour (one mask_level) in one batch, a small read between them."""
    (a, pa), (b, pb) = post_overlap(64, flavour), post_overlap(65, flavour)
    reads = [(a["anchors"], int(a["qlen"][0]), a["mini_pos"], 0), _read(_disjoint(3), 800), (b["anchors"], int(b["qlen"][0]), b["mini_pos"], 0)]
    return _single(reads, post=pa["post"], hits=[65, 3, 66], overlapped=[64, 0, 65])


# ---------------------------------------------------------------- mm_set_mapq

MAPQ_MIN_CHAIN_SCORE = 76


def _mapq_float(score, cnt, subsc, n_sub, sum_sc, rep_len, min_sc):
    f = np.float32
    uniq = f(sum_sc) / f(sum_sc + rep_len)
    pen_s1 = (f(1.0) if score > 100 else f(0.01) * f(score)) * uniq
    pen_cm = f(1.0) if cnt > 10 else f(0.1) * f(cnt)
    pen_cm = min(pen_s1, pen_cm)
    x = f(max(subsc, min_sc)) / f(score)
    return float(pen_cm * f(40.0) * (f(1.0) - x) * f(np.log(np.float64(score)))) - int(4.343 * np.log(n_sub + 1.0) + .499)


def mapq_read(n_final):
    """A read of n_final (64, 65) final hits, all primaries but three secondaries, the last-ranked hit a primary of score 60:
      scores 100 and 101 (pen_s1), counts 10 and 11 (pen_cm), secondaries of 75 and 77 under primaries of 105 (subsc below and above
      min_chain_score 76), a primary of score 600 without a secondary (clamps at 60), one with a secondary of its own score (0).
    rep_len is chosen so that the mapq of a primary moves when the last hit's score is missing from sum_sc."""
    chains, q = [], 100

    def put(c, adv):
        nonlocal q
        chains.append(c)
        q += adv
    put(_chain(1, 1000, q, 40), 900)                                                       # 600: clamps at 60
    chains.append(_chain(2, 1000, q, 20)); put(_chain(3, 5000, q, 20), 500)                # 300 and its equal: one is a secondary; 0
    put(_score_chain(4, 1000, q, 300, 100), 400)                                           # score 100, 7 anchors
    put(_score_chain(5, 1000, q, 300, 101), 400)                                           # score 101
    put(_chain(6, 1000, q, 10, step=12), 300)                                              # count 10, score 15 + 9 * 12 = 123
    put(_chain(7, 1000, q, 11, step=12), 300)                                              # count 11, score 135
    chains.append(_chain(8, 1000, q + 20, 5)); put(_chain(9, 1000, q, 7), 300)             # subsc 75 < 76 under 105
    chains.append(ps._steps_chain(10, 1000, q + 20, [15, 15, 15, 15, 2])); put(_chain(11, 1000, q, 7), 300)   # subsc 77 > 76 under 105
    n_rest = n_final - len(chains)
    chains += _disjoint(n_rest, rid0=100, q0=q, cnts=(5, 6, 4))
    qlen = q + PITCH * n_rest + 200
    # sum_sc of the primaries with and without the last-ranked hit (a 4-anchor primary, score 60)
    pri = [600, 300, 100, 101, 123, 135, 105, 105] + [15 * (5, 6, 4)[i % 3] for i in range(n_rest)]
    full, short = sum(pri), sum(pri) - 60
    rep = None
    for cand in range(2000, 200000, 7):
        moved = 0
        for sc, cnt, sub in ((90, 6, 0), (100, 7, 0), (101, 7, 0), (123, 10, 0), (135, 11, 0), (105, 7, 75), (105, 7, 77)):
            a, b = (_mapq_float(sc, cnt, sub, 0, s, cand, MAPQ_MIN_CHAIN_SCORE) for s in (full, short))
            lo, hi = min(a, b), max(a, b)
            if int(lo) != int(hi) and hi - int(hi) > 0.004 and int(hi) - lo > 0.004 and 1 <= int(lo) and int(hi) < 60:
                moved += 1
        if moved:
            rep = cand
            break
    if rep is None:
        raise ValueError("no rep_len at which sum_sc decides a mapq")
    read = _read(chains, qlen, rep)
    return read, dict(final=n_final, primaries=n_final - 3, sum_sc=full)


def mapq_batch(n_reads):
    """n_reads (4: one block of k_post_mapq; 5: two) reads, with 64 and 65 final hits among them."""
    if n_reads not in (4, 5):
        raise ValueError("4 or 5 reads")
    out = [mapq_read(64), mapq_read(65)]
    small = [(_read(_disjoint(n, cnts=(5, 6, 4)), _qend(n) + 200, 300), dict(final=n, primaries=n, sum_sc=sum(15 * (5, 6, 4)[i % 3] for i in range(n))))
             for n in (3, 9, 1)[:n_reads - 2]]
    out = [out[0], small[0], out[1]] + small[1:]
    return _single([r for r, _ in out], post=dict(min_chain_score=MAPQ_MIN_CHAIN_SCORE), **{k: [p[k] for _, p in out] for k in out[0][1]})


# ---------------------------------------------------------------- fragments (sr chaining parameters)

FSTEP, FPITCH = 10, 60           # a chain of two anchors covers 31 bases and scores 31


def _frag_pack(frags, **props):
    return fm._pack(frags), props


def _orphan(rid0=7000):
    ql = (150,)
    return _frag([_place(rid0, 80000, fm._run(0, 25, 6), ql), _place(rid0 + 1, 1000, fm._run(0, 40, 3), ql)], ql, 11)


def _disjoint_frag(n0, n1, rid0=0):
    """n0 two-anchor chains in segment 0 and n1 in segment 1, on distinct targets and disjoint positions: n0 + n1 hits, all primaries."""
    ql = (FPITCH * max(n0, 1) + 40, FPITCH * max(n1, 1) + 40)
    chains = [_place(rid0 + i, 1000, fm._run(0, 25 + FPITCH * i, 2), ql) for i in range(n0)]
    chains += [_place(rid0 + n0 + i, 1000, fm._run(1, 25 + FPITCH * i, 2), ql) for i in range(n1)]
    return _frag(chains, ql, 5)


def frag_hits(n):
    """A two-segment fragment with exactly n hits (k_frag_read: LDS up to 64, global scratch above), a few over both segments."""
    n0 = n // 2 - 1
    n1 = n - n0 - 2
    ql = (FPITCH * n0 + 40 + 200, FPITCH * n1 + 40 + 200)
    chains = [_place(i, 1000, fm._run(0, 25 + FPITCH * i, 2), ql) for i in range(n0)]
    chains += [_place(n0 + i, 1000, fm._run(1, 225 + FPITCH * i, 2), ql) for i in range(n1)]
    both = ql[0] - 160
    chains.append(_place(5000, 1000, fm._run(0, both, 16) + fm._run(1, 20, 12), ql))                  # over both segments
    chains.append(_place(5001, 1000, fm._run(0, both + 20, 8) + fm._run(1, 20, 4), ql))               # its secondary, over both
    return _frag_pack([_orphan(), _frag(chains, ql, 9), _orphan(7100)], hits=[2, n, 2], n_segs=[1, 2, 1])


def frag_seg_chains(n):
    """A fragment whose segment 0 keeps exactly n chains (k_frag_seg: LDS up to 64) and whose segment 1 keeps 3."""
    return _frag_pack([_disjoint_frag(n, 3), _orphan()], hits=[n + 3, 2], seg_chains=[n, 3, 2])


def frag_long_hit(n):
    """A hit with n anchors in segment 0 and 5 in segment 1 (k_frag_read / k_frag_split: a lane per anchor), and short hits."""
    ql = (FSTEP * n + 60, 300)
    long_ = _place(0, 1000, fm._run(0, 25, n) + fm._run(1, 21, 5), ql)
    rev = _place(1, 50000, fm._run(0, 25, n) + fm._run(1, 21, 5), ql, rev=True)
    short = [_place(2 + i, 1000, fm._run(1, 100 + 50 * i, 2), ql) for i in range(3)]
    return _frag_pack([_frag([long_, rev] + short, ql, 3), _orphan()], hits=[5, 2], anchors_in_seg0=n, anchors_in_seg1=5)


def frag_many_segments(n_segs):
    """A read of n_segs (64, 65, 255) segments of 70 bases with one two-anchor hit each and one hit over segments 0 and 1, a
    one-segment read on either side of it."""
    if not 2 <= n_segs <= 255:
        raise ValueError("2..255 segments")
    ql = (70,) * n_segs
    chains = [_place(s, 1000, fm._run(s, 30, 2), ql) for s in range(n_segs)]
    chains.append(_place(9000, 1000, fm._run(0, 45, 3) + fm._run(1, 21, 3), ql))
    return _frag_pack([_orphan(), _frag(chains, ql, 4), _orphan(7100)], hits=[2, n_segs + 1, 2], n_segs=[1, n_segs, 1])


def frag_all():
    """The fragment shapes of one stage concatenated: LDS and scratch fragments, long and short reads next to one another."""
    reads = []
    for sh_props in (frag_hits(64), frag_hits(65), frag_seg_chains(64), frag_seg_chains(65), frag_long_hit(64), frag_long_hit(65),
                     frag_many_segments(64), frag_many_segments(65)):
        reads.append(sh_props[0])
    return _frag_concat(reads), dict(reads=sum(len(s["n_segs"]) for s in reads))


def _frag_concat(batches):
    off = np.concatenate([[0]] + [b["off"][1:] + sum(int(x["off"][-1]) for x in batches[:i]) for i, b in enumerate(batches)]).astype(np.int64)
    mpo = np.concatenate([[0]] + [b["mini_pos_off"][1:] + sum(int(x["mini_pos_off"][-1]) for x in batches[:i]) for i, b in enumerate(batches)]).astype(np.int64)
    cat = lambda k: np.concatenate([b[k] for b in batches])
    return dict(off=off, anchors=cat("anchors"), n_segs=cat("n_segs"), seg_len=cat("seg_len"), qlen=cat("qlen"), mini_pos_off=mpo,
                mini_pos=cat("mini_pos"), rep_len=cat("rep_len"))
