"""Seeded synthetic reads for chain_post / mm_set_mapq: anchors (sorted by x per read, as map.c:233 leaves them) whose chains, after
mm_chain_dp_fpga + mm_chain_dp_bottom + mm_gen_regs under map-ont parameters, give the hit layouts the post steps are sensitive to:

  quirk     mm_select_sub reads a slot that a later kept hit has already overwritten, and its decision depends on it
  join      one alignment cut by deletions larger than bw (so the DP splits it) but within max_join_long: mm_join_long joins the pieces,
            a secondary of a joined piece has its parent moved by the fix-up, a dropped secondary leaves a gap that mm_squeeze_a closes
  ident     a hit identical (rid, rs, re, qs, qe) to its parent, on the other strand: mm_select_sub drops it
  repeats   tens to a few hundred overlapping hits: repeats, equal-score duplicates
  big       more hits than k_post_read keeps in LDS (its global-memory path)
  scthres   a joinable pair whose weaker flank scores exactly the double-add sc_thres (84 for min_join_flank_sc 205, gap 8244):
            joined by the reference, not with a float add of .499 (the float add gives 85)
  mask      a hit whose mask test is exactly 0.5 in float but above it in double (ol 1889, min 2673, uncov 784, max 3793):
            a primary of its own in the reference, a secondary with the test in double
  logf      a primary of score 1579, the smallest integer where glibc's logf is not the correctly rounded one

Each shape: dict(off int64[R+1], anchors uint64[n,2], qlen int32[R], mini_pos_off int64[R+1], mini_pos uint64[m], rep_len int32[R])."""
import numpy as np

SPAN = 15


def _chain(rid, r0, q0, n, step=20, rev=False, span=SPAN, qstep=None):
    qstep = step if qstep is None else qstep
    x = (np.uint64(1 << 63) if rev else np.uint64(0)) | np.uint64(rid) << np.uint64(32) | (np.uint64(r0) + np.arange(n, dtype=np.uint64) * np.uint64(step))
    y = np.uint64(span) << np.uint64(32) | (np.uint64(q0) + np.arange(n, dtype=np.uint64) * np.uint64(qstep))
    return np.stack([x, y], 1)


def _read(chains, qlen, rep_len=0):
    a = np.concatenate(chains) if chains else np.zeros((0, 2), np.uint64)
    a = a[np.lexsort((a[:, 1], a[:, 0]))]
    # minimizer positions: every anchor's forward query position (esterr.c:7-14 inverts the reverse ones), plus a few off-chain ones
    qpos = []
    for x, y in a:
        span = int(y >> np.uint64(32) & np.uint64(0xff))
        p = int(y & np.uint64(0xffffffff))
        qpos.append(qlen - 1 - (p + 1 - span) if int(x) >> 63 else p)
    qpos = sorted(set(q for q in qpos if 0 <= q < qlen) | set(range(7, qlen, 997)))
    mp = np.array([SPAN << 32 | q for q in qpos], np.uint64)
    return a, qlen, mp, rep_len


def quirk_read():
    # scores ~15 per anchor: A 1005 (X), D 705 (X, dropped: < 0.8 A), B 690 (Y, primary, moves to slot 1), E 555 (Y, kept, lands in
    # B's old slot 2), F 450 (Y, parent 2): compared with E (kept: 450 >= 0.8 * 555) where B was meant (dropped: 450 < 0.8 * 690)
    return _read([_chain(0, 1000, 20, 67), _chain(1, 1000, 20, 47), _chain(2, 1000, 3000, 46), _chain(3, 1000, 3000, 37),
                  _chain(4, 1000, 3000, 30)], 5000)


def join_read(rev=False):
    # three pieces on rid 0 cut by 3000-bp deletions; a secondary of the middle piece (rid 1); a dropped secondary of the first (rid 2)
    p1 = _chain(0, 10000, 100, 100, rev=rev)
    p2 = _chain(0, 10000 + 2000 + 3000, 100 + 2000, 100, rev=rev)
    p3 = _chain(0, 10000 + 4000 + 6000, 100 + 4000, 90, rev=rev)
    sec = _chain(1, 500, 100 + 2000, 95, rev=rev)
    drop = _chain(2, 500, 100, 20, rev=rev)
    return _read([p1, p2, p3, sec, drop], 7000)


def ident_read():
    qlen, n = 4000, 60
    fwd = _chain(0, 2000, 300, n)
    y0, yl = 300, 300 + (n - 1) * 20
    rev = _chain(0, 2000, qlen - yl - 2 + SPAN, n, rev=True)
    assert qlen - yl - 2 + SPAN - 0 >= 0 and y0 >= 0
    other = _chain(1, 100, 2500, 40)
    return _read([fwd, rev, other], qlen)


def _span_chain(rid, r0, y0, yl, step=20):
    """Anchors on one diagonal from query position y0 to yl (both included), `step` apart but for the last step."""
    ys = list(range(y0, yl, step)) + [yl]
    x = np.uint64(rid) << np.uint64(32) | (np.uint64(r0) + np.array([y - y0 for y in ys], np.uint64))
    y = np.uint64(SPAN) << np.uint64(32) | np.array(ys, np.uint64)
    return np.stack([x, y], 1)


def _steps_chain(rid, r0, y0, steps):
    pos = np.concatenate([[0], np.cumsum(steps)]).astype(np.uint64)
    x = np.uint64(rid) << np.uint64(32) | (np.uint64(r0) + pos)
    y = np.uint64(SPAN) << np.uint64(32) | (np.uint64(y0) + pos)
    return np.stack([x, y], 1)


def scthres_read():
    # r0: 15 + 9 + 4 x 15 = 84 over 4424 bp (>= 8244 >> 1); r1 8244 bp further on the reference, 20 bp on the query: 20 x 15 = 300
    r0 = _steps_chain(7, 1000, 200, [9, 1100, 1100, 1100, 1100])
    r1 = _steps_chain(7, 1000 + 4409 + 8244, 200 + 4409 + 20, [300] * 19)
    return _read([r0, r1], 11000)


def mask_read():
    # primary P: query [100, 3893) (3793 bp); hit i: [2004, 4677) (2673 bp), 1889 of them inside P
    return _read([_span_chain(8, 5000, 114, 3892), _span_chain(9, 5000, 2018, 4676)], 6000)


def logf_read():
    return _read([_steps_chain(10, 3000, 300, [4] + [20] * 104)], 4000)


def repeats_read(rng, n_hits, qlen=20000):
    chains = []
    anchor_q = rng.integers(0, qlen - 3000, size=max(1, n_hits // 8))
    for h in range(n_hits):
        q0 = int(anchor_q[rng.integers(len(anchor_q))]) + int(rng.integers(-200, 200))
        q0 = max(q0, SPAN)                                   # an anchor's y is the last base of its k-mer: qs >= 0
        n = int(rng.choice([4, 5, 8, 12, 20, 30, 45, 70]))
        if rng.random() < 0.2 and chains:                    # an equal-score duplicate of an earlier hit elsewhere in the reference
            n = len(chains[-1])
        rid = int(rng.integers(0, 4000))
        chains.append(_chain(rid, int(rng.integers(0, 1 << 20)) * 8, q0, n, rev=bool(rng.random() < 0.3)))
    if rng.random() < 0.5:                                   # a joinable alignment among the repeats
        r0 = 4001
        chains += [_chain(r0, 50000, 500, 80), _chain(r0, 50000 + 1600 + 2500, 500 + 1600, 80)]
    return _read(chains, qlen, int(rng.integers(0, 3000)))


def big_read(rng, n_hits=300):
    return repeats_read(rng, n_hits, qlen=60000)


def _pack(reads):
    a = [r[0] for r in reads]
    off = np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.int64)
    mpo = np.concatenate([[0], np.cumsum([len(r[2]) for r in reads])]).astype(np.int64)
    return dict(off=off, anchors=np.concatenate(a).astype(np.uint64), qlen=np.array([r[1] for r in reads], np.int32), mini_pos_off=mpo,
                mini_pos=np.concatenate([r[2] for r in reads]).astype(np.uint64), rep_len=np.array([r[3] for r in reads], np.int32))


def shapes(seed=7, n_random=12):
    """The synthetic set under map-ont chaining parameters: the trap reads, seeded repeat reads, one read above the LDS cap."""
    rng = np.random.default_rng(seed)
    reads = [quirk_read(), join_read(), join_read(rev=True), ident_read(), scthres_read(), mask_read(), logf_read()]
    for _ in range(n_random):
        reads.append(repeats_read(rng, int(rng.integers(10, 160))))
    reads.append(big_read(rng))
    return _pack(reads)
