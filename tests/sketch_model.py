"""CPU model of csrc/chaindp_sketch.hip: (w,k)-minimizers of a sequence as a chain of data-parallel steps, each of which the
kernels run with one lane per element.  The formulation ("Sketch on the GPU"):

  pushes   the bases that shift into the k-mer: every unambiguous base, or with homopolymer compression the last base of every
           run.  push rank = exclusive count of pushes (a tiled scan, `tile` bases per tile as the kernels do it).
  k-mers   forward / reverse k-mer of push p from the codes of pushes p-k+1..p (missing ones contribute zero bits, which is what
           shifting into two zeroed words gives).  sym[p] = the two are equal: such a push takes no window slot.
  slots    the ambiguous bases and the pushes that are not symmetric, in base order: one window slot each.
  l        slots since the last ambiguous one (0 on it); value = hash << 8 | span where l >= k and span < 256, else "none".
  window   slot s looks at the values of slots s-w..s only:  P = rightmost smallest of s-w..s-1.
             l == w+k-1 and P exists:   the slots of s-w+1..s-1 that tie with P (first-window ties)
             value(s) <= value(P):      P if l >= w+k          (a new minimum writes the old one)
             else if P is slot s-w:     P if l >= w+k-1        (the minimum leaves the window)
                                        then, Q = rightmost smallest of s-w+1..s, if l >= w+k-1: the slots of the window that tie with Q
           and after the last slot the current minimum.
Every emission of slot s is a function of 2w+k slots before it at the most, so any lane can compute any slot: no state is carried.

`sketch()` returns x, y (y = position << 1 | strand; the caller adds rid << 32 and the segment shift) and, in `traps`, how often each
emission site fired.  numpy only."""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)

NT4 = np.full(256, 4, np.uint8)
for _i, _s in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    NT4[_i] = _i                                   # the bytes 0..3 stand for themselves
    for _c in _s:
        NT4[ord(_c)] = _i


def hash64(key, mask):
    """The invertible integer hash of the k-mer (Thomas Wang's 64-bit mix under a 2k-bit mask), on uint64 arrays."""
    key = key.astype(np.uint64)
    m = np.uint64(mask)
    u = np.uint64
    key = (~key + (key << u(21))) & m
    key = key ^ (key >> u(24))
    key = ((key + (key << u(3))) + (key << u(8))) & m
    key = key ^ (key >> u(14))
    key = ((key + (key << u(2))) + (key << u(4))) & m
    key = key ^ (key >> u(28))
    key = (key + (key << u(31))) & m
    return key


def tiled_rank(flag, tile):
    """Exclusive count of set flags, computed the way the kernels do: per-tile totals, a scan of those, a scan inside the tile."""
    n = len(flag)
    if n == 0:
        return np.zeros(0, np.int64)
    nt = (n + tile - 1) // tile
    pad = np.zeros(nt * tile, np.int64)
    pad[:n] = flag
    pad = pad.reshape(nt, tile)
    tile_off = np.concatenate(([0], np.cumsum(pad.sum(1))[:-1]))
    inner = np.cumsum(pad, 1) - pad
    return (inner + tile_off[:, None]).reshape(-1)[:n]


def _rightmost_min(v, s, lo_d, hi_d):
    """For every slot index in s: (value, slot) of the rightmost smallest of slots s-hi_d .. s-lo_d (oldest first; slots < 0 hold NONE)."""
    bx = np.full(len(s), NONE, np.uint64)
    bt = s - hi_d
    for d in range(hi_d, lo_d - 1, -1):
        t = s - d
        val = np.where(t >= 0, v[np.maximum(t, 0)], NONE)
        upd = val <= bx
        bx = np.where(upd, val, bx)
        bt = np.where(upd, t, bt)
    return bx, bt


def sketch(seq, w, k, is_hpc, tile=256, traps=None, probe=None):
    """probe: a dict that receives the intermediate quantities (what the edge tier's claims are proved from); it changes nothing."""
    assert 0 < w < 256 and 0 < k <= 28
    if probe is not None:
        probe.update(n_push=0, n_slots=0)
    c = NT4[np.frombuffer(bytes(seq), np.uint8)] if not isinstance(seq, np.ndarray) else NT4[seq]
    n = len(c)
    ex = np.zeros(0, np.uint64)
    if n == 0:
        return ex, ex
    valid = c < 4
    if is_hpc:
        end = valid & (np.concatenate((c[1:], [5])) != c)
        start = valid & (np.concatenate(([5], c[:-1])) != c)
    else:
        end = start = valid
    rank = tiled_rank(end, tile)
    P = int(end.sum())
    if probe is not None:
        probe.update(code=c, end=end, start=start, rank=rank, n_push=P)
    if P == 0:
        return ex, ex
    pe = np.zeros(P, np.int64); ps = np.zeros(P, np.int64); pc = np.zeros(P, np.uint64)
    pe[rank[end]] = np.nonzero(end)[0]
    ps[rank[start]] = np.nonzero(start)[0]          # a run's first base sees the rank its last base will have
    pc[rank[end]] = c[end]
    # k-mers of every push
    k0 = np.zeros(P, np.uint64); k1 = np.zeros(P, np.uint64)
    pidx = np.arange(P)
    for j in range(k):
        q = pidx - j
        ok = q >= 0
        code = np.where(ok, pc[np.maximum(q, 0)], 0).astype(np.uint64)
        k0 |= np.where(ok, code << np.uint64(2 * j), 0).astype(np.uint64)
        k1 |= np.where(ok, (np.uint64(3) - code) << np.uint64(2 * (k - 1 - j)), 0).astype(np.uint64)
    sym = k0 == k1
    z = (k0 > k1).astype(np.uint64)
    hx = hash64(np.where(z == 1, k1, k0), (1 << 2 * k) - 1)
    # slots, in base order
    slot_flag = ~valid
    slot_flag[pe[~sym]] = True
    srank = tiled_rank(slot_flag, tile)
    S = int(slot_flag.sum())
    if probe is not None:
        probe.update(pend=pe, pstart=ps, sym=sym, slot_flag=slot_flag, n_slots=S)
    if S == 0:
        return ex, ex
    spos = np.nonzero(slot_flag)[0]
    is_n = ~valid[spos]
    sp = np.where(is_n, 0, rank[spos])              # push rank of a slot that is a push
    assert np.array_equal(srank[spos], np.arange(S))
    sidx = np.arange(S)
    last_n = np.maximum.accumulate(np.where(is_n, sidx, -1))
    l = sidx - last_n
    if is_hpc:
        span = np.where(l >= k, pe[sp] - ps[np.maximum(sp - k + 1, 0)] + 1, 0)
    else:
        span = np.full(S, k, np.int64)
    has = (~is_n) & (l >= k) & (span < 256)
    v = np.where(has, (hx[sp] << np.uint64(8)) | span.astype(np.uint64), NONE)
    y = np.where(has, (spos.astype(np.uint64) << np.uint64(1)) | z[sp], NONE)
    lcode = np.where(l >= w + k, 2, np.where(l == w + k - 1, 1, 0))
    # the window
    px, pt = _rightmost_min(v, sidx, 1, w)
    p_ok = px != NONE
    new_min = v <= px
    leaves = (~new_min) & (pt == sidx - w)
    em_s, em_ph, em_t = [], [], []

    def emit(s, ph, t):
        em_s.append(np.asarray(s, np.int64).reshape(-1)); em_ph.append(np.full(np.size(s), ph, np.int64)); em_t.append(np.asarray(t, np.int64).reshape(-1))

    def count(name, m):
        if traps is not None:
            traps[name] = traps.get(name, 0) + int(m)

    # first-window ties (rare: once per stretch without ambiguous bases)
    for s in np.nonzero((lcode == 1) & p_ok)[0]:
        lo = max(s - w + 1, 0)
        t = lo + np.nonzero(v[lo:s] == px[s])[0]
        t = t[t != pt[s]]
        emit(np.full(len(t), s), 0, t)
        count("first_window_tie", len(t))
    m = new_min & (lcode == 2) & p_ok
    emit(sidx[m], 1, pt[m]); count("old_min_on_new_min", m.sum())
    m = leaves & (lcode >= 1)
    emit(sidx[m], 1, pt[m]); count("min_left_window", m.sum())
    count("pending_min_dropped", (p_ok & is_n & (l == 0) & (np.concatenate(([0], l[:-1])) > 0)).sum())
    cs = sidx[leaves]
    qx, qt = _rightmost_min(v, cs, 0, w - 1)
    mcur_t = np.where(new_min, sidx, pt)
    mcur_x = np.where(new_min, v, px)
    mcur_t[cs] = qt; mcur_x[cs] = qx
    ties = np.zeros(len(cs), np.int64)
    for d in range(w):
        t = cs - d
        ties += (t >= 0) & (v[np.maximum(t, 0)] == qx)
    for j in np.nonzero((ties > 1) & (lcode[cs] >= 1) & (qx != NONE))[0]:
        s, lo = cs[j], max(cs[j] - w + 1, 0)
        t = lo + np.nonzero(v[lo:s + 1] == qx[j])[0]
        t = t[t != qt[j]]
        emit(np.full(len(t), s), 2, t)
        count("rescan_tie", len(t))
    if mcur_x[S - 1] != NONE:
        emit(S - 1, 3, mcur_t[S - 1]); count("final", 1)
        # the last minimum may be an entry from before the last ambiguous base: the window is not cleared there
        count("final_is_stale", mcur_t[S - 1] < last_n[S - 1])
        count("final_stale_beats_fresh", mcur_t[S - 1] < last_n[S - 1] and bool(has[last_n[S - 1]:].any()))
    if traps is not None:
        count("span_ge_256_slot", ((~is_n) & (l >= k) & (span >= 256)).sum())
        count("symmetric_skipped", sym.sum())
    es, eph, et = np.concatenate(em_s), np.concatenate(em_ph), np.concatenate(em_t)
    o = np.lexsort((et, eph, es))
    if probe is not None:
        probe.update(spos=spos, is_n=is_n, l=l, span=span, has=has, v=v, lcode=lcode, em_slot=es[o], em_phase=eph[o], em_target=et[o])
    return v[et[o]], y[et[o]]


def sketch_batch(seq, seq_off, w, k, is_hpc, n_segs_per_read=None, tile=256, traps=None):
    """mini_off[n_reads + 1], mini[n, 2] of a batch as the C ABI's chaindp_sketch returns them."""
    n_seqs = len(seq_off) - 1
    segs = np.ones(n_seqs, np.int64) if n_segs_per_read is None else np.asarray(n_segs_per_read, np.int64)
    out, off, q = [], [0], 0
    for ns in segs:
        shift = 0
        for rid in range(int(ns)):
            s = seq[int(seq_off[q]):int(seq_off[q + 1])]
            x, y = sketch(s, w, k, is_hpc, tile, traps)
            y = y + np.uint64((rid << 32) + (shift << 1))
            out.append(np.stack((x, y), 1))
            shift += len(s); q += 1
        off.append(off[-1] + sum(len(a) for a in out[len(out) - int(ns):]))
    assert q == n_seqs
    mini = np.concatenate(out) if out else np.zeros((0, 2), np.uint64)
    return np.array(off, np.int64), mini.reshape(-1, 2).astype(np.uint64)
