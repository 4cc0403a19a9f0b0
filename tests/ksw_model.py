"""numpy restatement of ksw_extd2_sse (reference ksw2_extd2_sse.c, the non-generic scoring path) with the reference's memory layout.

The nine byte arrays u v x y x2 y2 s sf qr are one zero-filled block, as at :99-102 of the reference, because the reference
computes the cells of a diagonal that lie outside the band [st0, en0] (it rounds the band out to multiples of 16), reads some
of them back on the next diagonal, and lets its unaligned 16-byte score stores and loads run from one array into the next.
Every diagonal is done as "all loads, then all stores", which is what the vector code does within a 16-byte word and what the
device kernel does across a wave.  H is int64 here (it stays far inside int32).

ksw_extd(...) returns (ez int32[10], cigar uint32[n_cigar]); ez = max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score,
reach_end.  Two variants exist only to prove that the two traps are real:
  variant="clean"  resets the out-of-band cells of every diagonal to their initial values;
  variant="first"  takes the first maximum of H along t as max_t instead of the reference's lane order."""
import numpy as np

NEG_INF = -0x40000000
SCORE_ONLY, RIGHT, GENERIC_SC, APPROX_MAX, APPROX_DROP, EXTZ_ONLY, REV_CIGAR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x40, 0x80
ACCEPTED_FLAGS = SCORE_ONLY | RIGHT | APPROX_MAX | EXTZ_ONLY | REV_CIGAR
EZ_FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "reach_end")

# a, b, q, e, q2, e2 of options.c: the default (map-ont, map-pb, ava-*), asm5, asm10, asm20, sr
SCORING = {"default": (2, 4, 4, 2, 24, 1), "asm5": (1, 19, 39, 3, 81, 1), "asm10": (1, 9, 16, 2, 41, 1), "asm20": (1, 4, 6, 2, 26, 1),
           "sr": (2, 8, 12, 2, 24, 1)}


def _i8(v):
    return np.int8((int(v) + 128) % 256 - 128)


def reset_ez():
    return np.array([0, 0, -1, -1, NEG_INF, -1, NEG_INF, -1, NEG_INF, 0], np.int64)


def long_gap(q, e, q2, e2):
    """long_thres, long_diff of :94-97 (q, e, q2, e2 after the swap at :70)."""
    lt = (int((q2 - q) / (e - e2)) - 1) if e != e2 else 0           # C division truncates
    if q2 + e2 + lt * e2 > q + e + lt * e:
        lt += 1
    return lt, lt * (e - e2) - (q2 - q) - e2


def geometry(qlen, tlen, w):
    """w as used, tlen_ * 16, qlen_ * 16, n_col_ * 16 of :82-87."""
    if w < 0:
        w = max(qlen, tlen)
    T, Q = (tlen + 15) // 16 * 16, (qlen + 15) // 16 * 16
    n_col = (min(qlen, tlen, w + 1) + 15) // 16 + 1
    return w, T, Q, n_col * 16


def _backtrack(p, off, off_end, n_col, i0, j0, rev):
    """ksw_backtrack with is_rot = 1, min_intron_len = 0."""
    cig = []

    def push(op, ln):
        if cig and cig[-1][0] == op:
            cig[-1][1] += ln
        else:
            cig.append([op, ln])
    i, j, state = i0, j0, 0
    while i >= 0 and j >= 0:
        r, force = i + j, -1
        if i < off[r]:
            force = 2
        if i > off_end[r]:
            force = 1
        tmp = int(p[r * n_col + i - off[r]]) if force < 0 else 0
        if state == 0:
            state = tmp & 7
        elif not (tmp >> (state + 2) & 1):
            state = 0
        if state == 0:
            state = tmp & 7
        if force >= 0:
            state = force
        if state == 0:
            push(0, 1); i -= 1; j -= 1
        elif state == 1 or state == 3:
            push(2, 1); i -= 1
        else:
            push(1, 1); j -= 1
    if i >= 0:
        push(2, i + 1)
    if j >= 0:
        push(1, j + 1)
    if not rev:
        cig.reverse()
    return np.array([ln << 4 | op for op, ln in cig], np.uint32)


def ksw_extd(query, target, a, b, q, e, q2, e2, w, zdrop, end_bonus, flag, variant=None):
    assert variant in (None, "clean", "first")
    assert not flag & ~ACCEPTED_FLAGS
    query, target = np.asarray(query, np.uint8), np.asarray(target, np.uint8)
    qlen, tlen = len(query), len(target)
    ez = reset_ez()
    none = np.zeros(0, np.uint32)
    if qlen <= 0 or tlen <= 0:
        return ez.astype(np.int32), none
    qe = q + e                      # :60, before the swap: what H of the first cell is seeded with is the caller's first gap cost
    if q2 + e2 < q + e:
        q, q2, e, e2 = q2, q, e2, e
    a, b = abs(a), abs(b)
    if b > 2 * (q + e):
        return ez.astype(np.int32), none
    with_cigar, approx = not flag & SCORE_ONLY, bool(flag & APPROX_MAX)
    w, T, Q, n_col = geometry(qlen, tlen, w)
    lt, ldiff = long_gap(q, e, q2, e2)
    # the block: u v x y x2 y2 s sf qr, and the 16 spare bytes of the allocation
    mem = np.zeros(8 * T + Q + 16, np.int8)
    U, V, X, Y, X2, Y2, S, SF, QR = (k * T for k in range(9))
    mem[U:X2] = _i8(-q - e)
    mem[X2:S] = _i8(-q2 - e2)
    mem[QR:QR + qlen] = query[::-1].view(np.int8)
    mem[SF:SF + tlen] = target.view(np.int8)
    H = np.full(T, NEG_INF, np.int64)
    n_diag = qlen + tlen - 1
    if with_cigar:
        p = np.zeros(n_diag * n_col + 16, np.uint8)
        off, off_end = np.zeros(n_diag, np.int64), np.zeros(n_diag, np.int64)
    sc_mch, sc_mis, sc_n = _i8(a), _i8(-b), _i8(-e2)
    zero = np.int8(0)
    H0 = last_H0_t = 0
    last_st = last_en = -1

    def edge(r):                                        # :150 and :154
        return -q - e if r == 0 else -e if r < lt else ldiff if r == lt else -e2

    for r in range(n_diag):
        st, en = max(0, r - qlen + 1, (r - w + 1) >> 1), min(tlen - 1, r, (r + w) >> 1)
        if st > en:
            ez[1] = 1
            break
        st0, en0 = st, en
        st, en = st // 16 * 16, (en + 16) // 16 * 16 - 1
        if st > 0:
            if last_st <= st - 1 <= last_en:
                x1, x21, v1 = mem[X + st - 1], mem[X2 + st - 1], mem[V + st - 1]
            else:
                x1, x21, v1 = _i8(-q - e), _i8(-q2 - e2), _i8(-q - e)
        else:
            x1, x21, v1 = _i8(-q - e), _i8(-q2 - e2), _i8(edge(r))
        if en >= r:
            mem[Y + r], mem[Y2 + r], mem[U + r] = _i8(-q - e), _i8(-q2 - e2), _i8(edge(r))
        # scores: whole 16-byte words from st0, loads before stores
        idx = st0 + np.arange(((en0 - st0) // 16 + 1) * 16)
        sq, sr = mem[SF + idx], mem[QR + (qlen - 1 - r) + idx]
        sc = np.where(sq == sr, sc_mch, sc_mis)
        mem[S + idx] = np.where((sq == 4) | (sr == 4), sc_n, sc)
        # the cells of [st, en], loads before stores
        t = np.arange(st, en + 1)
        z, ut = mem[S + t].copy(), mem[U + t].copy()
        xt1, vt1, x2t1 = mem[X + t - 1].copy(), mem[V + t - 1].copy(), mem[X2 + t - 1].copy()
        xt1[0], vt1[0], x2t1[0] = x1, v1, x21
        ca, cb, ca2, cb2 = xt1 + vt1, mem[Y + t] + ut, x2t1 + vt1, mem[Y2 + t] + ut
        if not flag & RIGHT:
            d = (ca > z).astype(np.uint8)
            z = np.maximum(z, ca)
            d = np.where(cb > z, 2, d); z = np.maximum(z, cb)
            d = np.where(ca2 > z, 3, d); z = np.maximum(z, ca2)
            d = np.where(cb2 > z, 4, d); z = np.maximum(z, cb2)
        else:
            d = np.where(z > ca, 0, 1).astype(np.uint8)
            z = np.maximum(z, ca)
            d = np.where(z > cb, d, 2); z = np.maximum(z, cb)
            d = np.where(z > ca2, d, 3); z = np.maximum(z, ca2)
            d = np.where(z > cb2, d, 4); z = np.maximum(z, cb2)
        z = np.minimum(z, sc_mch)
        mem[U + t], mem[V + t] = z - vt1, z - ut
        tq, tq2 = z - _i8(q), z - _i8(q2)
        ca, cb, ca2, cb2 = ca - tq, cb - tq, ca2 - tq2, cb2 - tq2
        for arr, base, pen, bit in ((ca, X, q + e, 0x08), (cb, Y, q + e, 0x10), (ca2, X2, q2 + e2, 0x20), (cb2, Y2, q2 + e2, 0x40)):
            mem[base + t] = np.maximum(arr, zero) - _i8(pen)
            d = d | np.where((arr >= 0) if flag & RIGHT else (arr > 0), bit, 0).astype(np.uint8)
        if with_cigar:
            off[r], off_end[r] = st, en
            p[r * n_col:r * n_col + len(t)] = d
        if variant == "clean":
            out = t[(t < st0) | (t > en0)]
            for base in (U, V, X, Y):
                mem[base + out] = _i8(-q - e)
            mem[X2 + out] = mem[Y2 + out] = _i8(-q2 - e2)
        v8, u8 = mem[V:X], mem[U:V]
        if not approx:
            if r > 0:
                H[en0] = H[en0 - 1] + u8[en0] if en0 > 0 else H[en0] + v8[en0]
                max_H, max_t = int(H[en0]), en0
                H[st0:en0] += v8[st0:en0]
                if variant == "first":
                    if en0 > st0 and H[st0:en0].max() > max_H:
                        max_t = st0 + int(np.argmax(H[st0:en0])); max_H = int(H[max_t])
                else:
                    en1 = st0 + (en0 - st0) // 4 * 4
                    init = max_H
                    for i in range(4):                              # the four lanes, merged in lane order with a strict compare
                        lane = H[st0 + i:en1:4]
                        if len(lane) and lane.max() > init and lane.max() > max_H:
                            k = int(np.argmax(lane))
                            max_H, max_t = int(lane[k]), st0 + i + 4 * k
                    for tt in range(en1, en0):
                        if H[tt] > max_H:
                            max_H, max_t = int(H[tt]), tt
            else:
                H[0] = int(v8[0]) - qe
                max_H, max_t = int(H[0]), 0
            if en0 == tlen - 1 and H[en0] > ez[6]:
                ez[6], ez[7] = H[en0], r - en
            if r - st0 == qlen - 1 and H[st0] > ez[4]:
                ez[4], ez[5] = H[st0], st0
            # ksw_apply_zdrop
            if max_H > ez[0]:
                ez[0], ez[3], ez[2] = max_H, max_t, r - max_t
            elif max_t >= ez[3] and r - max_t >= ez[2]:
                tl, ql = max_t - ez[3], (r - max_t) - ez[2]
                if zdrop >= 0 and ez[0] - max_H > zdrop + abs(tl - ql) * e2:
                    ez[1] = 1
                    break
            if r == qlen + tlen - 2 and en0 == tlen - 1:
                ez[8] = H[tlen - 1]
        else:
            if r > 0:
                if st0 <= last_H0_t <= en0 and st0 <= last_H0_t + 1 <= en0:
                    d0, d1 = int(v8[last_H0_t]), int(u8[last_H0_t + 1])
                    if d0 > d1:
                        H0 += d0
                    else:
                        H0 += d1; last_H0_t += 1
                elif st0 <= last_H0_t <= en0:
                    H0 += int(v8[last_H0_t])
                else:
                    last_H0_t += 1; H0 += int(u8[last_H0_t])
            else:
                H0, last_H0_t = int(v8[0]) - qe, 0
            if r == qlen + tlen - 2 and en0 == tlen - 1:
                ez[8] = H0
        last_st, last_en = st, en
    cigar = none
    if with_cigar:
        rev = bool(flag & REV_CIGAR)
        if not ez[1] and not flag & EXTZ_ONLY:
            cigar = _backtrack(p, off, off_end, n_col, tlen - 1, qlen - 1, rev)
        elif not ez[1] and flag & EXTZ_ONLY and ez[4] + end_bonus > ez[0]:
            ez[9] = 1
            cigar = _backtrack(p, off, off_end, n_col, int(ez[5]), qlen - 1, rev)
        elif ez[3] >= 0 and ez[2] >= 0:
            cigar = _backtrack(p, off, off_end, n_col, int(ez[3]), int(ez[2]), rev)
    return ez.astype(np.int32), cigar
