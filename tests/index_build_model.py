"""CHECKER ONLY: the reference's index image (blobs B, H, V, P; index.c:340-416 and 603-720) restated in numpy / Python, from
tests/sketch_model.py's minimizers to the four blobs, in CANONICAL form: B, P, every flag word of H, all padding and the key and value
of every occupied slot as the reference writes them; key and value of an empty slot zero (the reference writes `h->keys[j]` and
`h->vals[j]` of every slot, and khash never initialises those arrays, so there it is whatever the heap held).

With b = bucket bits and m = x >> 8 a minimizer lives in bucket m & (2^b - 1).  Per bucket the groups of equal m enter a khash table
(khash.h:232-336, hash = key >> 1 truncated to 32 bits) in ascending m: kh_resize(n_keys) first, then the puts, one expansion to
twice the size with the kick-out rehash when a put finds n_occupied >= upper.  Nothing is ever deleted."""
import numpy as np

import sketch_model as sm

ROUTE = ("sub_batches", "minimizers", "distinct", "buckets", "expanded", "max_keys", "passes_run", "passes_skipped")
U = np.uint64


def minimizers(seqs, w, k, is_hpc):
    """mm_sketch of every sequence with rid = its number: uint64[n, 2] (x, y), in sequence order."""
    xs, ys = [], []
    for rid, s in enumerate(seqs):
        x, y = sm.sketch(s, w, k, is_hpc)
        xs.append(x)
        ys.append(y | U(rid << 32))
    if not xs:
        return np.zeros((0, 2), np.uint64)
    return np.stack((np.concatenate(xs), np.concatenate(ys)), axis=1).astype(np.uint64)


def pos_word(y, rank):
    rid = y >> U(32)
    rk = rid if rank is None else np.asarray(rank, np.uint64)[rid.astype(np.int64)]
    return (rid & U(0x1FFFFF)) << U(43) | (y & U(0x3FFFFF)) << U(21) | (rk & U(0x1FFFFF))


def first_size(n_keys):
    n = 4
    while n < n_keys:
        n <<= 1
    return n


def upper(n):
    return int(n * 0.77 + 0.5)


def khash_table(keys):
    """The bucket's table after the puts of `keys` (ints, in order): (N, slot of every key, expanded, longest kick-out chain).  A chain is
    what one step of the rehash's outer loop places: the element it took out plus those it kicked out in turn."""
    n0 = first_size(len(keys))
    n, up = n0, upper(n0)
    slots, occ, expanded, chain = {}, [None] * n0, False, 0
    for idx, key in enumerate(keys):
        if idx >= up and not expanded:
            expanded, n = True, 2 * n0
            old, new = occ, [None] * n
            for j in range(n0):
                if old[j] is None:
                    continue
                e, old[j], length = old[j], None, 0
                while True:
                    length += 1
                    i, step = (keys[e] >> 1 & 0xFFFFFFFF) & (n - 1), 0
                    while new[i] is not None:
                        step += 1
                        i = (i + step) & (n - 1)
                    new[i] = e
                    if i < n0 and old[i] is not None:
                        e, old[i] = old[i], None
                    else:
                        break
                chain = max(chain, length)
            occ = new
        i, step = (key >> 1 & 0xFFFFFFFF) & (n - 1), 0
        while occ[i] is not None:
            step += 1
            i = (i + step) & (n - 1)
        occ[i] = idx
    for i, e in enumerate(occ):
        if e is not None:
            slots[e] = i
    return n, [slots[e] for e in range(len(keys))], expanded, chain


def sort_passes(key2, y):
    """(run, skipped) of the device's LSD radix sort over the sixteen bytes of (key2, y): a byte that is equal everywhere is skipped."""
    if not len(key2):
        return 0, 0
    run = 0
    for v in (key2, y):
        differ = int(np.bitwise_or.reduce(v)) ^ int(np.bitwise_and.reduce(v))
        run += sum(1 for d in range(8) if differ >> 8 * d & 255)
    return run, 16 - run


def build(mini, rank=None, b=14):
    """minimizers uint64[n, 2] -> ([B, H, V, P] uint8 arrays in canonical form, route dict with 'max_chain' besides ROUTE's names)."""
    mini = np.asarray(mini, np.uint64).reshape(-1, 2)
    nb = 1 << b
    m, y = mini[:, 0] >> U(8), mini[:, 1]
    bucket = (m & U(nb - 1)).astype(np.int64)
    hi = m >> U(b)
    key2 = (m & U(nb - 1)) << U(56 - b) | hi
    run, skipped = sort_passes(key2, y)
    o = np.lexsort((y, hi, bucket))
    bucket, hi, y = bucket[o], hi[o], y[o]
    words = pos_word(y, rank) if len(y) else np.zeros(0, np.uint64)
    n = len(y)
    new = np.ones(n, bool)
    new[1:] = (bucket[1:] != bucket[:-1]) | (hi[1:] != hi[:-1])
    gs = np.nonzero(new)[0]
    ge = np.concatenate((gs[1:], [n])).astype(np.int64)
    g_bucket, g_hi, g_cnt = bucket[gs], hi[gs], ge - gs
    B = np.zeros((nb, 2), np.uint64)
    Hg, Vs, Ps = [], [], []
    allh = allp = 0
    route = dict.fromkeys(ROUTE, 0)
    route.update(minimizers=n, distinct=len(gs), passes_run=run, passes_skipped=skipped, max_chain=0)
    first = np.searchsorted(g_bucket, np.arange(nb + 1))
    for bk in np.unique(g_bucket).tolist():
        g0, g1 = int(first[bk]), int(first[bk + 1])
        cnt = g_cnt[g0:g1].tolist()
        keys = [(int(h) << 1 | (c == 1)) for h, c in zip(g_hi[g0:g1].tolist(), cnt)]
        N, slot, expanded, chain = khash_table(keys)
        slots = (N + 7) & ~7
        kv, vv, start_p = np.zeros(slots, np.uint64), np.zeros(slots, np.uint64), 0
        occ = np.zeros(slots, bool)
        for g, (key, c, s) in enumerate(zip(keys, cnt, slot)):
            a = int(gs[g0 + g])
            occ[s] = True
            kv[s] = key & 0xFFFFFFFFFFFF
            if c == 1:
                vv[s] = words[a]
            else:
                vv[s] = start_p << 32 | c
                Ps.append(words[a:a + c])
                start_p += c
        grp = np.zeros((slots // 8, 64), np.uint8)
        for g in range(slots // 8):
            word = 0xAAAAAAAA
            for t in range(16):
                s = (g >> 1) * 16 + t
                if s < N and occ[s]:
                    word &= ~(3 << 2 * t)
            grp[g, 0:4] = np.frombuffer(np.uint32(word).tobytes(), np.uint8)
        grp[:, 4:52] = kv.view(np.uint8).reshape(-1, 8)[:, :6].reshape(-1, 48)
        Hg.append(grp.reshape(-1))
        Vs.append(vv)
        B[bk, 0] = (allp & 0xFF) << 56 | N << 24
        B[bk, 1] = allh << 28 | allp >> 8
        allh += slots
        allp += start_p
        route["buckets"] += 1
        route["expanded"] += int(expanded)
        route["max_keys"] = max(route["max_keys"], len(keys))
        route["max_chain"] = max(route["max_chain"], chain)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return [B.reshape(-1).view(np.uint8).copy(), cat(Hg, np.uint8), cat(Vs, np.uint64).view(np.uint8).copy(),
            cat(Ps, np.uint64).view(np.uint8).copy()], route


def _tables(blobs):
    """Per non-empty bucket of an image: (bucket, N, first slot, first P word), from B."""
    B = np.asarray(blobs[0], np.uint8).view(np.uint64).reshape(-1, 2)
    for bk in np.nonzero(B.any(axis=1))[0].tolist():
        w0, w1 = int(B[bk, 0]), int(B[bk, 1])
        yield bk, w0 >> 24 & 0xFFFFFFFF, w1 >> 28, (w1 & 0xFFFFFFF) << 8 | w0 >> 56


def occupied(blobs):
    """bool per slot of the image: inside its bucket's table and flagged neither empty nor deleted."""
    H = np.asarray(blobs[1], np.uint8).reshape(-1, 64)
    flags = H[:, 0:4].copy().view(np.uint32).reshape(-1)
    occ = np.zeros(len(H) * 8, bool)
    for _, N, h0, _ in _tables(blobs):
        s = np.arange(N)
        fw = flags[(h0 + s) >> 3]
        occ[h0 + s] = (fw >> ((s & 15) << 1).astype(np.uint32) & 3) == 0
    return occ


def canonical(blobs):
    """An image as the reference serialises it -> its canonical form: key and value of every slot that is not occupied set to zero."""
    B, H, V, P = [np.asarray(x, np.uint8).copy() for x in blobs]
    occ = occupied([B, H, V, P])
    keys = H.reshape(-1, 64)[:, 4:52].reshape(-1, 6)          # a copy: the slice is not contiguous
    keys[~occ] = 0
    H.reshape(-1, 64)[:, 4:52] = keys.reshape(-1, 48)
    V.view(np.uint64)[~occ] = 0
    return [B, H, V, P]


def counts(blobs):
    """Occurrences of every distinct minimizer of an image (index.c:322), in slot order."""
    occ = occupied(blobs)
    H = np.asarray(blobs[1], np.uint8).reshape(-1, 64)
    key0 = H[:, 4:52].reshape(-1, 6)[:, 0]
    v = np.asarray(blobs[2], np.uint8).view(np.uint64)
    c = np.where(key0 & 1, U(1), v & U(0xFFFFFFFF)).astype(np.uint32)
    return c[occ]


def cal_max_occ(blobs, f):
    """mm_idx_cal_max_occ (index.c:307-328) over an image."""
    f = np.float32(f)
    if f <= 0:
        return 0x7FFFFFFF
    c = np.sort(counts(blobs))
    n = len(c)
    return int(c[int((1.0 - float(f)) * n) & 0xFFFFFFFF]) + 1
