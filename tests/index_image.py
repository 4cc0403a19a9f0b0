"""CHECKER ONLY: an index image (the blobs B, H, V, P that chaindp_index_create and oracle_lib.SeedIndex open) built from sequences,
written from the format as oracle/seed_oracle.cpp reads it and as _build_image of test_gpu_seed_collect.py writes it:

  B   one 16-byte entry per bucket, 2^b_bits buckets; a minimizer m = x >> 8 lives in bucket m & (2^b_bits - 1).
      word 0: first P word (low 8 bits) << 56 | slots of the bucket's hash table << 24; word 1: first slot << 28 | first P word >> 8
  H   the hash tables, eight slots to a 64-byte group: the 32-bit flag word of the sixteen slots the group belongs to (two bits
      per slot, bit 1 = empty), eight 48-bit keys, twelve bytes of padding.  key = (m >> b_bits) << 1, | 1 where the minimizer
      occurs once; home slot (key >> 1) & (slots - 1), then steps of 1, 2, 3, ... to the first free slot
  V   one 64-bit value per slot: the position word itself (one occurrence), or first P word (relative to the bucket) << 32 | count
  P   the position words of the minimizers that occur more than once, in the order of the index's y

A position word: reference id 63..43 | position 42..22 | strand 21 | rank id 20..0.  The minimizers are tests/sketch_model.py's."""
import itertools

import numpy as np

import sketch_model as sm

POS_BITS = 21              # a position, a rank id and a reference id have 21 bits each
MAX_TARGETS = 1 << 21


def index_entries(seqs, w, k, is_hpc, rank=None):
    """{minimizer key (x >> 8) -> [position words, sorted by the index's y = rid << 32 | position << 1 | strand]} of the targets
    `seqs` (bytes or uint8 arrays; the reference id is the place in the list).  rank[i] is target i's rank by name: its id when
    the names are in order, which is the default."""
    assert len(seqs) <= MAX_TARGETS, "at most 2^21 targets"
    rank = list(range(len(seqs))) if rank is None else [int(r) for r in rank]
    assert len(rank) == len(seqs) and all(0 <= r < MAX_TARGETS for r in rank)
    u = np.uint64
    keys, ys, words = [], [], []
    for rid, s in enumerate(seqs):
        assert len(s) < 1 << POS_BITS, "target length < 2^21"
        x, y = sm.sketch(s, w, k, is_hpc)
        if not len(x):
            continue
        keys.append(x >> u(8))
        ys.append(u(rid << 32) | y)
        words.append(u(rid << 43) | (y >> u(1)) << u(22) | (y & u(1)) << u(21) | u(rank[rid]))
    if not keys:
        return {}
    keys, ys, words = np.concatenate(keys), np.concatenate(ys), np.concatenate(words)
    o = np.lexsort((ys, keys))
    keys, words = keys[o], words[o].tolist()
    starts = np.concatenate(([0], np.nonzero(np.diff(keys))[0] + 1, [len(keys)])).tolist()
    return {m: words[s:e] for m, s, e in zip(keys[starts[:-1]].tolist(), starts[:-1], starts[1:])}


def build_image(entries, b_bits=14):
    """{minimizer key -> [packed position words]} -> [B, H, V, P] (uint8 arrays).  Minimizers of one bucket enter its hash table in
    the dict's order (any order gives a table in which every lookup finds its key)."""
    n_b, u = 1 << b_bits, np.uint64
    n = len(entries)
    ms = np.fromiter(entries.keys(), np.uint64, n)
    cnt = np.fromiter((len(v) for v in entries.values()), np.int64, n)
    assert (cnt > 0).all() and (cnt < 1 << 32).all()
    bucket = (ms & u(n_b - 1)).astype(np.int64)
    o = np.argsort(bucket, kind="stable")
    ms, cnt, bucket = ms[o], cnt[o], bucket[o]
    n_keys = np.bincount(bucket, minlength=n_b)
    nb = np.where(n_keys > 0, 4, 0).astype(np.int64)                          # slots: a power of two, at least twice the keys
    while (nb < 2 * n_keys).any():
        nb = np.where(nb < 2 * n_keys, nb << 1, nb)
    slots = (nb + 7) & ~7
    h_base = np.concatenate(([0], np.cumsum(slots)))
    total = int(h_base[-1])
    multi = cnt > 1
    p_first = np.concatenate(([0], np.cumsum(np.where(multi, cnt, 0))))       # first P word of every minimizer, and the total
    p_base = p_first[np.searchsorted(bucket, np.arange(n_b))]                 # ... of every bucket
    assert total < 1 << 36 and int(p_first[-1]) < 1 << 36
    key = ms >> u(b_bits) << u(1)
    assert (key < u(1 << 48)).all()
    first_word = np.fromiter((v[0] for v in entries.values()), np.uint64, n)[o]
    value = np.where(multi, (p_first[:-1] - p_base[bucket]).astype(np.uint64) << u(32) | cnt.astype(np.uint64), first_word)
    # open addressing, all buckets at once: in every round the first minimizer that asks for a free slot gets it, the others of
    # that slot and those on a taken slot step on
    nbk = nb[bucket]
    at, step = ((key >> u(1)).astype(np.int64)) & (nbk - 1), np.zeros(n, np.int64)
    slot_of, taken, pending = np.full(n, -1, np.int64), np.zeros(total, bool), np.arange(n)
    while len(pending):
        gs = h_base[bucket[pending]] + at[pending]
        free = ~taken[gs]
        won_slot, first = np.unique(gs[free], return_index=True)
        winners = pending[free][first]
        slot_of[winners], taken[won_slot] = won_slot, True
        pending = np.setdiff1d(pending, winners, assume_unique=True)
        step[pending] += 1
        at[pending] = (at[pending] + step[pending]) & (nbk[pending] - 1)
    key_of, val_of = np.zeros(total, np.uint64), np.zeros(total, np.uint64)
    key_of[slot_of], val_of[slot_of] = key | (~multi).astype(np.uint64), value
    # flag words: sixteen slots of one table each, "empty" (bit 1) for the free slots of the table proper
    slot_bucket = np.repeat(np.arange(n_b), slots)
    rel = np.arange(total) - h_base[slot_bucket]
    bits = np.where(~taken & (rel < nb[slot_bucket]), u(2) << ((rel & 15) << 1).astype(np.uint64), u(0))
    _, word_of = np.unique(slot_bucket << 32 | rel >> 4, return_inverse=True)
    flag_words = np.zeros(int(word_of.max()) + 1 if total else 0, np.uint64)
    np.add.at(flag_words, word_of, bits)                                      # (distinct bits: a sum is their OR)
    grp = np.zeros((total >> 3, 64), np.uint8)
    grp[:, 0:4] = flag_words[word_of[::8]].astype(np.uint32).view(np.uint8).reshape(-1, 4)
    grp[:, 4:52] = key_of.view(np.uint8).reshape(-1, 8)[:, :6].reshape(-1, 48)
    B = np.zeros((n_b, 2), np.uint64)
    has = nb > 0
    B[has, 0] = (p_base[has].astype(np.uint64) & u(0xff)) << u(56) | nb[has].astype(np.uint64) << u(24)
    B[has, 1] = h_base[:-1][has].astype(np.uint64) << u(28) | p_base[has].astype(np.uint64) >> u(8)
    vals = list(entries.values())
    Pw = np.fromiter(itertools.chain.from_iterable(vals[i] for i in o[multi].tolist()), np.uint64, int(p_first[-1]))
    return [B.reshape(-1).view(np.uint8).copy(), grp.reshape(-1), val_of.view(np.uint8).copy(), Pw.view(np.uint8).copy()]
