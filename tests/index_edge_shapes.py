"""CHECKER ONLY: minimizer lists built directly (no sequences) that put the index build on every edge of its table and sort logic.
A shape: name, b (bucket bits), mini uint64[n, 2], rank (or None), and `hits`: what the model's route / image must show for the shape to
be what its name says (tests/test_index_edge_shapes_cpu.py asserts it; the GPU tier compares the device with the model on the same lists).

A minimizer: x = m << 8 | span with m = hi << b | bucket, y = rid << 32 | pos << 1 | strand."""
import numpy as np

import index_build_model as ibm

TILE = 1024                                   # records per workgroup of a radix pass (IX_TILE, chaindp_kernels.h)
KEY_COUNTS = (1, 3, 4, 6, 7, 12, 13, 16, 17, 25, 26)   # around the expansion bounds of 4, 8, 16 and 32 slots (upper = 3, 6, 12, 25)


def mini_of(b, bucket, hi, rid, pos, strand=0, span=15):
    m = (np.asarray(hi, np.uint64) << np.uint64(b)) | np.asarray(bucket, np.uint64)
    x = m << np.uint64(8) | np.uint64(span)
    y = np.asarray(rid, np.uint64) << np.uint64(32) | np.asarray(pos, np.uint64) << np.uint64(1) | np.asarray(strand, np.uint64)
    out = np.stack(np.broadcast_arrays(np.atleast_1d(x), np.atleast_1d(y)), axis=1).astype(np.uint64)
    assert len(np.unique(out, axis=0)) == len(out)
    return out


def _shuffled(rs, mini):
    return mini[rs.permutation(len(mini))]


def _key_counts(b):
    rs = np.random.RandomState(100 + b)
    parts = []
    for i, n in enumerate(KEY_COUNTS):
        bucket = i % (1 << b)
        hi = rs.permutation(1 << 12)[:n].astype(np.uint64) * np.uint64(len(KEY_COUNTS)) + np.uint64(i)   # distinct over the shape
        parts.append(mini_of(b, bucket, hi, rs.randint(0, 5, n), rs.randint(0, 1 << 20, n), rs.randint(0, 2, n)))
    return _shuffled(rs, np.concatenate(parts))


def _one_home(b, n):
    """n keys of one bucket whose hashes agree in their low 10 bits: one home slot in every table size up to 1024"""
    rs = np.random.RandomState(7)
    hi = (rs.choice(1 << 12, n, replace=False).astype(np.uint64) << np.uint64(10)) | np.uint64(5)
    return _shuffled(rs, mini_of(b, 3, hi, 0, np.arange(n)))


def _kick_chain(b, n_keys=13, want=3):
    """a bucket whose expansion moves a chain of `want` elements or more at one step: found by trying seeded key sets on the model"""
    for seed in range(10000):
        rs = np.random.RandomState(seed)
        hi = np.sort(rs.choice(1 << 16, n_keys, replace=False)).astype(np.uint64)
        if ibm.khash_table([int(h) << 1 | 1 for h in hi])[3] >= want:
            return _shuffled(rs, mini_of(b, 9, hi, 1, np.arange(n_keys)))
    raise AssertionError("no key set with a long kick-out chain")


def _groups(b):
    """groups of 1, 2 and 257 occurrences, over several sequences and both strands, in one bucket and in another"""
    rs = np.random.RandomState(3)
    parts = [mini_of(b, 1, 11, 2, 100), mini_of(b, 1, 12, [0, 3], [7, 7], [1, 0]),
             mini_of(b, 1, 13, rs.randint(0, 4, 257), np.arange(257) * 3, rs.randint(0, 2, 257), span=19),
             mini_of(b, 0, 13, [1, 1], [500, 400])]
    return _shuffled(rs, np.concatenate(parts))


def _random(n, b, seed):
    """n minimizers with distinct m: as many groups as minimizers"""
    rs = np.random.RandomState(seed)
    m = rs.permutation(np.unique(rs.randint(0, 1 << 30, 2 * n + 8)))[:n].astype(np.uint64)
    x = m << np.uint64(8) | np.uint64(15)
    y = rs.randint(0, 8, n).astype(np.uint64) << np.uint64(32) | rs.randint(0, 1 << 21, n).astype(np.uint64)
    return np.stack((x, y), axis=1)


def _one_digit(b):
    """every record equal but for the lowest byte of y: fifteen of the sixteen radix digits are constant"""
    return _shuffled(np.random.RandomState(5), mini_of(b, 2, 77, 0, np.arange(100), 1))


def shapes():
    rank8 = np.array([5, 2, 7, 0, 1, 6, 3, 4], np.uint32)
    out = []
    for b in (1, 6, 14):       # b = 1: the eleven counts share two buckets (68 keys, and 62 that pass the bound of 64 slots)
        hits = dict(buckets=2, expanded=1, max_keys=68) if b == 1 else dict(buckets=len(KEY_COUNTS), expanded=5, max_keys=26)
        out.append(dict(name=f"key_counts_b{b}", b=b, mini=_key_counts(b), rank=rank8, hits=dict(hits, distinct=sum(KEY_COUNTS))))
    for n in (12, 13, 26):
        out.append(dict(name=f"one_home_slot_{n}", b=14, mini=_one_home(14, n), rank=None,
                        hits=dict(distinct=n, buckets=1, max_keys=n, expanded=int(n > ibm.upper(ibm.first_size(n))))))
    out.append(dict(name="kick_out_chain", b=14, mini=_kick_chain(14), rank=rank8, hits=dict(expanded=1, max_chain=lambda v: v >= 3)))
    out.append(dict(name="groups_1_2_257", b=6, mini=_groups(6), rank=rank8, hits=dict(minimizers=262, distinct=4, buckets=2)))
    out.append(dict(name="empty", b=14, mini=np.zeros((0, 2), np.uint64), rank=None,
                    hits=dict(minimizers=0, distinct=0, buckets=0, passes_run=0)))
    for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.append(dict(name=f"sort_{n}", b=14, mini=_random(n, 14, n), rank=rank8, hits=dict(minimizers=n, distinct=n)))
    out.append(dict(name="sort_one_digit", b=14, mini=_one_digit(14), rank=None, hits=dict(passes_run=1, passes_skipped=15, distinct=1)))
    return out


def shape_hits(shape, route):
    """the names of `hits` the route misses (empty: the shape is what it says)"""
    return [k for k, want in shape["hits"].items() if not (want(route[k]) if callable(want) else route[k] == want)]
