"""ctypes access to oracle/_ref/libmm2sketch_ref.so: the unmodified reference's mm_sketch (sketch.c:77-143), which takes w, k and
is_hpc as arguments and therefore reaches what no preset of its dumper does (even k, w up to 255, w >= k + 2, the bytes 0..3).
CPU TIER ONLY: the library exists where oracle/_ref is built; where it is not, SketchRecord holds a case to what the reference
returned when tests/golden/make_sketch_edge_golden.py was run (tests/golden/sketch_edges/ref_digests.json), as oracle_lib.RefRecord
does for the chain stages.  Never imported by a GPU test."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKETCH_SO = os.path.join(ROOT, "oracle", "_ref", "libmm2sketch_ref.so")
DIGESTS = os.path.join(ROOT, "tests", "golden", "sketch_edges", "ref_digests.json")


class _V(C.Structure):                       # mm128_v (minimap.h:41): n, m, a
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


_lib = None
_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def have():
    return os.path.exists(SKETCH_SO)


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(SKETCH_SO)
        _lib.mm_sketch.restype = None
        _lib.mm_sketch.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(_V)]
    return _lib


def sketch(seq, w, k, is_hpc, rid=0):
    """mm_sketch(NULL, seq, len, w, k, rid, is_hpc) -> uint64[n, 2] (x, y).  An empty sequence yields nothing (mm_sketch asserts len > 0)."""
    s = bytes(seq) if not isinstance(seq, np.ndarray) else seq.astype(np.uint8).tobytes()
    if len(s) == 0:
        return np.zeros((0, 2), np.uint64)
    v = _V(0, 0, None)
    lib().mm_sketch(None, s, len(s), int(w), int(k), int(rid), int(bool(is_hpc)), C.byref(v))
    out = np.zeros((v.n, 2), np.uint64)
    if v.n:
        C.memmove(out.ctypes.data, v.a, v.n * 16)
    if v.a:
        _libc.free(v.a)                      # km == NULL: kalloc falls back to malloc / free
    return out


def sketch_batch(seq, seq_off, w, k, is_hpc, n_segs_per_read=None):
    """mini_off, mini of a batch with the rid and shift of collect_minimizers (map.c:87-99) applied here, as sketch_model.sketch_batch does."""
    seq = np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else seq
    n_seqs = len(seq_off) - 1
    segs = np.ones(n_seqs, np.int64) if n_segs_per_read is None else np.asarray(n_segs_per_read, np.int64)
    out, off, q = [], [0], 0
    for ns in segs:
        shift, n = 0, 0
        for rid in range(int(ns)):
            s = seq[int(seq_off[q]):int(seq_off[q + 1])]
            m = sketch(s, w, k, is_hpc, rid)
            m[:, 1] += np.uint64(shift << 1)
            out.append(m)
            n += len(m); shift += len(s); q += 1
        off.append(off[-1] + n)
    assert q == n_seqs
    mini = np.concatenate(out) if out else np.zeros((0, 2), np.uint64)
    return np.array(off, np.int64), mini.reshape(-1, 2).astype(np.uint64)


def digest(mini_off, mini):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(mini_off, "<i8").tobytes())
    h.update(np.ascontiguousarray(mini, "<u8").tobytes())
    return {"sha256": h.hexdigest(), "n": int(len(mini))}


_record = None


def record():
    global _record
    if _record is None:
        _record = json.load(open(DIGESTS)) if os.path.exists(DIGESTS) else {}
    return _record


def check(key, ours, theirs=None):
    """oracle_lib.RefRecord's rule for one case: ours = (mini_off, mini) of the model; where the library is built, theirs = the live
    reference's, and live reference == model == record; where it is not, model == record."""
    rec = record()
    assert key in rec, f"no recorded reference result for {key} (tests/golden/make_sketch_edge_golden.py)"
    mine = digest(*ours)
    if have():
        assert theirs is not None, f"{key}: the reference library is built but was not run"
        live = digest(*theirs)
        assert mine == live, f"{key}: the model differs from the live reference: {mine} != {live}"
        assert rec[key] == live, f"{key}: the recorded reference result differs from the reference's"
    else:
        assert mine == rec[key], f"{key}: the model differs from the recorded reference result"
