#!/usr/bin/env python3
"""Generates tests/golden/ksw/*.npz: what the UNMODIFIED reference's ksw_extd2_sse makes of the named problems of tests/ksw_shapes.py and
of its seeded fuzz batch (build container only: it needs the reference's sources and a C compiler).

ksw2_extd2_sse.c and kalloc.c are compiled where they lie (-DHAVE_KALLOC, km = NULL) into a shared object in a temporary directory
outside the repository, which is removed at the end; nothing of the reference is copied.  One file per call of the tests, i.e. per
scoring set: named_<set>.npz and fuzz_<set>.npz, each with scoring[6], the flat inputs of ksw_shapes.pack(), name[n], ez[n, 10],
cigar_off[n + 1], cigar, and clean_differs[n] / first_differs[n]: where the model's two variants (out-of-band cells reset; the first
maximum as max_t) do not give the reference's answer.

Asserts on the way: the model equals the reference on every problem; each variant differs on at least one; every accepted flag
combination, both reach_end values, zdropped by the band and by Z-drop, and the swap of the gap costs occur.  Prints the
reference's rate (cell updates per second, one thread) over the fuzz batch and the two large problems, for DESIGN.md."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ksw_model as M  # noqa: E402
import ksw_shapes as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")          # as oracle/Makefile
OUT = os.path.join(HERE, "ksw")


class Ez(C.Structure):
    _fields_ = [("max_zdropped", C.c_uint32), ("max_q", C.c_int), ("max_t", C.c_int), ("mqe", C.c_int), ("mqe_t", C.c_int), ("mte", C.c_int),
                ("mte_q", C.c_int), ("score", C.c_int), ("m_cigar", C.c_int), ("n_cigar", C.c_int), ("reach_end", C.c_int), ("cigar", C.POINTER(C.c_uint32))]


def build(tmp):
    so = os.path.join(tmp, "libksw_ref.so")
    subprocess.check_call(["gcc", "-O2", "-msse4.1", "-fPIC", "-shared", "-DHAVE_KALLOC", "-o", so, os.path.join(REF, "ksw2_extd2_sse.c"),
                           os.path.join(REF, "kalloc.c")])
    lib = C.CDLL(so)
    lib.ksw_extd2_sse.restype = None
    lib.ksw_extd2_sse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int8, C.c_void_p, C.c_int8, C.c_int8, C.c_int8, C.c_int8,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Ez)]
    return lib, C.CDLL(None).free


def simple_mat(a, b):
    """ksw_gen_simple_mat(5, mat, a, b) of align.c:9-21."""
    mat = np.zeros((5, 5), np.int8)
    mat[:4, :4] = -abs(b)
    mat[np.arange(4), np.arange(4)] = abs(a)
    return mat


def ref_call(lib, free, c):
    a, b, q, e, q2, e2 = S.SCORING[c["scoring"]]
    mat = simple_mat(a, b)
    qs, ts = np.ascontiguousarray(c["query"]), np.ascontiguousarray(c["target"])
    ez = Ez()
    lib.ksw_extd2_sse(None, len(qs), qs.ctypes.data, len(ts), ts.ctypes.data, 5, mat.ctypes.data, q, e, q2, e2, c["w"], c["zdrop"], c["end_bonus"],
                      c["flag"], C.byref(ez))
    out = np.array([ez.max_zdropped & 0x7fffffff, ez.max_zdropped >> 31, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score,
                    ez.reach_end], np.int64).astype(np.int32)
    cig = np.array([ez.cigar[k] for k in range(ez.n_cigar)], np.uint32)
    if ez.cigar:
        free(ez.cigar)
    return out, cig


def cells(c):
    ql, tl = len(c["query"]), len(c["target"])
    if not ql or not tl:
        return 0
    w = c["w"] if c["w"] >= 0 else max(ql, tl)
    return sum(max(0, min(tl - 1, r, (r + w) >> 1) - max(0, r - ql + 1, (r - w + 1) >> 1) + 1) for r in range(ql + tl - 1))


def main():
    tmp = tempfile.mkdtemp(prefix="ksw_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib, free = build(tmp)
        free.argtypes = [C.c_void_p]
        os.makedirs(OUT, exist_ok=True)
        seen_flags, reach, zdrop_band, zdrop_z, swapped, n_clean, n_first, total = set(), set(), 0, 0, 0, 0, 0, 0
        for kind, cases in (("named", S.named_cases()), ("fuzz", S.fuzz_cases())):
            for sc, group in S.groups(cases).items():
                a, b, q, e, q2, e2 = S.SCORING[sc]
                ezs, cigs, clean, first = [], [], [], []
                for c in group:
                    ez, cig = ref_call(lib, free, c)
                    args = (c["query"], c["target"], a, b, q, e, q2, e2, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
                    mez, mcig = M.ksw_extd(*args)
                    assert np.array_equal(mez, ez) and np.array_equal(mcig, cig), (c["name"], mez, ez, mcig, cig)
                    for variant, rec in (("clean", clean), ("first", first)):
                        vez, vcig = M.ksw_extd(*args, variant=variant)
                        rec.append(not (np.array_equal(vez, ez) and np.array_equal(vcig, cig)))
                    ezs.append(ez); cigs.append(cig)
                    computed = len(c["query"]) and len(c["target"]) and sc != "early"
                    if computed:
                        seen_flags.add(c["flag"]); swapped += q2 + e2 < q + e
                        if not c["flag"] & 1:
                            reach.add(int(ez[9]))
                        if ez[1]:
                            # the band ran out (st > en) if no diagonal up to the end could have dropped: tell the two apart by a run without Z-drop
                            nz, _ = M.ksw_extd(*args[:9], -1, *args[10:])
                            zdrop_band += int(nz[1]); zdrop_z += int(not nz[1])
                p = S.pack(group)
                off = np.concatenate([[0], np.cumsum([len(x) for x in cigs])]).astype(np.int64)
                np.savez_compressed(os.path.join(OUT, f"{kind}_{sc}.npz"), scoring=np.array([a, b, q, e, q2, e2], np.int32),
                                    name=np.array([c["name"] for c in group]), ez=np.array(ezs, np.int32).reshape(-1, 10), cigar_off=off,
                                    cigar=np.concatenate(cigs).astype(np.uint32) if off[-1] else np.zeros(0, np.uint32),
                                    clean_differs=np.array(clean, bool), first_differs=np.array(first, bool), **p)
                n_clean += sum(clean); n_first += sum(first); total += len(group)
                print(f"{kind}_{sc}.npz: {len(group)} problems, {off[-1]} CIGAR words, clean differs on {sum(clean)}, first on {sum(first)}")
        assert n_clean >= 1 and n_first >= 1, (n_clean, n_first)
        assert seen_flags >= set(S.FLAG_COMBOS), sorted(set(S.FLAG_COMBOS) - seen_flags)
        assert reach == {0, 1} and zdrop_band and zdrop_z and swapped, (reach, zdrop_band, zdrop_z, swapped)
        print(f"{total} problems; the model equals the reference on all; clean differs on {n_clean}, first on {n_first}; "
              f"zdropped by the band {zdrop_band}, by Z-drop {zdrop_z}")
        # the reference's rate, one thread
        for label, cases in (("fuzz batch", S.fuzz_cases()), ("two large problems", [c for c in S.named_cases() if c["name"].startswith("large_")])):
            n_cells = sum(cells(c) for c in cases if c["scoring"] != "early")
            best = 1e30
            for _ in range(5):
                t0 = time.perf_counter()
                for c in cases:
                    ref_call(lib, free, c)
                best = min(best, time.perf_counter() - t0)
            print(f"reference, one thread, {label}: {n_cells} cells in the band, {best * 1e3:.2f} ms, {n_cells / best / 1e9:.3f} G cell updates / s "
                  "(the fuzz figure includes the ctypes call, a few microseconds per problem)")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
