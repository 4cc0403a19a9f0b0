#!/usr/bin/env python3
"""Generates tests/golden/frag/*.npz: what the UNMODIFIED reference makes of a fragment's hits after mm_gen_regs in a non-CIGAR run on reads
of several segments (read_result_handle, map.c:870-890): mm_set_parent, mm_select_sub_multi, mm_join_long (chain_post, map.c:238-247),
mm_seg_gen, and per segment mm_set_parent and mm_set_mapq.  Run by hand in the build container only (needs oracle/_ref, `make -C oracle
ref`, for the chains, and the reference's sources): pe.c is not part of oracle/_ref, so this script compiles the reference's pe.c hit.c
misc.c kalloc.c esterr.c chain.c where they lie, with the flags of oracle/Makefile, into a temporary directory outside the repository,
loads the result with ctypes and deletes it.  Nothing compiled and no reference text is kept; only the recorded inputs and outputs are.

Inputs: (a) the anchors of tests/golden/syn_paired_sr.npz and syn_paired_nsegs2_mapont.npz, (b) the seeded fragments of tests/frag_model.py
(shapes(): two segments with orphans; shapes3(): three segments), each under an option grid.  Each file: the read inputs (off + anchors +
n_segs for the device, chain params, min_cnt, hash, qlen, seg_len, mini_pos, ref_len, regs_in + chains_off + b_off + b: the hits and chains
the post steps start from) and per option set NAME: NAME_opt (the chaindp_post_opt_t fields, float64), NAME_rep_len, NAME_seg_regs_off +
NAME_regs (uint8 [n, 80]), and for the sets of A_KEPT NAME_seg_a_off + NAME_seg_a (every segment's anchors); trap_names / trap_seen: what
the file's fragments exercise.

The generator asserts that the restatement (tests/frag_oracle.py) equals the reference on every fragment, and that every exactness trap
of TRAPS occurs somewhere in the files.  Where a trap is a choice the reference makes, the restatement with the other choice (VARIANTS)
must give a different result on some fragment: the float product p->score * pri1, and `is_chi_both ||` of pe.c:25."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frag_model as fm  # noqa: E402
import frag_oracle as fo  # noqa: E402
import oracle_lib as ol  # noqa: E402
import post_oracle as po  # noqa: E402
from minimap2_chaindp_amd import params as P  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(HERE, "frag")
LDS_CAP = 64           # FRAG_LDS_CAP of chaindp_frag.hip
SIZE_LIMIT = max(os.path.getsize(os.path.join(HERE, "post", f)) for f in os.listdir(os.path.join(HERE, "post")))
OPT_KEYS = [k for k, _ in P.PostOpt._fields_]
A_KEPT = ("sr", "cigar", "nonsr")
VARIANTS = ("pri1_double", "no_chi_both")
TRAPS = [b + "_" + o for b in fo.BRANCHES for o in ("no", "yes")] + [
    "best_n_cut", "sync_after_drop", "slot_overwritten", "squeezed_zero", "empty_segment", "reverse_hit", "three_segments", "above_lds_cap",
    "seg_gen_regs_over_64_or_equal_keys", "one_segment_read", "pri1_float_matters", "chi_both_matters"]


class SegT(C.Structure):                 # mm_seg_t, mmpriv.h:44-48
    _fields_ = [("n_u", C.c_int), ("n_a", C.c_int), ("u", C.POINTER(C.c_uint64)), ("a", C.POINTER(C.c_uint64))]


def build_ref():
    """The reference's own functions, compiled where they lie into a temporary directory; (library, directory to delete)."""
    tmp = tempfile.mkdtemp(prefix="fragref_")
    so = os.path.join(tmp, "libfragref.so")
    srcs = [os.path.join(REF, f) for f in ("pe.c", "hit.c", "misc.c", "kalloc.c", "esterr.c", "chain.c")]
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-DHAVE_KALLOC", "-fPIC", "-w", "-I" + REF, "-shared", "-o", so] + srcs + ["-lm"], check=True)
    L = C.CDLL(so)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.mm_set_parent.restype = None
    L.mm_set_parent.argtypes = [vp, f32, i32, vp, i32]
    L.mm_select_sub_multi.restype = None
    L.mm_select_sub_multi.argtypes = [vp, f32, f32, f32, i32, i32, i32, i32, vp, vp, vp]
    L.mm_join_long.restype = None
    L.mm_join_long.argtypes = [vp, vp, i32, vp, vp, vp]
    L.mm_seg_gen.restype = C.POINTER(SegT)
    L.mm_seg_gen.argtypes = [vp, C.c_uint32, i32, vp, i32, vp, vp, vp, vp]
    L.mm_seg_free.restype = None
    L.mm_seg_free.argtypes = [vp, i32, C.POINTER(SegT)]
    L.mm_set_mapq.restype = None
    L.mm_set_mapq.argtypes = [vp, i32, vp, i32, i32, i32, i32]
    return L, tmp


def ref_frag_read(L, opt, max_gap_ref, hash_, qlens, rep_len, ref_len, regs_in, b, mini_pos):
    """map.c:870-890 for one read by the reference's own functions -> per segment (final records, anchors)."""
    if len(qlens) == 1:
        r, a = po.ref_post_read(opt, int(qlens[0]), rep_len, ref_len, regs_in, b, mini_pos)
        return [(r, a)]
    n_segs, qlen = len(qlens), int(sum(qlens))
    ql = np.array(qlens, np.int32)
    n = len(regs_in)
    raw = np.zeros((max(n, 1), ol.REF_REG_BYTES), np.uint8)
    raw[:n, :72] = np.ascontiguousarray(regs_in, ol.REG_DTYPE).view(np.uint8).reshape(n, 80)[:, :72]
    a = np.array(b, np.uint64, copy=True).reshape(-1, 2)
    a_buf = a if len(a) else np.zeros((1, 2), np.uint64)
    mo = po.MapOpt(flag=opt["flag"], min_cnt=opt["min_cnt"], min_chain_score=opt["min_chain_score"], mask_level=opt["mask_level"],
                   pri_ratio=opt["pri_ratio"], best_n=opt["best_n"], max_join_long=opt["max_join_long"], max_join_short=opt["max_join_short"],
                   min_join_flank_sc=opt["min_join_flank_sc"], a=opt["match_sc"], b=opt["sub_diff"] - 2 * opt["match_sc"])
    nn = C.c_int(n)
    if not (opt["flag"] & po.MM_F_ALL_CHAINS):                              # chain_post, map.c:238-247
        L.mm_set_parent(None, opt["mask_level"], nn.value, raw.ctypes.data, opt["sub_diff"])
        L.mm_select_sub_multi(None, opt["pri_ratio"], 0.2, 0.7, max_gap_ref, opt["min_diff"], opt["best_n"], n_segs, ql.ctypes.data, C.addressof(nn),
                              raw.ctypes.data)
        if not (opt["flag"] & (po.MM_F_SPLICE | po.MM_F_SR | po.MM_F_NO_LJOIN)):
            L.mm_join_long(None, C.addressof(mo), qlen, C.addressof(nn), raw.ctypes.data, a_buf.ctypes.data)
    n_regs = (C.c_int * n_segs)()
    regs = (C.c_void_p * n_segs)()
    seg = L.mm_seg_gen(None, int(hash_), n_segs, ql.ctypes.data, nn.value, raw.ctypes.data, n_regs, regs, a_buf.ctypes.data)   # map.c:880
    out = []
    for s in range(n_segs):
        m = n_regs[s]
        L.mm_set_parent(None, opt["mask_level"], m, regs[s], opt["sub_diff"])                                                 # map.c:883
        if not (opt["flag"] & po.MM_F_CIGAR):
            L.mm_set_mapq(None, m, regs[s], opt["min_chain_score"], opt["match_sc"], rep_len, opt["is_sr"])                    # map.c:885
        rec = ol._ref_regs_to_np(regs[s], m) if m else np.zeros(0, ol.REG_DTYPE)
        na = seg[s].n_a
        sa = np.ctypeslib.as_array(seg[s].a, (na * 2,)).copy().reshape(na, 2) if na else np.zeros((0, 2), np.uint64)
        out.append((rec, sa))
        if regs[s]:
            ol._libc.free(regs[s])
    L.mm_seg_free(None, n_segs, seg)
    return out


def grid(rep_len):
    big = np.full_like(rep_len, 1000)
    return {
        "sr": (P.post_preset("sr"), rep_len),
        "best1": (P.post_preset("sr", best_n=1), rep_len),
        "pri0": (P.post_preset("sr", pri_ratio=0.0), rep_len),
        "pri08": (P.post_preset("sr", pri_ratio=0.8), rep_len),
        "cigar": (P.post_preset("sr", flag=P.MM_F_SR | P.MM_F_CIGAR), rep_len),
        "allchains": (P.post_preset("sr", flag=P.MM_F_SR | P.MM_F_ALL_CHAINS), rep_len),
        "nonsr": (P.post_preset("map-ont", min_cnt=2, min_chain_score=25, min_diff=42, pri_ratio=0.5, max_join_long=400, min_join_flank_sc=40), rep_len),
        "replen": (P.post_preset("sr"), big),
    }


def run_grid(L, name, inp, reads, max_gap_ref, seen_all):
    """reads: per read (regs_in, b, qlens, mini_pos).  Writes one file with every option set."""
    out = dict(inp)
    seen = {k: False for k in TRAPS}
    for cname, (opt, rep_len) in grid(inp["rep_len"]).items():
        od = po.opt_dict(opt)
        regs_all, a_all = [], []
        for r, (regs, b, qlens, mp) in enumerate(reads):
            args = (od, max_gap_ref, int(inp["hash"][r]), qlens, int(rep_len[r]), inp["ref_len"], regs, b, mp)
            got = ref_frag_read(L, *args)
            tr = fo.FragTrace()
            mine = fo.frag_read(*args, tr=tr)
            assert len(got) == len(mine) == len(qlens)
            for s in range(len(qlens)):
                assert got[s][0].tobytes() == mine[s][0].tobytes() and got[s][1].tobytes() == mine[s][1].tobytes(), \
                    f"{name}/{cname} read {r} segment {s}: restatement != reference"
                if len(qlens) > 1:
                    assert (got[s][0]["div"] == np.float32(-1.0)).all()
            for v, key in zip(VARIANTS, ("pri1_float_matters", "chi_both_matters")):
                alt = fo.frag_read(*args, variant=v)
                seen[key] |= any(alt[s][0].tobytes() != got[s][0].tobytes() for s in range(len(qlens)))
            if len(qlens) > 1:
                for bname, (no, yes) in tr.branch.items():
                    seen[bname + "_no"] |= no > 0; seen[bname + "_yes"] |= yes > 0
                seen["best_n_cut"] |= tr.best_n_cut
                seen["sync_after_drop"] |= tr.multi_dropped and tr.sync_ran
                seen["slot_overwritten"] |= tr.slot_overwritten_read
                seen["squeezed_zero"] |= tr.squeezed_zero
                seen["empty_segment"] |= tr.empty_segment
                seen["reverse_hit"] |= tr.reverse_hit
                seen["three_segments"] |= len(qlens) == 3
                seen["above_lds_cap"] |= len(regs) > LDS_CAP
                seen["seg_gen_regs_over_64_or_equal_keys"] |= tr.seg_chains_max > LDS_CAP or tr.seg_equal_keys
            else:
                seen["one_segment_read"] |= bool((inp["n_segs"] > 1).any())
            regs_all += [g[0] for g in got]; a_all += [g[1].reshape(-1, 2) for g in got]
        out[cname + "_opt"] = np.array([od[k] for k in OPT_KEYS], np.float64)
        out[cname + "_rep_len"] = np.asarray(rep_len, np.int32)
        out[cname + "_seg_regs_off"] = np.concatenate([[0], np.cumsum([len(x) for x in regs_all])]).astype(np.int64)
        out[cname + "_regs"] = np.concatenate(regs_all).view(np.uint8).reshape(-1, 80)
        if cname in A_KEPT:
            out[cname + "_seg_a_off"] = np.concatenate([[0], np.cumsum([len(x) for x in a_all])]).astype(np.int64)
            out[cname + "_seg_a"] = np.concatenate(a_all)
    out["trap_names"] = np.array(TRAPS)
    out["trap_seen"] = np.array([seen[k] for k in TRAPS])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= SIZE_LIMIT, (path, os.path.getsize(path), SIZE_LIMIT)
    for k in TRAPS:
        seen_all[k] |= seen[k]
    print(f"{name}: {len(reads)} reads, {len(inp['regs_in'])} hits in, {os.path.getsize(path)} B; traps here: {sum(seen.values())}/{len(TRAPS)}")


def from_anchors(L, name, sh, par, min_cnt, seen_all):
    """sh: dict(off, anchors, n_segs, seg_len, qlen, mini_pos_off, mini_pos, rep_len) -> chains by the reference, then the grid."""
    R = len(sh["qlen"])
    hash_ = (np.arange(R, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(sh["n_segs"])])
    reads, us, bs, regs_l = [], [], [], []
    for r in range(R):
        a = np.ascontiguousarray(sh["anchors"][sh["off"][r]:sh["off"][r + 1]])
        pr = P.ChainParams(*par.astuple()); pr.n_segs = int(sh["n_segs"][r])
        _, _, _, seeds = ol.ref_fpv_seeds(pr, a)
        u, b = ol.ref_bottom(min_cnt, par.min_sc, pr.n_segs, seeds) if len(seeds) else (np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64))
        b = b.reshape(-1, 2)
        regs = ol.ref_gen_regs(int(hash_[r]), int(sh["qlen"][r]), u, b)
        mp = sh["mini_pos"][sh["mini_pos_off"][r]:sh["mini_pos_off"][r + 1]]
        reads.append((regs, b, [int(x) for x in sh["seg_len"][first[r]:first[r + 1]]], mp)); us.append(u); bs.append(b); regs_l.append(regs)
    allr = np.concatenate(regs_l)
    n_ref = int(allr["rid"].max()) + 1
    ref_len = (np.arange(n_ref, dtype=np.int64) * 37 % 5000 + int(allr["re"].max()) + 100).astype(np.int32)
    pv = np.array(list(par.astuple())[:6] + [int(sh["n_segs"].max()), min_cnt], np.int32)
    inp = dict(params=pv, off=sh["off"], anchors=sh["anchors"], n_segs=sh["n_segs"], seg_len=sh["seg_len"], hash=hash_, qlen=sh["qlen"],
               mini_pos_off=sh["mini_pos_off"], mini_pos=sh["mini_pos"], rep_len=sh["rep_len"], ref_len=ref_len,
               regs_in=allr.view(np.uint8).reshape(-1, 80), chains_off=np.concatenate([[0], np.cumsum([len(u) for u in us])]).astype(np.int64),
               b_off=np.concatenate([[0], np.cumsum([len(b) for b in bs])]).astype(np.int64), b=np.concatenate(bs))
    run_grid(L, name, inp, reads, par.max_dist_x, seen_all)


def from_fixture(L, name, par, seen_all):
    """The anchors of an existing two-segment fixture.  Its segment ids are random per hit, unrelated to the positions, so the fragment is
    cut as (0, qlen): the one cut that keeps every per-segment coordinate non-negative, as real reads' are (mm_set_parent packs
    coordinates into unsigned words; negative ones are outside what either path computes)."""
    g = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    off, a = g["off"].astype(np.int64), g["anchors"]
    R = len(off) - 1
    qmax = int((a[:, 1] & np.uint64(0xffffffff)).max()) + 4
    l0 = 0
    rng = np.random.default_rng(5)
    mpo, mps = [0], []
    for r in range(R):
        mp = np.array([21 << 32 | q for q in range(5, qmax, 13)], np.uint64)
        mps.append(mp); mpo.append(mpo[-1] + len(mp))
    sh = dict(off=off, anchors=a, n_segs=np.full(R, 2, np.int32), seg_len=np.tile(np.array([l0, qmax - l0], np.int32), R), qlen=np.full(R, qmax, np.int32),
              mini_pos_off=np.array(mpo, np.int64), mini_pos=np.concatenate(mps), rep_len=rng.integers(0, 60, size=R).astype(np.int32))
    from_anchors(L, name, sh, par, int(g["min_cnt"]), seen_all)


def main():
    assert ol.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(OUT, exist_ok=True)
    L, tmp = build_ref()
    try:
        seen = {k: False for k in TRAPS}
        from_fixture(L, "syn_paired_sr", P.preset("sr"), seen)
        from_fixture(L, "syn_paired_nsegs2_mapont", P.preset("map-ont", n_segs=2), seen)
        from_anchors(L, "syn_frag", fm.shapes(), P.preset("sr"), 2, seen)
        from_anchors(L, "syn_frag3", fm.shapes3(), P.preset("sr", n_segs=3), 2, seen)
    finally:
        del L
        shutil.rmtree(tmp, ignore_errors=True)
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"traps never hit: {missing}"
    print("every trap hit:", ", ".join(seen))


if __name__ == "__main__":
    main()
