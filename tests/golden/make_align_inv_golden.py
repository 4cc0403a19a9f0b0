#!/usr/bin/env python3
"""Generates tests/golden/align_inv/*.npz: what the UNMODIFIED reference's mm_align1_inv, under the rule of the loop around it, makes of
the scenes of tests/inv_shapes.py (build container only: it needs the reference's sources and a C compiler).

A driver of this script's own #includes align.c where it lies, to reach the static mm_align1_inv, and is compiled beside the files it
needs into a shared object in a temporary directory outside the repository, which is removed at the end; nothing of the reference is
copied.  One file per scene with the flat inputs of inv_shapes.pack() and every output word: made, r_inv, extra, cigar_off, cigar, and
beside them ll (score, qe, te of every candidate) and prob (qlen, tlen, w of every extension).

The loop's rule is the reference's own: a pair is given to mm_align1_inv with the record the loop would find to its left, which after
an inversion was made is that inversion (split 0), so the reference itself returns early.  made = 3 is then written where the pair,
taken by itself, passes the early returns; 2 and 4 are told apart by ksw_ll_i16's score.

Asserts on the way: ll_ends (tests/inv_model.py) equals the compiled ksw_ll_i16 in score, qe and te on every stretch of every scene and
on a fuzz of its own up to 2000 bases under two scoring sets; the model equals the reference on every pair; no pair of any scene falls
into unspecified behaviour; every class in COVER occurred.  Prints the reference's one-thread ksw_ll_i16 rate for DESIGN.md."""
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
import align_model as A  # noqa: E402
import inv_model as M  # noqa: E402
import inv_shapes as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(HERE, "align_inv")

COVER = ("early_no_split_inv", "early_split1", "early_split2", "early_parent1", "early_parent2", "early_rid", "early_rev", "early_ql_low",
         "early_ql_high", "early_tl_low", "early_tl_high", "parent_is_id", "parent_tmp_pri", "ql_at_min", "ql_at_max_gap", "tl_at_min",
         "tl_at_max_gap", "strand_0", "strand_1", "score_at_min_dp_max", "score_below_min_dp_max_by_1", "low_score", "made", "no_cigar",
         "q_off_-7", "q_off_-4", "q_off_-1", "q_off_0_no_padding", "q_off_pos", "qe_in_padding", "wildcard_behind_best", "qe_tie_middle",
         "saturated", "route_lds", "route_wide", "route_global", "ext_zdropped", "fix_cigar_leading_I_strand_0", "fix_cigar_leading_I_strand_1",
         "fix_cigar_leading_D_strand_0", "fix_cigar_leading_D_strand_1", "n_ambi_strand_0", "n_ambi_strand_1", "skipped_behind_made",
         "made_behind_failed", "read_with_one_region", "read_without_regions", "ql_lt_tl", "ql_gt_tl") + tuple(
    "%s_%d" % (nm, v) for nm in ("ql", "tl") for v in (63, 64, 65, 127, 128, 129)) + tuple("ql_mod8_%d" % k for k in (7, 0, 1))

DRIVER = r"""
#include "%(ref)s/align.c"
extern unsigned char seq_nt4_table[256];
/* what the files beside this one expect of the program they are part of (map.c, main.c, the accelerator's driver): not used on this path */
struct mm_idx_bucket_s *g_B = 0;
int32_t g_b = 0;
double send_task1[100], send_task2[100], process_result[100];
void fpga_load_index(void *addr, int size, int type) { (void)addr; (void)size; (void)type; }
/* the sequence half of mm_idx_str (index.c:751-769): lengths, offsets and the 4-bit packed bases mm_idx_getseq reads */
void *drv_index(int w, int k, int n, const char **seqs)
{
	mm_idx_t *mi = (mm_idx_t*)calloc(1, sizeof(mm_idx_t));
	uint64_t sum_len = 0;
	int i;
	for (i = 0; i < n; ++i) sum_len += strlen(seqs[i]);
	mi->w = w, mi->k = k, mi->b = 10, mi->flag = MM_I_NO_NAME, mi->n_seq = n;
	mi->seq = (mm_idx_seq_t*)calloc(n, sizeof(mm_idx_seq_t));
	mi->S = (uint32_t*)calloc((sum_len + 7) / 8, 4);
	for (i = 0, sum_len = 0; i < n; ++i) {
		uint32_t j;
		mi->seq[i].offset = sum_len, mi->seq[i].len = strlen(seqs[i]);
		for (j = 0; j < mi->seq[i].len; ++j) mm_seq4_set(mi->S, sum_len + j, seq_nt4_table[(uint8_t)seqs[i][j]]);
		sum_len += mi->seq[i].len;
	}
	return mi;
}
void drv_index_free(void *mi_) { mm_idx_t *mi = (mm_idx_t*)mi_; free(mi->seq); free(mi->S); free(mi); }
int drv_inv(void *mi, const int *o, int qlen, const char *seq, const mm_reg1_t *r1, const mm_reg1_t *r2, mm_reg1_t *r_inv, int32_t *extra,
            uint32_t *cigar, int cap)
{
	mm_mapopt_t opt;
	uint8_t *qseq0[2];
	ksw_extz_t ez;
	int i, ret;
	mm_mapopt_init(&opt);
	opt.a = o[0], opt.b = o[1], opt.q = o[2], opt.e = o[3], opt.q2 = o[4], opt.e2 = o[5], opt.bw = o[6], opt.zdrop = o[7], opt.zdrop_inv = o[8];
	opt.end_bonus = o[9], opt.min_cnt = o[10], opt.min_chain_score = o[11], opt.min_dp_max = o[12], opt.min_ksw_len = o[13], opt.max_gap = o[14];
	opt.flag = o[15];
	qseq0[0] = (uint8_t*)malloc(qlen * 2 + 2); qseq0[1] = qseq0[0] + qlen;
	for (i = 0; i < qlen; ++i) {
		int c = seq_nt4_table[(uint8_t)seq[i]];
		qseq0[0][i] = c; qseq0[1][qlen - 1 - i] = c < 4? 3 - c : 4;
	}
	memset(&ez, 0, sizeof(ez));
	ret = mm_align1_inv(0, &opt, (const mm_idx_t*)mi, qlen, qseq0, r1, r2, r_inv, &ez);
	memset(extra, 0, 5 * sizeof(int32_t));
	if (r_inv->p) {
		int n = r_inv->p->n_cigar;
		extra[0] = 1, extra[1] = r_inv->p->dp_score, extra[2] = r_inv->p->dp_max, extra[3] = r_inv->p->n_ambi, extra[4] = n;
		if (n <= cap) memcpy(cigar, r_inv->p->cigar, n * 4);
		free(r_inv->p); r_inv->p = 0;
	}
	kfree(0, ez.cigar);
	free(qseq0[0]);
	return ret;
}
int drv_ll3(int qlen, const uint8_t *q, int tlen, const uint8_t *t, int a, int b, int gapo, int gape, int *out3)
{
	int8_t mat[25];
	void *qp;
	ksw_gen_simple_mat(5, mat, a, b);
	qp = ksw_ll_qinit(0, 2, qlen, q, 5, mat);
	out3[0] = ksw_ll_i16(qp, tlen, t, gapo, gape, &out3[1], &out3[2]);
	kfree(0, qp);
	return out3[0];
}
"""
SOURCES = ("index.c", "hit.c", "ksw2_extd2_sse.c", "ksw2_extz2_sse.c", "ksw2_exts2_sse.c", "ksw2_ll_sse.c", "kalloc.c", "sketch.c", "misc.c", "bseq.c",
           "kthread.c", "options.c")


def build(tmp):
    drv = os.path.join(tmp, "inv_driver.c")
    with open(drv, "w") as f:
        f.write(DRIVER % {"ref": REF})
    so = os.path.join(tmp, "libinv_ref.so")
    subprocess.check_call(["gcc", "-O2", "-msse4.1", "-fPIC", "-shared", "-w", "-DHAVE_KALLOC", "-I" + REF, "-o", so, drv]
                          + [os.path.join(REF, s) for s in SOURCES] + ["-lm", "-lz", "-lpthread"])
    lib = C.CDLL(so)
    lib.drv_index.restype = C.c_void_p
    lib.drv_index.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    lib.drv_index_free.argtypes = [C.c_void_p]
    lib.drv_inv.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p] + [C.c_void_p] * 5 + [C.c_int]
    lib.drv_ll3.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def ref_ll(lib, q, t, a, b, gapo, gape):
    out = np.zeros(3, np.int32)
    lib.drv_ll3(len(q), np.ascontiguousarray(q, np.uint8).ctypes.data, len(t), np.ascontiguousarray(t, np.uint8).ctypes.data, a, b, gapo, gape, out.ctypes.data)
    return tuple(int(v) for v in out)


def ref_scene(lib, p, model_made, model_ll):
    """The reference over a packed scene, its loop's rule included: (made, r_inv, extra, cigar_off, cigar)."""
    n_t = len(p["tseq_off"]) - 1
    tseqs = [bytes(p["tseq"][p["tseq_off"][i]:p["tseq_off"][i + 1]]) for i in range(n_t)]
    opt = np.ascontiguousarray(p["opt"], np.int32)
    o = dict(zip(A.OPT_FIELDS, (int(v) for v in opt)))
    mi = lib.drv_index(10, int(opt[16]), n_t, (C.c_char_p * n_t)(*tseqs))
    assert mi
    regs = p["regs"]
    n = len(regs)
    made, r_inv, extra = np.zeros(n, np.int32), np.zeros(n, S.REG_DTYPE), np.zeros(n, S.EXTRA_DTYPE)
    cigs, c = [], 0
    for rd in range(len(p["seq_off"]) - 1):
        seq = bytes(p["seq"][p["seq_off"][rd]:p["seq_off"][rd + 1]])
        left = None
        for g in range(int(p["regs_off"][rd]), int(p["regs_off"][rd + 1])):
            cig = np.zeros(2 * len(seq) + 16, np.uint32)
            if left is not None and regs["bits"][g] & M.BIT_SPLIT_INV:                      # align.c:748
                ret = lib.drv_inv(mi, opt.ctypes.data, len(seq), seq, left.ctypes.data, regs[g:g + 1].ctypes.data, r_inv[g:g + 1].ctypes.data,
                                  extra[g:g + 1].ctypes.data, cig.ctypes.data, len(cig))
                assert extra["n_cigar"][g] <= len(cig)
                candidate = M.early_return(o, S.reg_dict(regs[g - 1]), S.reg_dict(regs[g]))[0] is None
                if ret:
                    made[g] = M.MADE
                elif candidate:
                    tested = M.early_return(o, S.reg_dict(left[0]), S.reg_dict(regs[g]))[0] is None
                    made[g] = M.SKIPPED if not tested else M.LOW_SCORE if model_ll[c][0] < o["min_dp_max"] else M.NO_CIGAR
                c += candidate
            cigs.append(cig[:extra["n_cigar"][g]])
            left = r_inv[g:g + 1].copy() if made[g] == M.MADE else regs[g:g + 1]               # :750-751: the loop steps over the inversion
    lib.drv_index_free(mi)
    off = np.concatenate([[0], np.cumsum([len(c_) for c_ in cigs])]).astype(np.int64)
    return made, r_inv, extra, off, np.concatenate(cigs).astype(np.uint32) if len(cigs) and off[-1] else np.zeros(0, np.uint32)


def same(u, v):
    return u.shape == v.shape and np.array_equal(u.view(np.uint8) if u.dtype.fields else u, v.view(np.uint8) if v.dtype.fields else v)


def main():
    tmp = tempfile.mkdtemp(prefix="inv_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(OUT, exist_ok=True)
        scenes = S.named_scenes() + [S.fuzz_scene()]
        total = 0
        for sc in scenes:
            p = S.pack(sc)
            model = S.model_scene(p)          # raises align_model.Undefined where a pair falls into unspecified behaviour: none may
            ref = ref_scene(lib, p, model[0], model[5])
            for nm, u, v in zip(("made", "r_inv", "extra", "cigar_off", "cigar"), model, ref):
                if not same(u, v):
                    bad = np.nonzero(u != v)[0][:4] if u.shape == v.shape else (u.shape, v.shape)
                    raise AssertionError((sc["name"], nm, bad, u[bad] if u.shape == v.shape else None, v[bad] if u.shape == v.shape else None))
            made, r_inv, extra, off, cig = ref
            path = os.path.join(OUT, sc["name"] + ".npz")
            np.savez_compressed(path, made=made, r_inv=r_inv, extra=extra, cigar_off=off, cigar=cig, ll=model[5], prob=model[6], **p)
            assert os.path.getsize(path) < 64 << 10
            total += os.path.getsize(path)
            print(f"{sc['name']}.npz: {len(p['seq_off']) - 1} reads, {len(made)} slots, {len(model[5])} candidates, codes "
                  f"{np.bincount(made, minlength=5).tolist()}, {off[-1]} CIGAR words, {os.path.getsize(path)} bytes")
        print(f"{len(scenes)} files, {total} bytes")
        # ll_ends against the compiled ksw_ll_i16: every stretch of every scene ...
        n_pad = 0
        for q, t, gapo, gape, a_, b_, got in M.ll_seen:
            want = ref_ll(lib, q, t, a_, b_, gapo, gape)
            assert got == want, (len(q), len(t), got, want)
            n_pad += want[1] >= len(q)
        print(f"ll_ends equals ksw_ll_i16 (score, qe, te) on {len(M.ll_seen)} stretches of the scenes; qe >= ql in {n_pad}")
        # ... and a fuzz of its own: alphabets of 1 to 5 letters, half of the pairs with a copied stretch, two scoring sets
        rng = np.random.default_rng(11)
        for top, count in ((70, 4000), (600, 300), (2000, 30)):
            n_bad_unpadded = n_pad = 0
            for k in range(count):
                letters = int(rng.integers(1, 6))
                ql, tl = int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))
                q, t = rng.integers(0, letters, ql).astype(np.uint8), rng.integers(0, letters, tl).astype(np.uint8)
                if k & 1:
                    ln = int(rng.integers(1, min(ql, tl) + 1))
                    i, j = int(rng.integers(0, ql - ln + 1)), int(rng.integers(0, tl - ln + 1))
                    t[j:j + ln] = q[i:i + ln]
                for (a_, b_, q_, e_) in ((2, 4, 4, 2), (1, 9, 16, 2)):
                    want = ref_ll(lib, q, t, a_, b_, q_, e_)
                    mat = A.simple_mat(a_, b_)
                    got = M.ll_ends(q, t, mat, q_, e_)
                    assert got == want, (ql, tl, letters, got, want)
                    n_pad += want[1] >= ql
                    n_bad_unpadded += M.ll_ends(q, t, mat, q_, e_, pad=False) != want
            print(f"ll_ends equals ksw_ll_i16 on {count} pairs up to {top} bases x 2 scoring sets: padded model wrong 0, unpadded model wrong "
                  f"{n_bad_unpadded}, qe >= ql in {n_pad}")
        missing = [k for k in COVER if not M.cover[k]]
        print("coverage:", dict(sorted(M.cover.items())))
        assert not missing, missing
        # the reference's one-thread ksw_ll_i16 (query profile included) on stretches of 100, 1000 and 10000 bases
        for n in (100, 1000, 10000):
            q = rng.integers(0, 4, n).astype(np.uint8)
            t = np.where(rng.random(n) < 0.1, rng.integers(0, 4, n), q).astype(np.uint8)
            reps = max(1, 20000000 // (n * n))
            best = 1e30
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(reps):
                    ref_ll(lib, q, t, 2, 4, 4, 2)
                best = min(best, (time.perf_counter() - t0) / reps)
            print(f"reference ksw_ll_i16, one thread, {n} x {n}: {best * 1e6:.1f} us, {n * n / best / 1e9:.2f} G cells / s")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
