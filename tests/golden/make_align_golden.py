#!/usr/bin/env python3
"""Generates tests/golden/align/*.npz: what the UNMODIFIED reference's mm_align1 makes of the scenes of tests/align_shapes.py (build
container only: it needs the reference's sources and a C compiler).

A driver of this script's own #includes align.c where it lies, to reach the static mm_align1, and is compiled beside index.c
(mm_idx_getseq; the driver fills the sequence half of an mm_idx_t as mm_idx_str does), hit.c, the ksw2_* files, kalloc.c and what those need, into a shared object in a temporary directory
outside the repository, which is removed at the end; nothing of the reference is copied.  One file per scene with the flat inputs of
align_shapes.pack() and every output word: a_out, regs_out, regs2, extra, cigar_off, cigar.

Asserts on the way: the model (tests/align_model.py) equals the reference on every region; the local-score model equals ksw_ll_i16
on every stretch mm_test_zdrop tested and on a fuzz of its own up to max_gap long; every branch in COVER occurred, counted by the
model.  Prints the reference's one-thread rate (regions / s, aligned bases / s) for DESIGN.md."""
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
import align_shapes as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(HERE, "align")

# every branch the tests name, as align_model counts it
COVER = ("cnt_0", "cnt_1", "cnt_2", "cnt_3", "strand_0", "strand_1", "fix_bad_ends_start", "fix_bad_ends_end", "filter_n_le_1", "filter_runs_1",
         "filter_runs_2", "neighbour_left", "neighbour_right", "neighbour_left_binds_q", "neighbour_left_binds_r", "neighbour_right_binds_q",
         "neighbour_right_binds_r", "no_left_ext_qs", "no_left_ext_rs", "right_ext_to_read_end", "right_ext_to_target_end", "left_ext", "right_ext",
         "seed_self", "long_join_inner", "long_join_last", "skip_tandem", "tandem_last", "skip_ignore", "skip_short", "split_inv_in",
         "zdrop_code_0", "zdrop_code_1", "zdrop_code_2", "zdrop_inv_test", "drop_split_done", "drop_split_inv", "drop_no_split",
         "fix_cigar_leading_I", "fix_cigar_leading_D", "fix_cigar_shift", "fix_cigar_shift_whole_M", "stitch_equal_ops", "n_ambi")

DRIVER = r"""
#include "%(ref)s/align.c"
extern unsigned char seq_nt4_table[256];
/* what the files beside this one expect of the program they are part of (map.c, main.c, the accelerator's driver): not used on this path */
struct mm_idx_bucket_s *g_B = 0;
int32_t g_b = 0;
double send_task1[100], send_task2[100], process_result[100];
void fpga_load_index(void *addr, int size, int type) { (void)addr; (void)size; (void)type; }
/* the sequence half of mm_idx_str (index.c:751-769): lengths, offsets and the 4-bit packed bases mm_idx_getseq reads.  mm_align1 looks at
 * nothing else of an index; the minimizer half of mm_idx_str belongs to the accelerator's program in this reference and does not run without it. */
void *drv_index(int w, int k, int is_hpc, int n, const char **seqs)
{
	mm_idx_t *mi = (mm_idx_t*)calloc(1, sizeof(mm_idx_t));
	uint64_t sum_len = 0;
	int i;
	for (i = 0; i < n; ++i) sum_len += strlen(seqs[i]);
	mi->w = w, mi->k = k, mi->b = 10, mi->flag = (is_hpc? MM_I_HPC : 0) | MM_I_NO_NAME, mi->n_seq = n;
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
int drv_align1(void *mi, const int *o, int qlen, const char *seq, int n_a, mm128_t *a, mm_reg1_t *r, mm_reg1_t *r2, int32_t *extra,
               uint32_t *cigar, int cap)
{
	mm_mapopt_t opt;
	uint8_t *qseq0[2];
	ksw_extz_t ez;
	int i, n = 0;
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
	r->p = 0;
	memset(r2, 0, sizeof(*r2));
	mm_align1(0, &opt, (const mm_idx_t*)mi, qlen, qseq0, r, r2, n_a, a, &ez, 0);
	memset(extra, 0, 5 * sizeof(int32_t));
	if (r->p) {
		extra[0] = 1, extra[1] = r->p->dp_score, extra[2] = r->p->dp_max, extra[3] = r->p->n_ambi, extra[4] = n = r->p->n_cigar;
		if (n <= cap) memcpy(cigar, r->p->cigar, n * 4);
		free(r->p); r->p = 0;
	}
	kfree(0, ez.cigar);
	free(qseq0[0]);
	return n;
}
int drv_ll(int qlen, const uint8_t *q, int tlen, const uint8_t *t, int a, int b, int gapo, int gape)
{
	int8_t mat[25];
	int qe, te, s;
	void *qp;
	ksw_gen_simple_mat(5, mat, a, b);
	qp = ksw_ll_qinit(0, 2, qlen, q, 5, mat);
	s = ksw_ll_i16(qp, tlen, t, gapo, gape, &qe, &te);
	kfree(0, qp);
	return s;
}
"""
SOURCES = ("index.c", "hit.c", "ksw2_extd2_sse.c", "ksw2_extz2_sse.c", "ksw2_exts2_sse.c", "ksw2_ll_sse.c", "kalloc.c", "sketch.c", "misc.c", "bseq.c",
           "kthread.c", "options.c")


def build(tmp):
    drv = os.path.join(tmp, "align_driver.c")
    with open(drv, "w") as f:
        f.write(DRIVER % {"ref": REF})
    so = os.path.join(tmp, "libalign_ref.so")
    subprocess.check_call(["gcc", "-O2", "-msse4.1", "-fPIC", "-shared", "-w", "-DHAVE_KALLOC", "-I" + REF, "-o", so, drv]
                          + [os.path.join(REF, s) for s in SOURCES] + ["-lm", "-lz", "-lpthread"])
    lib = C.CDLL(so)
    lib.drv_index.restype = C.c_void_p
    lib.drv_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    lib.drv_index_free.argtypes = [C.c_void_p]
    lib.drv_align1.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
    lib.drv_ll.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    return lib


def ref_scene(lib, p):
    """The reference over a packed scene: the same tuple as align_shapes.model_scene."""
    n_t = len(p["tseq_off"]) - 1
    tseqs = [bytes(p["tseq"][p["tseq_off"][i]:p["tseq_off"][i + 1]]) for i in range(n_t)]
    opt = np.ascontiguousarray(p["opt"], np.int32)
    mi = lib.drv_index(10, int(opt[16]), int(opt[17]), n_t, (C.c_char_p * n_t)(*tseqs))
    assert mi
    a, regs = p["a"].copy(), p["regs"].copy()
    regs2, extra = np.zeros(len(regs), S.REG_DTYPE), np.zeros(len(regs), S.EXTRA_DTYPE)
    cigs = []
    for rd in range(len(p["seq_off"]) - 1):
        seq = bytes(p["seq"][p["seq_off"][rd]:p["seq_off"][rd + 1]])
        a0, a1 = int(p["a_off"][rd]), int(p["a_off"][rd + 1])
        ar = np.ascontiguousarray(a[a0:a1])
        for i in range(int(p["regs_off"][rd]), int(p["regs_off"][rd + 1])):
            cig = np.zeros(2 * len(seq) + 16, np.uint32)
            n = lib.drv_align1(mi, opt.ctypes.data, len(seq), seq, a1 - a0, ar.ctypes.data, regs[i:i + 1].ctypes.data, regs2[i:i + 1].ctypes.data,
                               extra[i:i + 1].ctypes.data, cig.ctypes.data, len(cig))
            assert n <= len(cig)
            cigs.append(cig[:n])
        a[a0:a1] = ar
    lib.drv_index_free(mi)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.int64)
    return a, regs, regs2, extra, off, np.concatenate(cigs).astype(np.uint32) if len(cigs) and off[-1] else np.zeros(0, np.uint32)


def same(x, y):
    return all(np.array_equal(u.view(np.uint8) if u.dtype.fields else u, v.view(np.uint8) if v.dtype.fields else v) for u, v in zip(x, y))


def main():
    tmp = tempfile.mkdtemp(prefix="align_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(OUT, exist_ok=True)
        scenes = S.named_scenes() + [S.fuzz_scene()]
        n_regs = n_bases = 0
        packed = []
        for sc in scenes:
            p = S.pack(sc)
            ref = ref_scene(lib, p)
            model = S.model_scene(p)
            for nm, u, v in zip(("a", "regs", "regs2", "extra", "cigar_off", "cigar"), model, ref):
                if not same([u], [v]):
                    bad = np.nonzero(u != v)[0][:4] if u.shape == v.shape else (u.shape, v.shape)
                    raise AssertionError((sc["name"], nm, bad, u[bad] if u.shape == v.shape else None, v[bad] if u.shape == v.shape else None))
            a, regs, regs2, extra, off, cig = ref
            path = os.path.join(OUT, sc["name"] + ".npz")
            np.savez_compressed(path, a_out=a, regs_out=regs, regs2=regs2, extra=extra, cigar_off=off, cigar=cig, **p)
            assert os.path.getsize(path) < 1 << 20
            n_regs += len(regs); n_bases += int((regs["qe"] - regs["qs"])[extra["has_extra"] == 1].sum())
            packed.append(p)
            print(f"{sc['name']}.npz: {len(p['seq_off']) - 1} reads, {len(regs)} regions, {int(extra['has_extra'].sum())} aligned, "
                  f"{int((regs2['cnt'] > 0).sum())} split, {off[-1]} CIGAR words, {os.path.getsize(path)} bytes")
        # the local-score model against ksw_ll_i16: every stretch mm_test_zdrop tested, and a fuzz up to max_gap long
        rng = np.random.default_rng(5)
        tested = list(A.ll_seen)
        for ln in (1, 2, 7, 8, 9, 63, 64, 65, 300, 1200, S.OPT["max_gap"] - 1):
            for k in range(2 if ln > 1000 else 6):
                q = rng.integers(0, 5 if k % 2 else 4, ln).astype(np.uint8)
                t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 20))).astype(np.uint8), q[: ln - ln // 3], rng.integers(0, 4, ln // 2).astype(np.uint8)])
                t = np.where(rng.random(len(t)) < 0.05, rng.integers(0, 4, len(t)), t).astype(np.uint8)[: S.OPT["max_gap"] - 1]
                tested.append((q, t, None))
        for (a_, b_, q_, e_) in ((2, 4, 4, 2), (1, 9, 16, 2)):
            for q, t, _ in tested:
                want = lib.drv_ll(len(q), np.ascontiguousarray(q).ctypes.data, len(t), np.ascontiguousarray(t).ctypes.data, a_, b_, q_, e_)
                got = A.ll_score(q, t, A.simple_mat(a_, b_), q_, e_)
                assert got == want, (len(q), len(t), got, want)
        print(f"ll_score equals ksw_ll_i16 on {len(tested)} stretches x 2 scoring sets ({len(A.ll_seen)} from mm_test_zdrop)")
        missing = [k for k in COVER if not A.cover[k]]
        print("coverage:", dict(sorted(A.cover.items())))
        assert not missing, missing
        best = 1e30
        for _ in range(5):
            t0 = time.perf_counter()
            for p in packed:
                ref_scene(lib, p)
            best = min(best, time.perf_counter() - t0)
        print(f"reference, one thread, all scenes: {n_regs} regions, {n_bases} aligned read bases, {best * 1e3:.2f} ms: {n_regs / best:.0f} regions / s, "
              f"{n_bases / best / 1e6:.2f} M aligned bases / s (index builds and the ctypes calls included)")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
