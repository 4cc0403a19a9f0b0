#!/usr/bin/env python3
"""Generates tests/golden/skeleton/*.npz: what the UNMODIFIED reference's mm_align_skeleton makes of the scenes of
tests/skeleton_shapes.py (build container only: it needs the reference's sources and a C compiler).

A driver of this script's own #includes align.c where it lies and is compiled beside the files it needs into a shared object in a
temporary directory outside the repository, which is removed at the end; nothing of the reference is copied.  The driver calls
mm_align_skeleton once per read, with malloc'd regions and km = 0, and records the final regions (p zeroed), what r->p held, the
CIGARs and a[], and through a tap on the loop's call of mm_filter_regs the list as the loop left it (placed_out).  One file per scene
with the flat inputs of skeleton_shapes.pack(), the reference's outputs (placed_off_out, placed_out, regs_off_out, regs_out, extra_out,
cigar_off_out, cigar_out, a_out) and, from the batched composition over the CPU models, what every stage call returned (t<k>_*: the
align1 rounds and the inversion call), for the GPU tier to hold the device's intermediate results against.

Asserts on the way: mm_squeeze_a leaves every scene's anchors where they are (in the driver, on a copy); the batched composition
(tests/skeleton_model.py over align_model and inv_model) equals the reference in every word on every read; no scene is refused
(unspecified behaviour, a region sorted without an alignment); every class of skeleton_model.COVER occurred."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_shapes as S  # noqa: E402
import skeleton_model as K  # noqa: E402
import skeleton_shapes as SS  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(HERE, "skeleton")
TRACED = dict(align1=("regs_off", "regs_in", "a", "regs", "regs2", "extra", "cigar_off", "cigar"),
              align1_inv=("regs_off", "regs_in", "made", "r_inv", "extra", "cigar_off", "cigar"))

DRIVER = r"""
/* mm_align_skeleton's call of mm_filter_regs goes through a tap of the driver's, which copies the list as the loop left it (the sort
 * hides where a record stood) and then calls the reference's mm_filter_regs */
#define mm_filter_regs drv_tap_filter_regs
#include "%(ref)s/align.c"
#undef mm_filter_regs
void mm_filter_regs(void *km, const mm_mapopt_t *opt, int qlen, int *n_regs, mm_reg1_t *regs);
static mm_reg1_t *tap_regs;
static int tap_n, tap_cap;
void drv_tap_filter_regs(void *km, const mm_mapopt_t *opt, int qlen, int *n_regs, mm_reg1_t *regs)
{
	int i;
	tap_n = *n_regs;
	for (i = 0; i < tap_n && i < tap_cap; ++i) {
		tap_regs[i] = regs[i];
		memset(&tap_regs[i].p, 0, sizeof(tap_regs[i].p));
	}
	mm_filter_regs(km, opt, qlen, n_regs, regs);
}
extern unsigned char seq_nt4_table[256];
/* what the files beside this one expect of the program they are part of (map.c, main.c, the accelerator's driver): not used on this path */
struct mm_idx_bucket_s *g_B = 0;
int32_t g_b = 0;
double send_task1[100], send_task2[100], process_result[100];
void fpga_load_index(void *addr, int size, int type) { (void)addr; (void)size; (void)type; }
/* the sequence half of mm_idx_str (index.c:751-769): lengths, offsets and the 4-bit packed bases mm_idx_getseq reads */
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
/* mm_align_skeleton on one read.  Returns the number of final regions; -2 where mm_squeeze_a would move an anchor or change a region,
 * -3 / -4 where the caller's room for regions / CIGAR words is too small. */
int drv_skeleton(void *mi, const int *o, int qlen, const char *seq, int n_regs, const mm_reg1_t *regs_in, int n_a, mm128_t *a, int cap_regs,
                 mm_reg1_t *regs_out, int32_t *extra, int64_t cap_cigar, uint32_t *cigar, int64_t *cigar_off, mm_reg1_t *placed, int *n_placed)
{
	mm_mapopt_t opt;
	mm_reg1_t *regs, *chk;
	mm128_t *a2;
	int i, same;
	int64_t n_cigar = 0;
	mm_mapopt_init(&opt);           /* max_clip_ratio stays at its default, as the reference's driver leaves it */
	opt.a = o[0], opt.b = o[1], opt.q = o[2], opt.e = o[3], opt.q2 = o[4], opt.e2 = o[5], opt.bw = o[6], opt.zdrop = o[7], opt.zdrop_inv = o[8];
	opt.end_bonus = o[9], opt.min_cnt = o[10], opt.min_chain_score = o[11], opt.min_dp_max = o[12], opt.min_ksw_len = o[13], opt.max_gap = o[14];
	opt.flag = o[15];
	chk = (mm_reg1_t*)malloc((n_regs + 1) * sizeof(mm_reg1_t));
	a2 = (mm128_t*)malloc((n_a + 1) * sizeof(mm128_t));
	memcpy(chk, regs_in, n_regs * sizeof(mm_reg1_t));
	memcpy(a2, a, n_a * sizeof(mm128_t));
	same = (n_regs == 0 || mm_squeeze_a(0, n_regs, chk, a2) == n_a) && memcmp(a2, a, n_a * sizeof(mm128_t)) == 0
	       && memcmp(chk, regs_in, n_regs * sizeof(mm_reg1_t)) == 0;
	free(chk); free(a2);
	if (!same) return -2;
	regs = (mm_reg1_t*)malloc((n_regs + 1) * sizeof(mm_reg1_t));
	memcpy(regs, regs_in, n_regs * sizeof(mm_reg1_t));
	tap_regs = placed, tap_cap = cap_regs, tap_n = -1;
	regs = mm_align_skeleton(0, &opt, (const mm_idx_t*)mi, qlen, seq, &n_regs, regs, a);
	*n_placed = tap_n;
	cigar_off[0] = 0;
	for (i = 0; i < n_regs; ++i) {
		mm_extra_t *p = regs[i].p;
		if (i < cap_regs) {
			regs_out[i] = regs[i];
			memset(&regs_out[i].p, 0, sizeof(regs_out[i].p));
			memset(&extra[5 * i], 0, 5 * sizeof(int32_t));
			if (p) {
				extra[5 * i] = 1, extra[5 * i + 1] = p->dp_score, extra[5 * i + 2] = p->dp_max, extra[5 * i + 3] = p->n_ambi, extra[5 * i + 4] = p->n_cigar;
				if (n_cigar + p->n_cigar <= cap_cigar) memcpy(cigar + n_cigar, p->cigar, p->n_cigar * 4);
			}
			n_cigar += p? p->n_cigar : 0;
			cigar_off[i + 1] = n_cigar;
		}
		free(p);
	}
	free(regs);
	return n_regs > cap_regs || tap_n > cap_regs? -3 : n_cigar > cap_cigar? -4 : n_regs;
}
"""
SOURCES = ("index.c", "hit.c", "ksw2_extd2_sse.c", "ksw2_extz2_sse.c", "ksw2_exts2_sse.c", "ksw2_ll_sse.c", "kalloc.c", "sketch.c", "misc.c", "bseq.c",
           "kthread.c", "options.c")


def build(tmp):
    drv = os.path.join(tmp, "skeleton_driver.c")
    with open(drv, "w") as f:
        f.write(DRIVER % {"ref": REF})
    so = os.path.join(tmp, "libskeleton_ref.so")
    subprocess.check_call(["gcc", "-O2", "-msse4.1", "-fPIC", "-shared", "-w", "-DHAVE_KALLOC", "-I" + REF, "-o", so, drv]
                          + [os.path.join(REF, s) for s in SOURCES] + ["-lm", "-lz", "-lpthread"])
    lib = C.CDLL(so)
    lib.drv_index.restype = C.c_void_p
    lib.drv_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    lib.drv_index_free.argtypes = [C.c_void_p]
    lib.drv_skeleton.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def ref_scene(lib, p):
    """The reference's loop over a packed scene, read by read: the dict skeleton_model.run returns."""
    n_t = len(p["tseq_off"]) - 1
    tseqs = [bytes(p["tseq"][p["tseq_off"][i]:p["tseq_off"][i + 1]]) for i in range(n_t)]
    opt = np.ascontiguousarray(p["opt"], np.int32)
    mi = lib.drv_index(10, int(opt[16]), int(opt[17]), n_t, (C.c_char_p * n_t)(*tseqs))
    assert mi
    a = p["a"].copy()
    regs, extra, cigs, placed = [], [], [], []
    for rd in range(len(p["seq_off"]) - 1):
        seq = bytes(p["seq"][p["seq_off"][rd]:p["seq_off"][rd + 1]])
        a0, a1, r0, r1 = (int(p[k][i]) for k in ("a_off", "regs_off") for i in (rd, rd + 1))
        ar, rin = np.ascontiguousarray(a[a0:a1]), np.ascontiguousarray(p["regs"][r0:r1])
        cap = 4 * (r1 - r0) + 8                        # every region can split and every pair make an inversion, more than once in a scene of this size
        rout, ex, cig, off = np.zeros(cap, S.REG_DTYPE), np.zeros(cap, S.EXTRA_DTYPE), np.zeros(cap * (2 * len(seq) + 16), np.uint32), np.zeros(cap + 1, np.int64)
        pl, n_pl = np.zeros(cap, S.REG_DTYPE), C.c_int(-1)
        n = lib.drv_skeleton(mi, opt.ctypes.data, len(seq), seq, r1 - r0, rin.ctypes.data, a1 - a0, ar.ctypes.data, cap, rout.ctypes.data, ex.ctypes.data,
                             len(cig), cig.ctypes.data, off.ctypes.data, pl.ctypes.data, C.byref(n_pl))
        assert n != -2, f"read {rd}: mm_squeeze_a moves the scene's anchors"
        assert n >= 0 and n_pl.value >= n, (rd, n, n_pl.value)
        placed.append(pl[:n_pl.value])
        a[a0:a1] = ar
        regs.append(rout[:n]); extra.append(ex[:n])
        cigs += [cig[int(off[i]):int(off[i + 1])] for i in range(n)]
    lib.drv_index_free(mi)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if sum(len(x) for x in parts) else np.zeros(0, dt)
    return dict(placed_off=K.offsets([len(r) for r in placed]), placed=cat(placed, S.REG_DTYPE), regs_off=K.offsets([len(r) for r in regs]), regs=cat(regs, S.REG_DTYPE), extra=cat(extra, S.EXTRA_DTYPE),
                cigar_off=K.offsets([len(c) for c in cigs]), cigar=cat(cigs, np.uint32), a=a)


def main():
    tmp = tempfile.mkdtemp(prefix="skeleton_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(OUT, exist_ok=True)
        K.cover.clear()
        total = 0
        for sc in SS.all_scenes():
            p = SS.pack(sc)
            trace = []
            model = SS.check(p, trace)                 # raises where the scene is refused: none may be
            ref = ref_scene(lib, p)
            for k in K.OUTPUTS:
                u, v = model[k], ref[k]
                if u.shape != v.shape or not np.array_equal(K.words(u), K.words(v)):
                    bad = np.nonzero(u != v)[0][:4] if u.shape == v.shape else (u.shape, v.shape)
                    raise AssertionError((sc["name"], k, bad, u[bad] if u.shape == v.shape else None, v[bad] if u.shape == v.shape else None))
            traced = {"t%d_%s" % (i, k): t[k] for i, t in enumerate(trace) for k in TRACED[t["stage"]]}
            path = os.path.join(OUT, sc["name"] + ".npz")
            np.savez_compressed(path, n_calls=np.int64(len(trace)), **{k + "_out": ref[k] for k in K.OUTPUTS}, **traced, **p)
            assert os.path.getsize(path) < 1 << 20
            total += os.path.getsize(path)
            made = trace[-1]["made"]
            print(f"{sc['name']}.npz: {len(p['seq_off']) - 1} reads, {len(p['regs'])} regions in, {len(trace) - 1} rounds, "
                  f"{sum(int((t['regs2']['cnt'] > 0).sum()) for t in trace[:-1])} split off, inversion codes {np.bincount(made, minlength=5).tolist()}, "
                  f"{len(ref['regs'])} regions out, {ref['cigar_off'][-1]} CIGAR words, {os.path.getsize(path)} bytes")
        print(f"{total} bytes")
        print("coverage:", dict(sorted(K.cover.items())))
        missing = [k for k in K.COVER if not K.cover[k]]
        assert not missing, missing
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
