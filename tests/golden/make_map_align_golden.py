#!/usr/bin/env python3
"""Generates tests/golden/map_align/*.npz: what the UNMODIFIED reference makes of the scenes of tests/map_align_shapes.py between
mm_chain_dp_bottom and a read's output in a run with MM_F_CIGAR (for a machine with the reference's sources and a C compiler).

A driver of this script's own #includes map.c where it lies, as oracle/mt_dump.c does (chain_post and align_regs are static there),
and is compiled beside the files it needs into a shared object in a temporary directory outside the repository, which is removed at
the end; nothing of the reference is copied.  align.c is compiled with mm_squeeze_a renamed to a tap of the driver's, which calls the
reference's mm_squeeze_a and then copies the regions and anchors as the skeleton's squeeze left them.  Per read, on the u[] / a[] of
mm_chain_dp_bottom that tests/e2e_model.py holds to the reference, with that read's hash, mini_pos and rep_len, the driver calls in
the order of map.c:862-877: mm_gen_regs, chain_post, mm_est_err, align_regs, mm_set_mapq.  One file per scene with the reference's
outputs: the final regions (p zeroed), what r->p held, dp_max2, the CIGARs, a[] with its marks, the tap (sq_*), rep_len, n_anchors
and a digest of the scene's bases, so that a scene that drifts from its golden is noticed.

Asserts on the way: the composition of tests/map_align_model.py equals the reference in every word on every read (div byte-equal:
both run the host's logf); no scene is refused (skeleton_model / align_model raise where the reference's behaviour is unspecified);
every class of map_align_model.COVER occurred."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
import align_shapes as AS  # noqa: E402
import apost_shapes as PS  # noqa: E402
import e2e_model as em  # noqa: E402
import map_align_model as M  # noqa: E402
import map_align_shapes as S  # noqa: E402
import skeleton_model as K  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(HERE, "map_align")

DRIVER = r"""
#include "%(ref)s/map.c"
extern unsigned char seq_nt4_table[256];
/* what the files beside this one expect of the program they are part of (main.c): not used on this path */
double send_task1[100], send_task2[100], process_result[100], soft_chaindp_time[100];
int max_task = 0, soft_chaindp_num = 0;
/* align.c is compiled with -Dmm_squeeze_a=drv_tap_squeeze: mm_align_skeleton's squeeze comes here */
static mm_reg1_t *tap_regs;
static mm128_t *tap_a;
static int tap_n, tap_na, tap_cap, tap_acap;
int drv_tap_squeeze(void *km, int n_regs, mm_reg1_t *regs, mm128_t *a)
{
	int i, n_a = mm_squeeze_a(km, n_regs, regs, a);
	tap_n = n_regs, tap_na = n_a;
	for (i = 0; i < n_regs && i < tap_cap; ++i) {
		tap_regs[i] = regs[i];
		memset(&tap_regs[i].p, 0, sizeof(tap_regs[i].p));
	}
	if (n_a <= tap_acap) memcpy(tap_a, a, (size_t)n_a * sizeof(mm128_t));
	return n_a;
}
/* the sequence half of mm_idx_str (index.c:751-769): lengths, offsets and the 4-bit packed bases mm_idx_getseq reads */
void *drv_index(int w, int k, int is_hpc, int n, const char **seqs, const int *lens)
{
	mm_idx_t *mi = (mm_idx_t*)calloc(1, sizeof(mm_idx_t));
	uint64_t sum_len = 0;
	int i;
	for (i = 0; i < n; ++i) sum_len += lens[i];
	mi->w = w, mi->k = k, mi->b = 10, mi->flag = (is_hpc? MM_I_HPC : 0) | MM_I_NO_NAME, mi->n_seq = n;
	mi->seq = (mm_idx_seq_t*)calloc(n + 1, sizeof(mm_idx_seq_t));
	mi->S = (uint32_t*)calloc((sum_len + 7) / 8 + 1, 4);
	for (i = 0, sum_len = 0; i < n; ++i) {
		uint32_t j;
		mi->seq[i].offset = sum_len, mi->seq[i].len = lens[i];
		for (j = 0; j < mi->seq[i].len; ++j) mm_seq4_set(mi->S, sum_len + j, seq_nt4_table[(uint8_t)seqs[i][j]]);
		sum_len += mi->seq[i].len;
	}
	return mi;
}
void drv_index_free(void *mi_) { mm_idx_t *mi = (mm_idx_t*)mi_; free(mi->seq); free(mi->S); free(mi); }
/* One read from mm_chain_dp_bottom's u[] / a[] to its output (map.c:862-877, n_segs == 1).  o: the row of align_model.OPT_FIELDS, po:
 * the row of apost_shapes.OPT_FIELDS.  Returns the number of final regions; -3 / -4 where the caller's room for regions / CIGAR words
 * is too small. */
int drv_read(void *mi_, const int *o, const double *po, int qlen, const char *seq, uint32_t hash, int n_u, const uint64_t *u_in, int n_a, mm128_t *a,
             int n_minipos, const uint64_t *mini_pos, int rep_len, int cap_regs, mm_reg1_t *regs_out, int32_t *extra, int32_t *dp_max2, int64_t cap_cigar,
             uint32_t *cigar, int64_t *cigar_off, mm_reg1_t *sq_regs, mm128_t *sq_a, int *n_sq, int *n_sq_a, mm_reg1_t *pre_regs, int *n_pre)
{
	const mm_idx_t *mi = (const mm_idx_t*)mi_;
	mm_mapopt_t opt;
	mm_reg1_t *regs;
	uint64_t *u;
	int i, n_regs = n_u, is_sr;
	int64_t n_cigar = 0;
	mm_mapopt_init(&opt);           /* max_clip_ratio stays at its default, as the reference's driver leaves it */
	opt.a = o[0], opt.b = o[1], opt.q = o[2], opt.e = o[3], opt.q2 = o[4], opt.e2 = o[5], opt.bw = o[6], opt.zdrop = o[7], opt.zdrop_inv = o[8];
	opt.end_bonus = o[9], opt.min_cnt = o[10], opt.min_chain_score = o[11], opt.min_dp_max = o[12], opt.min_ksw_len = o[13], opt.max_gap = o[14];
	opt.flag = o[15] | (int)po[0];
	opt.mask_level = (float)po[1], opt.pri_ratio = (float)po[2], opt.best_n = (int)po[3];
	opt.max_join_long = (int)po[6], opt.max_join_short = (int)po[7], opt.min_join_flank_sc = (int)po[8];
	is_sr = (int)po[12];
	u = (uint64_t*)malloc((n_u + 1) * 8);
	memcpy(u, u_in, n_u * 8);
	regs = mm_gen_regs(NULL, hash, qlen, n_u, u, a);
	free(u);
	chain_post(&opt, opt.max_gap_ref, mi, NULL, qlen, 1, &qlen, &n_regs, regs, a);
	if (!is_sr) mm_est_err(mi, qlen, n_regs, regs, a, n_minipos, mini_pos);
	*n_pre = n_regs;
	for (i = 0; i < n_regs && i < cap_regs; ++i) pre_regs[i] = regs[i];
	tap_regs = sq_regs, tap_a = sq_a, tap_cap = cap_regs, tap_acap = n_a, tap_n = tap_na = -1;
	regs = align_regs(&opt, mi, NULL, qlen, seq, &n_regs, regs, a);
	mm_set_mapq(NULL, n_regs, regs, opt.min_chain_score, opt.a, rep_len, is_sr);
	*n_sq = tap_n, *n_sq_a = tap_na;
	cigar_off[0] = 0;
	for (i = 0; i < n_regs; ++i) {
		mm_extra_t *p = regs[i].p;
		if (i < cap_regs) {
			regs_out[i] = regs[i];
			memset(&regs_out[i].p, 0, sizeof(regs_out[i].p));
			memset(&extra[5 * i], 0, 5 * sizeof(int32_t));
			dp_max2[i] = 0;
			if (p) {
				extra[5 * i] = 1, extra[5 * i + 1] = p->dp_score, extra[5 * i + 2] = p->dp_max, extra[5 * i + 3] = p->n_ambi, extra[5 * i + 4] = p->n_cigar;
				dp_max2[i] = p->dp_max2;
				if (n_cigar + p->n_cigar <= cap_cigar) memcpy(cigar + n_cigar, p->cigar, p->n_cigar * 4);
			}
			n_cigar += p? p->n_cigar : 0;
			cigar_off[i + 1] = n_cigar;
		}
		free(p);
	}
	free(regs);
	return n_regs > cap_regs || *n_pre > cap_regs || tap_n > cap_regs? -3 : n_cigar > cap_cigar? -4 : n_regs;
}
"""
# what map.c needs beside it (oracle/Makefile's REF_FRONT without align.c, which is compiled on its own for the tap)
SOURCES = ("sketch.c", "index.c", "bseq.c", "misc.c", "kalloc.c", "options.c", "kthread.c", "sdust.c", "chain.c", "fpga_chaindp.c", "hit.c", "esterr.c", "pe.c",
           "format.c", "ksw2_ll_sse.c", "ksw2_extz2_sse.c", "ksw2_extd2_sse.c", "ksw2_exts2_sse.c")
FLAGS = ["-O2", "-std=gnu99", "-msse4.1", "-fPIC", "-w", "-DHAVE_KALLOC", "-I" + REF]


def build(tmp):
    drv = os.path.join(tmp, "map_align_driver.c")
    with open(drv, "w") as f:
        f.write(DRIVER % {"ref": REF})
    tapped = os.path.join(tmp, "align_tapped.o")
    subprocess.check_call(["gcc"] + FLAGS + ["-Dmm_squeeze_a=drv_tap_squeeze", "-c", "-o", tapped, os.path.join(REF, "align.c")])
    so = os.path.join(tmp, "libmap_align_ref.so")
    # the accelerator driver's functions that map.c and index.c name are never called on this path: they stay unresolved, lazily bound
    subprocess.check_call(["gcc"] + FLAGS + ["-shared", "-o", so, drv, tapped] + [os.path.join(REF, s) for s in SOURCES]
                          + ["-Wl,-z,lazy", "-lm", "-lz", "-lpthread"])
    lib = C.CDLL(so, mode=os.RTLD_LAZY)
    lib.drv_index.restype = C.c_void_p
    lib.drv_index.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_void_p]
    lib.drv_index_free.argtypes = [C.c_void_p]
    lib.drv_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                             C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def digest(sc):
    return np.frombuffer(hashlib.sha256(bytes(sc.seq) + bytes(sc.tseq) + sc.seq_off.tobytes() + sc.tseq_off.tobytes() + sc.hash_.tobytes() + sc.bid.tobytes()).digest(), np.uint8)


def ref_scene(lib, sc, m):
    """The reference over a scene, read by read, from the model's u[] / b[]: the dict map_align_model.run returns."""
    row, prow = np.ascontiguousarray(M.align_row(sc.aopt), np.int32), np.ascontiguousarray(PS.opt_row(sc.opt.asdict()), np.float64)
    n_t = len(sc.targets)
    lens = np.array([len(t) for t in sc.targets], np.int32)
    mi = lib.drv_index(sc.w, int(row[16]), int(row[17]), n_t, (C.c_char_p * n_t)(*sc.targets), lens.ctypes.data)
    assert mi
    regs, extra, dp2, cigs, a_out, sq_regs, sq_a, pre = [], [], [], [], [], [], [], []
    for rd, seq in enumerate(sc.reads):
        u = np.ascontiguousarray(m.u[m.chains_off[rd]:m.chains_off[rd + 1]])
        a = np.ascontiguousarray(m.b[m.b_off[rd]:m.b_off[rd + 1]]).copy()
        mp = np.ascontiguousarray(m.mini_pos[m.mp_off[rd]:m.mp_off[rd + 1]])
        cap = 4 * len(u) + 8
        rout, ex, d2 = np.zeros(cap, AS.REG_DTYPE), np.zeros(cap, AS.EXTRA_DTYPE), np.zeros(cap, np.int32)
        cig, off = np.zeros(cap * (2 * len(seq) + 16), np.uint32), np.zeros(cap + 1, np.int64)
        sr, sa, pr = np.zeros(cap, AS.REG_DTYPE), np.zeros((len(a) + 1, 2), np.uint64), np.zeros(cap, AS.REG_DTYPE)
        n_sq, n_sq_a, n_pre = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        n = lib.drv_read(mi, row.ctypes.data, prow.ctypes.data, len(seq), seq, int(sc.hash_[rd]), len(u), u.ctypes.data, len(a), a.ctypes.data, len(mp),
                         mp.ctypes.data, int(m.rep_len[rd]), cap, rout.ctypes.data, ex.ctypes.data, d2.ctypes.data, len(cig), cig.ctypes.data, off.ctypes.data,
                         sr.ctypes.data, sa.ctypes.data, C.byref(n_sq), C.byref(n_sq_a), pr.ctypes.data, C.byref(n_pre))
        assert n >= 0 and n_sq.value >= 0 and n_sq_a.value >= 0, (rd, n, n_sq.value, n_sq_a.value)
        regs.append(rout[:n]); extra.append(ex[:n]); dp2.append(d2[:n])
        cigs += [cig[int(off[i]):int(off[i + 1])] for i in range(n)]
        a_out.append(a[:n_sq_a.value]); sq_regs.append(sr[:n_sq.value]); sq_a.append(sa[:n_sq_a.value]); pre.append(pr[:n_pre.value])
    lib.drv_index_free(mi)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if sum(len(x) for x in parts) else np.zeros(0, dt)
    cat2 = lambda parts: np.concatenate(parts) if sum(len(x) for x in parts) else np.zeros((0, 2), np.uint64)
    return dict(regs_off=K.offsets([len(r) for r in regs]), regs=cat(regs, AS.REG_DTYPE), extra=cat(extra, AS.EXTRA_DTYPE), dp_max2=cat(dp2, np.int32),
                cigar_off=K.offsets([len(c) for c in cigs]), cigar=cat(cigs, np.uint32), a_off=K.offsets([len(x) for x in a_out]), a=cat2(a_out),
                sq_regs_off=K.offsets([len(r) for r in sq_regs]), sq_regs=cat(sq_regs, AS.REG_DTYPE), sq_a_off=K.offsets([len(x) for x in sq_a]), sq_a=cat2(sq_a),
                pre_regs=cat(pre, AS.REG_DTYPE))


COMPARED = M.OUTPUTS + ("a_off", "a", "sq_regs_off", "sq_regs", "sq_a_off", "sq_a")


def main():
    tmp = tempfile.mkdtemp(prefix="map_align_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(OUT, exist_ok=True)
        M.cover.clear()
        total = 0
        for name in S.SCENES:
            sc = S.scene(name)
            model = M.run(sc)                          # raises where a scene is refused: none may be
            m = em.model_of(sc)
            ref = ref_scene(lib, sc, m)
            assert ref["pre_regs"].tobytes() == m.regs.tobytes(), (name, "the regions before alignment, div included")
            for k in COMPARED:
                u, v = np.asarray(model[k]), ref[k]
                if u.shape != v.shape or u.tobytes() != v.tobytes():
                    bad = np.nonzero(u != v)[0][:4] if u.shape == v.shape else (u.shape, v.shape)
                    raise AssertionError((name, k, bad, u[bad] if u.shape == v.shape else None, v[bad] if u.shape == v.shape else None))
            path = os.path.join(OUT, name + ".npz")
            np.savez_compressed(path, digest=digest(sc), rep_len=m.rep_len, n_anchors=np.int64(m.n_anchors), **{k + "_out": ref[k] for k in COMPARED})
            assert os.path.getsize(path) < 1 << 20
            total += os.path.getsize(path)
            print(f"{name}.npz: {len(sc.reads)} reads, {len(m.regs)} regions before alignment, {len(ref['regs'])} regions out, {ref['cigar_off'][-1]} CIGAR words, "
                  f"{len(ref['a'])} squeezed anchors of {int(m.b_off[-1])}, {dict(model['cover'])}, {os.path.getsize(path)} bytes")
        print(f"{total} bytes")
        print("coverage:", dict(sorted(M.cover.items())))
        missing = [k for k in M.COVER if not M.cover[k]]
        assert not missing, missing
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
