#!/usr/bin/env python3
"""Generates tests/golden/align_post/*.npz: what the UNMODIFIED reference makes of aligned regions between mm_align_skeleton and the
output -- the tail of align_regs (map.c:253-257) and mm_set_mapq (map.c:876) -- for the synthetic scenes of tests/apost_shapes.py and
for the alignments of the six scenes of skeleton_shapes and the two of align_reads_shapes (build container only: it needs the
reference's sources and a C compiler).

It follows make_skeleton_golden.py, whose driver text it extends: the driver is compiled beside the reference's files where they lie
into a shared object in a temporary directory outside the repository, which is removed at the end; nothing of the reference is copied.
drv_tail allocates each r->p (calloc: dp_max2 starts at 0, as mm_align1 leaves it), then calls mm_set_parent, mm_select_sub,
mm_set_sam_pri (unless MM_F_ALL_CHAINS) and mm_set_mapq in map.c's order, and records the regions (p zeroed), what r->p held, dp_max2
and the CIGARs.  For the real scenes drv_skeleton (mm_align_skeleton) runs first, per read, and the same tail after it, with a seeded
rep_len per read.

One file per scene: a synthetic scene's flat inputs (apost_shapes.pack) or a real scene's opt and rep_len (its regions are the
*_out arrays of its own golden), and the reference's outputs (regs_off_out, regs_out, extra_out, dp_max2_out, cigar_off_out, cigar_out).

Asserts on the way: tests/apost_model.py equals the reference in every word of every output; a real scene's alignment equals its own
golden; every class of apost_model.COVER occurred; the two rep_len reads of the mapq scene get different mapq; whether a dp_max on the
patch list of the patch scene's match_sc could be picked (printed)."""
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
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import apost_model as M  # noqa: E402
import apost_shapes as PS  # noqa: E402
import make_skeleton_golden as MS  # noqa: E402
from align_shapes import EXTRA_DTYPE, REG_DTYPE  # noqa: E402

OUT = PS.GOLDEN

TAIL = r"""
/* The tail of align_regs (map.c:253-257) and mm_set_mapq (map.c:876) over one read's n regions.  o: flag, mask_level, pri_ratio, best_n,
 * min_diff, sub_diff, min_chain_score, match_sc, is_sr.  extra: five words per region (has_extra, dp_score, dp_max, n_ambi, n_cigar);
 * every r->p is allocated here.  Returns the number of final regions. */
int drv_tail(const double *o, int n, mm_reg1_t *regs, const int32_t *extra, const int64_t *cigar_off, const uint32_t *cigar, int rep_len,
             int32_t *extra_out, int32_t *dp_max2, uint32_t *cigar_out, int64_t *cigar_off_out)
{
	int i, flag = (int)o[0];
	int64_t n_cigar = 0;
	for (i = 0; i < n; ++i) {
		const int32_t *x = extra + 5 * i;
		mm_extra_t *p = 0;
		if (x[0]) {
			p = (mm_extra_t*)calloc(1, sizeof(mm_extra_t) + (size_t)x[4] * 4);
			p->capacity = x[4], p->dp_score = x[1], p->dp_max = x[2], p->n_ambi = x[3], p->n_cigar = x[4];
			memcpy(p->cigar, cigar + cigar_off[i], (size_t)x[4] * 4);
		}
		regs[i].p = p;
	}
	if (!(flag & MM_F_ALL_CHAINS)) {
		mm_set_parent(0, (float)o[1], n, regs, (int)o[5]);
		mm_select_sub(0, (float)o[2], (int)o[4], (int)o[3], &n, regs);
		mm_set_sam_pri(n, regs);
	}
	mm_set_mapq(0, n, regs, (int)o[6], (int)o[7], rep_len, (int)o[8]);
	cigar_off_out[0] = 0;
	for (i = 0; i < n; ++i) {
		mm_extra_t *p = regs[i].p;
		memset(&extra_out[5 * i], 0, 5 * sizeof(int32_t));
		dp_max2[i] = 0;
		if (p) {
			extra_out[5 * i] = 1, extra_out[5 * i + 1] = p->dp_score, extra_out[5 * i + 2] = p->dp_max, extra_out[5 * i + 3] = p->n_ambi, extra_out[5 * i + 4] = p->n_cigar;
			dp_max2[i] = p->dp_max2;
			memcpy(cigar_out + n_cigar, p->cigar, p->n_cigar * 4);
			n_cigar += p->n_cigar;
			free(p);
		}
		cigar_off_out[i + 1] = n_cigar;
		memset(&regs[i].p, 0, sizeof(regs[i].p));
	}
	return n;
}
"""


def build(tmp):
    MS.DRIVER = MS.DRIVER + TAIL
    lib = MS.build(tmp)
    lib.drv_tail.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return lib


def ref_tail(lib, opt, rep_len, regs_off, regs, extra, cigar_off, cigar):
    """The reference's tail over a batch, read by read: the dict apost_model.run returns."""
    o = np.array([opt[k] for k in ("flag", "mask_level", "pri_ratio", "best_n", "min_diff", "sub_diff", "min_chain_score", "match_sc", "is_sr")], np.float64)
    outs = []
    for rd in range(len(regs_off) - 1):
        g0, g1 = int(regs_off[rd]), int(regs_off[rd + 1])
        n = g1 - g0
        r = np.ascontiguousarray(regs[g0:g1]).copy() if n else np.zeros(1, REG_DTYPE)
        x = np.ascontiguousarray(extra[g0:g1]).copy() if n else np.zeros(1, EXTRA_DTYPE)
        coff = np.ascontiguousarray(cigar_off[g0:g1 + 1] - cigar_off[g0])
        cig = np.ascontiguousarray(cigar[int(cigar_off[g0]):int(cigar_off[g1])]) if n else np.zeros(0, np.uint32)
        cig = cig if len(cig) else np.zeros(1, np.uint32)
        xo, d2, co, cofo = np.zeros(max(n, 1), EXTRA_DTYPE), np.zeros(max(n, 1), np.int32), np.zeros(max(int(coff[-1]), 1), np.uint32), np.zeros(n + 1, np.int64)
        k = lib.drv_tail(o.ctypes.data, n, r.ctypes.data, x.ctypes.data, coff.ctypes.data, cig.ctypes.data, int(rep_len[rd]), xo.ctypes.data, d2.ctypes.data,
                         co.ctypes.data, cofo.ctypes.data)
        assert 0 <= k <= n
        outs.append((r[:k], xo[:k], d2[:k], [co[int(cofo[i]):int(cofo[i + 1])] for i in range(k)]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if sum(len(p) for p in parts) else np.zeros(0, dt)
    cigs = [c for t in outs for c in t[3]]
    return dict(regs_off=M.offsets([len(t[0]) for t in outs]), regs=cat([t[0] for t in outs], REG_DTYPE), extra=cat([t[1] for t in outs], EXTRA_DTYPE),
                dp_max2=cat([t[2] for t in outs], np.int32), cigar_off=M.offsets([len(c) for c in cigs]), cigar=cat(cigs, np.uint32))


def words(x):
    return x.view(np.uint32) if x.dtype.fields else x


def compare(name, model, ref):
    for k in M.OUTPUTS:
        u, v = model[k], ref[k]
        if u.shape != v.shape or not np.array_equal(words(u), words(v)):
            bad = np.nonzero(u != v)[0][:4] if u.shape == v.shape else (u.shape, v.shape)
            raise AssertionError((name, k, bad, u[bad] if u.shape == v.shape else None, v[bad] if u.shape == v.shape else None))


def save(name, ref, **inputs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k + "_out": ref[k] for k in M.OUTPUTS}, **inputs)
    assert os.path.getsize(path) < 1 << 20
    print(f"{name}.npz: {len(inputs['rep_len'])} reads, {len(ref['regs'])} regions out, {int(ref['cigar_off'][-1])} CIGAR words, {os.path.getsize(path)} bytes")


def main():
    from minimap2_chaindp_amd import chaindp
    tmp = tempfile.mkdtemp(prefix="apost_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(OUT, exist_ok=True)
        M.cover.clear()
        pk, _ = chaindp.apost_logf_patches(PS.PATCH_MATCH_SC)
        pick = int(pk[pk >= 100][0]) if (pk >= 100).any() else None
        print(f"patch scene: match_sc {PS.PATCH_MATCH_SC}, {len(pk)} dp_max on the host's list, picked {pick}")
        assert (pick is not None) == bool((pk >= 100).any())
        for name in PS.SYNTHETIC:
            p = PS.pack(PS.scene(name, patch_dp_max=pick or 1000))
            opt = PS.opt_of(p["opt"])
            args = (opt, p["rep_len"], p["regs_off"], p["regs"], p["extra"], p["cigar_off"], p["cigar"])
            model, ref = M.run(*args), ref_tail(lib, *args)
            compare(name, model, ref)
            if name == "mapq":
                o = ref["regs_off"]
                a, b = ref["regs"]["bits"][o[7]:o[8]] & 0xff, ref["regs"]["bits"][o[8]:o[9]] & 0xff
                assert len(a) == len(b) and (a != b).any() and (a > 0).all() and (b > 0).all(), (a, b)
            save(name, ref, patch_dp_max=np.int64(pick or 0), **p)
        for name in PS.REAL:
            loader, sub = PS.real_source(name)
            g = loader(sub)
            sk = MS.ref_scene(lib, g)                                    # mm_align_skeleton, read by read
            for k in ("regs_off", "regs", "extra", "cigar_off", "cigar"):
                assert np.array_equal(words(sk[k]), words(g[k + "_out"])), (name, k)
            opt, rep_len = PS.real_opt(g["opt"]), PS.real_rep_len(name, len(g["seq_off"]) - 1)
            args = (opt, rep_len, sk["regs_off"], sk["regs"], sk["extra"], sk["cigar_off"], sk["cigar"])
            model, ref = M.run(*args), ref_tail(lib, *args)
            compare(name, model, ref)
            save(name, ref, opt=PS.opt_row(opt), rep_len=rep_len)
        print("coverage:", dict(sorted(M.cover.items())))
        missing = [k for k in M.COVER if not M.cover[k]]
        assert not missing, missing
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
