#!/usr/bin/env python3
"""Generates tests/golden/align_post_edges/*.npz: what the UNMODIFIED reference's tail of align_regs and mm_set_mapq make of the scenes
of tests/apost_edge_shapes.py (build container only: it needs the reference's sources and a C compiler).  The driver, its build in a
temporary directory outside the repository and the per-read run are make_apost_golden.py's; nothing of the reference is copied.  The
files have the format of tests/golden/align_post/*.npz, with the picked patch keys beside (`picks`, rows of PICK_LISTS).

The picks come from this host's logf lists: per list the first listed key >= 100, the first whose listed value is not the float
(float)log((double)x), and a (subsc, score0) at which that one ulp moves the recorded mapq.

Asserts on the way: tests/apost_model.py equals the reference in every word of every output; every class of apost_model.EDGE_COVER
occurred; every file is below 1 MiB.  Prints the sizes and the picks."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import apost_edge_shapes as E  # noqa: E402
import apost_model as M  # noqa: E402
import apost_shapes as PS  # noqa: E402
from make_apost_golden import build, compare, ref_tail  # noqa: E402

F32 = np.float32


def tune(lg_host, lg_cr, identity):
    """(subsc, score0) at which (int)(identity * 40 * (1 - subsc / score0) * lg) differs between the two logarithms and lies in 1..59
    with both; None if there is none."""
    subsc = np.arange(40, 2040, dtype=np.int64)[:, None]
    score0 = np.arange(41, 4041, dtype=np.int64)[None, :]
    with np.errstate(all="ignore"):
        f = F32(identity) * F32(1.0) * F32(40.0) * (F32(1.0) - subsc.astype(F32) / score0.astype(F32))
        a, b = (f * F32(lg_host)).astype(np.int64), (f * F32(lg_cr)).astype(np.int64)
    ok = (a != b) & (a > 0) & (a < 60) & (b > 0) & (b < 60) & (subsc < score0)
    hit = np.argwhere(ok)
    return (int(subsc[hit[0][0], 0]), int(score0[0, hit[0][1]])) if len(hit) else None


def pick(k, v, divisor, identity):
    """A list's picks (apost_edge_shapes.PICK_FIELDS)."""
    k, v = k.astype(np.int64), v.astype(F32)
    x = k.astype(F32) / F32(divisor)
    cr = np.log(x.astype(np.float64)).astype(F32)
    at = np.flatnonzero(k >= 100)
    if not len(at):
        return dict(E.NO_PICK)
    out = dict(E.NO_PICK, key=int(k[at[0]]))
    for i in at[v[at].view(np.uint32) != cr[at].view(np.uint32)][:64]:
        t = tune(v[i], cr[i], identity)
        if t:
            out.update(key_d=int(k[i]), subsc=t[0], score0=t[1])
            break
    return out


def main():
    from minimap2_chaindp_amd import chaindp
    tmp = tempfile.mkdtemp(prefix="apost_edge_ref_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        lib = build(tmp)
        os.makedirs(E.GOLDEN, exist_ok=True)
        M.cover.clear()
        picks = {"int": pick(*chaindp.post_logf_patches(), 1, 1.0)}
        for m in E.PATCH_SC:
            picks["sc%d" % m] = pick(*chaindp.apost_logf_patches(m), m, F32(900) / F32(1000))
        for l in E.PICK_LISTS:
            print(f"list {l}: picked {picks[l]}" + ("" if picks[l]["key"] else " (empty list: dp_max 1000)"))
        for name in E.SCENES:
            p = PS.pack(E.scene(name, picks))
            opt = PS.opt_of(p["opt"])
            args = (opt, p["rep_len"], p["regs_off"], p["regs"], p["extra"], p["cigar_off"], p["cigar"])
            model, ref = M.run(*args), ref_tail(lib, *args)
            compare(name, model, ref)
            path = os.path.join(E.GOLDEN, name + ".npz")
            np.savez_compressed(path, **{k + "_out": ref[k] for k in M.OUTPUTS}, picks=E.picks_row(picks), **p)
            assert os.path.getsize(path) < 1 << 20
            print(f"{name}.npz: {len(p['rep_len'])} reads, {len(p['regs'])} regions in, {len(ref['regs'])} out, {int(ref['cigar_off'][-1])} CIGAR words, "
                  f"{os.path.getsize(path)} bytes")
        print("coverage:", {k: M.cover[k] for k in M.EDGE_COVER})
        missing = [k for k in M.EDGE_COVER if not M.cover[k]]
        assert not missing, missing
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
