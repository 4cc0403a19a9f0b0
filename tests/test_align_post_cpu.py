"""CPU tier of Device.align_post (chaindp_align_post and its siblings): the goldens tests/golden/align_post/*.npz (made by
tests/golden/make_apost_golden.py from the unmodified reference's mm_set_parent, mm_select_sub, mm_set_sam_pri and mm_set_mapq) load,
are the scenes of tests/apost_shapes.py, reach every class and are reproduced by tests/apost_model.py; the calls' prototypes bind
through their header, their _CAPS rows retry by the fetch call, the no-GPU hook makes the refusals, and the host half of the logf
list reproduces the host's logf((float)dp_max / match_sc)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import apost_model as M
import apost_shapes as PS
import post_oracle as po

STABLE = ("chaindp_align_post", "chaindp_align_post_regs", "chaindp_align_reads_post", "chaindp_align_post_fetch")
HOOKS = ("chaindp_align_post_debug_check", "chaindp_align_post_debug_set_lds_cap", "chaindp_align_post_debug_ms", "chaindp_apost_logf_patches",
         "chaindp_apost_logf_selftest")


def words(x):
    return x.view(np.uint32) if x.dtype.fields else x


def same(u, v):
    return u.shape == v.shape and np.array_equal(words(np.ascontiguousarray(u)), words(np.ascontiguousarray(v)))


def inputs(name):
    """(golden, opt dict, rep_len, regs_off, regs, extra, cigar_off, cigar) of a scene, synthetic (the edge tier's too) or real."""
    g = PS.load(name)
    if name not in PS.REAL:
        src = g
        arrs = [g[k] for k in ("regs_off", "regs", "extra", "cigar_off", "cigar")]
    else:
        loader, sub = PS.real_source(name)
        src = loader(sub)
        arrs = [src[k + "_out"] for k in ("regs_off", "regs", "extra", "cigar_off", "cigar")]
    return (g, PS.opt_of(g["opt"]), g["rep_len"], *arrs)


def test_fixtures_are_there_and_small():
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PS.GOLDEN, "*.npz")))
    assert files == sorted(PS.SYNTHETIC + PS.REAL)
    assert all(os.path.getsize(os.path.join(PS.GOLDEN, n + ".npz")) < 1 << 20 for n in files)


def test_shapes_are_what_was_recorded():
    for name in PS.SYNTHETIC:
        g = PS.load(name)
        p = PS.pack(PS.scene(name, patch_dp_max=int(g["patch_dp_max"]) or 1000))
        for k in PS.INPUTS:
            assert same(np.asarray(p[k]), g[k]), (name, k)
    for name in PS.REAL:
        g = PS.load(name)
        loader, sub = PS.real_source(name)
        src = loader(sub)
        assert same(g["rep_len"], PS.real_rep_len(name, len(src["seq_off"]) - 1)) and same(g["opt"], PS.opt_row(PS.real_opt(src["opt"]))), name
    caps = {n: int(PS.load(n)["lds_cap"]) for n in PS.SYNTHETIC}
    assert caps["lds_cap"] == PS.SCENE_CAP and all(v == PS.AP_LDS_CAP for k, v in caps.items() if k != "lds_cap") and 2 < PS.SCENE_CAP < PS.AP_LDS_CAP < 64


def test_model_reproduces_the_reference_and_reaches_every_class():
    M.cover.clear()
    for name in PS.SYNTHETIC + PS.REAL:
        g, *args = inputs(name)
        got = M.run(*args)
        for k in M.OUTPUTS:
            assert same(got[k], g[k + "_out"]), (name, k)
    assert not [k for k in M.COVER if not M.cover[k]], dict(M.cover)


def test_scenes_show_what_they_are_named_for():
    g = PS.load("structure")
    o, oo = g["regs_off"], g["regs_off_out"]
    dropped = (o[1:] - o[:-1]) - (oo[1:] - oo[:-1])
    assert dropped[0] > 0 and dropped[-1] > 0                                   # the first and the last read of the batch drop a region
    assert g["dp_max2_out"][oo[3]] == 0 and g["dp_max2_out"][oo[4]] == 992      # identical hits after DP set no dp_max2; others do
    assert g["regs_out"]["n_sub"][oo[4]] == 1 and g["regs_out"]["n_sub"][oo[5]] == 0   # sub_diff exactly, and one more
    g = PS.load("keeps_all")
    assert same(g["regs_off"], g["regs_off_out"]) and same(g["cigar"], g["cigar_out"])
    g = PS.load("mapq")
    oo = g["regs_off_out"]
    assert (g["regs_out"]["bits"][oo[7]:oo[8]] & 0xff).tolist() != (g["regs_out"]["bits"][oo[8]:oo[9]] & 0xff).tolist()   # rep_len changes mapq
    g = PS.load("patch")
    k, _ = __import__("minimap2_chaindp_amd.chaindp", fromlist=["x"]).apost_logf_patches(PS.PATCH_MATCH_SC)
    print("patch scene: dp_max", int(g["patch_dp_max"]), "recorded;", len(k), "on this host's list")
    assert (int(g["patch_dp_max"]) > 0) or len(k) == 0


def test_the_header_binds():
    from minimap2_chaindp_amd import _cabi, chaindp
    assert chaindp.ALIGN_POST_SYMBOLS == STABLE + HOOKS
    lib = chaindp.lib()
    protos = _cabi.prototypes("chaindp_align_post.h")
    for name in STABLE + HOOKS:
        fn = getattr(lib, name)
        assert fn.restype is (C.c_int64 if "logf" in name else C.c_int) and list(fn.argtypes) == protos[name][1], name
    assert [len(protos[n][1]) for n in STABLE] == [13, 18, 20, 11]
    with open(os.path.join(_cabi.INCLUDE, "chaindp.h")) as f:
        includes = re.findall(r'#include "(chaindp_\w+\.h)"', f.read())
    assert includes.index("chaindp_align_post.h") == includes.index("chaindp_align_reads.h") + 1
    with open(os.path.join(_cabi.INCLUDE, "chaindp_align_post.h")) as f:
        text = f.read()
    assert '#include "chaindp_align_reads.h"' in text
    stable, hooks = text.split("NOT part of the stable ABI")
    assert all("%s(" % n in stable and "%s(" % n not in hooks for n in STABLE) and all("%s(" % n in hooks and " %s(" % n not in stable for n in HOOKS)
    # the sibling header keeps its functions: none of the new ones went there
    assert not set(_cabi.prototypes("chaindp_align_reads.h")) & set(STABLE + HOOKS)


def test_caps_rows_retry_by_the_fetch_call():
    from minimap2_chaindp_amd import chaindp
    for row in ("align_post", "align_post_cigar", "align_reads_post", "align_reads_post_cigar"):
        assert chaindp._CAPS[row].retry == "align_post_fetch" and chaindp._CAPS[row].explicit == "raise"
    assert "chaindp_" + chaindp._CAPS["align_post"].retry in STABLE
    for m in ("align_post", "align_reads_post", "align_post_ms", "align_post_set_lds_cap", "apost_logf_selftest", "_cigars"):
        assert callable(getattr(chaindp.Device, m))
    assert callable(chaindp.apost_logf_patches) and callable(chaindp.align_post_check)


def _check(name="structure", opt=None, caps=(0, 0), **arrays):
    from minimap2_chaindp_amd import chaindp
    g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
    po_ = PS.post_opt(PS.opt_row(dict(o, **(opt or {}))))
    a = dict(rep_len=rep_len, regs_off=regs_off, regs=regs, extra=extra, cigar_off=cigar_off, cigar=cigar)
    a.update(arrays)
    return chaindp.align_post_check(po_, a["rep_len"], a["regs_off"], a["regs"], a["extra"], a["cigar_off"], a["cigar"], *caps)


def test_debug_check_accepts_the_scenes():
    for name in PS.SYNTHETIC + PS.REAL:
        g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs(name)
        assert _check(name) == (0, len(regs), len(cigar)), name
    assert _check(regs_off=None, regs=None, extra=None, cigar_off=None, cigar=None) == (0, 0, 0)    # the resident form: opt, rep_len, capacities


def test_debug_check_refusals():
    g, o, rep_len, regs_off, regs, extra, cigar_off, cigar = inputs("structure")
    assert _check(caps=(5, 7))[0] == 0 and _check(opt=dict(is_sr=1))[0] == 0
    for opt in (dict(flag=0x1000), dict(flag=0x80), dict(flag=0x1000, is_sr=1), dict(match_sc=0), dict(match_sc=-2)):
        assert _check(opt=opt)[0] == -1, opt
    assert _check(caps=(-1, 0))[0] == -1 and _check(caps=(0, -1))[0] == -1
    rl = rep_len.copy(); rl[2] = -1
    assert _check(rep_len=rl)[0] == -1                                           # a negative rep_len
    off = regs_off.copy(); off[1] = off[2] + 1
    assert _check(regs_off=off)[0] == -1                                         # falling offsets
    off = regs_off.copy(); off[0] = 1
    assert _check(regs_off=off)[0] == -1                                         # not from 0
    coff = cigar_off.copy(); coff[3] = coff[4] + 1
    assert _check(cigar_off=coff)[0] == -1                                       # falling CIGAR offsets
    ex = extra.copy(); ex["n_cigar"][0] += 1
    assert _check(extra=ex)[0] == -1                                             # n_cigar disagrees with cigar_off
    ex = extra.copy(); ex["has_extra"][1] = 2
    assert _check(extra=ex)[0] == -1                                             # has_extra outside 0 / 1


@pytest.mark.parametrize("match_sc,kmax", [(1, 1 << 20), (4, 1 << 20), (2, 1 << 24), (3, 1 << 20), (5, 1 << 20)])
def test_logf_patch_list_reproduces_host_logf(match_sc, kmax):
    """(float)log((double)x) for x = (float)k / (float)match_sc, patched at the listed k, is the host's logf(x) for every k in [1, kmax];
    the list is built over [1, 2^24] whatever kmax is."""
    from minimap2_chaindp_amd import chaindp
    k, v = chaindp.apost_logf_patches(match_sc)
    assert np.all(np.diff(k.astype(np.int64)) > 0) and (len(k) == 0 or (k[0] >= 1 and k[-1] <= (1 << 24)))
    x = np.arange(1, kmax + 1, dtype=np.float32) / np.float32(match_sc)
    cr = np.log(x.astype(np.float64)).astype(np.float32)
    sel = k.astype(np.int64) <= kmax
    cr[k[sel].astype(np.int64) - 1] = v[sel]
    fn = po._libm.logf
    host = np.empty(kmax, np.float32)
    step = 1 << 16
    for s in range(0, kmax, step):
        host[s:s + step] = [fn(t) for t in x[s:s + step].tolist()]
    bad = np.flatnonzero(host.view(np.uint32) != cr.view(np.uint32))
    assert bad.size == 0, f"{bad.size} mismatches, first k = {bad[:5] + 1}"
    for kk, vv in zip(k[:64].tolist(), v[:64].tolist()):                        # the listed values are the host's
        assert po.host_logf(np.float32(kk) / np.float32(match_sc)) == np.float32(vv)
