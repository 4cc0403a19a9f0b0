"""DP parameter presets, as the reference derives them for mm_chain_dp_fpga.

Argument order and meaning follow reference chain.c:218 / mmpriv.h:69:
``max_dist_x`` = max_chain_gap_ref, ``max_dist_y`` = max_chain_gap_qry
(map.c:358-366, passed at map.c:525), ``bw``/``max_skip``/``min_sc``/``is_cdna``
from fpga_set_params (main.c:243), ``n_segs`` per read.
"""
import ctypes as C


class ChainParams(C.Structure):
    """Mirror of chaindp_params_t (include/chaindp.h) and co_params_t (oracle/chain_oracle.h)."""
    _fields_ = [(k, C.c_int32) for k in
                ("max_dist_x", "max_dist_y", "bw", "max_skip", "min_sc", "is_cdna", "n_segs")]

    def astuple(self):
        return tuple(getattr(self, k) for k, _ in self._fields_)

    def __repr__(self):
        return "ChainParams(" + ", ".join(f"{k}={getattr(self, k)}" for k, _ in self._fields_) + ")"


# options.c:29-34 (defaults), :84-87 (ava-ont), :88-92 (ava-pb), :95-96 (map-ont), :111-131 (sr), :132-139 (splice)
PRESETS = {
    "map-ont": dict(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=25, min_sc=40, is_cdna=0, n_segs=1),
    "ava-ont": dict(max_dist_x=10000, max_dist_y=10000, bw=500, max_skip=25, min_sc=100, is_cdna=0, n_segs=1),
    "ava-pb": dict(max_dist_x=10000, max_dist_y=10000, bw=2000, max_skip=25, min_sc=100, is_cdna=0, n_segs=1),
    # short paired reads, 2 x 150 bp: gap_ref = max(max_frag_len - qlen_sum, max_gap) = 500, gap_qry = max(qlen_sum, max_gap) = 300
    "sr": dict(max_dist_x=500, max_dist_y=300, bw=100, max_skip=25, min_sc=25, is_cdna=0, n_segs=2),
    "splice": dict(max_dist_x=200000, max_dist_y=2000, bw=200000, max_skip=25, min_sc=40, is_cdna=1, n_segs=1),
}


def preset(name, **overrides):
    d = dict(PRESETS[name])
    d.update(overrides)
    return ChainParams(**d)


def read_gaps(max_gap, max_gap_ref, max_frag_len, is_sr, qlen_sum):
    """The chaining gaps the reference derives per read from its total length (map.c:358-366; chaindp_read_gaps, needs no GPU):
    (gap_ref int32[n], gap_qry int32[n]) for qlen_sum int32[n] -- what Device.set_read_gaps and the `gaps=` keyword take."""
    import numpy as np
    from . import chaindp
    q = np.ascontiguousarray(qlen_sum, np.int32)
    gr, gq = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
    chaindp.lib().chaindp_read_gaps(int(max_gap), int(max_gap_ref), int(max_frag_len), int(bool(is_sr)), len(q),
                                    q.ctypes.data if len(q) else None, gr.ctypes.data if len(q) else None, gq.ctypes.data if len(q) else None)
    return gr, gq


# ---- chain_post / mm_set_mapq options (chaindp_post_opt_t) ---------------------------------------------------------------

MM_F_NO_DIAG, MM_F_NO_DUAL, MM_F_CIGAR = 0x001, 0x002, 0x004          # minimap.h:8-10
MM_F_SPLICE, MM_F_NO_LJOIN, MM_F_SR = 0x080, 0x400, 0x1000            # minimap.h:15,18,20
MM_F_ALL_CHAINS = 0x800000                                            # minimap.h:31


class PostOpt(C.Structure):
    """Mirror of chaindp_post_opt_t (include/chaindp.h): the mm_mapopt_t fields chain_post, mm_est_err and mm_set_mapq read."""
    _fields_ = [("flag", C.c_int32), ("mask_level", C.c_float), ("pri_ratio", C.c_float)] + \
               [(k, C.c_int32) for k in ("best_n", "min_diff", "sub_diff", "max_join_long", "max_join_short", "min_join_flank_sc",
                                          "min_cnt", "min_chain_score", "match_sc", "is_sr")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def __repr__(self):
        return "PostOpt(" + ", ".join(f"{k}={v}" for k, v in self.asdict().items()) + ")"


# mm_mapopt_init (options.c:28-45): mask_level, pri_ratio, best_n, the join limits, min_cnt, min_chain_score, a = 2, b = 4
_POST_DEFAULTS = dict(flag=0, mask_level=0.5, pri_ratio=0.8, best_n=5, max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000,
                      min_cnt=3, min_chain_score=40, match_sc=2, sub_diff=2 * 2 + 4, is_sr=0)
# mm_set_opt (options.c:84-96): k of the preset's index (min_diff = mi->k * 2, map.c:242), the map options it changes
POST_PRESETS = {
    "map-ont": dict(min_diff=2 * 15),
    "map-pb": dict(min_diff=2 * 19),
    "ava-ont": dict(min_diff=2 * 15, flag=MM_F_ALL_CHAINS | MM_F_NO_DIAG | MM_F_NO_DUAL | MM_F_NO_LJOIN, min_chain_score=100, pri_ratio=0.0),
    "ava-pb": dict(min_diff=2 * 19, flag=MM_F_ALL_CHAINS | MM_F_NO_DIAG | MM_F_NO_DUAL | MM_F_NO_LJOIN, min_chain_score=100, pri_ratio=0.0),
    # options.c:115-131: paired short reads (k = 21, a = 2, b = 8); chaindp_frag_post / map_frags / map_frag_seqs
    "sr": dict(min_diff=2 * 21, flag=MM_F_SR, pri_ratio=0.5, best_n=20, min_cnt=2, min_chain_score=25, match_sc=2, sub_diff=2 * 2 + 8, is_sr=1),
}


def post_preset(name, **overrides):
    d = dict(_POST_DEFAULTS)
    d.update(POST_PRESETS[name])
    d.update(overrides)
    return PostOpt(**d)


# ---- mm_align1 options (chaindp_align_opt_t) ------------------------------------------------------------------------------

class AlignOpt(C.Structure):
    """Mirror of chaindp_align_opt_t (include/chaindp_align.h): the fields of mm_mapopt_t and mm_idx_t that mm_align1 reads."""
    _fields_ = [(k, C.c_int32) for k in ("a", "b", "q", "e", "q2", "e2", "bw", "zdrop", "zdrop_inv", "end_bonus", "min_cnt", "min_chain_score",
                                         "min_dp_max", "min_ksw_len", "max_gap", "flag", "k", "is_hpc")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# options.c:29-48 (mm_mapopt_init) and, per preset, what mm_set_opt changes of it (options.c:84-114); flag holds only the bits
# mm_align1 looks at (none of these presets sets one)
_ALIGN_DEFAULTS = dict(a=2, b=4, q=4, e=2, q2=24, e2=1, bw=500, zdrop=400, zdrop_inv=200, end_bonus=-1, min_cnt=3, min_chain_score=40,
                       min_dp_max=80, min_ksw_len=200, max_gap=5000, flag=0, k=15, is_hpc=0)
ALIGN_PRESETS = {
    "map-ont": {},
    "map-pb": dict(k=19, is_hpc=1),
    "ava-ont": dict(min_chain_score=100, max_gap=10000),
    "ava-pb": dict(k=19, is_hpc=1, min_chain_score=100, max_gap=10000, bw=2000),
    "asm5": dict(k=19, a=1, b=19, q=39, q2=81, e=3, e2=1, zdrop=200, zdrop_inv=200, min_dp_max=200),
    "asm10": dict(k=19, a=1, b=9, q=16, q2=41, e=2, e2=1, zdrop=200, zdrop_inv=200, min_dp_max=200),
    "asm20": dict(k=19, a=1, b=4, q=6, q2=26, e=2, e2=1, zdrop=200, zdrop_inv=200, min_dp_max=200),
}


def align_opt(name, **overrides):
    """chaindp_align_opt_t of a long-read preset, what Device.align1 takes."""
    d = dict(_ALIGN_DEFAULTS)
    d.update(ALIGN_PRESETS[name])
    d.update(overrides)
    return AlignOpt(**d)
