"""Python front end of the C ABI in include/chaindp.h (libchaindp_hip.so).

Thin by design: numpy arrays in, numpy arrays out, every call goes through the C ABI to the HIP
kernels.  There is NO CPU implementation behind this module: a missing library or a missing GPU
raises.  Per read the results equal the reference's mm_chain_dp_fpga (chain.c:218-327).
"""
import collections
import contextlib
import ctypes as C
import os

import numpy as np


from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
# CHAINDP_LIB: an alternative build of the same library (A/B timing of kernel variants on one box, tools/ab.sh)
LIB_PATH = os.environ.get("CHAINDP_LIB") or os.path.join(_HERE, "csrc", "libchaindp_hip.so")

SEED_DTYPE = np.dtype([("x", "<u8"), ("y", "<u8"), ("p", "<i4"), ("f", "<i4")])  # struct new_seed (minimap.h:51-55)

# every symbol include/chaindp.h declares (tests check the library exports all of them)
ABI_SYMBOLS = tuple(_cabi.prototypes("chaindp.h"))
# ... and the ones of the header it includes for per-read gaps
GAPS_SYMBOLS = tuple(_cabi.prototypes("chaindp_gaps.h"))
# ... and for the alignment
KSW_SYMBOLS = tuple(_cabi.prototypes("chaindp_ksw.h"))
# KSW_EZ_* of the reference's ksw2.h that Device.ksw_extd takes, and the fields of its ez rows
KSW_SCORE_ONLY, KSW_RIGHT, KSW_APPROX_MAX, KSW_EXTZ_ONLY, KSW_REV_CIGAR = 0x01, 0x02, 0x08, 0x40, 0x80
KSW_EZ_FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "reach_end")
# ... and for mm_align1
ALIGN_SYMBOLS = tuple(_cabi.prototypes("chaindp_align.h"))
# ... and for mm_align1_inv
ALIGN_INV_SYMBOLS = tuple(_cabi.prototypes("chaindp_align_inv.h"))
# ... and for mm_align_skeleton
ALIGN_READS_SYMBOLS = tuple(_cabi.prototypes("chaindp_align_reads.h"))
# ... and for the tail of align_regs and mm_set_mapq over aligned regions
ALIGN_POST_SYMBOLS = tuple(_cabi.prototypes("chaindp_align_post.h"))
ALIGN_EXTRA_DTYPE = np.dtype([(k, "<i4") for k in ("has_extra", "dp_score", "dp_max", "n_ambi", "n_cigar")])   # chaindp_align_extra_t
ERR_CAPACITY = -2

# chaindp_reg_t == mm_reg1_t (minimap.h:100-115), 80 bytes; `bits` is the bit-field word (rev = bit 10)
REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as", "mlen", "blen", "n_sub", "score0")]
                     + [("bits", "<u4"), ("hash", "<u4"), ("div", "<f4"), ("reserved", "<u4", (2,))])


class ChainDPError(RuntimeError):
    pass


_lib = None


def lib():
    """The library, every function of include/chaindp.h, chaindp_gaps.h, chaindp_ksw.h, chaindp_align.h, chaindp_align_inv.h, chaindp_align_reads.h, chaindp_align_post.h, chaindp_map_align.h and chaindp_debug.h bound with the
    header's prototype."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ChainDPError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                               "(make -C minimap2_chaindp_amd/csrc); there is no fallback path")
        _lib = _cabi.bind(C.CDLL(LIB_PATH), "chaindp.h", "chaindp_gaps.h", "chaindp_ksw.h", "chaindp_align.h", "chaindp_align_inv.h", "chaindp_align_reads.h",
                          "chaindp_align_post.h", "chaindp_map_align.h", "chaindp_debug.h")
    return _lib


def post_logf_patches():
    """The host's logf patch list (needs no GPU): (k uint32[n], logf(k) float32[n]) for the integers k in [1, 2^24] where the host's
    logf differs from the correctly rounded (float)log((double)k)."""
    L = lib()
    n = int(L.chaindp_post_logf_patches(None, None, 0))
    k, v = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float32)
    L.chaindp_post_logf_patches(_ptr(k), _ptr(v), n)
    return k[:n], v[:n]


def apost_logf_patches(match_sc):
    """The host's patch list of logf((float)dp_max / match_sc) (needs no GPU): (dp_max uint32[n], value float32[n]) for the dp_max in
    [1, 2^24] where the host's logf is not the float the device computes by itself (the correctly rounded (float)log((double)x), x the
    float quotient), or where log(x) comes too close to a float rounding midpoint for that to be certain."""
    L = lib()
    n = int(L.chaindp_apost_logf_patches(int(match_sc), None, None, 0))
    if n < 0:
        raise ValueError("match_sc must be positive")
    k, v = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float32)
    L.chaindp_apost_logf_patches(int(match_sc), _ptr(k), _ptr(v), n)
    return k[:n], v[:n]


def align_post_check(opt, rep_len, regs_off=None, regs=None, extra=None, cigar_off=None, cigar=None, regs_cap=0, cigar_cap=0):
    """What Device.align_post makes of its arguments before anything touches the device (test hook, needs no GPU): (rc, regions,
    CIGAR words handed in); rc is 0 or CHAINDP_ERR_ARG (-1)."""
    rep_len = _arr(rep_len, np.int32)
    regs_off, regs, extra = _arr(regs_off, np.int64), _arr(regs, REG_DTYPE), _arr(extra, ALIGN_EXTRA_DTYPE)
    cigar_off, cigar = _arr(cigar_off, np.int64), _arr(cigar, np.uint32)
    out = (C.c_int64 * 2)()
    rc = lib().chaindp_align_post_debug_check(C.byref(opt) if opt is not None else None, len(rep_len), _ptr0(rep_len), _ptr(regs_off), _ptr0(regs), _ptr0(extra),
                                              _ptr(cigar_off), _ptr0(cigar), int(regs_cap), int(cigar_cap), out)
    return rc, int(out[0]), int(out[1])


def device_count():
    return lib().chaindp_device_count()


def ksw_routing():
    """What Device.ksw_extd routes a problem by (needs no GPU): dict of lds_budget and the bytes of state per_target, per_query (both
    lengths rounded up to 16 first) and fixed; a problem whose sum fits the budget keeps its state in LDS, others in global scratch;
    a sum above wide_bytes gets wide_waves waves instead of one."""
    out = (C.c_int64 * 6)()
    lib().chaindp_ksw_debug_routing(out)
    return dict(zip(("lds_budget", "per_target", "per_query", "fixed", "wide_bytes", "wide_waves"), (int(x) for x in out)))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _ptr0(a):
    """_ptr, but an empty array goes as NULL too."""
    return None if a is None or not len(a) else a.ctypes.data


def _arr(x, dtype):
    """x as a C-contiguous array of dtype; None stays None (the C side's "not given")."""
    return None if x is None else np.ascontiguousarray(x, dtype)


# What the calls that return hits do about the room for them.  regs_cap=None allocates max(source // divisor, REGS_CAP_FLOOR) records
# (floored=False: at least 1), where source is the batch's minimizer count ("n_mini"), its bases ("n_bases") or the resident batch's
# anchors ("total").  When the C call answers CHAINDP_ERR_CAPACITY with more hits than that: a guess is always retried, a cap the
# caller gave is retried or raises (explicit); retry names the call that fetches the hits with the exact count ("again": the whole
# call once more, None: nothing to retry with).  state: _n_reads / _total follow the batch "before" or "after" rc is looked at.
REGS_CAP_FLOOR = 1024
_Cap = collections.namedtuple("_Cap", "source divisor floored explicit retry state")
_CAPS = {
    "map_batch":     _Cap("n_mini",  4,  True,  "retry", "gen_regs",   "after"),
    "chain_post":    _Cap("total",   1,  False, "raise", None,         None),      # room for every input hit: never short
    "map_reads":     _Cap("n_mini",  4,  True,  "retry", "chain_post", "before"),
    "map_seqs":      _Cap("n_bases", 32, True,  "retry", "chain_post", "before"),
    "frag_post":     _Cap("total",   4,  True,  "raise", "again",      None),
    "map_frags":     _Cap("n_mini",  2,  True,  "raise", "frag_post",  "before"),
    "map_frag_seqs": _Cap("n_bases", 16, True,  "raise", "again",      "before"),  # again: the flip is part of the call
    # _cigars: the room is for CIGAR words, not hits.  align1: a guess of one word per four read bases, the whole call again with the exact count
    "align1":        _Cap("n_bases", 4,  True,  "raise", "again",      None),
    "align1_inv":    _Cap("n_bases", 4,  True,  "raise", "again",      None),      # the same for the inversions' CIGAR words
    # align_reads has both kinds of room: final regions (a guess of twice the input regions) and their CIGAR words.  The result stays
    # resident, so a guess that was short is made good by the fetch call, nothing is computed again
    "align_reads":       _Cap("n_regs2", 1, True, "raise", "align_reads_fetch", None),
    "align_reads_cigar": _Cap("n_bases", 4, True, "raise", "align_reads_fetch", None),
    # align_post finishes regions that are on the device or come from the host: nothing is added, so the regions and words handed in are
    # room enough; for the resident result of align_reads the host knows neither count, guesses, and fetches what was short
    "align_post":        _Cap("n_regs",  1, True, "raise", "align_post_fetch", None),
    "align_post_cigar":  _Cap("n_words", 1, True, "raise", "align_post_fetch", None),
    "align_reads_post":       _Cap("n_regs2", 1, True, "raise", "align_post_fetch", None),
    "align_reads_post_cigar": _Cap("n_bases", 4, True, "raise", "align_post_fetch", None),
    # align_resident works on what chain_post left on the device: the host knows the reads and the batch's anchors, guesses two regions a
    # read and a CIGAR word per anchor; map_align_seqs knows the bases alone.  Both results stay resident: the fetch makes a guess good
    "align_resident":        _Cap("n_reads2", 1,  True, "raise", "align_post_fetch", None),
    "align_resident_cigar":  _Cap("total",    1,  True, "raise", "align_post_fetch", None),
    "map_align_seqs":        _Cap("n_bases",  32, True, "raise", "align_post_fetch", None),
    "map_align_seqs_cigar":  _Cap("n_bases",  4,  True, "raise", "align_post_fetch", None),
    "ksw_extd":      _Cap("n_span",  1,  False, "raise", None,         None),      # room for q_len + t_len words a problem: never short
}


class Device:
    """One chaining context on one GPU (chaindp_ctx_t)."""

    def __init__(self, device=0, max_anchors=1 << 24, max_reads=1 << 20, ring=None):
        self._lib = lib()
        if self._lib.chaindp_device_count() <= 0:
            raise ChainDPError("no HIP device visible: the chaining DP runs only on the GPU (no CPU fallback)")
        self._ctx = self._lib.chaindp_create(device, max_anchors, max_reads)
        if not self._ctx:
            raise ChainDPError(self._lib.chaindp_last_error(None).decode())
        self.device = device
        self.max_anchors, self.max_reads = max_anchors, max_reads
        self._n_reads = self._total = self._sk_n_mini = 0
        self._indexes = []
        if ring is not None:
            self._check(self._lib.chaindp_set_ring(self._ctx, ring))

    # -- lifecycle
    def close(self):
        if self._ctx:
            for h in self._indexes:
                self._lib.chaindp_index_destroy(h)
            self._indexes = []
            self._lib.chaindp_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ChainDPError(f"chaindp error {rc}: {self._lib.chaindp_last_error(self._ctx).decode()}")

    @staticmethod
    def _prep(off, anchors, n_segs):
        off = np.ascontiguousarray(off, np.int64)
        anchors = np.ascontiguousarray(anchors, np.uint64).reshape(-1, 2)
        if len(off) < 1 or off[0] != 0 or int(off[-1]) != anchors.shape[0]:
            raise ValueError("off must start at 0 and end at the number of anchors")
        ns = None if n_segs is None else np.ascontiguousarray(n_segs, np.int32)
        if ns is not None and len(ns) != len(off) - 1:
            raise ValueError("n_segs must have one entry per read")
        return off, anchors, ns

    # -- per-read chaining gaps (chaindp_set_read_gaps): read r's own (gap_ref, gap_qry) in the place of par.max_dist_x / max_dist_y
    def set_read_gaps(self, gap_ref, gap_qry):
        """gap_ref, gap_qry int32[n_reads] (params.read_gaps makes them): in force for every run on this context until
        clear_read_gaps(); a batch with another number of reads is refused meanwhile."""
        gr, gq = np.ascontiguousarray(gap_ref, np.int32), np.ascontiguousarray(gap_qry, np.int32)
        if gr.shape != gq.shape or gr.ndim != 1:
            raise ValueError("gap_ref and gap_qry need one entry per read each")
        if not len(gr):
            raise ValueError("no reads: clear_read_gaps() takes the gaps out of force")
        self._check(self._lib.chaindp_set_read_gaps(self._ctx, len(gr), _ptr(gr), _ptr(gq)))

    def clear_read_gaps(self):
        self._check(self._lib.chaindp_set_read_gaps(self._ctx, 0, None, None))

    @contextlib.contextmanager
    def _gaps(self, gaps):
        """What the `gaps=` keyword of the run and map calls does: gaps = (gap_ref, gap_qry) set for the call and cleared behind it,
        None: the call as it is."""
        if gaps is None:
            yield
            return
        self.set_read_gaps(*gaps)
        try:
            yield
        finally:
            self.clear_read_gaps()

    # -- host-buffer path
    def chain_batch(self, par, off, anchors, n_segs=None, want_v=True, gaps=None):
        """f, p, v (int32[total]) of every read of the batch; mm_chain_dp_fpga's arrays (chain.c:246-284).  gaps = (gap_ref, gap_qry)
        int32[n_reads]: every read chained with its own gaps instead of par's (here and in every call that takes `gaps`)."""
        off, anchors, ns = self._prep(off, anchors, n_segs)
        tot = anchors.shape[0]
        f, p = np.empty(tot, np.int32), np.empty(tot, np.int32)
        v = np.empty(tot, np.int32) if want_v else None
        with self._gaps(gaps):
            self._check(self._lib.chaindp_chain_batch(self._ctx, C.byref(par), len(off) - 1, _ptr(off), _ptr(anchors), _ptr(ns),
                                                      _ptr(f), _ptr(p), _ptr(v)))
        self._n_reads, self._total = len(off) - 1, tot
        return f, p, v

    def upload(self, off, anchors, n_segs=None):
        off, anchors, ns = self._prep(off, anchors, n_segs)
        self._check(self._lib.chaindp_upload(self._ctx, len(off) - 1, _ptr(off), _ptr(anchors), _ptr(ns)))
        self._n_reads, self._total = len(off) - 1, anchors.shape[0]

    def run(self, par, gaps=None):
        with self._gaps(gaps):
            self._check(self._lib.chaindp_run(self._ctx, C.byref(par)))

    def run_full(self, par, gaps=None):
        """run() + the compaction kernels, asynchronous, results stay in HBM (the benchmark's step)."""
        with self._gaps(gaps):
            self._check(self._lib.chaindp_run_full(self._ctx, C.byref(par)))

    def sync(self):
        self._check(self._lib.chaindp_sync(self._ctx))

    def download(self, want_v=True):
        f, p = np.empty(self._total, np.int32), np.empty(self._total, np.int32)
        v = np.empty(self._total, np.int32) if want_v else None
        self._check(self._lib.chaindp_download(self._ctx, _ptr(f), _ptr(p), _ptr(v)))
        return f, p, v

    def compact(self, par):
        """new_seed[] of every read (chain.c:286-317): (seeds_off int64[n_reads+1], seeds SEED_DTYPE[...])."""
        soff = np.zeros(self._n_reads + 1, np.int64)
        seeds = np.zeros(max(self._total, 1), SEED_DTYPE)
        self._check(self._lib.chaindp_compact(self._ctx, C.byref(par), _ptr(soff), _ptr(seeds)))
        return soff, seeds[:int(soff[-1])]

    def backtrack(self, par, min_cnt=3):
        """mm_chain_dp_bottom (chain.c:329-431) of every read on the GPU, after compact()/run_full():
        (chains_off, u uint64[...], b_off, b uint64[...,2])."""
        coff = np.zeros(self._n_reads + 1, np.int64)
        boff = np.zeros(self._n_reads + 1, np.int64)
        cap = max(self._total, 1)
        u = np.zeros(cap, np.uint64)
        b = np.zeros((cap, 2), np.uint64)
        self._check(self._lib.chaindp_backtrack(self._ctx, C.byref(par), min_cnt, _ptr(coff), _ptr(u), _ptr(boff), _ptr(b)))
        return coff, u[:int(coff[-1])], boff, b[:int(boff[-1])]

    # -- chains to hits (mm_gen_regs, hit.c:52-95; mm_est_err, esterr.c:30-64), after backtrack()
    def gen_regs(self, hash_, qlen, n_chains):
        """hash_ uint32[n_reads], qlen int32[n_reads] -> REG_DTYPE[n_chains] (n_chains = chains_off[-1] of backtrack())."""
        hash_ = np.ascontiguousarray(hash_, np.uint32)
        qlen = np.ascontiguousarray(qlen, np.int32)
        regs = np.zeros(max(int(n_chains), 1), REG_DTYPE)
        self._check(self._lib.chaindp_gen_regs(self._ctx, _ptr(hash_), _ptr(qlen), _ptr(regs)))
        return regs[:int(n_chains)]

    def est_err(self, regs_off, regs, qlen, ref_len, mini_pos_off=None, mini_pos=None):
        """mm_est_err on the hits `regs` (REG_DTYPE, read r owns regs_off[r]:regs_off[r+1]) -> (regs with div, n_match, n_tot).
        mini_pos_off / mini_pos None: the minimizer positions collect_seeds() left on the device."""
        regs_off, regs = _arr(regs_off, np.int64), _arr(regs, REG_DTYPE).copy()
        qlen, ref_len = _arr(qlen, np.int32), _arr(ref_len, np.int32)
        mt = np.zeros((max(len(regs), 1), 2), np.int32)
        mpo, mp = _arr(mini_pos_off, np.int64), _arr(mini_pos, np.uint64)
        self._check(self._lib.chaindp_est_err(self._ctx, _ptr(regs_off), _ptr0(regs), _ptr(qlen), _ptr0(ref_len), len(ref_len), _ptr(mpo), _ptr0(mp),
                                              _ptr(mt)))
        return regs, mt[:len(regs), 0].copy(), mt[:len(regs), 1].copy()

    # -- seed collection on the GPU (collect_seed_hits, map.c:187-236, over the FPGA index image)
    def load_index(self, img):
        """img: the four blobs B, H, V, P of the reference's index image (index.c:603-720) -> a handle for collect_seeds."""
        blobs = [np.ascontiguousarray(b, np.uint8) for b in img]
        h = self._lib.chaindp_index_create(self.device, *sum(([_ptr(b) if b.size else None, int(b.size)] for b in blobs), []))
        if not h:
            raise ChainDPError((self._lib.chaindp_last_error(None) or b"").decode())
        self._indexes.append(h)
        return h

    # -- the index image built on the device (chaindp_index_build): what replaces the reference's mm_idx_gen
    INDEX_ROUTE = ("sub_batches", "minimizers", "distinct", "buckets", "expanded", "max_keys", "passes_run", "passes_skipped")

    def build_index(self, w, k, is_hpc, seq, seq_off, rank=None, b=14):
        """Target sequences (bytes or uint8, concatenated; seq_off int64[n_seqs+1]) -> a handle like load_index's, the image built on the
        device in the reference's canonical form.  rank[n_seqs]: each sequence's rank by name (None: its number); b: bucket bits."""
        seq, seq_off = self._seqs(seq, seq_off)
        rk = None if rank is None else np.ascontiguousarray(rank, np.uint32)
        if rk is not None and len(rk) != len(seq_off) - 1:
            raise ChainDPError("rank needs one entry per sequence")
        h = self._lib.chaindp_index_build(self._ctx, int(w), int(k), int(b), int(bool(is_hpc)), len(seq_off) - 1, _ptr(seq_off),
                                          _ptr(seq) if len(seq) else None, None if rk is None or not len(rk) else _ptr(rk))
        if not h:
            self._check(self._lib.chaindp_index_build_status(self._ctx))
            raise ChainDPError("chaindp_index_build returned no index")
        self._indexes.append(h)
        return h

    def index_from_minimizers(self, b, mini, n_seqs=0, rank=None):
        """Test hook: the build behind the sketch, from minimizers uint64[n, 2] of the caller's."""
        mini = np.ascontiguousarray(mini, np.uint64).reshape(-1, 2)
        rk = None if rank is None else np.ascontiguousarray(rank, np.uint32)
        h = self._lib.chaindp_debug_index_from_minimizers(self._ctx, int(b), len(mini), _ptr(mini) if len(mini) else None,
                                                          int(n_seqs if rk is None else len(rk)), None if rk is None or not len(rk) else _ptr(rk))
        if not h:
            raise ChainDPError((self._lib.chaindp_last_error(self._ctx) or b"").decode())
        self._indexes.append(h)
        return h

    def set_index_chunk_bases(self, n=0):
        """Test hook: bases per sketch sub-batch of build_index (0: as many as a sketch takes)."""
        self._check(self._lib.chaindp_debug_index_chunk_bases(self._ctx, int(n)))

    def index_blobs(self, index):
        """[B, H, V, P] (uint8 arrays) of any index handle."""
        nb = (C.c_size_t * 4)()
        self._check(self._lib.chaindp_index_sizes(index, nb))
        blobs = [np.zeros(int(n), np.uint8) for n in nb]
        self._check(self._lib.chaindp_index_download(index, *[_ptr(x) if x.size else None for x in blobs]))
        return blobs

    def index_max_occ(self, index, f):
        """mm_idx_cal_max_occ(mi, f) of any index handle."""
        out = C.c_int32(0)
        self._check(self._lib.chaindp_index_cal_max_occ(index, float(f), C.byref(out)))
        return int(out.value)

    def index_route(self, index):
        """What the build of `index` did: a dict over INDEX_ROUTE."""
        out = np.zeros(8, np.int64)
        self._check(self._lib.chaindp_debug_index_route(index, _ptr(out)))
        return dict(zip(self.INDEX_ROUTE, out.tolist()))

    def index_stage_ms(self, index):
        """Milliseconds the build of `index` spent: (sketch sub-batches with their uploads, host clock; sort; grouping; tables -- device)."""
        ms = np.zeros(4, np.float64)
        self._check(self._lib.chaindp_debug_index_stage_ms(index, _ptr(ms)))
        return ms.tolist()

    def _minimizers(self, mini_off, mini, bid):
        """(mini_off, mini, n_reads, n_mini) of the caller's minimizers; mini_off = mini = None: of the ones the last sketch() left on
        the device, which go to the C side as two NULLs."""
        if mini_off is None and mini is None:
            return None, None, len(bid), self._sk_n_mini
        mini_off, mini = np.ascontiguousarray(mini_off, np.int64), np.ascontiguousarray(mini, np.uint64).reshape(-1, 2)
        return mini_off, mini, len(mini_off) - 1, len(mini)

    def collect_seeds(self, index, flag, max_occ, mini_off, mini, bid, qlen, n_segs=None):
        """Minimizers of a batch -> sorted anchors resident on the device (as after upload()).  Returns (off int64[n_reads+1],
        anchors uint64[n,2], rep_len int32[n_reads], mini_pos_off, mini_pos uint64[...]).  mini_off = mini = None: the minimizers the last
        sketch() left on the device (qlen = None then: the lengths it saw)."""
        mini_off, mini, n_reads, _ = self._minimizers(mini_off, mini, bid)
        bid, qlen, ns = _arr(bid, np.uint32), _arr(qlen, np.int32), _arr(n_segs, np.int32)
        off = np.zeros(n_reads + 1, np.int64); mpo = np.zeros(n_reads + 1, np.int64); rep = np.zeros(max(n_reads, 1), np.int32)
        self._check(self._lib.chaindp_collect_seeds(self._ctx, index, int(flag), int(max_occ), n_reads, _ptr(mini_off), _ptr(mini), _ptr(bid),
                                                    _ptr(qlen), _ptr(ns), _ptr(off), _ptr(rep), _ptr(mpo)))
        self._n_reads, self._total = n_reads, int(off[-1])
        a = np.zeros((max(self._total, 1), 2), np.uint64)
        self._check(self._lib.chaindp_download_anchors(self._ctx, _ptr(a)))
        mp = np.zeros(max(int(mpo[-1]), 1), np.uint64)
        self._check(self._lib.chaindp_download_mini_pos(self._ctx, _ptr(mp)))
        return off, a[:self._total], rep[:n_reads], mpo, mp[:int(mpo[-1])]

    # -- the calls that return hits: one path, what differs between them is the C call and their row of _CAPS
    def _hits(self, method, regs_cap, n_off, call, n_reads=None, again=(), **size):
        """Allocates the outputs, makes the C call -- call(off, regs, cap, rep_len, n_anchors) -> rc -- and deals with a buffer that was
        too small as the method's row of _CAPS says: (off int64[n_off + 1], regs REG_DTYPE[off[-1]], rep_len int32[n_reads], n_anchors).
        n_reads None: a post step on the resident batch (no rep_len, no n_anchors, _n_reads / _total stay).  again: the leading
        arguments of the row's retry call; size: the row's source where it is not _total."""
        row = _CAPS[method]
        source = self._total if row.source == "total" else size[row.source]
        cap = int(regs_cap) if regs_cap is not None else max(source // row.divisor, REGS_CAP_FLOOR if row.floored else 1)
        while True:
            off, regs, na = np.zeros(n_off + 1, np.int64), np.zeros(max(cap, 1), REG_DTYPE), C.c_int64(0)
            rep = None if n_reads is None else np.zeros(max(n_reads, 1), np.int32)
            rc = call(off, regs, cap, rep, na)
            if row.state == "before" and (rc in (0, -2) or na.value):        # a call refused at its entry left the resident batch as it was
                self._n_reads, self._total = n_reads, int(na.value)
            n = int(off[-1])
            short = rc == -2 and n > cap and row.retry is not None and (regs_cap is None or row.explicit == "retry")
            if not (short and row.retry == "again"):
                break
            cap = n                                                            # more hits than guessed: again with room for them
        if not short:
            self._check(rc)
        elif row.retry == "gen_regs":                                          # the hits are resident: fetch them
            regs = self.gen_regs(*again, n)
        else:                                                                  # run the post steps again with room for them
            off, regs = getattr(self, row.retry)(*again, regs_cap=n)
        if row.state == "after":
            self._n_reads, self._total = n_reads, int(na.value)
        return off, regs[:int(off[-1])], None if rep is None else rep[:n_reads], int(na.value)

    # -- the calls that return CIGARs: the same for their room, by their rows of _CAPS
    def _cigars(self, method, cigar_cap, alloc, call, names, **size):
        """alloc() -> the call's output arrays but the CIGARs, fresh ones, cigar_off last; call(*outputs, cigar pointer, cap) -> rc.
        cigar_cap None: the row's guess, and where the row says so the call again with the exact count when it was short.  A cap that
        stays short raises ChainDPError with the outputs attached under `names`.  Returns (*outputs, cigar uint32[cigar_off[-1]])."""
        row = _CAPS[method]
        cap = int(cigar_cap) if cigar_cap is not None else max(size[row.source] // row.divisor, REGS_CAP_FLOOR if row.floored else 1)
        while True:
            outs = alloc()
            off, cigar = outs[-1], np.zeros(max(cap, 1), np.uint32)
            rc = call(*outs, _ptr(cigar) if cap > 0 else None, max(cap, 0))
            short = rc == ERR_CAPACITY and int(off[-1]) > cap >= 0
            if not (short and cigar_cap is None and row.retry == "again"):
                break
            cap = int(off[-1])
        if short:
            err = ChainDPError(f"chaindp error {rc}: {self._lib.chaindp_last_error(self._ctx).decode()}")
            err.__dict__.update(zip(names, outs))
            raise err
        self._check(rc)
        return (*outs, cigar[:int(off[-1])])

    def map_batch(self, index, flag, max_occ, par, min_cnt, mini_off, mini, bid, qlen, hash_, regs_cap=None, gaps=None):
        """Minimizers in, hits out, everything in between resident (chaindp_map_batch): (regs_off int64[n_reads+1], regs REG_DTYPE[...],
        rep_len int32[n_reads], n_anchors)."""
        mini_off, mini = _arr(mini_off, np.int64), _arr(mini, np.uint64).reshape(-1, 2)
        n_reads = len(mini_off) - 1
        bid, qlen, hash_ = _arr(bid, np.uint32), _arr(qlen, np.int32), _arr(hash_, np.uint32)

        def call(roff, regs, cap, rep, na):
            return self._lib.chaindp_map_batch(self._ctx, index, int(flag), int(max_occ), C.byref(par), int(min_cnt), n_reads, _ptr(mini_off), _ptr(mini),
                                               _ptr(bid), _ptr(qlen), _ptr(hash_), _ptr(roff), _ptr(regs), cap, _ptr(rep), C.byref(na))
        with self._gaps(gaps):
            return self._hits("map_batch", regs_cap, n_reads, call, n_reads, again=(hash_, qlen), n_mini=len(mini))

    # -- chain_post + mm_est_err + mm_set_mapq (map.c:870-877, one segment, no alignment), after gen_regs() / map_batch()
    def chain_post(self, opt, ref_len, qlen=None, rep_len=None, mini_pos_off=None, mini_pos=None, regs_cap=None, want_anchors=False):
        """The final hits of every read (chaindp_chain_post) from the hits gen_regs() left on the device: (regs_off int64[n_reads+1],
        regs REG_DTYPE[...]) and, with want_anchors, (a_off int64[n_reads+1], a uint64[...,2]): the anchors as chain_post left them.
        qlen / rep_len / mini_pos None: the ones already on the device.  regs_cap None: room for every input hit (never fewer)."""
        ref_len, ql, rl = _arr(ref_len, np.int32), _arr(qlen, np.int32), _arr(rep_len, np.int32)
        mpo, mp = _arr(mini_pos_off, np.int64), _arr(mini_pos, np.uint64)
        aoff = np.zeros(self._n_reads + 1, np.int64) if want_anchors else None
        a = np.zeros((max(self._total, 1), 2), np.uint64) if want_anchors else None

        def call(roff, regs, cap, rep, na):
            return self._lib.chaindp_chain_post(self._ctx, C.byref(opt), _ptr(ql), _ptr(rl), _ptr0(ref_len), len(ref_len), _ptr(mpo), _ptr0(mp),
                                                _ptr(roff), _ptr(regs), cap, _ptr(aoff), _ptr(a))
        roff, regs, _, _ = self._hits("chain_post", regs_cap, self._n_reads, call)
        return (roff, regs, aoff, a[:int(aoff[-1])]) if want_anchors else (roff, regs)

    def map_reads(self, index, flag, max_occ, par, min_cnt, opt, mini_off, mini, bid, qlen, hash_, ref_len, regs_cap=None, gaps=None):
        """Minimizers in, final hits out (chaindp_map_reads): (regs_off int64[n_reads+1], regs REG_DTYPE[...], rep_len int32[n_reads],
        n_anchors).  regs_cap None: a guess from the minimizer count, retried with the exact count if the hits need more.
        mini_off = mini = None: the minimizers the last sketch() left on the device (qlen = None then: the lengths it saw)."""
        mini_off, mini, n_reads, n_mini = self._minimizers(mini_off, mini, bid)
        bid, qlen, hash_, ref_len = _arr(bid, np.uint32), _arr(qlen, np.int32), _arr(hash_, np.uint32), _arr(ref_len, np.int32)

        def call(roff, regs, cap, rep, na):
            return self._lib.chaindp_map_reads(self._ctx, index, int(flag), int(max_occ), C.byref(par), int(min_cnt), C.byref(opt), n_reads, _ptr(mini_off),
                                               _ptr(mini), _ptr(bid), _ptr(qlen), _ptr(hash_), _ptr0(ref_len), len(ref_len), _ptr(roff), _ptr(regs), cap,
                                               _ptr(rep), C.byref(na))
        with self._gaps(gaps):
            return self._hits("map_reads", regs_cap, n_reads, call, n_reads, again=(opt, ref_len), n_mini=n_mini)

    # -- sketch on the device: bases in, minimizers resident (chaindp_sketch)
    @staticmethod
    def _seqs(seq, seq_off):
        if isinstance(seq, (bytes, bytearray)):
            seq = np.frombuffer(seq, np.uint8)
        return np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(seq_off, np.int64)

    def sketch(self, w, k, is_hpc, seq, seq_off, n_segs=None):
        """mm_sketch of a batch of sequences (bytes or uint8, concatenated; seq_off int64[n_seqs+1]) -> mini_off int64[n_reads+1]; the
        minimizers stay on the device for collect_seeds / map_reads with mini_off = mini = None, download_minimizers() fetches them."""
        seq, seq_off = self._seqs(seq, seq_off)
        ns = None if n_segs is None else np.ascontiguousarray(n_segs, np.int32)
        n_reads = len(seq_off) - 1 if ns is None else len(ns)
        mini_off = np.zeros(n_reads + 1, np.int64)
        self._check(self._lib.chaindp_sketch(self._ctx, int(w), int(k), int(bool(is_hpc)), len(seq_off) - 1, _ptr(seq_off), _ptr(seq) if len(seq) else None,
                                             _ptr(ns), _ptr(mini_off)))
        self._sk_n_mini = int(mini_off[-1])
        return mini_off

    def download_minimizers(self):
        """uint64[n, 2] (x, y) of the last sketch()."""
        m = np.zeros((max(self._sk_n_mini, 1), 2), np.uint64)
        self._check(self._lib.chaindp_download_minimizers(self._ctx, _ptr(m)))
        return m[:self._sk_n_mini]

    def map_seqs(self, index, w, k, is_hpc, flag, max_occ, par, min_cnt, opt, seq, seq_off, bid, hash_, ref_len, regs_cap=None, gaps=None):
        """Bases in, final hits out (chaindp_map_seqs = sketch() + map_reads()): (regs_off, regs, rep_len, n_anchors)."""
        seq, seq_off = self._seqs(seq, seq_off)
        n_reads = len(seq_off) - 1
        bid, hash_, ref_len = _arr(bid, np.uint32), _arr(hash_, np.uint32), _arr(ref_len, np.int32)

        def call(roff, regs, cap, rep, na):
            return self._lib.chaindp_map_seqs(self._ctx, index, int(w), int(k), int(bool(is_hpc)), int(flag), int(max_occ), C.byref(par), int(min_cnt),
                                              C.byref(opt), n_reads, _ptr(seq_off), _ptr0(seq), _ptr(bid), _ptr(hash_), _ptr0(ref_len), len(ref_len),
                                              _ptr(roff), _ptr(regs), cap, _ptr(rep), C.byref(na))
        with self._gaps(gaps):
            return self._hits("map_seqs", regs_cap, n_reads, call, n_reads, again=(opt, ref_len), n_bases=len(seq))

    # -- reads of several segments (paired reads): chain_post with mm_select_sub_multi, mm_seg_gen, per-segment mm_set_parent / mm_set_mapq
    def frag_post(self, opt, ref_len, n_segs, seg_len=None, rep_len=None, mini_pos_off=None, mini_pos=None, regs_cap=None, want_anchors=False):
        """The final hits of every segment (chaindp_frag_post) from the hits gen_regs() left on the device: (seg_regs_off int64[n_seqs+1],
        regs REG_DTYPE[...]) and, with want_anchors, (seg_a_off int64[n_seqs+1], seg_a uint64[...,2]): every segment's anchors.  n_segs
        int32[n_reads]: the segments of every read (1..255), as the batch was chained; seg_len int32[n_seqs] (None: the lengths the last
        sketch() saw); rep_len / mini_pos None: the ones on the device.  regs_cap None: retried with the exact count if a guess is short."""
        ns = _arr(n_segs, np.int32)
        n_seqs = int(ns.sum())
        ref_len, sl, rl = _arr(ref_len, np.int32), _arr(seg_len, np.int32), _arr(rep_len, np.int32)
        mpo, mp = _arr(mini_pos_off, np.int64), _arr(mini_pos, np.uint64)
        aoff = np.zeros(n_seqs + 1, np.int64) if want_anchors else None
        a = np.zeros((max(self._total, 1), 2), np.uint64) if want_anchors else None

        def call(soff, regs, cap, rep, na):
            return self._lib.chaindp_frag_post(self._ctx, C.byref(opt), n_seqs, _ptr(ns), _ptr(sl), _ptr(rl), _ptr0(ref_len), len(ref_len), _ptr(mpo),
                                               _ptr0(mp), _ptr(soff), _ptr(regs), cap, _ptr(aoff), _ptr(a))
        soff, regs, _, _ = self._hits("frag_post", regs_cap, n_seqs, call)
        return (soff, regs, aoff, a[:int(aoff[-1])]) if want_anchors else (soff, regs)

    def map_frags(self, index, flag, max_occ, par, min_cnt, opt, mini_off, mini, bid, qlen, hash_, n_segs, seg_len, ref_len, regs_cap=None, gaps=None):
        """Minimizers in, per-segment final hits out (chaindp_map_frags): (seg_regs_off int64[n_seqs+1], regs REG_DTYPE[...], rep_len
        int32[n_reads], n_anchors).  mini_off = mini = None: the minimizers the last sketch() left on the device (qlen = seg_len = None
        then: the lengths it saw).  One `par` per call; reads of mixed lengths go in one call with gaps = params.read_gaps(...)."""
        ns = _arr(n_segs, np.int32)
        n_seqs = int(ns.sum())
        mini_off, mini, n_reads, n_mini = self._minimizers(mini_off, mini, bid)
        bid, qlen, hash_ = _arr(bid, np.uint32), _arr(qlen, np.int32), _arr(hash_, np.uint32)
        sl, ref_len = _arr(seg_len, np.int32), _arr(ref_len, np.int32)

        def call(soff, regs, cap, rep, na):
            return self._lib.chaindp_map_frags(self._ctx, index, int(flag), int(max_occ), C.byref(par), int(min_cnt), C.byref(opt), n_reads, _ptr(mini_off),
                                               _ptr(mini), _ptr(bid), _ptr(qlen), _ptr(hash_), n_seqs, _ptr(ns), _ptr(sl), _ptr0(ref_len), len(ref_len),
                                               _ptr(soff), _ptr(regs), cap, _ptr(rep), C.byref(na))
        with self._gaps(gaps):
            return self._hits("map_frags", regs_cap, n_seqs, call, n_reads, again=(opt, ref_len, ns, sl), n_mini=n_mini)

    def map_frag_seqs(self, index, w, k, is_hpc, flag, max_occ, par, min_cnt, opt, seq, seq_off, n_segs, bid, hash_, ref_len, pe_ori=-1, regs_cap=None,
                      gaps=None):
        """Bases in, per-segment final hits out (chaindp_map_frag_seqs = sketch(n_segs) + map_frags()): (seg_regs_off, regs, rep_len,
        n_anchors).  pe_ori 0..3: a pair's segments are reverse-complemented on the device before the sketch and their hits flipped back
        afterwards, as the reference's worker_for does (map.c:608-631); -1 leaves the reads alone."""
        seq, seq_off = self._seqs(seq, seq_off)
        ns = _arr(n_segs, np.int32)
        n_reads, n_seqs = len(ns), len(seq_off) - 1
        bid, hash_, ref_len = _arr(bid, np.uint32), _arr(hash_, np.uint32), _arr(ref_len, np.int32)

        def call(soff, regs, cap, rep, na):
            return self._lib.chaindp_map_frag_seqs(self._ctx, index, int(w), int(k), int(bool(is_hpc)), int(flag), int(max_occ), C.byref(par), int(min_cnt),
                                                   C.byref(opt), int(pe_ori), n_reads, n_seqs, _ptr(ns), _ptr(seq_off), _ptr0(seq), _ptr(bid), _ptr(hash_),
                                                   _ptr0(ref_len), len(ref_len), _ptr(soff), _ptr(regs), cap, _ptr(rep), C.byref(na))
        with self._gaps(gaps):
            return self._hits("map_frag_seqs", regs_cap, n_seqs, call, n_reads, n_bases=len(seq))

    # -- base-level alignment: ksw_extd2_sse for a batch of problems (chaindp_ksw_extd)
    def ksw_extd(self, bases, q_beg, q_len, t_beg, t_len, scoring, w, zdrop, end_bonus, flag, cigar_cap=None):
        """Problem i aligns bases[q_beg[i] : q_beg[i] + q_len[i]] (query) to bases[t_beg[i] : t_beg[i] + t_len[i]] (target); bases uint8, codes
        0..4.  scoring = (a, b, q, e, q2, e2) for the whole call; w, zdrop, end_bonus, flag per problem (a scalar serves all of them).
        Returns (ez int32[n, 10] with the columns KSW_EZ_FIELDS, cigar_off int64[n + 1], cigar uint32[cigar_off[-1]]).  cigar_cap=None
        makes room for sum(q_len + t_len) words, which no batch exceeds; with a cap that is too small the call raises ChainDPError and
        err.ez / err.cigar_off hold what the C call filled in (cigar_off[-1] words are enough)."""
        bases = np.ascontiguousarray(bases, np.uint8)
        q_beg, t_beg = np.ascontiguousarray(q_beg, np.int64), np.ascontiguousarray(t_beg, np.int64)
        q_len, t_len = np.ascontiguousarray(q_len, np.int32), np.ascontiguousarray(t_len, np.int32)
        n = len(q_beg)
        if not (q_beg.shape == q_len.shape == t_beg.shape == t_len.shape == (n,)):
            raise ValueError("q_beg, q_len, t_beg, t_len need one entry per problem each")
        per = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (n,))) for v in (w, zdrop, end_bonus, flag)]
        if n and (int((q_beg + q_len).max()) > len(bases) or int((t_beg + t_len).max()) > len(bases)):
            raise ValueError("a problem reaches past the end of bases")
        a, b, q, e, q2, e2 = (int(v) for v in scoring)

        def call(ez, off, cigar, cap):
            return self._lib.chaindp_ksw_extd(self._ctx, n, _ptr0(bases), _ptr(q_beg), _ptr(q_len), _ptr(t_beg), _ptr(t_len), a, b, q, e, q2, e2,
                                              *[_ptr(v) for v in per], _ptr(ez), _ptr(off), cigar, cap)
        return self._cigars("ksw_extd", cigar_cap, lambda: (np.zeros((n, 10), np.int32), np.zeros(n + 1, np.int64)), call, ("ez", "cigar_off"),
                            n_span=int(q_len.astype(np.int64).sum() + t_len.astype(np.int64).sum()))

    # -- base-level alignment of regions: mm_align1 around that DP (chaindp_align1)
    def align_set_targets(self, seq_off, seq):
        """The target sequences as characters (seq_off int64[n + 1], seq bytes / uint8), encoded on the device and kept resident until
        the next call or align_clear_targets()."""
        seq, seq_off = self._seqs(seq, seq_off)
        if len(seq_off) < 1 or int(seq_off[-1]) != len(seq):
            raise ValueError("seq_off must end at the number of bases")
        self._check(self._lib.chaindp_align_set_targets(self._ctx, len(seq_off) - 1, _ptr(seq_off), _ptr0(seq)))

    def align_clear_targets(self):
        self._check(self._lib.chaindp_align_clear_targets(self._ctx))

    def align1(self, opt, seq_off, seq, a_off, a, regs_off, regs, regs2=None, cigar_cap=None):
        """mm_align1 for every region of every read (chaindp_align1): opt a params.AlignOpt; seq the reads' bases as characters; a uint64[n, 2]
        each read's anchors after mm_squeeze_a; regs REG_DTYPE, `as` relative to the read's first anchor.  Nothing is changed in place.
        Returns (a, regs, regs2, extra ALIGN_EXTRA_DTYPE[n_regions], cigar_off int64[n_regions + 1], cigar uint32[...]): the anchors with
        their MM_SEED_IGNORE marks, the updated regions, what was split off (cnt 0 where nothing was; regs2 given: its other fields stay).
        cigar_cap None: a guess, and the call again with the exact count where it was short (the _CAPS row); with a cap of the caller's
        that is too small the call raises ChainDPError and err.a / .regs / .regs2 / .extra / .cigar_off hold what the C call filled in."""
        (seq, seq_off), a_off, regs_off = self._seqs(seq, seq_off), _arr(a_off, np.int64), _arr(regs_off, np.int64)
        a_in, regs_in = _arr(a, np.uint64).reshape(-1, 2), _arr(regs, REG_DTYPE)
        n_reads, n_regs = len(seq_off) - 1, len(regs_in)
        if len(a_off) != n_reads + 1 or len(regs_off) != n_reads + 1 or int(a_off[-1]) != len(a_in) or int(regs_off[-1]) != n_regs or int(seq_off[-1]) != len(seq):
            raise ValueError("seq_off, a_off and regs_off need one entry per read and one more, and must end at the sizes of seq, a and regs")

        def alloc():
            r2 = np.zeros(n_regs, REG_DTYPE) if regs2 is None else _arr(regs2, REG_DTYPE).copy()
            return a_in.copy(), regs_in.copy(), r2, np.zeros(n_regs, ALIGN_EXTRA_DTYPE), np.zeros(n_regs + 1, np.int64)

        def call(a_out, regs_out, r2, extra, off, cigar, cap):
            return self._lib.chaindp_align1(self._ctx, C.byref(opt), n_reads, _ptr(seq_off), _ptr0(seq), _ptr(a_off), _ptr0(a_out), _ptr(regs_off),
                                            _ptr0(regs_out), _ptr0(r2), _ptr0(extra), _ptr(off), cigar, cap)
        return self._cigars("align1", cigar_cap, alloc, call, ("a", "regs", "regs2", "extra", "cigar_off"), n_bases=len(seq))

    def align1_inv(self, opt, seq_off, seq, regs_off, regs, cigar_cap=None):
        """mm_align1_inv for every pair of neighbouring regions of every read (chaindp_align1_inv), after all align1 rounds: regs REG_DTYPE in
        mm_align_skeleton's order, what regs2 split off inserted behind its region, no inversion records among them.  Slot g (region i >= 1
        of its read) is the pair (i - 1, i).  Returns (made int32[n_regions], r_inv REG_DTYPE[n_regions], extra ALIGN_EXTRA_DTYPE[n_regions],
        cigar_off int64[n_regions + 1], cigar uint32[...]); made: 0 no test, 1 made, 2 below min_dp_max, 3 not tested because the pair before
        it was made, 4 no CIGAR.  cigar_cap as align1's; a cap of the caller's that is too small raises ChainDPError with err.made /
        .r_inv / .extra / .cigar_off holding what the C call filled in."""
        (seq, seq_off), regs_off = self._seqs(seq, seq_off), _arr(regs_off, np.int64)
        regs_in = _arr(regs, REG_DTYPE)
        n_reads, n_regs = len(seq_off) - 1, len(regs_in)
        if len(regs_off) != n_reads + 1 or int(regs_off[-1]) != n_regs or int(seq_off[-1]) != len(seq):
            raise ValueError("seq_off and regs_off need one entry per read and one more, and must end at the sizes of seq and regs")

        def alloc():
            return np.zeros(n_regs, np.int32), np.zeros(n_regs, REG_DTYPE), np.zeros(n_regs, ALIGN_EXTRA_DTYPE), np.zeros(n_regs + 1, np.int64)

        def call(made, r_inv, extra, off, cigar, cap):
            return self._lib.chaindp_align1_inv(self._ctx, C.byref(opt), n_reads, _ptr(seq_off), _ptr0(seq), _ptr(regs_off), _ptr0(regs_in), _ptr0(made),
                                                _ptr0(r_inv), _ptr0(extra), _ptr(off), cigar, cap)
        return self._cigars("align1_inv", cigar_cap, alloc, call, ("made", "r_inv", "extra", "cigar_off"), n_bases=len(seq))

    # -- whole reads: mm_align_skeleton's loop around the two stages (chaindp_align_reads)
    def align_reads(self, opt, seq_off, seq, a_off, a, regs_off, regs, regs_cap=None, cigar_cap=None):
        """mm_align_skeleton for every read (chaindp_align_reads): the inputs of align1; every round of align1, the inversions, mm_filter_regs
        and mm_hit_sort_by_dp happen in the one call, bases, anchors and CIGAR words staying on the device between the rounds.  Nothing is
        changed in place.  Returns (a, regs_off int64[n_reads + 1], regs REG_DTYPE[...], extra ALIGN_EXTRA_DTYPE[...], cigar_off
        int64[len(regs) + 1], cigar uint32[...]): the anchors with their MM_SEED_IGNORE marks and each read's final regions in
        mm_hit_sort_by_dp's order with their CIGARs.  regs_cap / cigar_cap None: a guess, and where it was short the resident result
        fetched with the exact room (the _CAPS rows); a cap of the caller's that is too small raises ChainDPError and err.a / .regs_off /
        .need hold what the C call filled in (need: final regions, CIGAR words)."""
        (seq, seq_off), a_off, regs_off = self._seqs(seq, seq_off), _arr(a_off, np.int64), _arr(regs_off, np.int64)
        a_out, regs_in = _arr(a, np.uint64).reshape(-1, 2).copy(), _arr(regs, REG_DTYPE)
        n_reads, n_regs = len(seq_off) - 1, len(regs_in)
        if len(a_off) != n_reads + 1 or len(regs_off) != n_reads + 1 or int(a_off[-1]) != len(a_out) or int(regs_off[-1]) != n_regs or int(seq_off[-1]) != len(seq):
            raise ValueError("seq_off, a_off and regs_off need one entry per read and one more, and must end at the sizes of seq, a and regs")
        size = dict(n_regs2=2 * n_regs, n_bases=len(seq))
        given = (regs_cap, cigar_cap)
        caps = [int(c) if c is not None else max(size[row.source] // row.divisor, REGS_CAP_FLOOR if row.floored else 1)
                for c, row in zip(given, (_CAPS["align_reads"], _CAPS["align_reads_cigar"]))]
        out_off, need = np.zeros(n_reads + 1, np.int64), np.zeros(2, np.int64)

        def outputs():
            return (np.zeros(max(caps[0], 1), REG_DTYPE), np.zeros(max(caps[0], 1), ALIGN_EXTRA_DTYPE), np.zeros(max(caps[0], 0) + 1, np.int64),
                    np.zeros(max(caps[1], 1), np.uint32))

        def room(o):
            return _ptr(out_off), _ptr(o[0]), _ptr(o[1]), caps[0], _ptr(o[2]), _ptr(o[3]), caps[1], _ptr(need)
        o = outputs()
        rc = self._lib.chaindp_align_reads(self._ctx, C.byref(opt), n_reads, _ptr(seq_off), _ptr0(seq), _ptr(a_off), _ptr0(a_out), _ptr(regs_off),
                                           _ptr0(regs_in), *room(o))
        if rc == 0 or (rc == ERR_CAPACITY and (int(need[0]) > caps[0] or int(need[1]) > caps[1])):   # a result is resident: a call refused
            # at its entry leaves the one before, one that ran out of device memory leaves none and says nothing of need
            self._align_reads_n = n_reads
        if rc == ERR_CAPACITY and (int(need[0]) > caps[0] or int(need[1]) > caps[1]):
            if any(c is not None and int(n) > cap for c, n, cap in zip(given, need, caps)):
                err = ChainDPError(f"chaindp error {rc}: {self._lib.chaindp_last_error(self._ctx).decode()}")
                err.__dict__.update(a=a_out, regs_off=out_off, need=need)
                raise err
            caps = [max(cap, int(n)) for cap, n in zip(caps, need)]
            o = outputs()
            rc = getattr(self._lib, "chaindp_" + _CAPS["align_reads"].retry)(self._ctx, n_reads, *room(o))
        self._check(rc)
        n, m = int(need[0]), int(need[1])
        return a_out, out_off, o[0][:n], o[1][:n], o[2][:n + 1], o[3][:m]

    # -- aligned reads finished: the tail of align_regs and mm_set_mapq (chaindp_align_post and its siblings)
    def _finished(self, rows, given, size, n_reads, call, attach):
        """The room logic of the calls that return finished regions, by their two rows of _CAPS (regions, CIGAR words), as _cigars does it
        for one kind of room: call(*room) -> rc with room = (out_off, regs, extra, dp_max2, regs_cap, cigar_off, cigar, cigar_cap, need).
        A guess that was short is made good by the rows' fetch call; a cap of the caller's that is short raises ChainDPError with
        `attach` and regs_off, need attached.  Returns (regs_off, regs, extra, dp_max2, cigar_off, cigar)."""
        rows = [_CAPS[r] for r in rows]
        caps = [int(c) if c is not None else max(size[row.source] // row.divisor, REGS_CAP_FLOOR if row.floored else 1) for c, row in zip(given, rows)]
        out_off, need = np.zeros(n_reads + 1, np.int64), np.zeros(2, np.int64)

        def outputs():
            return (np.zeros(max(caps[0], 1), REG_DTYPE), np.zeros(max(caps[0], 1), ALIGN_EXTRA_DTYPE), np.zeros(max(caps[0], 1), np.int32),
                    np.zeros(max(caps[0], 0) + 1, np.int64), np.zeros(max(caps[1], 1), np.uint32))

        def room(o):
            return _ptr(out_off), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), caps[0], _ptr(o[3]), _ptr(o[4]), caps[1], _ptr(need)
        o = outputs()
        rc = call(*room(o))
        short = rc == ERR_CAPACITY and (int(need[0]) > caps[0] or int(need[1]) > caps[1])   # else out of device memory, or a logf argument
        if short:
            if any(c is not None and int(n) > cap for c, n, cap in zip(given, need, caps)):
                err = ChainDPError(f"chaindp error {rc}: {self._lib.chaindp_last_error(self._ctx).decode()}")
                err.__dict__.update(attach, regs_off=out_off, need=need)
                raise err
            caps = [max(cap, int(n)) for cap, n in zip(caps, need)]
            o = outputs()
            rc = getattr(self._lib, "chaindp_" + rows[0].retry)(self._ctx, n_reads, *room(o))
        self._check(rc)
        n, m = int(need[0]), int(need[1])
        return out_off, o[0][:n], o[1][:n], o[2][:n], o[3][:n + 1], o[4][:m]

    def align_post(self, opt, rep_len, regs_off=None, regs=None, extra=None, cigar_off=None, cigar=None, regs_cap=None, cigar_cap=None):
        """What the reference does with aligned regions before it prints them (chaindp_align_post / chaindp_align_post_regs): mm_set_parent
        with r->p, mm_select_sub, mm_set_sam_pri (unless MM_F_ALL_CHAINS), then mm_set_mapq with mm_set_inv_mapq.  opt: params.PostOpt;
        rep_len int32[n_reads].  regs_off None: on the resident result of the last align_reads, which stays valid; else on the regions
        given, in the form align_reads returns them (a region with has_extra == 0 takes the r->p == NULL branches).  Returns (regs_off
        int64[n_reads + 1], regs REG_DTYPE[...], extra ALIGN_EXTRA_DTYPE[...], dp_max2 int32[...], cigar_off int64[len(regs) + 1], cigar
        uint32[...]).  regs_cap / cigar_cap as in align_reads; a short cap of the caller's raises with err.regs_off / .need."""
        rep_len = _arr(rep_len, np.int32)
        n_reads = len(rep_len)
        if regs_off is None:
            if any(x is not None for x in (regs, extra, cigar_off, cigar)):
                raise ValueError("regs, extra, cigar_off and cigar go with regs_off")
            size = dict(n_regs=0, n_words=0)

            def call(*room):
                return self._lib.chaindp_align_post(self._ctx, C.byref(opt), n_reads, _ptr0(rep_len), *room)
        else:
            regs_off, regs_in, extra_in = _arr(regs_off, np.int64), _arr(regs, REG_DTYPE), _arr(extra, ALIGN_EXTRA_DTYPE)
            coff, cig = _arr(cigar_off, np.int64), _arr(cigar, np.uint32)
            if len(regs_off) != n_reads + 1 or len(extra_in) != len(regs_in) or len(coff) != len(regs_in) + 1:
                raise ValueError("regs_off needs one entry per read and one more, extra one per region, cigar_off one per region and one more")
            size = dict(n_regs=len(regs_in), n_words=len(cig))

            def call(*room):
                return self._lib.chaindp_align_post_regs(self._ctx, C.byref(opt), n_reads, _ptr0(rep_len), _ptr(regs_off), _ptr0(regs_in), _ptr0(extra_in),
                                                         _ptr(coff), _ptr0(cig), *room)
        return self._finished(("align_post", "align_post_cigar"), (regs_cap, cigar_cap), size, n_reads, call, {})

    def align_reads_post(self, aopt, opt, seq_off, seq, a_off, a, regs_off, regs, rep_len, regs_cap=None, cigar_cap=None):
        """align_reads and align_post in one call (chaindp_align_reads_post): only the finished result comes down.  Returns (a, regs_off,
        regs, extra, dp_max2, cigar_off, cigar); both results are resident afterwards."""
        (seq, seq_off), a_off, regs_off = self._seqs(seq, seq_off), _arr(a_off, np.int64), _arr(regs_off, np.int64)
        a_out, regs_in, rep_len = _arr(a, np.uint64).reshape(-1, 2).copy(), _arr(regs, REG_DTYPE), _arr(rep_len, np.int32)
        n_reads, n_regs = len(seq_off) - 1, len(regs_in)
        if len(a_off) != n_reads + 1 or len(regs_off) != n_reads + 1 or int(a_off[-1]) != len(a_out) or int(regs_off[-1]) != n_regs or int(seq_off[-1]) != len(seq) \
                or len(rep_len) != n_reads:
            raise ValueError("seq_off, a_off and regs_off need one entry per read and one more, rep_len one per read, and the offsets must end at the sizes of seq, a and regs")

        def call(*room):
            rc = self._lib.chaindp_align_reads_post(self._ctx, C.byref(aopt), C.byref(opt), n_reads, _ptr(seq_off), _ptr0(seq), _ptr(a_off), _ptr0(a_out),
                                                    _ptr(regs_off), _ptr0(regs_in), _ptr0(rep_len), *room)
            if rc in (0, ERR_CAPACITY):
                self._align_reads_n = n_reads
            return rc
        return (a_out, *self._finished(("align_reads_post", "align_reads_post_cigar"), (regs_cap, cigar_cap), dict(n_regs2=2 * n_regs, n_bases=len(seq)), n_reads,
                                       call, dict(a=a_out)))

    # -- mapping with base alignment: chain_post's result handed to the alignment stages on the device (chaindp_map_align.h)
    def _resident_anchors(self, n_reads):
        """(a_off int64[n_reads + 1], a uint64[..., 2]): the squeezed anchors of the last align_resident / map_align_seqs with their marks."""
        a_off = np.zeros(n_reads + 1, np.int64)
        rc = self._lib.chaindp_align_resident_anchors(self._ctx, n_reads, _ptr(a_off), None, 0)
        if rc != ERR_CAPACITY:
            self._check(rc)
        a = np.zeros((max(int(a_off[-1]), 1), 2), np.uint64)
        self._check(self._lib.chaindp_align_resident_anchors(self._ctx, n_reads, _ptr(a_off), _ptr(a), len(a)))
        return a_off, a[:int(a_off[-1])]

    def align_resident(self, aopt, opt, regs_cap=None, cigar_cap=None, want_anchors=False):
        """The rest of a read's path after chain_post(opt with MM_F_CIGAR) / map_reads / map_seqs on this batch, on the device
        (chaindp_align_resident): the hand-off (mm_squeeze_a), align_reads and align_post on the resident bases of the batch's sketch(),
        its resident rep_len and the targets of align_set_targets().  Returns (regs_off, regs, extra, dp_max2, cigar_off, cigar) as
        align_post does and, with want_anchors, (a_off int64[n_reads + 1], a uint64[..., 2]) behind them: the squeezed anchors with the
        marks of the alignment.  regs_cap / cigar_cap as in align_reads; a short cap of the caller's raises with err.regs_off / .need."""
        n_reads = self._n_reads
        # the anchors come with the call itself: the chain anchors are some of the batch's, whose number the host knows
        a_off = np.zeros(n_reads + 1, np.int64) if want_anchors else None
        a = np.zeros((max(self._total, 1), 2), np.uint64) if want_anchors else None

        def call(*room):
            rc = self._lib.chaindp_align_resident(self._ctx, C.byref(aopt), C.byref(opt), n_reads, *room, _ptr(a_off), _ptr(a))
            if rc in (0, ERR_CAPACITY):
                self._align_reads_n = n_reads
            return rc
        out = self._finished(("align_resident", "align_resident_cigar"), (regs_cap, cigar_cap), dict(n_reads2=2 * n_reads, total=self._total), n_reads, call, {})
        return (*out, a_off, a[:int(a_off[-1])]) if want_anchors else out

    def map_align_seqs(self, index, w, k, is_hpc, flag, max_occ, par, min_cnt, opt, aopt, seq, seq_off, bid, hash_, ref_len, regs_cap=None, cigar_cap=None,
                       want_anchors=False, gaps=None):
        """Bases in, the final hits of a run with MM_F_CIGAR and their CIGARs out (chaindp_map_align_seqs = map_seqs() with opt.flag |
        MM_F_CIGAR + align_resident()): (regs_off, regs, extra, dp_max2, cigar_off, cigar, rep_len int32[n_reads], n_anchors) and, with
        want_anchors, (a_off, a) behind them.  The targets must have been set with align_set_targets()."""
        seq, seq_off = self._seqs(seq, seq_off)
        n_reads = len(seq_off) - 1
        bid, hash_, ref_len = _arr(bid, np.uint32), _arr(hash_, np.uint32), _arr(ref_len, np.int32)
        rep, na = np.zeros(max(n_reads, 1), np.int32), C.c_int64(0)

        def call(*room):
            rc = self._lib.chaindp_map_align_seqs(self._ctx, index, int(w), int(k), int(bool(is_hpc)), int(flag), int(max_occ), C.byref(par), int(min_cnt),
                                                  C.byref(opt), C.byref(aopt), n_reads, _ptr(seq_off), _ptr0(seq), _ptr(bid), _ptr(hash_), _ptr0(ref_len),
                                                  len(ref_len), *room, None, None, _ptr(rep), C.byref(na))
            if rc in (0, ERR_CAPACITY) or na.value:                           # a call refused at its entry left the resident batch as it was
                self._n_reads, self._total = n_reads, int(na.value)
            if rc in (0, ERR_CAPACITY):
                self._align_reads_n = n_reads
            return rc
        with self._gaps(gaps):
            out = self._finished(("map_align_seqs", "map_align_seqs_cigar"), (regs_cap, cigar_cap), dict(n_bases=len(seq)), n_reads, call, {})
        out = (*out, rep[:n_reads], int(na.value))
        return (*out, *self._resident_anchors(n_reads)) if want_anchors else out

    def map_align_handoff(self):
        """The regions as the hand-off of the last align_resident / map_align_seqs left them, before any alignment (test hook): (regs_off
        int64[n_reads + 1], regs REG_DTYPE[...] with `as` into the squeezed anchors, a_off int64[n_reads + 1])."""
        n_reads = self._n_reads
        roff, aoff = np.zeros(n_reads + 1, np.int64), np.zeros(n_reads + 1, np.int64)
        rc = self._lib.chaindp_map_align_debug_handoff(self._ctx, n_reads, _ptr(roff), None, 0, _ptr(aoff))
        if rc != ERR_CAPACITY:
            self._check(rc)
        regs = np.zeros(max(int(roff[-1]), 1), REG_DTYPE)
        self._check(self._lib.chaindp_map_align_debug_handoff(self._ctx, n_reads, _ptr(roff), _ptr(regs), len(regs), _ptr(aoff)))
        return roff, regs[:int(roff[-1])], aoff

    def map_align_run_handoff(self, regs_off, regs, b_off, b):
        """The hand-off alone on regions and anchors from the host, in the form chain_post(want_anchors=True) returns them (test hook):
        (regs REG_DTYPE[...] with their new `as`, a_off int64[n_reads + 1], a uint64[..., 2])."""
        regs_off, regs, b_off, b = _arr(regs_off, np.int64), _arr(regs, REG_DTYPE), _arr(b_off, np.int64), _arr(b, np.uint64).reshape(-1, 2)
        if len(regs_off) != len(b_off) or int(regs_off[-1]) != len(regs) or int(b_off[-1]) != len(b):
            raise ValueError("regs_off and b_off need one entry per read and one more and must end at the sizes of regs and b")
        out, a_off, a = np.zeros(max(len(regs), 1), REG_DTYPE), np.zeros(len(regs_off), np.int64), np.zeros((max(len(b), 1), 2), np.uint64)
        self._check(self._lib.chaindp_map_align_debug_run_handoff(self._ctx, len(regs_off) - 1, _ptr(regs_off), _ptr0(regs), _ptr(b_off), _ptr0(b), _ptr(out),
                                                                 _ptr(a_off), _ptr(a)))
        return out[:len(regs)], a_off, a[:int(a_off[-1])]

    def map_align_ms(self):
        """Device milliseconds of the last align_resident / map_align_seqs made while profiling was on (tuning hook): dict of handoff,
        then align_reads_ms()'s rounds, inv, finish, gather and align_post_ms()'s read, post_gather."""
        ms = (C.c_double * 7)()
        self._check(self._lib.chaindp_map_align_debug_ms(self._ctx, ms))
        return dict(zip(("handoff", "rounds", "inv", "finish", "gather", "read", "post_gather"), (float(x) for x in ms)))

    def map_align_set_lds_cap(self, cap=0):
        """Test hook: later hand-offs rank lists of up to `cap` regions in LDS and longer ones in global memory; 0: the built-in cap,
        which is returned."""
        out = np.zeros(1, np.int32)
        self._check(self._lib.chaindp_map_align_debug_set_lds_cap(self._ctx, int(cap), _ptr(out)))
        return int(out[0])

    def align_post_ms(self):
        """Device milliseconds of the last align_post / align_reads_post made while profiling was on (tuning hook): dict of read (the one
        kernel of the tail and mapq, with the scans) and gather."""
        ms = (C.c_double * 2)()
        self._check(self._lib.chaindp_align_post_debug_ms(self._ctx, ms))
        return dict(zip(("read", "gather"), (float(x) for x in ms)))

    def align_post_set_lds_cap(self, cap=0):
        """Test hook: later align_post calls stage lists of up to `cap` regions in LDS and longer ones in global memory; 0: the built-in
        cap, which is returned."""
        out = np.zeros(1, np.int32)
        self._check(self._lib.chaindp_align_post_debug_set_lds_cap(self._ctx, int(cap), _ptr(out)))
        return int(out[0])

    def apost_logf_selftest(self, match_sc, kmax=1 << 24):
        """The number of dp_max in [1, kmax] where the device's logf((float)dp_max / match_sc) differs from the host's (test hook)."""
        n = int(self._lib.chaindp_apost_logf_selftest(self._ctx, int(match_sc), int(kmax)))
        if n < 0:
            self._check(n)
        return n

    def align_reads_placed(self):
        """Each read's list of the last align_reads as it stood ahead of mm_filter_regs, split-off regions and inversions in their places
        (test hook): (placed_off int64[n_reads + 1], placed REG_DTYPE[...])."""
        n_reads = getattr(self, "_align_reads_n", 0)             # the reads of the last align_reads; the C side refuses any other count
        off = np.zeros(n_reads + 1, np.int64)
        rc = self._lib.chaindp_align_reads_debug_placed(self._ctx, n_reads, _ptr(off), None, 0)
        if rc != ERR_CAPACITY:
            self._check(rc)
        placed = np.zeros(max(int(off[-1]), 1), REG_DTYPE)
        self._check(self._lib.chaindp_align_reads_debug_placed(self._ctx, n_reads, _ptr(off), _ptr(placed), len(placed)))
        return off, placed[:int(off[-1])]

    def align_reads_rounds(self):
        """The regions of every round of align1 the last align_reads made (test hook): int64[rounds]."""
        n = np.zeros(1, np.int64)
        self._check(self._lib.chaindp_align_reads_debug_rounds(self._ctx, _ptr(n), 1))
        out = np.zeros(int(n[0]) + 1, np.int64)
        self._check(self._lib.chaindp_align_reads_debug_rounds(self._ctx, _ptr(out), len(out)))
        return out[1:]

    def align_reads_ms(self):
        """Device milliseconds of the last align_reads made while profiling was on (tuning hook): dict of rounds, inv, finish, gather."""
        ms = (C.c_double * 4)()
        self._check(self._lib.chaindp_align_reads_debug_ms(self._ctx, ms))
        return dict(zip(("rounds", "inv", "finish", "gather"), (float(x) for x in ms)))

    def align_reads_set_lds_cap(self, cap=0):
        """Test hook: later align_reads calls rank lists of up to `cap` records in LDS and longer ones in global memory; 0: the built-in
        cap, which is returned."""
        out = np.zeros(1, np.int32)
        self._check(self._lib.chaindp_align_reads_debug_set_lds_cap(self._ctx, int(cap), _ptr(out)))
        return int(out[0])

    def align_inv_ll(self, n):
        """score, qe, te of ksw_ll_i16 for the n candidate pairs of the last align1_inv, on the reversed stretches (test hook): int32[n, 3]."""
        out = np.zeros((max(int(n), 1), 3), np.int32)
        self._check(self._lib.chaindp_align_inv_debug_ll(self._ctx, int(n), _ptr(out)))
        return out[:int(n)]

    def align_inv_ms(self):
        """Device milliseconds of the last align1_inv made while profiling was on (tuning hook): dict of ll, dp, finish, pack."""
        ms = (C.c_double * 4)()
        self._check(self._lib.chaindp_align_inv_debug_ms(self._ctx, ms))
        return dict(zip(("ll", "dp", "finish", "pack"), (float(x) for x in ms)))

    def align_ms(self):
        """Device milliseconds of the last align1 made while profiling was on (tuning hook): dict of plan, dp, zdrop, stitch, extra."""
        ms = (C.c_double * 5)()
        self._check(self._lib.chaindp_align_debug_ms(self._ctx, ms))
        return dict(zip(("plan", "dp", "zdrop", "stitch", "extra"), (float(x) for x in ms)))

    def ksw_route(self, n):
        """The route each of the n problems of the last ksw_extd took, as the device reported it (test hook): 0 the reference's early
        return, 1 state in LDS, 2 state in global scratch, 3 state in LDS and several waves."""
        route = np.zeros(max(int(n), 1), np.int32)
        self._check(self._lib.chaindp_ksw_debug_route(self._ctx, int(n), _ptr(route)))
        return route[:int(n)]

    def ksw_set_grid_cap(self, cap=0):
        """Test hook: every later DP plan (ksw_extd, align1, align1_inv) launches at most `cap` workgroups of either kind; 0: the plan's own."""
        self._check(self._lib.chaindp_ksw_debug_set_grid_cap(self._ctx, int(cap)))

    def ksw_launch(self):
        """The last DP plan of this context (test hook): dict of count, grid, lds_bytes, path_stride, each a pair (the one-wave launch,
        the several-wave launch)."""
        out = (C.c_int64 * 8)()
        self._check(self._lib.chaindp_ksw_debug_launch(self._ctx, out))
        return {k: (int(out[2 * i]), int(out[2 * i + 1])) for i, k in enumerate(("count", "grid", "lds_bytes", "path_stride"))}

    def ksw_ms(self):
        """Device milliseconds of the DP kernel in the last ksw_extd made while profiling was on (tuning hook); -1 before."""
        return float(self._lib.chaindp_ksw_debug_ms(self._ctx))

    def set_frag_lds_cap(self, cap=64):
        """Test hook: fragments (and segments) with more than `cap` hits (0..64) keep their work arrays in global scratch, not LDS."""
        self._check(self._lib.chaindp_debug_set_frag_lds_cap(self._ctx, int(cap)))

    def sketch_ms(self, reset=False):
        """(device ms, calls) of the sketch kernels accumulated while profiling is on."""
        ms, n = C.c_double(0), C.c_int64(0)
        self._check(self._lib.chaindp_get_sketch_ms(self._ctx, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, int(n.value)

    def post_logf_selftest(self, kmax=1 << 24):
        """Mismatches of the device's logf of the integers 1..kmax against the host's (0 expected)."""
        n = self._lib.chaindp_post_logf_selftest(self._ctx, int(kmax))
        if n < 0:
            self._check(int(n))
        return int(n)

    # -- device-pointer path (torch tensors or any other HBM allocation)
    def run_device(self, par, n_reads, total, d_off, d_a, d_n_segs, d_f, d_p, d_v, stream=0):
        self._check(self._lib.chaindp_run_device(self._ctx, C.byref(par), n_reads, total, d_off, d_a, d_n_segs or None,
                                                 d_f, d_p, d_v, stream or None))

    def set_ring(self, ring):
        self._check(self._lib.chaindp_set_ring(self._ctx, ring))

    def set_variant(self, force_general):
        """0 / False: two units per wave (k_chain_twin) + one per wave for what it hands over; 1 / True: everything through the
        general variant of k_chain_units; 2: k_chain_units only (table-driven where it applies)."""
        self._check(self._lib.chaindp_set_variant(self._ctx, int(force_general)))

    # -- measurement
    def set_profiling(self, on=True):
        self._check(self._lib.chaindp_set_profiling(self._ctx, int(bool(on))))

    def kernel_ms(self, reset=False):
        """Accumulated HIP-event device time per kernel: dict name -> (ms, launches)."""
        ms = (C.c_double * 4)()
        n = (C.c_int64 * 4)()
        self._check(self._lib.chaindp_get_kernel_ms(self._ctx, ms, n, int(reset)))
        return {k: (ms[i], n[i]) for i, k in enumerate(("prepass", "chain_dp", "compact", "backtrack"))}

    def leftover_units(self):
        """Units the two-per-wave kernel handed over to the one-per-wave kernel in the last run (test / tuning hook)."""
        return int(self._lib.chaindp_debug_leftover(self._ctx))

    def seed_route(self):
        """How the last collect_seeds was routed (read-only test hook): dict of max_n, max_n2, lab_cap (the limits the context settled
        on when it first collected seeds), items (buckets k_seed_sort_huge handed to the LDS sort) and tied (units with equal x)."""
        out = (C.c_int64 * 5)()
        self._check(self._lib.chaindp_debug_seed_route(self._ctx, out))
        return dict(zip(("max_n", "max_n2", "lab_cap", "items", "tied"), (int(x) for x in out)))

    def device_bytes(self):
        """Bytes of device memory the context owns at this moment (test hook)."""
        return int(self._lib.chaindp_debug_device_bytes(self._ctx))

    def deep_units(self):
        """Units the one-per-wave kernel handed over to k_chain_dense in the last run (test / tuning hook)."""
        return int(self._lib.chaindp_debug_deep_units(self._ctx))

    def set_twin_tables(self, two=True):
        """Test hook: True keeps k_chain_twin on its layout with a cost table per half even where the batch has one table key (the
        layout with one table per wave takes such batches otherwise); False lets the device decide."""
        self._check(self._lib.chaindp_debug_set_twin_tables(self._ctx, int(bool(two))))

    def twin_tables(self):
        """Which layout k_chain_twin ran the last batch with (test hook): 1 one cost table per wave, 2 one per half, 0 neither."""
        return int(self._lib.chaindp_debug_twin_tables(self._ctx))

    def set_twin_handover(self, mode=0):
        """Test hook: what k_chain_twin hands over to k_chain_units whatever the units look like -- 0 nothing extra, 1 every unit
        untouched, 2 every unit after its first 64-anchor tile (k_chain_units resumes behind the flushed tiles)."""
        self._check(self._lib.chaindp_debug_set_twin_handover(self._ctx, int(mode)))

    def set_deep_handover(self, on=True):
        """Test hook: False keeps every unit in the launch that took it (k_chain_units then serves long scans from HBM/L2); 2 hands
        over any unit with a few deep scans, whatever its length, to k_chain_dense, 3 to k_chain_dense1, 4 to k_chain_dense16 (small
        test inputs reach every kernel)."""
        self._check(self._lib.chaindp_debug_set_deep_handover(self._ctx, on if on in (2, 3, 4) else int(bool(on))))

    def stats(self):
        st = (C.c_int64 * 4)()
        self._check(self._lib.chaindp_get_stats(self._ctx, st))
        return dict(units=st[0], singletons=st[1], anchors=st[2], reads=st[3])


class PinnedArray:
    """A numpy view of pinned (DMA-able) host memory from chaindp_host_alloc; what makes Pipe's copies asynchronous."""

    def __init__(self, shape, dtype):
        self._lib = lib()
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        self._ptr = self._lib.chaindp_host_alloc(max(n, 1))
        if not self._ptr:
            raise ChainDPError("chaindp_host_alloc failed (no GPU runtime or out of pinned memory)")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(n, 1)).from_address(self._ptr))[:n].view(dtype).reshape(shape)

    def free(self):
        if self._ptr:
            self.array = None
            self._lib.chaindp_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _PipeResult(C.Structure):
    _fields_ = [("tag", C.c_int64), ("n_reads", C.c_int64), ("n_anchors", C.c_int64), ("n_seeds", C.c_int64),
                ("seeds_off", C.c_void_p), ("seeds", C.c_void_p)]


class Pipe:
    """chaindp_pipe_t: batches stream through `depth` contexts so that H2D(n+1), kernels(n) and D2H(n-1) overlap."""

    def __init__(self, device=0, depth=3, max_anchors=1 << 24, max_reads=1 << 20):
        self._lib = lib()
        if self._lib.chaindp_device_count() <= 0:
            raise ChainDPError("no HIP device visible: the chaining DP runs only on the GPU (no CPU fallback)")
        self._p = self._lib.chaindp_pipe_create(device, depth, max_anchors, max_reads)
        if not self._p:
            raise ChainDPError((self._lib.chaindp_pipe_last_error(None) or b"").decode())
        self.depth = depth
        self._keep = collections.deque()       # host arrays of the batches in flight, oldest first (batches complete in submission order)

    def close(self):
        if self._p:
            self._lib.chaindp_pipe_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise ChainDPError(f"chaindp pipe error {rc}: {self._lib.chaindp_pipe_last_error(self._p).decode()}")

    def submit(self, par, off, anchors, n_segs=None, tag=0):
        """Asynchronous.  off / anchors / n_segs must stay alive (they are kept referenced here) until wait() returns the batch."""
        off, anchors, ns = Device._prep(off, anchors, n_segs)
        rc = self._lib.chaindp_pipe_submit(self._p, C.byref(par), len(off) - 1, _ptr(off), _ptr(anchors), _ptr(ns), tag)
        if rc == -5:
            return False
        self._check(rc)
        self._keep.append((off, anchors, ns))   # by submission, not by tag: two batches may carry the same tag
        return True

    def wait(self, copy=True):
        """Oldest batch: (tag, seeds_off, seeds).  With copy=False the arrays alias the pipe's pinned buffers and are valid
        until release()."""
        r = _PipeResult()
        self._check(self._lib.chaindp_pipe_wait(self._p, C.byref(r)))
        soff = np.ctypeslib.as_array((C.c_int64 * (r.n_reads + 1)).from_address(r.seeds_off))
        seeds = np.ctypeslib.as_array((C.c_uint8 * max(r.n_seeds * 24, 1)).from_address(r.seeds))[:r.n_seeds * 24].view(SEED_DTYPE)
        if copy:
            soff, seeds = soff.copy(), seeds.copy()
        if self._keep:
            self._keep.popleft()
        return r.tag, soff, seeds

    def release(self):
        self._check(self._lib.chaindp_pipe_release(self._p))
