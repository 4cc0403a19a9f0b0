// chaindp_ctx.h -- what the translation units of the host ABI (chaindp_abi*.cpp) share: the context, the index image, HIP_TRY and
// the helpers and stage entry points that more than one stage uses.  Host only; nothing else includes it.
#ifndef CHAINDP_CTX_H
#define CHAINDP_CTX_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>
#include "../../include/chaindp.h"
#include "../../include/chaindp_debug.h"
#include "chaindp_kernels.h"
#include "chaindp_devmem.h"
#include "chaindp_apost_plan.h"

struct EventSet { hipEvent_t e[3]; int n; int slot0; };  // e[0..n): consecutive kernel boundaries; slot0 = first ms[] index

struct chaindp_ctx {
	int device = -1;
	chaindp::DpDevice dp;            // what the DP launchers need of the device and the process (filled by chaindp_create)
	// every device buffer below is an entry of this pool: allocated, grown and freed through it and nowhere else
	chaindp::DevPool pool{[](void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }, [](void *p) { return (int)hipFree(p); }};
	hipStream_t stream = nullptr;
	int64_t cap_anchors = 0, cap_reads = 0;
	int ring = 128;
	// resident batch
	int64_t n_reads = 0, total = 0, n_seeds = 0;
	bool has_n_segs = false, ran = false;
	bool singles_pending = false;    // the last run left f, p, v, flags[] of its singletons to k_fill_singles (chaindp_download runs it)
	chaindp_params_t ran_par{};      // the parameters of that run
	// per-read chaining gaps (chaindp_set_read_gaps): int2 (gap_ref, gap_qry) per read
	chaindp::DevGrow gaps_set;       // the gaps in force, for gaps_n reads
	chaindp::DevGrow gaps_ran;       // the last run's own copy of them: what the stages behind that run read
	int64_t gaps_n = -1;             // reads the gaps in force were set for; -1: none are in force
	bool ran_gaps = false;           // the last run took its gaps from gaps_ran instead of ran_par.max_dist_x / max_dist_y
	int64_t *d_off = nullptr;
	void *d_a = nullptr;
	int32_t *d_n_segs = nullptr;
	int32_t *d_f = nullptr, *d_p = nullptr, *d_v = nullptr;
	// scratch
	unsigned long long *d_tg = nullptr;   // deep-path marks, tagged with the run epoch (never re-initialised)
	uint32_t epoch = 0;
	unsigned long long *d_sumq = nullptr;
	chaindp::Unit *d_units = nullptr;
	chaindp::UnitAux *d_unit_aux = nullptr;   // per unit, beside d_units: what k_chain_twin needs to pick it up without further loads
	chaindp::Unit *d_left = nullptr;          // units the two-per-wave kernel hands over to k_chain_units
	unsigned long long *d_left_cnt = nullptr; // the four hand-over words: counts, queue words and the route flag (chaindp::HandoverWords)
	chaindp::Unit *d_deep = nullptr;          // units k_chain_units hands over to its k_chain_dense (scans that keep reaching past the ring)
	int deep_route = 0;                   // test hook: 1 k_chain_dense, 2 k_chain_dense1 whatever the batch looks like
	int deep_eager = 0;                   // test hook: hand over any unit with a few deep scans, whatever its length
	bool deep_handover = true;            // CHAINDP_NO_DEEP_HANDOVER (diagnostic / A-B): every unit stays in the launch that took it
	int twin_two_tables = 0;              // chaindp_debug_set_twin_tables (tests): 1 keeps one-key batches on k_chain_twin's two-table layout
	int twin_force_left = 0;              // CHAINDP_TWIN_FORCE_LEFT / chaindp_debug_set_twin_handover (tests): 1 k_chain_twin hands every unit
	                                      // over untouched, 2 after its first tile (k_chain_units resumes there); the variable is read once, at chaindp_create
	int variant = 0;                      // 0: k_chain_twin + k_chain_units for the rest; 1: k_chain_units, general variant; 2: k_chain_units only
	unsigned long long *d_counters = nullptr;
	chaindp::PrepassScratch pre = {nullptr, nullptr, nullptr, nullptr, nullptr};
	chaindp::CompactScratch cmp = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	chaindp::BottomScratch bot = {};
	// first-use groups of buffers: each flag is set once, after its group's allocations have all succeeded, and never reset
	bool compact_ready = false, bot_ready = false, seed_ready = false, regs_ready = false, post_ready = false, logf_ready = false;
	chaindp::DevGrow lut;            // uint16_t[]: the per-read gap-cost tables of the fast variant
	chaindp::DevGrow ptrs;           // void*[]: per-read host pointers for the gather / scatter kernels
	bool use_lut = true;
	// compaction (allocated on first use)
	int32_t *d_first_child = nullptr;
	unsigned int *d_twin_queue = nullptr;   // k_chain_twin's eight grab counters, a cache line apart (2 KB)
	int64_t *d_seeds_off = nullptr;
	void *d_seeds = nullptr;
	// seed collection (allocated on first use, grown with the batch)
	chaindp::SeedScratch seed = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	void *d_mini = nullptr;
	int64_t *d_mini_off = nullptr, *d_mp_off = nullptr;
	uint32_t *d_bid = nullptr;
	int32_t *d_qlen = nullptr, *d_rep_len = nullptr;
	unsigned long long *d_mini_pos = nullptr;
	int64_t seed_cap_mini = 0, n_mini_pos = 0;
	int seed_max_n = -1, seed_max_n2 = -1; // largest reads the two configurations of the LDS sort take on this device
	int seed_lab_cap = 0;                  // digits k_seed_sort_huge keeps in LDS
	bool seed_route_valid = false;         // seed.totals[2..3] are the last collection's (chaindp_debug_seed_route): its sort was launched
	// chains to hits (allocated on first use, grown with the batch)
	chaindp::DevGrow regs, reg_counts, ref_len, mp_up;
	uint32_t *d_rhash = nullptr;
	int32_t *d_rqlen = nullptr;
	int64_t *d_regs_off = nullptr, *d_mp_off_up = nullptr;
	unsigned long long *d_sum_k = nullptr;
	int64_t bot_n_reads = -1, bot_n_chains = 0, bot_n_b = 0;   // what the last chaindp_backtrack left resident (-1: nothing of this batch)
	bool mp_resident = false;                                  // this batch's mini_pos are on the device (it came from chaindp_collect_seeds)
	bool regs_resident = false;      // regs / d_rqlen hold what chaindp_gen_regs made of the resident chains (chaindp_est_err's upload clears it)
	// chain_post + mm_set_mapq (allocated on first use, grown with the batch)
	chaindp::DevGrow post_stage, post_out, post_sq, post_scratch;
	unsigned long long *d_post_off = nullptr, *d_post_tile = nullptr;
	int32_t *d_post_qlen = nullptr, *d_post_rep = nullptr, *d_post_err = nullptr;
	uint32_t *d_logf_k = nullptr;
	float *d_logf_v = nullptr;
	int n_logf = 0;
	// reads of several segments: chaindp_frag_post (allocated on first use, grown with the batch)
	chaindp::DevGrow frag_seq, frag_cnt, frag_u, frag_a, frag_stage, frag_z, frag_stacks, frag_out;
	// alignment, chaindp_ksw_extd (allocated on first use, grown with the batch): sequences; problem records and their order, result
	// words behind the counters and CSR offsets (both laid out by KswLayout, read through ksw_view); the workgroups' slices of DP state
	// (global route) and of path matrix; CIGARs as the DP left them
	chaindp::DevGrow ksw_bases, ksw_prob, ksw_ez, ksw_state, ksw_path, ksw_cig;
	chaindp::DevGrow cigar_out;                // the packed CIGARs of whichever alignment call ran last (cigar_pack_out): none overlap on a context
	double ksw_ms = -1;                        // k_ksw_extd's device time in the last call made while profiling was on
	int ksw_grid_cap = 0;                      // chaindp_ksw_debug_set_grid_cap: at most so many workgroups per DP launch (0: the plan's own)
	int64_t ksw_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the last plan ksw_reserve saw: count, grid, lds_bytes, path_stride of the two launches (chaindp_ksw_debug_launch)
	int64_t ksw_n = -1;                        // problems of the last chaindp_ksw_extd whose results are resident (chaindp_ksw_debug_route)
	// mm_align1, chaindp_align1 (allocated on first use, grown with the batch): the targets' codes and offsets; the reads, anchors and
	// regions of the batch with their offsets; the regions' plans, problem slots and side records; the first pass's results and CIGARs
	// kept over the second pass; the Z-drop codes and the second pass's index; the stitched CIGARs
	chaindp::DevGrow al_tgt, al_toff, al_in, al_reg, al_slot, al_side, al_ez1, al_cig1, al_code, al_stage;
	std::vector<int64_t> al_t_off;             // the resident targets' offsets (host copy); empty: none set
	double al_ms[5] = {-1, -1, -1, -1, -1};    // plan, DP, zdrop, stitch, extra of the last chaindp_align1 made while profiling was on
	// mm_align1_inv, chaindp_align1_inv (allocated on first use, grown with the batch): the reads and regions of the batch with the
	// candidate list; the per-slot results; the local scores, survivors and their problems
	chaindp::DevGrow inv_in, inv_res, inv_ll;
	int64_t inv_n = -1;                        // candidates of the last chaindp_align1_inv whose local scores are resident (chaindp_align_inv_debug_ll)
	double inv_ms[4] = {-1, -1, -1, -1};       // local score, gather + DP, finish + skip, pack of the last call made while profiling was on
	// mm_align_skeleton, chaindp_align_reads (allocated on first use, grown with the batch): the reads' offsets, bases and anchors for
	// all rounds; the pool of records and the pool of CIGAR words the rounds and the inversion call leave (each one of a pair of
	// buffers: a pool that grows moves to the other one, what it holds copied); the lists with the finish's work arrays; the result
	chaindp::DevGrow rd_in, rd_rec[2], rd_cig[2], rd_list, rd_out, rd_out_cig;
	int rd_rec_cur = 0, rd_cig_cur = 0;
	int64_t rd_n_reads = -1;                   // reads of the resident result of the last chaindp_align_reads (-1: none)
	int64_t rd_n_rec = 0;                      // records in its pool
	int64_t rd_need[2] = {0, 0};               // its final regions and CIGAR words
	size_t rd_out_at[5] = {0, 0, 0, 0, 0};     // where out_off, regs, extra, cigar_off lie in rd_out, and placed in rd_list
	std::vector<int64_t> rd_rounds;            // regions per round of that call (chaindp_align_reads_debug_rounds)
	std::vector<int64_t> rd_list_off;          // its lists: offsets and pool records, for chaindp_align_reads_debug_placed
	std::vector<int32_t> rd_item;
	int rd_lds_cap = RD_LDS_CAP;               // chaindp_align_reads_debug_set_lds_cap (tests): shorter lists stay in LDS
	double rd_ms[4] = {-1, -1, -1, -1};        // rounds, inversions, finish, gather of the last call made while profiling was on
	// the tail of align_regs and mm_set_mapq, chaindp_align_post (allocated on first use, grown with the batch): what comes up from the
	// host; the kernels' work arrays, with out_off; the result; its CIGAR words; the logf list of one match_sc
	chaindp::DevGrow ap_in, ap_work, ap_out, ap_out_cig, ap_dp;
	int64_t ap_n_reads = -1;                   // reads of the resident result of the last chaindp_align_post (-1: none)
	int64_t ap_need[2] = {0, 0};               // its final regions and CIGAR words
	size_t ap_at[5] = {0, 0, 0, 0, 0};         // where out_off lies in ap_work and regs, extra, dp_max2, cigar_off in ap_out
	int ap_dp_sc = 0, ap_n_dp = 0;             // the match_sc whose list ap_dp holds (0: none) and its entries
	int ap_lds_cap = AP_LDS_CAP;               // chaindp_align_post_debug_set_lds_cap (tests): shorter lists stay in LDS
	double ap_ms[2] = {-1, -1};                // k_apost_read with the scans, the gathers of the last call made while profiling was on
	// chain_post to the alignment stages, chaindp_align_resident (allocated on first use, grown with the batch): a_off with the scan's
	// scratch behind it; the squeezed anchors; the regions with their new `as`
	chaindp::DevGrow ho_off, ho_a, ho_regs, ho_in;   // (ho_in: what chaindp_map_align_debug_run_handoff brings up)
	int64_t post_n_reads = -1;                 // reads of the batch whose chaindp_chain_post result is whole in post_out / post_sq / d_post_off (-1: none)
	int64_t post_n_out = 0;                    // its final regions
	bool post_cigar = false;                   // it ran with MM_F_CIGAR
	std::vector<int32_t> post_ref_len;         // the ref_len it was given
	bool from_sketch = false;                  // the resident batch's minimizers were the resident sketch's (begin_batch clears it)
	int64_t ho_n_reads = -1;                   // reads of the last hand-off (-1: none) and the host's copy of what it left, which the planner reads
	std::vector<int64_t> ho_h_regs_off, ho_h_a_off;
	std::vector<int32_t> ho_h_regs;
	std::vector<uint64_t> ho_h_a;
	int ho_lds_cap = HO_LDS_CAP;              // chaindp_map_align_debug_set_lds_cap (tests): shorter lists stay in LDS
	double ho_ms = -1;                         // the hand-off's kernels in the last chaindp_align_resident made while profiling was on
	int frag_lds_cap = FRAG_LDS_CAP;           // chaindp_debug_set_frag_lds_cap (tests): fewer hits per fragment stay in LDS
	// sketch (allocated on first use, grown with the batch)
	chaindp::SketchArgs sk = {};
	int64_t sk_cap_bases = -1, sk_cap_chunks = -1, sk_cap_seqs = -1;
	int64_t sk_max_bases = 0x7fffff00;         // CHAINDP_SKETCH_MAX_BASES (test switch) lowers it; positions and ranks are 32-bit
	unsigned long long *d_sk_totals = nullptr;
	bool sk_valid = false;                     // d_mini / d_mini_off hold what the last chaindp_sketch made
	int64_t sk_n_reads = 0, sk_n_mini = 0;
	int ix_status = 0;                         // code of the last chaindp_index_build (chaindp_index_build_status)
	int64_t ix_chunk_bases = 0;                // chaindp_debug_index_chunk_bases (tests): bases per sketch sub-batch of an index build, 0 = sk_max_bases
	std::vector<int64_t> sk_mini_off;          // its mini_off and the reads' lengths, for the calls that say "the resident ones"
	std::vector<int32_t> sk_qlen;
	std::vector<int32_t> sk_seq_len;           // ... and the lengths of its sequences (the segments of chaindp_frag_post)
	hipEvent_t sk_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the two phases of a sketch while profiling is on (created once)
	double sk_ms = 0;
	int64_t sk_calls = 0;
	// profiling
	bool prof = false;
	std::vector<EventSet> pending;
	double ms[4] = {0, 0, 0, 0};
	int64_t launches[4] = {0, 0, 0, 0};
	int64_t stats[4] = {0, 0, 0, 0};
	std::string err;
};

struct chaindp_index {
	int device = -1;
	uint8_t *blob[4] = {nullptr, nullptr, nullptr, nullptr};
	size_t bytes[4] = {0, 0, 0, 0};
	int b_bits = 0;
	bool built = false;              // made by chaindp_index_build / chaindp_debug_index_from_minimizers
	int64_t route[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // what the build did (chaindp_debug_index_route)
	double stage_ms[4] = {0, 0, 0, 0};             // sketch sub-batches with their uploads (host clock); sort, grouping, tables (device, events)
};

// (ctx: a context or a pipe)
#define HIP_TRY(ctx, call)                                                                         \
	do {                                                                                           \
		hipError_t e_ = (call);                                                                    \
		if (e_ != hipSuccess) {                                                                    \
			(ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
			return CHAINDP_ERR_HIP;                                                                \
		}                                                                                          \
	} while (0)

namespace chaindp {

extern thread_local std::string g_create_error;     // what chaindp_last_error(NULL) / chaindp_pipe_last_error(NULL) return

// ---- helpers (chaindp_abi.cpp unless noted)
int first_use(chaindp_ctx *ctx, bool &ready, const char *what, std::initializer_list<DevBuf> bufs);
hipError_t dev_grow(chaindp_ctx *ctx, DevGrow &g, size_t need);
void begin_batch(chaindp_ctx *ctx, int64_t n_reads, int64_t total, bool mp_resident = false);
hipError_t stage_n_segs(chaindp_ctx *ctx, const int32_t *n_segs_per_read, int64_t n_reads, hipStream_t st);
hipError_t prof_begin(chaindp_ctx *ctx, EventSet &es, int n, int slot0, hipStream_t st);
hipError_t prof_mark(chaindp_ctx *ctx, EventSet &es, int k, hipStream_t st);
Params to_params(const chaindp_params_t *p);
int check_params(chaindp_ctx *ctx, const chaindp_params_t *par);
int check_read_gaps(chaindp_ctx *ctx, int64_t n_reads);   // ERR_ARG while per-read gaps are in force for another number of reads
int check_batch(const chaindp_ctx *ctx, int64_t n_reads, const int64_t *off, const void *payload, bool per_read, const char *owner,
                std::string &err, int64_t &total);
int stage_pointers(chaindp_ctx *ctx, const void *const *ptrs, int64_t n);
// chaindp_abi_hits.cpp
int regs_per_read_buffers(chaindp_ctx *ctx);
int mini_pos_check(chaindp_ctx *ctx, const int64_t *mini_pos_off, const uint64_t *mini_pos);
int stage_mini_pos(chaindp_ctx *ctx, int64_t R, const int64_t *mini_pos_off, const uint64_t *mini_pos, const int32_t *ref_len, int32_t n_ref,
                   const int64_t *&d_mpo, const unsigned long long *&d_mp);
// chaindp_abi_seed.cpp
int seed_reserve(chaindp_ctx *ctx, int64_t n_mini, bool oom_is_capacity = false);
// chaindp_abi_post.cpp
int post_reserve(chaindp_ctx *ctx, int64_t n_c, int64_t n_b);
PostOpt to_post_opt(const chaindp_post_opt_t *o);
int post_require_hits(chaindp_ctx *ctx, const char *who);
int post_stage_rep_len(chaindp_ctx *ctx, const int32_t *rep_len, int64_t R, const int32_t **d_rep);
int post_finish(chaindp_ctx *ctx);
int post_logf_upload(chaindp_ctx *ctx);           // post_logf_int's list on the device: d_logf_k, d_logf_v, n_logf

// chaindp_abi_ksw.cpp: the host scaffold of the alignment stages (chaindp_ksw_extd, chaindp_align1, chaindp_align1_inv, and any new one)
int ksw_grow(chaindp_ctx *ctx, DevGrow &g, size_t need, const char *what, const char *who);
int ksw_reserve(chaindp_ctx *ctx, const KswPlan &pl, int64_t n_bases, const char *who);
// Every copy of the alignment stages between host and device: in pieces of KSW_COPY_PIECE bytes, which the runtime moves through its own
// staging buffers.  Given megabytes of pageable memory in one copy it pins the pages instead, and the pages of arrays that are
// freed afterwards (a call's temporaries, a caller's outputs) cost a later synchronise 15 to 29 ms on an MI355X.
#define KSW_COPY_PIECE ((size_t)256 << 10)
hipError_t host_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st);
// where the DP's records and results for N problems lie on the device (KswLayout over ksw_prob and ksw_ez), and its CIGAR staging
struct KswView { KswProb *prob; int32_t *order; unsigned int *counter; int64_t *off; int32_t *ez; uint32_t *cig; };
KswView ksw_view(const chaindp_ctx *ctx, size_t N);
// While profiling is on: an event at every boundary between the stages of a call; destroyed on every way out of it.
struct StageEvents {
	explicit StageEvents(chaindp_ctx *c) : ctx(c) {}
	StageEvents(const StageEvents&) = delete;
	~StageEvents();
	hipError_t mark(int stage);      // the time since the last mark belongs to `stage` (-1: host time, not counted); nothing while profiling is off
	int fold(double *ms, int n);     // with any mark made: ms[0..n) = the milliseconds of every stage, ms[] untouched otherwise
	chaindp_ctx *ctx;
	std::vector<hipEvent_t> e;
	std::vector<int> stage;          // the stage that ends at e[k]
};
// the records and their order up, the two launches; the bases are on the device already.  ev (or null): the launches alone are its stage 0
int ksw_dispatch(chaindp_ctx *ctx, const KswPlan &pl, StageEvents *ev);
// The end of a call that returns CIGARs: cigar_off[0..n] is filled and sums to total.  Refuses a total above cigar_cap
// (CHAINDP_ERR_CAPACITY); else offsets up to d_off, launch(out) packs into cigar_out, the words come down into cigar, the stream is idle.
int cigar_pack_out(chaindp_ctx *ctx, const char *who, const int64_t *cigar_off, int64_t n, int64_t total, uint32_t *cigar, int64_t cigar_cap,
                   int64_t *d_off, const std::function<hipError_t(uint32_t *out)> &launch);

// The end of a call that leaves its CIGARs on the device: as cigar_pack_out, but launch(out) packs to the address room(total) names
// (room returns 0 or the call's error code) and nothing comes down; the stream is idle afterwards.
int cigar_pack_dev(chaindp_ctx *ctx, const int64_t *cigar_off, int64_t n, int64_t total, int64_t *d_off, const std::function<int(int64_t total, uint32_t **out)> &room,
                   const std::function<hipError_t(uint32_t *out)> &launch);

// ---- stage entry points that other stages call
// A batch of an alignment stage whose reads are on the device already (chaindp_align_reads): the device addresses of seq_off, seq and,
// for chaindp_align1, a_off and the anchors, which the stage then neither uploads nor, the anchors, downloads; where its packed
// CIGARs go (total words in, a device address out; 0 or an error code).  The stage fills in where it left its per-region records on
// the device: regs, extra (chaindp_align1) or r_inv, extra (chaindp_align1_inv), valid until the next call of that stage.
struct AlignResident {
	const int64_t *seq_off; const char *seq; const int64_t *a_off; void *a;
	std::function<int(int64_t total, uint32_t **out)> room;
	const AlignPlan *plan = nullptr;           // chaindp_align1 only: the caller has run align_plan on exactly these arguments already
	const int32_t *d_regs = nullptr, *d_extra = nullptr;
};
// chaindp_align1 / chaindp_align1_inv with their arguments; res == nullptr: exactly the public call.  With res, seq and a are read only
// by the planner (a may carry the marks of an earlier round or not: the planner reads none of a[].y's flag bits), cigar and cigar_cap
// are ignored and cigar_off is still filled.
int align1_impl(chaindp_ctx *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const int64_t *a_off,
                chaindp_anchor_t *a, const int64_t *regs_off, chaindp_reg_t *regs, chaindp_reg_t *regs2, chaindp_align_extra_t *extra, int64_t *cigar_off,
                uint32_t *cigar, int64_t cigar_cap, AlignResident *res);
int align1_inv_impl(chaindp_ctx *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const int64_t *regs_off,
                    const chaindp_reg_t *regs, int32_t *made, chaindp_reg_t *r_inv, chaindp_align_extra_t *extra, int64_t *cigar_off, uint32_t *cigar,
                    int64_t cigar_cap, AlignResident *res);
// chaindp_align_reads up to its resident result (chaindp_abi_reads.cpp): everything but the delivery into the caller's arrays.
// from == nullptr: the reads go up from the host arrays.  Else the reads are on the device already (from's seq_off, seq, a_off, a;
// chaindp_align_resident): nothing of them goes up, seq is not read, the host's seq_off, a_off, a and regs serve the planner alone,
// and a receives the device anchors' marks only with marks_down.
int align_reads_compute(chaindp_ctx *ctx, const chaindp_align_opt_t *opt, int64_t n_reads, const int64_t *seq_off, const char *seq, const int64_t *a_off,
                        chaindp_anchor_t *a, const int64_t *regs_off, const chaindp_reg_t *regs, int64_t regs_cap, int64_t cigar_cap,
                        const AlignResident *from = nullptr, bool marks_down = true);
// chaindp_chain_post (chaindp_abi_post.cpp); keep_only: the final hits stay in HBM, regs_off is filled, regs and regs_cap are not looked at
int chain_post_impl(chaindp_ctx *ctx, const chaindp_post_opt_t *opt, const int32_t *qlen, const int32_t *rep_len, const int32_t *ref_len, int32_t n_ref,
                    const int64_t *mini_pos_off, const uint64_t *mini_pos, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap, int64_t *a_off,
                    chaindp_anchor_t *a, bool keep_only);
// the stage of chaindp_align_post over the resident result of align_reads_compute, and the delivery of its own result (chaindp_abi_apost.cpp).
// d_rep_len: the reads' rep_len on the device (rep_len is then not read), or nullptr: rep_len comes up from the host
int align_post_resident(chaindp_ctx *ctx, const char *who, const chaindp_post_opt_t *opt, int64_t n_reads, const int32_t *rep_len, const int32_t *d_rep_len);
int align_post_deliver(chaindp_ctx *ctx, const char *who, int64_t n_reads, int64_t *out_off, chaindp_reg_t *out_regs, chaindp_align_extra_t *out_extra,
                       int32_t *out_dp_max2, int64_t regs_cap, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t need[2]);
int collect_seeds_impl(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, int64_t n_reads,
                       const int64_t *mini_off, const chaindp_anchor_t *mini, const chaindp_anchor_t *const *read_mini,
                       const uint32_t *bid, const int32_t *qlen,
                       const int32_t *n_segs_per_read, int64_t *off, int32_t *rep_len, int64_t *mini_pos_off);
int sketch_impl(chaindp_ctx *ctx, int w, int k, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const char *seq,
                const int32_t *n_segs_per_read, int64_t *mini_off, int pe_ori, int64_t rid_base = -1);
int gen_regs_impl(chaindp_ctx *ctx, const uint32_t *hash, const int32_t *qlen, chaindp_reg_t *regs, bool download);
int map_prefix(chaindp_ctx *ctx, const chaindp_index_t *ix, int flag, int max_occ, const chaindp_params_t *par, int min_cnt, int64_t n_reads,
               const int64_t *mini_off, const chaindp_anchor_t *mini, const uint32_t *bid, const int32_t *&qlen, const int32_t *n_segs_per_read,
               const uint32_t *hash, int32_t *rep_len, int64_t *n_anchors, int64_t *regs_off, chaindp_reg_t *regs, int64_t regs_cap);

}  // namespace chaindp
#endif
