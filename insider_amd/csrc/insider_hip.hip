// insider_hip.hip — host driver and C ABI of libinsider_hip.so (see include/insider_hip.h).
//
// The outer alternating loop is the reference's optimize() (src/optimize.cpp:255-422) re-derived as
// "statistics, then solve" (DESIGN.md section 2): two streaming passes over (X, mask codes) per outer iteration
// — one per sample for the row update, one per gene fused with the elastic-net solve — and a handful of small
// dense kernels.  Everything is enqueued on one HIP stream; the host synchronises only at the reference's loss
// checkpoints (every 10th iteration) and around the optional cross-rank all-reduce.
#include "insider_kernels.hpp"
#include "insider_posthoc.hpp"
#include "insider_vardecomp.hpp"
#include "insider_sampdecomp.hpp"
#include "insider_levelscores.hpp"
#include "insider_factdecomp.hpp"
#include "insider_rescomp.hpp"
#include "insider_outliers.hpp"
#include "insider_neighbors.hpp"
#include "insider_coexpr.hpp"
#include "insider_coexpr_pc.hpp"
#include "insider_enrich.hpp"
#include "insider_kmeans.hpp"
#include "insider_hclust.hpp"
#include "insider_tsne.hpp"

#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <atomic>
#include <string>
#include <utility>
#include <vector>

#include "../../include/insider_hip.h"

using namespace insider;

#include "insider_plan.hpp"

namespace {

thread_local std::string g_err;
thread_local double g_last_cd_ms = 0.0;   // per calling thread: the ABI is re-entrant per handle / per thread
thread_local int g_last_cd_solver = 0;     // (ColSolver)
thread_local double g_last_neighbors_ms = 0.0;
thread_local double g_last_gram_topk_ms = 0.0;
thread_local double g_last_enrichment_ms = 0.0;
thread_local double g_last_kmeans_ms = 0.0;
thread_local double g_last_hclust_ms = 0.0;
thread_local double g_last_tsne_ms = 0.0;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIPCHECK(call)                                                                                  \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? INSIDER_ERR_ALLOC : INSIDER_ERR_HIP,                \
                        std::string(#call) + ": " + hipGetErrorString(e_));                             \
    } while (0)

#define KCHECK() HIPCHECK(hipGetLastError())


// Device bytes allocated (and not freed again) by the calling thread while a Tally is open: what a data set's set-up
// allocated for itself (DataSet::bytes_own), temporaries of the stages excluded.
struct Tally {
    int64_t bytes = 0;
    Tally *prev;
    static Tally *&open() { static thread_local Tally *t = nullptr; return t; }
    Tally() : prev(open()) { open() = this; }
    ~Tally() { open() = prev; }
    Tally(const Tally &) = delete;
    Tally &operator=(const Tally &) = delete;
    static void add(int64_t b) { if (open()) open()->bytes += b; }
};

// One device allocation of count T, handed to launches as a raw pointer.  The allocation is freed when the last DevBuf that
// holds it is destroyed or reassigned: alloc() makes a fresh one, share() joins another buffer's (a re-masked data set
// holds the mask-independent arrays of its source this way: nothing is copied, and either side may go first).
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : blk_(std::move(o.blk_)), p_(o.p_), count_(o.count_), own_(o.own_) { o.p_ = nullptr; o.count_ = 0; o.own_ = false; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            blk_ = std::move(o.blk_);
            std::swap(p_, o.p_);
            std::swap(count_, o.count_);
            std::swap(own_, o.own_);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p_ && own_) Tally::add(-(int64_t)bytes());
        blk_.reset();
        p_ = nullptr;
        count_ = 0;
        own_ = false;
    }
    // a fresh allocation of count elements (at least one); the old one is let go first
    int alloc(size_t count)
    {
        reset();
        if (count == 0) count = 1;
        T *p = nullptr;
        HIPCHECK(hipMalloc((void **)&p, count * sizeof(T)));
        blk_ = std::make_shared<Block>(p);
        p_ = p;
        count_ = count;
        own_ = true;
        Tally::add((int64_t)bytes());
        return INSIDER_OK;
    }
    // at least count elements: a new allocation only when the current one is smaller (contents are not kept)
    int grow(size_t count) { return std::max<size_t>(count, 1) <= count_ ? INSIDER_OK : alloc(count); }
    // an allocation of max(v.size(), count) elements that starts with the host vector v
    int upload(const std::vector<T> &v, size_t count = 0)
    {
        if (int rc = alloc(std::max(v.size(), count))) return rc;
        HIPCHECK(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return INSIDER_OK;
    }
    // the allocation of o, held jointly (nothing when o holds none); returns the bytes now shared
    size_t share(const DevBuf &o)
    {
        reset();
        blk_ = o.blk_;
        p_ = o.p_;
        count_ = o.count_;
        return bytes();
    }
    size_t bytes() const { return p_ ? count_ * sizeof(T) : 0; }
    T *get() const { return p_; }
    operator T *() const { return p_; }

private:
    struct Block {
        void *p;
        explicit Block(void *q) : p(q) {}
        Block(const Block &) = delete;
        Block &operator=(const Block &) = delete;
        ~Block() { if (p) (void)hipFree(p); }
    };
    std::shared_ptr<Block> blk_;
    T *p_ = nullptr;
    size_t count_ = 0;
    bool own_ = false;                // allocated here (alloc), not joined (share)
};

// An owned stream or event, destroyed with its owner.
template <typename H, hipError_t (*Destroy)(H)>
class HipObject {
public:
    HipObject() = default;
    HipObject(const HipObject &) = delete;
    HipObject &operator=(const HipObject &) = delete;
    HipObject(HipObject &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    HipObject &operator=(HipObject &&o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(h_, o.h_);
        }
        return *this;
    }
    ~HipObject() { reset(); }
    void reset()
    {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H *out() { reset(); return &h_; }   // for the create call
    operator H() const { return h_; }

private:
    H h_ = nullptr;
};
using Stream = HipObject<hipStream_t, hipStreamDestroy>;
using Event = HipObject<hipEvent_t, hipEventDestroy>;

struct CovTables {   // per covariate, device
    int L = 0, nchunks = 0;
    DevBuf<int> chunk_level, chunk_begin, chunk_end, lvl_chunk_ptr;
    // merged masked row update (insider_row_merged.hpp), built once per data set
    DevBuf<uint32_t> grp;             // [p][L + 1] positions of the level groups inside each gene's sorted held-out samples
    DevBuf<uint16_t> slev;            // per entry of every gene's level-grouped held-out samples: stacked level of each other covariate
    DevBuf<uint32_t> item_begin, item_end;   // weighted-SYRK work items: ranges of the (gene, count) lists
    DevBuf<int> lvl_item_ptr;         // [L + 1] items of every level
    int nitems = 0;
    int64_t npairs = 0;               // (level, gene) pairs with held-out samples
    DevBuf<int> wl_idx;               // (gene, count) lists of every level, padded like the held-out lists
    DevBuf<double> wl_w;
    DevBuf<double> paircnt;           // [L][SL] samples in (level of this covariate, stacked level of another one); its own block
                                      // is zero, columns SLcat .. SL - 1 hold sum_{r in l} z_rk (stage_pair_tables)
};
// continuous columns share one table: a single pseudo-level whose members are all samples, in 16-sample chunks

// Host copies of the small inputs the mask-dependent stages read (stage_merged, stage_cont_factored): kept with the
// mask-independent part, so that a re-mask runs the same stages without the caller's arrays.
struct HostTables {
    std::vector<int> lev0;            // c x n: 0-based level of every sample, covariate by covariate
    std::vector<double> ctns;         // n x m column-major: the continuous covariates
};

// Fold ids of the resident matrix (insider_hip_set_folds): 0 = NA, 1..F = the fold an entry is held out in
struct FoldIds {
    DevBuf<uint8_t> id;               // layout of X: gene-major lines of pitch ldn, pad elements 0
    int F = 0;
};

// The read-only DATA SET: everything insider_hip_create builds (X-derived lists, level sums, pair counts, chunk tables) and
// the shape facts that describe it.  Shared by the handles of insider_hip_clone — each has its own workspace, streams and
// options, so that several fits of one data set (tune()'s grid points) run on the GPU at the same time — and freed with the
// last of them.
// It has two parts.  The MASK-INDEPENDENT part depends on X and the covariates only: X, lev, members_all, lvl_ptr_all,
// lvl_count_all, lvl_off_d, the chunk tables and paircnt of every CovTables, cont, Zc, ident_members, one_count, cont_pair,
// cont_cnt, S, yy_all, host, the fold ids and the shape facts.  The MASK-DEPENDENT part is everything else.  A re-masked data set
// (insider_hip_remask, insider_hip_remask_fold) holds the allocations of its source's mask-independent part jointly
// (share_resident: DevBuf::share, nothing copied) and builds the mask-dependent part for its own masks with the stages
// insider_hip_create_ex runs (build_masked).
struct DataSet {
    int device = 0;
    int n_simd = 1024;                // SIMDs of the device (4 per CU)
    int64_t n = 0, p = 0, ldn = 0, ldp = 0;
    int c = 0, SL = 0, SLP = 0;       // SL: rows of the stacked row factors = all levels of all covariates + m
    int m = 0, SLcat = 0;             // continuous covariates (columns of ctns_confounder) and the categorical level total
    std::vector<int> n_levels, lvl_off;   // lvl_off has c + 1 entries
    DevBuf<double> X;                 // gene-major lines of pitch ldn
    DevBuf<uint8_t> codes;            // mask codes, same layout
    DevBuf<int> lev, lvl_off_d, members_all, lvl_ptr_all, lvl_count_all;
    std::vector<CovTables> cov;
    CovTables cont;                   // chunk tables shared by every continuous column
    DevBuf<double> Zc;                // m x n
    DevBuf<int> one_count;            // a "member count" of 1 for the single pseudo-level of a continuous column
    DevBuf<int> ident_members;        // 0..n-1
    int max_chunks = 0, max_L = 0, max_items = 0;
    DevBuf<double> S, yy_train, yy_all;
    DevBuf<double> Strain;            // per-level sums of X over TRAIN entries (p x SLP).  Its continuous columns are written, and
                                      // read, only with cont_merged (k_zt_build: S - S^held); zero otherwise
    DevBuf<double> Sheld;             // S - Strain: per-level sums over the held-out entries (continuous columns, cont_merged:
                                      // the sums of x z over the held-out list; without cont_merged they equal S and nothing reads them)
    double cnt_train = 0, cnt_test = 0;
    bool no_na = false;               // every entry is train or test: held-out == test
    // held-out lists (element index, value) of every gene (col) and of every sample (row); padded to LIST_ALIGN
    DevBuf<uint32_t> col_ptr, row_ptr;
    DevBuf<int> col_idx, row_idx;
    DevBuf<double> col_val, row_val;
    DevBuf<uint8_t> col_flag;         // per column-side list entry: 1 = test entry (only kept when the data has NA entries)
    uint64_t col_entries = 0, row_entries = 0;
    bool merged = false;              // the merged masked row update is available (categorical covariates only)
    // factored column statistics (insider_col_factored.hpp)
    ColFacArgs cf;                    // its static part
    int cf_pos[CF_MAXC] = {0};        // position of covariate i in cf's order (decreasing level count)
    bool cf_pair_ok = false;
    DevBuf<uint8_t> cf_cnt;           // dense pair counts of every gene (pair-count form)
    DevBuf<float> cf_hn;              // 1/2 held-out count per (gene, level) in the pair-count kernel's order (ColFacArgs::hn)
    DevBuf<double> cf_sq;             // S and S^held per (gene, level) in k_col_paircnt4's order (ColFacArgs::sq; categorical covariates only)
    DevBuf<double> cf_zt;             // real-valued counts of the continuous covariates in the same order (ColFacArgs::zt), m <= 4
    // merged row update with continuous covariates (m <= 4, real-valued counts ColFacArgs::zt): column k is a ONE-level
    // covariate whose membership weights are z_rk — its (gene, weight) list carries sum_{r in H(j)} z_rk^2, its pair "counts"
    // sum_{r in l} z_rk per categorical level and (Z'Z)[k][k'] per other column, its |l| = sum_r z_rk^2.  The columns' lists
    // are the same (every gene): one copy, contm_lists; contm[k] holds the weights and pair counts of column k
    std::vector<CovTables> contm;
    CovTables contm_lists;
    DevBuf<double> cont_cnt;          // [m] sum_r z_rk^2
    bool cont_merged = false;
    // mask-independent: the pair "counts" of continuous column k (contm[k].paircnt holds the same allocation)
    std::vector<DevBuf<double>> cont_pair;
    std::shared_ptr<const HostTables> host;
    // fold ids: set after creation (insider_hip_set_folds), read when a handle is derived; a derived data set keeps the ids
    // it was derived under
    mutable std::mutex fold_mu;
    mutable std::shared_ptr<const FoldIds> folds;
    std::shared_ptr<const FoldIds> get_folds() const { std::lock_guard<std::mutex> g(fold_mu); return folds; }
    // device bytes of the DevBufs above: held jointly with the source data set / allocated by this one
    size_t bytes_shared = 0, bytes_own = 0;

    // the row factors as blocks of the stacked factor: covariate b < c, then (m > 0) the continuous columns
    struct Block { int rows, off; };
    int blocks() const { return c + (m > 0 ? 1 : 0); }
    Block block(int b) const { return b < c ? Block{n_levels[b], lvl_off[b]} : Block{m, SLcat}; }

    DataSet() = default;
    DataSet(const DataSet &) = delete;
    DataSet &operator=(const DataSet &) = delete;
    ~DataSet() { (void)hipSetDevice(device); }   // (runs before the members free their buffers)
};

// The factor-dependent WORKSPACE of one handle for the current K (ensure_workspace), and the state that starts over with it.
struct Workspace {
    static constexpr int EARLY = 3;
    int K = 0, NB = 0, KP = 0, nseg = 1;
    int gram_blocks_p = 0, gram_blocks_n = 0, sc_blocks = 0;
    DevBuf<double> Astack, R, C, RtR, CCt, Qfull, SC, stat, stat_col, gram_part, sc_part, lvl_part, eq, lvl_sum;
    DevBuf<double> fperm;             // max(n, p) x KP: the factor rows in k_tile_perm's order (k_list_stats4)
    DevBuf<double> lvl_zero;          // max_L x (STAT + 2 KP + 2) zeros: the (empty) held-out sums of the unmasked row update (unmasked_fused)
    DevBuf<double> Qheld;             // p x KP: sum_l A_l' Sheld[j][l]
    DevBuf<double> U, Ylvl, wpart, Vlev;   // merged row update
    DevBuf<double> lvl_sum_all;       // [SLcat][STAT + 2 KP + 2]: the level records of every covariate
    DevBuf<double> gram_part2, sc_part2;   // partial-sum buffers of the side-stream products
    DevBuf<double> wg_part;           // k_wgemm's per-slab partial sums
    DevBuf<uint8_t> wg_pair;          // packed pair index -> (a, b), a >= b: [2][16 ntile]
    DevBuf<double> sse_train, sse_test, b2, b1, loss_buf, stage;
    size_t stage_count = 0;
    DevBuf<int> sweeps, failflag;
    DevBuf<int> sweep_key;            // smoothed sweep counts: the longest-first scheduling key (k_sched_bucket)
    DevBuf<unsigned long long> sweep_total;
    DevBuf<unsigned> pc4_ticket;      // k_col_paircnt4's gene tickets: counters that only grow
    unsigned pc4_base[2] = {0, 0};    // ... and the value they stand at when the next launch starts: [one counter ? 1 : 0]
    // where the register-resident sweep kernel of the current K keeps its table of code blocks (K <= 32; 0 = not asked yet): the
    // order table holds absolute block addresses (insider_cd_reg.hpp), published by a probe launch of that kernel
    unsigned long long cd_code_base = 0, cd_pair_base = 0;
    DevBuf<unsigned long long> code_base_dev;   // where the probe launch stores them
    uint8_t *order = nullptr;         // the sweep-order table the next column solve reads: one of order_buf
    DevBuf<uint8_t> order_buf[2];     // two tables: the next outer iteration's is built while the current solve runs
    int order_rows = 0;
    // gene scheduling for the CD kernel: genes sorted by the sweep count of their previous solve
    DevBuf<int> gene_perm;
    // the bucket sort behind it (k_sched_bucket / k_sched_scatter): two alternating sets of bucket counters, per gene its bucket
    // and its rank in the bucket
    DevBuf<int> sched_cnt[2], sched_rank;
    DevBuf<uint16_t> sched_bkt;
    int sched_flip = 0;
    // multi-pass column solves in the cold outer iterations (CdParams::sweep_limit): saved state of the unfinished genes,
    // their estimated remaining lengths (two buffers, alternating between passes) and the order of the next pass
    DevBuf<double> cd_hsave, cd_isave;
    DevBuf<uint32_t> cd_pass_slot;
    DevBuf<int> cd_pass_perm[2], cd_pass_cnt;   // cd_pass_cnt: CD_BUCKETS counters + 2 list lengths
    // longest-first gene orders of outer iterations 0..2 of the previous optimize() on this handle: the early iterations
    // of the next call (tune()'s next grid point) have similar per-gene sweep counts, its later ones do not
    DevBuf<int> perm_early[EARLY];
    bool have_early[EARLY] = {false, false, false};
    bool have_perm = false;
};

// events that order the handle's own streams against each other on ONE device: no timing, and no system-scope fence — what one
// stream's kernels wrote must reach the other stream's kernels (device scope: every kernel boundary does that), not the host
constexpr unsigned EV_SYNC = hipEventDisableTiming | hipEventDisableSystemFence;

// A stream join that one function opens and another closes: the event and whether a wait for it is still owed.
struct Join {
    Event ev;
    bool pending = false;
    int record(hipStream_t s) { HIPCHECK(hipEventRecord(ev, s)); pending = true; return INSIDER_OK; }
    int wait(hipStream_t s)           // enqueued only when a record is outstanding
    {
        if (pending) HIPCHECK(hipStreamWaitEvent(s, ev, 0));
        pending = false;
        return INSIDER_OK;
    }
    void drop() { pending = false; }
};

// The streams and events of one handle (each handle, clones included, has its own).
struct Streams {
    Stream stream;
    // scheduling work that nothing but the next column solve needs (sweep keys -> gene order, the next iteration's sweep-order
    // table) runs on a side stream, next to the row update, between two events
    Stream side;
    // the weighted SYRK of the merged row update depends on C only: all covariates' level sums are formed on a second
    // side stream while the main stream computes V, u and U'C
    Stream side2;
    Stream side3;                     // C'C and (S^train C') of the merged row update, next to the weighted SYRK
    Event ev_cd_done, ev_prep, ev_c_ready;
    Event ev_head;                    // recorded on side2 in front of the level Gram GEMM: the main chain's k_gene_u waits for it
    std::vector<Event> ev_w;          // per covariate (and continuous column): its level Gram sums are done
    Event ev_a_ready, ev_tab;
    // the joins of the running optimize() that cross functions: Qfull = S A on the side stream and Qheld = S^held A of the
    // factored column statistics on side3 (phase_R -> launch_col_solve / launch_col_stats); the gene order and sweep-order table
    // on the side stream (launch_col_solve marks it pending, side_close records it, the next launch_col_solve waits)
    Join qfull, qheld, side_done;

    int create(int n_w)
    {
        HIPCHECK(hipStreamCreate(stream.out()));
        for (Stream *s : {&side, &side2, &side3}) HIPCHECK(hipStreamCreateWithFlags(s->out(), hipStreamNonBlocking));
        for (Event *e : {&ev_prep, &ev_c_ready, &ev_head, &ev_a_ready, &qfull.ev, &qheld.ev, &ev_cd_done, &side_done.ev, &ev_tab})
            HIPCHECK(hipEventCreateWithFlags(e->out(), EV_SYNC));
        ev_w.resize(n_w);
        for (Event &e : ev_w) HIPCHECK(hipEventCreateWithFlags(e.out(), EV_SYNC));
        return INSIDER_OK;
    }
    int synchronize_sides() const
    {
        for (const Stream *s : {&side, &side2, &side3}) HIPCHECK(hipStreamSynchronize(*s));
        return INSIDER_OK;
    }
    void synchronize() const
    {
        for (const Stream *s : {&stream, &side, &side2, &side3}) if (*s) (void)hipStreamSynchronize(*s);
    }
};

struct Options {
    int max_sweeps = 1 << 24, order_mode = 0, profile = 0, verbose = 0, cd_variant = 0, force_allreduce = 0;
    int col_factored = 1;             // factored column statistics (insider_col_factored.hpp): 0 list kernel, 1 cost model, 2 look-up form, 3 pair-count form
    int row_counts = 1;               // k_gene_u from the dense pair counts when they exist
    int row_merged = 1;               // use the merged masked row update
    int row_gemm = 1;                 // "row_gemm": weighted SYRK of a many-level covariate as one GEMM over genes (k_wgemm)
    int wg_waves = 1024;              // "row_gemm_waves": waves the GEMM is cut into (sets the number of gene slabs)
    int row_fused = 1;                // "row_fused": level records' tail + equations + solve of the merged update in one launch
    int mm_fast = 1;                  // "mm_fast": the small dense products on k_mm_rows2 / k_mm_reduce2 (default; 2: two column tiles per wave in the reductions)
    int mm_tiles = 0;                 // "mm_tiles": tiles of 16 rows a wave of k_mm_rows2 takes (0, default = mm_tiles_per_wave()'s rule, insider_plan.hpp)
    int col_mfma4 = 1;                // "col_mfma4": pair-count statistics with the second product on v_mfma_f64_4x4x4 (k_col_paircnt4; default)
    int stats_own_q = 1;              // "stats_own_q": k_col_paircnt4 forms Q = S A and Qheld = S^held A itself (stats_own_q, insider_plan.hpp): 1 (default) where a column solve follows, 2 in insider_hip_col_stats too, 0 = the two products over the genes
    int cd_pairs = 1;                 // "cd_pairs": route the sweeps through the kernel's blocks of two coordinate steps (default)
    int list_fine = 1;                // "list_fine": 1 (default) = k_list_stats4 (4x4x4 matrix instruction) where it applies, 0 = k_list_stats
    int cd_cold_iters = 3, cd_pass_first = 64, cd_pass_ratio = 4;   // "cd_cold_iters", "cd_pass1" (0 = single pass), "cd_pass_ratio"
    double resid_stage_mb = 256.0;    // "resid_stage_mb": size of the device buffer the residual is copied out through
    // "vd_stage_kb" bounds the LDS a block of k_vd_stats may stage its genes' level tables in (KiB)
    double vd_stage_kb = 48.0;
    int sd_slabs = 0;                 // "sd_slabs": gene slabs of k_sd_stats (0 = automatic; at most 256)
    int ls_slabs = 0;                 // "ls_slabs": gene slabs of k_ls_prod (0 = automatic; at most 256)
    double ls_part_mb = 256.0;        // "ls_part_mb": bound (MB) on the slabs' partial scores of the automatic slab count
    int glm_slabs = 0;                // "glm_slabs": gene slabs of k_resid_stats (0 = automatic; at most 64)
    int rc_slabs = 0;                 // "rc_slabs": gene slabs of k_rc_fwd (0 = automatic; at most 256)
};

// device workspace of the post-hoc calls (section "post-hoc interaction GLM"): grown on demand, freed with the handle
struct PostWs {
    // Ast: stacked row factors (SL x KPW, blocks not subtracted zero); U: n x KPW; cp: p x KPW; nz: K flags;
    // part: slab partials of the per-sample statistics; stats: n x (K + 1); stage: residual copy-out buffer;
    // gpart / gram: C C'; ints: host-built group tables; cpart / gsum: group sums; L / dinv / info: the factor;
    // outs: coeff, se, dof
    DevBuf<double> Ast, U, cp, part, stats, stage, gpart, gram, cpart, gsum, L, dinv, outs;
    DevBuf<int> nz, ints, info;
    // vin = the host factors as upload_factors leaves them (A blocks at row offset x K, then C as p rows of K).  Variance
    // decomposition: vtab = the level table T (p rows of SL); vrec = the p records
    DevBuf<double> vin, vtab, vrec;
    // sample decomposition: spart = the slabs' partial records (slabs x n x (4 + 3 BW)); srec = the n records
    DevBuf<double> spart, srec;
    // level scores: lcand = the candidates (L x KPW); ltab = the candidate table Tc (p rows of ldt); lpart / lcnt = the slabs'
    // partial scores (slabs x n x ldt) and counts (slabs x n); lout = sse (n x L column-major), then cnt (n)
    DevBuf<double> lcand, ltab, lpart, lcnt, lout;
    // factor decomposition: fwall = [W | W .* W] (padded rows x 2 ldq); fprod = the p rows [P1 | P2 | P3]; fbase = the p base
    // slots; frec = the p records
    DevBuf<double> fwall, fprod, fbase, frec;
    // residual products: rq = Q (n rows of ldq); rcs = the p pairs (centre, inverse scale); rz = Z (p rows of ldq); rpart = the
    // slabs' partial Y (slabs x n x ldq); rin = the caller's Q, centre and scale as they came; rout = Z (p x q column-major),
    // Y (n x q column-major), rss (p)
    DevBuf<double> rq, rcs, rz, rpart, rin, rout;
    // outlier calls: ocs = center (p; unused without one) then scale (p); obits = the bitmap of flagged entries (p x ldn / 32
    // words); ogcnt / oscnt = the p / n pairs {low, high}; ooffs = the p + 1 list offsets; orows / ocols / oz = the list
    DevBuf<double> ocs, oz;
    DevBuf<uint32_t> obits;
    DevBuf<int> ogcnt, oscnt, orows, ocols;
    DevBuf<long long> ooffs;
};

}  // namespace

struct insider_hip_handle {
    std::shared_ptr<const DataSet> ds;
    Streams st;
    Options opt;
    Workspace ws;
    // post-hoc interaction GLM / residual / variance and sample decomposition: a workspace of its own, so that nothing
    // insider_hip_optimize() reads is touched
    PostWs post;
    // state of the running optimize() (its pending stream joins: Streams)
    FitPlan plan;                     // the kernel path of the call that is running, or ran last (plan_call)
    bool w_ready = false;
    bool prep_joined = false;         // the main stream is already ordered behind this iteration's ev_prep (join_side)
    // sharding
    int64_t gene_offset = 0;
    int rank = 0, world = 1;
    insider_allreduce_fn allreduce = nullptr;
    void *allreduce_user = nullptr;
    ncclComm_t comm = nullptr;        // RCCL communicator over the gene-sharded ranks (insider_hip_comm_init); owned
    // profile of the last optimize()
    std::vector<Event> ev_col, ev_row, ev_cd, ev_test;
    double prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double steady_cd_ms = 0, steady_col_ms = 0;   // means over the outer iterations >= 5 of the last profiled optimize()
    // of the last optimize() / optimize_col(): genes whose elastic-net solve was ended by max_sweeps, not by convergence
    // (the reference has no cap, src/coordinate_descent.cpp:86-114), and the longest solve in sweeps
    int cap_hits = 0, max_gene_sweeps = 0;
    // of the last column solve: the kernel that ran the solve and the one that ran the evaluation pass after it (ColSolver), and
    // whether the ridge solve launched the general-route fallback for the genes the register kernel marked
    int col_solver = 0, col_eval = 0, col_ridge_fallback = 0;
    // of the last column-side statistics launch (launch_col_stats): the kernel that formed them (ColStatsKernel), and for
    // k_col_paircnt4 the ticket counters it drew from and its grid size (0 for the other kernels)
    int col_stats_kernel = 0, col_stats_tickets = 0, col_stats_blocks = 0;
    int col_stats_own_q = 0;          // ... and whether it formed Q = S A and Qheld = S^held A itself (FitPlan::stats_own_q)
    // of the last Q = S A / Qheld = S^held A product (launch_q): 1 = k_mm_rows, 2 = k_mm_rows2; and tiles_per_wave of the
    // last k_mm_rows2 launch from either site (launch_q, launch_gene_v)
    int col_q_kernel = 0, mm_rows2_tiles = 0;
    // of the last optimize() / optimize_row(): one bit per row-phase kernel form it launched (RowKernel)
    uint64_t row_kernels = 0;
    // the form the last variance decomposition ran (1 = tables in LDS, 2 = from global)
    int vd_path = 0;
    // the form the last sample decomposition ran (1 = tables in LDS, 2 = from global) and its gene slabs
    int sd_path = 0, sd_slabs = 0;
    // the form the last level scores ran (1 = one level window, 2 = several) and its gene slabs
    int ls_path = 0, ls_slabs = 0;
    // of the last interaction GLM: the gene slabs of k_resid_stats and its form, 10 NB + GT
    int glm_slabs = 0, glm_form = 0;
    int fd_path = 0;
    // the (QT, KS) instantiation of the heavy launch of the last level scores (k_ls_prod), factor decomposition (k_fd_prod with
    // the residual), residual products (k_rc_back / k_rc_fwd), as 10 QT + KS, and of the last co-expression (k_cx_stage), KS
    int ls_form = 0, fd_form = 0, rc_form = 0, cx_form = 0;
    // of the last residual products: the gene slabs of k_rc_fwd (0: no forward pass) and the HIP-event time of its kernels
    int rc_slabs = 0;
    double rc_ms = 0.0;
    // of the last co-expression call: the staged megabytes and the HIP-event times of the staging kernels (k_cx_stage,
    // k_cx_norm / k_cx_std_pc) and of the product kernel (k_cx_topk: cx_ms; k_cx_topk_pc, the pairwise-complete form: cx_pc_ms)
    double cx_stage_mb = 0.0, cx_stage_ms = 0.0, cx_ms = 0.0, cx_pc_ms = 0.0;
    // the form the flag pass of the last outlier call ran (1 = tables in LDS, 2 = from global)
    int ol_path = 0;

    // work still in flight is drained and the communicator closed before the members free their buffers (the data set with
    // its last handle)
    ~insider_hip_handle()
    {
        if (ds) (void)hipSetDevice(ds->device);
        st.synchronize();
        if (comm) (void)ncclCommDestroy(comm);
    }
};

namespace {

// the kernel forms the row phase can launch, as insider_hip_get_info("row_kernels") reports them: bit RK_* is set on the host
// where its form is launched (include/insider_hip.h; insider_amd/_lib.py ROW_KERNELS names them in this order)
enum RowKernel {
    RK_WGEMM4 = 0, RK_WGEMM5, RK_WGEMM6, RK_WGEMM7, RK_WGEMM_CHUNKS, RK_WSYRK, RK_GRAM_SIDE,   // level Gram sums
    RK_GENE_U_CNT, RK_GENE_U, RK_GENE_UC,                                                       // u
    RK_MERGED_SOLVE, RK_MERGED, RK_MERGED_ZERO, RK_PACK_REDUCE,                                 // record tail + equations (+ solve)
    RK_LIST_STATS4, RK_LIST_STATS, RK_LEVEL_PARTIAL, RK_LEVEL_SOLVE, RK_CONT_CD,               // per-sample statistics, solves
    RK_MM_ROWS2, RK_MM_ROWS, RK_MM_REDUCE2_2, RK_MM_REDUCE2_4, RK_MM_REDUCE                     // V = C A', Y = U'C
};
inline uint64_t rk_bit(RowKernel k) { return 1ull << (int)k; }
inline void row_mark(insider_hip_handle *h, RowKernel k) { h->row_kernels |= rk_bit(k); }

// the facts of handle h for a call with K factors (the workspace's geometry as it stands: none before the first call)
PlanFacts plan_facts(const insider_hip_handle *h, int K)
{
    const DataSet &d = *h->ds;
    PlanFacts f;
    const Options &o = h->opt;
    f.opt = {o.row_merged, o.col_factored, o.row_fused, o.row_gemm, o.row_counts, o.mm_fast, o.force_allreduce, o.wg_waves,
             o.list_fine, o.mm_tiles, o.col_mfma4, o.cd_variant, o.cd_pairs, o.cd_cold_iters, o.cd_pass_first, o.cd_pass_ratio, o.max_sweeps,
             o.stats_own_q};
    f.world = h->world; f.n_simd = d.n_simd;
    f.K = K; f.NB = h->ws.NB; f.KP = h->ws.KP; f.lvl_zero = (bool)h->ws.lvl_zero; f.fperm = (bool)h->ws.fperm;
    f.merged = d.merged; f.cont_merged = d.cont_merged; f.cf_pair_ok = d.cf_pair_ok; f.cf_hn = (bool)d.cf_hn; f.cf_zt = (bool)d.cf_zt; f.cf_sq = (bool)d.cf_sq;
    f.c = d.c; f.m = d.m; f.SL = d.SL; f.SLP = d.SLP; f.SLcat = d.SLcat; f.n = d.n; f.p = d.p; f.col_entries = d.col_entries; f.row_entries = d.row_entries;
    for (const CovTables &ct : d.cov) { f.L.push_back(ct.L); f.npairs.push_back(ct.npairs); }
    f.cf_c = d.cf.c; f.cf_tab_rows = d.cf.tab_rows; f.cf_nsteps = d.cf.nsteps;
    std::copy(d.cf.L, d.cf.L + CF_MAXC + 1, f.cf_L);
    std::copy(d.cf.nlater, d.cf.nlater + CF_MAXC + 1, f.cf_nlater);
    return f;
}

int ensure_workspace(insider_hip_handle *h, int K)
{
    if (K < 1 || K > INSIDER_MAX_K) return fail(INSIDER_ERR_UNSUPPORTED, "K must be in 1..63");
    if (h->ws.K == K) return INSIDER_OK;
    h->ws = Workspace();   // the old buffers go first: two workspaces are never held at once
    const DataSet &d = *h->ds;
    const hipStream_t st = h->st.stream;
    Workspace w;
    const int NB = (K + 1 + 15) / 16, KP = 16 * NB, NBLK = NB * (NB + 1) / 2, STAT = NBLK * 256;
    w.NB = NB;
    w.KP = KP;
    // row-side segmentation: enough work items to fill 256 CUs even for few samples: split long lists into up to 64 segments
    const int64_t avg_batches = (int64_t)(d.row_entries / (uint64_t)LIST_ALIGN / (uint64_t)std::max<int64_t>(d.n, 1));
    int nseg = (int)std::min<int64_t>(std::max<int64_t>(1, cdiv(8192, d.n)), std::max<int64_t>(1, avg_batches / 16));
    nseg = std::min(nseg, 64);
    w.nseg = nseg;
    w.gram_blocks_p = cdiv(d.p, MM_SLAB);
    w.gram_blocks_n = cdiv(d.n, MM_SLAB);
    w.sc_blocks = cdiv(d.p, MM_SLAB);
    const size_t rec = STAT + 2 * KP + 2, max_L = std::max(d.max_L, 1);
    int rc;
    // 16 rows of zero padding: the pair-count statistics kernel reads whole blocks of 16 levels without clamping
    if ((rc = w.Astack.alloc((size_t)(d.SL + 16) * KP))) return rc;
    HIPCHECK(hipMemset(w.Astack, 0, (size_t)(d.SL + 16) * KP * sizeof(double)));
    if ((rc = w.R.alloc((size_t)d.n * KP))) return rc;
    if ((rc = w.C.alloc((size_t)(std::max<int64_t>(d.p, d.ldp) + 4) * KP))) return rc;   // + 4 zero rows: k_wgemm reads whole steps of four genes
    if ((rc = w.RtR.alloc((size_t)KP * KP))) return rc;
    if ((rc = w.CCt.alloc((size_t)KP * KP))) return rc;
    if ((rc = w.Qfull.alloc((size_t)d.p * KP))) return rc;
    if ((rc = w.SC.alloc((size_t)d.SL * KP))) return rc;
    if ((rc = w.stat.alloc((size_t)nseg * d.n * STAT))) return rc;
    if ((rc = w.stat_col.alloc((size_t)d.p * STAT))) return rc;
    if ((rc = w.gram_part.alloc((size_t)std::max(w.gram_blocks_p, w.gram_blocks_n) * KP * KP))) return rc;
    if ((rc = w.sc_part.alloc((size_t)w.sc_blocks * d.SL * KP))) return rc;
    if ((rc = w.lvl_part.alloc((size_t)d.max_chunks * rec))) return rc;
    if ((rc = w.lvl_sum.alloc(max_L * rec))) return rc;
    if (NB == 2 && K >= 16)   // (the statistics kernels that read it exist for 16 <= K <= 31)
        if ((rc = w.fperm.alloc((size_t)std::max(d.n, d.p) * KP))) return rc;
    if ((rc = w.lvl_zero.alloc(max_L * rec))) return rc;
    HIPCHECK(hipMemsetAsync(w.lvl_zero, 0, max_L * rec * sizeof(double), st));
    if (d.merged) {
        // k_wgemm (weighted SYRK as a GEMM over genes): partial sums per gene slab, and the packed pair index -> (a, b) table
        size_t wg_len = 0;
        int wg_ntile = 0;
        const PlanFacts facts = plan_facts(h, K);
        for (int i = 0; i < d.c; ++i) {
            const WgPlan g = wgemm_plan(facts, i, true);
            if (g.use) {
                wg_len = std::max(wg_len, (size_t)g.nslab * (16 * g.tiles) * (16 * g.ntile));
                wg_ntile = g.ntile;
            }
        }
        if (wg_len) {
            if ((rc = w.wg_part.alloc(wg_len))) return rc;
            std::vector<uint8_t> ab((size_t)2 * 16 * wg_ntile, (uint8_t)(KP - 1));   // padded pairs: column KP - 1 of C, always zero
            int idx = 0;
            for (int a = 0; a < K; ++a)
                for (int b = 0; b <= a; ++b, ++idx) {
                    ab[idx] = (uint8_t)a;
                    ab[(size_t)16 * wg_ntile + idx] = (uint8_t)b;
                }
            if ((rc = w.wg_pair.upload(ab))) return rc;
        }
        if ((rc = w.U.alloc((size_t)d.p * round_up(max_L, 2)))) return rc;
        if ((rc = w.Ylvl.alloc(max_L * KP))) return rc;
        if ((rc = w.wpart.alloc((size_t)std::max(d.max_items, 1) * STAT))) return rc;
        if ((rc = w.lvl_sum_all.alloc((size_t)std::max(d.SL, 1) * rec))) return rc;
        if ((rc = w.gram_part2.alloc((size_t)std::max(w.gram_blocks_p, w.gram_blocks_n) * KP * KP))) return rc;
        if ((rc = w.sc_part2.alloc((size_t)w.sc_blocks * d.SL * KP))) return rc;
        if ((rc = w.Vlev.alloc((size_t)d.p * d.SLP))) return rc;
        HIPCHECK(hipMemsetAsync(w.Vlev, 0, (size_t)d.p * d.SLP * sizeof(double), st));   // (columns are filled as they are first needed)
        if ((rc = w.Qheld.alloc((size_t)d.p * KP))) return rc;
    }
    if ((rc = w.eq.alloc((size_t)d.max_L * (KP * KP + KP)))) return rc;
    for (DevBuf<double> *b : {&w.sse_train, &w.sse_test, &w.b2, &w.b1})
        if ((rc = b->alloc((size_t)d.p))) return rc;
    if ((rc = w.loss_buf.alloc(8))) return rc;
    w.stage_count = (size_t)std::max<int64_t>(std::max<int64_t>(d.p, d.n), d.SL) * KP;
    if ((rc = w.stage.alloc(w.stage_count))) return rc;
    if ((rc = w.sweeps.alloc((size_t)d.p))) return rc;
    // [0] a system was singular, [1] ridge genes wait for the general route, [2] genes stopped by max_sweeps, [3] longest solve
    if ((rc = w.failflag.alloc(4))) return rc;
    if ((rc = w.sweep_total.alloc(256))) return rc;
    if ((rc = w.pc4_ticket.alloc((size_t)(PC4_PARTS + 1) * 32))) return rc;   // (a 128-byte line per counter)
    HIPCHECK(hipMemsetAsync(w.pc4_ticket, 0, (size_t)(PC4_PARTS + 1) * 32 * sizeof(unsigned), st));
    if ((rc = w.gene_perm.alloc((size_t)d.p))) return rc;
    if ((rc = w.sched_cnt[0].alloc((size_t)SCHED_BUCKETS))) return rc;
    if ((rc = w.sched_cnt[1].alloc((size_t)SCHED_BUCKETS))) return rc;
    if ((rc = w.sched_rank.alloc((size_t)d.p))) return rc;
    if ((rc = w.sched_bkt.alloc((size_t)d.p))) return rc;
    if ((rc = w.sweep_key.alloc((size_t)d.p))) return rc;
    if ((rc = w.cd_hsave.alloc((size_t)d.p * KP))) return rc;
    if ((rc = w.cd_isave.alloc((size_t)d.p * KP))) return rc;
    if ((rc = w.cd_pass_slot.alloc((size_t)d.p))) return rc;
    if ((rc = w.cd_pass_perm[0].alloc((size_t)d.p))) return rc;
    if ((rc = w.cd_pass_perm[1].alloc((size_t)d.p))) return rc;
    if ((rc = w.cd_pass_cnt.alloc((size_t)CD_BUCKETS + 2))) return rc;
    if ((rc = w.code_base_dev.alloc(2))) return rc;
    for (DevBuf<int> &b : w.perm_early)
        if ((rc = b.alloc((size_t)d.p))) return rc;
    HIPCHECK(hipMemsetAsync(w.sched_cnt[0], 0, SCHED_BUCKETS * sizeof(int), st));
    HIPCHECK(hipMemsetAsync(w.sched_cnt[1], 0, SCHED_BUCKETS * sizeof(int), st));
    // rows of the padded factor buffers beyond K must stay zero: C rows are gathered with pitch KP and the
    // pad genes of the transposed layout index rows p..ldp-1
    HIPCHECK(hipMemsetAsync(w.C, 0, (size_t)(std::max<int64_t>(d.p, d.ldp) + 4) * KP * sizeof(double), st));
    HIPCHECK(hipMemsetAsync(w.R, 0, (size_t)d.n * KP * sizeof(double), st));
    HIPCHECK(hipMemsetAsync(w.failflag, 0, 4 * sizeof(int), st));
    w.K = K;
    h->ws = std::move(w);
    return INSIDER_OK;
}

// ---- launch helpers (dispatch on NB) -----------------------------------------------------------------------
#define NB_DISPATCH(NBV, ...)                                                           \
    switch (NBV) {                                                                      \
        case 1: { constexpr int NB_ = 1; constexpr int WPB_ = 4; __VA_ARGS__; } break;   \
        case 2: { constexpr int NB_ = 2; constexpr int WPB_ = 4; __VA_ARGS__; } break;   \
        case 3: { constexpr int NB_ = 3; constexpr int WPB_ = 2; __VA_ARGS__; } break;   \
        default: { constexpr int NB_ = 4; constexpr int WPB_ = 1; __VA_ARGS__; } break;  \
    }

// the post-hoc and embedding kernels' forms per number of 16-column tiles of K (1..4): the body sees it as KT_
#define KT_DISPATCH(KTV, ...)                                   \
    switch (KTV) {                                              \
        case 1: { constexpr int KT_ = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int KT_ = 2; __VA_ARGS__; } break;  \
        case 3: { constexpr int KT_ = 3; __VA_ARGS__; } break;  \
        default: { constexpr int KT_ = 4; __VA_ARGS__; } break; \
    }

// mark: when given, the bit of the form launched (RK_LIST_STATS4 / RK_LIST_STATS) is or'ed into it
int launch_list_stats(insider_hip_handle *h, bool cols, int nseg, const double *F, double *stat,
                      const double *base = nullptr, uint64_t *mark = nullptr)
{
    const int units = cols ? (int)h->ds->p : (int)h->ds->n;
    const int64_t f_rows = cols ? h->ds->n : h->ds->p;
    const uint32_t *ptr = cols ? h->ds->col_ptr : h->ds->row_ptr;
    const int *lidx = cols ? h->ds->col_idx : h->ds->row_idx;
    const double *lval = cols ? h->ds->col_val : h->ds->row_val;
    const int64_t items = (int64_t)units * nseg;
    if (h->plan.list4) {
        const int NT = (h->ws.K + 4) / 4;
        // the rows in the tile-pair order the kernel's 16-byte loads want (a copy: every other consumer keeps F's order)
        hipLaunchKernelGGL(k_tile_perm, dim3(cdiv(f_rows * h->ws.KP, 256)), dim3(256), 0, h->st.stream, F, f_rows, h->ws.KP, h->ws.fperm);
#define LS4(NT_)                                                                                                               \
    hipLaunchKernelGGL((k_list_stats4<2, NT_, 4>), dim3(cdiv(items, 4)), dim3(256), 0, h->st.stream, ptr, lidx, lval, units, nseg,   \
                       (const double *)h->ws.fperm, f_rows, stat, base, h->ws.K)
        switch (NT) {
            case 5: LS4(5); break;
            case 6: LS4(6); break;
            case 7: LS4(7); break;
            default: LS4(8); break;
        }
#undef LS4
        KCHECK();
        if (mark) *mark |= rk_bit(RK_LIST_STATS4);
        return INSIDER_OK;
    }
    NB_DISPATCH(h->ws.NB, hipLaunchKernelGGL((k_list_stats<NB_, WPB_>), dim3(cdiv(items, WPB_)), dim3(WPB_ * 64), 0,
                                           h->st.stream, ptr, lidx, lval, units, nseg, F, f_rows, stat, base, h->ws.K));
    KCHECK();
    if (mark) *mark |= rk_bit(RK_LIST_STATS);
    return INSIDER_OK;
}

// ---- the small dense products on MFMA (insider_mm.hpp) -------------------------------------------------------------------
// out[p x KP] = Sx[p x SL] Astack[SL x KP] for Sx = S (Q) or S^held (Qheld): p rows of pitch SLP   (Astack row-major with pitch KP)
int launch_q(insider_hip_handle *h, const double *X, double *out, hipStream_t st = nullptr)
{
    if (!st) st = h->st.stream;
    const int64_t ldx = h->ds->SLP;
    const int M = (int)h->ds->p, Kd = h->ds->SL;
    const double *W = h->ws.Astack;
    if (h->plan.q_rows2) {
        const int tiles = cdiv(M, 16), tpw = h->plan.mm_tpw;
        const size_t lds2 = (size_t)4 * cdiv(Kd, 16) * h->ws.NB * 64 * sizeof(double);   // W staged in LDS
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_mm_rows2<NB_, false>), dim3(cdiv(cdiv(tiles, tpw), 4), 1), dim3(256), lds2, st, X, ldx, M, Kd, W,
                               h->ws.KP, h->ws.KP, out, (int64_t)h->ws.KP, h->ws.KP, tpw);
        });
        KCHECK();
        h->col_q_kernel = 2;
        h->mm_rows2_tiles = tpw;
        return INSIDER_OK;
    }
    NB_DISPATCH(h->ws.NB, {
        (void)WPB_;
        hipLaunchKernelGGL((k_mm_rows<NB_, false>), dim3(cdiv(cdiv(M, 16), 4), 1), dim3(256), 0, st, X, ldx, M, Kd, W,
                           h->ws.KP, h->ws.KP, out, (int64_t)h->ws.KP, h->ws.KP);
    });
    KCHECK();
    h->col_q_kernel = 1;
    return INSIDER_OK;
}

// part[slab][L][KP] = sum over slabs of MM_SLAB rows of X[m][l] Y[m][n], then the fixed-order sum over slabs -> out[L][KP]
// out == nullptr: the partial sums are left in `part` for the consumer to add up (k_level_merged); returns the slab count in *nslab
// mark: when given, the bit of the form launched (RK_MM_REDUCE2_2 / RK_MM_REDUCE2_4 / RK_MM_REDUCE) is or'ed into it
int launch_mm_reduce_kp(insider_hip_handle *h, const double *X, int64_t ldx, const double *Y, int M, int L, double *part,
                        double *out, hipStream_t st = nullptr, int *nslab = nullptr, uint64_t *mark = nullptr)
{
    if (!st) st = h->st.stream;
    const int slabs = cdiv(M, MM_SLAB);
    if (nslab) *nslab = slabs;
    const ReduceForm form = reduce_form(h->plan, M, L);
    if (form != MR_REDUCE) {
        const int lt = cdiv(L, 16);
#define MR2(NBV, LTV)                                                                                                         \
    hipLaunchKernelGGL((k_mm_reduce2<NBV, LTV>), dim3(slabs, cdiv(lt, LTV)), dim3(64), 0, st, X, ldx, Y, (int64_t)h->ws.KP, M,   \
                       MM_SLAB, L, h->ws.KP, part, h->ws.KP)
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            if (form == MR_REDUCE2_2) {
                MR2(NB_, 2);
                if (mark) *mark |= rk_bit(RK_MM_REDUCE2_2);
            } else {
                MR2(NB_, 4);
                if (mark) *mark |= rk_bit(RK_MM_REDUCE2_4);
            }
        });
#undef MR2
    } else {
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_mm_reduce<NB_>), dim3(slabs, cdiv(L, 16)), dim3(64), 0, st, X, ldx, Y, (int64_t)h->ws.KP, M,
                               MM_SLAB, L, h->ws.KP, part, h->ws.KP);
        });
        if (mark) *mark |= rk_bit(RK_MM_REDUCE);
    }
    KCHECK();
    if (out)
        hipLaunchKernelGGL(k_sum_partials, dim3(cdiv(L * h->ws.KP, 16)), dim3(256), 0, st, (const double *)part, slabs,
                           L * h->ws.KP, out);
    KCHECK();
    return INSIDER_OK;
}

// the row16 kernel with three slots keeps up to 4 x 48 x 48 doubles of Gram matrices per wave in LDS (72 KB): beyond the 64 KB a
// kernel may ask for dynamically without opting in
int r16_wide_lds(size_t bytes)
{
    if (bytes > 160 * 1024) return fail(INSIDER_ERR_UNSUPPORTED, "K too large for the LDS-resident sweep kernel");
    // the attribute belongs to the CURRENT device's function object: one flag per device (a process may drive several GPUs)
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    HIPCHECK(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (dev >= 64 || !(done.load() & bit)) {
        const int lim = 160 * 1024;
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cd_cols_r16<3>), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
        done.fetch_or(bit);
    }
    return INSIDER_OK;
}

int launch_gram(insider_hip_handle *h, const double *F, int64_t rows, double *out, hipStream_t st = nullptr,
                double *part = nullptr)
{
    return launch_mm_reduce_kp(h, F, h->ws.KP, F, (int)rows, h->ws.KP, part ? part : h->ws.gram_part, out, st);
}

int launch_build_R(insider_hip_handle *h)
{
    hipLaunchKernelGGL(k_build_R, dim3(cdiv(h->ds->n * h->ws.KP, 256)), dim3(256), 0, h->st.stream, (const int *)h->ds->lev,
                       (const int *)h->ds->lvl_off_d, h->ds->c, (int)h->ds->n, (const double *)h->ws.Astack, h->ws.KP,
                       (const double *)h->ds->Zc, h->ds->m, h->ds->SLcat, h->ws.R);
    KCHECK();
    return INSIDER_OK;
}

// R, R'R and Qfull from the current row factors (src/optimize.cpp:365-369 and the Xty of :222,235 via level sums)
// use_side: Qfull, which only the column solve reads, is formed on the side stream next to R'R and the column statistics
// r_is_current: the row updates have just rebuilt R (every row_update() ends with k_build_R): do not build it again
int phase_R(insider_hip_handle *h, bool use_side = false, bool r_is_current = false, bool want_qheld = false)
{
    // the statistics kernel forms Q and Qheld itself (FitPlan::stats_own_q; every masked call launches it behind this): no
    // product over the genes, no side stream, no join
    const bool own_q = h->plan.stats_own_q;
    if (use_side && !own_q) {
        HIPCHECK(hipEventRecord(h->st.ev_a_ready, h->st.stream));
        // Qheld = S^held A, which the factored column statistics read: on the third stream (idle since the row phase's C'C),
        // beside R'R on the main one instead of behind it, and beside Qfull on the side stream (Qfull behind Qheld: DESIGN §4.5)
        HIPCHECK(hipStreamWaitEvent(h->st.side, h->st.ev_a_ready, 0));
        if (want_qheld && h->ws.Qheld && h->plan.col_path != 0) {
            HIPCHECK(hipStreamWaitEvent(h->st.side3, h->st.ev_a_ready, 0));
            if (int rh = launch_q(h, h->ds->Sheld, h->ws.Qheld, h->st.side3)) return rh;
            if (int rh = h->st.qheld.record(h->st.side3)) return rh;
        }
        int rq = launch_q(h, h->ds->S, h->ws.Qfull, h->st.side);
        if (rq) return rq;
        if ((rq = h->st.qfull.record(h->st.side))) return rq;
    }
    int rc = r_is_current ? INSIDER_OK : launch_build_R(h);
    if (rc) return rc;
    rc = launch_gram(h, h->ws.R, h->ds->n, h->ws.RtR);
    if (rc) return rc;
    if (use_side || own_q) return INSIDER_OK;
    return launch_q(h, h->ds->S, h->ws.Qfull);
}

struct Timer {   // HIP-event pair around one launch on the library's stream (option "profile")
    Event e0, e1;
    int begin(insider_hip_handle *h, bool on)
    {
        if (!on || !h->opt.profile) return INSIDER_OK;
        // timing only: no system-scope fence (the cache write-back and invalidation it brings cost the FOLLOWING kernel ~20 us behind
        // a statistics launch that has just written 300 MB; nothing reads these events' work from the host)
        HIPCHECK(hipEventCreateWithFlags(e0.out(), hipEventDisableSystemFence));
        HIPCHECK(hipEventCreateWithFlags(e1.out(), hipEventDisableSystemFence));
        HIPCHECK(hipEventRecord(e0, h->st.stream));
        return INSIDER_OK;
    }
    int end(insider_hip_handle *h, std::vector<Event> &into)
    {
        if (!e0) return INSIDER_OK;
        HIPCHECK(hipEventRecord(e1, h->st.stream));
        into.push_back(std::move(e0));
        into.push_back(std::move(e1));
        return INSIDER_OK;
    }
};

// the kernel time a call reports (insider_hip_last_*_ms, "rc_ms"): a pair of default-flag HIP events on the call's stream
struct Stopwatch {
    Event e0, e1;
    bool marked = false;
    int start(hipStream_t st)   // (a second start reuses the pair: the batch CD entry times every chunk)
    {
        if (!e0) {
            HIPCHECK(hipEventCreate(e0.out()));
            HIPCHECK(hipEventCreate(e1.out()));
        }
        marked = false;
        HIPCHECK(hipEventRecord(e0, st));
        return INSIDER_OK;
    }
    // the end of the timed stretch alone, for a call that enqueues more work before the host may wait
    int mark(hipStream_t st)
    {
        HIPCHECK(hipEventRecord(e1, st));
        marked = true;
        return INSIDER_OK;
    }
    // marks the end unless mark() did, waits for it and reads the time (0 when the runtime cannot give one)
    int stop_ms(hipStream_t st, float *ms)
    {
        if (!marked)
            if (int rc = mark(st)) return rc;
        HIPCHECK(hipEventSynchronize(e1));
        *ms = 0.0f;
        (void)hipEventElapsedTime(ms, e0, e1);
        return INSIDER_OK;
    }
};

// the elastic-net parameters as the kernels take them: the column update's and the batch entry's
static CdParams cd_params(double lambda, double alpha, double tol, int max_sweeps, const uint8_t *order)
{
    CdParams c;
    c.lambda = lambda;
    c.alpha = alpha;
    c.tol = tol;
    c.la = lambda * alpha;
    c.l2 = lambda * (1.0 - alpha);
    c.two_la = 2.0 * c.la;
    c.inv_two_la = c.la > 0.0 ? 0.5 / c.la : 0.0;
    c.max_sweeps = max_sweeps;
    c.order = order;
    return c;
}

// one launch of the elastic-net kernel s over the a.p genes of `a` (a.mode: the solve or, outside the register-resident
// kernel, the evaluation only)
static int launch_cd(ColSolver s, const ColArgs &a, hipStream_t st)
{
    const size_t r16_bytes = (size_t)r16_lds_doubles(a.K) * sizeof(double);
    switch (s) {
        case CS_CD_REG:
        case CS_CD_REG3:
            REG_ANY_DISPATCH(a.K, hipLaunchKernelGGL((k_cd_cols_reg<SL_, KM_, true>), dim3(cdiv(a.p, 4)), dim3(64), 0, st, a));
            break;
        case CS_CD_R16_1: hipLaunchKernelGGL((k_cd_cols_r16<1>), dim3(cdiv(a.p, 4)), dim3(64), r16_bytes, st, a); break;
        case CS_CD_R16_2: hipLaunchKernelGGL((k_cd_cols_r16<2>), dim3(cdiv(a.p, 4)), dim3(64), r16_bytes, st, a); break;
        case CS_CD_R16_3:
            if (int rl = r16_wide_lds(r16_bytes)) return rl;
            hipLaunchKernelGGL((k_cd_cols_r16<3>), dim3(cdiv(a.p, 4)), dim3(64), r16_bytes, st, a);
            break;
        case CS_CD_COLS16: hipLaunchKernelGGL((k_cd_cols<16, 4>), dim3(cdiv(a.p, 16)), dim3(256), 0, st, a); break;
        case CS_CD_COLS32: hipLaunchKernelGGL((k_cd_cols<32, 2>), dim3(cdiv(a.p, 4)), dim3(128), 0, st, a); break;
        case CS_CD_COLS64: hipLaunchKernelGGL((k_cd_cols<64, 1>), dim3((unsigned)a.p), dim3(64), 0, st, a); break;
        default: return fail(INSIDER_ERR_ARG, "not an elastic-net solve kernel");
    }
    KCHECK();
    return INSIDER_OK;
}

// The addresses of the table of code blocks [0] and of the blocks of two steps [1] of k_cd_cols_reg<., KMAX(K), true> on the
// current device (reg_pairs(KMAX) only): a probe launch with a null gene set, through the two device words d.
static int probe_code_base(int K, unsigned long long *d, hipStream_t st, unsigned long long (&v)[2])
{
    HIPCHECK(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), st));
    ColArgs a{};
    a.K = K;
    a.code_base = d;
    REG_DISPATCH(K, hipLaunchKernelGGL((k_cd_cols_reg<SL_, KM_, true>), dim3(1), dim3(64), 0, st, a));
    KCHECK();
    v[0] = v[1] = 0;
    HIPCHECK(hipMemcpyAsync(v, d, sizeof(v), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (!v[0] || !v[1]) return fail(INSIDER_ERR_HIP, "the sweep kernel did not publish the addresses of its code blocks");
    return INSIDER_OK;
}

// The sweep-order table (one period of rows at most, + the look-ahead row).  wide: its rows carry 64 row offsets
// (order_wide_rows, insider_plan.hpp).  code_base / pair_base: probe_code_base's addresses (pair_base 0: one step per block).
static int launch_order_table(uint64_t seed, uint32_t iter, int K, int rows, int order_mode, bool wide,
                              unsigned long long code_base, unsigned long long pair_base, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_order_table, dim3(cdiv((int64_t)(rows + 1) * 64, 256)), dim3(256), 0, st, seed, iter, K, rows, order_mode,
                       K * 8, reg_kmax(K), wide ? 1 : 0, code_base, pair_base, out);
    KCHECK();
    return INSIDER_OK;
}

// the code addresses of the register-resident kernel for K (K <= 30) on this device: one probe launch per workspace
int ensure_code_base(insider_hip_handle *h, int K)
{
    if (!reg_pairs(reg_kmax(K)) || h->ws.cd_code_base) return INSIDER_OK;
    unsigned long long v[2];
    if (int rc = probe_code_base(K, h->ws.code_base_dev, h->st.stream, v)) return rc;
    h->ws.cd_code_base = v[0];
    h->ws.cd_pair_base = v[1];
    return INSIDER_OK;
}

// Builds the sweep-order table of outer iteration `iter` into order_buf[slot] (on `stream`); the caller makes it current
// (h->ws.order) when its solve is launched.  Two buffers: an outer iteration's table depends on (seed, iter) only, so the NEXT one
// is built while the current solve runs — the sweep kernel leaves no room for other waves, so the builder runs in its tail,
// on SIMDs that have already drained — instead of competing with the row phase.
int ensure_order_table(insider_hip_handle *h, uint64_t seed, uint32_t iter, int K, int max_sweeps, int order_mode,
                       hipStream_t stream = nullptr, int slot = 0)
{
    if (int rb = ensure_code_base(h, K)) return rb;
    if (!stream) stream = h->st.stream;
    // one period of the order sequence at most (include/insider_perm.h): the table does not grow with max_sweeps
    const int rows = std::min<int64_t>(max_sweeps, INSIDER_PERM_PERIOD);
    if (h->ws.order_rows < rows) {
        for (auto &b : h->ws.order_buf)
            if (int rc = b.alloc((size_t)(rows + 4) * ORDER_ROW)) return rc;   // + the look-ahead row (and the prologue's touch of the one after)
        h->ws.order_rows = rows;
    }
    if (int rc = launch_order_table(seed, iter, K, rows, order_mode, h->plan.order_wide, h->ws.cd_code_base,
                                    h->plan.order_pairs ? h->ws.cd_pair_base : 0ull, h->ws.order_buf[slot], stream))
        return rc;
    if (!h->ws.order) h->ws.order = h->ws.order_buf[slot];
    return INSIDER_OK;
}

// the launch order of the next column solve: genes by decreasing key, a bucket sort on a log scale (insider_kernels.hpp).
// sweeps != null: the keys are first updated from the last solve's sweep counts (reset: replaced, else smoothed)
// bucketed: the solve kernel has already done k_sched_bucket's part (ColArgs::sched_key ...), with the same counter set
int launch_gene_order(insider_hip_handle *h, const int *sweeps, int reset, int float_bits, hipStream_t st, bool bucketed = false)
{
    int *cnt = h->ws.sched_cnt[h->ws.sched_flip], *cnt_next = h->ws.sched_cnt[h->ws.sched_flip ^ 1];
    h->ws.sched_flip ^= 1;
    if (!bucketed)
        hipLaunchKernelGGL(k_sched_bucket, dim3(cdiv(h->ds->p, 256)), dim3(256), 0, st, sweeps, (int)h->ds->p, reset, float_bits,
                           h->ws.sweep_key, cnt, h->ws.sched_bkt, h->ws.sched_rank);
    KCHECK();
    hipLaunchKernelGGL(k_sched_scatter, dim3(cdiv(h->ds->p, 256)), dim3(256), 0, st, (const int *)cnt, cnt_next,
                       (const uint16_t *)h->ws.sched_bkt, (const int *)h->ws.sched_rank, (int)h->ds->p, h->ws.gene_perm);
    KCHECK();
    return INSIDER_OK;
}

// the pair-count statistics kernel (insider_col_factored.hpp) over every gene, on the main stream
int launch_paircnt(insider_hip_handle *h, const ColFacArgs &a)
{
    const FitPlan &plan = h->plan;
    const size_t lds = plan.pc_lds;
    switch (plan.pc_kernel) {
        case CSK_PAIRCNT4_MS4:
        case CSK_PAIRCNT4_MS8:
        case CSK_PAIRCNT4_MS4_ZT: {
            const int nb = plan.pc_blocks, npart = plan.pc_parts, cap = cdiv(a.p, npart);
            // a launch with ONE counter (few blocks) has a counter of its own behind the sixteen, so that the sixteen always
            // stand at the same value
            const int which = npart == 1 ? 1 : 0;
            unsigned *tk = h->ws.pc4_ticket + (size_t)which * PC4_PARTS * 32;
            const unsigned tbase = h->ws.pc4_base[which];
#define PC4(NBV, MS)                                                                                                         \
    {                                                                                                                        \
        if (plan.stats_own_q) hipLaunchKernelGGL((k_col_paircnt4<NBV, 4, 4, false, true>), dim3(nb), dim3(256), lds, h->st.stream, a, tk, tbase, npart, cap); /* (MS = 4 only: stats_own_q) */ \
        else if (a.zt) hipLaunchKernelGGL((k_col_paircnt4<NBV, 4, MS, true>), dim3(nb), dim3(256), lds, h->st.stream, a, tk, tbase, npart, cap); \
        else hipLaunchKernelGGL((k_col_paircnt4<NBV, 4, MS, false>), dim3(nb), dim3(256), lds, h->st.stream, a, tk, tbase, npart, cap); \
    }
            const bool ms4 = plan.pc_kernel != CSK_PAIRCNT4_MS8;
            if (h->ws.NB == 1 && ms4) PC4(1, 4)
            else if (h->ws.NB == 1) PC4(1, 8)
            else if (ms4) PC4(2, 4)
            else PC4(2, 8)
#undef PC4
            KCHECK();
            // what the launch takes from each counter in use: its items and one ticket per wave (only once it is known to be enqueued)
            h->ws.pc4_base[which] += (unsigned)cap + 4u * (unsigned)(nb / npart);
            h->col_stats_kernel = a.zt ? CSK_PAIRCNT4_MS4_ZT : ms4 ? CSK_PAIRCNT4_MS4 : CSK_PAIRCNT4_MS8;
            h->col_stats_tickets = npart;
            h->col_stats_blocks = nb;
            return INSIDER_OK;
        }
        case CSK_PAIRCNT:
        case CSK_PAIRCNT_ZT:
            NB_DISPATCH(h->ws.NB, {
                (void)WPB_;
                if (a.zt) hipLaunchKernelGGL((k_col_paircnt<NB_, 4, true>), dim3(cdiv(a.p, 4)), dim3(256), lds, h->st.stream, a);
                else hipLaunchKernelGGL((k_col_paircnt<NB_, 4, false>), dim3(cdiv(a.p, 4)), dim3(256), lds, h->st.stream, a);
            });
            KCHECK();
            h->col_stats_kernel = a.zt ? CSK_PAIRCNT_ZT : CSK_PAIRCNT;
            h->col_stats_tickets = h->col_stats_blocks = 0;
            return INSIDER_OK;
        default: return fail(INSIDER_ERR_ARG, "the call's plan names no pair-count statistics kernel");
    }
}

// masked Gram/XtY complement statistics of every gene (column side of src/optimize.cpp:216-222)
int launch_col_stats(insider_hip_handle *h, bool timed)
{
    Timer t;
    int rc;
    const bool factored = h->plan.col_path != 0, own_q = h->plan.stats_own_q;
    if (own_q) {
        if ((rc = t.begin(h, timed))) return rc;
    } else if (factored && h->st.qheld.pending) {   // Qheld = S^held A formed on side3 since the row factors were final (phase_R):
        if ((rc = h->st.qheld.wait(h->st.stream))) return rc;   // joined BEFORE the timer, which then holds the statistics kernel alone
        if ((rc = t.begin(h, timed))) return rc;
    } else {
        if ((rc = t.begin(h, timed))) return rc;
        if (factored)
            if ((rc = launch_q(h, h->ds->Sheld, h->ws.Qheld))) return rc;
    }
    if (factored) {
        ColFacArgs a = h->ds->cf;
        a.K = h->ws.K;
        a.Astack = h->ws.Astack;
        a.Qheld = h->ws.Qheld;
        a.sq = own_q ? (const double *)h->ds->cf_sq : nullptr;
        a.Qfull_out = own_q ? (double *)h->ws.Qfull : nullptr;
        a.RtR = h->ws.RtR;
        a.yy_all = h->ds->yy_all;
        a.yy_train = h->ds->yy_train;
        a.stat = h->ws.stat_col;
        if (h->plan.col_path == 2) {
            a.cnt = h->ds->cf_cnt;
            a.hn = h->ds->cf_hn;
            a.zt = h->ds->cf_zt;
            rc = launch_paircnt(h, a);
            if (rc) return rc;
        } else {
            NB_DISPATCH(h->ws.NB, {
                (void)WPB_;
                const size_t lds = ((size_t)(a.tab_rows + 1) * Geo<NB_>::KP + (size_t)4 * 16 * 17) * sizeof(double) + (size_t)4 * CF_CAP * 2;
                hipLaunchKernelGGL((k_col_factored<NB_, 4>), dim3(cdiv(h->ds->p, 4)), dim3(256), lds, h->st.stream, a);
            });
            h->col_stats_kernel = CSK_FACTORED;
            h->col_stats_tickets = h->col_stats_blocks = 0;
        }
        KCHECK();
    } else {
        uint64_t mark = 0;
        rc = launch_list_stats(h, true, 1, h->ws.R, h->ws.stat_col, h->ws.RtR, &mark);   // the record's K x K part = R'R - complement
        if (rc) return rc;
        h->col_stats_kernel = (mark & rk_bit(RK_LIST_STATS4)) ? CSK_LIST4 : CSK_LIST;
        h->col_stats_tickets = h->col_stats_blocks = 0;
    }
    h->col_stats_own_q = own_q ? 1 : 0;
    return t.end(h, h->ev_col);
}

// what ColArgs and RidgeArgs share: the statistics, the factors and where the per-gene loss terms go
template <typename Args>
void col_args_head(const insider_hip_handle *h, int masked, int checkpoint, Args &a)
{
    a.stat = masked ? h->ws.stat_col : nullptr;
    a.stat_len = h->plan.stat_len;
    a.p = (int)h->ds->p;
    a.K = h->ws.K;
    a.KP = h->ws.KP;
    a.RtR = h->ws.RtR;
    a.Qfull = h->ws.Qfull;
    a.C = h->ws.C;
    a.yy = masked ? h->ds->yy_train : h->ds->yy_all;
    a.checkpoint = checkpoint;
    a.sse_train = h->ws.sse_train;
    a.b2 = h->ws.b2;
    a.b1 = h->ws.b1;
    a.sse_test = h->ws.sse_test;
    a.test_from_stats = masked && h->ds->no_na;
}

// column update from the statistics: elastic-net CD (alpha > 0) or ridge (alpha == 0), or evaluation only
int launch_col_solve(insider_hip_handle *h, int masked, bool solve, double lambda, double alpha, double tol,
                     int checkpoint, bool timed, int outer_iter = -1, bool side = false)
{
    const bool early = outer_iter >= 0 && outer_iter < Workspace::EARLY;
    int rc;
    // (every stream join is a barrier packet on the main queue, ~5 us of bubble each at c3: qfull's event is recorded on the side stream
    // AFTER the previous iteration's side_done — phase_R comes after side_close — so it stands for both)
    if ((rc = h->st.side_done.wait(h->st.stream))) return rc;   // the gene order / sweep-order table prepared on the side stream
    if ((rc = h->st.qfull.wait(h->st.stream))) return rc;
    Timer t;
    if ((rc = t.begin(h, timed))) return rc;
    const FitPlan &plan = h->plan;
    const ColSolver cs = plan.col_solver;
    if (cs == CS_NONE || (alpha == 0.0) != (cs == CS_RIDGE_REG || cs == CS_RIDGE))
        return fail(INSIDER_ERR_ARG, "the call's plan names no kernel for this column solve");
    bool eval_after = false, fused_bucket = false;
    ColArgs eval_args;
    h->col_solver = h->col_eval = h->col_ridge_fallback = CS_NONE;
    if (alpha == 0.0) {
        RidgeArgs a;
        col_args_head(h, masked, checkpoint, a);
        a.lambda = lambda;
        a.solve = solve ? 1 : 0;
        a.fail = h->ws.failflag;
        a.mark = h->ws.sweeps;          // free in the alpha == 0 path: cleared below
        a.retry = h->ws.failflag + 1;
        a.only_marked = 0;
        if (cs == CS_RIDGE_REG) {
            if (solve) {
                HIPCHECK(hipMemsetAsync(h->ws.sweeps, 0, (size_t)h->ds->p * sizeof(int), h->st.stream));
                HIPCHECK(hipMemsetAsync(h->ws.failflag + 1, 0, sizeof(int), h->st.stream));
            }
            REG_DISPATCH(h->ws.K, hipLaunchKernelGGL((k_ridge_cols_reg<SL_, KM_>), dim3(cdiv(h->ds->p, 4)), dim3(64), 0, h->st.stream, a));
            h->col_solver = CS_RIDGE_REG;
            KCHECK();
            if (solve && plan.ridge_fallback) {   // genes whose system was not positive definite: solve(..., likely_sympd)'s general route
                a.only_marked = 1;
                hipLaunchKernelGGL((k_ridge_cols<1>), dim3((unsigned)h->ds->p), dim3(64), 0, h->st.stream, a);   // unmarked genes exit at once
                h->col_ridge_fallback = 1;
            }
        } else {
            hipLaunchKernelGGL((k_ridge_cols<1>), dim3((unsigned)h->ds->p), dim3(64), 0, h->st.stream, a);
            h->col_solver = CS_RIDGE;
        }
        KCHECK();
        if (solve) HIPCHECK(hipMemsetAsync(h->ws.sweeps, 0, (size_t)h->ds->p * sizeof(int), h->st.stream));
    } else {
        ColArgs a;
        col_args_head(h, masked, checkpoint, a);
        a.mode = solve ? COL_CD : COL_EVAL;
        a.cd = cd_params(lambda, alpha, tol, h->opt.max_sweeps, h->ws.order);
        a.sweeps = h->ws.sweeps;
        a.sweep_bins = (timed && solve) ? h->ws.sweep_total : nullptr;
        a.gene_perm = !solve ? nullptr : (early && h->ws.have_early[outer_iter]) ? h->ws.perm_early[outer_iter]
                                       : h->ws.have_perm                         ? h->ws.gene_perm
                                                                              : nullptr;
        a.hsave = h->ws.cd_hsave;
        a.isave = h->ws.cd_isave;
        a.pass_count = nullptr;
        a.resume = 0;
        a.pass_slot = nullptr;
        a.bucket_cnt = nullptr;
        a.cap_hits = solve ? h->ws.failflag + 2 : nullptr;
        a.sched_key = a.sched_cnt = a.sched_rank = nullptr;
        a.sched_bkt = nullptr;
        a.sched_reset = 0;
        if (cs == CS_CD_REG || cs == CS_CD_REG3) {
            // Cold outer iterations: thousands of sweeps per gene whose counts no history predicts, so a wave's four genes
            // finish far apart (measured at c3: 1.17x / 1.44x / 2.1x the ideal wave time in outer iterations 0 / 1 / 2).
            // The solve then runs in passes over geometrically growing sweep ranges: a limited pass stops at its sweep
            // index, the genes still running save their state and an estimate of their remaining length (from the decay
            // of the loss change), k_pass_scatter groups them by that estimate, and the next pass continues them
            // bit-identically in waves of similar length (insider_cd_reg.hpp).  A pass with nothing left exits at once.
            if (solve) {   // every gene's part of the next launch order, when it finishes (launch_gene_order below skips k_sched_bucket)
                a.sched_key = h->ws.sweep_key;
                a.sched_cnt = h->ws.sched_cnt[h->ws.sched_flip];
                a.sched_rank = h->ws.sched_rank;
                a.sched_bkt = h->ws.sched_bkt;
                a.sched_reset = (outer_iter < Workspace::EARLY || !h->ws.have_perm) ? 1 : 0;
                fused_bucket = true;
            }
            const int npass = (solve && outer_iter >= 0 && outer_iter < plan.cold_iters) ? plan.npass : 0;
            int start = 0;
            const int *perm_in = a.gene_perm;
            for (int pass = 0;; ++pass) {
                const int limit = pass < npass ? plan.pass_limit[pass] : 0;
                a.cd.start_sweep = start;
                a.cd.sweep_limit = limit;
                a.pass_slot = npass ? h->ws.cd_pass_slot : nullptr;
                a.bucket_cnt = limit ? h->ws.cd_pass_cnt : nullptr;
                if (limit) HIPCHECK(hipMemsetAsync(h->ws.cd_pass_cnt, 0, CD_BUCKETS * sizeof(int), h->st.stream));
                if (solve) {
                    if ((rc = launch_cd(cs, a, h->st.stream))) return rc;
                    h->col_solver = cs;
                }
                if (!limit) break;
                int *count_out = h->ws.cd_pass_cnt + CD_BUCKETS + (pass & 1);
                hipLaunchKernelGGL(k_pass_scatter, dim3(cdiv(h->ds->p, 256)), dim3(256), 0, h->st.stream,
                                   (const uint32_t *)h->ws.cd_pass_slot, (const int *)h->ws.cd_pass_cnt, perm_in, a.pass_count, (int)h->ds->p,
                                   h->ws.cd_pass_perm[pass & 1], count_out);
                KCHECK();
                perm_in = a.gene_perm = h->ws.cd_pass_perm[pass & 1];
                a.pass_count = count_out;
                a.resume = 1;
                start = limit;
            }
            eval_after = checkpoint != 0;
            eval_args = a;
        } else {
            if ((rc = launch_cd(cs, a, h->st.stream))) return rc;
            h->col_solver = cs;
        }
    }
    if ((rc = t.end(h, h->ev_cd))) return rc;
    if (eval_after) {   // the per-gene loss statistics of the (updated) columns: the evaluation kernel, all genes (not part of the solve's time)
        eval_args.gene_perm = nullptr;
        eval_args.pass_count = nullptr;
        eval_args.resume = 0;
        if (plan.col_eval == CS_CD_REG) {
            REG_DISPATCH(h->ws.K, hipLaunchKernelGGL((k_cd_cols_reg<SL_, KM_, false>), dim3(cdiv(h->ds->p, 4)), dim3(64), 0, h->st.stream, eval_args));
            h->col_eval = CS_CD_REG;
        } else {   // three slots: the row16 kernel's evaluation part (the sweep kernel's registers are all taken)
            const size_t eb = (size_t)r16_lds_doubles(h->ws.K) * sizeof(double);
            if (int rl = r16_wide_lds(eb)) return rl;
            eval_args.mode = COL_EVAL;
            hipLaunchKernelGGL((k_cd_cols_r16<3>), dim3(cdiv(h->ds->p, 4)), dim3(64), eb, h->st.stream, eval_args);
            h->col_eval = CS_CD_R16_3;
        }
        KCHECK();
    }
    if (solve && alpha != 0.0) {
        // schedule the next solve longest-first, genes of similar length sharing a wave.  (The bucket sort's order inside a
        // bucket is the order of the solve kernel's atomics: which genes share a wave — and so the timings — may differ from
        // run to run; no result depends on it.)
        hipStream_t st = h->st.stream;
        if (side) {
            HIPCHECK(hipEventRecord(h->st.ev_cd_done, h->st.stream));
            HIPCHECK(hipStreamWaitEvent(h->st.side, h->st.ev_cd_done, 0));
            st = h->st.side;
        }
        if ((rc = launch_gene_order(h, h->ws.sweeps, (outer_iter < Workspace::EARLY || !h->ws.have_perm) ? 1 : 0, 0, st, fused_bucket)))
            return rc;
        h->ws.have_perm = true;
        if (early) {
            HIPCHECK(hipMemcpyAsync(h->ws.perm_early[outer_iter], h->ws.gene_perm, (size_t)h->ds->p * sizeof(int),
                                    hipMemcpyDeviceToDevice, st));
            h->ws.have_early[outer_iter] = true;
        }
        // the caller may add the next sweep-order table to the side stream, then closes it with side_close()
        if (side) h->st.side_done.pending = true;
    }
    return INSIDER_OK;
}

int side_close(insider_hip_handle *h)
{
    return h->st.side_done.pending ? h->st.side_done.record(h->st.side) : INSIDER_OK;
}

// sum over test entries of the squared residual per gene (evaluate(), src/utils.cpp:67); checkpoints only
int launch_test_sse(insider_hip_handle *h, int masked, bool timed)
{
    if (!masked) {
        HIPCHECK(hipMemsetAsync(h->ws.sse_test, 0, (size_t)h->ds->p * sizeof(double), h->st.stream));
        return INSIDER_OK;
    }
    if (h->ds->no_na) return INSIDER_OK;   // the column kernel derived the test residuals from the statistics
    Timer t;
    int rc = t.begin(h, timed);
    if (rc) return rc;
    hipLaunchKernelGGL((k_test_sse_list<4>), dim3(cdiv(h->ds->p, 4)), dim3(256), 0, h->st.stream, (const uint32_t *)h->ds->col_ptr,
                       (const int *)h->ds->col_idx, (const double *)h->ds->col_val, (const uint8_t *)h->ds->col_flag, (int)h->ds->p,
                       (const double *)h->ws.R, (const double *)h->ws.C, h->ws.K, h->ws.KP, h->ws.sse_test);
    KCHECK();
    return t.end(h, h->ev_test);
}

// col: the call's column solve (none: a call that runs no column solve)
void plan_call(insider_hip_handle *h, int masked, const ColCall *col = nullptr) { h->plan = build_plan(plan_facts(h, h->ws.K), masked, col); }

// V = C A' for the stacked levels [q_begin, q_end) (all of them once per outer iteration, then the updated covariate's)
int launch_gene_v(insider_hip_handle *h, int q_begin, int q_end)
{
    // V[:, q_begin:q_end) = C A[q_begin:q_end, :]'  (A given "transposed": one row per output column)
    const int N = q_end - q_begin;
    if (N <= 0) return INSIDER_OK;
    if (h->plan.v_rows2) {   // A' staged in LDS once per block, C read in 16-byte pieces (k_mm_rows2)
        const int tiles = cdiv((int)h->ds->p, 16), tpw = h->plan.mm_tpw;
        const size_t ldsb = (size_t)4 * cdiv(h->ws.K, 16) * 64 * sizeof(double);
#define GV2_LAUNCH(NT_)                                                                                                       \
    hipLaunchKernelGGL((k_mm_rows2<NT_, true>), dim3(cdiv(cdiv(tiles, tpw), 4), cdiv(N, 16 * NT_)), dim3(256), ldsb * NT_, h->st.stream, \
                       (const double *)h->ws.C, (int64_t)h->ws.KP, (int)h->ds->p, h->ws.K,                                                \
                       (const double *)(h->ws.Astack + (size_t)q_begin * h->ws.KP), h->ws.KP, N, h->ws.Vlev + q_begin, (int64_t)h->ds->SLP, N, tpw)
        switch (mm_rows_nt(N)) {
            case 1: GV2_LAUNCH(1); break;
            case 2: GV2_LAUNCH(2); break;
            default: GV2_LAUNCH(4); break;
        }
#undef GV2_LAUNCH
        KCHECK();
        row_mark(h, RK_MM_ROWS2);
        h->mm_rows2_tiles = tpw;
        return INSIDER_OK;
    }
#define GV_LAUNCH(NT_)                                                                                                        \
    hipLaunchKernelGGL((k_mm_rows<NT_, true>), dim3(cdiv(cdiv((int)h->ds->p, 16), 4), cdiv(N, 16 * NT_)), dim3(256), 0, h->st.stream, \
                       (const double *)h->ws.C, (int64_t)h->ws.KP, (int)h->ds->p, h->ws.K,                                                \
                       (const double *)(h->ws.Astack + (size_t)q_begin * h->ws.KP), h->ws.KP, N, h->ws.Vlev + q_begin, (int64_t)h->ds->SLP, N)
    switch (mm_rows_nt(N)) {
        case 1: GV_LAUNCH(1); break;
        case 2: GV_LAUNCH(2); break;
        default: GV_LAUNCH(4); break;
    }
#undef GV_LAUNCH
    KCHECK();
    row_mark(h, RK_MM_ROWS);
    return INSIDER_OK;
}

int launch_row_stats(insider_hip_handle *h, bool timed)
{
    Timer t;
    int rc = t.begin(h, timed);
    if (rc) return rc;
    rc = launch_list_stats(h, false, h->ws.nseg, h->ws.C, h->ws.stat, nullptr, &h->row_kernels);
    if (rc) return rc;
    return t.end(h, h->ev_row);
}

int do_allreduce(insider_hip_handle *h, double *buf, int64_t count)
{
    if (!h->plan.allreduce) return INSIDER_OK;
    if (h->comm) {
        // in-library RCCL: the collective is enqueued on the library's own stream, between the kernels that produce
        // and consume `buf`; no host synchronisation, no callback into the host language
        const ncclResult_t r = ncclAllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, h->comm, h->st.stream);
        if (r != ncclSuccess) return fail(INSIDER_ERR_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
        return INSIDER_OK;
    }
    if (!h->allreduce) {
        if (h->world > 1) return fail(INSIDER_ERR_COMM, "world > 1 needs insider_hip_comm_init() or an all-reduce callback");
        return INSIDER_OK;
    }
    // stream-ordered: the callback enqueues the collective against h->st.stream (see include/insider_hip.h)
    if (h->allreduce(h->allreduce_user, buf, count, (void *)h->st.stream) != 0)
        return fail(INSIDER_ERR_COMM, "all-reduce callback failed");
    return INSIDER_OK;
}

// level records' Gram part of covariate i: sum_j n_jl c_j c_j' for every level -> rec[l][0 .. STAT)
int launch_level_gram(insider_hip_handle *h, int i, hipStream_t st, double *rec, const CovTables *cont_ct = nullptr)
{
    const CovTables &ct = cont_ct ? *cont_ct : h->ds->cov[i];
    const CovTables &lists = cont_ct ? h->ds->contm_lists : ct;   // (the continuous columns' lists and work items: one copy)
    const WgPlan w = cont_ct ? WgPlan() : h->plan.wg[i];
    const int stat_len = h->plan.stat_len, plen = h->plan.plen;
    if (w.use) {
        const float *hn = h->ds->cf_hn + h->ds->cf.hn_off[h->ds->cf_pos[i]];
        const dim3 grid(cdiv(cdiv(w.ntile, 2) * w.nslab, 4), 1, w.zch);   // (slab, pair-tile pair) items, four waves per block
#define WG_LAUNCH(LT_)                                                                                                     \
    hipLaunchKernelGGL((k_wgemm<LT_>), grid, dim3(256), 0, st, hn, h->ds->cf.hn_stride, w.tiles, (const double *)h->ws.C, h->ws.KP,   \
                       (int)h->ds->p, w.slab, w.nslab, (const uint8_t *)h->ws.wg_pair, w.ntile, h->ws.wg_part)
        switch (w.LT) {
            case 4: WG_LAUNCH(4); row_mark(h, RK_WGEMM4); break;
            case 5: WG_LAUNCH(5); row_mark(h, RK_WGEMM5); break;
            case 6: WG_LAUNCH(6); row_mark(h, RK_WGEMM6); break;
            default: WG_LAUNCH(7); row_mark(h, RK_WGEMM7); break;
        }
#undef WG_LAUNCH
        if (w.zch > 1) row_mark(h, RK_WGEMM_CHUNKS);
        KCHECK();
        hipLaunchKernelGGL(k_wgemm_sum, dim3(cdiv(stat_len, 256), ct.L), dim3(256), 0, st, (const double *)h->ws.wg_part, w.nslab,
                           w.tiles, w.ntile, h->ws.K, stat_len, rec, plen);
        KCHECK();
        return INSIDER_OK;
    }
    NB_DISPATCH(h->ws.NB, {
        if (ct.nitems > 0) {   // no held-out entry at all: every level sum is zero
            hipLaunchKernelGGL((k_wsyrk<NB_, WPB_>), dim3(cdiv(ct.nitems, WPB_)), dim3(WPB_ * 64), 0, st,
                               (const uint32_t *)lists.item_begin, (const uint32_t *)lists.item_end, ct.nitems,
                               (const int *)lists.wl_idx, (const double *)ct.wl_w, (const double *)h->ws.C, (int64_t)h->ds->p, h->ws.wpart);
            row_mark(h, RK_WSYRK);
        }
        hipLaunchKernelGGL(k_level_sum, dim3(cdiv(stat_len, 16), ct.L), dim3(256), 0, st, (const double *)h->ws.wpart,
                           (const int *)lists.lvl_item_ptr, stat_len, rec, plen);
    });
    KCHECK();
    return INSIDER_OK;
}

// merged row update: the weighted SYRK + level sums of every covariate (they depend on C and the static lists only) on the
// second side stream, from the point where C is final; row_update() waits for its covariate's event
int launch_wsyrk_side(insider_hip_handle *h)
{
    HIPCHECK(hipEventRecord(h->st.ev_c_ready, h->st.stream));
    HIPCHECK(hipStreamWaitEvent(h->st.side2, h->st.ev_c_ready, 0));
    // The weighted SYRK of the first covariate is the longest kernel of the row phase (MFMA-bound on its (level, gene)
    // pairs) and the first thing the main chain waits for: it starts at once.  C'C and (S^train C') (launch_row_prep) run on
    // a third stream: they are first read by k_level_reduce, which waits for ev_prep.
    // Who is dispatched first decides the phase's length (round 4): when the main chain's k_gene_u (12500 blocks) reaches the
    // CUs before the level Gram GEMM of covariate 0 (255 blocks, one wave per SIMD), the GEMM's blocks land unevenly between
    // them and it takes 220 us instead of 140 — 590 against 460 us for the phase, the mode chosen by how the queues happen to
    // wake up after the solve.  So k_gene_u waits for this event, recorded on the GEMM's stream directly in front of it: its
    // queue goes on to dispatch the GEMM at once, the main stream's wake-up comes a few microseconds later (and behind V).
    HIPCHECK(hipEventRecord(h->st.ev_head, h->st.side2));
    HIPCHECK(hipStreamWaitEvent(h->st.side3, h->st.ev_c_ready, 0));
    if (int rp = launch_gram(h, h->ws.C, h->ds->p, h->ws.CCt, h->st.side3, h->ws.gram_part2)) return rp;
    if (int rp = launch_mm_reduce_kp(h, h->ds->Strain, h->ds->SLP, h->ws.C, (int)h->ds->p, h->ds->SL, h->ws.sc_part2, h->ws.SC, h->st.side3)) return rp;
    HIPCHECK(hipEventRecord(h->st.ev_prep, h->st.side3));
    h->prep_joined = false;
    row_mark(h, RK_GRAM_SIDE);
    const size_t plen = h->plan.plen;
    for (int i = 0; i < h->ds->c; ++i) {
        if (int rg = launch_level_gram(h, i, h->st.side2, h->ws.lvl_sum_all + (size_t)h->ds->lvl_off[i] * plen)) return rg;
        HIPCHECK(hipEventRecord(h->st.ev_w[i], h->st.side2));
    }
    for (int k = 0; k < (h->ds->cont_merged ? h->ds->m : 0); ++k) {   // continuous columns: one-level covariates with real-valued weights
        if (int rg = launch_level_gram(h, 0, h->st.side2, h->ws.lvl_sum_all + (size_t)(h->ds->SLcat + k) * plen, &h->ds->contm[k])) return rg;
        HIPCHECK(hipEventRecord(h->st.ev_w[h->ds->c + k], h->st.side2));
    }
    h->w_ready = true;
    return INSIDER_OK;
}

// merged row update behind launch_wsyrk_side(): the main stream waits for the level sums of row-update w (side2) and, in the
// FIRST update of the iteration only, for C'C and (S^train C') (side3).  ev_prep is recorded once per iteration and every later
// update is ordered behind the first one's wait: another wait is a barrier packet on the serial chain for nothing.
int join_side(insider_hip_handle *h, int w)
{
    HIPCHECK(hipStreamWaitEvent(h->st.stream, h->st.ev_w[w], 0));
    if (!h->prep_joined) HIPCHECK(hipStreamWaitEvent(h->st.stream, h->st.ev_prep, 0));
    h->prep_joined = true;
    return INSIDER_OK;
}

// one covariate's row update: categorical covariate i (optimize_row, src/optimize.cpp:139-198), or continuous
// column j (optimize_continuous_v2, :76-137) when cont_col >= 0
int row_update(insider_hip_handle *h, int i, int cont_col, int masked, double lambda1, bool rebuild_R = true)
{
    const bool cont = cont_col >= 0;
    const FitPlan &plan = h->plan;
    const bool fused_solve = !cont && plan.fused_solve;   // (a continuous column's solve is k_cont_cd's cyclic passes)
    const CovTables &ct = cont ? h->ds->cont : h->ds->cov[i];
    const int row0 = cont ? h->ds->SLcat + cont_col : h->ds->lvl_off[i];   // first row of this covariate in Astack / SC
    LevelArgs la;
    la.stat = h->ws.stat;
    la.nseg = h->ws.nseg;
    la.n = (int)h->ds->n;
    la.K = h->ws.K;
    la.masked = masked;
    la.R = h->ws.R;
    la.lev = h->ds->lev;
    la.lvl_off = h->ds->lvl_off_d;
    la.cov = cont ? -1 : i;
    la.own_row = row0;
    la.weights = cont ? h->ds->Zc + (size_t)cont_col * h->ds->n : nullptr;
    la.chunk_begin = ct.chunk_begin;
    la.chunk_end = ct.chunk_end;
    la.members = cont ? h->ds->ident_members : h->ds->members_all + (size_t)i * h->ds->n;
    la.nchunks = ct.nchunks;
    la.Astack = h->ws.Astack;
    la.part = h->ws.lvl_part;
    LevelReduceArgs ra;
    ra.part = h->ws.lvl_sum;
    ra.L = ct.L;
    ra.K = h->ws.K;
    ra.CCt = h->ws.CCt;
    ra.SC = h->ws.SC;
    ra.sc_off = row0;
    ra.eq = h->ws.eq;
    if (cont && plan.merged) {
        // merged update of continuous column cont_col (optimize_continuous_v2, src/optimize.cpp:76-137): the one-level covariate
        // with real-valued membership weights z_r — u_j from the real-valued count table, Y = U'C, the level record's Gram sum
        // from the (gene, sum z^2) list, sum_r z_r s_r from the real-valued pair counts; then the reference's cyclic scalar
        // passes on (H, b) (k_cont_cd) as on the per-sample path
        const int KP = h->ws.KP;
        const CovTables &cm = h->ds->contm[cont_col];
        ColFacArgs ca = h->ds->cf;
        ca.zt = h->ds->cf_zt;
        hipLaunchKernelGGL((k_gene_uc<4>), dim3(cdiv(h->ds->p, 4)), dim3(256), 0, h->st.stream, ca, cont_col, (const double *)h->ws.Vlev, h->ds->SLP,
                           h->ws.U);
        KCHECK();
        row_mark(h, RK_GENE_UC);
        int ypart_n = 0;
        if (int rcy = launch_mm_reduce_kp(h, h->ws.U, 2, h->ws.C, (int)h->ds->p, 1, h->ws.sc_part, nullptr, nullptr, &ypart_n, &h->row_kernels))
            return rcy;
        if (h->w_ready)
            if (int rj = join_side(h, h->ds->c + cont_col)) return rj;
        double *rec = h->w_ready ? h->ws.lvl_sum_all + (size_t)row0 * plan.plen : h->ws.lvl_sum;
        if (!h->w_ready)
            if (int rg = launch_level_gram(h, 0, h->st.stream, rec, &cm)) return rg;
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_level_merged<NB_>), dim3(1), dim3(256), 0, h->st.stream, (const double *)rec, (const double *)h->ws.sc_part,
                               ypart_n, (const double *)cm.paircnt, h->ds->SL, (const double *)h->ws.Astack, (const int *)h->ds->one_count,
                               (const double *)h->ws.CCt, (const double *)(h->ws.SC + (size_t)row0 * KP), 1, h->ws.K, lambda1, 0, h->ws.eq,
                               h->ws.Astack + (size_t)row0 * KP, h->ws.failflag, (const double *)(h->ds->cont_cnt + cont_col));
        });
        row_mark(h, RK_MERGED);
    } else if (!cont && plan.merged) {
        // merged update: one weighted rank-one term per (level, gene) pair, one look-up per held-out entry
        const int L = ct.L, LP = (int)round_up(L, 2), KP = h->ws.KP;
        if (plan.u_cnt[i]) {   // u from the dense pair counts (insider_col_factored.hpp)
            const size_t gu_lds = (size_t)4 * (h->ds->SL + LP + GU_BATCH * WAVE) * sizeof(double);
            ColFacArgs ca = h->ds->cf;
            ca.cnt = h->ds->cf_cnt;
            ca.zt = h->ds->m > 0 ? h->ds->cf_zt : nullptr;   // (+ the continuous covariates' term from the real-valued counts)
            hipLaunchKernelGGL((k_gene_u_cnt<4>), dim3(cdiv(h->ds->p, 4)), dim3(256), gu_lds, h->st.stream, ca, h->ds->cf_pos[i], LP,
                               (const double *)h->ws.Vlev, h->ds->SLP, h->ds->SL, h->ws.U);
            row_mark(h, RK_GENE_U_CNT);
        } else {
            // (k_gene_u knows nothing of the continuous covariates' term: insider_hip_create_ex leaves cont_merged off when a
            // covariate's k_gene_u_cnt record does not fit, so this branch is never reached with m > 0)
            if (h->ds->m > 0) return fail(INSIDER_ERR_UNSUPPORTED, "merged row update with continuous covariates needs the pair-count form");
            hipLaunchKernelGGL((k_gene_u<4>), dim3(cdiv(h->ds->p, 4)), dim3(256), (size_t)4 * (h->ds->SLcat + GU_TILE) * sizeof(double),
                               h->st.stream, (const uint32_t *)ct.grp, (const uint16_t *)ct.slev,
                               (size_t)h->ds->col_entries + LIST_BLOCK, h->ds->c - 1, L, LP, (const double *)h->ws.Vlev, h->ds->SLP, (int)h->ds->p,
                               h->ds->SLcat, h->ws.U);
            row_mark(h, RK_GENE_U);
        }
        KCHECK();
        // Y = U'C, the same reduction over genes as (S C'); with the fused level kernel its per-slab partial sums are added up
        // there (k_sum_partials' order), which takes one launch per covariate off the main chain
        int ypart_n = 0;
        if (int rcy = launch_mm_reduce_kp(h, h->ws.U, LP, h->ws.C, (int)h->ds->p, L, h->ws.sc_part, plan.row_fused ? nullptr : h->ws.Ylvl, nullptr,
                                          &ypart_n, &h->row_kernels))
            return rcy;
        if (!plan.row_fused) ypart_n = 0;
        if (h->w_ready)   // wsyrk + level sums came from side2, C'C and (S^train C') from side3
            if (int rj = join_side(h, i)) return rj;
        if (!h->w_ready)
            if (int rg = launch_level_gram(h, i, h->st.stream, h->ws.lvl_sum)) return rg;
        double *rec = h->w_ready ? h->ws.lvl_sum_all + (size_t)row0 * plan.plen : h->ws.lvl_sum;
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            if (plan.row_fused) {   // the level records' tail, the level equations and (fused_solve) the solves: one launch
                hipLaunchKernelGGL((k_level_merged<NB_>), dim3(L), dim3(256), 0, h->st.stream, (const double *)rec,
                                   (const double *)(ypart_n ? h->ws.sc_part : h->ws.Ylvl), ypart_n, (const double *)ct.paircnt, h->ds->SL, (const double *)h->ws.Astack,
                                   (const int *)(h->ds->lvl_count_all + h->ds->lvl_off[i]), (const double *)h->ws.CCt,
                                   (const double *)(h->ws.SC + (size_t)row0 * KP), L, h->ws.K, lambda1, fused_solve ? 1 : 0, h->ws.eq,
                                   h->ws.Astack + (size_t)row0 * KP, h->ws.failflag);
                row_mark(h, fused_solve ? RK_MERGED_SOLVE : RK_MERGED);
            } else {
                hipLaunchKernelGGL(k_level_pack, dim3(L), dim3(256), 0, h->st.stream, (const double *)h->ws.Ylvl,
                                   (const double *)ct.paircnt, h->ds->SL, (const double *)h->ws.Astack,
                                   (const int *)(h->ds->lvl_count_all + h->ds->lvl_off[i]), L, h->ws.K, KP, plan.stat_len, rec);
                ra.part = rec;
                hipLaunchKernelGGL((k_level_reduce<NB_>), dim3(L), dim3(64), 0, h->st.stream, ra);
                row_mark(h, RK_PACK_REDUCE);
            }
        });
    } else if (!cont && plan.unmasked_fused) {
        const int L = ct.L, KP = h->ws.KP;
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_level_merged<NB_>), dim3(L), dim3(256), 0, h->st.stream, (const double *)h->ws.lvl_zero,
                               (const double *)h->ws.lvl_zero, 0, (const double *)ct.paircnt, h->ds->SL, (const double *)h->ws.Astack,
                               (const int *)(h->ds->lvl_count_all + h->ds->lvl_off[i]), (const double *)h->ws.CCt,
                               (const double *)(h->ws.SC + (size_t)row0 * KP), L, h->ws.K, lambda1, fused_solve ? 1 : 0, h->ws.eq,
                               h->ws.Astack + (size_t)row0 * KP, h->ws.failflag);
        });
        row_mark(h, fused_solve ? RK_MERGED_SOLVE : RK_MERGED);
        row_mark(h, RK_MERGED_ZERO);
    } else {
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_level_partial<NB_>), dim3(ct.nchunks), dim3(64), 0, h->st.stream, la);
            hipLaunchKernelGGL(k_level_sum, dim3(cdiv(plan.plen, 16), ct.L), dim3(256), 0, h->st.stream,
                               (const double *)h->ws.lvl_part, (const int *)ct.lvl_chunk_ptr, plan.plen, h->ws.lvl_sum, plan.plen);
            hipLaunchKernelGGL((k_level_reduce<NB_>), dim3(ct.L), dim3(64), 0, h->st.stream, ra);
        });
        row_mark(h, RK_LEVEL_PARTIAL);
    }
    KCHECK();
    if (fused_solve) return rebuild_R ? launch_build_R(h) : INSIDER_OK;
    int rc = do_allreduce(h, h->ws.eq, (int64_t)ct.L * (h->ws.KP * h->ws.KP + h->ws.KP));
    if (rc) return rc;
    if (cont && masked) {
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_cont_cd<NB_>), dim3(1), dim3(64), 0, h->st.stream, (const double *)h->ws.eq, h->ws.K, lambda1,
                               h->ws.Astack + (size_t)row0 * h->ws.KP);
        });
        row_mark(h, RK_CONT_CD);
    } else {
        NB_DISPATCH(h->ws.NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_level_solve<NB_>), dim3(ct.L), dim3(64), 0, h->st.stream, (const double *)h->ws.eq,
                               (const int *)(cont ? h->ds->one_count : h->ds->lvl_count_all + h->ds->lvl_off[i]), ct.L, h->ws.K, lambda1,
                               h->ws.Astack + (size_t)row0 * h->ws.KP, h->ws.failflag);
        });
        row_mark(h, RK_LEVEL_SOLVE);
    }
    KCHECK();
    // the next covariate's Gauss-Seidel residual sees this update (:353-355, :347-349): the per-sample path reads it from R;
    // the merged update works from the stacked factors and the gene tables, so there only the last covariate rebuilds R
    return rebuild_R ? launch_build_R(h) : INSIDER_OK;
}

struct LossOut {
    double sum_residual, train_rmse, test_rmse, row_reg_half, col_reg_half, l1_reg, loss;
};

// evaluate() + compute_loss() (src/utils.cpp:56-102) from the per-gene statistics of the last column pass
int loss_checkpoint(insider_hip_handle *h, int tuning, double lambda1, double lambda2, double alpha, LossOut *o)
{
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, h->st.stream, h->ws.sse_train, h->ws.sse_test, h->ws.b2, h->ws.b1,
                       (int)h->ds->p, h->ws.Astack, h->ds->SL, h->ws.K, h->ws.KP, h->ws.loss_buf);
    KCHECK();
    // layout: [0]=sse_train [1]=sse_test [2]=sum c^2 [3]=sum |c| [4]=cnt_train [5]=cnt_test | [6]=sum a^2 (replicated)
    double cnt[2] = {tuning == 1 ? h->ds->cnt_train : (double)h->ds->n * (double)h->ds->p, h->ds->cnt_test};
    HIPCHECK(hipMemcpyAsync(h->ws.loss_buf + 4, cnt, 2 * sizeof(double), hipMemcpyHostToDevice, h->st.stream));
    int rc = do_allreduce(h, h->ws.loss_buf, 6);
    if (rc) return rc;
    double v[8];
    HIPCHECK(hipMemcpyAsync(v, h->ws.loss_buf, 8 * sizeof(double), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    o->sum_residual = v[0];
    o->train_rmse = std::sqrt(v[0] / v[4]);                                                   // :63,66
    o->test_rmse = (tuning == 1 && v[5] > 0) ? std::sqrt(v[1] / v[5]) : std::numeric_limits<double>::quiet_NaN();
    const double nfA = std::sqrt(v[6]), nfC = std::sqrt(v[2]);
    o->row_reg_half = lambda1 * nfA * nfA / 2;                                                // :83-86 (all A_i share lambda1)
    o->col_reg_half = lambda2 * (1 - alpha) * nfC * nfC / 2;                                  // :88
    o->l1_reg = lambda2 * alpha * v[3];                                                       // :91
    o->loss = o->sum_residual / 2 + o->row_reg_half + o->col_reg_half + o->l1_reg;            // :93
    return INSIDER_OK;
}

int check_fail_flag(insider_hip_handle *h)
{
    int f = 0;
    HIPCHECK(hipMemcpyAsync(&f, h->ws.failflag, sizeof(int), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    if (f) {
        HIPCHECK(hipMemsetAsync(h->ws.failflag, 0, sizeof(int), h->st.stream));
        return fail(INSIDER_ERR_SOLVE, "a ridge normal-equation system was not positive definite");
    }
    return INSIDER_OK;
}

// cap-hit counter and longest solve of the column updates since the last reset (failflag[2..3])
int read_cap_hits(insider_hip_handle *h)
{
    int v[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(v, h->ws.failflag + 2, sizeof(v), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    h->cap_hits = v[0];
    h->max_gene_sweeps = v[1];
    return INSIDER_OK;
}

void clear_events(insider_hip_handle *h)
{
    for (auto *v : {&h->ev_col, &h->ev_row, &h->ev_cd, &h->ev_test}) v->clear();
}

// host row/column factors -> padded device layout (the reference aliases R's memory, src/optimize.cpp:283-284)
int upload_factors(insider_hip_handle *h, double *const *A, const double *C, int K)
{
    const DataSet &d = *h->ds;
    const int KP = h->ws.KP;
    const hipStream_t st = h->st.stream;
    for (int b = 0; b < d.blocks(); ++b) {
        const DataSet::Block blk = d.block(b);
        HIPCHECK(hipMemcpyAsync(h->ws.stage, A[b], (size_t)blk.rows * K * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pack_A, dim3(cdiv(blk.rows * KP, 256)), dim3(256), 0, st, (const double *)h->ws.stage, blk.rows, K, KP,
                           h->ws.Astack + (size_t)blk.off * KP);
        KCHECK();
        HIPCHECK(hipStreamSynchronize(st));   // stage is reused
    }
    if (!C) return INSIDER_OK;   // (the row factors alone: insider_hip_col_stats)
    HIPCHECK(hipMemcpyAsync(h->ws.stage, C, (size_t)d.p * K * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pack_rows, dim3(cdiv(d.p * KP, 256)), dim3(256), 0, st, (const double *)h->ws.stage, d.p, K, KP, h->ws.C);
    KCHECK();
    return INSIDER_OK;
}

// device factors -> the caller's buffers (the reference returns copies AND has mutated its inputs in place, :413-421)
int download_factors(insider_hip_handle *h, double *const *A, double *C, int K)
{
    const DataSet &d = *h->ds;
    const int KP = h->ws.KP;
    const hipStream_t st = h->st.stream;
    for (int b = 0; A && b < d.blocks(); ++b) {
        const DataSet::Block blk = d.block(b);
        hipLaunchKernelGGL(k_unpack_A, dim3(cdiv(blk.rows * K, 256)), dim3(256), 0, st,
                           (const double *)(h->ws.Astack + (size_t)blk.off * KP), blk.rows, K, KP, h->ws.stage);
        KCHECK();
        HIPCHECK(hipMemcpyAsync(A[b], h->ws.stage, (size_t)blk.rows * K * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
    }
    if (C) {
        hipLaunchKernelGGL(k_unpack_rows, dim3(cdiv(d.p * K, 256)), dim3(256), 0, st, (const double *)h->ws.C, d.p, K, KP,
                           h->ws.stage);
        KCHECK();
        HIPCHECK(hipMemcpyAsync(C, h->ws.stage, (size_t)d.p * K * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
    }
    return INSIDER_OK;
}

// C C' and S_i C' for the row step (src/optimize.cpp:332 and the unmasked part of :166,188)
int launch_row_prep(insider_hip_handle *h)
{
    int rc = launch_gram(h, h->ws.C, h->ds->p, h->ws.CCt);
    if (rc) return rc;
    // the merged update wants (S^train C'): the per-level sums of the TRAIN entries, i.e. (S C') minus sum_r bc_r
    return launch_mm_reduce_kp(h, h->plan.merged ? h->ds->Strain : h->ds->S, h->ds->SLP, h->ws.C, (int)h->ds->p, h->ds->SL, h->ws.sc_part, h->ws.SC);
}

int check_factor_args(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int tuning)
{
    if (!h || !A || !C) return fail(INSIDER_ERR_ARG, "null argument");
    if (tuning != 0 && tuning != 1)   // the reference prints and exit(1)s here (src/optimize.cpp:249-251)
        return fail(INSIDER_ERR_ARG, "Parameter tuning should be either 0 or 1!");
    if (inc_continuous != 0 && inc_continuous != 1)   // src/optimize.cpp:270-272
        return fail(INSIDER_ERR_ARG, "The value of prarameter inc_continuous can only be 0 or 1.");
    if (inc_continuous == 1 && h->ds->m == 0)
        return fail(INSIDER_ERR_ARG, "inc_continuous = 1 needs a handle created with ctns_confounder (insider_hip_create_ex)");
    if (inc_continuous == 0 && h->ds->m > 0)
        return fail(INSIDER_ERR_ARG, "this handle carries continuous covariates: pass inc_continuous = 1");
    for (int b = 0; b < h->ds->blocks(); ++b) if (!A[b]) return fail(INSIDER_ERR_ARG, "null row factor");
    return INSIDER_OK;
}

}  // namespace

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

#ifndef INSIDER_SOURCE_SHA
#define INSIDER_SOURCE_SHA "unknown-source-sha"   /* __graft_entry__.build() passes the hash of csrc/ + include/ (insider_amd/_build.py) */
#endif
const char *insider_hip_version(void) { return "insider_hip 0.4.0 (gfx950) src:" INSIDER_SOURCE_SHA; }

const char *insider_hip_last_error(void) { return g_err.c_str(); }

int insider_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"

namespace {
int stream_events(int c, int m) { return (c > 0 ? c : 1) + m; }   // Streams::ev_w: one per covariate and continuous column

// ---- insider_hip_create_ex in stages: each fills its part of the DataSet ---------------------------------------------------
struct CreateArgs {
    const double *X;
    int64_t n, p;
    const int32_t *levels;
    int c;
    const int32_t *n_levels;
    const double *ctns;
    int m;
    const uint8_t *M_train, *M_test;
};

int check_create_args(const CreateArgs &a, int device)
{
    if (!a.X || !a.levels || !a.n_levels || !a.M_train || !a.M_test) return fail(INSIDER_ERR_ARG, "null input");
    if (a.n < 1 || a.p < 1 || a.c < 1) return fail(INSIDER_ERR_ARG, "n, p, c must be positive");
    if (a.n > (1 << 30) || a.p > (1 << 30)) return fail(INSIDER_ERR_ARG, "dimension too large");
    if (a.n >= LIST_PAD || a.p >= LIST_PAD) return fail(INSIDER_ERR_UNSUPPORTED, "n and p must be below 2^23");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(INSIDER_ERR_NO_DEVICE, "no HIP device visible: libinsider_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(INSIDER_ERR_ARG, "bad device ordinal");
    // level ids must be exactly 1..L_i (src/optimize.cpp:175,286)
    for (int i = 0; i < a.c; ++i) {
        if (a.n_levels[i] < 1) return fail(INSIDER_ERR_ARG, "n_levels must be positive");
        for (int64_t r = 0; r < a.n; ++r) {
            const int32_t l = a.levels[r + (size_t)i * a.n];
            if (l < 1 || l > a.n_levels[i]) return fail(INSIDER_ERR_ARG, "level ids must be within 1..L_i");
        }
    }
    return INSIDER_OK;
}

// the host copies the later stages read instead of the caller's arrays
std::shared_ptr<const HostTables> host_tables(const CreateArgs &a)
{
    auto t = std::make_shared<HostTables>();
    t->lev0.resize((size_t)a.c * a.n);
    for (size_t e = 0; e < t->lev0.size(); ++e) t->lev0[e] = a.levels[e] - 1;
    if (a.m > 0) t->ctns.assign(a.ctns, a.ctns + (size_t)a.m * a.n);
    return t;
}

void describe(DataSet &d, const CreateArgs &a, int device)
{
    d.device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) d.n_simd = 4 * cus;
    d.n = a.n;
    d.p = a.p;
    d.c = a.c;
    d.ldn = round_up(a.n, CHUNK);
    d.ldp = round_up(a.p, CHUNK);
    d.n_levels.assign(a.n_levels, a.n_levels + a.c);
    d.lvl_off.assign(a.c + 1, 0);
    for (int i = 0; i < a.c; ++i) d.lvl_off[i + 1] = d.lvl_off[i] + a.n_levels[i];
    d.m = a.m;
    d.SLcat = d.lvl_off[a.c];
    d.SL = d.SLcat + a.m;
    d.SLP = (int)round_up(d.SL, 2);
    d.host = host_tables(a);
}

// ---- the mask-independent part -----------------------------------------------------------------------------------------------
// X (gene-major lines of pitch ldn)
int stage_matrix(DataSet &d, const CreateArgs &a, hipStream_t st)
{
    const int64_t n = a.n, p = a.p;
    int rc;
    if ((rc = d.X.alloc((size_t)p * d.ldn))) return rc;
    HIPCHECK(hipMemsetAsync(d.X, 0, (size_t)p * d.ldn * sizeof(double), st));
    HIPCHECK(hipMemcpy2DAsync(d.X, d.ldn * sizeof(double), a.X, n * sizeof(double), n * sizeof(double), p, hipMemcpyHostToDevice,
                              st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// mask codes (layout of X) from the caller's two masks
int codes_from_masks(DataSet &d, const uint8_t *M_train, const uint8_t *M_test, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    int rc;
    if ((rc = d.codes.alloc((size_t)p * d.ldn))) return rc;
    DevBuf<uint8_t> mtr, mte;
    if ((rc = mtr.alloc((size_t)n * p)) || (rc = mte.alloc((size_t)n * p))) return rc;
    HIPCHECK(hipMemcpyAsync(mtr, M_train, (size_t)n * p, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(mte, M_test, (size_t)n * p, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_make_codes, dim3(cdiv(p * d.ldn, 256)), dim3(256), 0, st, mtr, mte, n, p, d.ldn, d.codes);
    KCHECK();
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// mask codes of one fold from the resident fold ids: nothing is uploaded
int codes_from_fold(DataSet &d, const FoldIds &f, int fold, hipStream_t st)
{
    int rc;
    if ((rc = d.codes.alloc((size_t)d.p * d.ldn))) return rc;
    const int blocks = (int)std::min<int64_t>(cdiv(d.p, 4), 8 * (int64_t)d.n_simd);
    hipLaunchKernelGGL(k_fold_codes, dim3(blocks), dim3(256), 0, st, (const uint8_t *)f.id, (int)d.n, (int)d.p, (int)d.ldn, fold,
                       d.codes);
    KCHECK();
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// level tables: members of every level, and the chunk tables of the two-stage level reduction
int stage_levels(DataSet &d, const CreateArgs &a)
{
    const int64_t n = a.n;
    const int c = a.c;
    const std::vector<int> &lev0 = d.host->lev0;
    std::vector<int> members((size_t)c * n), lvl_ptr((size_t)d.SLcat + c), lvl_count(d.SLcat);
    d.cov.resize(c);
    int rc;
    for (int i = 0; i < c; ++i) {
        const int L = a.n_levels[i];
        std::vector<int> cnt(L, 0);
        for (int64_t r = 0; r < n; ++r) cnt[lev0[(size_t)i * n + r]]++;
        int *ptr = lvl_ptr.data() + d.lvl_off[i] + i;
        ptr[0] = 0;
        for (int l = 0; l < L; ++l) { ptr[l + 1] = ptr[l] + cnt[l]; lvl_count[d.lvl_off[i] + l] = cnt[l]; }
        std::vector<int> fill(ptr, ptr + L);
        for (int64_t r = 0; r < n; ++r) members[(size_t)i * n + fill[lev0[(size_t)i * n + r]]++] = (int)r;
        std::vector<int> ch_level, ch_begin, ch_end, lcp(L + 1, 0);
        for (int l = 0; l < L; ++l) {
            lcp[l] = (int)ch_level.size();
            for (int b = ptr[l]; b < ptr[l + 1]; b += LEVEL_CHUNK) {
                ch_level.push_back(l);
                ch_begin.push_back(b);
                ch_end.push_back(std::min(b + LEVEL_CHUNK, ptr[l + 1]));
            }
        }
        lcp[L] = (int)ch_level.size();
        CovTables &ct = d.cov[i];
        ct.L = L;
        ct.nchunks = (int)ch_level.size();
        d.max_chunks = std::max(d.max_chunks, ct.nchunks);
        d.max_L = std::max(d.max_L, L);
        if ((rc = ct.chunk_level.upload(ch_level)) || (rc = ct.chunk_begin.upload(ch_begin)) || (rc = ct.chunk_end.upload(ch_end)) ||
            (rc = ct.lvl_chunk_ptr.upload(lcp)))
            return rc;
    }
    if ((rc = d.lev.upload(lev0)) || (rc = d.members_all.upload(members)) || (rc = d.lvl_ptr_all.upload(lvl_ptr)) ||
        (rc = d.lvl_count_all.upload(lvl_count)) || (rc = d.lvl_off_d.upload(d.lvl_off)))
        return rc;
    return INSIDER_OK;
}

// continuous covariates: one pseudo-level whose members are all samples, weighted by z
int stage_continuous(DataSet &d, const CreateArgs &a)
{
    const int64_t n = a.n;
    if (a.m == 0) return INSIDER_OK;
    int rc;
    if ((rc = d.Zc.alloc((size_t)a.m * n))) return rc;
    HIPCHECK(hipMemcpy(d.Zc, a.ctns, (size_t)a.m * n * sizeof(double), hipMemcpyHostToDevice));   // n x m column-major == m x n rows
    std::vector<int> ident(n), cb, ce, lcp(2, 0);
    for (int64_t r = 0; r < n; ++r) ident[r] = (int)r;
    for (int64_t b0 = 0; b0 < n; b0 += LEVEL_CHUNK) { cb.push_back((int)b0); ce.push_back((int)std::min<int64_t>(b0 + LEVEL_CHUNK, n)); }
    lcp[1] = (int)cb.size();
    d.cont.L = 1;
    d.cont.nchunks = (int)cb.size();
    d.max_chunks = std::max(d.max_chunks, d.cont.nchunks);
    d.max_L = std::max(d.max_L, 1);
    if ((rc = d.ident_members.upload(ident)) || (rc = d.cont.chunk_begin.upload(cb)) || (rc = d.cont.chunk_end.upload(ce)) ||
        (rc = d.cont.lvl_chunk_ptr.upload(lcp)) || (rc = d.one_count.upload(std::vector<int>{1})))
        return rc;
    return INSIDER_OK;
}

// per-level sums of X over all entries
int stage_all_sums(DataSet &d, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    const int c = d.c, m = d.m;
    int rc;
    if ((rc = d.S.alloc((size_t)p * d.SLP))) return rc;
    HIPCHECK(hipMemsetAsync(d.S, 0, (size_t)p * d.SLP * sizeof(double), st));
    hipLaunchKernelGGL(k_level_sums, dim3(cdiv(p * d.SLcat, 256)), dim3(256), 0, st, (const double *)d.X, (const uint8_t *)nullptr,
                       d.ldn, (int)p, (const int *)d.members_all, (const int *)d.lvl_ptr_all, (const int *)d.lvl_off_d, c, (int)n,
                       d.SLcat, d.SLP, d.S);
    if (m > 0)
        hipLaunchKernelGGL(k_cont_sums, dim3(cdiv(p * m, 256)), dim3(256), 0, st, (const double *)d.X, d.ldn, (int)p,
                           (const double *)d.Zc, m, (int)n, d.SLcat, d.SLP, d.S);
    KCHECK();
    return INSIDER_OK;
}

// the merged row update's tables exist for data sets of this shape (stage_merged)
bool merged_shape(const DataSet &d) { return d.m <= 4 && (size_t)4 * (d.SLcat + GU_TILE) * sizeof(double) <= 64 * 1024; }

// level-pair sample counts of the merged row update (insider_row_merged.hpp): they count samples, not entries
int stage_pair_tables(DataSet &d)
{
    const int64_t n = d.n;
    const int c = d.c, m = d.m;
    if (!merged_shape(d)) return INSIDER_OK;
    const std::vector<int> &lev0 = d.host->lev0;
    const double *ctns = d.host->ctns.data();
    int rc;
    for (int i = 0; i < c; ++i) {
        // samples per (level of covariate i, stacked level of another covariate): sum_{r in l} s_r = paircnt A
        // (+ m columns sum_{r in l} z_rk: a continuous column is a stacked "level" with real-valued counts)
        std::vector<double> pc((size_t)d.cov[i].L * d.SL, 0.0);
        for (int64_t r = 0; r < n; ++r) {
            const int l = lev0[(size_t)i * n + r];
            for (int q = 0; q < c; ++q)
                if (q != i) pc[(size_t)l * d.SL + d.lvl_off[q] + lev0[(size_t)q * n + r]] += 1.0;
            for (int k = 0; k < m; ++k) pc[(size_t)l * d.SL + d.SLcat + k] += ctns[(size_t)k * n + r];
        }
        if ((rc = d.cov[i].paircnt.upload(pc))) return rc;
    }
    if (m == 0 || c > CF_MAXC) return INSIDER_OK;
    // the continuous columns as one-level covariates (stage_cont_factored): their pair "counts" and |l| = sum_r z_rk^2
    std::vector<double> zz((size_t)m * m, 0.0);
    for (int k = 0; k < m; ++k)
        for (int k2 = 0; k2 < m; ++k2) {
            double acc = 0.0;
            for (int64_t r = 0; r < n; ++r) acc += ctns[(size_t)k * n + r] * ctns[(size_t)k2 * n + r];
            zz[(size_t)k * m + k2] = acc;
        }
    std::vector<double> cc(m);
    d.cont_pair.resize(m);
    for (int k = 0; k < m; ++k) {
        std::vector<double> pc((size_t)d.SL, 0.0);
        for (int64_t r = 0; r < n; ++r)
            for (int q = 0; q < c; ++q) pc[d.lvl_off[q] + lev0[(size_t)q * n + r]] += ctns[(size_t)k * n + r];
        for (int k2 = 0; k2 < m; ++k2) pc[d.SLcat + k2] = k2 == k ? 0.0 : zz[(size_t)k * m + k2];
        if ((rc = d.cont_pair[k].upload(pc))) return rc;
        cc[k] = zz[(size_t)k * m + k];
    }
    return d.cont_cnt.upload(cc);
}

// ---- the mask-dependent part: run from the device codes and the data set's own copies alone ------------------------------------
// factor-independent statistics of the masks: per-gene sums of squares, per-level sums of X over the train entries, entry counts
int stage_sums(DataSet &d, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    const int c = d.c;
    int rc;
    // (the kernel forms both sums of squares; a data set that holds its source's yy_all writes the second one to a scratch line)
    DevBuf<double> yy_scratch;
    const bool own_all = !d.yy_all;
    if ((rc = d.yy_train.alloc((size_t)p)) || (rc = (own_all ? d.yy_all : yy_scratch).alloc((size_t)p))) return rc;
    DevBuf<unsigned long long> cnt;
    if ((rc = cnt.alloc(3))) return rc;
    HIPCHECK(hipMemsetAsync(cnt, 0, 3 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_line_sumsq, dim3(cdiv(p, 4)), dim3(256), 0, st, (const double *)d.X, (const uint8_t *)d.codes, d.ldn, (int)n,
                       (int)p, d.yy_train, own_all ? d.yy_all.get() : yy_scratch.get(), cnt);
    // train-only sums for the merged masked row update / the factored column statistics (the categorical columns)
    if ((rc = d.Strain.alloc((size_t)p * d.SLP))) return rc;
    HIPCHECK(hipMemsetAsync(d.Strain, 0, (size_t)p * d.SLP * sizeof(double), st));
    hipLaunchKernelGGL(k_level_sums, dim3(cdiv(p * d.SLcat, 256)), dim3(256), 0, st, (const double *)d.X, (const uint8_t *)d.codes,
                       d.ldn, (int)p, (const int *)d.members_all, (const int *)d.lvl_ptr_all, (const int *)d.lvl_off_d, c, (int)n,
                       d.SLcat, d.SLP, d.Strain);
    KCHECK();
    unsigned long long hc[3];
    HIPCHECK(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    d.cnt_train = (double)hc[0];
    d.cnt_test = (double)hc[1];
    d.no_na = hc[2] == 0;   // (not cnt_train + cnt_test == n p: an entry that is train and test would hide an NA entry)
    return INSIDER_OK;
}

// held-out lists of both sides (the masks never change: built once).  The row side is read from transposed copies
// (sample-major lines of pitch ldp) that live only here.
int stage_lists(DataSet &d, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    int rc;
    DevBuf<double> Xt;
    DevBuf<uint8_t> codes_t;
    if ((rc = Xt.alloc((size_t)n * d.ldp)) || (rc = codes_t.alloc((size_t)n * d.ldp))) return rc;
    HIPCHECK(hipMemsetAsync(Xt, 0, (size_t)n * d.ldp * sizeof(double), st));
    HIPCHECK(hipMemsetAsync(codes_t, CODE_TRAIN, (size_t)n * d.ldp, st));
    const dim3 grid(cdiv(n, 32), cdiv(p, 32));   // input: p lines (rows) x n columns
    hipLaunchKernelGGL((k_transpose<double>), grid, dim3(256), 0, st, (const double *)d.X, p, n, d.ldn, Xt, d.ldp);
    hipLaunchKernelGGL((k_transpose<uint8_t>), grid, dim3(256), 0, st, (const uint8_t *)d.codes, p, n, d.ldn, codes_t, d.ldp);
    KCHECK();
    for (int side = 0; side < 2; ++side) {
        const bool cols = side == 0;
        const int lines = cols ? (int)p : (int)n, len = cols ? (int)n : (int)p;
        const double *vals = cols ? d.X : Xt;
        const uint8_t *cds = cols ? d.codes : codes_t;
        const int64_t pitch = cols ? d.ldn : d.ldp;
        DevBuf<int> cnt_d;
        if ((rc = cnt_d.alloc((size_t)lines))) return rc;
        hipLaunchKernelGGL(k_count_heldout, dim3(cdiv(lines, 4)), dim3(256), 0, st, cds, pitch, len, lines, cnt_d);
        KCHECK();
        std::vector<int> cnt(lines);
        HIPCHECK(hipMemcpyAsync(cnt.data(), cnt_d, (size_t)lines * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        std::vector<uint32_t> ptr((size_t)lines + 1);
        uint64_t tot = 0;
        for (int i = 0; i < lines; ++i) { ptr[i] = (uint32_t)tot; tot += (uint64_t)round_up(cnt[i], LIST_ALIGN); }
        ptr[lines] = (uint32_t)tot;
        if (tot >= (1ull << 32)) return fail(INSIDER_ERR_UNSUPPORTED, "more than 2^32 held-out entries");
        DevBuf<uint32_t> &dptr = cols ? d.col_ptr : d.row_ptr;
        DevBuf<int> &didx = cols ? d.col_idx : d.row_idx;
        DevBuf<double> &dval = cols ? d.col_val : d.row_val;
        (cols ? d.col_entries : d.row_entries) = tot;
        if ((rc = dptr.upload(ptr)) || (rc = didx.alloc((size_t)tot + LIST_BLOCK)) || (rc = dval.alloc((size_t)tot + LIST_BLOCK)))
            return rc;
        uint8_t *dflag = nullptr;
        if (cols && !d.no_na) {
            if ((rc = d.col_flag.alloc((size_t)tot + LIST_BLOCK))) return rc;
            dflag = d.col_flag;
        }
        hipLaunchKernelGGL(k_fill_lists, dim3(cdiv(lines, 4)), dim3(256), 0, st, vals, cds, pitch, len, lines, (const uint32_t *)dptr,
                           didx, dval, dflag);
        KCHECK();
        HIPCHECK(hipStreamSynchronize(st));
    }
    return INSIDER_OK;
}

constexpr uint32_t SEG = 1024;   // list entries per weighted-SYRK work item (multiple of LIST_ALIGN)

// merged masked row update: per covariate, the genes' held-out samples grouped by level, the (gene, count) lists of every
// level and the level-pair sample counts (insider_row_merged.hpp).
// (k_gene_u keeps a gene's SLcat look-up values per wave in LDS: beyond ~1500 stacked levels the per-sample path stays)
// (with continuous covariates, m <= 4: the same tables serve the pair-count column statistics, ColFacArgs::zt)
// (the level-pair sample counts do not depend on the masks: stage_pair_tables)
int stage_merged(DataSet &d, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    const int c = d.c;
    if (!merged_shape(d)) return INSIDER_OK;
    int rc;
    for (int i = 0; i < c; ++i) {
        CovTables &ct = d.cov[i];
        const int L = ct.L;
        if ((rc = ct.grp.alloc((size_t)p * (L + 1)))) return rc;
        const size_t plane = (size_t)d.col_entries + LIST_BLOCK;
        if (d.SLcat > 65535) return fail(INSIDER_ERR_UNSUPPORTED, "more than 65535 levels in total");
        if ((rc = ct.slev.alloc(plane * (size_t)std::max(c - 1, 1)))) return rc;
        const size_t lds = (size_t)4 * L * sizeof(int);
        if (lds > 60 * 1024) return fail(INSIDER_ERR_UNSUPPORTED, "a covariate has more than 3840 levels");
        hipLaunchKernelGGL(k_group_count, dim3(cdiv(p, 4)), dim3(256), lds, st, (const uint32_t *)d.col_ptr, (const int *)d.col_idx,
                           (const int *)(d.lev + (size_t)i * n), L, (int)p, ct.grp);
        hipLaunchKernelGGL(k_group_fill, dim3(cdiv(p, 4)), dim3(256), lds, st, (const uint32_t *)d.col_ptr, (const int *)d.col_idx,
                           (const int *)d.lev, (const int *)d.lvl_off_d, c, (int)n, i, L, (int)p, (const uint32_t *)ct.grp, ct.slev,
                           plane);
        KCHECK();
        std::vector<uint32_t> grp((size_t)p * (L + 1));
        HIPCHECK(hipMemcpyAsync(grp.data(), ct.grp, grp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        // (gene, count) list of every level, padded to LIST_ALIGN; work items of at most SEG entries
        std::vector<int> widx, lip(L + 1, 0);
        std::vector<double> ww;
        std::vector<uint32_t> ib, ie;
        for (int l = 0; l < L; ++l) {
            lip[l] = (int)ib.size();
            const size_t start = widx.size();
            for (int64_t j = 0; j < p; ++j) {
                const uint32_t cnt = grp[(size_t)j * (L + 1) + l + 1] - grp[(size_t)j * (L + 1) + l];
                if (cnt) { widx.push_back((int)j); ww.push_back((double)cnt); }
            }
            while ((widx.size() - start) % LIST_ALIGN) { widx.push_back(LIST_PAD); ww.push_back(0.0); }
            for (size_t b = start; b < widx.size(); b += SEG) {
                ib.push_back((uint32_t)b);
                ie.push_back((uint32_t)std::min(b + SEG, widx.size()));
            }
        }
        lip[L] = (int)ib.size();
        if (widx.size() >= (1ull << 32)) return fail(INSIDER_ERR_UNSUPPORTED, "level lists too long");
        ct.nitems = (int)ib.size();
        ct.npairs = 0;
        for (double wv : ww) ct.npairs += wv != 0.0;
        d.max_items = std::max(d.max_items, ct.nitems);
        if ((rc = ct.wl_idx.upload(widx, widx.size() + LIST_BLOCK)) || (rc = ct.wl_w.upload(ww, ww.size() + LIST_BLOCK)) ||
            (rc = ct.item_begin.upload(ib, ib.size() + 1)) || (rc = ct.item_end.upload(ie, ie.size() + 1)) ||
            (rc = ct.lvl_item_ptr.upload(lip)))
            return rc;
    }
    d.merged = true;
    if ((rc = d.Sheld.alloc((size_t)p * d.SLP))) return rc;
    hipLaunchKernelGGL(k_sub, dim3(cdiv((int64_t)p * d.SLP, 256)), dim3(256), 0, st, (const double *)d.S, (const double *)d.Strain,
                       (size_t)p * d.SLP, d.Sheld);
    KCHECK();
    return INSIDER_OK;
}

// factored column statistics: covariates by decreasing level count, the planes of the later ones; the dense pair counts
// and half counts of the pair-count form when they are small enough
int stage_factored(DataSet &d, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    const int c = d.c;
    if (!d.merged || c > CF_MAXC) return INSIDER_OK;
    std::vector<int> ord(c);
    for (int i = 0; i < c; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return d.n_levels[x] > d.n_levels[y]; });
    ColFacArgs &cf = d.cf;
    cf.p = (int)p;
    cf.c = c;
    cf.plane = (size_t)d.col_entries + LIST_BLOCK;
    for (int t = 0; t < c; ++t) {
        const int o = ord[t];
        d.cf_pos[o] = t;
        cf.grp[t] = d.cov[o].grp;
        cf.slev[t] = d.cov[o].slev;
        cf.L[t] = d.n_levels[o];
        cf.off[t] = d.lvl_off[o];
        cf.nlater[t] = c - 1 - t;
        for (int k = t + 1; k < c; ++k) cf.later_plane[t][k - t - 1] = ord[k] < o ? ord[k] : ord[k] - 1;
    }
    cf.tab_skip_lo = d.lvl_off[ord[0]];
    cf.tab_skip_n = d.n_levels[ord[0]];
    cf.tab_rows = d.SLcat - cf.tab_skip_n;
    // pair-count form: the dense per-gene count tables (one byte per cell), when they are small enough
    cf.nsteps = (cf.tab_rows + 3) / 4;
    bool fits = cf.nsteps <= CP_MAXSTEPS;
    int off = 0;
    for (int t = 0; t < c; ++t) {
        const int cells = ((cf.L[t] + 15) / 16) * 64 * (cf.nsteps <= 4 ? 4 : 8);   // bytes: 4 or 8 per lane and block
        cf.cnt_off[t] = off;
        if (cf.nlater[t] > 0) off += cells;
    }
    cf.cnt_stride = off;
    cf.cnt = nullptr;
    int rc;
    if (fits && off <= 64 * 1024 && (size_t)p * (size_t)off <= ((size_t)1 << 32)) {   // <= 64 KB of counts per gene
        if (off > 0) {
            DevBuf<int> ovf;
            if ((rc = d.cf_cnt.alloc((size_t)p * off)) || (rc = ovf.alloc(1))) return rc;
            HIPCHECK(hipMemsetAsync(ovf, 0, sizeof(int), st));
            hipLaunchKernelGGL((k_pair_count_build<2>), dim3(cdiv(p, 2)), dim3(128), 0, st, cf, d.cf_cnt, ovf);
            KCHECK();
            int hv = 0;
            HIPCHECK(hipMemcpyAsync(&hv, ovf, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHECK(hipStreamSynchronize(st));
            fits = hv == 0;
        }
        if (fits && n < ((int64_t)1 << 24)) {   // (1/2 n as a float is exact)
            int hoff = 0;
            for (int t = 0; t < c; ++t) {
                cf.hn_off[t] = hoff;
                hoff += ((cf.L[t] + 15) / 16) * 16;
            }
            cf.hn_stride = hoff;
            if ((rc = d.cf_hn.alloc((size_t)(p + 4) * hoff))) return rc;   // + 4 zero rows: k_wgemm reads whole steps of four genes
            HIPCHECK(hipMemsetAsync(d.cf_hn, 0, (size_t)(p + 4) * hoff * sizeof(float), st));
            hipLaunchKernelGGL(k_half_counts, dim3((unsigned)cdiv((int64_t)p * hoff, 256)), dim3(256), 0, st, cf, d.cf_hn);
            KCHECK();
            // the level sums in k_col_paircnt4's order, for the launches that form Q themselves (stats_own_q, insider_plan.hpp)
            cf.sq_stride = hoff / 16 * CF_SQ_BLOCK;
            if (d.m == 0 && (int64_t)p * cf.sq_stride / 256 < ((int64_t)1 << 31)) {
                // (no room for the table: the data set stands without it and stats_own_q() keeps the products)
                if (d.cf_sq.alloc((size_t)p * cf.sq_stride)) { (void)hipGetLastError(); d.cf_sq.reset(); }
                else hipLaunchKernelGGL(k_own_q_table, dim3((unsigned)cdiv((int64_t)p * cf.sq_stride, 256)), dim3(256), 0, st, cf,
                                   (const double *)d.S, (const double *)d.Sheld, (int)d.SLP, (double *)d.cf_sq);
                KCHECK();
            }
        } else {
            fits = false;
        }
        d.cf_pair_ok = fits;
    }
    cf.zt = nullptr;
    cf.m = d.m;
    cf.SLcat = d.SLcat;
    for (int t = 0; t < c; ++t) cf.pos_cov[t] = ord[t];
    return INSIDER_OK;
}

// continuous covariates on the pair-count form: the real-valued count table, and the continuous columns as one-level
// covariates of the merged row update
int stage_cont_factored(DataSet &d, hipStream_t st)
{
    const int64_t n = d.n, p = d.p;
    const int c = d.c, m = d.m;
    // The merged row update with continuous columns takes u_j from k_gene_u_cnt ALONE (only it adds the term of the
    // real-valued counts, ColFacArgs::zt; k_gene_u reads the categorical columns of V only): every covariate's launch
    // of it must fit its per-wave LDS record — V row [SL] | out [LP] | GU_BATCH x 64 partial sums, four waves per block
    // — or the whole data set stays on the per-sample / per-entry paths (a covariate with ~770 levels or more).
    bool gu_fits = true;
    for (int t = 0; t < c; ++t)
        gu_fits = gu_fits && (size_t)4 * (d.SL + round_up(d.n_levels[t], 2) + GU_BATCH * WAVE) * sizeof(double) <= 64 * 1024;
    if (!(m > 0 && d.cf_pair_ok && gu_fits)) return INSIDER_OK;
    // one more position (the m columns as pseudo-levels, no count bytes, 1/2 n = 0: sixteen more zero floats per gene would
    // do, the block reads what follows its offset -> its own zero region) and the real-valued count table
    ColFacArgs &cf = d.cf;
    cf.L[c] = m;
    cf.off[c] = d.SLcat;
    cf.nlater[c] = 0;
    cf.cnt_off[c] = 0;
    int zoff = 0;
    for (int t = 0; t < c; ++t) { cf.zt_off[t] = zoff; zoff += ((cf.L[t] + 15) / 16) * 64; }
    cf.zt_off[c] = zoff;
    cf.zt_stride = zoff + 64;
    // 1/2 n of position c: a zero region behind the table (rebuilt with the longer stride)
    d.cf_hn.reset();
    cf.hn_off[c] = cf.hn_stride;
    cf.hn_stride += 16;
    int rc;
    if ((rc = d.cf_hn.alloc((size_t)(p + 4) * cf.hn_stride))) return rc;
    HIPCHECK(hipMemsetAsync(d.cf_hn, 0, (size_t)(p + 4) * cf.hn_stride * sizeof(float), st));
    hipLaunchKernelGGL(k_half_counts, dim3((unsigned)cdiv((int64_t)p * cf.hn_stride, 256)), dim3(256), 0, st, cf, d.cf_hn);
    KCHECK();
    if ((rc = d.cf_zt.alloc((size_t)p * cf.zt_stride))) return rc;
    HIPCHECK(hipMemsetAsync(d.cf_zt, 0, (size_t)p * cf.zt_stride * sizeof(double), st));
    // (Sheld's continuous columns: sum over the held-out entries of x z, next to S - S^train of the categorical ones)
    hipLaunchKernelGGL(k_zt_build, dim3(cdiv(p, 4)), dim3(256), 0, st, cf, (const uint32_t *)d.col_ptr, (const int *)d.col_idx,
                       (const double *)d.col_val, (const int *)d.lev, (const double *)d.Zc, (int)n, d.cf_zt, d.Sheld, d.SLP,
                       (const double *)d.S, d.Strain);
    KCHECK();
    HIPCHECK(hipStreamSynchronize(st));
    // ---- the continuous columns as one-level covariates of the merged row update: one (gene) list and work items for all ----
    const size_t plen_l = (size_t)round_up(p, LIST_ALIGN);
    std::vector<int> widx(plen_l, LIST_PAD);
    for (int64_t j = 0; j < p; ++j) widx[j] = (int)j;
    std::vector<uint32_t> ib, ie;
    for (size_t b = 0; b < plen_l; b += SEG) { ib.push_back((uint32_t)b); ie.push_back((uint32_t)std::min(b + SEG, plen_l)); }
    CovTables &lists = d.contm_lists;
    lists.L = 1;
    lists.nitems = (int)ib.size();
    lists.npairs = p;
    if ((rc = lists.wl_idx.upload(widx, plen_l + LIST_BLOCK)) || (rc = lists.item_begin.upload(ib, ib.size() + 1)) ||
        (rc = lists.item_end.upload(ie, ie.size() + 1)) || (rc = lists.lvl_item_ptr.upload(std::vector<int>{0, (int)ib.size()})))
        return rc;
    d.max_items = std::max(d.max_items, (int)ib.size());
    d.contm.resize(m);
    for (int k = 0; k < m; ++k) {
        CovTables &ct = d.contm[k];
        ct.L = 1;
        ct.nitems = lists.nitems;
        ct.npairs = p;
        if ((rc = ct.wl_w.alloc(plen_l + LIST_BLOCK))) return rc;
        HIPCHECK(hipMemsetAsync(ct.wl_w, 0, (plen_l + LIST_BLOCK) * sizeof(double), st));
        hipLaunchKernelGGL(k_cont_weights, dim3(cdiv(p, 256)), dim3(256), 0, st, (const double *)d.cf_zt, cf.zt_stride, cf.zt_off[c], k,
                           (int)p, ct.wl_w);
        KCHECK();
        ct.paircnt.share(d.cont_pair[k]);   // (mask-independent: stage_pair_tables)
    }
    HIPCHECK(hipStreamSynchronize(st));
    d.cont_merged = true;
    return INSIDER_OK;
}

// everything that depends on the masks, from the codes on the device: insider_hip_create_ex and the re-masks run this
int build_masked(DataSet &d, hipStream_t st)
{
    int rc;
    if ((rc = stage_sums(d, st)) || (rc = stage_lists(d, st)) || (rc = stage_merged(d, st)) || (rc = stage_factored(d, st)) ||
        (rc = stage_cont_factored(d, st)))
        return rc;
    return INSIDER_OK;
}

// d holds the mask-independent part of src jointly: the shape facts are copied, every device array is shared
void share_resident(DataSet &d, const DataSet &s)
{
    d.device = s.device; d.n_simd = s.n_simd;
    d.n = s.n; d.p = s.p; d.ldn = s.ldn; d.ldp = s.ldp;
    d.c = s.c; d.SL = s.SL; d.SLP = s.SLP; d.m = s.m; d.SLcat = s.SLcat;
    d.n_levels = s.n_levels; d.lvl_off = s.lvl_off;
    d.max_chunks = s.max_chunks; d.max_L = s.max_L;
    d.host = s.host;
    d.folds = s.get_folds();
    size_t b = 0;
    b += d.X.share(s.X) + d.lev.share(s.lev) + d.lvl_off_d.share(s.lvl_off_d) + d.members_all.share(s.members_all) +
         d.lvl_ptr_all.share(s.lvl_ptr_all) + d.lvl_count_all.share(s.lvl_count_all) + d.Zc.share(s.Zc) +
         d.one_count.share(s.one_count) + d.ident_members.share(s.ident_members) + d.S.share(s.S) + d.yy_all.share(s.yy_all) +
         d.cont_cnt.share(s.cont_cnt);
    auto chunks = [&b](CovTables &o, const CovTables &i) {
        o.L = i.L;
        o.nchunks = i.nchunks;
        b += o.chunk_level.share(i.chunk_level) + o.chunk_begin.share(i.chunk_begin) + o.chunk_end.share(i.chunk_end) +
             o.lvl_chunk_ptr.share(i.lvl_chunk_ptr) + o.paircnt.share(i.paircnt);
    };
    d.cov.resize(s.cov.size());
    for (size_t i = 0; i < s.cov.size(); ++i) chunks(d.cov[i], s.cov[i]);
    chunks(d.cont, s.cont);
    d.cont_pair.resize(s.cont_pair.size());
    for (size_t k = 0; k < s.cont_pair.size(); ++k) b += d.cont_pair[k].share(s.cont_pair[k]);
    if (d.folds) b += d.folds->id.bytes();
    d.bytes_shared = b;
}

// A handle with src's options and shard settings and a workspace, streams and diagnostics of its own (insider_hip_clone)
int handle_like(const insider_hip_handle *src, std::unique_ptr<insider_hip_handle> &h)
{
    h = std::make_unique<insider_hip_handle>();
    h->opt = src->opt;
    h->gene_offset = src->gene_offset;
    h->rank = src->rank;
    h->world = src->world;
    h->allreduce = src->allreduce;
    h->allreduce_user = src->allreduce_user;
    return h->st.create(stream_events(src->ds->c, src->ds->m));
}

// A handle on a new data set over src's resident X whose codes `make_codes` writes
template <typename F>
int derive(insider_hip_handle *src, insider_hip_handle **out, F make_codes)
{
    if (src->world > 1) return fail(INSIDER_ERR_UNSUPPORTED, "a gene-sharded handle cannot be re-masked");
    HIPCHECK(hipSetDevice(src->ds->device));
    // (d before h: on an error the handle drains its streams before the data set's buffers go)
    auto d = std::make_shared<DataSet>();
    std::unique_ptr<insider_hip_handle> h;
    int rc;
    if ((rc = handle_like(src, h))) return rc;
    share_resident(*d, *src->ds);
    {
        Tally own;
        if ((rc = make_codes(*d, (hipStream_t)h->st.stream)) || (rc = build_masked(*d, h->st.stream))) return rc;
        d->bytes_own = (size_t)own.bytes;
    }
    h->ds = std::move(d);
    *out = h.release();
    return INSIDER_OK;
}
}  // namespace

extern "C" {

void insider_hip_destroy(insider_hip_handle *h) { delete h; }

int insider_hip_clone(insider_hip_handle *src, insider_hip_handle **out)
{
    if (!out) return fail(INSIDER_ERR_ARG, "out is null");
    *out = nullptr;
    if (!src || !src->ds) return fail(INSIDER_ERR_ARG, "null handle");
    HIPCHECK(hipSetDevice(src->ds->device));
    // the data set, the options and the shard settings; a workspace, streams, diagnostics of its own (a sharded clone joins
    // its own communicator: insider_hip_comm_init)
    std::unique_ptr<insider_hip_handle> h;
    if (int rc = handle_like(src, h)) return rc;
    h->ds = src->ds;
    *out = h.release();
    return INSIDER_OK;
}

int insider_hip_remask(insider_hip_handle *src, const uint8_t *M_train, const uint8_t *M_test, insider_hip_handle **out)
{
    if (!out) return fail(INSIDER_ERR_ARG, "out is null");
    *out = nullptr;
    if (!src || !src->ds) return fail(INSIDER_ERR_ARG, "null handle");
    if (!M_train || !M_test) return fail(INSIDER_ERR_ARG, "null mask");
    return derive(src, out, [&](DataSet &d, hipStream_t st) { return codes_from_masks(d, M_train, M_test, st); });
}

int insider_hip_set_folds(insider_hip_handle *h, const uint8_t *fold_id, int F)
{
    if (!h || !h->ds || !fold_id) return fail(INSIDER_ERR_ARG, "null");
    if (F < 1 || F > 255) return fail(INSIDER_ERR_ARG, "F must be in 1..255");
    const DataSet &d = *h->ds;
    const size_t np = (size_t)d.n * (size_t)d.p;
    for (size_t e = 0; e < np; ++e)
        if (fold_id[e] > F) return fail(INSIDER_ERR_ARG, "fold ids must be within 0..F");
    HIPCHECK(hipSetDevice(d.device));
    auto f = std::make_shared<FoldIds>();
    f->F = F;
    if (int rc = f->id.alloc((size_t)d.p * d.ldn)) return rc;
    HIPCHECK(hipMemset(f->id, 0, (size_t)d.p * d.ldn));
    HIPCHECK(hipMemcpy2D(f->id, (size_t)d.ldn, fold_id, (size_t)d.n, (size_t)d.n, (size_t)d.p, hipMemcpyHostToDevice));
    std::lock_guard<std::mutex> g(d.fold_mu);
    d.folds = std::move(f);
    return INSIDER_OK;
}

int insider_hip_remask_fold(insider_hip_handle *src, int fold, insider_hip_handle **out)
{
    if (!out) return fail(INSIDER_ERR_ARG, "out is null");
    *out = nullptr;
    if (!src || !src->ds) return fail(INSIDER_ERR_ARG, "null handle");
    if (src->world > 1) return fail(INSIDER_ERR_UNSUPPORTED, "a gene-sharded handle cannot be re-masked");
    const std::shared_ptr<const FoldIds> f = src->ds->get_folds();
    if (!f) return fail(INSIDER_ERR_ARG, "no fold ids set: insider_hip_set_folds");
    if (fold < 1 || fold > f->F) return fail(INSIDER_ERR_ARG, "fold must be in 1..F");
    return derive(src, out, [&](DataSet &d, hipStream_t st) { return codes_from_fold(d, *f, fold, st); });
}

int insider_hip_create(const double *X, int64_t n, int64_t p, const int32_t *levels, int c, const int32_t *n_levels,
                       const uint8_t *M_train, const uint8_t *M_test, int device, insider_hip_handle **out)
{
    return insider_hip_create_ex(X, n, p, levels, c, n_levels, nullptr, 0, M_train, M_test, device, out);
}

int insider_hip_create_ex(const double *X, int64_t n, int64_t p, const int32_t *levels, int c, const int32_t *n_levels,
                          const double *ctns, int m, const uint8_t *M_train, const uint8_t *M_test, int device,
                          insider_hip_handle **out)
{
    if (m < 0 || (m > 0 && !ctns)) { if (out) *out = nullptr; return fail(INSIDER_ERR_ARG, "bad continuous covariates"); }
    if (!out) return fail(INSIDER_ERR_ARG, "out is null");
    *out = nullptr;
    const CreateArgs a{X, n, p, levels, c, n_levels, ctns, m, M_train, M_test};
    int rc = check_create_args(a, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    // (d before h: on an error the handle drains its streams before the data set's buffers go)
    auto d = std::make_shared<DataSet>();
    auto h = std::make_unique<insider_hip_handle>();
    describe(*d, a, device);
    if ((rc = h->st.create(stream_events(c, m)))) return rc;
    const hipStream_t st = h->st.stream;
    {
        Tally own;
        if ((rc = stage_matrix(*d, a, st)) || (rc = stage_levels(*d, a)) || (rc = stage_continuous(*d, a)) ||
            (rc = stage_all_sums(*d, st)) || (rc = stage_pair_tables(*d)) || (rc = codes_from_masks(*d, M_train, M_test, st)) ||
            (rc = build_masked(*d, st)))
            return rc;
        d->bytes_own = (size_t)own.bytes;
    }
    h->ds = std::move(d);
    *out = h.release();
    return INSIDER_OK;
}

int insider_hip_set_shard(insider_hip_handle *h, int64_t gene_offset, int rank, int world, insider_allreduce_fn fn,
                          void *user)
{
    if (!h || world < 1 || rank < 0 || rank >= world || gene_offset < 0) return fail(INSIDER_ERR_ARG, "bad shard");
    // world > 1 without a callback is completed by insider_hip_comm_init(); optimize() refuses to run with neither.
    // Installing a callback drops a communicator of an earlier insider_hip_comm_init(): the callback is then the exchange.
    if (fn && h->comm) {
        (void)hipSetDevice(h->ds->device);
        (void)ncclCommDestroy(h->comm);
        h->comm = nullptr;
    }
    h->gene_offset = gene_offset;
    h->rank = rank;
    h->world = world;
    h->allreduce = fn;
    h->allreduce_user = user;
    return INSIDER_OK;
}

int insider_hip_comm_unique_id(void *out, int out_bytes)
{
    if (!out || out_bytes < (int)sizeof(ncclUniqueId)) return fail(INSIDER_ERR_ARG, "unique-id buffer too small (INSIDER_COMM_ID_BYTES)");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(INSIDER_ERR_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memset(out, 0, (size_t)out_bytes);
    std::memcpy(out, &id, sizeof(id));
    return INSIDER_OK;
}

int insider_hip_comm_init(insider_hip_handle *h, const void *unique_id, int rank, int world)
{
    if (!h || !unique_id || world < 1 || rank < 0 || rank >= world) return fail(INSIDER_ERR_ARG, "bad communicator arguments");
    if (h->world != world || h->rank != rank) return fail(INSIDER_ERR_ARG, "rank / world differ from insider_hip_set_shard()");
    HIPCHECK(hipSetDevice(h->ds->device));
    if (h->comm) { (void)ncclCommDestroy(h->comm); h->comm = nullptr; }
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const ncclResult_t r = ncclCommInitRank(&h->comm, world, id, rank);
    if (r != ncclSuccess) { h->comm = nullptr; return fail(INSIDER_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)); }
    return INSIDER_OK;
}

int insider_hip_set_option(insider_hip_handle *h, const char *name, double value)
{
    if (!h || !name) return fail(INSIDER_ERR_ARG, "null");
    const std::string s(name);
    if (s == "max_sweeps") h->opt.max_sweeps = value < 1 ? 1 : (int)value;
    else if (s == "order_mode") h->opt.order_mode = (int)value;
    else if (s == "profile") h->opt.profile = (int)value;
    else if (s == "verbose") h->opt.verbose = (int)value;
    else if (s == "force_allreduce") h->opt.force_allreduce = (int)value;   // call the all-reduce callback even when world == 1
    else if (s == "col_factored") h->opt.col_factored = (int)value;   // 1 = cost model picks list / look-up / pair-count form (default), 2 = look-up form, 3 = pair-count form, 0 = k_list_stats
    else if (s == "row_counts") h->opt.row_counts = (int)value;   // 1 = the merged row update takes u from the dense pair counts when they exist (default), 0 = from the entry lists
    else if (s == "row_merged") h->opt.row_merged = (int)value;   // 1 = merged masked row update when the time model favours it (default), 2 = always, 0 = per-sample statistics
    else if (s == "row_gemm_waves") {   // (re-plans the workspace: the next call builds it anew)
        h->opt.wg_waves = std::max(64, (int)value);
        HIPCHECK(hipSetDevice(h->ds->device));
        h->ws = Workspace();
    }
    else if (s == "row_gemm") h->opt.row_gemm = (int)value;       // 1 (default) = k_wgemm for covariates with >= 49 levels, 0 = k_wsyrk everywhere
    else if (s == "row_fused") h->opt.row_fused = (int)value;     // 1 (default) = k_level_merged (one launch per covariate), 0 = k_level_pack / k_level_reduce / k_level_solve
    else if (s == "cd_cold_iters") h->opt.cd_cold_iters = (int)value;   // outer iterations 0 .. value-1 of a call solve in passes
    else if (s == "cd_pass1") h->opt.cd_pass_first = (int)value;        // sweep index where the first pass stops (0 = single pass)
    else if (s == "cd_pass_ratio") h->opt.cd_pass_ratio = (int)value;   // each further pass stops at ratio x the previous limit
    else if (s == "list_fine") h->opt.list_fine = (int)value;       // 1 (default) = per-entry statistics on v_mfma_f64_4x4x4 for 16 <= K <= 31, 0 = on 16x16x4
    else if (s == "mm_fast") h->opt.mm_fast = (int)value;             // 0 = k_mm_rows / k_mm_reduce as in round 4
    else if (s == "mm_tiles") h->opt.mm_tiles = value < 1 ? 0 : (int)value;   // tiles of 16 rows per wave of k_mm_rows2 (0, default = as many as keep the grid at two waves per SIMD)
    else if (s == "stats_own_q") h->opt.stats_own_q = (int)value;     // 1 = k_col_paircnt4 forms Q and Qheld itself where a column solve follows, 2 = in insider_hip_col_stats too, 0 = never
    else if (s == "col_mfma4") h->opt.col_mfma4 = (int)value;         // 1 = k_col_paircnt4 (K <= 31, factor rows fit LDS), 0 = k_col_paircnt
    else if (s == "cd_pairs") h->opt.cd_pairs = (int)value;           // 1 (default) = sweeps routed through the blocks of two coordinate steps (K <= 30; same iterates), 0 = one step per block
    else if (s == "resid_stage_mb") h->opt.resid_stage_mb = value;   // device buffer insider_hip_residual() copies out through (MB; at least 16 genes of the window)
    else if (s == "vd_stage_kb") h->opt.vd_stage_kb = value;         // LDS budget (KiB, default 48, at most 60) of the staged level tables of k_vd_stats (0 = always the global form)
    else if (s == "ls_slabs") h->opt.ls_slabs = value < 1 ? 0 : (int)std::min(value, 256.0);   // gene slabs of k_ls_prod (0 = from n, p, the compute units and "ls_part_mb"; at most 256)
    else if (s == "rc_slabs") h->opt.rc_slabs = value < 1 ? 0 : (int)std::min(value, 256.0);   // gene slabs of k_rc_fwd (0 = from n, p, the compute units and "ls_part_mb"; at most 256)
    else if (s == "ls_part_mb") h->opt.ls_part_mb = value;          // bound (MB, default 256) on the partial scores of the automatic slab count of k_ls_prod
    else if (s == "glm_slabs") h->opt.glm_slabs = value < 1 ? 0 : (int)std::min(value, 64.0);   // gene slabs of k_resid_stats (0 = from n and the compute units; at most 64)
    else if (s == "sd_slabs") h->opt.sd_slabs = value < 1 ? 0 : (int)std::min(value, 256.0);   // gene slabs of k_sd_stats (0 = from n, p and the compute units; at most 256)
    else if (s == "cd_variant") h->opt.cd_variant = (int)value;   // 0 = register-resident (4 genes per wave; K <= 32, and 32 < K <= 48 with the third slot's columns in LDS), 1 = group kernel, 2 = row16 (LDS, K <= 48)
    else return fail(INSIDER_ERR_ARG, "unknown option " + s);
    return INSIDER_OK;
}

// Nothing of an earlier call is owed any more: its joins, its level Gram sums, its timer events.  drain: an early return
// leaves enqueued work on every stream, so they are drained first and the next call starts clean
static void reset_call_state(insider_hip_handle *h, bool drain)
{
    if (drain) (void)hipSetDevice(h->ds->device);
    if (drain) h->st.synchronize();
    h->w_ready = false;
    for (Join *j : {&h->st.qfull, &h->st.qheld, &h->st.side_done}) j->drop();
    clear_events(h);
}

// the sub-problem tolerance's factor from the last checkpoint's loss decrease (src/optimize.cpp:389-403)
static double decay_for(double delta_loss)
{
    for (double d : {1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1})
        if (delta_loss / 1000 <= d) return d;
    return 1.0;
}

// profile of the call that has just ended (insider_hip_profile): launches and HIP-event time per timed kernel, the steady-state
// means, and which statistics paths its plan ran
static void profile_summary(insider_hip_handle *h, double wall_ms, double iterations, double sweeps_total)
{
    for (double &v : h->prof) v = 0;
    auto sum_events = [](std::vector<Event> &ev, size_t first, double *launches, double *ms) {
        for (size_t i = first; i + 1 < ev.size(); i += 2) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) { *ms += t; *launches += 1; }
        }
    };
    sum_events(h->ev_col, 0, &h->prof[0], &h->prof[1]);
    sum_events(h->ev_row, 0, &h->prof[2], &h->prof[3]);
    sum_events(h->ev_cd, 0, &h->prof[4], &h->prof[5]);
    sum_events(h->ev_test, 0, &h->prof[6], &h->prof[7]);
    auto tail_mean = [&](std::vector<Event> &ev) {   // one event pair per outer iteration: the mean from iteration 5 on
        double ms = 0.0, cnt = 0.0;
        sum_events(ev, 10, &cnt, &ms);
        return cnt ? ms / cnt : 0.0;
    };
    h->steady_cd_ms = tail_mean(h->ev_cd);
    h->steady_col_ms = tail_mean(h->ev_col);
    h->prof[8] = wall_ms;
    h->prof[9] = iterations;
    h->prof[10] = sweeps_total;
    const FitPlan &p = h->plan;
    h->prof[11] = (p.masked && p.col_path != 0 ? 1.0 : 0.0) + (p.merged ? 2.0 : 0.0) + (p.masked && p.col_path == 2 ? 4.0 : 0.0);
    clear_events(h);
}

static int optimize_body(insider_hip_handle *h, double *const *A, double *C, int inc_continuous, int K, double lambda1,
                         double lambda2, double alpha, int tuning, double global_tol, double sub_tol, uint32_t max_iter,
                         uint64_t seed, double *out_train_rmse, double *out_test_rmse, double *out_loss, double *traj,
                         int traj_cap, int *out_traj_rows, int *out_iters)
{
    int rc = check_factor_args(h, A, C, inc_continuous, tuning);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(h->ds->device));
    // work a failed earlier call may have left on the side streams must not race with this call's
    if ((rc = h->st.synchronize_sides())) return rc;
    if ((rc = ensure_workspace(h, K))) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    reset_call_state(h, false);
    h->row_kernels = 0;
    const int masked = tuning == 1;
    const ColCall col{alpha, lambda2 * alpha};
    plan_call(h, masked, &col);
    const FitPlan &plan = h->plan;
    if ((rc = upload_factors(h, A, C, K))) return rc;

    // ---- fit of the initial values (src/optimize.cpp:320-323) ----------------------------------------------------
    LossOut lo;
    if ((rc = phase_R(h))) return rc;
    if (masked) if ((rc = launch_col_stats(h, false))) return rc;
    if ((rc = launch_col_solve(h, masked, false, lambda2, alpha, sub_tol, 1, false))) return rc;
    if ((rc = launch_test_sse(h, masked, false))) return rc;
    if ((rc = loss_checkpoint(h, tuning, lambda1, lambda2, alpha, &lo))) return rc;
    double loss = lo.loss, pre_loss, decay = 1.0;
    double train_rmse = lo.train_rmse, test_rmse = lo.test_rmse;
    int trows = 0;
    auto put_traj = [&](double it, double delta, double dec) {
        if (traj && trows < traj_cap) {
            double *t = traj + (size_t)trows * INSIDER_TRAJ_STRIDE;
            t[0] = it; t[1] = lo.train_rmse; t[2] = lo.test_rmse; t[3] = lo.sum_residual / 2; t[4] = lo.row_reg_half;
            t[5] = lo.col_reg_half; t[6] = lo.l1_reg; t[7] = lo.loss; t[8] = delta; t[9] = dec;
            ++trows;
        }
    };
    put_traj(-1, std::numeric_limits<double>::quiet_NaN(), decay);

    uint32_t iter = 0;
    unsigned long long sweeps_total = 0;
    HIPCHECK(hipMemsetAsync(h->ws.sweep_total, 0, 256 * sizeof(unsigned long long), h->st.stream));
    HIPCHECK(hipMemsetAsync(h->ws.failflag + 2, 0, 2 * sizeof(int), h->st.stream));
    if (alpha != 0.0 && !h->ws.have_perm && !h->ws.have_early[0]) {   // no history on this handle: order the genes by sum of squares
        hipLaunchKernelGGL(k_yy_key, dim3(cdiv(h->ds->p, 256)), dim3(256), 0, h->st.stream,
                           (const double *)(masked ? h->ds->yy_train : h->ds->yy_all), (int)h->ds->p, h->ws.sweep_key);
        KCHECK();
        if ((rc = launch_gene_order(h, nullptr, 0, 1, h->st.stream))) return rc;
        h->ws.have_perm = true;
    }
    while (iter <= max_iter) {                                                                  // :325
        if (h->opt.verbose && iter % 10 == 0) printf("Iteration %u ---------------------------------\n", iter);
        // ---- row step: all covariates, Gauss-Seidel (:332-362) -------------------------------------------------
        if (plan.merged) {
            if ((rc = launch_wsyrk_side(h))) return rc;                                         // incl. the row prep
            // V = C A' of the covariates 1 .. c-1: what covariate 0's update reads.  Covariate 0's own columns are first read by
            // covariate 1's update, after they have been recomputed from the updated factors (below): not formed here
            // (with continuous covariates on the merged form: their columns of V too — s_r carries A_c' z_r)
            if ((rc = launch_gene_v(h, h->ds->c > 1 ? h->ds->lvl_off[1] : h->ds->SLcat, h->ds->SL))) return rc;
            HIPCHECK(hipStreamWaitEvent(h->st.stream, h->st.ev_head, 0));                         // launch_wsyrk_side
        } else {
            if ((rc = launch_row_prep(h))) return rc;                                           // :332
            if (masked) if ((rc = launch_row_stats(h, true))) return rc;
        }
        const bool cont_follow = inc_continuous && h->ds->m > 0;
        for (int i = 0; i < h->ds->c; ++i) {
            const bool need_R = !(plan.merged || plan.unmasked_fused) || (i + 1 == h->ds->c && !cont_follow);
            if ((rc = row_update(h, i, -1, masked, lambda1, need_R))) return rc;                // :339
            if (plan.merged && (i + 1 < h->ds->c || cont_follow))   // (the continuous columns read every categorical column of V)
                if ((rc = launch_gene_v(h, h->ds->lvl_off[i], h->ds->lvl_off[i + 1]))) return rc;
        }
        if (cont_follow)
            for (int j = 0; j < h->ds->m; ++j) {
                if ((rc = row_update(h, 0, j, masked, lambda1, !plan.merged || j + 1 == h->ds->m))) return rc;   // :340-351
                if (plan.merged && j + 1 < h->ds->m)
                    if ((rc = launch_gene_v(h, h->ds->SLcat + j, h->ds->SLcat + j + 1))) return rc;
            }
        h->w_ready = false;
        // ---- column step (:365-378) -------------------------------------------------------------------------------
        if ((rc = phase_R(h, true, true, masked != 0))) return rc;
        const int checkpoint = iter % 10 == 0;
        if (alpha != 0.0 && iter == 0)   // later iterations: built on the side stream while the previous solve ran
            if ((rc = ensure_order_table(h, seed, iter, K, h->opt.max_sweeps, h->opt.order_mode, nullptr, 0))) return rc;
        if (masked) if ((rc = launch_col_stats(h, true))) return rc;
        if (alpha != 0.0) {
            h->ws.order = h->ws.order_buf[iter & 1];
            if (iter < max_iter) {   // the next iteration's table, from here on: beside this iteration's solve
                HIPCHECK(hipEventRecord(h->st.ev_tab, h->st.stream));
                HIPCHECK(hipStreamWaitEvent(h->st.side, h->st.ev_tab, 0));
                if ((rc = ensure_order_table(h, seed, iter + 1, K, h->opt.max_sweeps, h->opt.order_mode, h->st.side, (int)((iter + 1) & 1))))
                    return rc;
            }
        }
        if ((rc = launch_col_solve(h, masked, true, lambda2, alpha, sub_tol * decay, checkpoint, true, (int)iter, true))) return rc;  // :376
        if (alpha != 0.0)
            if ((rc = side_close(h))) return rc;
        if (checkpoint) {                                                                       // :381-408
            if ((rc = launch_test_sse(h, masked, true))) return rc;
            pre_loss = loss;
            if ((rc = loss_checkpoint(h, tuning, lambda1, lambda2, alpha, &lo))) return rc;
            if ((rc = check_fail_flag(h))) return rc;
            loss = lo.loss;
            train_rmse = lo.train_rmse;
            test_rmse = lo.test_rmse;
            const double delta_loss = pre_loss - loss;
            decay = decay_for(delta_loss);                                                      // :389-403
            put_traj(iter, delta_loss, decay);
            if (h->opt.verbose) {
                printf("insider iter %u: train rmse = %.12g\n", iter, train_rmse);
                if (tuning == 1) printf("insider iter %u: test rmse = %.12g\n", iter, test_rmse);
                printf("total_residual\t%.12g;\nrow_reg_loss:\t%.12g;\ncol_reg_loss:\t%.12g;\nl1_reg_loss:\t%.12g.\n",
                       lo.sum_residual / 2, lo.row_reg_half, lo.col_reg_half, lo.l1_reg);
                printf("Delta loss for iter %u:%.12g\n", iter, delta_loss);
            }
            if ((pre_loss - loss) / pre_loss < global_tol) break;                               // :405-407
        }
        ++iter;
    }
    if ((rc = download_factors(h, A, C, K))) return rc;
    if ((rc = check_fail_flag(h))) return rc;
    if ((rc = read_cap_hits(h))) return rc;
    if ((rc = h->st.synchronize_sides())) return rc;   // (the side stream: the gene orders kept for the next call)
    h->st.side_done.drop();
    {
        unsigned long long bins[256];
        // (on the handle's own stream: a null-stream copy would wait for every other handle's work, insider_hip_clone)
        HIPCHECK(hipMemcpyAsync(bins, h->ws.sweep_total, sizeof(bins), hipMemcpyDeviceToHost, h->st.stream));
        HIPCHECK(hipStreamSynchronize(h->st.stream));
        for (unsigned long long v : bins) sweeps_total += v;
    }
    if (out_train_rmse) *out_train_rmse = train_rmse;
    if (out_test_rmse) *out_test_rmse = test_rmse;
    if (out_loss) *out_loss = loss;
    if (out_traj_rows) *out_traj_rows = trows;
    if (out_iters) *out_iters = (int)iter;
    profile_summary(h, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(),
                    (double)std::min<uint64_t>((uint64_t)iter + 1, (uint64_t)max_iter + 1), (double)sweeps_total);
    return INSIDER_OK;
}

int insider_hip_optimize(insider_hip_handle *h, double *const *A, double *C, int inc_continuous, int K, double lambda1,
                         double lambda2, double alpha, int tuning, double global_tol, double sub_tol, uint32_t max_iter,
                         uint64_t seed, double *out_train_rmse, double *out_test_rmse, double *out_loss, double *traj,
                         int traj_cap, int *out_traj_rows, int *out_iters)
{
    const int rc = optimize_body(h, A, C, inc_continuous, K, lambda1, lambda2, alpha, tuning, global_tol, sub_tol, max_iter,
                                 seed, out_train_rmse, out_test_rmse, out_loss, traj, traj_cap, out_traj_rows, out_iters);
    if (rc != INSIDER_OK && h && h->st.stream) {
        const std::string keep = g_err;
        reset_call_state(h, true);
        if (h->ws.failflag) (void)hipMemset(h->ws.failflag, 0, 4 * sizeof(int));
        g_err = keep;
    }
    return rc;
}

int insider_hip_optimize_oneshot_ex(const double *X, int64_t n, int64_t p, double *const *A, double *C,
                                    const int32_t *levels, int c, const int32_t *n_levels, const double *ctns, int m,
                                    const uint8_t *M_train, const uint8_t *M_test, int inc_continuous, int K,
                                    double lambda1, double lambda2, double alpha, int tuning, double global_tol,
                                    double sub_tol, uint32_t max_iter, uint64_t seed, int device, double *out_train_rmse,
                                    double *out_test_rmse, double *out_loss)
{
    if (inc_continuous != 0 && inc_continuous != 1)   // src/optimize.cpp:270-272
        return fail(INSIDER_ERR_ARG, "The value of prarameter inc_continuous can only be 0 or 1.");
    if (inc_continuous == 1 && (!ctns || m < 1))
        return fail(INSIDER_ERR_ARG, "inc_continuous = 1 needs ctns_confounder (n x m, m >= 1)");
    insider_hip_handle *h = nullptr;
    // the reference ignores ctns_confounder when inc_continuous = 0 (src/optimize.cpp:276-291): so does the upload
    int rc = insider_hip_create_ex(X, n, p, levels, c, n_levels, inc_continuous ? ctns : nullptr, inc_continuous ? m : 0,
                                   M_train, M_test, device, &h);
    if (rc) return rc;
    rc = insider_hip_optimize(h, A, C, inc_continuous, K, lambda1, lambda2, alpha, tuning, global_tol, sub_tol, max_iter,
                              seed, out_train_rmse, out_test_rmse, out_loss, nullptr, 0, nullptr, nullptr);
    const std::string keep = g_err;
    insider_hip_destroy(h);
    g_err = keep;
    return rc;
}

int insider_hip_optimize_oneshot(const double *X, int64_t n, int64_t p, double *const *A, double *C,
                                 const int32_t *levels, int c, const int32_t *n_levels, const uint8_t *M_train,
                                 const uint8_t *M_test, int inc_continuous, int K, double lambda1, double lambda2,
                                 double alpha, int tuning, double global_tol, double sub_tol, uint32_t max_iter,
                                 uint64_t seed, double *out_train_rmse, double *out_test_rmse, double *out_loss)
{
    if (inc_continuous == 1)
        return fail(INSIDER_ERR_ARG, "continuous covariates need insider_hip_optimize_oneshot_ex (ctns_confounder)");
    return insider_hip_optimize_oneshot_ex(X, n, p, A, C, levels, c, n_levels, nullptr, 0, M_train, M_test, inc_continuous,
                                           K, lambda1, lambda2, alpha, tuning, global_tol, sub_tol, max_iter, seed, 0,
                                           out_train_rmse, out_test_rmse, out_loss);
}

// One row update of one covariate, the reference's optimize_row() as optimize() calls it (src/optimize.cpp:339 with
// :139-198): the residual is X minus the contributions of every OTHER covariate (their A_i as passed), A[cov] is
// replaced by the per-level ridge solutions.  lambda = 0 on an interaction covariate with the other factors zero is
// fit_interaction()'s arithmetic (src/fit_interaction.cpp:10-90).  cov >= c addresses continuous column cov - c
// (optimize_continuous_v2, :76-137).
int insider_hip_optimize_row(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int cov,
                             double lambda, int tuning)
{
    int rc = check_factor_args(h, A, C, inc_continuous, tuning);
    if (rc) return rc;
    if (cov < 0 || cov >= h->ds->c + (inc_continuous ? h->ds->m : 0)) return fail(INSIDER_ERR_ARG, "covariate index out of range");
    if (!(lambda == lambda)) return fail(INSIDER_ERR_ARG, "lambda is NaN");   // any finite value, like the reference
    HIPCHECK(hipSetDevice(h->ds->device));
    if ((rc = ensure_workspace(h, K))) return rc;
    h->row_kernels = 0;
    h->w_ready = false;
    plan_call(h, tuning);
    if ((rc = upload_factors(h, A, C, K))) return rc;
    if ((rc = launch_row_prep(h))) return rc;
    if (tuning == 1 && !h->plan.merged) if ((rc = launch_row_stats(h, false))) return rc;
    if ((rc = launch_build_R(h))) return rc;
    if (h->plan.merged) if ((rc = launch_gene_v(h, 0, h->ds->SL))) return rc;
    if (cov < h->ds->c) rc = row_update(h, cov, -1, tuning, lambda);
    else rc = row_update(h, 0, cov - h->ds->c, tuning, lambda);
    if (rc) return rc;
    if ((rc = download_factors(h, A, nullptr, K))) return rc;
    return check_fail_flag(h);
}

// One column update, the reference's optimize_col() as optimize() calls it (src/optimize.cpp:376 with :200-253):
// every gene's elastic-net (alpha > 0, warm start C) or ridge (alpha == 0) regression of X on the row factor built
// from A.  `iter` selects the sweep-order stream (include/insider_perm.h).
int insider_hip_optimize_col(insider_hip_handle *h, double *const *A, double *C, int inc_continuous, int K, double lambda,
                             double alpha, int tuning, double tol, uint64_t seed, uint32_t iter)
{
    int rc = check_factor_args(h, A, C, inc_continuous, tuning);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(h->ds->device));
    if ((rc = ensure_workspace(h, K))) return rc;
    const ColCall col{alpha, lambda * alpha};
    plan_call(h, tuning, &col);
    if ((rc = upload_factors(h, A, C, K))) return rc;
    if ((rc = phase_R(h))) return rc;
    if (alpha != 0.0) {
        if ((rc = ensure_order_table(h, seed, iter, K, h->opt.max_sweeps, h->opt.order_mode, nullptr, 0))) return rc;
        h->ws.order = h->ws.order_buf[0];
    }
    if (tuning == 1) if ((rc = launch_col_stats(h, false))) return rc;
    HIPCHECK(hipMemsetAsync(h->ws.failflag + 2, 0, 2 * sizeof(int), h->st.stream));
    if ((rc = launch_col_solve(h, tuning, true, lambda, alpha, tol, 0, false))) return rc;
    if ((rc = download_factors(h, nullptr, C, K))) return rc;
    if ((rc = read_cap_hits(h))) return rc;
    return check_fail_flag(h);
}

// Device part shared by the two strong_coordinate_descent entries: dG / dq / dw hold nprob problems on the current device.
// They run on the column update's kernels (cd_solver, launch_cd; default options): k_pack_cols writes a chunk of problems in
// the layout of the column statistics, one record per problem, and one solve launch per chunk — a single pass, no launch order,
// no evaluation — leaves the solutions in rows of pitch KP.  A record is much larger than K x K at small K (256 doubles at
// K = 1), so a chunk holds CD_BATCH_DOUBLES of records at most; the problems are independent and the order table does not
// depend on the problem index, so the chunking changes no result.
constexpr int64_t CD_BATCH_DOUBLES = int64_t(1) << 26;
static int strong_cd_device(const double *dG, const double *dq, const double *dw, int K, int64_t nprob,
                            double lambda, double alpha, double tol, uint64_t seed, uint32_t iter, int order_mode,
                            int max_sweeps, double *beta_out, int32_t *sweeps_out)
{
    const int KP = 16 * ((K + 16) / 16), NB = KP / 16, stat_len = NB * (NB + 1) / 2 * 256;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nprob, CD_BATCH_DOUBLES / stat_len));
    const ColSolver cs = cd_solver(K, lambda * alpha, 0);
    const int ms = max_sweeps < 1 ? 1 : max_sweeps;
    const int rows = std::min<int64_t>(ms, INSIDER_PERM_PERIOD);   // one period of the order sequence (include/insider_perm.h)
    DevBuf<double> stat, Qfull, C, RtR;
    DevBuf<int> sw;
    DevBuf<uint8_t> order;
    DevBuf<unsigned long long> cb;
    int rc;
    if ((rc = stat.alloc((size_t)chunk * stat_len)) || (rc = Qfull.alloc((size_t)chunk * KP)) || (rc = C.alloc((size_t)chunk * KP)) ||
        (rc = RtR.alloc((size_t)KP * KP)) || (rc = sw.alloc((size_t)chunk)) || (rc = cb.alloc(2)) ||
        (rc = order.alloc((size_t)(rows + 4) * ORDER_ROW)))   // + the look-ahead row
        return rc;
    HIPCHECK(hipMemset(RtR, 0, (size_t)KP * KP * sizeof(double)));   // (every problem has its record: R'R is not read, but valid)
    unsigned long long code[2] = {0, 0};
    if (cs == CS_CD_REG && reg_pairs(reg_kmax(K)))
        if ((rc = probe_code_base(K, cb, nullptr, code))) return rc;
    if ((rc = launch_order_table(seed, iter, K, rows, order_mode, order_wide_rows(K, cs), code[0], code[1], order, nullptr))) return rc;
    ColArgs a{};
    a.stat = stat;
    a.stat_len = stat_len;
    a.K = K;
    a.KP = KP;
    a.RtR = RtR;
    a.Qfull = Qfull;
    a.C = C;
    a.mode = COL_CD;
    a.cd = cd_params(lambda, alpha, tol, ms, order);
    a.sweeps = sw;
    a.hsave = a.isave = C;   // read by a resumed pass only (none here)
    Stopwatch watch;
    float total = 0.0f;
    for (int64_t b0 = 0; b0 < nprob; b0 += chunk) {
        const int n = (int)std::min<int64_t>(chunk, nprob - b0);
        hipLaunchKernelGGL(k_pack_cols, dim3(cdiv((int64_t)n * stat_len, 256)), dim3(256), 0, 0, dG + (size_t)b0 * K * K,
                           dq + (size_t)b0 * K, dw + (size_t)b0 * K, K, KP, n, stat_len, stat, Qfull, C);
        KCHECK();
        a.p = n;
        float msf = 0.0f;
        if ((rc = watch.start(0)) || (rc = launch_cd(cs, a, 0)) || (rc = watch.stop_ms(0, &msf))) return rc;
        total += msf;
        HIPCHECK(hipMemcpy2D(beta_out + (size_t)b0 * K, (size_t)K * sizeof(double), C, (size_t)KP * sizeof(double),
                             (size_t)K * sizeof(double), (size_t)n, hipMemcpyDeviceToHost));
        if (sweeps_out) HIPCHECK(hipMemcpy(sweeps_out + b0, sw, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    }
    g_last_cd_ms = total;
    g_last_cd_solver = cs;
    return INSIDER_OK;
}

static int cd_common_checks(int K, int64_t nprob, int device)
{
    if (K < 1 || K > 64 || nprob < 0) return fail(INSIDER_ERR_ARG, "K must be in 1..64");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(INSIDER_ERR_NO_DEVICE, "no HIP device visible: libinsider_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(INSIDER_ERR_ARG, "bad device ordinal");
    return INSIDER_OK;
}

int insider_hip_strong_cd(const double *XtX, const double *Xty, const double *wstart, int K, int64_t nprob, double lambda,
                          double alpha, double tol, uint64_t seed, uint32_t iter, int order_mode,
                          int max_sweeps, int device, double *beta_out, int32_t *sweeps_out)
{
    if (!XtX || !Xty || !wstart || !beta_out) return fail(INSIDER_ERR_ARG, "null argument");
    int rc = cd_common_checks(K, nprob, device);
    if (rc) return rc;
    if (nprob == 0) return INSIDER_OK;
    HIPCHECK(hipSetDevice(device));
    DevBuf<double> dG, dq, dw;
    if ((rc = dG.alloc((size_t)nprob * K * K)) || (rc = dq.alloc((size_t)nprob * K)) || (rc = dw.alloc((size_t)nprob * K))) return rc;
    HIPCHECK(hipMemcpy(dG, XtX, (size_t)nprob * K * K * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dq, Xty, (size_t)nprob * K * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dw, wstart, (size_t)nprob * K * sizeof(double), hipMemcpyHostToDevice));
    return strong_cd_device(dG, dq, dw, K, nprob, lambda, alpha, tol, seed, iter, order_mode, max_sweeps, beta_out,
                            sweeps_out);
}

int insider_hip_strong_cd_xy(const double *X, const double *y, int64_t m, int K, const double *wstart, double lambda,
                             double alpha, const double *XtX, const double *Xty, double tol, uint64_t seed, uint32_t iter,
                             int order_mode, int max_sweeps, int device, double *beta_out, int32_t *sweeps_out)
{
    if (!wstart || !beta_out) return fail(INSIDER_ERR_ARG, "null argument");
    if ((!XtX || !Xty) && (!X || !y)) return fail(INSIDER_ERR_ARG, "pass (X, y), or XtX and Xty, or all four");
    if (m < 0) return fail(INSIDER_ERR_ARG, "m must be >= 0");
    int rc = cd_common_checks(K, 1, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    DevBuf<double> dG, dq, dw;
    if ((rc = dG.alloc((size_t)K * K)) || (rc = dq.alloc((size_t)K)) || (rc = dw.alloc((size_t)K))) return rc;
    if (!XtX || !Xty) {   // X'X and X'y on the device from the design matrix and outcome (src/optimize.cpp:219-222,234-235)
        DevBuf<double> dX, dy;
        if ((rc = dX.alloc((size_t)m * K)) || (rc = dy.alloc((size_t)m))) return rc;
        HIPCHECK(hipMemcpy(dX, X, (size_t)m * K * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dy, y, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_xtx_xty, dim3(K, K + 1), dim3(64), 0, 0, (const double *)dX, (const double *)dy, m, K, dG, dq);
        KCHECK();
    }
    if (XtX) HIPCHECK(hipMemcpy(dG, XtX, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice));
    if (Xty) HIPCHECK(hipMemcpy(dq, Xty, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dw, wstart, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    return strong_cd_device(dG, dq, dw, K, 1, lambda, alpha, tol, seed, iter, order_mode, max_sweeps, beta_out,
                            sweeps_out);
}

// solve(A, b, likely_sympd) on a caller's systems, by the stand-alone kernel (form 0: k_solve_batch, pitch K) or by the fit's own
// level solve (form 1: every system packed as the level equation record [KP x KP | KP] with a count of 1, k_level_solve<NB>
// launched as row_update() launches it).  lambda is added to the diagonal on the device in both forms.
int insider_hip_solve_sympd_form(const double *A, const double *b, int K, int64_t nsys, double lambda, int form, int device,
                                 double *x, int32_t *route)
{
    if (!A || !b || !x) return fail(INSIDER_ERR_ARG, "null argument");
    if (form != 0 && form != 1) return fail(INSIDER_ERR_ARG, "form must be 0 (batch) or 1 (level)");
    if (!(lambda == lambda)) return fail(INSIDER_ERR_ARG, "lambda is NaN");
    int rc = cd_common_checks(K, nsys, device);
    if (rc) return rc;
    if (form == 1 && K > INSIDER_MAX_K) return fail(INSIDER_ERR_UNSUPPORTED, "form 1 (the level solve) needs K in 1..63");
    if (nsys == 0) return INSIDER_OK;
    HIPCHECK(hipSetDevice(device));
    DevBuf<double> dA, db, dx;
    DevBuf<int> dr;
    std::vector<int> hr(nsys);
    if (form == 0) {
        if ((rc = dA.alloc((size_t)nsys * K * K)) || (rc = db.alloc((size_t)nsys * K)) || (rc = dx.alloc((size_t)nsys * K)) ||
            (rc = dr.alloc((size_t)nsys)))
            return rc;
        HIPCHECK(hipMemcpy(dA, A, (size_t)nsys * K * K * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(db, b, (size_t)nsys * K * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_solve_batch, dim3((unsigned)nsys), dim3(64), 0, 0, (const double *)dA, (const double *)db, K, nsys,
                           lambda, dx, dr);
        KCHECK();
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(x, dx, (size_t)nsys * K * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        const int NB = (K + 1 + 15) / 16, KP = 16 * NB;
        const size_t len = (size_t)KP * KP + KP;
        std::vector<double> rec((size_t)nsys * len, 0.0);   // element (r, c) at r * KP + c, b behind it; zeros outside K
        for (int64_t s = 0; s < nsys; ++s) {
            double *q = rec.data() + (size_t)s * len;
            const double *As = A + (size_t)s * K * K;
            for (int r = 0; r < K; ++r) {
                for (int c = 0; c < K; ++c) q[(size_t)r * KP + c] = As[r + (size_t)c * K];
                q[(size_t)KP * KP + r] = b[(size_t)s * K + r];
            }
        }
        DevBuf<int> dcnt, dfail;
        if ((rc = dA.alloc((size_t)nsys * len)) || (rc = dx.alloc((size_t)nsys * KP)) || (rc = dr.alloc((size_t)nsys)) ||
            (rc = dcnt.alloc((size_t)nsys)) || (rc = dfail.alloc(1)))
            return rc;
        const std::vector<int> ones(nsys, 1);
        HIPCHECK(hipMemcpy(dA, rec.data(), (size_t)nsys * len * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dcnt, ones.data(), (size_t)nsys * sizeof(int), hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(dx, 0, (size_t)nsys * KP * sizeof(double)));
        HIPCHECK(hipMemset(dfail, 0, sizeof(int)));
        NB_DISPATCH(NB, {
            (void)WPB_;
            hipLaunchKernelGGL((k_level_solve<NB_>), dim3((unsigned)nsys), dim3(64), 0, 0, (const double *)dA, (const int *)dcnt,
                               (int)nsys, K, lambda, dx, dfail, dr);
        });
        KCHECK();
        HIPCHECK(hipDeviceSynchronize());
        std::vector<double> hx((size_t)nsys * KP);
        HIPCHECK(hipMemcpy(hx.data(), dx, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t s = 0; s < nsys; ++s)
            for (int r = 0; r < K; ++r) x[(size_t)s * K + r] = hx[(size_t)s * KP + r];
    }
    HIPCHECK(hipMemcpy(hr.data(), dr, (size_t)nsys * sizeof(int), hipMemcpyDeviceToHost));
    bool singular = false;
    for (int64_t i = 0; i < nsys; ++i) {
        if (route) route[i] = hr[i];
        singular = singular || hr[i] < 0;
    }
    if (singular) return fail(INSIDER_ERR_SOLVE, "a system is singular to working precision");
    return INSIDER_OK;
}

int insider_hip_solve_sympd(const double *A, const double *b, int K, int64_t nsys, int device, double *x, int32_t *route)
{
    return insider_hip_solve_sympd_form(A, b, K, nsys, 0.0, 0, device, x, route);
}

// ---- neighbours (insider_neighbors.hpp) ------------------------------------------------------------------------------------
static bool all_finite(const double *v, size_t count)
{
    for (size_t e = 0; e < count; ++e)
        if (!std::isfinite(v[e])) return false;
    return true;
}

int insider_hip_neighbors(const double *Q, int64_t nq, const double *B, int64_t nb, int K, int metric, int k,
                          int64_t self_offset, int device, int32_t *idx_out, double *score_out)
{
    if (!Q || !B || !idx_out || !score_out) return fail(INSIDER_ERR_ARG, "null argument");
    if (K < 1 || K > INSIDER_MAX_K) return fail(INSIDER_ERR_ARG, "K must be in 1..63");
    if (k < 1 || k > NN_MAX_TOPK) return fail(INSIDER_ERR_ARG, "k must be in 1..64");
    if (nq < 0) return fail(INSIDER_ERR_ARG, "nq must be >= 0");
    if (nb < 1 || nb > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "nb must be in 1..2^31-1");
    if (metric != 0 && metric != 1) return fail(INSIDER_ERR_ARG, "metric must be 0 (cosine) or 1 (dot)");
    if (self_offset < -1) return fail(INSIDER_ERR_ARG, "self_offset must be >= -1");
    if (self_offset >= 0 && (nq > nb || self_offset > nb - nq))
        return fail(INSIDER_ERR_ARG, "self_offset + nq must be <= nb");
    if (nq > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_UNSUPPORTED, "nq must be < 2^31");
    // the queries are a window of the base (the self call): one check, one upload
    const bool window = self_offset >= 0 && Q == B + (size_t)self_offset * K;
    if (!all_finite(B, (size_t)nb * K) || (!window && !all_finite(Q, (size_t)nq * K)))
        return fail(INSIDER_ERR_ARG, "Q and B must be finite");
    int rc = cd_common_checks(K, nq, device);
    if (rc) return rc;
    if (nq == 0) return INSIDER_OK;
    HIPCHECK(hipSetDevice(device));
    const int K4 = (K + 3) & ~3, KS = (K4 + 15) / 16;
    const int NT = K4 <= 32 ? 4 : 2;
    const int64_t nbpad = round_up(nb, 64), nqpad = round_up(nq, 16);
    auto lds = [&](int nw) { return (size_t)(NT * 16 * K4 + nw * 16 * (k + NN_CAP)) * 8 + (size_t)(NT * 16 + nw * 16 * (k + NN_CAP)) * 4; };
    const int NW = lds(4) <= 64 * 1024 ? 4 : 2;
    DevBuf<double> dB, dQ, dBp, dQp, dscore;
    DevBuf<int> dba, dqa;
    DevBuf<int32_t> didx;
    if ((rc = dB.alloc((size_t)nb * K)) || (rc = dBp.alloc((size_t)nbpad * K4)) || (rc = dQp.alloc((size_t)nqpad * K4)) ||
        (rc = dba.alloc((size_t)nbpad)) || (rc = dqa.alloc((size_t)nqpad)) || (rc = dscore.alloc((size_t)nq * k)) ||
        (rc = didx.alloc((size_t)nq * k)))
        return rc;
    HIPCHECK(hipMemcpy(dB, B, (size_t)nb * K * sizeof(double), hipMemcpyHostToDevice));
    const double *qsrc = dB.get() + (size_t)(window ? self_offset : 0) * K;
    if (!window) {
        if ((rc = dQ.alloc((size_t)nq * K))) return rc;
        HIPCHECK(hipMemcpy(dQ, Q, (size_t)nq * K * sizeof(double), hipMemcpyHostToDevice));
        qsrc = dQ;
    }
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    hipLaunchKernelGGL(k_nn_prep, dim3(cdiv(nbpad, 256)), dim3(256), 0, 0, (const double *)dB, nb, nbpad, K, K4, metric, dBp.get(),
                       dba.get());
    KCHECK();
    hipLaunchKernelGGL(k_nn_prep, dim3(cdiv(nqpad, 256)), dim3(256), 0, 0, qsrc, nq, nqpad, K, K4, metric, dQp.get(), dqa.get());
    KCHECK();
    const dim3 grid(cdiv(nq, 16 * NW)), block(64 * NW);
    KT_DISPATCH(KS, hipLaunchKernelGGL((k_nn_topk<KT_>), grid, block, lds(NW), 0, (const double *)dQp, (const int *)dqa, nq,
                                       (const double *)dBp, (const int *)dba, nbpad, K4, NT, k, self_offset, didx.get(),
                                       dscore.get()));
    KCHECK();
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_neighbors_ms = ms;
    HIPCHECK(hipMemcpy(idx_out, didx, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(score_out, dscore, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

double insider_hip_last_neighbors_ms(void) { return g_last_neighbors_ms; }

// ---- co-expression: the deep product with fused top-k (insider_coexpr.hpp) -------------------------------------------------
// the launch of k_cx_topk over the query groups that meet the window, on stream st
static int launch_cx_topk(const double *P, const int *alive, int64_t npad, int64_t Dpad, int k, int64_t first, int64_t count,
                          int32_t *idx, double *score, hipStream_t st)
{
    const size_t lds = cx_topk_lds(k);
    // above 64 KB of dynamic LDS (k > 10 or so) the launch needs the function attribute
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cx_topk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t groups = (first + count - 1) / CX_QB - first / CX_QB + 1;
    hipLaunchKernelGGL(k_cx_topk, dim3((unsigned)groups), dim3(64 * CX_WAVES), lds, st, P, alive, npad, Dpad, k, first, count, idx,
                       score);
    KCHECK();
    return INSIDER_OK;
}

int insider_hip_gram_topk(const double *V, int64_t depth, int64_t N, int metric, int k, int64_t first, int64_t count,
                          int device, int32_t *idx_out, double *score_out)
{
    if (!V || !idx_out || !score_out) return fail(INSIDER_ERR_ARG, "null argument");
    if (depth < 1) return fail(INSIDER_ERR_ARG, "depth must be >= 1");
    if (N < 1 || N > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "N must be in 1..2^31-1");
    if (k < 1 || k > NN_MAX_TOPK) return fail(INSIDER_ERR_ARG, "k must be in 1..64");
    if (metric < 0 || metric > 2) return fail(INSIDER_ERR_ARG, "metric must be 0 (correlation), 1 (cosine) or 2 (dot)");
    if (first < 0 || count < 0 || first > N || count > N - first)
        return fail(INSIDER_ERR_ARG, "the window must satisfy 0 <= first, 0 <= count, first + count <= N");
    if (depth > (int64_t)(std::numeric_limits<size_t>::max() / sizeof(double)) / N)
        return fail(INSIDER_ERR_ARG, "depth x N does not fit the address space");
    if (!all_finite(V, (size_t)N * depth)) return fail(INSIDER_ERR_ARG, "V must be finite");
    int rc = cd_common_checks(1, count, device);
    if (rc) return rc;
    if (count == 0) return INSIDER_OK;
    HIPCHECK(hipSetDevice(device));
    const int64_t npad = round_up(N, CX_PAD), Dpad = round_up(depth, CX_DC);
    DevBuf<double> dV, dP, dscore;
    DevBuf<int> dalive;
    DevBuf<int32_t> didx;
    if ((rc = dV.alloc((size_t)N * depth)) || (rc = dP.alloc((size_t)npad * Dpad)) || (rc = dalive.alloc((size_t)npad)) ||
        (rc = dscore.alloc((size_t)count * k)) || (rc = didx.alloc((size_t)count * k)))
        return rc;
    HIPCHECK(hipMemcpy(dV, V, (size_t)N * depth * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(dP, 0, (size_t)npad * Dpad * sizeof(double)));
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    hipLaunchKernelGGL(k_cx_prep, dim3(cdiv(npad, 64)), dim3(64), 0, 0, (const double *)dV, depth, N, npad, Dpad, metric, dP.get(),
                       dalive.get());
    KCHECK();
    if ((rc = launch_cx_topk(dP, dalive, npad, Dpad, k, first, count, didx, dscore, 0))) return rc;
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_gram_topk_ms = ms;
    HIPCHECK(hipMemcpy(idx_out, didx, (size_t)count * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(score_out, dscore, (size_t)count * k * sizeof(double), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

double insider_hip_last_gram_topk_ms(void) { return g_last_gram_topk_ms; }

// the launch of k_cx_topk_pc (insider_coexpr_pc.hpp) over the query groups that meet the window, on stream st
static int launch_cx_topk_pc(const double *P, const int *alive, int64_t npad, int64_t Dpad, int64_t depth, int64_t min_overlap,
                             int k, int64_t first, int64_t count, int32_t *idx, double *score, int32_t *overlap, hipStream_t st)
{
    const size_t lds = cx_topk_pc_lds(k);
    // above 64 KB of dynamic LDS (k > 7) the launch needs the function attribute
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cx_topk_pc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t groups = (first + count - 1) / CX_QB - first / CX_QB + 1;
    const double vfloor = 16.0 * (double)(depth + 8) * 0x1p-52;
    hipLaunchKernelGGL(k_cx_topk_pc, dim3((unsigned)groups), dim3(64 * CX_WAVES), lds, st, P, alive, npad, Dpad, min_overlap, vfloor,
                       k, first, count, idx, score, overlap);
    KCHECK();
    return INSIDER_OK;
}

int insider_hip_gram_topk_pairwise(const double *V, int64_t depth, int64_t N, int64_t min_overlap, int k, int64_t first,
                                   int64_t count, int device, int32_t *idx_out, double *score_out, int32_t *overlap_out)
{
    if (!V || !idx_out || !score_out || !overlap_out) return fail(INSIDER_ERR_ARG, "null argument");
    if (depth < 1 || depth > (int64_t)std::numeric_limits<int32_t>::max())
        return fail(INSIDER_ERR_ARG, "depth must be in 1..2^31-1");
    if (N < 1 || N > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "N must be in 1..2^31-1");
    if (min_overlap < 3) return fail(INSIDER_ERR_ARG, "min_overlap must be >= 3");
    if (k < 1 || k > NN_MAX_TOPK) return fail(INSIDER_ERR_ARG, "k must be in 1..64");
    if (first < 0 || count < 0 || first > N || count > N - first)
        return fail(INSIDER_ERR_ARG, "the window must satisfy 0 <= first, 0 <= count, first + count <= N");
    if (depth > (int64_t)(std::numeric_limits<size_t>::max() / sizeof(double)) / N)
        return fail(INSIDER_ERR_ARG, "depth x N does not fit the address space");
    for (size_t e = 0, ne = (size_t)N * depth; e < ne; ++e)
        if (std::isinf(V[e])) return fail(INSIDER_ERR_ARG, "V must be finite or NaN (a missing entry)");
    int rc = cd_common_checks(1, count, device);
    if (rc) return rc;
    if (count == 0) return INSIDER_OK;
    HIPCHECK(hipSetDevice(device));
    const int64_t npad = round_up(N, CX_PAD), Dpad = round_up(depth, CX_DC);
    DevBuf<double> dV, dP, dscore;
    DevBuf<int> dalive;
    DevBuf<int32_t> didx, dover;
    if ((rc = dV.alloc((size_t)N * depth)) || (rc = dP.alloc((size_t)npad * Dpad)) || (rc = dalive.alloc((size_t)npad)) ||
        (rc = dscore.alloc((size_t)count * k)) || (rc = didx.alloc((size_t)count * k)) || (rc = dover.alloc((size_t)count * k)))
        return rc;
    HIPCHECK(hipMemcpy(dV, V, (size_t)N * depth * sizeof(double), hipMemcpyHostToDevice));
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    hipLaunchKernelGGL(k_cx_std_pc, dim3(cdiv(npad, 64)), dim3(64), 0, 0, (const double *)dV, depth, N, npad, Dpad, dP.get(),
                       dalive.get());   // (writes every double of P)
    KCHECK();
    if ((rc = launch_cx_topk_pc(dP, dalive, npad, Dpad, depth, min_overlap, k, first, count, didx, dscore, dover, 0))) return rc;
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_gram_topk_ms = ms;
    HIPCHECK(hipMemcpy(idx_out, didx, (size_t)count * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(score_out, dscore, (size_t)count * k * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(overlap_out, dover, (size_t)count * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

// ---- k-means (insider_kmeans.hpp) -----------------------------------------------------------------------------------------
int insider_hip_kmeans(const double *P, int64_t N, int D, int k, int metric, const double *init, int restarts, int max_iter,
                       uint64_t seed, int device, double *centers, int32_t *label, double *dist, int32_t *second, double *dist2,
                       int32_t *sizes, double *traj, double *final_inertia, int32_t *iters, int32_t *converged, int32_t *best)
{
    if (!P || !centers || !label || !dist || !second || !dist2 || !sizes || !traj || !final_inertia || !iters || !converged ||
        !best)
        return fail(INSIDER_ERR_ARG, "null argument");
    if (D < 1 || D > INSIDER_MAX_K) return fail(INSIDER_ERR_ARG, "D must be in 1..63");
    if (k < 1 || k > KM_MAX_K) return fail(INSIDER_ERR_ARG, "k must be in 1..4096");
    if (N < 1 || N > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "N must be in 1..2^31-1");
    if (metric != 0 && metric != 1) return fail(INSIDER_ERR_ARG, "metric must be 0 (cosine) or 1 (Euclidean)");
    if (restarts < 1 || restarts > 256) return fail(INSIDER_ERR_ARG, "restarts must be in 1..256");
    if (init && restarts != 1) return fail(INSIDER_ERR_ARG, "restarts must be 1 when init is given");
    if (max_iter < 0 || max_iter > 10000) return fail(INSIDER_ERR_ARG, "max_iter must be in 0..10000");
    if (!all_finite(P, (size_t)N * D) || (init && !all_finite(init, (size_t)k * D)))
        return fail(INSIDER_ERR_ARG, "P and init must be finite");
    // the alive points, by k_nn_prep's rule: the sum of squares in index order is not 0
    auto zero_norm = [D](const double *c) {
        double ss = 0.0;
        for (int d = 0; d < D; ++d) ss = std::fma(c[d], c[d], ss);
        return !(std::sqrt(ss) > 0.0);
    };
    std::vector<int32_t> alive_idx;
    int64_t Na = N;
    if (metric == 0) {
        Na = 0;
        if (!init) alive_idx.reserve((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            if (zero_norm(P + (size_t)i * D)) continue;
            ++Na;
            if (!init) alive_idx.push_back((int32_t)i);
        }
    }
    if (k > Na) return fail(INSIDER_ERR_ARG, "k must not exceed the number of alive points");
    if (!init && Na < 2) return fail(INSIDER_ERR_ARG, "a drawn start needs at least 2 alive points");
    if (init && metric == 0)
        for (int j = 0; j < k; ++j)
            if (zero_norm(init + (size_t)j * D)) return fail(INSIDER_ERR_ARG, "an init column has norm 0");
    std::vector<int32_t> pick;   // restart r starts from the points pick[r k ..]
    if (!init) {
        pick.resize((size_t)restarts * k);
        const uint32_t half = insider_sample_half((uint32_t)Na);
        for (int r = 0; r < restarts; ++r) {
            const uint32_t key = insider_sample_key(seed, (uint32_t)r);
            for (int j = 0; j < k; ++j) {
                const uint32_t a = insider_sample_phi(key, half, (uint32_t)Na, (uint32_t)j);
                pick[(size_t)r * k + j] = metric == 0 ? alive_idx[a] : (int32_t)a;
            }
        }
        std::vector<int32_t>().swap(alive_idx);
    }
    int rc = cd_common_checks(D, N, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    const int K4 = (D + 3) & ~3, KS = (K4 + 15) / 16;
    const int NT = std::min(K4 <= 32 ? 4 : 2, (k + 15) / 16);
    const int kpad = (int)round_up(k, 16 * NT);
    const int64_t npad = round_up(N, 16);
    const int nblk = cdiv(N, 16 * KM_NW);
    const int B = (int)std::min<int64_t>(KM_MAX_CHUNKS, (N + 1023) / 1024);   // B k <= 4 N + k
    const int64_t chunk = (N + B - 1) / B;
    const size_t lds = (size_t)(NT * 16 * K4 + NT * 16) * sizeof(double);
    const bool keep = restarts > 1;
    DevBuf<double> dX, dXp, dxx, dC, dCp, dh, ddist, ddist2, dpin, drec, bC, bdist, bdist2;
    DevBuf<int> dalive, dpch, dtable, dfirst;
    DevBuf<int32_t> dlabel, dsecond, dsize, dmember, dpick, blabel, bsecond, bsize;
    if ((rc = dX.alloc((size_t)N * D)) || (rc = dXp.alloc((size_t)npad * K4)) || (rc = dalive.alloc((size_t)npad)) ||
        (rc = dxx.alloc((size_t)std::max<int64_t>(N, k))) || (rc = dC.alloc((size_t)k * D)) || (rc = dCp.alloc((size_t)kpad * K4)) ||
        (rc = dh.alloc((size_t)kpad)) || (rc = ddist.alloc((size_t)N)) || (rc = ddist2.alloc((size_t)N)) ||
        (rc = dlabel.alloc((size_t)N)) || (rc = dsecond.alloc((size_t)N)) || (rc = dpin.alloc((size_t)nblk)) ||
        (rc = dpch.alloc((size_t)nblk)) || (rc = drec.alloc(2)) || (rc = dtable.alloc((size_t)B * k)) ||
        (rc = dfirst.alloc((size_t)k)) || (rc = dsize.alloc((size_t)k)) || (rc = dmember.alloc((size_t)N)))
        return rc;
    if (keep && ((rc = bC.alloc((size_t)k * D)) || (rc = bdist.alloc((size_t)N)) || (rc = bdist2.alloc((size_t)N)) ||
                 (rc = blabel.alloc((size_t)N)) || (rc = bsecond.alloc((size_t)N)) || (rc = bsize.alloc((size_t)k))))
        return rc;
    HIPCHECK(hipMemcpy(dX, P, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice));
    if (!init && (rc = dpick.upload(pick))) return rc;
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    hipLaunchKernelGGL(k_nn_prep, dim3(cdiv(npad, 256)), dim3(256), 0, 0, (const double *)dX, N, npad, D, K4, metric, dXp.get(),
                       dalive.get());
    KCHECK();
    hipLaunchKernelGGL(k_km_points, dim3(cdiv(N, 256)), dim3(256), 0, 0, dX.get(), N, D, metric, dxx.get());
    KCHECK();
    // one assignment against dC, its record and the clusters' sizes
    auto assign = [&]() -> int {
        hipLaunchKernelGGL(k_km_cprep, dim3(cdiv(kpad, 256)), dim3(256), 0, 0, (const double *)dC, k, kpad, D, K4, metric,
                           dCp.get(), dh.get());
        KCHECK();
        KT_DISPATCH(KS, hipLaunchKernelGGL((k_km_assign<KT_>), dim3(nblk), dim3(64 * KM_NW), lds, 0, (const double *)dXp,
                                           (const int *)dalive, N, (const double *)dCp, (const double *)dh, k, kpad, K4, NT, metric,
                                           (const double *)dxx, dlabel.get(), dsecond.get(), ddist.get(), ddist2.get(),
                                           dpin.get(), dpch.get()));
        KCHECK();
        hipLaunchKernelGGL(k_km_reduce, dim3(1), dim3(256), 0, 0, (const double *)dpin, (const int *)dpch, nblk, drec.get());
        KCHECK();
        hipLaunchKernelGGL(k_km_hist, dim3(B), dim3(64), (size_t)k * sizeof(int), 0, (const int32_t *)dlabel, N, chunk, k,
                           dtable.get());
        KCHECK();
        hipLaunchKernelGGL(k_km_colscan, dim3(cdiv(k, 256)), dim3(256), 0, 0, dtable.get(), B, k, dsize.get());
        KCHECK();
        return INSIDER_OK;
    };
    std::vector<double> tr((size_t)max_iter + 1), best_tr;
    std::vector<double> fin((size_t)restarts);
    std::vector<int32_t> its((size_t)restarts), conv((size_t)restarts);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int best_r = 0;
    for (int r = 0; r < restarts; ++r) {
        if (init) {
            HIPCHECK(hipMemcpy(dC, init, (size_t)k * D * sizeof(double), hipMemcpyHostToDevice));
            if (metric == 0) {   // the columns normalised as the points are (|c|^2 goes to a corner nobody reads again)
                hipLaunchKernelGGL(k_km_points, dim3(cdiv(k, 256)), dim3(256), 0, 0, dC.get(), (int64_t)k, D, metric, dh.get());
                KCHECK();
            }
        } else {
            hipLaunchKernelGGL(k_km_gather, dim3(cdiv((int64_t)k * D, 256)), dim3(256), 0, 0, (const double *)dX,
                               (const int32_t *)dpick.get() + (size_t)r * k, k, D, dC.get());
            KCHECK();
        }
        HIPCHECK(hipMemsetAsync(dlabel, 0xFF, (size_t)N * sizeof(int32_t), 0));
        std::fill(tr.begin(), tr.end(), nan);
        double rec[2];
        if ((rc = assign())) return rc;
        HIPCHECK(hipMemcpy(rec, drec, sizeof(rec), hipMemcpyDeviceToHost));
        tr[0] = rec[0];
        int t = 0, cv = 0;
        while (t < max_iter) {
            hipLaunchKernelGGL(k_km_scan, dim3(1), dim3(256), 0, 0, (const int32_t *)dsize, k, dfirst.get());
            KCHECK();
            hipLaunchKernelGGL(k_km_scatter, dim3(B), dim3(64), (size_t)k * sizeof(int), 0, (const int32_t *)dlabel, N, chunk, k,
                               (const int *)dtable, (const int *)dfirst, dmember.get());
            KCHECK();
            hipLaunchKernelGGL(k_km_sum, dim3(k), dim3(256), 0, 0, (const double *)dX, (const int32_t *)dmember,
                               (const int *)dfirst, (const int32_t *)dsize, D, metric, dC.get());
            KCHECK();
            if ((rc = assign())) return rc;
            HIPCHECK(hipMemcpy(rec, drec, sizeof(rec), hipMemcpyDeviceToHost));   // the iteration's record: all the host reads
            tr[++t] = rec[0];
            if (rec[1] == 0.0) {
                cv = 1;
                break;
            }
        }
        fin[r] = tr[t];
        its[r] = t;
        conv[r] = cv;
        if (r == 0 || fin[r] < fin[best_r]) {
            best_r = r;
            best_tr = tr;
            if (keep) {
                HIPCHECK(hipMemcpyAsync(bC, dC, (size_t)k * D * sizeof(double), hipMemcpyDeviceToDevice, 0));
                HIPCHECK(hipMemcpyAsync(bdist, ddist, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0));
                HIPCHECK(hipMemcpyAsync(bdist2, ddist2, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0));
                HIPCHECK(hipMemcpyAsync(blabel, dlabel, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, 0));
                HIPCHECK(hipMemcpyAsync(bsecond, dsecond, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, 0));
                HIPCHECK(hipMemcpyAsync(bsize, dsize, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToDevice, 0));
            }
        }
    }
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_kmeans_ms = ms;
    // every result is staged on the host first: a failed download leaves the caller's arrays as they were
    std::vector<double> hC((size_t)k * D), hdist((size_t)N), hdist2((size_t)N);
    std::vector<int32_t> hlabel((size_t)N), hsecond((size_t)N), hsize((size_t)k);
    HIPCHECK(hipMemcpy(hC.data(), keep ? bC : dC, hC.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hdist.data(), keep ? bdist : ddist, hdist.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hdist2.data(), keep ? bdist2 : ddist2, hdist2.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hlabel.data(), keep ? blabel : dlabel, hlabel.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hsecond.data(), keep ? bsecond : dsecond, hsecond.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hsize.data(), keep ? bsize : dsize, hsize.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::copy(hC.begin(), hC.end(), centers);
    std::copy(hdist.begin(), hdist.end(), dist);
    std::copy(hdist2.begin(), hdist2.end(), dist2);
    std::copy(hlabel.begin(), hlabel.end(), label);
    std::copy(hsecond.begin(), hsecond.end(), second);
    std::copy(hsize.begin(), hsize.end(), sizes);
    std::copy(best_tr.begin(), best_tr.end(), traj);
    std::copy(fin.begin(), fin.end(), final_inertia);
    std::copy(its.begin(), its.end(), iters);
    std::copy(conv.begin(), conv.end(), converged);
    *best = best_r;
    return INSIDER_OK;
}

double insider_hip_last_kmeans_ms(void) { return g_last_kmeans_ms; }

// ---- agglomerative clustering (insider_hclust.hpp) ------------------------------------------------------------------------
namespace {

// The records of a finished run (emission order: a, b ids of the run, d, size) brought into the order and the numbering of the
// result (include/insider_hip.h): heights made monotone along the tree, a stable sort by height, row r creates id N + r.
void hc_finish(int64_t N, const std::vector<int32_t> &pt_alive, int metric, const std::vector<int32_t> &ra,
               const std::vector<int32_t> &rb, const std::vector<double> &rd, const std::vector<int32_t> &rn, int32_t *merge,
               double *height, int32_t *size, int32_t *order)
{
    const int64_t R = (int64_t)ra.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> h((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        double v = metric == 1 ? std::sqrt(2.0 * rd[r]) : rd[r];
        if (ra[r] >= N) v = std::max(v, h[ra[r] - N]);   // (a child was emitted before its parent)
        if (rb[r] >= N) v = std::max(v, h[rb[r] - N]);
        h[r] = v;
    }
    std::vector<int64_t> perm((size_t)R), row((size_t)R);
    for (int64_t r = 0; r < R; ++r) perm[r] = r;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return h[x] < h[y]; });
    for (int64_t r = 0; r < R; ++r) row[perm[r]] = r;
    for (int64_t r = 0; r < N - 1; ++r) {
        if (r < R) {
            const int64_t e = perm[r];
            const int64_t x = ra[e] < N ? ra[e] : N + row[ra[e] - N], y = rb[e] < N ? rb[e] : N + row[rb[e] - N];
            merge[2 * r] = (int32_t)std::min(x, y);
            merge[2 * r + 1] = (int32_t)std::max(x, y);
            height[r] = h[e];
            size[r] = rn[e];
        } else {
            merge[2 * r] = merge[2 * r + 1] = -1;
            height[r] = nan;
            size[r] = -1;
        }
    }
    // leaf order: depth first from the last row, the lower id first; a lone alive point is its own tree; dead points last
    int64_t o = 0;
    std::vector<int64_t> stack;
    if (R > 0) stack.push_back(N + R - 1);
    else
        for (int64_t i = 0; i < N; ++i)
            if (pt_alive[i]) stack.push_back(i);
    while (!stack.empty()) {
        const int64_t c = stack.back();
        stack.pop_back();
        if (c < N) {
            order[o++] = (int32_t)c;
        } else {
            stack.push_back(merge[2 * (c - N) + 1]);
            stack.push_back(merge[2 * (c - N)]);
        }
    }
    for (int64_t i = 0; i < N; ++i)
        if (!pt_alive[i]) order[o++] = (int32_t)i;
}

}  // namespace

int insider_hip_hclust(const double *P, int64_t N, int D, int metric, int linkage, int max_rounds, int device, int32_t *merge,
                       double *height, int32_t *size, int32_t *order, int32_t *rounds, int64_t *queries, int32_t *alive)
{
    if (!P || !merge || !height || !size || !order || !rounds || !queries || !alive)
        return fail(INSIDER_ERR_ARG, "null argument");
    if (D < 1 || D > HC_MAX_D) return fail(INSIDER_ERR_ARG, "D must be in 1..63");
    if (N < 1 || 2 * N - 1 > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "N must be in 1..2^30");
    if (!((metric == 0 && linkage == 0) || (metric == 1 && linkage == 1)))
        return fail(INSIDER_ERR_ARG, "metric / linkage must be 0 / 0 (cosine, average) or 1 / 1 (Euclidean, Ward)");
    if (max_rounds < 1) return fail(INSIDER_ERR_ARG, "max_rounds must be at least 1");
    if (!all_finite(P, (size_t)N * D)) return fail(INSIDER_ERR_ARG, "P must be finite");
    int rc = cd_common_checks(D, N, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    const int K4 = (D + 3) & ~3, KS = (K4 + 15) / 16;
    const int NT = K4 <= 32 ? 4 : 2;
    const int64_t M = 2 * N - 1, npad = round_up(N, 16 * NT);
    const int64_t nbmax = cdiv(M, 256);
    const size_t lds = (size_t)(NT * 16 * K4 + 2 * NT * 16) * sizeof(double) + (size_t)NT * 16 * sizeof(int);
    DevBuf<double> dS, dmean, dCp, dQp, dcn, dch, dqn, dqh, dnnd, drd;
    DevBuf<int32_t> dsize, dalive, dnn, dact, dstale, dpairs, dcid, dqid, dra, drb, drn;
    DevBuf<int> dbc, dtot;
    if ((rc = dS.alloc((size_t)M * D)) || (rc = dmean.alloc((size_t)D)) || (rc = dCp.alloc((size_t)npad * K4)) ||
        (rc = dQp.alloc((size_t)npad * K4)) || (rc = dcn.alloc((size_t)npad)) || (rc = dch.alloc((size_t)npad)) ||
        (rc = dqn.alloc((size_t)npad)) || (rc = dqh.alloc((size_t)npad)) || (rc = dnnd.alloc((size_t)M)) ||
        (rc = drd.alloc((size_t)N)) || (rc = dsize.alloc((size_t)M)) || (rc = dalive.alloc((size_t)M)) ||
        (rc = dnn.alloc((size_t)M)) || (rc = dact.alloc((size_t)N)) || (rc = dstale.alloc((size_t)N)) ||
        (rc = dpairs.alloc((size_t)N)) || (rc = dcid.alloc((size_t)npad)) || (rc = dqid.alloc((size_t)npad)) ||
        (rc = dra.alloc((size_t)N)) || (rc = drb.alloc((size_t)N)) || (rc = drn.alloc((size_t)N)) ||
        (rc = dbc.alloc((size_t)2 * nbmax)) || (rc = dtot.alloc(4)))
        return rc;
    HIPCHECK(hipMemcpy(dS, P, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(dalive, 0, (size_t)M * sizeof(int32_t)));
    HIPCHECK(hipMemset(dnn, 0xFF, (size_t)M * sizeof(int32_t)));
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    if (metric == 1) {
        hipLaunchKernelGGL(k_hc_mean, dim3(D), dim3(256), 0, 0, (const double *)dS, N, D, dmean.get());
        KCHECK();
    }
    hipLaunchKernelGGL(k_hc_points, dim3(cdiv(N, 256)), dim3(256), 0, 0, dS.get(), N, D, metric, (const double *)dmean,
                       dsize.get(), dalive.get(), dnn.get());
    KCHECK();
    // the ordered lists of mode over the ids < top: totals to dtot[2 mode ..]
    auto lists = [&](int mode, int force, int64_t top) -> int {
        const int64_t nb = cdiv(top, 256);
        hipLaunchKernelGGL(k_hc_count, dim3((unsigned)nb), dim3(256), 0, 0, mode, force, top, (const int32_t *)dalive, (const int32_t *)dnn,
                           dbc.get());
        KCHECK();
        hipLaunchKernelGGL(k_hc_offsets, dim3(1), dim3(256), 0, 0, dbc.get(), nb, dtot.get() + 2 * mode);
        KCHECK();
        hipLaunchKernelGGL(k_hc_compact, dim3((unsigned)nb), dim3(256), 0, 0, mode, force, top, (const int32_t *)dalive,
                           (const int32_t *)dnn, (const int *)dbc, mode == 0 ? dact.get() : dpairs.get(),
                           mode == 0 ? dstale.get() : (int32_t *)nullptr);
        KCHECK();
        return INSIDER_OK;
    };
    int tot[4] = {0, 0, 0, 0};   // alive, stale, pairs of the last round
    if ((rc = lists(0, 0, N))) return rc;
    HIPCHECK(hipMemcpy(tot, dtot, sizeof(tot), hipMemcpyDeviceToHost));
    std::vector<int32_t> pt_alive((size_t)N);   // (before any merge: the points that are not dead)
    HIPCHECK(hipMemcpy(pt_alive.data(), dalive, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int Na = tot[0];
    int na = Na, ns = tot[1], base = 0, nround = 0;
    int64_t nquery = 0;
    bool unfinished = false;
    while (na > 1) {
        if (nround == max_rounds) {
            unfinished = true;
            break;
        }
        const int napad = (int)round_up(na, 16 * NT), nspad = (int)round_up(ns, 16);
        hipLaunchKernelGGL(k_hc_cprep, dim3(cdiv(napad, 256)), dim3(256), 0, 0, (const int32_t *)dact, na, napad, (const double *)dS,
                           (const int32_t *)dsize, D, K4, dCp.get(), dcid.get(), dcn.get(), dch.get());
        KCHECK();
        if (ns < 1) return fail(INSIDER_ERR_HIP, "hclust: a round without a stale cluster");   // (cannot happen: a merge makes one)
        hipLaunchKernelGGL(k_hc_cprep, dim3(cdiv(nspad, 256)), dim3(256), 0, 0, (const int32_t *)dstale, ns, nspad,
                           (const double *)dS, (const int32_t *)dsize, D, K4, dQp.get(), dqid.get(), dqn.get(), dqh.get());
        KCHECK();
        KT_DISPATCH(KS, hipLaunchKernelGGL((k_hc_nn<KT_>), dim3(cdiv(ns, 16 * HC_NW)), dim3(64 * HC_NW), lds, 0, (const double *)dQp,
                                           (const int32_t *)dqid, (const double *)dqn, (const double *)dqh, ns, (const double *)dCp,
                                           (const int32_t *)dcid, (const double *)dcn, (const double *)dch, na, napad, K4, NT, metric,
                                           dnn.get(), dnnd.get()));
        KCHECK();
        const int64_t top = N + base;
        if ((rc = lists(1, 0, top))) return rc;
        hipLaunchKernelGGL(k_hc_merge, dim3(cdiv(na / 2, 4)), dim3(256), 0, 0, (const int32_t *)dpairs, (const int *)dtot.get() + 2, N,
                           base, D, dS.get(), dsize.get(), dalive.get(), dnn.get(), (const double *)dnnd, dra.get(), drb.get(),
                           drd.get(), drn.get());
        KCHECK();
        if ((rc = lists(0, 0, top + na / 2))) return rc;
        HIPCHECK(hipMemcpy(tot, dtot, sizeof(tot), hipMemcpyDeviceToHost));   // the round's record: all the host reads
        ++nround;
        nquery += ns;
        if (tot[2] == 0) {   // no reciprocal pair among kept and new neighbours: everything is asked again
            if ((rc = lists(0, 1, top))) return rc;
            HIPCHECK(hipMemcpy(tot, dtot, sizeof(tot), hipMemcpyDeviceToHost));
        }
        base += tot[2];
        na = tot[0];
        ns = tot[1];
    }
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_hclust_ms = ms;
    if (unfinished) return fail(INSIDER_ERR_UNFINISHED, "max_rounds reached before one cluster was left");
    std::vector<int32_t> ra((size_t)base), rb((size_t)base), rn((size_t)base);
    std::vector<double> rd((size_t)base);
    if (base > 0) {
        HIPCHECK(hipMemcpy(ra.data(), dra, (size_t)base * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(rb.data(), drb, (size_t)base * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(rn.data(), drn, (size_t)base * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(rd.data(), drd, (size_t)base * sizeof(double), hipMemcpyDeviceToHost));
    }
    hc_finish(N, pt_alive, metric, ra, rb, rd, rn, merge, height, size, order);
    *rounds = nround;
    *queries = nquery;
    *alive = Na;
    return INSIDER_OK;
}

double insider_hip_last_hclust_ms(void) { return g_last_hclust_ms; }

// ---- t-SNE (insider_tsne.hpp) ---------------------------------------------------------------------------------------------
int insider_hip_tsne(const int32_t *nbr_idx, const double *nbr_d2, int64_t N, int k, double perplexity, const double *init,
                     int max_iter, int exag_iters, int kl_every, double exaggeration, double eta, uint64_t seed, int slabs,
                     int device, double *Y, double *kl_traj, double *final_kl, double *beta, double *p_cond, double *grad, double *Z)
{
    if (!nbr_idx || !nbr_d2 || !Y || !kl_traj || !final_kl) return fail(INSIDER_ERR_ARG, "null argument");
    if (N < 1 || N > ((int64_t)1 << 20)) return fail(INSIDER_ERR_ARG, "N must be in 1..2^20");
    if (k < 1 || k > TS_MAX_K) return fail(INSIDER_ERR_ARG, "k must be in 1..64");
    if (!std::isfinite(perplexity) || perplexity < 1.0) return fail(INSIDER_ERR_ARG, "perplexity must be finite and >= 1");
    if (max_iter < 0 || max_iter > 10000) return fail(INSIDER_ERR_ARG, "max_iter must be in 0..10000");
    if (exag_iters < 0 || exag_iters > 10000) return fail(INSIDER_ERR_ARG, "exag_iters must be in 0..10000");
    if (kl_every < 1) return fail(INSIDER_ERR_ARG, "kl_every must be >= 1");
    if (!std::isfinite(exaggeration) || exaggeration < 1.0) return fail(INSIDER_ERR_ARG, "exaggeration must be finite and >= 1");
    if (!std::isfinite(eta) || eta < 0.0) return fail(INSIDER_ERR_ARG, "eta must be finite and >= 0");
    if (slabs < 0 || slabs > TS_MAX_SLABS) return fail(INSIDER_ERR_ARG, "slabs must be in 0..64");
    if (max_iter == 0 && !init) return fail(INSIDER_ERR_ARG, "max_iter = 0 needs init");
    // the graph: filled slots first, in range, no self edge, no repeat within a row, d2 finite and >= 0; the in-degrees
    std::vector<int32_t> rev_ptr((size_t)N + 1, 0);
    {
        std::vector<int32_t> seen((size_t)N, -1);   // the last row each target was met in
        for (int64_t i = 0; i < N; ++i) {
            bool open = false;
            for (int s = 0; s < k; ++s) {
                const int32_t j = nbr_idx[(size_t)i * k + s];
                if (j < 0) {
                    if (j != -1) return fail(INSIDER_ERR_ARG, "neighbour index out of range");
                    open = true;
                    continue;
                }
                if (open) return fail(INSIDER_ERR_ARG, "a filled slot follows an open one");
                if (j >= N) return fail(INSIDER_ERR_ARG, "neighbour index out of range");
                if (j == i) return fail(INSIDER_ERR_ARG, "a row names itself");
                if (seen[j] == (int32_t)i) return fail(INSIDER_ERR_ARG, "an index is repeated within a row");
                seen[j] = (int32_t)i;
                const double d = nbr_d2[(size_t)i * k + s];
                if (!std::isfinite(d) || d < 0.0) return fail(INSIDER_ERR_ARG, "d2 must be finite and >= 0 in a filled slot");
                ++rev_ptr[(size_t)j + 1];
            }
        }
    }
    if (init && !all_finite(init, (size_t)2 * N)) return fail(INSIDER_ERR_ARG, "init must be finite");
    // alive = a filled slot of its own or a place in somebody's row; cmp = the compact number of an alive point
    std::vector<int32_t> cmp((size_t)N, -1), alive;
    alive.reserve((size_t)N);
    for (int64_t i = 0; i < N; ++i)
        if (nbr_idx[(size_t)i * k] >= 0 || rev_ptr[(size_t)i + 1] > 0) {
            cmp[i] = (int32_t)alive.size();
            alive.push_back((int32_t)i);
        }
    const int n = (int)alive.size();
    if (n < 2) return fail(INSIDER_ERR_ARG, "fewer than 2 alive points");
    const size_t nk = (size_t)n * k;
    // the compacted graph and its transpose: a stable counting sort of the edges by target (sources ascend, then slots)
    std::vector<int32_t> cidx(nk, -1), mate(nk, -1), ro_ptr((size_t)n + 1, 0), ro_src, ro_flat;
    std::vector<double> cd2(nk, 0.0);
    {
        std::vector<int32_t> rptr((size_t)n + 1, 0);
        for (int c = 0; c < n; ++c) rptr[(size_t)c + 1] = rptr[c] + rev_ptr[(size_t)alive[c] + 1];
        std::vector<int32_t>().swap(rev_ptr);
        const size_t ne = (size_t)rptr[n];
        std::vector<int32_t> rev_src(ne), rev_slot(ne), next(rptr.begin(), rptr.end() - 1);
        for (int c = 0; c < n; ++c) {
            const size_t src = (size_t)alive[c] * k;
            for (int s = 0; s < k && nbr_idx[src + s] >= 0; ++s) {
                const int32_t t = cmp[nbr_idx[src + s]];
                cidx[(size_t)c * k + s] = t;
                cd2[(size_t)c * k + s] = nbr_d2[src + s];
                rev_src[next[t]] = c;
                rev_slot[next[t]] = s;
                ++next[t];
            }
        }
        // a reverse edge whose source is in the row merges into that forward slot (mate); the others form the reverse-only list
        std::vector<int32_t> where((size_t)n, -1);   // the slot of target t in the current row
        ro_src.reserve(ne);
        ro_flat.reserve(ne);
        for (int c = 0; c < n; ++c) {
            for (int s = 0; s < k && cidx[(size_t)c * k + s] >= 0; ++s) where[cidx[(size_t)c * k + s]] = s;
            for (int32_t e = rptr[c]; e < rptr[(size_t)c + 1]; ++e) {
                const int32_t j = rev_src[e], flat = j * k + rev_slot[e];
                if (where[j] >= 0) mate[(size_t)c * k + where[j]] = flat;
                else {
                    ro_src.push_back(j);
                    ro_flat.push_back(flat);
                }
            }
            for (int s = 0; s < k && cidx[(size_t)c * k + s] >= 0; ++s) where[cidx[(size_t)c * k + s]] = -1;
            ro_ptr[(size_t)c + 1] = (int32_t)ro_src.size();
        }
    }
    const size_t nro = ro_src.size();
    if (nro == 0) {   // (an upload is never empty)
        ro_src.push_back(0);
        ro_flat.push_back(0);
    }
    // the start, compacted: the caller's, or the draw of include/insider_hip.h
    std::vector<double> y0((size_t)2 * n);
    {
        const uint32_t key = insider_sample_key(seed, 0U);
        for (int c = 0; c < n; ++c)
            for (int d = 0; d < 2; ++d) {
                const size_t e = (size_t)2 * alive[c] + d;
                y0[(size_t)2 * c + d] = init ? init[e] : insider_tsne_draw(key, (uint32_t)e);
            }
    }
    int rc = cd_common_checks(1, N, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    const int tiles = cdiv(n, TS_TILE);
    if (slabs == 0) slabs = std::max(1, std::min({TS_MAX_SLABS, cdiv(TS_BLOCKS, tiles), n / TS_MIN_SLAB}));
    const int slab_len = cdiv(n, slabs);
    const int nb = cdiv(n, 256), nsb = cdiv(n, TS_ROWS);
    const int nrec = max_iter / kl_every + 1;
    const double eta_used = eta > 0.0 ? eta : std::max((double)n / (4.0 * exaggeration), 50.0);
    DevBuf<int32_t> didx, dmate, dro_ptr, dro_src, dro_flat;
    DevBuf<double> dd2, dbeta, dpc, dPF, dPR, dYa, dYb, dV, dG, dgrad, dpart, drep, dzpart, dspart, dscal, dkl;
    if ((rc = didx.upload(cidx)) || (rc = dmate.upload(mate)) || (rc = dro_ptr.upload(ro_ptr)) || (rc = dro_src.upload(ro_src)) ||
        (rc = dro_flat.upload(ro_flat)) || (rc = dd2.upload(cd2)) || (rc = dYa.upload(y0)) || (rc = dbeta.alloc((size_t)n)) ||
        (rc = dpc.alloc(nk)) || (rc = dPF.alloc(nk)) || (rc = dPR.alloc(nro)) || (rc = dYb.alloc((size_t)2 * n)) ||
        (rc = dV.alloc((size_t)2 * n)) || (rc = dG.alloc((size_t)2 * n)) || (rc = dgrad.alloc((size_t)2 * n)) ||
        (rc = dpart.alloc((size_t)slabs * n * 3)) || (rc = drep.alloc((size_t)n * 3)) || (rc = dzpart.alloc((size_t)nb)) ||
        (rc = dspart.alloc((size_t)nsb * 3)) || (rc = dscal.alloc(8)) || (rc = dkl.alloc((size_t)nrec)))
        return rc;
    {
        const std::vector<double> ones((size_t)2 * n, 1.0);
        HIPCHECK(hipMemcpy(dG, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(dV, 0, (size_t)2 * n * sizeof(double)));
    }
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    hipLaunchKernelGGL(k_ts_calibrate, dim3(nb), dim3(256), 0, 0, (const int32_t *)didx, (const double *)dd2, n, k, perplexity,
                       dbeta.get(), dpc.get());
    KCHECK();
    hipLaunchKernelGGL(k_ts_joint, dim3(cdiv((int64_t)std::max(nk, nro), 256)), dim3(256), 0, 0, (const double *)dpc,
                       (const int32_t *)dmate, (int64_t)nk, (const int32_t *)dro_flat, (int64_t)nro, 2.0 * (double)n, dPF.get(),
                       dPR.get());
    KCHECK();
    double2 *ycur = (double2 *)dYa.get(), *ynew = (double2 *)dYb.get();
    double *zsum = dscal.get(), *ssum = dscal.get() + 1, *zout = dscal.get() + 4;
    // Z and the rows' repulsive sums at ycur
    auto repulse = [&]() -> int {
        hipLaunchKernelGGL(k_ts_repulse, dim3(tiles, slabs), dim3(256), 0, 0, (const double2 *)ycur, n, slab_len, dpart.get());
        KCHECK();
        hipLaunchKernelGGL(k_ts_reduce, dim3(nb), dim3(256), 0, 0, (const double *)dpart, slabs, n, drep.get(), dzpart.get());
        KCHECK();
        hipLaunchKernelGGL(k_ts_fold, dim3(1), dim3(256), 0, 0, (const double *)dzpart, nb, 1, zsum);
        KCHECK();
        return INSIDER_OK;
    };
    auto step = [&](double a, double mu, int update, int record) -> int {
        hipLaunchKernelGGL(k_ts_step, dim3(nsb), dim3(256), 0, 0, (const int32_t *)didx, (const double *)dPF,
                           (const int32_t *)dro_ptr, (const int32_t *)dro_src, (const double *)dPR, (const double *)drep,
                           (const double *)zsum, n, k, a, mu, eta_used, update, record, (const double2 *)ycur, ynew,
                           (double2 *)dV.get(), (double2 *)dG.get(), (double2 *)dgrad.get(), dspart.get(), update ? nullptr : zout);
        KCHECK();
        hipLaunchKernelGGL(k_ts_fold, dim3(1), dim3(256), 0, 0, (const double *)dspart, nsb, 3, ssum);
        KCHECK();
        return INSIDER_OK;
    };
    for (int t = 0; t < max_iter; ++t) {
        const bool early = t < exag_iters, record = t % kl_every == 0;
        if ((rc = repulse()) || (rc = step(early ? exaggeration : 1.0, early ? 0.5 : 0.8, 1, record))) return rc;
        hipLaunchKernelGGL(k_ts_centre, dim3(nb), dim3(256), 0, 0, (const double *)ssum, n, ynew,
                           record ? dkl.get() + t / kl_every : nullptr);
        KCHECK();
        std::swap(ycur, ynew);
    }
    // the final Y: Z, KL and the gradient under exaggeration 1; nothing moves
    if ((rc = repulse()) || (rc = step(1.0, 0.0, 0, 1))) return rc;
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_tsne_ms = ms;
    // every result is staged on the host first: a failed download leaves the caller's arrays as they were
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> hY((size_t)2 * n), hkl((size_t)nrec, nan), hbeta, hpc, hgrad;
    double scal[8];
    HIPCHECK(hipMemcpy(hY.data(), ycur, hY.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(scal, dscal, sizeof(scal), hipMemcpyDeviceToHost));
    const int nloop = (max_iter + kl_every - 1) / kl_every;   // the records of the loop: t = 0, kl_every, ... < max_iter
    if (nloop) HIPCHECK(hipMemcpy(hkl.data(), dkl, (size_t)nloop * sizeof(double), hipMemcpyDeviceToHost));
    if (max_iter % kl_every == 0) hkl[(size_t)max_iter / kl_every] = scal[3];
    if (beta) {
        hbeta.resize((size_t)n);
        HIPCHECK(hipMemcpy(hbeta.data(), dbeta, hbeta.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (p_cond) {
        hpc.resize(nk);
        HIPCHECK(hipMemcpy(hpc.data(), dpc, hpc.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (grad) {
        hgrad.resize((size_t)2 * n);
        HIPCHECK(hipMemcpy(hgrad.data(), dgrad, hgrad.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::fill(Y, Y + (size_t)2 * N, nan);
    if (beta) std::fill(beta, beta + (size_t)N, nan);
    if (p_cond) std::fill(p_cond, p_cond + (size_t)N * k, 0.0);
    if (grad) std::fill(grad, grad + (size_t)2 * N, nan);
    for (int c = 0; c < n; ++c) {
        const size_t i = (size_t)alive[c];
        Y[2 * i] = hY[(size_t)2 * c];
        Y[2 * i + 1] = hY[(size_t)2 * c + 1];
        if (beta) beta[i] = hbeta[c];
        if (p_cond) std::copy(hpc.begin() + (size_t)c * k, hpc.begin() + (size_t)(c + 1) * k, p_cond + i * k);
        if (grad) {
            grad[2 * i] = hgrad[(size_t)2 * c];
            grad[2 * i + 1] = hgrad[(size_t)2 * c + 1];
        }
    }
    std::copy(hkl.begin(), hkl.end(), kl_traj);
    *final_kl = scal[3];
    if (Z) *Z = scal[4];
    return INSIDER_OK;
}

double insider_hip_last_tsne_ms(void) { return g_last_tsne_ms; }

// ---- enrichment (insider_enrich.hpp) -----------------------------------------------------------------------------------------
int insider_hip_enrichment_sample(uint64_t seed, uint32_t perm, int64_t m, int64_t p, int32_t *out)
{
    if (!out) return fail(INSIDER_ERR_ARG, "null argument");
    if (p < 2 || p > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "p must be in 2..2^31-1");
    if (m < 0 || m > p) return fail(INSIDER_ERR_ARG, "m must be in 0..p");
    const uint32_t key = insider_sample_key(seed, perm), half = insider_sample_half((uint32_t)p);
    for (int64_t j = 0; j < m; ++j) out[j] = (int32_t)insider_sample_phi(key, half, (uint32_t)p, (uint32_t)j);
    return INSIDER_OK;
}

int insider_hip_enrichment(const double *scores, int64_t R, int64_t p, const int64_t *set_ptr, const int32_t *set_genes,
                           int64_t S, int weight, int nperm, uint64_t seed, int device, double *es, int32_t *peak,
                           int32_t *n_ge, int32_t *n_same, double *sum_same, int32_t *hits_nonzero)
{
    if (!scores || !set_ptr || !set_genes || !es || !peak || !n_ge || !n_same || !sum_same || !hits_nonzero)
        return fail(INSIDER_ERR_ARG, "null argument");
    if (R < 0 || S < 0) return fail(INSIDER_ERR_ARG, "R and S must be >= 0");
    if (p < 2 || p > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_ARG, "p must be in 2..2^31-1");
    if (weight != 0 && weight != 1) return fail(INSIDER_ERR_ARG, "weight must be 0 or 1");
    if (nperm < 1 || nperm > 65536) return fail(INSIDER_ERR_ARG, "nperm must be in 1..65536");
    if (S > (int64_t)std::numeric_limits<int32_t>::max()) return fail(INSIDER_ERR_UNSUPPORTED, "S must be < 2^31");
    if (set_ptr[0] < 0) return fail(INSIDER_ERR_ARG, "set_ptr must not be negative");
    if (S > 0) {
        std::vector<int32_t> seen((size_t)p, -1);   // the last set each gene was met in
        for (int64_t s = 0; s < S; ++s) {
            const int64_t m = set_ptr[s + 1] - set_ptr[s];
            if (m < 0) return fail(INSIDER_ERR_ARG, "set_ptr must not decrease");
            if (m < 1 || m >= p || m > GS_MAX_SET) return fail(INSIDER_ERR_ARG, "a set must hold 1..min(p - 1, 4096) genes");
            for (int64_t e = set_ptr[s]; e < set_ptr[s + 1]; ++e) {
                const int32_t g = set_genes[e];
                if (g < 0 || g >= p) return fail(INSIDER_ERR_ARG, "gene index out of range");
                if (seen[g] == (int32_t)s) return fail(INSIDER_ERR_ARG, "a gene is repeated within a set");
                seen[g] = (int32_t)s;
            }
        }
    }
    if (!all_finite(scores, (size_t)R * p)) return fail(INSIDER_ERR_ARG, "scores must be finite");
    if (R == 0 || S == 0) return INSIDER_OK;
    int rc = cd_common_checks(1, R, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    // the ranking: descending score, ties by ascending gene (a stable sort of 0..p-1)
    std::vector<int32_t> rank((size_t)R * p), order((size_t)p);
    std::vector<double> aw((size_t)R * p);
    for (int64_t r = 0; r < R; ++r) {
        const double *sc = scores + (size_t)r * p;
        for (int64_t g = 0; g < p; ++g) order[g] = (int32_t)g;
        std::stable_sort(order.begin(), order.end(), [sc](int32_t a, int32_t b) { return sc[a] > sc[b]; });
        for (int64_t t = 0; t < p; ++t) {
            rank[(size_t)r * p + order[t]] = (int32_t)t;
            aw[(size_t)r * p + t] = std::fabs(sc[order[t]]);
        }
    }
    // the sets by size: size_sets lists the set ids in ascending (size, id), sizes / size_ptr its runs of one size
    std::vector<int32_t> size_sets((size_t)S), sizes, size_ptr;
    for (int64_t s = 0; s < S; ++s) size_sets[s] = (int32_t)s;
    auto msize = [set_ptr](int32_t s) { return (int32_t)(set_ptr[s + 1] - set_ptr[s]); };
    std::stable_sort(size_sets.begin(), size_sets.end(), [&](int32_t a, int32_t b) { return msize(a) < msize(b); });
    for (int64_t q = 0; q < S; ++q)
        if (q == 0 || msize(size_sets[q]) != sizes.back()) {
            sizes.push_back(msize(size_sets[q]));
            size_ptr.push_back((int32_t)q);
        }
    size_ptr.push_back((int32_t)S);
    const int64_t nnz = set_ptr[S];
    DevBuf<int32_t> drank, dgenes, dsets, dsizes, dszptr, dpeak, dnge, dnsame, dhits;
    DevBuf<double> daw, des, dsum;
    DevBuf<int64_t> dptr;
    if ((rc = drank.upload(rank)) || (rc = daw.upload(aw)) || (rc = dsets.upload(size_sets)) || (rc = dsizes.upload(sizes)) ||
        (rc = dszptr.upload(size_ptr)) || (rc = dgenes.alloc((size_t)nnz)) || (rc = dptr.alloc((size_t)S + 1)) ||
        (rc = des.alloc((size_t)R * S)) || (rc = dsum.alloc((size_t)R * S)) || (rc = dpeak.alloc((size_t)R * S)) ||
        (rc = dnge.alloc((size_t)R * S)) || (rc = dnsame.alloc((size_t)R * S)) || (rc = dhits.alloc((size_t)R * S)))
        return rc;
    HIPCHECK(hipMemcpy(dgenes, set_genes, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dptr, set_ptr, ((size_t)S + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    const uint32_t half = insider_sample_half((uint32_t)p);
    Stopwatch watch;
    if ((rc = watch.start(0))) return rc;
    // one pair of launches per class of sizes that sort at the same padded length M2
    const int nsz_all = (int)sizes.size();
    for (int z0 = 0; z0 < nsz_all;) {
        int M2 = 64;
        while (M2 < sizes[z0]) M2 <<= 1;
        int z1 = z0;
        while (z1 < nsz_all && sizes[z1] <= M2) ++z1;
        const int q0 = size_ptr[z0], nsets = size_ptr[z1] - q0, nsz = z1 - z0;
        const int64_t ntask_o = R * nsets, ntask_n = R * nsz;
        const int64_t cap = (int64_t)1 << 20;
        hipLaunchKernelGGL(k_gs_observed, dim3((unsigned)std::min(ntask_o, cap)), dim3(64), (size_t)M2 * sizeof(int), 0,
                           (const int32_t *)drank, (const double *)daw, p, (const int64_t *)dptr, (const int32_t *)dgenes,
                           (const int32_t *)dsets.get() + q0, nsets, ntask_o, M2, weight, S, des.get(), dpeak.get(), dhits.get());
        KCHECK();
#define GS_NULL(NW_)                                                                                                         \
    hipLaunchKernelGGL((k_gs_null<NW_>), dim3((unsigned)std::min(ntask_n, cap)), dim3(64 * NW_),                             \
                       (size_t)NW_ * M2 * sizeof(int) + GS_CHUNK * sizeof(double), 0, (const double *)daw, p, half, seed,    \
                       nperm, (const int32_t *)dsizes.get() + z0, (const int32_t *)dszptr.get() + z0, (const int32_t *)dsets, \
                       nsz, ntask_n, M2, weight, S, (const double *)des, dnge.get(), dnsame.get(), dsum.get())
        if (M2 <= 2048) GS_NULL(4);
        else GS_NULL(2);
#undef GS_NULL
        KCHECK();
        z0 = z1;
    }
    float ms = 0.0f;
    if ((rc = watch.stop_ms(0, &ms))) return rc;
    g_last_enrichment_ms = ms;
    HIPCHECK(hipMemcpy(es, des, (size_t)R * S * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(sum_same, dsum, (size_t)R * S * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(peak, dpeak, (size_t)R * S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(n_ge, dnge, (size_t)R * S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(n_same, dnsame, (size_t)R * S * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hits_nonzero, dhits, (size_t)R * S * sizeof(int32_t), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

double insider_hip_last_enrichment_ms(void) { return g_last_enrichment_ms; }

// optimize_continuous_v2 (src/optimize.cpp:76-137) with the reference's eight arguments, on an arbitrary `data` matrix
// (insider_cont_v2.hpp): one streaming pass over (data, indicator) for the per-gene sums, the K x K weighted Gram, then the
// reference's cyclic scalar passes (tuning = 1, k_cont_cd) or its one ridge solve (tuning = 0, k_level_solve).
int insider_hip_optimize_continuous_v2(const double *data, int64_t n, int64_t p, const uint8_t *indicator,
                                       double *updating_factor, const double *c_factor, int K, const double *updating_confd,
                                       const double *gram, double lambda, int tuning, int device)
{
    if (tuning != 0 && tuning != 1)   // the reference prints and exit(1)s (src/optimize.cpp:133-136)
        return fail(INSIDER_ERR_ARG, "Parameter tuning should be either 0 or 1!");
    if (!data || !updating_factor || !c_factor || !updating_confd) return fail(INSIDER_ERR_ARG, "null argument");
    if (tuning == 1 && !indicator) return fail(INSIDER_ERR_ARG, "tuning = 1 needs the indicator matrix");
    if (tuning == 0 && !gram) return fail(INSIDER_ERR_ARG, "tuning = 0 needs gram (K x K)");
    if (n < 1 || p < 1) return fail(INSIDER_ERR_ARG, "n and p must be >= 1");
    if (!(lambda == lambda)) return fail(INSIDER_ERR_ARG, "lambda is NaN");
    if (K < 1 || K > INSIDER_MAX_K) return fail(INSIDER_ERR_UNSUPPORTED, "K must be in 1..63");
    int rc = cd_common_checks(K, 1, device);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(device));
    const int NB = (K + 1 + 15) / 16, KP = 16 * NB, len = KP * KP + KP;
    const int nslab = cdiv(p, CV2_SLAB);
    const size_t np = (size_t)n * (size_t)p;
    DevBuf<double> dD, dC, dz, dw, dt, dpart, deq, du, dg, dzz;
    DevBuf<uint8_t> dM;
    DevBuf<int> dflag;   // [0] the solve's fail flag, [1] a level count of 1 for k_level_solve
    if ((rc = dD.alloc(np)) || (rc = dC.alloc((size_t)K * p)) || (rc = dz.alloc((size_t)n)) || (rc = dt.alloc((size_t)p)) ||
        (rc = dpart.alloc((size_t)nslab * len)) || (rc = deq.alloc((size_t)len)) || (rc = du.alloc((size_t)KP)) || (rc = dflag.alloc(2)))
        return rc;
    HIPCHECK(hipMemcpy(dD, data, np * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dC, c_factor, (size_t)K * p * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dz, updating_confd, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(du, 0, (size_t)KP * sizeof(double)));
    HIPCHECK(hipMemcpy(du, updating_factor, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    const int flag0[2] = {0, 1};
    HIPCHECK(hipMemcpy(dflag, flag0, sizeof(flag0), hipMemcpyHostToDevice));
    if (tuning == 1) {
        if ((rc = dM.alloc(np)) || (rc = dw.alloc((size_t)p))) return rc;
        HIPCHECK(hipMemcpy(dM, indicator, np, hipMemcpyHostToDevice));
        hipLaunchKernelGGL((k_cv2_gene<true>), dim3(cdiv(p, 4)), dim3(256), 0, 0, (const double *)dD, (const uint8_t *)dM,
                           (const double *)dz, n, p, dw, dt);
    } else {
        if ((rc = dg.alloc((size_t)K * K)) || (rc = dzz.alloc(1))) return rc;
        HIPCHECK(hipMemcpy(dg, gram, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_cv2_zz, dim3(1), dim3(64), 0, 0, (const double *)dz, n, dzz);
        hipLaunchKernelGGL((k_cv2_gene<false>), dim3(cdiv(p, 4)), dim3(256), 0, 0, (const double *)dD, (const uint8_t *)nullptr,
                           (const double *)dz, n, p, (double *)nullptr, dt);
    }
    KCHECK();
    hipLaunchKernelGGL(k_cv2_eq_part, dim3(nslab), dim3(256), 0, 0, (const double *)dC, (const double *)dw, (const double *)dt, K, KP,
                       p, dpart);
    KCHECK();
    hipLaunchKernelGGL(k_cv2_eq_sum, dim3(cdiv(len, 256)), dim3(256), 0, 0, (const double *)dpart, nslab, K, KP,
                       (const double *)dg, (const double *)dzz, deq);
    KCHECK();
    NB_DISPATCH(NB, {
        (void)WPB_;
        if (tuning == 1)   // :102-126
            hipLaunchKernelGGL((k_cont_cd<NB_>), dim3(1), dim3(64), 0, 0, (const double *)deq, K, lambda, du);
        else               // :127-131
            hipLaunchKernelGGL((k_level_solve<NB_>), dim3(1), dim3(64), 0, 0, (const double *)deq, (const int *)(dflag + 1), 1, K,
                               lambda, du, dflag);
    });
    KCHECK();
    HIPCHECK(hipDeviceSynchronize());
    int flag = 0;
    HIPCHECK(hipMemcpy(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost));
    if (flag) return fail(INSIDER_ERR_SOLVE, "the ridge system of the continuous covariate is singular to working precision");
    HIPCHECK(hipMemcpy(updating_factor, du, (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

static int masked_gram_common(insider_hip_handle *h, bool cols, const double *Fhost, int K, double *G_out, double *q_out)
{
    if (!h || !Fhost || !G_out || !q_out) return fail(INSIDER_ERR_ARG, "null argument");
    HIPCHECK(hipSetDevice(h->ds->device));
    int rc = ensure_workspace(h, K);
    if (rc) return rc;
    plan_call(h, 1);
    const int KP = h->ws.KP, STAT = h->plan.stat_len;
    const int64_t units = cols ? h->ds->p : h->ds->n, flen = cols ? h->ds->n : h->ds->p;
    double *F = cols ? h->ws.R : h->ws.C, *full = cols ? h->ws.RtR : h->ws.CCt;
    // host factor: cols -> R is n x K column-major; rows -> C is K x p column-major (= p rows of K)
    HIPCHECK(hipMemcpy(h->ws.stage, Fhost, (size_t)flen * K * sizeof(double), hipMemcpyHostToDevice));
    if (cols) hipLaunchKernelGGL(k_pack_A, dim3(cdiv(flen * KP, 256)), dim3(256), 0, h->st.stream, (const double *)h->ws.stage,
                                 (int)flen, K, KP, F);
    else hipLaunchKernelGGL(k_pack_rows, dim3(cdiv(flen * KP, 256)), dim3(256), 0, h->st.stream, (const double *)h->ws.stage,
                            flen, K, KP, F);
    KCHECK();
    if ((rc = launch_gram(h, F, flen, full))) return rc;
    const int nseg = cols ? 1 : h->ws.nseg;
    DevBuf<double> stat, qf, Gd, qd;
    if ((rc = stat.alloc((size_t)nseg * units * STAT)) || (rc = qf.alloc((size_t)units * KP)) || (rc = Gd.alloc((size_t)units * K * K)) ||
        (rc = qd.alloc((size_t)units * K)))
        return rc;
    if ((rc = launch_list_stats(h, cols, nseg, F, stat))) return rc;
    // dense X'F over all entries from the gene-major copy (rows: strided reads; stand-alone API only)
    if (cols) hipLaunchKernelGGL(k_line_dense_xty, dim3((unsigned)units), dim3(64), 0, h->st.stream, (const double *)h->ds->X,
                                 h->ds->ldn, (int)flen, (const double *)F, K, KP, qf);
    else hipLaunchKernelGGL(k_row_dense_xty, dim3((unsigned)units), dim3(64), 0, h->st.stream, (const double *)h->ds->X, h->ds->ldn,
                            (int)flen, (const double *)F, K, KP, qf);
    KCHECK();
    NB_DISPATCH(h->ws.NB, {
        (void)WPB_;
        hipLaunchKernelGGL((k_stats_to_dense<NB_>), dim3((unsigned)units), dim3(64), 0, h->st.stream, (const double *)stat,
                           nseg, (int)units, K, (const double *)full, (const double *)qf, Gd, qd, (double *)nullptr);
    });
    KCHECK();
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    HIPCHECK(hipMemcpy(G_out, Gd, (size_t)units * K * K * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(q_out, qd, (size_t)units * K * sizeof(double), hipMemcpyDeviceToHost));
    // the pad rows of C (genes p..ldp-1) were not touched; R/C now hold the caller's factor
    return INSIDER_OK;
}

int insider_hip_masked_gram_cols(insider_hip_handle *h, const double *R, int K, double *G_out, double *q_out)
{
    return masked_gram_common(h, true, R, K, G_out, q_out);
}

int insider_hip_masked_gram_rows(insider_hip_handle *h, const double *C, int K, double *H_out, double *b_out)
{
    return masked_gram_common(h, false, C, K, H_out, b_out);
}

// The column-side statistics the column solve reads, densified: the first half of insider_hip_optimize_col() with tuning = 1
// (R, R'R, Qfull; the statistics kernel the handle's options pick), then the record of every gene as G, q and its corner.
int insider_hip_col_stats(insider_hip_handle *h, double *const *A, int inc_continuous, int K, double *G_out, double *q_out,
                          double *ss_out)
{
    if (!h || !G_out || !q_out || !ss_out) return fail(INSIDER_ERR_ARG, "null argument");
    int rc = check_factor_args(h, A, G_out, inc_continuous, 1);   // (G_out stands in for the column factor this entry does not take)
    if (rc) return rc;
    if (h->world > 1) return fail(INSIDER_ERR_UNSUPPORTED, "insider_hip_col_stats on a sharded handle");
    HIPCHECK(hipSetDevice(h->ds->device));
    if ((rc = ensure_workspace(h, K))) return rc;
    plan_call(h, 1);
    if ((rc = upload_factors(h, A, nullptr, K))) return rc;
    if ((rc = phase_R(h))) return rc;
    if ((rc = launch_col_stats(h, false))) return rc;
    const int64_t p = h->ds->p;
    DevBuf<double> Gd, qd, sd;
    if ((rc = Gd.alloc((size_t)p * K * K)) || (rc = qd.alloc((size_t)p * K)) || (rc = sd.alloc((size_t)p))) return rc;
    NB_DISPATCH(h->ws.NB, {
        (void)WPB_;   // full = null: the record's K x K part already holds XtX_j (R'R - complement)
        hipLaunchKernelGGL((k_stats_to_dense<NB_>), dim3((unsigned)p), dim3(64), 0, h->st.stream, (const double *)h->ws.stat_col, 1,
                           (int)p, K, (const double *)nullptr, (const double *)h->ws.Qfull, Gd, qd, sd);
    });
    KCHECK();
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    HIPCHECK(hipMemcpy(G_out, Gd, (size_t)p * K * K * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(q_out, qd, (size_t)p * K * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(ss_out, sd, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

double insider_hip_last_cd_ms(void) { return g_last_cd_ms; }
int insider_hip_last_cd_solver(void) { return g_last_cd_solver; }

}  // extern "C"

namespace {
// ---- read-back of the resident data set (diagnostics: insider_hip_get_array "ds:<name>", insider_hip_get_info "ds_bytes:<name>") ----
// Every DevBuf of DataSet, of its CovTables and of FoldIds under the member's name.  The members of CovTables are "<member>:<i>"
// for cov[i], "cont.<member>" for cont, "contm.<member>:<k>" for contm[k] and "contm_lists.<member>" for contm_lists; cont_pair[k]
// is "cont_pair:<k>" (contm[k].paircnt holds the same allocation) and FoldIds::id is "fold_id".
constexpr const char *DS_COV_MEMBERS[] = {"chunk_level", "chunk_begin", "chunk_end", "lvl_chunk_ptr", "grp", "slev", "item_begin",
                                          "item_end", "lvl_item_ptr", "wl_idx", "wl_w", "paircnt"};
constexpr const char *DS_MEMBERS[] = {"X", "codes", "lev", "lvl_off_d", "members_all", "lvl_ptr_all", "lvl_count_all", "Zc",
                                      "one_count", "ident_members", "S", "yy_train", "yy_all", "Strain", "Sheld", "col_ptr",
                                      "row_ptr", "col_idx", "row_idx", "col_val", "row_val", "col_flag", "cf_cnt", "cf_hn",
                                      "cf_sq", "cf_zt", "cont_cnt"};
constexpr int DS_GEOMETRY_INTS = 10 + 6 * (CF_MAXC + 1) + CF_MAXC + CF_MAXC * CF_MAXC;

struct DsView { const void *p = nullptr; size_t bytes = 0; };

template <typename T>
DsView ds_view(const DevBuf<T> &b) { return DsView{b.get(), b.bytes()}; }

bool ds_cov_member(const CovTables &t, const std::string &f, DsView &v)
{
    if (f == "chunk_level") v = ds_view(t.chunk_level);
    else if (f == "chunk_begin") v = ds_view(t.chunk_begin);
    else if (f == "chunk_end") v = ds_view(t.chunk_end);
    else if (f == "lvl_chunk_ptr") v = ds_view(t.lvl_chunk_ptr);
    else if (f == "grp") v = ds_view(t.grp);
    else if (f == "slev") v = ds_view(t.slev);
    else if (f == "item_begin") v = ds_view(t.item_begin);
    else if (f == "item_end") v = ds_view(t.item_end);
    else if (f == "lvl_item_ptr") v = ds_view(t.lvl_item_ptr);
    else if (f == "wl_idx") v = ds_view(t.wl_idx);
    else if (f == "wl_w") v = ds_view(t.wl_w);
    else if (f == "paircnt") v = ds_view(t.paircnt);
    else return false;
    return true;
}

bool ds_member(const DataSet &d, const std::string &f, DsView &v)
{
    if (f == "X") v = ds_view(d.X);
    else if (f == "codes") v = ds_view(d.codes);
    else if (f == "lev") v = ds_view(d.lev);
    else if (f == "lvl_off_d") v = ds_view(d.lvl_off_d);
    else if (f == "members_all") v = ds_view(d.members_all);
    else if (f == "lvl_ptr_all") v = ds_view(d.lvl_ptr_all);
    else if (f == "lvl_count_all") v = ds_view(d.lvl_count_all);
    else if (f == "Zc") v = ds_view(d.Zc);
    else if (f == "one_count") v = ds_view(d.one_count);
    else if (f == "ident_members") v = ds_view(d.ident_members);
    else if (f == "S") v = ds_view(d.S);
    else if (f == "yy_train") v = ds_view(d.yy_train);
    else if (f == "yy_all") v = ds_view(d.yy_all);
    else if (f == "Strain") v = ds_view(d.Strain);
    else if (f == "Sheld") v = ds_view(d.Sheld);
    else if (f == "col_ptr") v = ds_view(d.col_ptr);
    else if (f == "row_ptr") v = ds_view(d.row_ptr);
    else if (f == "col_idx") v = ds_view(d.col_idx);
    else if (f == "row_idx") v = ds_view(d.row_idx);
    else if (f == "col_val") v = ds_view(d.col_val);
    else if (f == "row_val") v = ds_view(d.row_val);
    else if (f == "col_flag") v = ds_view(d.col_flag);
    else if (f == "cf_cnt") v = ds_view(d.cf_cnt);
    else if (f == "cf_hn") v = ds_view(d.cf_hn);
    else if (f == "cf_sq") v = ds_view(d.cf_sq);
    else if (f == "cf_zt") v = ds_view(d.cf_zt);
    else if (f == "cont_cnt") v = ds_view(d.cont_cnt);
    else return false;
    return true;
}

// "<name>" or "<name>:<i>" -> the array (v.p null: the data set did not build it).  false: no such name.
bool ds_lookup(const DataSet &d, const std::string &full, DsView &v)
{
    v = DsView{};
    std::string name = full;
    long idx = -1;
    const size_t colon = full.find(':');
    if (colon != std::string::npos) {
        const std::string tail = full.substr(colon + 1);
        if (tail.empty() || tail.size() > 6 || tail.find_first_not_of("0123456789") != std::string::npos) return false;
        idx = std::stol(tail);
        name = full.substr(0, colon);
    }
    if (name == "fold_id") {
        if (idx >= 0) return false;
        if (const std::shared_ptr<const FoldIds> f = d.get_folds()) v = ds_view(f->id);
        return true;
    }
    if (name == "cont_pair") {
        if (idx < 0 || idx >= std::max(d.m, 1)) return false;
        if ((size_t)idx < d.cont_pair.size()) v = ds_view(d.cont_pair[idx]);
        return true;
    }
    if (name.rfind("cont.", 0) == 0) return idx < 0 && ds_cov_member(d.cont, name.substr(5), v);
    if (name.rfind("contm_lists.", 0) == 0) return idx < 0 && ds_cov_member(d.contm_lists, name.substr(12), v);
    if (name.rfind("contm.", 0) == 0) {
        if (idx < 0 || idx >= std::max(d.m, 1)) return false;
        static const CovTables none;
        return ds_cov_member((size_t)idx < d.contm.size() ? d.contm[idx] : none, name.substr(6), v);
    }
    if (idx >= 0) return idx < d.c && ds_cov_member(d.cov[idx], name, v);
    return ds_member(d, name, v);
}

// every name ds_lookup knows, one per line; ":#" marks a name that takes an index (covariate, or continuous column)
std::string ds_name_list()
{
    std::string s;
    for (const char *f : DS_MEMBERS) s += std::string(f) + "\n";
    s += "cont_pair:#\nfold_id\n";
    for (const char *f : DS_COV_MEMBERS) s += std::string(f) + ":#\n";
    for (const char *f : DS_COV_MEMBERS) s += std::string("cont.") + f + "\n";
    for (const char *f : DS_COV_MEMBERS) s += std::string("contm.") + f + ":#\n";
    for (const char *f : DS_COV_MEMBERS) s += std::string("contm_lists.") + f + "\n";
    return s;
}

// the static part of ColFacArgs as int32 (order: include/insider_hip.h, "ds:cf_geometry")
std::vector<int32_t> ds_geometry(const DataSet &d)
{
    const ColFacArgs &cf = d.cf;
    std::vector<int32_t> g;
    g.reserve(DS_GEOMETRY_INTS);
    for (int x : {cf.c, cf.nsteps, cf.tab_skip_lo, cf.tab_skip_n, cf.tab_rows, cf.cnt_stride, cf.hn_stride, cf.zt_stride,
                  cf.sq_stride, cf.m})
        g.push_back(x);
    for (const int *a : {cf.L, cf.off, cf.nlater, cf.cnt_off, cf.hn_off, cf.zt_off})
        for (int t = 0; t <= CF_MAXC; ++t) g.push_back(a[t]);
    for (int t = 0; t < CF_MAXC; ++t) g.push_back(cf.pos_cov[t]);
    for (int t = 0; t < CF_MAXC; ++t)
        for (int k = 0; k < CF_MAXC; ++k) g.push_back(cf.later_plane[t][k]);
    return g;
}

// the scalar facts of the data set ("ds_..."); false: not one of them
bool ds_info(const DataSet &d, const std::string &s, double *out)
{
    if (s == "ds_ldn") *out = (double)d.ldn;
    else if (s == "ds_ldp") *out = (double)d.ldp;
    else if (s == "ds_SLP") *out = d.SLP;
    else if (s == "ds_cnt_train") *out = d.cnt_train;
    else if (s == "ds_cnt_test") *out = d.cnt_test;
    else if (s == "ds_no_na") *out = d.no_na ? 1.0 : 0.0;
    else if (s == "ds_merged") *out = d.merged ? 1.0 : 0.0;
    else if (s == "ds_cont_merged") *out = d.cont_merged ? 1.0 : 0.0;
    else if (s == "ds_cf_pair_ok") *out = d.cf_pair_ok ? 1.0 : 0.0;
    else if (s == "ds_max_chunks") *out = d.max_chunks;
    else if (s == "ds_max_L") *out = d.max_L;
    else if (s == "ds_max_items") *out = d.max_items;
    else if (s.rfind("ds_nitems:", 0) == 0 || s.rfind("ds_npairs:", 0) == 0) {
        const std::string tail = s.substr(10);
        if (tail.empty() || tail.size() > 6 || tail.find_first_not_of("0123456789") != std::string::npos) return false;
        const long i = std::stol(tail);
        if (i >= d.c) return false;
        *out = s[4] == 'i' ? (double)d.cov[i].nitems : (double)d.cov[i].npairs;
    } else return false;
    return true;
}
}  // namespace

extern "C" {

int insider_hip_get_sweeps(insider_hip_handle *h, int32_t *out)
{
    if (!h || !out) return fail(INSIDER_ERR_ARG, "null");
    if (!h->ws.sweeps) return fail(INSIDER_ERR_ARG, "no column update has run yet");
    HIPCHECK(hipSetDevice(h->ds->device));
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    HIPCHECK(hipMemcpy(out, h->ws.sweeps, (size_t)h->ds->p * sizeof(int), hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

int insider_hip_get_info(insider_hip_handle *h, const char *name, double *out)
{
    if (!h || !name || !out) return fail(INSIDER_ERR_ARG, "null");
    const std::string s(name);
    const int NB = h->ws.NB;
    // (the path keys answer for the options as they stand now: a fresh plan, not the last call's)
    if (s == "col_stats_path") *out = build_plan(plan_facts(h, h->ws.K), 1).col_path;
    else if (s == "row_merged") *out = build_plan(plan_facts(h, h->ws.K), 1).merged ? 1.0 : 0.0;
    else if (s == "col_entries") *out = (double)h->ds->col_entries;      // padded held-out list entries, column side
    else if (s == "row_entries") *out = (double)h->ds->row_entries;
    else if (s == "data_bytes_shared") *out = (double)h->ds->bytes_shared;   // device bytes of the data set held jointly with its source (0: a created one) ...
    else if (s == "data_bytes_own") *out = (double)h->ds->bytes_own;         // ... and allocated by the data set itself
    else if (s == "stat_doubles") *out = NB ? NB * (NB + 1) / 2 * 256.0 : 0.0;
    else if (s == "kp") *out = h->ws.KP;
    else if (s == "pair_count_bytes_per_gene") *out = h->ds->cf_pair_ok ? h->ds->cf.cnt_stride : 0.0;
    else if (s == "lists_bytes") *out = 12.0 * ((double)h->ds->col_entries + (double)h->ds->row_entries);
    else if (s == "cap_hits") *out = h->cap_hits;                   // last optimize() / optimize_col(): solves ended by max_sweeps
    else if (s == "max_gene_sweeps") *out = h->max_gene_sweeps;     // ... and the longest solve, in sweeps
    else if (s == "max_sweeps") *out = h->opt.max_sweeps;
    else if (s == "col_solver") *out = h->col_solver;               // last column solve: the kernel that ran it (ColSolver) ...
    else if (s == "col_eval") *out = h->col_eval;                   // ... and the one that ran its evaluation pass (0 = none)
    else if (s == "col_ridge_fallback") *out = h->col_ridge_fallback;   // ... and whether the ridge solve launched the general route
    else if (s == "col_stats_kernel") *out = h->col_stats_kernel;   // last column-side statistics: the kernel (ColStatsKernel) ...
    else if (s == "col_stats_tickets") *out = h->col_stats_tickets; // ... k_col_paircnt4's ticket counters (1 or 16; 0: another kernel)
    else if (s == "col_stats_blocks") *out = h->col_stats_blocks;   // ... and its grid size (0: another kernel)
    else if (s == "col_stats_own_q") *out = h->col_stats_own_q;     // ... and whether it formed Q = S A and Qheld = S^held A itself (option "stats_own_q")
    else if (s == "col_q_kernel") *out = h->col_q_kernel;           // last Q = S A product: 0 = none yet, 1 = k_mm_rows, 2 = k_mm_rows2
    else if (s == "mm_rows2_tiles") *out = h->mm_rows2_tiles;       // tiles per wave of the last k_mm_rows2 launch (Q or V), 0 = none yet
    else if (s == "n_simd") *out = h->ds->n_simd;
    else if (s == "row_kernels") *out = (double)h->row_kernels;     // last optimize() / optimize_row(): row-phase kernel forms (RowKernel bits)
    else if (s == "cd_ms_steady") *out = h->steady_cd_ms;           // option "profile": mean over outer iterations >= 5 of the last call
    else if (s == "col_stats_ms_steady") *out = h->steady_col_ms;
    else if (s == "ol_path") *out = h->ol_path;                     // last outlier call: 1 = level tables in LDS, 2 = read from global
    else if (s == "vd_path") *out = h->vd_path;                     // last variance decomposition: 1 = level tables in LDS, 2 = read from global
    else if (s == "sd_path") *out = h->sd_path;                     // last sample decomposition: 1 = level tables in LDS, 2 = read from global
    else if (s == "ls_path") *out = h->ls_path;                     // last level scores: 1 = one level window (X read once), 2 = several
    else if (s == "ls_slabs") *out = h->ls_slabs;                   // ... and its gene slabs
    else if (s == "sd_slabs") *out = h->sd_slabs;                   // ... and its gene slabs
    else if (s == "glm_slabs") *out = h->glm_slabs;                 // gene slabs of the last interaction GLM's k_resid_stats
    else if (s == "glm_form") *out = h->glm_form;                   // ... and its form, 10 NB + GT (18, 24, 32, 42)
    else if (s == "ls_form") *out = h->ls_form;                     // last level scores: k_ls_prod<QT,KS> as 10 QT + KS (QT 1 or 8)
    else if (s == "fd_form") *out = h->fd_form;                     // last factor decomposition: k_fd_prod<QT,KS,true> as 10 QT + KS (QT 8)
    else if (s == "rc_form") *out = h->rc_form;                     // last residual products: k_rc_back / k_rc_fwd<QT,KS> as 10 QT + KS
    else if (s == "cx_form") *out = h->cx_form;                     // last co-expression call: k_cx_stage<KS> as KS
    else if (s == "rc_slabs") *out = h->rc_slabs;                   // last residual products: the gene slabs of k_rc_fwd (0 = no forward pass)
    else if (s == "cx_stage_mb") *out = h->cx_stage_mb;             // last co-expression call: the staged megabytes,
    else if (s == "cx_stage_ms") *out = h->cx_stage_ms;             // ... the HIP-event time of its staging kernels (k_cx_stage, k_cx_norm)
    else if (s == "cx_ms") *out = h->cx_ms;                         // ... and of its product kernel (k_cx_topk)
    else if (s == "cx_pc_ms") *out = h->cx_pc_ms;                   // last pairwise co-expression call: k_cx_topk_pc
    else if (s == "rc_ms") *out = h->rc_ms;                         // ... and the HIP-event time of its kernels (k_rc_back, k_rc_fwd, k_rc_reduce)
    else if (s == "fd_path") *out = h->fd_path;                     // last factor decomposition: 1 = one column window (X read once), 2 = several
    else if (s == "col_mfma_per_gene") {
        // v_mfma_f64_16x16x4_f64 instructions the column-side statistics kernel issues per gene (2048 flops each; the 4x4x4 form
        // of the per-entry kernel is counted in the same unit: a quarter per instruction)
        if (!NB) return fail(INSIDER_ERR_ARG, "no workspace yet: run an update first");
        const FitPlan fresh = build_plan(plan_facts(h, h->ws.K), 1);
        const int path = fresh.col_path;
        double v = 0.0;
        if (path == 0) {
            const int NT = (h->ws.K + 4) / 4;
            if (fresh.list4)   // k_list_stats4: NT (NT + 1) / 2 instructions of 512 flops per 16 entries
                v = (double)h->ds->col_entries / (double)std::max<int64_t>(h->ds->p, 1) / 16.0 * (NT * (NT + 1) / 2) / 4.0;
            else
                v = (double)h->ds->col_entries / (double)std::max<int64_t>(h->ds->p, 1) / 4.0 * (NB * (NB + 1) / 2);
        } else
            for (int t = 0; t < h->ds->cf.c; ++t) {
                v += std::ceil(h->ds->cf.L[t] / 4.0) * NB * NB;                                           // M += A' P
                if (path == 2 && h->ds->cf.nlater[t] > 0) v += std::ceil(h->ds->cf.L[t] / 16.0) * h->ds->cf.nsteps * NB;   // P = N_j Tab
                if (path == 2 && h->ds->m > 0) v += std::ceil(h->ds->cf.L[t] / 16.0) * NB;                            // + real-valued counts
            }
        if (path == 2 && h->ds->m > 0) v += std::ceil(h->ds->m / 4.0) * NB * NB + NB;                                 // the continuous position
        *out = v;
    } else if (s.rfind("ds_bytes:", 0) == 0) {
        // size in bytes of a data-set array (insider_hip_get_array "ds:<name>"); 0: this data set did not build it
        const std::string a = s.substr(9);
        DsView v;
        if (a == "cf_geometry") *out = (double)(DS_GEOMETRY_INTS * sizeof(int32_t));
        else if (a == "names") *out = (double)ds_name_list().size();
        else if (ds_lookup(*h->ds, a, v)) *out = v.p ? (double)v.bytes : 0.0;
        else return fail(INSIDER_ERR_ARG, "unknown data-set array " + a);
    } else if (ds_info(*h->ds, s, out)) {
    } else return fail(INSIDER_ERR_ARG, "unknown info key " + s);
    return INSIDER_OK;
}

int insider_hip_get_array(insider_hip_handle *h, const char *name, void *out, int64_t bytes)
{
    if (!h || !name || !out) return fail(INSIDER_ERR_ARG, "null");
    const std::string s(name);
    const void *src = nullptr;
    int64_t have = 0;
    if (s == "cd_pass_slot") { src = h->ws.cd_pass_slot; have = h->ds->p * (int64_t)sizeof(int); }
    else if (s == "gene_perm") { src = h->ws.gene_perm; have = h->ds->p * (int64_t)sizeof(int); }
    else if (s == "order_table") { src = h->ws.order; have = (int64_t)(h->ws.order_rows + 1) * ORDER_ROW; }   // rows of ORDER_ROW bytes: the last solve's
    else if (s == "ds:cf_geometry" || s == "ds:names") {   // host facts of the data set: nothing to wait for
        const std::vector<int32_t> g = ds_geometry(*h->ds);
        const std::string names = ds_name_list();
        const bool geo = s == "ds:cf_geometry";
        have = geo ? (int64_t)(g.size() * sizeof(int32_t)) : (int64_t)names.size();
        if (bytes < 0 || bytes > have) return fail(INSIDER_ERR_ARG, "array not available or too short");
        std::memcpy(out, geo ? (const void *)g.data() : (const void *)names.data(), (size_t)bytes);
        return INSIDER_OK;
    } else if (s.rfind("ds:", 0) == 0) {
        DsView v;
        if (!ds_lookup(*h->ds, s.substr(3), v)) return fail(INSIDER_ERR_ARG, "unknown data-set array " + s.substr(3));
        if (!v.p) return fail(INSIDER_ERR_ARG, "this data set did not build " + s.substr(3));
        if (bytes < 0) return fail(INSIDER_ERR_ARG, "negative size");
        src = v.p;
        have = (int64_t)v.bytes;
    } else return fail(INSIDER_ERR_ARG, "unknown array " + s);
    if (!src || bytes > have) return fail(INSIDER_ERR_ARG, "array not available or too short");
    HIPCHECK(hipSetDevice(h->ds->device));
    HIPCHECK(hipStreamSynchronize(h->st.stream));
    HIPCHECK(hipMemcpy(out, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return INSIDER_OK;
}

int insider_hip_get_profile(insider_hip_handle *h, double *out12)
{
    if (!h || !out12) return fail(INSIDER_ERR_ARG, "null");
    for (int i = 0; i < 12; ++i) out12[i] = h->prof[i];
    return INSIDER_OK;
}

}  // extern "C"

// =================================================================================================================
// post-hoc interaction GLM (glm_interaction(), R/glm_interaction.R:2-30) on the resident data set: the residual of the
// subtracted covariate blocks and the per-group regression on the column factor (kernels: insider_posthoc.hpp).  Own
// workspace and the handle's main stream only: nothing insider_hip_optimize() reads is written.
// =================================================================================================================
namespace {

int ph_check(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, const int32_t *subtract)
{
    if (!h) return fail(INSIDER_ERR_ARG, "null handle");
    if (!A || !C || !subtract) return fail(INSIDER_ERR_ARG, "null argument");
    if (K < 1 || K > INSIDER_MAX_K) return fail(INSIDER_ERR_UNSUPPORTED, "K must be in 1..63");
    if (inc_continuous != 0 && inc_continuous != 1)
        return fail(INSIDER_ERR_ARG, "The value of prarameter inc_continuous can only be 0 or 1.");
    if (inc_continuous == 1 && h->ds->m == 0)
        return fail(INSIDER_ERR_ARG, "inc_continuous = 1 needs a handle created with ctns_confounder (insider_hip_create_ex)");
    if (inc_continuous == 0 && h->ds->m > 0)
        return fail(INSIDER_ERR_ARG, "this handle carries continuous covariates: pass inc_continuous = 1");
    if (h->world > 1)
        return fail(INSIDER_ERR_UNSUPPORTED, "the post-hoc calls need the whole matrix: not available on a sharded handle "
                                             "(world > 1)");
    for (int b = 0; b < h->ds->c + inc_continuous; ++b)
        if (subtract[b] && !A[b]) return fail(INSIDER_ERR_ARG, "null row factor of a subtracted block");
    return INSIDER_OK;
}

// the checks of a call on the whole fit (every block enters it) over the entries selected by `entries`
int fit_check(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int entries)
{
    if (!h) return fail(INSIDER_ERR_ARG, "null handle");
    const std::vector<int32_t> every((size_t)h->ds->c + 2, 1);
    int rc = ph_check(h, A, C, inc_continuous, K, every.data());
    if (rc) return rc;
    if (entries < 0 || entries > 2) return fail(INSIDER_ERR_ARG, "entries must be 0 (all), 1 (train) or 2 (test)");
    return INSIDER_OK;
}

// the kernels' entry selector: 0 takes every observed entry, else the mask code an entry must carry
int entry_code(int entries) { return entries == 0 ? 0 : entries == 1 ? CODE_TRAIN : CODE_TEST; }

// the continuous columns that enter the fit
int ctns_cols(const DataSet &d, int inc_continuous) { return inc_continuous ? d.m : 0; }

// bytes of dynamic LDS a kernel may stage level tables in: option "vd_stage_kb", at most 60 KiB (beside a kernel's static
// buffers: no launch attribute needed)
double table_lds_budget(const insider_hip_handle *h) { return std::min(std::max(h->opt.vd_stage_kb, 0.0), 60.0) * 1024.0; }

// gene slabs of a streaming pass whose grid is `tiles` sample tiles x slabs: `option` slabs when positive, else eight blocks
// per compute unit (2 n_simd / tiles) and, where one slab's partials take part_bytes > 0, no more than option "ls_part_mb"
// holds; at most 256.  Returns the slabs that hold genes and writes the genes per slab.
int gene_slabs(const insider_hip_handle *h, int option, int tiles, double part_bytes, int64_t *slab_len)
{
    int want = option;
    if (want <= 0) {
        want = cdiv(2 * h->ds->n_simd, tiles);
        if (part_bytes > 0.0) {
            const double cap = std::max(h->opt.ls_part_mb, 0.0) * 1048576.0 / part_bytes;
            want = (int)std::min<double>(want, std::max(cap, 1.0));
        }
    }
    *slab_len = cdiv(h->ds->p, (int64_t)std::max(1, std::min(want, 256)));
    return (int)cdiv(h->ds->p, *slab_len);
}

// the host factors on the device, enqueued on the main stream: the row factors' blocks stacked in PostWs::Ast as SL rows of
// KPW (the rows of a block whose flag in `use` is 0 are zero; use == NULL takes every block) and C as p rows of K in
// PostWs::vin behind the SL rows of K the blocks came through.  Returns C's place through Cd.
int upload_factors(insider_hip_handle *h, double *const *A, const double *C, int K, int KPW, const int32_t *use,
                   const double **Cd)
{
    const DataSet &d = *h->ds;
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    int rc;
    if ((rc = w.vin.grow((size_t)(d.SL + d.p) * K)) || (rc = w.Ast.grow((size_t)d.SL * KPW))) return rc;
    double *vin = w.vin, *Ast = w.Ast;
    if (use) HIPCHECK(hipMemsetAsync(Ast, 0, (size_t)d.SL * KPW * sizeof(double), st));
    for (int b = 0; b < d.blocks(); ++b) {
        if (use && !use[b]) continue;
        const DataSet::Block blk = d.block(b);
        HIPCHECK(hipMemcpyAsync(vin + (size_t)blk.off * K, A[b], (size_t)blk.rows * K * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pack_A, dim3(cdiv((int64_t)blk.rows * KPW, 256)), dim3(256), 0, st,
                           (const double *)(vin + (size_t)blk.off * K), blk.rows, K, KPW, Ast + (size_t)blk.off * KPW);
        KCHECK();
    }
    HIPCHECK(hipMemcpyAsync(vin + (size_t)d.SL * K, C, (size_t)d.p * K * sizeof(double), hipMemcpyHostToDevice, st));
    *Cd = vin + (size_t)d.SL * K;
    return INSIDER_OK;
}

// U (n x KPW) = the sum of the subtracted blocks' contributions, and C in the kernels' layout (cp, nz), enqueued on the main
// stream
int ph_prepare(insider_hip_handle *h, double *const *A, const double *C, int K, const int32_t *subtract, int KPW)
{
    const DataSet &d = *h->ds;
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const double *Cd = nullptr;
    int rc;
    if ((rc = upload_factors(h, A, C, K, KPW, subtract, &Cd)) || (rc = w.U.grow((size_t)d.n * KPW)) ||
        (rc = w.cp.grow((size_t)d.p * KPW)) || (rc = w.nz.grow(64)))
        return rc;
    double *U = w.U, *cp = w.cp;
    int *nz = w.nz;
    hipLaunchKernelGGL(k_build_R, dim3(cdiv(d.n * KPW, 256)), dim3(256), 0, st, (const int *)d.lev, (const int *)d.lvl_off_d, d.c,
                       (int)d.n, (const double *)w.Ast, KPW, (const double *)d.Zc, d.m, d.SLcat, U);
    KCHECK();
    HIPCHECK(hipMemsetAsync(nz, 0, 64 * sizeof(int), st));
    hipLaunchKernelGGL(k_ph_pack_c, dim3(cdiv(d.p * KPW, 256)), dim3(256), 0, st, Cd, d.p, K, KPW, cp, nz);
    KCHECK();
    return INSIDER_OK;
}

// the residual and GLM kernels' second constant: genes staged per round, by the number of K tiles
constexpr int ph_gene_tiles(int kt) { return kt == 1 ? 8 : kt == 2 ? 4 : 2; }

int residual_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                  const int32_t *subtract, int64_t row_begin, int64_t row_end, double *out)
{
    int rc = ph_check(h, A, C, inc_continuous, K, subtract);
    if (rc) return rc;
    if (row_begin < 0 || row_end > h->ds->n || row_begin > row_end)
        return fail(INSIDER_ERR_ARG, "rows must satisfy 0 <= row_begin <= row_end <= n");
    const int64_t nrows = row_end - row_begin;
    if (nrows == 0) return INSIDER_OK;
    if (!out) return fail(INSIDER_ERR_ARG, "null output");
    HIPCHECK(hipSetDevice(h->ds->device));
    const int NB = (K + 15) / 16, KPW = 16 * NB;
    if ((rc = ph_prepare(h, A, C, K, subtract, KPW))) return rc;
    // gene slabs of the window that fit the stage buffer (multiples of 16 genes, at least one tile)
    const double cap = std::max(h->opt.resid_stage_mb, 0.0) * 1048576.0;
    int64_t gw = (int64_t)(cap / (8.0 * (double)nrows)) / 16 * 16;
    gw = std::max<int64_t>(16, std::min<int64_t>(gw, round_up(h->ds->p, 16)));
    if ((rc = h->post.stage.grow((size_t)nrows * gw))) return rc;
    double *stage = h->post.stage;
    const double *U = h->post.U, *cp = h->post.cp;
    const int row_blocks = cdiv(cdiv(nrows, 16), PH_WPB);
    for (int64_t jb = 0; jb < h->ds->p; jb += gw) {
        const int64_t je = std::min<int64_t>(jb + gw, h->ds->p);
        KT_DISPATCH(NB, {
            constexpr int GT_ = ph_gene_tiles(KT_);
            const size_t lds = (size_t)GT_ * 4 * KT_ * 64 * sizeof(double);
            hipLaunchKernelGGL((k_resid_write<KT_, GT_>), dim3(row_blocks, cdiv(je - jb, 16 * GT_)), dim3(64 * PH_WPB), lds,
                               h->st.stream, (const double *)h->ds->X, h->ds->ldn, row_begin, row_end, U, cp, K, jb, je, stage, nrows);
        });
        KCHECK();
        HIPCHECK(hipMemcpyAsync(out + jb * nrows, stage, (size_t)nrows * (je - jb) * sizeof(double), hipMemcpyDeviceToHost,
                                h->st.stream));
        HIPCHECK(hipStreamSynchronize(h->st.stream));
    }
    return INSIDER_OK;
}

int interaction_glm_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                         const int32_t *subtract, const int32_t *group, int G, double *coeff, double *se, double *dof)
{
    int rc = ph_check(h, A, C, inc_continuous, K, subtract);
    if (rc) return rc;
    if (!group || !coeff || !se || !dof) return fail(INSIDER_ERR_ARG, "null argument");
    if (G < 1) return fail(INSIDER_ERR_ARG, "G must be positive");
    const int64_t n = h->ds->n, p = h->ds->p;
    // group tables on the host: members by group (sample order inside a group), chunks of <= PH_CHUNK members
    std::vector<int> cnt((size_t)G + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t gi = group[i];
        if (gi < 0 || gi > G) return fail(INSIDER_ERR_ARG, "group ids must be within 0..G");
        cnt[gi]++;
    }
    std::vector<int> gptr((size_t)G + 1, 0);   // members of group id g + 1 (id 0 is no group)
    for (int g = 0; g < G; ++g) gptr[g + 1] = gptr[g] + cnt[g + 1];
    const int nmem = gptr[G];
    std::vector<int> members(std::max(nmem, 1)), fill(gptr.begin(), gptr.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        if (group[i] > 0) members[fill[group[i] - 1]++] = (int)i;
    std::vector<int> ch_begin, ch_end, grp_chunk((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) {
        grp_chunk[g] = (int)ch_begin.size();
        for (int b = gptr[g]; b < gptr[g + 1]; b += PH_CHUNK) {
            ch_begin.push_back(b);
            ch_end.push_back(std::min(b + PH_CHUNK, gptr[g + 1]));
        }
    }
    grp_chunk[G] = (int)ch_begin.size();
    const int nchunks = grp_chunk[G];
    HIPCHECK(hipSetDevice(h->ds->device));
    const int NB = (K + 15) / 16, KPW = 16 * NB, ldw = K + 1;
    if ((rc = ph_prepare(h, A, C, K, subtract, KPW))) return rc;
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    // ---- one pass over X: per-sample w = C r and ss = ||r||^2, gene slabs summed in slab order ----------------------
    const int ntiles = cdiv(n, 16), row_blocks = cdiv(ntiles, PH_WPB);
    int64_t slab_len = 0;
    int slabs = 1;
    KT_DISPATCH(NB, {
        constexpr int GT_ = ph_gene_tiles(KT_);
        // enough blocks for every SIMD of the device several times over (or option "glm_slabs"), slabs of whole staging
        // rounds
        const int want = h->opt.glm_slabs > 0
                             ? h->opt.glm_slabs
                             : std::max(1, std::min(64, cdiv(4 * h->ds->n_simd, (int64_t)row_blocks * PH_WPB)));
        slab_len = round_up(cdiv(p, want), 16 * GT_);
        slabs = cdiv(p, slab_len);
        h->glm_form = 10 * KT_ + GT_;
    });
    h->glm_slabs = slabs;
    if ((rc = w.part.grow((size_t)slabs * n * ldw)) || (rc = w.stats.grow((size_t)n * ldw))) return rc;
    double *part = w.part, *stats = w.stats;
    const double *U = w.U, *cp = w.cp;
    KT_DISPATCH(NB, {
        constexpr int GT_ = ph_gene_tiles(KT_);
        const size_t lds = (size_t)2 * GT_ * 4 * KT_ * 64 * sizeof(double);
        hipLaunchKernelGGL((k_resid_stats<KT_, GT_>), dim3(row_blocks, slabs), dim3(64 * PH_WPB), lds, st,
                           (const double *)h->ds->X, h->ds->ldn, (int)n, p, U, cp, K, slab_len, part);
    });
    KCHECK();
    hipLaunchKernelGGL(k_sum_partials, dim3(cdiv(n * ldw, 16)), dim3(256), 0, st, (const double *)part, slabs,
                       (int)(n * ldw), stats);
    KCHECK();
    // ---- per-group sums -----------------------------------------------------------------------------------------------
    const size_t n_ints = (size_t)(G + 1) + members.size() + 2 * std::max(nchunks, 1) + (size_t)(G + 1);
    if ((rc = w.ints.grow(n_ints))) return rc;
    int *ints = w.ints;
    int *d_gptr = ints, *d_mem = d_gptr + (G + 1), *d_cb = d_mem + members.size(), *d_ce = d_cb + std::max(nchunks, 1),
        *d_gc = d_ce + std::max(nchunks, 1);
    std::vector<int> packed;
    packed.reserve(n_ints);
    packed.insert(packed.end(), gptr.begin(), gptr.end());
    packed.insert(packed.end(), members.begin(), members.end());
    ch_begin.resize(std::max(nchunks, 1), 0);
    ch_end.resize(std::max(nchunks, 1), 0);
    packed.insert(packed.end(), ch_begin.begin(), ch_begin.end());
    packed.insert(packed.end(), ch_end.begin(), ch_end.end());
    packed.insert(packed.end(), grp_chunk.begin(), grp_chunk.end());
    HIPCHECK(hipMemcpyAsync(ints, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if ((rc = w.cpart.grow((size_t)std::max(nchunks, 1) * ldw)) || (rc = w.gsum.grow((size_t)G * ldw))) return rc;
    double *cpart = w.cpart, *gsum = w.gsum;
    if (nchunks > 0) {
        hipLaunchKernelGGL(k_ph_chunk_sums, dim3(cdiv(nchunks, 4)), dim3(256), 0, st, (const double *)stats, ldw,
                           (const int *)d_mem, (const int *)d_cb, (const int *)d_ce, nchunks, cpart);
        KCHECK();
    }
    hipLaunchKernelGGL(k_ph_group_sums, dim3(G), dim3(256), 0, st, (const double *)cpart, ldw, (const int *)d_gc, gsum);
    KCHECK();
    // ---- G = C C', its reduced Cholesky factor, and every group's coefficients ------------------------------------------
    const int gslabs = cdiv(p, MM_SLAB);
    if ((rc = w.gpart.grow((size_t)gslabs * K * K)) || (rc = w.gram.grow((size_t)K * K)) || (rc = w.L.grow((size_t)64 * 64)) ||
        (rc = w.dinv.grow(64)) || (rc = w.info.grow(2 + 64)) || (rc = w.outs.grow((size_t)2 * G * K + G)))
        return rc;
    double *gpart = w.gpart, *gram = w.gram, *L = w.L, *dinv = w.dinv, *outs = w.outs;
    int *info = w.info;
    KT_DISPATCH(NB, hipLaunchKernelGGL((k_mm_reduce<KT_>), dim3(gslabs, cdiv(K, 16)), dim3(64), 0, st, cp, (int64_t)KPW, cp,
                                       (int64_t)KPW, (int)p, MM_SLAB, K, K, gpart, K));
    KCHECK();
    hipLaunchKernelGGL(k_sum_partials, dim3(cdiv(K * K, 16)), dim3(256), 0, st, (const double *)gpart, gslabs, K * K, gram);
    KCHECK();
    hipLaunchKernelGGL(k_glm_factor, dim3(1), dim3(64), 0, st, (const double *)gram, (const int *)w.nz, K, L, dinv, info);
    KCHECK();
    double *d_coeff = outs, *d_se = outs + (size_t)G * K, *d_dof = outs + (size_t)2 * G * K;
    hipLaunchKernelGGL(k_glm_groups, dim3(G), dim3(64), 0, st, (const double *)gsum, ldw, (const int *)d_gptr, K, p,
                       (const int *)w.nz, (const double *)L, (const double *)dinv, (const int *)info, G, d_coeff, d_se,
                       d_dof);
    KCHECK();
    int hinfo[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(hinfo, info, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    // more non-zero rows than genes: C C' is rank-deficient whatever rounding leaves in its last pivots
    if (!hinfo[0] && hinfo[1] > p)
        return fail(INSIDER_ERR_SOLVE, "insider_hip_interaction_glm: the column factor has " + std::to_string(hinfo[1]) +
                                       " non-zero rows over " + std::to_string(p) + " genes: C C' is rank-deficient");
    if (hinfo[0])
        return fail(INSIDER_ERR_SOLVE, "insider_hip_interaction_glm: C C' restricted to the non-zero rows of C is singular to "
                                       "working precision (pivot " + std::to_string(hinfo[0]) + " of " +
                                       std::to_string(hinfo[1]) + "): the column factor has linearly dependent rows");
    HIPCHECK(hipMemcpyAsync(coeff, d_coeff, (size_t)G * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(se, d_se, (size_t)G * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(dof, d_dof, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// a failed call may leave work enqueued: drain the stream so that the next call starts clean
int ph_finish(insider_hip_handle *h, int rc)
{
    if (rc != INSIDER_OK && h && h->st.stream) {
        const std::string keep = g_err;
        (void)hipSetDevice(h->ds->device);
        (void)hipStreamSynchronize(h->st.stream);
        g_err = keep;
    }
    return rc;
}

// ---- variance / sample decomposition (kernels: insider_vardecomp.hpp, insider_sampdecomp.hpp) -------------------------
// the level table T = [A_stack; B_c] C of every block, gene-major (T[j][0..SL)), enqueued on the main stream into
// PostWs::vtab
int vd_build_table(insider_hip_handle *h, double *const *A, const double *C, int K)
{
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const int SL = h->ds->SL, KPW = 16 * ((K + 15) / 16);
    const int64_t p = h->ds->p;
    const double *Cd = nullptr;
    int rc;
    if ((rc = upload_factors(h, A, C, K, KPW, nullptr, &Cd)) || (rc = w.vtab.grow((size_t)p * SL))) return rc;
    const double *Ast = w.Ast;
    double *T = w.vtab;
    // T[j][s] = sum_k Ast[s][k] C[k][j]: gene-major, one gene's table contiguous
#define VT_LAUNCH(NT_)                                                                                                      \
    hipLaunchKernelGGL((k_mm_rows<NT_, true>), dim3(cdiv(cdiv((int)p, 16), 4), cdiv(SL, 16 * NT_)), dim3(256), 0, st,         \
                       Cd, (int64_t)K, (int)p, K, Ast, KPW, SL, T, (int64_t)SL, SL)
    if (SL <= 16) VT_LAUNCH(1);
    else if (SL <= 32) VT_LAUNCH(2);
    else VT_LAUNCH(4);
#undef VT_LAUNCH
    KCHECK();
    return INSIDER_OK;
}

int variance_decomposition_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                int entries, double *out)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (!out) return fail(INSIDER_ERR_ARG, "null output");
    HIPCHECK(hipSetDevice(h->ds->device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const int nb = h->ds->c + inc_continuous, SL = h->ds->SL, rec = 4 + 3 * nb;
    const int64_t n = h->ds->n, p = h->ds->p;
    if ((rc = vd_build_table(h, A, C, K)) || (rc = w.vrec.grow((size_t)p * rec))) return rc;
    double *T = w.vtab, *R = w.vrec;
    // one pass over X per window of BW blocks
    const int sel = entry_code(entries), m = ctns_cols(*h->ds, inc_continuous);
    const double budget = table_lds_budget(h);
#define VD_LAUNCH(BW_, GW_)                                                                                                 \
    do {                                                                                                                     \
        const bool staged = (double)GW_ * SL * sizeof(double) <= budget;                                                     \
        h->vd_path = staged ? 1 : 2;                                                                                         \
        for (int b0 = 0; b0 < nb; b0 += BW_) {                                                                               \
            if (staged)                                                                                                      \
                hipLaunchKernelGGL((k_vd_stats<BW_, GW_, true>), dim3(cdiv(p, GW_)), dim3(64 * VD_WAVES),                    \
                                   (size_t)GW_ * SL * sizeof(double), st, (const double *)h->ds->X, (const uint8_t *)h->ds->codes,   \
                                   h->ds->ldn, (int)n, p, (const int *)h->ds->lev, (const int *)h->ds->lvl_off_d, h->ds->c,                  \
                                   (const double *)h->ds->Zc, m, h->ds->SLcat, (const double *)T, SL, sel, nb, b0, R);               \
            else                                                                                                             \
                hipLaunchKernelGGL((k_vd_stats<BW_, GW_, false>), dim3(cdiv(p, GW_)), dim3(64 * VD_WAVES), 0, st,            \
                                   (const double *)h->ds->X, (const uint8_t *)h->ds->codes, h->ds->ldn, (int)n, p, (const int *)h->ds->lev,  \
                                   (const int *)h->ds->lvl_off_d, h->ds->c, (const double *)h->ds->Zc, m, h->ds->SLcat, (const double *)T,   \
                                   SL, sel, nb, b0, R);                                                                      \
            KCHECK();                                                                                                        \
        }                                                                                                                    \
    } while (0)
    // two genes per wave: 126 / 154 / 215 VGPRs for windows of 1 / 2 / 4 blocks (four genes: 227 / 256, fewer waves per SIMD)
    if (nb == 1) VD_LAUNCH(1, 2);
    else if (nb == 2) VD_LAUNCH(2, 2);
    else VD_LAUNCH(4, 2);
#undef VD_LAUNCH
    HIPCHECK(hipMemcpyAsync(out, R, (size_t)p * rec * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// the same record per sample: the level table, then per window of BW blocks one streaming pass over X and the codes whose
// grid is sample tiles x gene slabs (k_sd_stats) and the sum of the slabs' partial records in slab order (k_sd_reduce)
int sample_decomposition_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                              int entries, double *out)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (!out) return fail(INSIDER_ERR_ARG, "null output");
    HIPCHECK(hipSetDevice(h->ds->device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const int nb = h->ds->c + inc_continuous, SL = h->ds->SL, rec = 4 + 3 * nb;
    const int64_t n = h->ds->n, p = h->ds->p;
    // gene slabs: from n, p, the device's compute units and option "sd_slabs" alone (gene_slabs; a block is SD_WAVES waves,
    // three are resident per unit at 130 - 170 registers)
    const int tiles = cdiv(n, SD_TILE);
    int64_t slab_len = 0;
    const int slabs = gene_slabs(h, h->opt.sd_slabs, tiles, 0.0, &slab_len);
    const int BW = nb == 1 ? 1 : nb == 2 ? 2 : 4, RW = 4 + 3 * BW;
    if ((rc = vd_build_table(h, A, C, K)) || (rc = w.spart.grow((size_t)slabs * n * RW)) ||
        (rc = w.srec.grow((size_t)n * rec)))
        return rc;
    double *T = w.vtab, *part = w.spart, *R = w.srec;
    const int sel = entry_code(entries), m = ctns_cols(*h->ds, inc_continuous);
    // tables staged in groups of whole load steps of SD_GU genes, as many as table_lds_budget holds; when not even one step's
    // tables fit: the global form
    const double budget = table_lds_budget(h);
    const int fit = (int)std::min<double>(budget / ((double)SL * sizeof(double)), SD_GROUP_MAX) / SD_GU * SD_GU;
    const bool staged = fit >= SD_GU;
    const int gg = staged ? fit : (int)std::min<int64_t>(slab_len, INT32_MAX);
    h->sd_path = staged ? 1 : 2;
    h->sd_slabs = slabs;
#define SD_LAUNCH(BW_)                                                                                                      \
    for (int b0 = 0; b0 < nb; b0 += BW_) {                                                                                   \
        if (staged)                                                                                                          \
            hipLaunchKernelGGL((k_sd_stats<BW_, true>), dim3(tiles, slabs), dim3(64 * SD_WAVES),                             \
                               (size_t)gg * SL * sizeof(double), st, (const double *)h->ds->X, (const uint8_t *)h->ds->codes, \
                               h->ds->ldn, (int)n, p, (const int *)h->ds->lev, (const int *)h->ds->lvl_off_d, h->ds->c,      \
                               (const double *)h->ds->Zc, m, h->ds->SLcat, (const double *)T, SL, sel, b0, slab_len, gg, part); \
        else                                                                                                                 \
            hipLaunchKernelGGL((k_sd_stats<BW_, false>), dim3(tiles, slabs), dim3(64 * SD_WAVES), 0, st,                     \
                               (const double *)h->ds->X, (const uint8_t *)h->ds->codes, h->ds->ldn, (int)n, p,               \
                               (const int *)h->ds->lev, (const int *)h->ds->lvl_off_d, h->ds->c, (const double *)h->ds->Zc, m, \
                               h->ds->SLcat, (const double *)T, SL, sel, b0, slab_len, gg, part);                            \
        KCHECK();                                                                                                            \
        hipLaunchKernelGGL(k_sd_reduce, dim3(cdiv(n * RW, 256)), dim3(256), 0, st, (const double *)part, slabs, n, RW, nb,   \
                           b0, R);                                                                                           \
        KCHECK();                                                                                                            \
    }
    if (BW == 1) SD_LAUNCH(1)
    else if (BW == 2) SD_LAUNCH(2)
    else SD_LAUNCH(4)
#undef SD_LAUNCH
    HIPCHECK(hipMemcpyAsync(out, R, (size_t)n * rec * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// ---- level scores (kernels: insider_levelscores.hpp) -------------------------------------------------------------------
// U_{-cov} and C in the kernels' layout (ph_prepare with every block but cov), the candidate table Tc = cand C (k_pack_A +
// k_mm_rows, as vd_build_table builds T), then one streaming pass over X and the codes per window of LS_QT level tiles on a
// grid of sample tiles x gene slabs x windows (k_ls_prod) and the sum of the slabs' partial scores in slab order
// (k_ls_reduce).  cand == NULL scores the rows of A[cov] through the very same path: the same bits as passing them.
int level_scores_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int entries,
                      int cov, const double *cand, int n_cand, double *sse, double *cnt)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (!sse || !cnt) return fail(INSIDER_ERR_ARG, "null output");
    const DataSet &d = *h->ds;
    if (cov < 0 || cov >= d.c) return fail(INSIDER_ERR_ARG, "cov must be a categorical covariate block in 0..c-1");
    if (cand && n_cand < 1) return fail(INSIDER_ERR_ARG, "n_cand must be positive when candidates are given");
    if (!cand && n_cand != 0) return fail(INSIDER_ERR_ARG, "n_cand must be 0 without candidates");
    HIPCHECK(hipSetDevice(d.device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const int KS = (K + 15) / 16, KPW = 16 * KS;
    const int L = cand ? n_cand : d.block(cov).rows;
    const double *E = cand ? cand : A[cov];
    const int64_t n = d.n, p = d.p;
    std::vector<int32_t> sub((size_t)d.c + 2, 1);   // every block but cov enters d
    sub[cov] = 0;
    if ((rc = ph_prepare(h, A, C, K, sub.data(), KPW))) return rc;
    const int ldt = (int)round_up(L, 16), ltiles = ldt / 16, nwin = cdiv(ltiles, LS_QT);
    // gene slabs (gene_slabs, option "ls_slabs"): when automatic, no more than keep the partial scores within "ls_part_mb"
    const int tiles = cdiv(n, LS_TILE);
    int64_t slab_len = 0;
    const int slabs = gene_slabs(h, h->opt.ls_slabs, tiles, (double)n * ldt * sizeof(double), &slab_len);
    if ((rc = w.stage.grow((size_t)L * K)) || (rc = w.lcand.grow((size_t)L * KPW)) || (rc = w.ltab.grow((size_t)p * ldt)) ||
        (rc = w.lpart.grow((size_t)slabs * n * ldt)) || (rc = w.lcnt.grow((size_t)slabs * n)) ||
        (rc = w.lout.grow((size_t)n * L + n)))
        return rc;
    double *tmp = w.stage, *Ec = w.lcand, *Tc = w.ltab, *part = w.lpart, *cpart = w.lcnt, *out = w.lout;
    const double *U = w.U, *cp = w.cp;
    HIPCHECK(hipMemcpyAsync(tmp, E, (size_t)L * K * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pack_A, dim3(cdiv((int64_t)L * KPW, 256)), dim3(256), 0, st, (const double *)tmp, L, K, KPW, Ec);
    KCHECK();
    // Tc[j][l] = sum_k C[k][j] cand[l][k]: gene-major, zero beyond L
#define LT_LAUNCH(NT_)                                                                                                      \
    hipLaunchKernelGGL((k_mm_rows<NT_, true>), dim3(cdiv(cdiv((int)p, 16), 4), cdiv(ldt, 16 * NT_)), dim3(256), 0, st, cp,    \
                       (int64_t)KPW, (int)p, K, (const double *)Ec, KPW, L, Tc, (int64_t)ldt, ldt)
    if (ltiles <= 1) LT_LAUNCH(1);
    else if (ltiles <= 2) LT_LAUNCH(2);
    else LT_LAUNCH(4);
#undef LT_LAUNCH
    KCHECK();
    const int sel = entry_code(entries);
    h->ls_path = nwin == 1 ? 1 : 2;
    h->ls_slabs = slabs;
#define LS_LAUNCH(QT_)                                                                                                      \
    KT_DISPATCH(KS, {                                                                                                        \
        h->ls_form = 10 * QT_ + KT_;                                                                                         \
        hipLaunchKernelGGL((k_ls_prod<QT_, KT_>), dim3(tiles, slabs, cdiv(ltiles, QT_)), dim3(64 * LS_WAVES),                \
                           ls_lds_bytes(QT_, KT_), st, (const double *)d.X, (const uint8_t *)d.codes, d.ldn,                 \
                           (int)n, p, U, cp, K, (const double *)Tc, ldt, sel, slab_len, part, cpart);                        \
    })
    // one level tile: 84 - 102 registers; else the window form of LS_QT tiles: 196 - 215 (tools/kernel_regs.sh), no scratch, two
    // waves per SIMD; tiles beyond the live ones of a window are skipped by a uniform branch.  (Forms of 2 and 4 tiles were
    // dropped: the 4-tile one compiled to 446 - 468 registers, one wave per SIMD.)
    if (ltiles <= 1) { LS_LAUNCH(1) }
    else { LS_LAUNCH(LS_QT) }
#undef LS_LAUNCH
    KCHECK();
    hipLaunchKernelGGL(k_ls_reduce, dim3(cdiv(n * ldt, 256)), dim3(256), 0, st, (const double *)part, (const double *)cpart,
                       slabs, n, ldt, L, out, out + (size_t)n * L);
    KCHECK();
    HIPCHECK(hipStreamSynchronize(st));   // the caller's arrays are written only after the kernels ran
    HIPCHECK(hipMemcpyAsync(sse, out, (size_t)n * L * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(cnt, out + (size_t)n * L, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// ---- factor decomposition (kernels: insider_factdecomp.hpp) ----------------------------------------------------------
// Wall = [W | W .* W] from the packed row factors, then the heavy pass over X and the codes (P1 and the base slots, the
// B K columns of the covariate blocks in windows of FD_QT tiles of 16), the light pass over the codes (P2, P3, every
// column) and k_fd_finish
constexpr int FD_QT = 8;   // tiles of 16 columns per window at most (64 accumulator registers)

int factor_decomposition_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                              int entries, double *out)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (!out) return fail(INSIDER_ERR_ARG, "null output");
    HIPCHECK(hipSetDevice(h->ds->device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const DataSet &d = *h->ds;
    const int nb = d.c + inc_continuous, KPW = 16 * ((K + 15) / 16), KS = KPW / 16;
    const int rec = 4 + 3 * (nb + 1) * K;
    const int64_t n = d.n, p = d.p;
    const int ldq = (int)round_up((int64_t)(nb + 1) * K, 16), ldw = 2 * ldq, ldp = 3 * ldq;
    const int64_t rows = round_up(n, FD_CHUNK);
    const double *Cd = nullptr;
    if ((rc = upload_factors(h, A, C, K, KPW, nullptr, &Cd)) || (rc = w.fwall.grow((size_t)rows * ldw)) ||
        (rc = w.fprod.grow((size_t)p * ldp)) || (rc = w.fbase.grow((size_t)p * 4)) || (rc = w.frec.grow((size_t)p * rec)))
        return rc;
    const double *Ast = w.Ast;
    double *Wall = w.fwall, *P = w.fprod, *base = w.fbase, *R = w.frec;
    const int m = ctns_cols(d, inc_continuous);
    HIPCHECK(hipMemsetAsync(Wall, 0, (size_t)rows * ldw * sizeof(double), st));
    hipLaunchKernelGGL(k_fd_build_w, dim3(cdiv(n * K, 256)), dim3(256), 0, st, (const int *)d.lev, (const int *)d.lvl_off_d, d.c,
                       (int)n, Ast, KPW, (const double *)d.Zc, m, d.SLcat, K, ldq, Wall);
    KCHECK();
    const int sel = entry_code(entries);
    const int heavy_tiles = cdiv(nb * K, 16), light_tiles = ldw / 16;
    h->fd_path = heavy_tiles <= FD_QT ? 1 : 2;
    const dim3 grid((unsigned)cdiv(p, (int64_t)FD_GENES)), block(64 * FD_WAVES);
#define FD_LAUNCH(QT_, KS_)                                                                                                 \
    do {                                                                                                                     \
        h->fd_form = 10 * QT_ + KS_;                                                                                         \
        const size_t lw = (size_t)FD_CHUNK * (16 * QT_ + 4) * sizeof(double);                                                \
        const size_t lr = (size_t)FD_CHUNK * (16 * KS_ + 2) * sizeof(double);                                                \
        for (int t0 = 0; t0 < heavy_tiles; t0 += QT_) {                                                                      \
            hipLaunchKernelGGL((k_fd_prod<QT_, KS_, true>), grid, block, lw + lr, st, (const double *)d.X,                   \
                               (const uint8_t *)d.codes, d.ldn, (int)n, p, (const double *)Wall, ldw, 16 * t0,               \
                               std::min(QT_, heavy_tiles - t0), nb * K, Cd, K, sel, P, ldp, 16 * t0, base);                  \
            KCHECK();                                                                                                        \
        }                                                                                                                    \
        for (int t0 = 0; t0 < light_tiles; t0 += QT_) {                                                                      \
            hipLaunchKernelGGL((k_fd_prod<QT_, 1, false>), grid, block, lw, st, (const double *)d.X,                         \
                               (const uint8_t *)d.codes, d.ldn, (int)n, p, (const double *)Wall, ldw, 16 * t0,               \
                               std::min(QT_, light_tiles - t0), 0, Cd, K, sel, P, ldp, ldq + 16 * t0,                        \
                               (double *)nullptr);                                                                           \
            KCHECK();                                                                                                        \
        }                                                                                                                    \
    } while (0)
    // one window width for every shape: the form with 8 tiles needs 132 - 157 registers (three blocks per compute unit); tiles
    // beyond the live ones of a window are skipped by a uniform branch
    KT_DISPATCH(KS, FD_LAUNCH(FD_QT, KT_));
#undef FD_LAUNCH
    hipLaunchKernelGGL(k_fd_finish, dim3(cdiv(p * K, 256)), dim3(256), 0, st, (const double *)P, ldq, (const double *)base,
                       Cd, p, K, nb, R);
    KCHECK();
    HIPCHECK(hipMemcpyAsync(out, R, (size_t)p * rec * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// ---- residual products (kernels: insider_rescomp.hpp) ----------------------------------------------------------------
// U and C in the kernels' layout (ph_prepare with every block), Q packed to rows of ldq, the pairs (centre, inverse scale),
// then k_rc_back (Z = R' Q and rss: one streaming pass over X and the codes, a block per 64 genes) and, when Y is wanted,
// k_rc_fwd on a grid of sample tiles x gene slabs and k_rc_reduce (the slabs' partial Y summed in slab order).  Nothing is
// written to the caller's arrays before every check passed and the kernels ran.
int residual_products_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int entries,
                           const double *center, const double *scale, const double *Q, int q, double *Z, double *Y,
                           double *rss)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (!Q || !Z) return fail(INSIDER_ERR_ARG, "null Q or Z");
    if (q < 1 || q > 64) return fail(INSIDER_ERR_ARG, "q must be in 1..64");
    const DataSet &d = *h->ds;
    const int64_t n = d.n, p = d.p;
    for (int64_t e = 0; e < n * q; ++e)
        if (!std::isfinite(Q[e])) return fail(INSIDER_ERR_ARG, "Q holds a value that is not finite");
    HIPCHECK(hipSetDevice(d.device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const int KS = (K + 15) / 16, KPW = 16 * KS;
    const std::vector<int32_t> every((size_t)d.c + 2, 1);   // every block enters the fit
    if ((rc = ph_prepare(h, A, C, K, every.data(), KPW))) return rc;
    const int QT = (q + 15) / 16, ldq = 16 * QT;
    // gene slabs of the forward pass (gene_slabs, option "rc_slabs"): when automatic, no more than keep the partial Y within
    // "ls_part_mb"
    const int tiles = cdiv(n, RC_TILE);
    int64_t slab_len = 0;
    const int slabs = Y ? gene_slabs(h, h->opt.rc_slabs, tiles, (double)n * ldq * sizeof(double), &slab_len) : 0;
    const size_t n_in = (size_t)n * q + 2 * (size_t)p, n_out = (size_t)p * q + (size_t)n * q + (size_t)p;
    if ((rc = w.rin.grow(n_in)) || (rc = w.rq.grow((size_t)n * ldq)) || (rc = w.rcs.grow((size_t)2 * p)) ||
        (rc = w.rz.grow((size_t)p * ldq)) || (rc = w.rpart.grow((size_t)std::max(slabs, 1) * n * ldq)) ||
        (rc = w.rout.grow(n_out)))
        return rc;
    double *q_in = w.rin, *c_in = q_in + (size_t)n * q, *s_in = c_in + p;
    double *Qd = w.rq, *cs = w.rcs, *Zd = w.rz, *part = w.rpart;
    double *z_out = w.rout, *y_out = z_out + (size_t)p * q, *r_out = y_out + (size_t)n * q;
    const double *U = w.U, *cp = w.cp;
    HIPCHECK(hipMemcpyAsync(q_in, Q, (size_t)n * q * sizeof(double), hipMemcpyHostToDevice, st));
    if (center) HIPCHECK(hipMemcpyAsync(c_in, center, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    if (scale) HIPCHECK(hipMemcpyAsync(s_in, scale, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rc_pack_q, dim3(cdiv(n * ldq, 256)), dim3(256), 0, st, (const double *)q_in, n, q, ldq, Qd);
    KCHECK();
    hipLaunchKernelGGL(k_rc_center_scale, dim3(cdiv(p, 256)), dim3(256), 0, st, (const double *)(center ? c_in : nullptr),
                       (const double *)(scale ? s_in : nullptr), p, cs);
    KCHECK();
    const int sel = entry_code(entries);
    Stopwatch watch;
    if ((rc = watch.start(st))) return rc;
#define RC_LAUNCH(QT_, KS_)                                                                                                 \
    do {                                                                                                                     \
        h->rc_form = 10 * QT_ + KS_;                                                                                         \
        hipLaunchKernelGGL((k_rc_back<QT_, KS_>), dim3((unsigned)cdiv(p, (int64_t)RC_GENES)), dim3(64 * RC_WAVES),           \
                           rc_back_lds(QT_, KS_), st, (const double *)d.X, (const uint8_t *)d.codes, d.ldn, (int)n, p, U, cp, \
                           K, (const double *)Qd, (const double *)cs, sel, Zd, r_out);                                       \
        KCHECK();                                                                                                            \
        if (Y) {                                                                                                             \
            hipLaunchKernelGGL((k_rc_fwd<QT_, KS_>), dim3(tiles, slabs), dim3(64 * RC_WAVES), rc_fwd_lds(QT_, KS_), st,      \
                               (const double *)d.X, (const uint8_t *)d.codes, d.ldn, (int)n, p, U, cp, K, (const double *)Zd, \
                               (const double *)cs, sel, slab_len, part);                                                     \
            KCHECK();                                                                                                        \
        }                                                                                                                    \
    } while (0)
    // one form per number of column tiles of Q and of K: registers per form in DESIGN (tools/kernel_regs.sh), no scratch
    switch (QT) {
        case 1: KT_DISPATCH(KS, RC_LAUNCH(1, KT_)) break;
        case 2: KT_DISPATCH(KS, RC_LAUNCH(2, KT_)) break;
        case 3: KT_DISPATCH(KS, RC_LAUNCH(3, KT_)) break;
        default: KT_DISPATCH(KS, RC_LAUNCH(4, KT_)) break;
    }
#undef RC_LAUNCH
    if (Y) {
        hipLaunchKernelGGL(k_rc_reduce, dim3(cdiv(n * ldq, 256)), dim3(256), 0, st, (const double *)part, slabs, n, ldq, q, y_out);
        KCHECK();
    }
    if ((rc = watch.mark(st))) return rc;
    hipLaunchKernelGGL(k_rc_unpack, dim3(cdiv(p * q, 256)), dim3(256), 0, st, (const double *)Zd, p, q, ldq, z_out);
    KCHECK();
    HIPCHECK(hipStreamSynchronize(st));   // the caller's arrays are written only after the kernels ran
    float ms = 0.f;
    if ((rc = watch.stop_ms(st, &ms))) return rc;
    h->rc_ms = ms;
    h->rc_slabs = slabs;
    HIPCHECK(hipMemcpyAsync(Z, z_out, (size_t)p * q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (Y) HIPCHECK(hipMemcpyAsync(Y, y_out, (size_t)n * q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (rss) HIPCHECK(hipMemcpyAsync(rss, r_out, (size_t)p * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// ---- co-expression (kernels: insider_coexpr.hpp) -----------------------------------------------------------------------
// U and C in the kernels' layout (ph_prepare with every block) and the pairs (centre, inverse scale) of the residual products;
// the standardised residual staged once in operand order for the axis (k_cx_stage: one pass over X and the codes; k_cx_norm:
// one over the staged buffer), in a buffer of this call alone; then the deep product with the fused selection.  Nothing is
// written to the caller's arrays before every check passed and the kernels ran.  pairwise: the pairwise-complete form
// (insider_coexpr_pc.hpp: k_cx_std_pc keeps the unselected entries NaN, k_cx_topk_pc forms the six sums) with min_overlap and
// overlap_out; otherwise neither is looked at.
int coexpression_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int entries,
                      const double *center, const double *scale, int axis, int k, int32_t *idx_out, double *score_out,
                      bool pairwise = false, int64_t min_overlap = 0, int32_t *overlap_out = nullptr)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (axis != 0 && axis != 1) return fail(INSIDER_ERR_ARG, "axis must be 0 (genes) or 1 (samples)");
    if (k < 1 || k > NN_MAX_TOPK) return fail(INSIDER_ERR_ARG, "k must be in 1..64");
    if (!idx_out || !score_out || (pairwise && !overlap_out)) return fail(INSIDER_ERR_ARG, "null output");
    if (pairwise && min_overlap < 3) return fail(INSIDER_ERR_ARG, "min_overlap must be >= 3");
    const DataSet &d = *h->ds;
    const int64_t n = d.n, p = d.p;
    const int64_t N = axis == 0 ? p : n, depth = axis == 0 ? n : p;
    HIPCHECK(hipSetDevice(d.device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const int KS = (K + 15) / 16, KPW = 16 * KS;
    const std::vector<int32_t> every((size_t)d.c + 2, 1);   // every block enters the fit
    if ((rc = ph_prepare(h, A, C, K, every.data(), KPW))) return rc;
    const int64_t npad = round_up(N, CX_PAD), Dpad = round_up(depth, CX_DC);
    DevBuf<double> stage, dscore;
    DevBuf<int> dalive;
    DevBuf<int32_t> didx, dover;
    if ((rc = w.rin.grow(2 * (size_t)p)) || (rc = w.rcs.grow((size_t)2 * p)) || (rc = stage.alloc((size_t)npad * Dpad)) ||
        (rc = dalive.alloc((size_t)npad)) || (rc = dscore.alloc((size_t)N * k)) || (rc = didx.alloc((size_t)N * k)) ||
        (pairwise && (rc = dover.alloc((size_t)N * k))))
        return rc;
    double *c_in = w.rin, *s_in = c_in + p, *cs = w.rcs;
    const double *U = w.U, *cp = w.cp;
    if (center) HIPCHECK(hipMemcpyAsync(c_in, center, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    if (scale) HIPCHECK(hipMemcpyAsync(s_in, scale, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rc_center_scale, dim3(cdiv(p, 256)), dim3(256), 0, st, (const double *)(center ? c_in : nullptr),
                       (const double *)(scale ? s_in : nullptr), p, cs);
    KCHECK();
    HIPCHECK(hipMemsetAsync(stage, 0, (size_t)npad * Dpad * sizeof(double), st));
    // sample tiles x gene slabs of whole fit tiles, eight blocks per compute unit
    const int tiles = cdiv(n, RC_TILE);
    int64_t slab_len = 0;
    (void)gene_slabs(h, 0, tiles, 0.0, &slab_len);
    slab_len = round_up(slab_len, 16);
    const int slabs = cdiv(p, slab_len);
    const int sel = entry_code(entries);
    Stopwatch stage_watch, watch;
    if ((rc = stage_watch.start(st))) return rc;
    KT_DISPATCH(KS, {
        h->cx_form = KT_;
        hipLaunchKernelGGL((k_cx_stage<KT_>), dim3(tiles, slabs), dim3(64 * RC_WAVES), (size_t)4 * KT_ * 64 * sizeof(double),
                           st, (const double *)d.X, (const uint8_t *)d.codes, d.ldn, (int)n, p, U, cp, K,
                           (const double *)cs, sel, slab_len, axis, Dpad, stage.get());
    });
    KCHECK();
    if (pairwise)
        hipLaunchKernelGGL(k_cx_std_pc, dim3(cdiv(npad, 64)), dim3(64), 0, st, (const double *)nullptr, depth, N, npad, Dpad,
                           stage.get(), dalive.get());
    else
        hipLaunchKernelGGL(k_cx_norm, dim3(cdiv(npad, 64)), dim3(64), 0, st, stage.get(), depth, N, npad, Dpad, dalive.get());
    KCHECK();
    if ((rc = stage_watch.mark(st)) || (rc = watch.start(st))) return rc;
    if ((rc = pairwise ? launch_cx_topk_pc(stage, dalive, npad, Dpad, depth, min_overlap, k, 0, N, didx, dscore, dover, st)
                       : launch_cx_topk(stage, dalive, npad, Dpad, k, 0, N, didx, dscore, st)))
        return rc;
    if ((rc = watch.mark(st))) return rc;
    HIPCHECK(hipStreamSynchronize(st));   // the caller's arrays are written only after the kernels ran
    float ms_stage = 0.f, ms = 0.f;
    if ((rc = stage_watch.stop_ms(st, &ms_stage)) || (rc = watch.stop_ms(st, &ms))) return rc;
    h->cx_stage_mb = (double)npad * (double)Dpad * sizeof(double) / 1048576.0;
    h->cx_stage_ms = ms_stage;
    (pairwise ? h->cx_pc_ms : h->cx_ms) = ms;
    HIPCHECK(hipMemcpyAsync(idx_out, didx, (size_t)N * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(score_out, dscore, (size_t)N * k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pairwise) HIPCHECK(hipMemcpyAsync(overlap_out, dover, (size_t)N * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return INSIDER_OK;
}

// ---- outlier calls (kernels: insider_outliers.hpp) -------------------------------------------------------------------
// the level table, the flag pass over X and the codes (bitmap + per-gene counts), the scan of the genes' totals, and the fill
// pass over the bitmap (the list + per-sample counts).  Nothing is written to the caller's arrays before every check passed.
int outliers_body(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int entries,
                  const double *center, const double *scale, double threshold, int64_t cap, int32_t *rows, int32_t *cols,
                  double *z, int64_t *total, int32_t *gene_counts, int32_t *sample_counts)
{
    int rc = fit_check(h, A, C, inc_continuous, K, entries);
    if (rc) return rc;
    if (!scale) return fail(INSIDER_ERR_ARG, "null scale");
    if (!total) return fail(INSIDER_ERR_ARG, "null total");
    if (!(threshold > 0.0) || !std::isfinite(threshold)) return fail(INSIDER_ERR_ARG, "threshold must be finite and > 0");
    if (cap < 0) return fail(INSIDER_ERR_ARG, "cap must not be negative");
    if (cap > 0 && (!rows || !cols || !z)) return fail(INSIDER_ERR_ARG, "cap > 0 needs rows, cols and z");
    HIPCHECK(hipSetDevice(h->ds->device));
    PostWs &w = h->post;
    hipStream_t st = h->st.stream;
    const DataSet &d = *h->ds;
    const int SL = d.SL;
    const int64_t n = d.n, p = d.p, wpl = d.ldn / 32;
    if ((rc = vd_build_table(h, A, C, K)) || (rc = w.ocs.grow((size_t)2 * p)) || (rc = w.obits.grow((size_t)p * wpl)) ||
        (rc = w.ogcnt.grow((size_t)2 * p)) || (rc = w.oscnt.grow((size_t)2 * n)) || (rc = w.ooffs.grow((size_t)p + 1)))
        return rc;
    const double *T = w.vtab;
    double *d_scale = w.ocs.get() + p, *d_center = center ? w.ocs.get() : nullptr;
    if (center) HIPCHECK(hipMemcpyAsync(d_center, center, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_scale, scale, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(w.oscnt, 0, (size_t)2 * n * sizeof(int), st));
    const int sel = entry_code(entries), m = ctns_cols(d, inc_continuous);
    const bool staged = (double)OL_GW * SL * sizeof(double) <= table_lds_budget(h);
    h->ol_path = staged ? 1 : 2;
    // four genes per block: 132 VGPRs staged, 113 from global (tools/kernel_regs.sh), no scratch: three / four waves per SIMD
    if (staged)
        hipLaunchKernelGGL((k_ol_flag<OL_GW, true>), dim3(cdiv(p, OL_GW)), dim3(64 * OL_WAVES), (size_t)OL_GW * SL * sizeof(double),
                           st, (const double *)d.X, (const uint8_t *)d.codes, d.ldn, (int)n, p, (const int *)d.lev,
                           (const int *)d.lvl_off_d, d.c, (const double *)d.Zc, m, d.SLcat, T, SL, sel, (const double *)d_center,
                           (const double *)d_scale, threshold, w.obits.get(), w.ogcnt.get());
    else
        hipLaunchKernelGGL((k_ol_flag<OL_GW, false>), dim3(cdiv(p, OL_GW)), dim3(64 * OL_WAVES), 0, st, (const double *)d.X,
                           (const uint8_t *)d.codes, d.ldn, (int)n, p, (const int *)d.lev, (const int *)d.lvl_off_d, d.c,
                           (const double *)d.Zc, m, d.SLcat, T, SL, sel, (const double *)d_center, (const double *)d_scale,
                           threshold, w.obits.get(), w.ogcnt.get());
    KCHECK();
    hipLaunchKernelGGL(k_ol_scan, dim3(1), dim3(OL_SCAN_THREADS), 0, st, (const int *)w.ogcnt, p, w.ooffs.get());
    KCHECK();
    long long tot = 0;
    HIPCHECK(hipMemcpyAsync(&tot, w.ooffs.get() + p, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    // the list holds the first min(total, cap) calls; the fill pass also runs without a list, for the per-sample counts
    const long long keep = std::min<long long>(tot, cap);
    if ((rc = w.orows.grow((size_t)keep)) || (rc = w.ocols.grow((size_t)keep)) || (rc = w.oz.grow((size_t)keep))) return rc;
    if (tot > 0 && (keep > 0 || sample_counts)) {
        hipLaunchKernelGGL(k_ol_fill, dim3(cdiv(p, OL_WAVES)), dim3(64 * OL_WAVES), 0, st, (const double *)d.X, d.ldn, (int)n, p,
                           (const int *)d.lev, (const int *)d.lvl_off_d, d.c, (const double *)d.Zc, m, d.SLcat, T, SL,
                           (const double *)d_center, (const double *)d_scale, (const uint32_t *)w.obits,
                           (const long long *)w.ooffs, keep, w.orows.get(), w.ocols.get(), w.oz.get(), w.oscnt.get());
        KCHECK();
    }
    if (keep > 0) {
        HIPCHECK(hipMemcpyAsync(rows, w.orows, (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(cols, w.ocols, (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(z, w.oz, (size_t)keep * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (gene_counts) HIPCHECK(hipMemcpyAsync(gene_counts, w.ogcnt, (size_t)2 * p * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (sample_counts) HIPCHECK(hipMemcpyAsync(sample_counts, w.oscnt, (size_t)2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    *total = (int64_t)tot;
    return INSIDER_OK;
}

}  // namespace

extern "C" {

int insider_hip_residual(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                         const int32_t *subtract, int64_t row_begin, int64_t row_end, double *out)
{
    return ph_finish(h, residual_body(h, A, C, inc_continuous, K, subtract, row_begin, row_end, out));
}

int insider_hip_interaction_glm(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                const int32_t *subtract, const int32_t *group, int G, double *coeff, double *se,
                                double *dof)
{
    return ph_finish(h, interaction_glm_body(h, A, C, inc_continuous, K, subtract, group, G, coeff, se, dof));
}

int insider_hip_variance_decomposition(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                       int entries, double *out)
{
    return ph_finish(h, variance_decomposition_body(h, A, C, inc_continuous, K, entries, out));
}

int insider_hip_sample_decomposition(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                     int entries, double *out)
{
    return ph_finish(h, sample_decomposition_body(h, A, C, inc_continuous, K, entries, out));
}

int insider_hip_level_scores(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                             int entries, int cov, const double *cand, int n_cand, double *sse, double *cnt)
{
    return ph_finish(h, level_scores_body(h, A, C, inc_continuous, K, entries, cov, cand, n_cand, sse, cnt));
}

int insider_hip_factor_decomposition(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                     int entries, double *out)
{
    return ph_finish(h, factor_decomposition_body(h, A, C, inc_continuous, K, entries, out));
}

int insider_hip_residual_products(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                  int entries, const double *center, const double *scale, const double *Q, int q, double *Z,
                                  double *Y, double *rss)
{
    return ph_finish(h, residual_products_body(h, A, C, inc_continuous, K, entries, center, scale, Q, q, Z, Y, rss));
}

int insider_hip_coexpression(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                             int entries, const double *center, const double *scale, int axis, int k, int32_t *idx_out,
                             double *score_out)
{
    return ph_finish(h, coexpression_body(h, A, C, inc_continuous, K, entries, center, scale, axis, k, idx_out, score_out));
}

int insider_hip_coexpression_pairwise(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                      int entries, const double *center, const double *scale, int axis, int64_t min_overlap,
                                      int k, int32_t *idx_out, double *score_out, int32_t *overlap_out)
{
    return ph_finish(h, coexpression_body(h, A, C, inc_continuous, K, entries, center, scale, axis, k, idx_out, score_out, true,
                                          min_overlap, overlap_out));
}

int insider_hip_outliers(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                         int entries, const double *center, const double *scale, double threshold, int64_t cap,
                         int32_t *rows, int32_t *cols, double *z, int64_t *total, int32_t *gene_counts,
                         int32_t *sample_counts)
{
    return ph_finish(h, outliers_body(h, A, C, inc_continuous, K, entries, center, scale, threshold, cap, rows, cols, z, total,
                                      gene_counts, sample_counts));
}

}  // extern "C"
