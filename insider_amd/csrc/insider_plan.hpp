// The kernel path of one fit call, decided once: what it is decided from (PlanFacts), the two cost models, the weighted-SYRK
// tiling, the rule of every kernel form a launch helper can take, and the builder (build_plan).  Plain host C++ over the
// constants of insider_shapes.hpp: nothing here sees a handle or a device buffer, so a CPU program compiles this file and
// compares its answers case by case (tests/plan_driver.cpp, tests/test_plan_cpu.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "insider_shapes.hpp"

namespace {

using namespace insider;

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// the kernels of the column solve, as insider_hip_get_info("col_solver" / "col_eval") reports them, and the one the batch entry
// launched (insider_hip_last_cd_solver; include/insider_hip.h; insider_amd/_lib.py COL_SOLVERS mirrors the names)
enum ColSolver {
    CS_NONE = 0, CS_RIDGE_REG = 1, CS_RIDGE = 2, CS_CD_REG = 3, CS_CD_REG3 = 4, CS_CD_COLS16 = 5, CS_CD_COLS32 = 6,
    CS_CD_COLS64 = 7, CS_CD_R16_1 = 8, CS_CD_R16_2 = 9, CS_CD_R16_3 = 10
};

// the kernels of the column-side statistics, as insider_hip_get_info("col_stats_kernel") reports them (include/insider_hip.h;
// insider_amd/_lib.py COL_STATS_KERNELS mirrors the names).  k_col_paircnt4<., ., 8, true> is compiled (the PC4 macro
// instantiates it) but never launched: real-valued counts with more than four k-steps take k_col_paircnt.
enum ColStatsKernel {
    CSK_NONE = 0, CSK_LIST = 1, CSK_LIST4 = 2, CSK_FACTORED = 3, CSK_PAIRCNT = 4, CSK_PAIRCNT_ZT = 5, CSK_PAIRCNT4_MS4 = 6,
    CSK_PAIRCNT4_MS8 = 7, CSK_PAIRCNT4_MS4_ZT = 8
};

// the forms of a reduction product over rows (reduce_form): k_mm_reduce<NB>, k_mm_reduce2<NB, 2>, k_mm_reduce2<NB, 4>
enum ReduceForm { MR_REDUCE = 0, MR_REDUCE2_2 = 2, MR_REDUCE2_4 = 4 };

// The weighted SYRK of one covariate as a GEMM over genes (k_wgemm): whether, and its tiling (wgemm_plan)
struct WgPlan {
    bool use = false;
    int tiles = 0, LT = 0, zch = 0, ntile = 0, npair = 0, slab = 0, nslab = 0;
};

// What a call's kernel path is decided from, as plain values (plan_facts fills them from the data set, the options and K): a
// device buffer appears only as "is there one"
struct PlanFacts {
    struct {                          // the options that decide a path (Options, by name)
        int row_merged, col_factored, row_fused, row_gemm, row_counts, mm_fast, force_allreduce, wg_waves;
        int list_fine, mm_tiles, col_mfma4, cd_variant, cd_pairs, cd_cold_iters, cd_pass_first, cd_pass_ratio, max_sweeps;
        int stats_own_q;
    } opt{};
    int world = 1, n_simd = 1024;
    int K = 0, NB = 0, KP = 0;        // NB = KP = 0: no workspace yet (insider_hip_get_info before the first call)
    bool lvl_zero = false;            // the workspace holds its all-zero level records
    bool fperm = false;               // ... and the buffer of k_tile_perm's row order (k_list_stats4)
    bool merged = false, cont_merged = false, cf_pair_ok = false, cf_hn = false, cf_zt = false, cf_sq = false;
    int c = 0, m = 0, SL = 0, SLP = 0, SLcat = 0;
    int64_t n = 0, p = 0;
    uint64_t col_entries = 0, row_entries = 0;
    std::vector<int> L;               // per covariate: levels, and (level, gene) pairs with held-out samples
    std::vector<int64_t> npairs;
    // the factored statistics' static part (ColFacArgs), position order
    int cf_c = 0, cf_tab_rows = 0, cf_nsteps = 0, cf_L[CF_MAXC + 1] = {0}, cf_nlater[CF_MAXC + 1] = {0};
};

// The column solve a call runs (build_plan): none, or the one with these parameters
struct ColCall {
    double alpha, la;                 // alpha, and lambda alpha as the kernel receives it (CdParams::la)
};

// The kernel path of ONE call, decided once (build_plan) after ensure_workspace and before its first launch: every launch
// helper reads it from the handle, none decides again.  DESIGN §4 has the table of what runs for which plan.
struct FitPlan {
    bool masked = false;
    bool merged = false;              // masked row update without per-sample statistics (use_merged)
    bool unmasked_fused = false;      // unmasked row update as k_level_merged on an all-zero record
    bool fused_solve = false;         // ... and either of them with the level solves in that launch
    bool row_fused = false;           // option "row_fused" as the plan saw it: k_level_merged, not k_level_pack / k_level_reduce
    bool allreduce = false;           // the level equations and the loss sums cross ranks: a collective is enqueued
    bool list4 = false;               // per-entry statistics of either side on k_list_stats4<2, NT, 4>, not k_list_stats<NB>
    int mm_fast = 0;                  // option "mm_fast" as the plan saw it (reduce_form reads it)
    bool q_rows2 = false;             // Q = S A and Qheld = S^held A on k_mm_rows2, not k_mm_rows
    bool v_rows2 = false;             // V = C A' the same
    int mm_tpw = 1;                   // ... and the tiles of 16 genes a wave of k_mm_rows2 takes, at either site
    int col_path = 0;                 // column statistics: 0 = per-entry lists, 1 = look-up form, 2 = pair-count form (col_stats_path)
    int NB = 0, KP = 0, stat_len = 0, plen = 0;   // record geometry: 16-column blocks, padded K, doubles per statistics / level record
    std::vector<WgPlan> wg;           // per covariate: its level Gram sums as a GEMM over genes?
    std::vector<uint8_t> u_cnt;       // per covariate: u from the dense pair counts (k_gene_u_cnt), not from the entry lists?
    // the pair-count statistics (col_path == 2): the kernel, its dynamic LDS, and for k_col_paircnt4 its grid and the ticket
    // counters in use (else 0)
    ColStatsKernel pc_kernel = CSK_NONE;
    size_t pc_lds = 0;
    int pc_blocks = 0, pc_parts = 0;
    // ... and whether k_col_paircnt4 forms Q = S A and Qheld = S^held A of its genes itself (stats_own_q): the two products over
    // the genes and their stream joins are then not launched
    bool stats_own_q = false;
    // the column solve (CS_NONE: the call runs none), the kernel of the evaluation pass behind a register-resident solve
    // (CS_NONE: the solve kernel evaluates), and whether a ridge solve is followed by the general route for the genes it marked
    ColSolver col_solver = CS_NONE, col_eval = CS_NONE;
    bool ridge_fallback = false;
    // outer iterations 0 .. cold_iters - 1 solve in passes: pass i stops at sweep pass_limit[i], one more runs to the end
    int cold_iters = 0, npass = 0, pass_limit[16] = {0};
    // the sweep-order table: rows of 64 row offsets (row16 kernel), and blocks of two coordinate steps (their base address)
    bool order_wide = false, order_pairs = false;
};

// ---- the rules of the launch helpers: plain functions of the facts, the plan so far and a launch site's integers ---------------

// 16 <= K <= 31: the 4x4x4 form of the matrix instruction (fewer wasted outputs: 28 tiles instead of 3 blocks at K = 25)
inline bool list_stats4(const PlanFacts &f)
{
    const int NT = (f.K + 4) / 4;
    return f.opt.list_fine && f.NB == 2 && NT >= 5 && NT <= 8 && f.fperm;
}

// k_mm_rows2: tiles of 16 rows one wave takes — one until the grid fills every SIMD twice, then as many as keep it at that
// (option "mm_tiles" >= 1: that many)
inline int mm_tiles_per_wave(const PlanFacts &f, int tiles)
{
    if (f.opt.mm_tiles >= 1) return f.opt.mm_tiles;
    return std::max(1, tiles / (2 * f.n_simd));
}

// out[M x KP] = X[M x Kd] W[Kd x KP] on k_mm_rows2: from MM_FAST_MIN rows on, 16-byte reads of X's rows, W staged in LDS
inline bool mm_rows2_fits(const PlanFacts &f, int64_t ldx, int64_t M, int Kd)
{
    return f.opt.mm_fast && M >= MM_FAST_MIN && ldx % 2 == 0 && (size_t)4 * cdiv(Kd, 16) * f.NB * 64 * sizeof(double) <= 64 * 1024;
}

// V = C A' for N stacked levels: the tiles of 16 output columns a block of k_mm_rows / k_mm_rows2 takes (1, 2 or 4; a covariate
// with few levels: one tile, not four)
inline int mm_rows_nt(int N) { return N <= 16 ? 1 : N <= 32 ? 2 : 4; }

// The reduction X'Y over M rows into L x KP sums: several column tiles of X per wave with a deeper look-ahead (k_mm_reduce2, two
// or four tiles; the same partial sums) from MM_FAST_MIN rows and 17 columns on.  Its sites: the Gram of R (n, KP) and of C
// (p, KP), S'C (p, SL) and U'C of covariate i (p, L_i; 1 for a continuous column).
inline ReduceForm reduce_form(const FitPlan &p, int64_t M, int L)
{
    if (!(p.mm_fast && M >= MM_FAST_MIN && L > 16)) return MR_REDUCE;
    return (cdiv(L, 16) <= 2 || p.mm_fast == 2 || p.NB > 2) ? MR_REDUCE2_2 : MR_REDUCE2_4;
}

// The pair-count statistics kernel (insider_col_factored.hpp) over every gene: k_col_paircnt4 (second product on the 4x4x4
// matrix instruction, factor rows of every position staged in LDS) where it applies and fits, else k_col_paircnt
inline void paircnt_plan(const PlanFacts &f, FitPlan &p)
{
    const int blocks = cdiv(f.p, 4), KP = f.KP, nsteps = f.cf_nsteps;
    const bool zt = f.cf_zt;
    if (f.opt.col_mfma4 && f.NB <= 2 && !(zt && nsteps > 4)) {   // (real-valued counts with more than four k-steps: 180 registers, two waves per SIMD)
        size_t quads = 1;
        for (int t = 0; t < f.cf_c + (zt ? 1 : 0); ++t) quads += (size_t)(f.cf_L[t] + 3) / 4;
        const size_t lds = ((size_t)4 * 16 * 17 + (size_t)KP * KP + (size_t)4 * nsteps * KP + 4 * quads * KP) * sizeof(double);
        if (lds <= 64 * 1024) {
            // as many blocks as stay resident (48.6 KB of LDS at c3: three per CU); each walks the groups of four genes with the grid's stride
            const int resident = std::max(1, std::min((int)(160 * 1024 / lds), 3)) * std::max(1, f.n_simd / 4);   // registers: 148 - 166
            int nb = std::min(blocks, resident);
            p.pc_parts = nb >= PC4_PARTS ? PC4_PARTS : 1;      // ticket counters in use (k_col_paircnt4)
            p.pc_blocks = nb - nb % p.pc_parts;
            p.pc_lds = lds;
            p.pc_kernel = zt ? CSK_PAIRCNT4_MS4_ZT : nsteps <= 4 ? CSK_PAIRCNT4_MS4 : CSK_PAIRCNT4_MS8;
            return;
        }
    }
    p.pc_lds = ((size_t)4 * 16 * 17 + (size_t)KP * KP + (size_t)4 * nsteps * KP) * sizeof(double);
    p.pc_kernel = zt ? CSK_PAIRCNT_ZT : CSK_PAIRCNT;
}

// k_col_paircnt4 forms each gene's rows of Q = S A and Qheld = S^held A itself, in two free columns of its second product (option
// "stats_own_q"; insider_col_factored.hpp)?  Needs K <= KP - 2, the level sums in the kernel's order (categorical covariates
// only) and one rank (a shard keeps the products).  Option 1: calls that run a column solve (the fit, the column update); 2: the
// densifying entry insider_hip_col_stats too.
inline bool stats_own_q(const PlanFacts &f, const FitPlan &p, bool col_call)
{
    if (!(f.opt.stats_own_q >= 2 || (f.opt.stats_own_q == 1 && col_call))) return false;
    // (k_col_paircnt4 with eight k-steps would go past 168 registers and lose its third wave per SIMD: it keeps the products)
    if (!(p.masked && p.col_path == 2 && p.pc_kernel == CSK_PAIRCNT4_MS4)) return false;
    return f.cf_sq && f.m == 0 && !f.cf_zt && f.world <= 1 && f.K <= f.KP - 2;
}

// 32 < K <= 48 with an l1 term: the register-resident kernel with its third slot's matrix columns in LDS (insider_cd_reg.hpp)
inline bool reg3_path(int K, double la) { return K > 32 && K <= 48 && la > 0.0; }

// The elastic-net solve kernel for K, lambda alpha and the option cd_variant: the column update's and the batch entry's.
inline ColSolver cd_solver(int K, double la, int cd_variant)
{
    // the register-resident kernel scales its state by 1 / (2 lambda alpha): lambda alpha = 0 (alpha < 0 or lambda = 0: no l1
    // term at all) takes the group kernel below
    if (cd_variant == 0 && (K <= 32 || reg3_path(K, la)) && la > 0.0) return K <= 32 ? CS_CD_REG : CS_CD_REG3;
    if (cd_variant == 2 && K <= 16) return CS_CD_R16_1;
    if (cd_variant == 2 && K <= 32) return CS_CD_R16_2;
    if (K <= 16) return CS_CD_COLS16;
    if (K <= 32) return CS_CD_COLS32;
    // 32 < K <= 48 when the register-resident kernel's three-slot form does not apply (cd_variant = 2, or no l1 term): four genes
    // per wavefront with the whole Gram matrices in LDS (row16 kernel, three coordinate slots per lane).  Beyond 48 a CU's LDS
    // holds one such wave and the group kernel is faster; it also stays as cd_variant = 1 (cross-check)
    if (cd_variant != 1 && K <= 48) return CS_CD_R16_3;
    return CS_CD_COLS64;
}

// rows of the sweep-order table for K > 32 carry 64 row offsets (row16 kernel) unless s takes the register-resident kernel's
// successor list
inline bool order_wide_rows(int K, ColSolver s) { return K > 32 && s != CS_CD_REG3; }

// The column solve of a call: the ridge kernels (alpha == 0) or cd_solver's, the evaluation pass and the cold passes' limits
inline void col_solve_plan(const PlanFacts &f, const ColCall &c, FitPlan &p)
{
    const bool ridge = c.alpha == 0.0;
    p.col_solver = !ridge ? cd_solver(f.K, c.la, f.opt.cd_variant) : (f.K <= 32 && f.opt.cd_variant == 0) ? CS_RIDGE_REG : CS_RIDGE;
    // genes whose system was not positive definite: solve(..., likely_sympd)'s general route
    p.ridge_fallback = p.col_solver == CS_RIDGE_REG;
    // the per-gene loss statistics behind a register-resident solve: its evaluation form; three slots: the row16 kernel's
    // evaluation part (the sweep kernel's registers are all taken)
    p.col_eval = p.col_solver == CS_CD_REG ? CS_CD_REG : p.col_solver == CS_CD_REG3 ? CS_CD_R16_3 : CS_NONE;
    if (p.col_eval != CS_NONE && f.opt.cd_pass_first >= 32) {
        p.cold_iters = f.opt.cd_cold_iters;
        for (int64_t l = f.opt.cd_pass_first; l < std::min<int64_t>(f.opt.max_sweeps, 4 * (int64_t)INSIDER_PERM_PERIOD) && p.npass < 16;
             l *= std::max(f.opt.cd_pass_ratio, 2))
            p.pass_limit[p.npass++] = (int)l;   // the last pass runs from the last limit to the end, however far that is
    }
    p.order_wide = order_wide_rows(f.K, p.col_solver);
}

// The weighted SYRK of covariate i as a GEMM over genes (k_wgemm, insider_row_merged.hpp)?  Needs the static half-count table
// of the pair-count statistics; pays when the covariate has at least four tiles of 16 levels and the GEMM needs clearly fewer
// MFMAs than the per-(level, gene) form.
WgPlan wgemm_plan(const PlanFacts &f, int i, bool whatever_the_option = false)
{
    WgPlan w;
    const int K = f.K;
    if (!((f.opt.row_gemm || whatever_the_option) && f.cf_pair_ok && f.cf_hn && f.merged && f.c <= CF_MAXC && K >= 1)) return w;
    const int NB = (K + 1 + 15) / 16;
    const int L = f.L[i], NBLK = NB * (NB + 1) / 2;
    w.tiles = cdiv(L, 16);
    w.npair = K * (K + 1) / 2;
    w.ntile = cdiv(w.npair, 16);
    if (w.tiles < 4 || (double)w.tiles * w.ntile >= 0.9 * (double)L * NBLK) return w;
    w.zch = cdiv(w.tiles, 7);
    w.LT = cdiv(w.tiles, w.zch);
    const int waves_per_slab = cdiv(w.ntile, 2) * w.zch;
    // one wave per SIMD: the kernel runs beside the main stream's V -> u -> U'C chain (other waves fill the machine), its
    // operands are prefetched a step ahead, and every slab costs a partial record (levels x pairs doubles) to write and re-read
    // (rounded DOWN: at most wg_waves waves in all — with the default, one per SIMD: a surplus block would run as a second round)
    const int want = std::max(1, std::min<int>(f.opt.wg_waves / waves_per_slab, (int)cdiv(f.p, 64)));
    w.slab = (int)round_up(cdiv(f.p, want), 4);
    w.nslab = (int)cdiv(f.p, w.slab);
    w.use = true;
    return w;
}

// Which kernel forms the column-side statistics: 0 = k_list_stats (one rank-one MFMA group per held-out entry), 1 =
// k_col_factored (look-up form), 2 = k_col_paircnt (pair-count form).  Issue-cycle models per gene with E held-out
// entries: the list kernel spends NBLK MFMAs (64 cycles) per 4 entries; the look-up form NB^2 MFMAs per 4 levels plus, per
// later covariate and 16-entry batch of a level group, 16 x (2 + NB) vector instructions (4.6 cycles); the pair-count form
// NB^2 MFMAs per 4 levels plus ceil(rows / 4) x NB MFMAs per 16 levels.  Measured at c3 / c5: look-up 0.51 vs list 1.30 ms
// (model 14.5k vs 48k cycles) and 2.44 vs 0.66 ms (72k vs 24k).
int col_stats_path(const PlanFacts &f)
{
    if (!(f.merged && f.opt.col_factored && f.c <= CF_MAXC)) return 0;
    if (f.m > 0) return (f.cf_pair_ok && f.cf_zt) ? 2 : 0;   // continuous covariates: the pair-count form with real-valued counts, or the lists
    const bool lookup_fits = ((size_t)(f.cf_tab_rows + 1) * f.KP + 4 * 16 * 17) * sizeof(double) + (size_t)4 * CF_CAP * 2 <= 64 * 1024;
    if (f.opt.col_factored == 3 && f.cf_pair_ok) return 2;                   // forced
    if (f.opt.col_factored >= 2) return lookup_fits ? 1 : (f.cf_pair_ok ? 2 : 0);   // forced (3 without a count table: look-up form)
    const double E = (double)f.col_entries / (double)std::max<int64_t>(f.p, 1);
    const int NB = f.NB;
    const double list = E * (NB * (NB + 1) / 2) * 16.0;
    double fac = 0.0, pair = 0.0;
    for (int t = 0; t < f.cf_c; ++t) {
        const double batches = std::ceil(std::max(1.0, E / f.cf_L[t]) / 16.0);
        fac += std::ceil(f.cf_L[t] / 4.0) * (NB * NB * 64.0 + f.cf_nlater[t] * batches * 16.0 * (2 + NB) * 4.6);
        pair += std::ceil(f.cf_L[t] / 4.0) * NB * NB * 64.0 +
                std::ceil(f.cf_L[t] / 16.0) * ((f.cf_nlater[t] > 0 ? f.cf_nsteps * NB * 64.0 : 0.0) + 150.0);
    }
    double best = list;
    int path = 0;
    if (lookup_fits && 1.3 * fac < best) { best = 1.3 * fac; path = 1; }
    if (f.cf_pair_ok && 1.3 * pair < best) { best = 1.3 * pair; path = 2; }
    return path;
}

// masked update without per-sample statistics (insider_row_merged.hpp)?  Time model (us at c3 / c5 rates): per-sample
// path = one rank-one MFMA group per held-out entry + the level kernels; merged path per covariate = one weighted group per
// (level, gene) pair + one look-up per entry and other covariate + the small products over its levels.  Measured at
// c3: 0.55 vs 1.4 ms (model 0.45 vs 1.38); at c5 (4 covariates): 1.37 vs 0.85 ms (model 1.24 vs 0.84).
bool use_merged(const PlanFacts &f, int masked)
{
    if (!(masked && f.merged && f.opt.row_merged && (f.m == 0 || f.cont_merged))) return false;
    if (f.opt.row_merged == 2 || f.m > 0) return true;   // forced / continuous covariates: the per-sample pass is the slow alternative
    const int NB = f.NB ? f.NB : 2;
    const double mf = (NB * (NB + 1) / 2) * 16.0 / (1024.0 * 2100.0);   // us per rank-one group entry on the whole GPU
    const double E = (double)f.row_entries, pscale = (double)f.p / 5.0e4;
    const double old_us = E * mf * 1.15 + 50.0 * f.c;
    double merged_us = 0.0;
    for (int i = 0; i < f.c; ++i)
        merged_us += (double)f.npairs[i] * mf * 1.1 + E * (f.c - 1) * 1.3e-6 + 33.0 * pscale * f.SLcat / 110.0 / f.c +
                     37.0 * pscale * f.L[i] / 100.0 + 40.0;
    return 1.1 * merged_us < old_us;
}

// The plan of a call: a pure function of the facts.  The two cost models (use_merged, col_stats_path) are asked here and
// nowhere else: insider_hip_get_info answers its path keys from a fresh plan.
FitPlan build_plan(const PlanFacts &f, int masked, const ColCall *col = nullptr)
{
    FitPlan p;
    p.masked = masked != 0;
    p.merged = use_merged(f, masked);
    // tuning = 0 (src/optimize.cpp:178-191): XtX_l = |l| CC' + lambda I and Xty_l = (S C')[l] - CC' sum_{r in l} s_r are the merged
    // update's equations with EMPTY held-out sums, and sum_{r in l} s_r comes from the level-pair sample counts: one launch per
    // covariate (k_level_merged on an all-zero record) instead of five over the samples, and R is rebuilt once per outer iteration.
    // What it buys is launch latency: on small data a long unmasked fit (the reference's fit() default) is a chain of ~5 us kernels.
    p.unmasked_fused = !masked && f.merged && f.opt.row_merged && f.opt.row_fused && f.m == 0 && f.lvl_zero;
    // the level records' tail, the level equations and (unless the equations still have to cross ranks) the solves: one launch
    p.fused_solve = (p.merged || p.unmasked_fused) && f.world <= 1 && !f.opt.force_allreduce && f.opt.row_fused && f.NB <= 2;
    p.row_fused = f.opt.row_fused != 0;
    p.allreduce = f.world > 1 || f.opt.force_allreduce;
    p.list4 = list_stats4(f);
    p.mm_fast = f.opt.mm_fast;
    p.q_rows2 = mm_rows2_fits(f, f.SLP, f.p, f.SL);   // (S and S^held: p rows of pitch SLP, SL stacked levels)
    p.v_rows2 = f.opt.mm_fast && f.p >= MM_FAST_MIN;   // A' staged in LDS once per block, C read in 16-byte pieces
    p.mm_tpw = mm_tiles_per_wave(f, cdiv(f.p, 16));
    p.col_path = col_stats_path(f);
    if (p.col_path == 2) paircnt_plan(f, p);
    p.stats_own_q = stats_own_q(f, p, col != nullptr);
    if (col) col_solve_plan(f, *col, p);
    p.order_pairs = f.opt.cd_pairs && reg_pairs(reg_kmax(f.K));
    p.NB = f.NB;
    p.KP = f.KP;
    p.stat_len = f.NB * (f.NB + 1) / 2 * 256;
    p.plen = p.stat_len + 2 * f.KP + 2;
    for (int i = 0; i < f.c; ++i) {
        p.wg.push_back(wgemm_plan(f, i));
        // u from the dense pair counts (insider_col_factored.hpp) when its per-wave record — V row [SL] | out [LP] | partial sums — fits LDS
        const size_t gu_lds = (size_t)4 * (f.SL + round_up(f.L[i], 2) + GU_BATCH * WAVE) * sizeof(double);
        p.u_cnt.push_back(f.cf_pair_ok && (f.opt.row_counts || f.m > 0) && f.c <= CF_MAXC && gu_lds <= 64 * 1024);
    }
    return p;
}

}  // namespace
