// The kernel path of one fit call, decided once: what it is decided from (PlanFacts), the two cost models and the weighted-SYRK
// tiling, and the builder (build_plan).  Plain host C++: nothing here sees a handle or a device buffer, so a CPU program can
// compile this file and compare its answers case by case.  Expects CF_MAXC, CF_CAP, GU_BATCH (insider_col_factored.hpp) and
// WAVE (insider_kernels.hpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

constexpr int MM_FAST_MIN = 16384;   // rows from which k_mm_rows2 / k_mm_reduce2 run (below: the staging and the longer waves cost more than they save; c1: 5000 genes)

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
    } opt{};
    int world = 1;
    int K = 0, NB = 0, KP = 0;        // NB = KP = 0: no workspace yet (insider_hip_get_info before the first call)
    bool lvl_zero = false;            // the workspace holds its all-zero level records
    bool merged = false, cont_merged = false, cf_pair_ok = false, cf_hn = false, cf_zt = false;
    int c = 0, m = 0, SL = 0, SLcat = 0;
    int64_t p = 0;
    uint64_t col_entries = 0, row_entries = 0;
    std::vector<int> L;               // per covariate: levels, and (level, gene) pairs with held-out samples
    std::vector<int64_t> npairs;
    // the factored statistics' static part (ColFacArgs), position order
    int cf_c = 0, cf_tab_rows = 0, cf_nsteps = 0, cf_L[CF_MAXC + 1] = {0}, cf_nlater[CF_MAXC + 1] = {0};
};

// The kernel path of ONE call, decided once (build_plan) after ensure_workspace and before its first launch: every launch
// helper reads it from the handle, none decides again.  DESIGN §4 has the table of what runs for which plan.
struct FitPlan {
    bool masked = false;
    bool merged = false;              // masked row update without per-sample statistics (use_merged)
    bool unmasked_fused = false;      // unmasked row update as k_level_merged on an all-zero record
    bool fused_solve = false;         // ... and either of them with the level solves in that launch
    bool mm_fast = false;             // k_mm_rows2 / k_mm_reduce2 apply to products over the p genes
    int col_path = 0;                 // column statistics: 0 = per-entry lists, 1 = look-up form, 2 = pair-count form (col_stats_path)
    int NB = 0, KP = 0, stat_len = 0, plen = 0;   // record geometry: 16-column blocks, padded K, doubles per statistics / level record
    std::vector<WgPlan> wg;           // per covariate: its level Gram sums as a GEMM over genes?
    std::vector<uint8_t> u_cnt;       // per covariate: u from the dense pair counts (k_gene_u_cnt), not from the entry lists?
};

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
FitPlan build_plan(const PlanFacts &f, int masked)
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
    p.mm_fast = f.opt.mm_fast && f.p >= MM_FAST_MIN;
    p.col_path = col_stats_path(f);
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
