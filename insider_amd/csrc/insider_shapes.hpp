// The shape constants that the kernels and the call plan (insider_plan.hpp) both read, each defined once.  Nothing but constexpr
// values and inline integer functions: no HIP header, so a host compiler alone takes it.
#pragma once

#include "../../include/insider_perm.h"   // INSIDER_PERM_PERIOD

#if defined(__HIPCC__)
#define INSIDER_SHAPE_FN __host__ __device__ constexpr
#else
#define INSIDER_SHAPE_FN constexpr
#endif

namespace insider {

constexpr int WAVE = 64;

// factored column statistics (insider_col_factored.hpp)
constexpr int CF_MAXC = 8;        // covariates
constexpr int CF_CAP = 2048;      // uint16 look-up indices staged per wave (entries x later covariates)
constexpr int GU_BATCH = 8;       // blocks of 16 levels whose partial sums share one trip through LDS (k_gene_u_cnt)
constexpr int PC4_PARTS = 16;     // ticket counters of k_col_paircnt4
constexpr int CF_SQ_BLOCK = 36;     // doubles per gene and block of 16 levels of the level sums in k_col_paircnt4's order (ColFacArgs::sq): 16 of S, 16 of S^held, 4 zeros

// the small dense products (insider_mm.hpp)
constexpr int MM_SLAB = 128;          // rows per partial of the reduction products
constexpr int MM_FAST_MIN = 16384;    // rows from which k_mm_rows2 / k_mm_reduce2 run (below: the staging and the longer waves cost more than they save; c1: 5000 genes)

// the register-resident sweep kernel (insider_cd_reg.hpp)
// does the instantiation take its successor list as absolute address pairs (else: 32-bit offsets)?
INSIDER_SHAPE_FN bool reg_pairs(int KMAX) { return KMAX <= 30; }
// smallest instantiated KMAX >= K
INSIDER_SHAPE_FN int reg_kmax(int K) { return K <= 16 ? 16 : (K <= 32 ? (K + 1) & ~1 : (K + 3) & ~3); }

}  // namespace insider
