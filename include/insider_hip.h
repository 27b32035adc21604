/*
 * insider_hip.h — C ABI of libinsider_hip.so, the MI355X-native INSIDER
 * factorisation core.
 *
 * This is the drop-in boundary for the reference's Rcpp exports
 * (/root/reference/src/RcppExports.cpp:112-124, R/RcppExports.R:4-22): plain
 * pointers and sizes, no SEXP / Rcpp / Armadillo / torch types.  All host
 * matrices are column-major fp64 exactly as R hands them to the reference
 * (zero-copy views, src/optimize.cpp:283-284); masks are uint8 instead of the
 * reference's fp64 copies (src/RcppExports.cpp:96-97); level ids are int32,
 * 1-based, exactly 1..L_i per covariate (src/optimize.cpp:175,286 index rows as
 * level-1; validated here, status INSIDER_ERR_ARG otherwise).
 *
 * Error model: every entry point returns an int status (0 = ok) and never
 * calls exit() (the reference does on bad `tuning`, src/optimize.cpp:249-251,
 * 270-272); insider_hip_last_error() returns the message of the calling
 * thread's last failure.  The library fails loudly (INSIDER_ERR_NO_DEVICE)
 * when no HIP device is present: there is no CPU fallback.
 */
#ifndef INSIDER_HIP_H
#define INSIDER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INSIDER_OK 0
#define INSIDER_ERR_ARG 1        /* bad argument (tuning not in {0,1}, level ids not 1..L_i, K out of range, ...) */
#define INSIDER_ERR_SOLVE 2      /* a normal-equation system is singular to working precision (neither route of
                                    solve(..., likely_sympd) could solve it) */
#define INSIDER_ERR_ALLOC 3      /* host or device allocation failed */
#define INSIDER_ERR_HIP 4        /* HIP runtime error (message has the call) */
#define INSIDER_ERR_NO_DEVICE 5  /* no HIP device / extension unusable: no fallback exists */
#define INSIDER_ERR_UNSUPPORTED 6 /* K > 63, n or p >= 2^23, ... */
#define INSIDER_ERR_COMM 7       /* RCCL or the all-reduce callback reported failure, or world > 1 has neither */
#define INSIDER_ERR_UNFINISHED 8 /* insider_hip_hclust: max_rounds was reached before one cluster was left */

/* Largest latent dimension the kernels support (K + 1 augmented column <= 64). */
#define INSIDER_MAX_K 63

/* Number of doubles per trajectory row written by insider_hip_optimize():
 * {iter, train_rmse, test_rmse, SSE/2, row_reg/2, col_reg/2, l1_reg, loss, delta_loss, decay}.
 * Row 0 is the evaluation of the initial values (iter = -1; src/optimize.cpp:320-323); one row per
 * checkpoint follows (iter % 10 == 0; src/optimize.cpp:381-408).  These are the quantities the reference
 * prints to stdout (src/utils.cpp:70-76,95-100). */
#define INSIDER_TRAJ_STRIDE 10

typedef struct insider_hip_handle insider_hip_handle;

/* Sum-all-reduce of `count` doubles at device pointer `dev_buf`, in place, across the gene-sharded ranks.
 * Called by insider_hip_optimize() on the calling thread.  `stream` is the library's HIP stream (a hipStream_t):
 * the kernels producing dev_buf have been ENQUEUED on it, not necessarily completed, and the consumers will be
 * enqueued on it after the call returns.  The callback must therefore order the reduction after the prior work of
 * `stream` and before its later work — either by enqueueing the collective on / against that stream (no host
 * synchronisation needed; insider_amd/dist.py does this through torch.cuda.ExternalStream), or by synchronising
 * the stream, reducing, and synchronising again.  Return 0 on success. */
typedef int (*insider_allreduce_fn)(void *user, double *dev_buf, int64_t count, void *stream);

/* "insider_hip <version> (gfx950) src:<sha16>": the hash is over the sources the library was compiled from
 * (insider_amd/csrc, include/, compiler flags; insider_amd/_build.py), so a caller can tell which sources a number belongs to. */
const char *insider_hip_version(void);
const char *insider_hip_last_error(void);
/* Number of visible HIP devices (0 if none); does not create a context. */
int insider_hip_device_count(void);

/*
 * Upload one data set (or one gene slab of it) to HBM and precompute everything that does not depend on the
 * factors: the combined uint8 mask codes, transposed copies for the row-side pass, per-level row sums of X,
 * per-gene sums of squares.  Replaces the per-call marshaling of src/RcppExports.cpp:91-97 — tune()'s grid
 * (R/insider.R:142-174) re-uploads nothing but the inits.
 *   X        n x p column-major fp64 (NA entries must hold 0, R/insider.R:26)
 *   levels   n x c column-major int32, 1-based ids (cfd_indicators, src/optimize.cpp:256)
 *   n_levels c entries, L_i
 *   M_train  n x p uint8 (train_indicator), M_test n x p uint8 (test_indicator); an entry with both 0 is NA
 *   device   HIP device ordinal
 */
int insider_hip_create(const double *X, int64_t n, int64_t p, const int32_t *levels, int c, const int32_t *n_levels,
                       const uint8_t *M_train, const uint8_t *M_test, int device, insider_hip_handle **out);
/* The same with continuous covariates (ctns_confounder of R/insider.R:48-51; src/optimize.cpp:276-291): ctns is
 * n x m column-major fp64 (NULL / 0 for none).  insider_hip_optimize() must then be called with inc_continuous = 1
 * and c + 1 row-factor pointers, the last one m x K column-major (cfd_matrices(cfd_num-1), :281-291). */
int insider_hip_create_ex(const double *X, int64_t n, int64_t p, const int32_t *levels, int c, const int32_t *n_levels,
                          const double *ctns, int m, const uint8_t *M_train, const uint8_t *M_test, int device,
                          insider_hip_handle **out);
void insider_hip_destroy(insider_hip_handle *h);

/* A second handle on the SAME resident data set: the read-only device arrays insider_hip_create built (X, mask codes,
 * held-out lists, level sums, pair counts: all of it) are shared, the factor workspace, the streams and the options (copied
 * from `src` as they stand) are the clone's own.  Handles of one data set may run insider_hip_optimize() at the same time
 * from different host threads: tune()'s grid points (R/insider.R:142-174) are independent fits of one data set, and a
 * data set of the size real INSIDER inputs have (377 x 5000 ... 44477, README.md:30) does not fill the GPU with one fit.
 * Every handle is destroyed with insider_hip_destroy(); the data set is freed with the last of them.  Results of a fit do
 * not depend on which handle ran it or on what ran beside it. */
int insider_hip_clone(insider_hip_handle *src, insider_hip_handle **out);

/* A handle on a NEW data set over the SAME resident X: the mask-independent device arrays of src's data set (X, the level
 * and chunk tables, the all-entry sums, the pair counts) are shared — not copied, not uploaded again; the codes, held-out
 * lists, train sums, group tables and per-gene counts are built for the new masks (n x p uint8 column-major, as for
 * insider_hip_create) by the stages insider_hip_create_ex runs.  Workspace, streams and options as insider_hip_clone (options
 * copied as they stand).  src may be a clone or itself a re-masked handle; either may be destroyed first; the shared arrays
 * go with the last handle that uses them.  A fit on the new handle is bit-identical to one on a handle that
 * insider_hip_create_ex made from the same inputs.  A sharded src (world > 1): INSIDER_ERR_UNSUPPORTED.
 * insider_hip_get_info "data_bytes_shared" / "data_bytes_own": device bytes of the handle's data set that it holds jointly
 * with its source / that it allocated itself (the first is 0 for a handle of insider_hip_create_ex). */
int insider_hip_remask(insider_hip_handle *src, const uint8_t *M_train, const uint8_t *M_test, insider_hip_handle **out);

/* Fold ids of the resident matrix: n x p uint8 column-major, 0 = NA, 1..F = the fold the entry is held out in (F <= 255).
 * Stored once on the device in the layout of X, with the shared part of the data set (clones of h see them).  Values above
 * F: INSIDER_ERR_ARG.  Calling it again replaces the ids for handles derived afterwards. */
int insider_hip_set_folds(insider_hip_handle *h, const uint8_t *fold_id, int F);
/* Re-mask by fold, nothing uploaded: test = entries whose id == fold, train = entries with any other id >= 1, NA = id 0.
 * Otherwise as insider_hip_remask (the new handle carries the ids too).  fold outside 1..F or no ids set: INSIDER_ERR_ARG. */
int insider_hip_remask_fold(insider_hip_handle *src, int fold, insider_hip_handle **out);

/* Gene-axis sharding: this handle holds genes [gene_offset, gene_offset + p) of the global
 * matrix.  gene_offset keys the per-gene sweep order so results do not depend on the sharding.  `fn` (may be
 * NULL when world == 1, or when insider_hip_comm_init() supplies the exchange) is called once per covariate per outer
 * iteration (level normal equations) and once per checkpoint (loss terms).  A non-NULL `fn` replaces a communicator
 * installed earlier by insider_hip_comm_init(). */
int insider_hip_set_shard(insider_hip_handle *h, int64_t gene_offset, int rank, int world, insider_allreduce_fn fn,
                          void *user);

/* In-library RCCL (the collective BASELINE.json's north star names): the per-covariate level equations and the loss
 * terms are summed over the gene-sharded ranks by ncclAllReduce ENQUEUED ON THE LIBRARY'S OWN STREAM, between the kernels
 * that produce and consume them; the callback of insider_hip_set_shard() is then not used (it remains as the fallback
 * for hosts that bring their own communicator).  Rank 0 obtains an id with insider_hip_comm_unique_id(), the host
 * distributes those INSIDER_COMM_ID_BYTES bytes to every rank by any means (insider_amd/dist.py: one broadcast over
 * torch.distributed), and every rank calls insider_hip_comm_init() after insider_hip_set_shard(h, offset, rank, world,
 * NULL, NULL).  Collective call: returns when all `world` ranks have joined.  The communicator is destroyed with the
 * handle. */
#define INSIDER_COMM_ID_BYTES 128
int insider_hip_comm_unique_id(void *out, int out_bytes);
int insider_hip_comm_init(insider_hip_handle *h, const void *unique_id, int rank, int world);

/* Options: "max_sweeps" (safety cap on the sweeps of one elastic-net subproblem, default 2^24: the reference's loop has none,
 * src/coordinate_descent.cpp:86-114, and neither does this library in practice — the sweep-order table holds one period of
 * the order sequence, INSIDER_PERM_PERIOD = 16384 rows, whatever the cap; insider_hip_get_info("cap_hits") counts the solves
 * of the last call that the cap ended), "order_mode" (0 = hashed random order of
 * include/insider_perm.h, 1 = cyclic), "profile" (1 = time the statistics / solve kernels with HIP events),
 * "verbose" (1 = print the reference's per-checkpoint lines to stdout), "cd_variant" (elastic-net sweep kernel:
 * 0 = four genes per wavefront with the Gram matrix in registers [K <= 32; 32 < K <= 48 with the third coordinate slot's
 * columns in LDS], 2 = four genes per wavefront with the Gram matrix in LDS [K <= 48], 1 = one lane group per gene [also
 * what K > 48 takes]; all three follow the same sweep orders and agree to rounding), "row_merged" (1, default = masked
 * row update from per-(level, gene) weighted terms, 0 = from per-sample statistics; same results), "col_factored" (1,
 * default = a cost model picks the form of the column-side masked Gram statistics, 0 = one rank-one update per held-out
 * entry, 2 = per-(covariate, level) terms with one table look-up per entry, 3 = per-(covariate, level) terms from the
 * gene's dense level-pair counts [falls back to 2 when a count exceeds one byte]; same results), "row_counts" (1, default = the merged row update takes its per-gene level sums from the dense
 * level-pair counts when they exist, 0 = from the entry lists; same results), "force_allreduce" (1 = call the all-reduce callback even
 * when world == 1: plumbing rehearsal), "row_fused" (1, default = the merged row update forms a level's equations and
 * solve in one launch; with tuning = 0 the whole unmasked row update of a covariate is that one launch; 0 = separate launches),
 * "list_fine" (1, default = the per-entry statistics kernel uses the 4x4x4 form of the f64 matrix instruction for 16 <= K <= 31
 * [fewer wasted outputs than 16 x 16 blocks], 0 = the 16x16x4 form; same sums in another order), "row_gemm" / "row_gemm_waves" (1, default = the per-level weighted Gram sums of a covariate with >= 49
 * levels come from one GEMM over genes, cut into row_gemm_waves [1024] waves; 0 = one weighted rank-one update per (level, gene);
 * same sums in another order, results agree to rounding), "col_mfma4" (1, default = the pair-count column statistics [K <= 31, the
 * factor rows of all covariates within 64 KB of LDS] form sum_l a_l p_l' on the 4x4x4 form of the f64 matrix instruction, rows read
 * in four rotations from LDS, resident blocks whose waves draw genes by ticket; 0 = the 16x16x4 form; same sums to rounding),
 * "stats_own_q" (1, default = that kernel [categorical covariates, one rank, K not 15 or 31, at most four k-steps] forms each
 * gene's rows of S A and S^held A itself, in two free columns of its second product, in the calls that run a column solve, so
 * the two products over the genes and their stream joins are not launched; 2 = in insider_hip_col_stats too — with 1 that entry
 * keeps the products for no other reason than that insider_hip_get_info's facts about the last product over the genes go on
 * reporting a launch after it, which the suite's cases of the streaming products read; 0 = the products; same sums in another
 * order),
 * "mm_fast" (1, default = the streaming products of the row phase [V = C A', S A, U'C, S'C: from 16384 rows on] stage their small
 * operand in LDS once per block and read the tall one in 16-byte pieces / several column tiles per wave; 0 = round 4's kernels;
 * same sums, the row products in another order), "mm_tiles" (0, default = a wave of k_mm_rows2 takes one tile of 16 rows until
 * the grid holds two waves per SIMD, then as many as keep it there; t >= 1 = t tiles per wave, in S A and in V = C A'; a tile's sums
 * do not depend on the wave that takes it: same bits), "cd_pairs" (1, default = the register-resident sweep kernel [K <= 30] is routed through its blocks of TWO
 * coordinate steps wherever two consecutive coordinates of a sweep's order share a coordinate slot: a third fewer computed jumps,
 * the same steps in the same order — bit-identical iterates; 0 = one step per block), "cd_pass1" / "cd_pass_ratio" / "cd_cold_iters" (multi-pass column solves in the first
 * cd_cold_iters outer iterations of a call [default 3]: the register-resident sweep kernel stops at sweep cd_pass1 [64; 0 = one
 * pass], cd_pass1 x ratio [4], ..., re-packing the genes still running by their estimated remaining length between passes;
 * the iterates are bit-identical to the single-pass solve), "resid_stage_mb" (size in MB of the device buffer
 * insider_hip_residual() copies the residual out through, default 256; at least 16 genes of the window), "vd_stage_kb" (LDS budget in
 * KiB for the level tables insider_hip_variance_decomposition() stages per block, default 48, at most 60; tables that do not
 * fit are read from global memory instead, with the same result; 0 = always that form; insider_hip_sample_decomposition()
 * stages its groups of genes' tables under the same budget), "sd_slabs" (gene slabs the streaming pass of
 * insider_hip_sample_decomposition() is cut into, summed in slab order; 0, default = from n, p and the device's compute units;
 * at most 256 and at most p; another count gives the same sums in another order), "ls_slabs" / "ls_part_mb" (gene slabs the
 * streaming pass of insider_hip_level_scores() is cut into, summed in slab order; 0, default = the rule of "sd_slabs" on that
 * pass's sample tiles, lowered until the slabs' partial scores [slabs x n x the levels padded to 16, doubles] stay within
 * ls_part_mb MB, default 256: a memory budget, not a tuned value; a count given explicitly is used as it is, at most 256 and at
 * most p; another count gives the same sums in another order), "rc_slabs" (gene slabs the forward pass of
 * insider_hip_residual_products() is cut into, summed in slab order; 0, default = the rule of "ls_slabs" with the partial Y
 * [slabs x n x q padded to 16, doubles] kept within ls_part_mb MB; a count given explicitly is used as it is, at most 256 and at
 * most p; another count gives the same sums in another order), "glm_slabs" (gene slabs the streaming pass of
 * insider_hip_interaction_glm() is cut into, summed in slab order; 0, default = from n and the device's compute units, at most
 * 64; s >= 1 [at most 64] = slabs of cdiv(p, s) genes rounded up to whole staging rounds of k_resid_stats; another count gives
 * the same sums in another order). */
int insider_hip_set_option(insider_hip_handle *h, const char *name, double value);

/*
 * The reference's optimize() (src/optimize.cpp:255-422; .Call symbol _insider_optimize,
 * src/RcppExports.cpp:87-110) for categorical covariates.  Same argument meaning:
 *   A            c pointers, A[i] is L_i x K column-major, IN/OUT (the reference mutates cfd_factors in place,
 *                src/optimize.cpp:283-284)
 *   C            K x p column-major, IN/OUT (column_factor, mat&)
 *   lambda1/lambda2/alpha/tuning/global_tol/sub_tol/max_iter as src/optimize.cpp:256-257
 *                (max_iter + 1 outer iterations are run: `iter <= max_iter`, :325)
 *   seed         replaces Rcpp::RNGScope / R's global RNG (src/RcppExports.cpp:90)
 *   out_*        train_rmse, test_rmse (NaN when tuning = 0: uninitialised in the reference, :264), loss.  The sums of
 *                squared residuals behind them are formed from statistics as differences of sums of squares: their error
 *                is absolute, of the order 2^-52 * sum x^2 (an RMSE far below sqrt(2^-52 * sum x^2 / count) is noise), and a
 *                per-gene sum that comes out negative counts as 0, so no RMSE is NaN for it; only the test sum of data with
 *                NA entries is formed from explicit residuals and is accurate relative to itself
 *   traj         optional, traj_cap rows of INSIDER_TRAJ_STRIDE doubles; out_traj_rows rows written
 *   out_iters    value of `iter` when the loop ended
 * inc_continuous must be 1 exactly when the handle was created with continuous covariates
 * (insider_hip_create_ex); each column j is then updated after the categorical covariates by
 * optimize_continuous_v2 (src/optimize.cpp:76-137,340-351): cyclic scalar CD to sum|du| < 0.1 (tuning = 1) or one
 * ridge solve (tuning = 0).  The one-shot form takes categorical covariates only.
 */
int insider_hip_optimize(insider_hip_handle *h, double *const *A, double *C, int inc_continuous, int K,
                         double lambda1, double lambda2, double alpha, int tuning, double global_tol, double sub_tol,
                         uint32_t max_iter, uint64_t seed, double *out_train_rmse, double *out_test_rmse,
                         double *out_loss, double *traj, int traj_cap, int *out_traj_rows, int *out_iters);

/* One-shot form with the reference's 16 logical arguments (create + optimize + destroy): the direct replacement of
 * .Call(`_insider_optimize`, ...) (src/RcppExports.cpp:87-110, R/RcppExports.R:20-22) that r/insider_hip_shim.c binds.
 *   ctns / m     ctns_confounder (n x m column-major); read only when inc_continuous = 1, exactly as the reference
 *                ignores it otherwise (src/optimize.cpp:276-291); A then carries c + 1 pointers (the last one m x K)
 *   device       HIP device ordinal
 * insider_hip_optimize_oneshot() is the same for categorical covariates on device 0. */
int insider_hip_optimize_oneshot_ex(const double *X, int64_t n, int64_t p, double *const *A, double *C,
                                    const int32_t *levels, int c, const int32_t *n_levels, const double *ctns, int m,
                                    const uint8_t *M_train, const uint8_t *M_test, int inc_continuous, int K,
                                    double lambda1, double lambda2, double alpha, int tuning, double global_tol,
                                    double sub_tol, uint32_t max_iter, uint64_t seed, int device, double *out_train_rmse,
                                    double *out_test_rmse, double *out_loss);
int insider_hip_optimize_oneshot(const double *X, int64_t n, int64_t p, double *const *A, double *C,
                                 const int32_t *levels, int c, const int32_t *n_levels, const uint8_t *M_train,
                                 const uint8_t *M_test, int inc_continuous, int K, double lambda1, double lambda2,
                                 double alpha, int tuning, double global_tol, double sub_tol, uint32_t max_iter,
                                 uint64_t seed, double *out_train_rmse, double *out_test_rmse, double *out_loss);

/*
 * The two block updates as stand-alone operators (the reference's internal optimize_row / optimize_col, reachable
 * there only through optimize()).  Both take the factors in the host layout of insider_hip_optimize.
 *
 * insider_hip_optimize_row — one row update of covariate `cov` (src/optimize.cpp:139-198 as called at :339): the
 *   residual is X minus the contributions of every other covariate as passed in A; A[cov] (L_cov x K) is replaced by
 *   the per-level solutions of (sum_{r in level}(CC' - C_z C_z') + lambda I) a = sum_r C_nz resid[r, nz] (tuning = 1)
 *   or (|level| CC' + lambda I) a = sum_r C resid[r, :]' (tuning = 0).  lambda = 0 with the other
 *   factors zero is fit_interaction()'s arithmetic (src/fit_interaction.cpp:10-90, which applies no ridge term).  The
 *   solve is solve(..., likely_sympd): a system that is not positive definite (lambda <= 0) takes the general route.
 *   cov in [c, c+m) with inc_continuous = 1 updates row cov-c of the continuous factor (optimize_continuous_v2,
 *   src/optimize.cpp:76-137).  Returns INSIDER_ERR_SOLVE when a level's system is singular to working precision.
 * insider_hip_optimize_col — one column update (src/optimize.cpp:200-253 as called at :376): every gene's
 *   elastic-net regression of X[:, j] on the row factor R = sum_i Z_i A_i over its training entries, warm-started
 *   at C[:, j] (alpha > 0), or the ridge solve (alpha == 0); C is updated in place.  `iter` picks the sweep-order
 *   stream of include/insider_perm.h (optimize() passes its outer iteration number).
 */
int insider_hip_optimize_row(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K, int cov,
                             double lambda, int tuning);
int insider_hip_optimize_col(insider_hip_handle *h, double *const *A, double *C, int inc_continuous, int K,
                             double lambda, double alpha, int tuning, double tol, uint64_t seed, uint32_t iter);

/*
 * strong_coordinate_descent (src/coordinate_descent.cpp:56-127; .Call symbol
 * _insider_strong_coordinate_descent, src/RcppExports.cpp:35-50), batched: nprob independent K-variable
 * elastic-net subproblems solved in covariance form from (XtX, Xty), by the kernels of the column update
 * (insider_hip_last_cd_solver() says which) — the design matrix X and outcome y of the reference signature
 * enter only through XtX = X'X and Xty = X'y, which the reference's callers always pass alongside
 * (src/optimize.cpp:228,246), so they are not taken here.
 *   XtX    nprob blocks of K x K (column-major; symmetric: only the upper triangle is read), Xty / wstart /
 *          beta_out nprob blocks of K
 *   seed, iter  key the per-sweep coordinate order (include/insider_perm.h; the same for every subproblem)
 *   sweeps_out  optional, nprob ints
 */
int insider_hip_strong_cd(const double *XtX, const double *Xty, const double *wstart, int K, int64_t nprob,
                          double lambda, double alpha, double tol, uint64_t seed, uint32_t iter, int order_mode,
                          int max_sweeps, int device, double *beta_out, int32_t *sweeps_out);
/* The same solver with the reference's eight arguments, one subproblem (.Call `_insider_strong_coordinate_descent`,
 * src/RcppExports.cpp:35-50: X, y, wstart, lambda, alpha, XtX, Xty, tol): X is m x K column-major, y has m entries.
 * XtX / Xty may be NULL: they are then formed on the device as X'X and X'y (what the reference's callers pass,
 * src/optimize.cpp:219-222,234-235).  When they are given, X and y may be NULL. */
int insider_hip_strong_cd_xy(const double *X, const double *y, int64_t m, int K, const double *wstart, double lambda,
                             double alpha, const double *XtX, const double *Xty, double tol, uint64_t seed, uint32_t iter,
                             int order_mode, int max_sweeps, int device, double *beta_out, int32_t *sweeps_out);

/* solve(A, b, solve_opts::likely_sympd) as the row / ridge updates use it (src/optimize.cpp:175,190,226,240;
 * src/fit_interaction.cpp:54), batched: nsys systems of K x K (column-major) with one right-hand side each.  The
 * positive-definite route (Cholesky) first; when a pivot is not positive, the general route (Gaussian elimination with
 * partial pivoting) — Armadillo's documented behaviour.  route (optional, nsys ints): 0 = Cholesky, 1 = general, -1 =
 * singular (status INSIDER_ERR_SOLVE; route and the other systems' x are filled in all the same).  K <= 64.  This is
 * insider_hip_solve_sympd_form(..., lambda = 0, form = 0): the stand-alone kernel k_solve_batch, which runs the LDS
 * Cholesky and the pivoted elimination at row pitch K.  The updates of the fit reach the same two routines at pitch KP,
 * and a register Gauss-Jordan for K <= 31, through k_level_solve: form = 1 below. */
int insider_hip_solve_sympd(const double *A, const double *b, int K, int64_t nsys, int device, double *x, int32_t *route);

/* The same solve of (A + lambda I) x = b with the kernel chosen by the caller; lambda is added on the device.
 *   form = 0  k_solve_batch, K <= 64; A may be non-symmetric (the general route then solves A x = b).
 *   form = 1  the fit's own level solve, K <= 63: every system is packed as the level equation record of the row update
 *             (KP = 16 ceil((K + 1) / 16); KP KP + KP doubles, zeros outside K; a level count of 1) and k_level_solve<NB>
 *             is launched as the row update launches it: the register Gauss-Jordan for K <= 31, the LDS Cholesky at pitch
 *             KP for K >= 32, the pivoted elimination at pitch KP on a reloaded system after a non-positive pivot.
 *             SYMMETRIC INPUT ONLY: the register route reads the record by columns, the LDS routes by rows.  The x of a
 *             singular system is returned as zeros.
 * route and the status are those of insider_hip_solve_sympd.  Input must be finite. */
int insider_hip_solve_sympd_form(const double *A, const double *b, int K, int64_t nsys, double lambda, int form, int device,
                                 double *x, int32_t *route);

/* optimize_continuous_v2 with the reference's eight arguments (src/optimize.cpp:76-137; .Call symbol
 * `_insider_optimize_continuous_v2`, src/RcppExports.cpp:69-85, R/RcppExports.R:16-18): the update of ONE continuous
 * covariate's K-vector against an arbitrary n x p matrix `data` (inside optimize() it is the Gauss-Seidel residual with this
 * column's own contribution added back, src/optimize.cpp:344-345).
 *   data             n x p column-major
 *   indicator        n x p uint8, non-zero = the entry takes part (train_indicator); read only when tuning = 1
 *   updating_factor  K doubles, IN/OUT (the reference's rowvec&)
 *   c_factor         K x p column-major (column_factor)
 *   updating_confd   n doubles (one column of ctns_confounder)
 *   gram             K x K column-major (column_factor column_factor'); read only when tuning = 0, exactly like the reference
 * tuning = 1: cyclic scalar passes u_i = Xty_i / (XtX_i + lambda) over the masked entries until sum |du| < 0.1 (:102-126);
 * tuning = 0: one solve of ((z'z) gram + lambda I) u = C data' z (:127-131, solve(..., likely_sympd)).  Any other value:
 * INSIDER_ERR_ARG (the reference prints and exit(1)s, :133-136).  Inside a fit the same update runs on the resident data set
 * (insider_hip_optimize / insider_hip_optimize_row with cov >= c); this entry uploads its arguments, runs and frees. */
int insider_hip_optimize_continuous_v2(const double *data, int64_t n, int64_t p, const uint8_t *indicator,
                                       double *updating_factor, const double *c_factor, int K, const double *updating_confd,
                                       const double *gram, double lambda, int tuning, int device);

/*
 * The masked Gram / XtY reductions on their own (for parity tests and profiling).
 * Column side (src/optimize.cpp:216-222): for every gene j, XtX_j = R'R - sum_{i: M_train[i,j]=0} r_i r_i',
 * Xty_j = sum_i M_train[i,j] x_ij r_i.   R is n x K column-major (row_factor).
 *   G_out  p blocks of K x K column-major, q_out p blocks of K.
 * Row side (src/optimize.cpp:162-171 with the data matrix in place of the Gauss-Seidel residual): for every
 * sample r, XtX_r = CC' - sum_{j: M_train[r,j]=0} c_j c_j', Xty_r = sum_j M_train[r,j] x_rj c_j.
 *   C is K x p column-major;  H_out n blocks of K x K, b_out n blocks of K.
 */
int insider_hip_masked_gram_cols(insider_hip_handle *h, const double *R, int K, double *G_out, double *q_out);
int insider_hip_masked_gram_rows(insider_hip_handle *h, const double *C, int K, double *H_out, double *b_out);

/*
 * The column-side statistics the column solve of insider_hip_optimize_col() (tuning = 1) reads, from the row factors A
 * alone (as in insider_hip_optimize(); no column factor): R = sum_i Z_i A_i (+ Z_c A_c, inc_continuous = 1), R'R, X'R, then
 * the statistics kernel the handle's options pick (insider_hip_get_info "col_stats_kernel") and its record densified.  For
 * every gene j with training entries T(j):
 *   G_out  p blocks of K x K column-major: sum_{i in T(j)} r_i r_i';
 *   q_out  p blocks of K: sum_{i in T(j)} x_ij r_i;
 *   ss_out p doubles: sum_{i not in T(j)} x_ij^2 (held-out and NA entries; what the test SSE starts from).
 * Writes the workspace buffers insider_hip_optimize_col() overwrites and nothing else an optimize() reads.  A sharded handle
 * (world > 1) returns INSIDER_ERR_UNSUPPORTED.
 */
int insider_hip_col_stats(insider_hip_handle *h, double *const *A, int inc_continuous, int K, double *G_out, double *q_out,
                          double *ss_out);

/*
 * glm_interaction() (R/glm_interaction.R:2-30) on the resident data set: per-level coefficients and standard errors of
 * interaction effects on the metagenes, without the residual matrix ever leaving the device.
 *   Covariate blocks are numbered 0..c-1 (the categorical covariates) and, with inc_continuous = 1, c (the continuous
 *   block): the order of A in insider_hip_optimize().  subtract holds one int32 flag per block (c + inc_continuous).
 *   The residual is r_ij = X_ij - (sum_{b: subtract[b] != 0} u_b(i)) C[:, j] with u_b(i) = A_b[level_b(i)] for a
 *   categorical block and u_c(i) = z_i B for the continuous one.  X is the handle's matrix as given to
 *   insider_hip_create[_ex]: every entry, whatever the masks say (glm_interaction ignores train_indicator).
 * insider_hip_residual — residual rows [row_begin, row_end) of X, written column-major ((row_end - row_begin) x p, leading
 *   dimension row_end - row_begin) to host `out`.  The rows stream through a device buffer of option "resid_stage_mb"
 *   (default 256) in slabs of genes.
 * insider_hip_interaction_glm — group is an int32 vector of n ids in 0..G (0 = the sample is in no group; anything else:
 *   INSIDER_ERR_ARG).  For every group g with m_g samples: G = C C', beta_g = G^-1 C mean_{i in g}(r_i),
 *   RSS_g = sum_{i in g} ||r_i - C' beta_g||^2, dof_g = m_g p - rank, se_g = sqrt(RSS_g / dof_g diag(G^-1) / m_g).
 *   RSS_g is formed as sum ||r_i||^2 - m_g beta_g' C mean(r_i); where the group's residual rows lie in the row space of C
 *   that difference cancels to rounding noise of either sign, and a negative one is returned as 0 (se = 0, never NaN).
 *   coeff and se are G x K column-major (row g-1 for id g, like the factors), dof has G entries.  A group without samples
 *   gives zero rows and dof 0.  A latent dimension whose row of C is exactly zero is dropped from G (rank counts the
 *   others) and its coefficient and standard error are NaN (R's glm reports NA); any other pivot of the Cholesky
 *   factorisation of the reduced G that is not larger than rank x machine epsilon times its diagonal entry returns
 *   INSIDER_ERR_SOLVE, and so does a C with more non-zero rows than genes (the reduced G is then rank-deficient whatever
 *   rounding leaves in its last pivots).  p-values are left to the caller: 2 P(T_dof > |coeff / se|).
 * Both work on any handle (clones included), on the handle's main stream, with a workspace of their own (allocated on first
 * use, freed by insider_hip_destroy): nothing insider_hip_optimize() reads is touched, and an optimize() after them is
 * bit-identical to one without.  K is bounded as in insider_hip_optimize() (1..63).  A sharded handle (world > 1) returns
 * INSIDER_ERR_UNSUPPORTED.
 */
int insider_hip_residual(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                         const int32_t *subtract, int64_t row_begin, int64_t row_end, double *out);
int insider_hip_interaction_glm(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                const int32_t *subtract, const int32_t *group, int G, double *coeff, double *se,
                                double *dof);

/*
 * Per-gene variance decomposition of a fitted model on the resident data set.  Covariate blocks are numbered as in
 * insider_hip_residual(): 0..c-1 the categorical covariates, c the continuous block (inc_continuous = 1); B = c +
 * inc_continuous.  For sample i and gene j, block b contributes g_b(i,j) = A_b[level_b(i)] . C[:, j] (categorical) or
 * g_c(i,j) = z_i B_c C[:, j] (continuous: z_i = row i of ctns_confounder, B_c = A[c], m x K).  The fit is f = sum_b g_b
 * and the residual r = x - f, with x the handle's X as given to insider_hip_create[_ex].
 * entries chooses the entries S_j of each gene: 0 = every entry, 1 = entries whose train bit is set (the handle's
 * train_indicator), 2 = entries whose test bit is set (test_indicator).  On a handle built for fit() (train = train + test,
 * test = NA) 1 is the observed set; on a tuning handle 2 is each gene's held-out set.
 * out holds p records of 4 + 3 B doubles, record j at out + j (4 + 3 B): n_j = |S_j|, sum x, sum x^2, sum r^2 (formed from
 * r itself), then for b = 0..B-1 at 4 + 3 b: sum g_b, sum g_b^2, sum r g_b.  All sums run over S_j.
 * Arguments, status codes and scope as in the post-hoc calls above (K 1..63, the same inc_continuous rules, a sharded
 * handle returns INSIDER_ERR_UNSUPPORTED); entries outside 0..2 return INSIDER_ERR_ARG.  Works on clones, on the handle's
 * main stream, in the post-hoc workspace: an optimize() after it is bit-identical to one without.  Every sum runs in a fixed
 * order without atomics: repeated calls give bit-identical records.  insider_hip_get_info("vd_path") tells which form of
 * the streaming pass the last call ran (1 = level tables staged in LDS, 2 = read from global memory; option "vd_stage_kb").
 */
int insider_hip_variance_decomposition(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                       int entries, double *out);

/*
 * Per-sample fit diagnostics of a fitted model on the resident data set: the record of insider_hip_variance_decomposition()
 * along the other axis.  Blocks, g_b(i,j), f, r, x and the meaning of entries are those of that call; S_i is the set of genes j
 * whose entry (i, j) is selected.
 * out holds n records of 4 + 3 B doubles, record i at out + i (4 + 3 B): n_i = |S_i|, sum x, sum x^2, sum r^2 (formed from r
 * itself), then for b = 0..B-1 at 4 + 3 b: sum g_b, sum g_b^2, sum r g_b.  All sums run over S_i.  Summed over the samples, a
 * slot equals the same slot of the per-gene records summed over the genes (to rounding).
 * Arguments, status codes and scope as in insider_hip_variance_decomposition() (K 1..63, the same inc_continuous rules, entries
 * outside 0..2 and a null out return INSIDER_ERR_ARG, a sharded handle returns INSIDER_ERR_UNSUPPORTED).  Works on clones and
 * re-masked handles, on the handle's main stream, in the post-hoc workspace: an optimize() after it is bit-identical to one
 * without.  The pass is one stream over X and the mask codes on a grid of sample tiles x gene slabs; the slabs' partial records
 * are summed in slab order, without atomics: repeated calls with the same options on the same device give bit-identical
 * records.  The slab count follows from n, p, the device's compute units and option "sd_slabs" alone;
 * insider_hip_get_info("sd_slabs") tells the count of the last call and "sd_path" the form of its pass (1 = level tables
 * staged in LDS in groups of genes, 2 = read from global memory; option "vd_stage_kb"; both forms give the same bits).
 */
int insider_hip_sample_decomposition(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                     int entries, double *out);

/*
 * Every sample scored against every level of one categorical covariate, on the resident data set: how well is the row of
 * sample i explained when its embedding for covariate cov is replaced by each candidate embedding in turn?  Blocks, u_b(i), x,
 * entries (0 all / 1 train bit / 2 test bit) and S_i, the set of selected genes of sample i, are those of
 * insider_hip_sample_decomposition().
 *   cov    a CATEGORICAL block, 0 <= cov < c.
 *   cand   the candidates e_1 .. e_L in R^K: NULL (with n_cand = 0) = the rows of A[cov], L = n_levels[cov]; else the rows of
 *          cand (n_cand x K, column-major like a factor), L = n_cand >= 1: any embeddings in the model's latent space.
 * With d_ij = x_ij - sum_{b != cov} u_b(i) . C[:, j] (the continuous block included when inc_continuous = 1):
 *   sse[i][l] = sum_{j in S_i} (d_ij - e_l . C[:, j])^2      n x L, column-major (leading dimension n)
 *   cnt[i]    = |S_i|                                        n doubles
 * A sample with S_i empty gets a row of zeros and cnt = 0.  The device sums the expanded form (below), whose three terms
 * cancel when a candidate fits a sample almost exactly: a sum that comes out negative is returned as 0, so sse >= 0 always, and
 * a value that small carries the absolute error of the tolerance (about 1e-16 of sum (|x| + |fit| + |e_l . C|)^2), not its own
 * digits.  The column of a sample's assigned level is the rss of
 * insider_hip_sample_decomposition() (to rounding).  A sample's own level was fitted WITH that sample: on the entries the fit
 * used the assigned level is favoured, most for levels with few samples (a level with one sample fits itself); on a tuning
 * handle entries = 2 scores on entries no embedding has seen.  The call reports this nowhere and corrects nothing.
 * Status codes: the checks of the post-hoc calls above (K 1..63: K > 63 returns INSIDER_ERR_UNSUPPORTED; the same
 * inc_continuous rules; entries outside 0..2 returns INSIDER_ERR_ARG; a sharded handle returns INSIDER_ERR_UNSUPPORTED); cov
 * outside 0..c-1 (the continuous block included), cand != NULL with n_cand < 1, cand == NULL with n_cand != 0 and a NULL sse or
 * cnt return INSIDER_ERR_ARG.  Nothing is written to the caller's arrays unless the status is INSIDER_OK.  Works on clones and
 * re-masked handles, on the handle's main stream, in the post-hoc workspace: an optimize() after it is bit-identical to one
 * without.
 * The device forms the candidate table Tc = cand C and, in one streaming pass over X and the mask codes per window of 128
 * levels, sse = sum M d^2 - 2 (M .* d) Tc + M (Tc .* Tc) (M the 0/1 selection) as two masked products over the genes on the
 * f64 matrix instruction, the fit of a tile from the same instruction, on a grid of sample tiles x gene slabs x windows; the
 * slabs' partial scores are summed in slab order.  Every sum runs in a fixed order without atomics: repeated calls with the same
 * options on the same device return identical bits, and cand equal to A[cov] returns the same bits as cand == NULL.
 * insider_hip_get_info("ls_path") tells the form of the last call (1 = one level window, X read once; 2 = several, X read once
 * per window of 128 levels) and "ls_slabs" its gene slabs (options "ls_slabs", "ls_part_mb").
 */
int insider_hip_level_scores(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                             int entries, int cov, const double *cand, int n_cand, double *sse, double *cnt);

/*
 * Per-factor decomposition of a fitted model on the resident data set: the record of
 * insider_hip_variance_decomposition() split along the K latent factors.  Blocks b = 0..B-1 (B = c + inc_continuous) have the
 * per-sample embeddings u_b(i) in R^K (A_b[level_b(i)] for a categorical block, z_i B_c for the continuous one); one more
 * block b = B, the total, has u_B(i) = sum_b u_b(i), row i of the row factor.  Factor k contributes
 * h_{b,k}(i, j) = u_b(i)[k] C[k][j] through block b; the fit is f = sum_k h_{B,k} and r = x - f.  S_j, A, C, entries as in
 * insider_hip_variance_decomposition().
 * out: p records of 4 + 3 (B + 1) K doubles, record j at out + j (4 + 3 (B + 1) K): n_j = |S_j|, sum x, sum x^2, sum r^2
 * (formed from r itself), then for b = 0..B, k = 0..K-1 at 4 + 3 (b K + k): sum h_{b,k}, sum h_{b,k}^2, sum r h_{b,k}.  All
 * sums run over S_j.  The total's sum h and sum r h are the sums of the blocks' slots in block order; its sum h^2 is formed
 * from u_B itself (it carries the cross terms between blocks).  A factor whose row of C is zero has slots that are 0.
 * Arguments, status codes and scope as in the post-hoc calls above (K 1..63, the same inc_continuous rules; entries outside
 * 0..2 and a null out return INSIDER_ERR_ARG, a sharded handle returns INSIDER_ERR_UNSUPPORTED).  Works on clones and
 * re-masked handles, on the handle's main stream, in the post-hoc workspace: an optimize() after it is bit-identical to one
 * without.  Per gene the device forms (M_j .* r_j)' W, M_j' W and M_j' (W .* W) against W = [U_0 | ... | U_B] on the f64
 * matrix instruction: a heavy pass over X and the mask codes (the fit of a tile from the same instruction) and a light pass
 * over the codes alone, each in windows of at most 128 columns of W.  Every sum runs in a fixed order without atomics:
 * repeated calls on the same device give bit-identical records.  insider_hip_get_info("fd_path") tells the form of the heavy
 * pass of the last call: 1 = the B K columns fit one window (X is read once), 2 = several windows (X is read once per window
 * of 128 columns).
 */
int insider_hip_factor_decomposition(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                     int entries, double *out);

/*
 * The masked, standardised residual of a fitted model as an operator on a block of vectors: the two thin products of one step
 * of a subspace iteration for the leading singular directions of R (structure shared across samples and genes that the model
 * has left behind: an unmodelled batch, a hidden gradient, a missing interaction).  Blocks, u_b(i), f = sum_b g_b (in block
 * order), x and the meaning of entries (0 all / 1 train bit / 2 test bit) are exactly those of
 * insider_hip_variance_decomposition().  The working residual is
 *   r_ij = (x_ij - f_ij - center_j) / scale_j on the selected entries, 0 elsewhere.
 * center holds p doubles (NULL = 0), scale holds p doubles (NULL = 1); a gene whose scale is not finite or not > 0 is an
 * all-zero column of R (not an error, as in insider_hip_outliers()).  The device multiplies by 1 / scale_j.
 *   Q    n x q, column-major (leading dimension n), 1 <= q <= 64, every value finite.
 *   Z    = R' Q,       p x q, column-major (leading dimension p).
 *   Y    = R Z = R (R' Q), n x q, column-major (leading dimension n); may be NULL: the forward pass is then skipped and Z has
 *        the same bits as with it.
 *   rss  rss_j = sum_i r_ij^2, p doubles; may be NULL.
 * Status codes: the checks of the post-hoc calls above (K 1..63: K > 63 returns INSIDER_ERR_UNSUPPORTED; the same
 * inc_continuous rules; a sharded handle returns INSIDER_ERR_UNSUPPORTED); entries outside 0..2, a NULL Q or Z, q outside 1..64
 * and a value of Q that is not finite return INSIDER_ERR_ARG.  Nothing is written to the caller's arrays unless the status is
 * INSIDER_OK.  Works on clones and re-masked handles, on the handle's main stream, in the post-hoc workspace: an optimize()
 * after it is bit-identical to one without.
 * R is never stored.  Each product is one streaming pass over X and the mask codes on the f64 matrix instruction, the fit of a
 * 16 x 16 tile from the same instruction (K deep: the cost does not depend on the number of blocks or levels).  Z: a block owns
 * 64 genes and walks the samples in order, so a gene's sums have no partials.  Y: a grid of sample tiles x gene slabs, the
 * slabs' partial Y summed in slab order.  Every sum runs in a fixed order without atomics: repeated calls with the same options
 * on the same device return identical bits.  insider_hip_get_info("rc_slabs") tells the gene slabs of the last call's forward
 * pass (0 = skipped; option "rc_slabs") and "rc_ms" the HIP-event time of its kernels in milliseconds.
 */
int insider_hip_residual_products(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                  int entries, const double *center, const double *scale, const double *Q, int q,
                                  double *Z, double *Y, double *rss);

/*
 * Residual co-expression: the top-k correlated partners of every gene (axis 0) or of every sample (axis 1) in what a fitted
 * model has left behind (insider_amd/csrc/insider_coexpr.hpp).  The working residual is exactly that of
 * insider_hip_residual_products(): r_ij = (x_ij - f_ij - center_j) / scale_j on the selected entries, 0 elsewhere, the same
 * blocks in the same order, the same meaning of entries (0 all / 1 train bit / 2 test bit), center NULL = 0, scale NULL = 1, a
 * gene whose scale is not finite or not > 0 an all-zero column (its entries stay selected entries of value 0).
 *   axis 0  genes:   N = p vectors, the contraction runs over the samples;
 *   axis 1  samples: N = n vectors, the contraction runs over the genes.
 * Standardisation.  With m the number of selected entries of a vector: mean = (sum of r over the selected entries, in index
 * order) / m; the selected entries are centred by it, the unselected ones stay 0; the vector is divided by the root of its
 * centred sum of squares (index order).  A vector with m < 2 or a sum of squares that is not > 0 is DEAD: nobody's partner,
 * its own row all open slots.
 * Score.  The plain sum over the whole depth of the products of the standardised values; an entry missing in either vector
 * contributes 0.  With a full selection this is Pearson's r.  With missing entries it is the ZERO-FILLED correlation: |score|
 * <= 1 and it shrinks with missingness.  It is NOT the pairwise-complete correlation: that is
 * insider_hip_coexpression_pairwise() below (six products where this needs one).  Scores are not clipped: a correlation may
 * exceed 1 by rounding.
 *   idx_out / score_out  N x k, vector-major: row i lists the partners of vector i (never i itself) in descending score, equal
 *   scores (-0.0 == 0.0) by ascending index; a row with fewer than k eligible partners ends in -1 / NaN: the rules of
 *   insider_hip_neighbors().  1 <= k <= 64.
 * Status codes: the checks of the post-hoc calls above (K 1..63: K > 63 returns INSIDER_ERR_UNSUPPORTED; the same
 * inc_continuous rules; a sharded handle returns INSIDER_ERR_UNSUPPORTED); entries outside 0..2, axis outside 0..1, k outside
 * 1..64 and a NULL output return INSIDER_ERR_ARG.  Nothing is written to the caller's arrays unless the status is INSIDER_OK.
 * Works on clones and re-masked handles, on the handle's main stream: an optimize() after it is bit-identical to one without.
 * The standardised residual is staged once on the device in operand order: N and the depth rounded up to 64 and 32, 8 bytes
 * each (4 GB at n = 10000, p = 50000), allocated for the call and freed before it returns, outside the post-hoc workspace;
 * INSIDER_ERR_ALLOC when it cannot be allocated.  One streaming pass over X and the mask codes writes it (the fit of a 16 x 16
 * tile on the f64 matrix instruction), one pass over the staged buffer standardises it, and one product kernel forms every
 * score, K-independent, with the selection fused behind it: the N x N matrix never exists.  The score of a pair is one
 * accumulator chain over the depth in ascending order; no floating-point atomics: repeated calls return identical bits.
 * insider_hip_get_info: "cx_stage_mb" the staged bytes of the last call in MB, "cx_stage_ms" the HIP-event time of its staging
 * kernels and "cx_ms" that of its product kernel, in milliseconds.
 */
int insider_hip_coexpression(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                             int entries, const double *center, const double *scale, int axis, int k, int32_t *idx_out,
                             double *score_out);

/*
 * Pairwise-complete residual co-expression: insider_hip_coexpression() with Pearson's r of every pair taken over the entries
 * selected in BOTH vectors (insider_amd/csrc/insider_coexpr_pc.hpp).  The residual, entries, center, scale, axis, the
 * standardisation of a vector over its own selected entries and the rule for a DEAD vector are those of
 * insider_hip_coexpression(); the definition of the score, the eligibility of a pair (min_overlap >= 3, the variance floor),
 * the order and the open slots are those of insider_hip_gram_topk_pairwise() below, the depth being n (axis 0) or p (axis 1).
 *   idx_out / score_out / overlap_out  N x k, vector-major; overlap_out holds the pair's N = the number of jointly selected
 *   entries, -1 in an open slot.
 * Status codes: those of insider_hip_coexpression(), and INSIDER_ERR_ARG for min_overlap < 3 or a NULL overlap_out; a sharded
 * handle returns INSIDER_ERR_UNSUPPORTED.  Nothing is written to the caller's arrays unless the status is INSIDER_OK.  Works on
 * clones and re-masked handles, on the handle's main stream: an optimize() after it is bit-identical to one without.  The
 * staged buffer is that of insider_hip_coexpression(), an unselected entry and the padding held as NaN.
 * insider_hip_get_info: "cx_stage_mb" and "cx_stage_ms" as for insider_hip_coexpression() (the staging kernels here are
 * k_cx_stage and k_cx_std_pc), "cx_pc_ms" the HIP-event time of the product kernel k_cx_topk_pc in milliseconds.
 */
int insider_hip_coexpression_pairwise(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                                      int entries, const double *center, const double *scale, int axis,
                                      int64_t min_overlap, int k,
                                      int32_t *idx_out, double *score_out, int32_t *overlap_out);

/*
 * Aberrant entries of a fitted model on the resident data set: the (sample, gene) entries whose standardised residual the
 * model cannot explain.  Blocks, g_b(i,j), f = sum_b g_b (in block order), r = x - f, x, the meaning of entries (0 all / 1 train
 * bit / 2 test bit) and S_j are exactly those of insider_hip_variance_decomposition().
 * Standardised residual: z_ij = (r_ij - center_j) / scale_j.  center holds p doubles (NULL = 0), scale holds p doubles and is
 * required; a gene whose scale is not finite or not > 0 yields no call (not an error).  posthoc.residual_center_scale() derives
 * both from a variance-decomposition record.
 * Call: an entry in S_j with |z_ij| >= threshold; it is low when z < 0 and high when z > 0.  threshold must be finite and > 0.
 * Counts: *total = the number of calls (always written on success); gene_counts = p pairs {low, high}, sample_counts = n pairs
 * {low, high}; either may be NULL, and when present both are complete whatever cap is.
 * List: rows[t], cols[t] (0-based sample and gene) and z[t] hold the calls in ascending gene, then ascending sample.  Only the
 * first min(total, cap) calls are written and nothing beyond them.  cap = 0 with NULL list pointers is the counts-only form;
 * cap < 0, and cap > 0 with any NULL list pointer, return INSIDER_ERR_ARG.  total > cap is not an error: the caller compares
 * the two (and may call again with cap = total).
 * Arguments, status codes and scope as in the post-hoc calls above: K 1..63 (K > 63 returns INSIDER_ERR_UNSUPPORTED), the same
 * inc_continuous rules; entries outside 0..2, a NULL scale or a NULL total return INSIDER_ERR_ARG; a sharded handle returns
 * INSIDER_ERR_UNSUPPORTED.  No output is written when a status other than INSIDER_OK is returned for an argument.  Works on
 * clones and re-masked handles, on the handle's main stream, in the post-hoc workspace: an optimize() after it is bit-identical
 * to one without.
 * The device builds the level table, then makes one streaming pass over X and the mask codes that forms z per entry and writes
 * a bitmap of the calls (one bit per entry, n p / 8 bytes) and the per-gene counts; an exclusive scan of the genes' totals gives
 * 64-bit list offsets; a second pass reads the bitmap, not X, and for set bits only forms z again through the same device
 * function and stores the call at its offset + rank.  Membership is decided once, in the first pass, so the list of a gene is
 * exactly as long as its count.  The per-sample counts are integer atomics; everything else runs in a fixed order: repeated
 * calls on one device return identical bits for the list, the z values and the counts.  insider_hip_get_info("ol_path") tells
 * which form of the first pass the last call ran (1 = level tables staged in LDS, 2 = read from global memory; option
 * "vd_stage_kb", as for "vd_path").
 */
int insider_hip_outliers(insider_hip_handle *h, double *const *A, const double *C, int inc_continuous, int K,
                         int entries, const double *center, const double *scale, double threshold,
                         int64_t cap, int32_t *rows, int32_t *cols, double *z, int64_t *total,
                         int32_t *gene_counts, int32_t *sample_counts);

/* Top-k nearest neighbours of embeddings (insider_amd/csrc/insider_neighbors.hpp).  Handle-free, one device.
 *   Q (K x nq) and B (K x nb) are column-major: one embedding is K contiguous doubles, the layout of column_factor.  For every
 *   query the k base columns with the largest score, metric 0 = cosine (q.b / (|q| |b|)), 1 = dot (q.b).  idx_out / score_out
 *   are nq x k, query-major: row i lists the neighbours of query i in descending score, equal scores (-0.0 == 0.0) by ascending
 *   base index, so the answer is a pure function of the inputs.  self_offset = s >= 0: Q is the window B[:, s : s + nq] and
 *   query i never returns base index s + i (pass Q = B + s K and the matrix is uploaded once); -1: no exclusion.  A query with
 *   fewer than k eligible candidates ends its row with index -1 / score NaN.  Under cosine a zero-norm base column (its sum of
 *   squares is 0 in fp64) is nobody's neighbour and a zero-norm query gets a row of open slots; under dot zero columns are
 *   ordinary candidates of score 0.  Raw Euclidean distance is not offered: on unit-normalised columns it orders as cosine.
 *   The score of a pair is the same instruction sequence wherever the pair falls: repeated calls return identical bits, and a
 *   call on a window of the queries returns exactly the rows of the full call.  Device memory is O((nq + nb) K + nq k).
 *   INSIDER_ERR_ARG: a NULL pointer, K outside 1..63, k outside 1..64, nq < 0, nb < 1 or nb > INT32_MAX, an unknown metric,
 *   self_offset < -1 or self_offset + nq > nb, a non-finite value in Q or B (checked on the host); nothing is written then.
 *   nq = 0 returns INSIDER_OK and writes nothing.  insider_hip_last_neighbors_ms: of the calling THREAD's last call, the
 *   HIP-event time in ms of its kernels (transfers excluded). */
int insider_hip_neighbors(const double *Q, int64_t nq, const double *B, int64_t nb, int K, int metric, int k,
                          int64_t self_offset, int device, int32_t *idx_out, double *score_out);
double insider_hip_last_neighbors_ms(void);

/* Top-k partners among N deep vectors: the Gram matrix V' V of the standardised vectors with the selection fused behind the
 * product (insider_amd/csrc/insider_coexpr.hpp).  Handle-free, one device.
 *   V holds N vectors of `depth` contiguous doubles (column-major, depth x N: the layout insider_hip_neighbors uses for its
 *   K x n matrices, but the depth is not limited).  For every vector of the window [first, first + count) its k partners among
 *   all N vectors; a vector is never its own partner.  idx_out / score_out are count x k, query-major, in descending score,
 *   equal scores (-0.0 == 0.0) by ascending index; a row with fewer than k eligible partners ends in -1 / NaN.
 *   metric 0 = correlation: each vector is centred by its own mean (sum / depth) and divided by the root of its centred sum of
 *   squares; 1 = cosine: divided by the root of its sum of squares, no centring; 2 = dot: a plain copy.  Every sum runs in index
 *   order.  Under metrics 0 and 1 a vector whose (centred) sum of squares is not > 0 is DEAD: nobody's partner, its own row all
 *   open slots; under metric 2 nothing is dead.  Scores are not clipped: a correlation may exceed 1 by rounding.
 *   The score of a pair is one accumulator chain over the depth in ascending order, wherever the pair falls in tiles, windows
 *   or the launch grid: repeated calls return identical bits, and a call on a window returns exactly those rows of the full
 *   call.  Device memory is O(N depth + count k).
 *   INSIDER_ERR_ARG, nothing written: a NULL pointer, depth < 1, N < 1 or N > INT32_MAX, k outside 1..64, an unknown metric,
 *   first < 0, count < 0 or first + count > N, a non-finite value in V (checked on the host).  count = 0 returns INSIDER_OK
 *   and writes nothing; a failed device allocation returns INSIDER_ERR_ALLOC and writes nothing.
 *   insider_hip_last_gram_topk_ms: of the calling THREAD's last call, the HIP-event time in ms of its kernels (transfers
 *   excluded). */
int insider_hip_gram_topk(const double *V, int64_t depth, int64_t N, int metric, int k, int64_t first, int64_t count,
                          int device, int32_t *idx_out, double *score_out);
double insider_hip_last_gram_topk_ms(void);

/* Pairwise-complete top-k partners among N deep vectors with missing entries (insider_amd/csrc/insider_coexpr_pc.hpp).
 * Handle-free, one device.  V, depth, N, k, the window and the outputs' layout as in insider_hip_gram_topk(); a NaN in V is a
 * MISSING entry (+-inf is refused).
 *   Definition.  A pair of vectors a, b has values v and selection indicators m in {0, 1} (m = 0 where missing).  With J = the
 *   positions selected in both:  N = |J|,  Sa = sum_J a,  Sb = sum_J b,  Saa = sum_J a^2,  Sbb = sum_J b^2,  Sab = sum_J a b,
 *       cov = Sab - Sa Sb / N,   va = Saa - Sa^2 / N,   vb = Sbb - Sb^2 / N,   score = cov / sqrt(va vb):
 *   Pearson's r over the jointly selected positions, not clipped.
 *   Staged values.  The sums are taken over the staged values: each vector is first standardised over its own selected entries
 *   exactly as under metric 0 of insider_hip_gram_topk() (centred by the mean of its selected entries, divided by the root of
 *   their centred sum of squares, sums in index order).  The score is invariant under that affine map, and the map keeps the
 *   cancellation in va and vb mild.  A vector with fewer than two selected entries or no variance is DEAD, as there.
 *   Eligibility.  A pair is eligible when both vectors are alive, a != b, N >= min_overlap, va > floor Saa and vb > floor Sbb
 *   with floor = 16 (depth + 8) 2^-52.  The floor comes from the first-order rounding error of va computed this way, at most
 *   (3 depth + 3) 2^-53 Saa: a vector that is exactly constant on J always lands under it, any other vector with Saa / va
 *   below about 10^12 above it.  N is a sum of 0 / 1 products and is exact.
 *   Order: descending score, equal scores (-0.0 == 0.0) by ascending index, never the vector itself; a row with fewer than k
 *   eligible partners ends in -1 / NaN / -1.  overlap_out (count x k) holds the pair's N.
 *   Bits.  Each of the six sums is one accumulator chain over the depth in ascending order and the final formula is symmetric
 *   in a and b: score(a, b) and score(b, a) have the same bits, a window returns exactly the rows of the full call, repeated
 *   calls return identical bits; no floating-point atomics.
 *   INSIDER_ERR_ARG, nothing written: a NULL pointer, depth < 1 or > INT32_MAX, N < 1 or N > INT32_MAX, min_overlap < 3 (with
 *   N = 2 every pair scores +-1), k outside 1..64, first < 0, count < 0 or first + count > N, an infinite value in V.
 *   min_overlap above the depth is allowed and leaves every row open.  count = 0 returns INSIDER_OK and writes nothing; a
 *   failed device allocation returns INSIDER_ERR_ALLOC and writes nothing.  insider_hip_last_gram_topk_ms covers this call too. */
int insider_hip_gram_topk_pairwise(const double *V, int64_t depth, int64_t N, int64_t min_overlap, int k,
                                   int64_t first, int64_t count, int device,
                                   int32_t *idx_out, double *score_out, int32_t *overlap_out);

/* Preranked gene-set enrichment with a permutation null (insider_amd/csrc/insider_enrich.hpp).  Handle-free, one device.
 *   Inputs.  scores is R x p, row-major: profile r is p contiguous doubles.  set_ptr (int64, S + 1) and set_genes (int32) hold S
 *   sets in CSR form: set s is set_genes[set_ptr[s] .. set_ptr[s + 1]), 0-based gene indices, distinct within a set.
 *   Ranking.  Within a profile the genes are ordered by descending score, equal scores (-0.0 == 0.0) by ascending gene index;
 *   position 0 is the top.  The ranking runs on the host inside the library (a stable sort); everything behind it on the device.
 *   Weights.  weight = 0: w(t) = 1; weight = 1: w(t) = |score of the gene at position t|.
 *   Enrichment score of a position set T = {t_1 < ... < t_m}, 1 <= m < p:  P_i = w(t_1) + ... + w(t_i), N = P_m (N == 0: w = 1
 *   for this set, the classic statistic, so nothing divides by zero), miss_i = t_i - (i - 1),
 *       hi = max_i (P_i / N - miss_i / (p - m)),    lo = min_i (P_{i-1} / N - miss_i / (p - m)),    P_0 = 0,
 *   ES = hi if hi >= -lo, else lo; peak = the smallest t_i at which the chosen extreme is attained.  Each deviation is evaluated
 *   exactly as written (an fp64 division, another, one subtraction; no reciprocals): with integer-valued weights the result is
 *   a pure function of integers, identical on host and device.  This equals the running sum over all p positions.
 *   Observed score of (profile, set): T = the rank positions of the set's genes.
 *   Null draw b (0 <= b < nperm) of size m: T = { phi(j) : j = 0 .. m - 1 }, phi the keyed bijection of [0, p) of
 *   include/insider_sample.h: bits = the smallest even number >= 2 with 2^bits >= p, half = bits / 2, mask = 2^half - 1,
 *   key = h32(h32(lo32(seed) ^ 0x9E3779B9) ^ hi32(seed) ^ 0x85EBCA6B * b); x = j, then until x < p (cycle walking):
 *   L = x >> half, Rr = x & mask; for i = 1..8: t = L ^ (h32(Rr ^ key ^ 0xC2B2AE35 * i) & mask), L = Rr, Rr = t;
 *   x = L << half | Rr.  h32 = insider_h32 (include/insider_perm.h), uint32 arithmetic that wraps.  A draw depends on
 *   (seed, b, p, m) only, not on the profile or the set, and the sizes are nested.
 *   Counts per (profile, set), over the nperm draws of the set's size scored on the profile: the side of a score is positive
 *   when ES >= 0; n_same = the draws on the observed side, n_ge = those of them with |ES_b| >= |ES|, sum_same = the sum of
 *   their ES_b (added in draw order), hits_nonzero = the set's genes whose score is not 0.  The caller derives
 *   p = (n_ge + 1) / (n_same + 1) and NES = ES / (sum_same / n_same).
 *   Outputs are R x S, profile-major.  No atomics: repeated calls return identical bits, a call on some of the profiles returns
 *   exactly those rows and a call on some of the sets exactly those columns.  Device memory is O(R p + nnz + R S).
 *   INSIDER_ERR_ARG, nothing written: a NULL pointer, R < 0, S < 0, p < 2 or p > INT32_MAX, weight outside {0, 1}, nperm outside
 *   1..65536, a set with m < 1, m >= p or m > 4096, a gene index out of range or repeated within a set, a set_ptr that
 *   decreases or starts below 0, a non-finite score (all checked on the host, before a device is opened).  R == 0 or S == 0
 *   returns INSIDER_OK and writes nothing.
 *   insider_hip_last_enrichment_ms: of the calling THREAD's last call, the HIP-event time in ms of its kernels (ranking and
 *   transfers excluded).
 *   insider_hip_enrichment_sample: host only, opens no device: out[j] = phi(j), j < m, of draw `perm` under `seed` on [0, p)
 *   (0 <= m <= p, p as above; otherwise INSIDER_ERR_ARG). */
int insider_hip_enrichment(const double *scores, int64_t R, int64_t p, const int64_t *set_ptr, const int32_t *set_genes,
                           int64_t S, int weight, int nperm, uint64_t seed, int device, double *es, int32_t *peak,
                           int32_t *n_ge, int32_t *n_same, double *sum_same, int32_t *hits_nonzero);
double insider_hip_last_enrichment_ms(void);
int insider_hip_enrichment_sample(uint64_t seed, uint32_t perm, int64_t m, int64_t p, int32_t *out);

/* K-means (Lloyd) clustering of embeddings (insider_amd/csrc/insider_kmeans.hpp).  Handle-free, one device.
 *   Layout.  P is D x N, column-major: one point is D contiguous doubles, the layout of column_factor.  init is D x k or NULL,
 *   centers D x k; label, dist, second, dist2 have length N, sizes length k, traj max_iter + 1 entries; final_inertia, iters and
 *   converged have length `restarts`; best is one int.
 *   Working points.  metric 0 = cosine (spherical k-means): x_i = p_i / |p_i|, |p_i| the square root of the sum of squares taken
 *   in index order (as insider_hip_neighbors normalises); a point whose sum of squares is 0 is DEAD: label = second = -1,
 *   dist = dist2 = NaN, it is in no cluster, no sum, no size, and never an initial centre.  metric 1 = Euclidean: x_i = p_i and
 *   every point is alive.  Na = the number of alive points.
 *   Score of (point i, centre j).  Cosine: s = x_i . c_j (centres have unit norm).  Euclidean: s = x_i . c_j - h_j,
 *   h_j = 0.5 * (the sum of squares of c_j in index order).  The centre of a point (label) is the one with the largest s, equal
 *   scores (-0.0 == 0.0) to the lowest centre index; second is the next centre in that order (-1 / NaN when k = 1).
 *   Distances.  Cosine: dist = 1 - s.  Euclidean: dist = max(0, |x_i|^2 - 2 s), |x_i|^2 summed in index order.  dist2 is the same
 *   of the second centre.
 *   Update.  Cluster j = the alive points with label j, n_j its size.  Euclidean: c_j = (sum of the members) / n_j, one division
 *   per coordinate, no reciprocal.  Cosine: c_j = (sum of the members) / |sum| (index order).  A cluster with n_j = 0 keeps its
 *   centre and reports size 0; so does a cluster under cosine whose sum has norm 0.
 *   Loop of one restart.  Assign to the initial centres: L_0 and J_0, J = the sum of dist over the alive points (the inertia).
 *   For t = 0, 1, ...: if t == max_iter stop, unconverged; else update the centres from L_t and assign again: L_{t+1}, J_{t+1};
 *   if L_{t+1} == L_t stop, converged.  iters = the number of updates; traj = J_0 .. J_iters, NaN beyond; label, second, dist,
 *   dist2 and sizes always come from the last assignment, which was made against the returned centres.  max_iter = 0 with
 *   init given is therefore "assign these points to these centres".
 *   Initial centres.  init given: restarts must be 1; under cosine its columns are normalised (a zero-norm column is an
 *   argument error).  init NULL (Forgy): with a_0 < a_1 < ... the Na alive point indices, restart r starts from x at
 *   a_{phi(j)}, j < k, phi = insider_sample_phi on [0, Na) under insider_sample_key(seed, r) (include/insider_sample.h;
 *   insider_hip_enrichment_sample(seed, r, k, Na, out) names the draw).  Duplicate points may give duplicate centres: the tie
 *   rule then leaves the higher-indexed one empty.
 *   Restarts are independent; best = the restart with the lowest final_inertia (= its last J), ties to the lowest r; centers,
 *   label, dist, second, dist2, sizes and traj belong to best.
 *   Purity.  Centre sums use no floating-point atomics (a stable counting sort by label, then sums in member order; the counts
 *   are integer atomics): the result is a pure function of the arguments and repeated calls return identical bits.  The score of
 *   a pair is the same instruction sequence wherever the pair falls: with max_iter = 0 a call on a window of the points returns
 *   exactly those rows of the full call.
 *   Device memory is O((N + k) D + N) (the counting sort adds at most 4 N + k integers).  Between the upload and the final
 *   download the only thing that crosses the bus is one record per iteration: the inertia and the count of changed labels.
 *   INSIDER_ERR_ARG, nothing written: a NULL pointer (init may be NULL), D outside 1..63, k outside 1..4096, N < 1 or
 *   N > INT32_MAX, an unknown metric, restarts outside 1..256, restarts != 1 with init given, max_iter outside 0..10000, a
 *   non-finite value in P or init, k > Na, init NULL with Na < 2 (all checked on the host, before a device is opened).
 *   insider_hip_last_kmeans_ms: of the calling THREAD's last call, the HIP-event time in ms from its first kernel to its last
 *   (the per-iteration records included, the upload and the download excluded). */
int insider_hip_kmeans(const double *P, int64_t N, int D, int k, int metric, const double *init, int restarts, int max_iter,
                       uint64_t seed, int device, double *centers, int32_t *label, double *dist, int32_t *second, double *dist2,
                       int32_t *sizes, double *traj, double *final_inertia, int32_t *iters, int32_t *converged, int32_t *best);
double insider_hip_last_kmeans_ms(void);

/* Agglomerative (hierarchical) clustering of embeddings (insider_amd/csrc/insider_hclust.hpp).  Handle-free, one device.
 *   Layout.  P is D x N, column-major: one point is D contiguous doubles, the layout of column_factor.  merge is (N - 1) x 2
 *   int32, row-major (row r = the two children of merge r); height and size have N - 1 entries, order has N.
 *   Linkages.  Two are offered: those that are reducible and whose cluster-to-cluster distance is a function of the clusters'
 *   sums.  n = the size, S = the sum of the member vectors, mu = S / n (one division per coordinate).
 *     metric 0, linkage 0: cosine, average.  Members x = p / |p|, |p| the square root of the sum of squares (products and sums
 *       rounded one by one in index order); a point whose sum of squares is 0 is DEAD: it is in no cluster.
 *       d(A, B) = 1 - mu_A . mu_B, which is exactly the mean pairwise cosine distance (UPGMA).  height = d.
 *     metric 1, linkage 1: Euclidean, Ward.  Members x = p - m, m = the grand mean (coordinate by coordinate: partial i < 256 adds
 *       the points i, i + 256, ... in that order, the partials are added in order, one division by N): Ward is translation
 *       invariant, and centring removes the cancellation of data far from the origin.  Every point is alive.
 *       d(A, B) = max(0, n_A n_B / (n_A + n_B) * ((h_A + h_B) - 2 mu_A . mu_B)), h = |mu|^2.  height = sqrt(2 d), the
 *       convention of scipy's linkage(method="ward").
 *     Every other pair of codes is refused.  Single and complete linkage are not functions of the sums; centroid and median
 *     linkage are not reducible.  None of them is offered.
 *   Tie rule.  Candidates are ordered by (d ascending, cluster id ascending); d is bitwise symmetric in (A, B).  Ids of a run:
 *   0 .. N - 1 are the points, the r-th merge the run emits is N + r.
 *   Algorithm: rounds of reciprocal nearest neighbours.  A cluster is STALE when it has no stored neighbour or its stored
 *   neighbour was merged.  A round (1) finds, for every stale cluster, its first candidate among all other clusters in the order
 *   above (in round 1 every cluster is stale), (2) merges every pair a < b with nn[a] = b and nn[b] = a, emitting them in
 *   ascending a: S_new = S_a + S_b, n_new = n_a + n_b.  Everybody else keeps its neighbour (reducibility).  A round that finds no
 *   pair (rounding can break reducibility in the last bit) merges nothing, and in the next round every cluster is stale; such a
 *   round always holds a pair (the lowest id on any minimal pair and its neighbour name each other).  The run ends when one
 *   cluster is left; rounds = the rounds run, queries = the sum of their stale counts, alive = the points that are not dead.
 *   When max_rounds rounds (>= 1; 2 N always suffices) did not finish the run: INSIDER_ERR_UNFINISHED, nothing written.
 *   Result.  The height of a merge is raised to the larger height of its children where rounding left it below; the merges are
 *   sorted by height, equal heights by emission (a stable sort: children come before parents), and renumbered as scipy's
 *   linkage numbers them: row r creates id N + r; a leaf keeps its point index (with no dead point this is scipy's Z).  merge
 *   holds the lower id first; size is the number of points under the merge.  alive - 1 rows are filled (none when alive <= 1);
 *   the rows beyond hold -1 / NaN / -1.  order = the leaves of a depth-first walk from the last row, the lower id first, then
 *   the dead points in ascending index.
 *   Purity.  No floating-point atomics and no order that depends on the launch: the result is a pure function of the arguments
 *   and repeated calls return identical bits.  The N x N distances never exist: device memory is O(N D).  Between the upload
 *   and the final download the only thing that crosses the bus is one record of three ints per round.
 *   INSIDER_ERR_ARG, nothing written: a NULL pointer, D outside 1..63, N < 1 or 2 N - 1 > INT32_MAX, a pair (metric, linkage)
 *   other than the two above, max_rounds < 1, a non-finite value in P (all checked on the host, before a device is opened).
 *   insider_hip_last_hclust_ms: of the calling THREAD's last call, the HIP-event time in ms from its first kernel to its last
 *   (the per-round records included, the upload and the final download excluded); set by an unfinished run too. */
int insider_hip_hclust(const double *P, int64_t N, int D, int metric, int linkage, int max_rounds, int device, int32_t *merge,
                       double *height, int32_t *size, int32_t *order, int32_t *rounds, int64_t *queries, int32_t *alive);
double insider_hip_last_hclust_ms(void);

/* Exact t-SNE map of a neighbour graph (insider_amd/csrc/insider_tsne.hpp).  Handle-free, one device.
 *   Input: a graph, not points.  nbr_idx is N x k int32, point-major (row i = the k slots of point i), 0-based, -1 = an open
 *   slot; nbr_d2 is N x k double, the squared distance >= 0 of every filled slot (open slots are not read; NaN by convention).
 *   This is what insider_hip_neighbors returns under cosine with d2 = max(0, 2 - 2 score).  A row's filled slots come first; no
 *   row names itself or one index twice.  m_i = the filled slots of row i.  A point with m_i = 0 that is in nobody's row is DEAD:
 *   its coordinates (and beta, grad) are NaN, its p_cond row 0, and it takes part in no sum.  Na = the number of alive points.
 *   Calibration of row i.  d_s = d2_s - (the smallest d2 of the row).  perplexity >= m_i: p_s|i = 1 / m_i, beta = 1.  Otherwise
 *   exactly 100 steps from beta = 1, lo = 0, hi = inf on H(beta) = log S + beta T / S, S = sum_s exp(-beta d_s),
 *   T = sum_s d_s exp(-beta d_s) (sums in slot order): H > log(perplexity): lo = beta, then beta = 2 beta while hi is inf, else
 *   (beta + hi) / 2; otherwise hi = beta, then beta = (lo + beta) / 2.  p_s|i = exp(-beta d_s) / S with the last beta.  A row of
 *   equal distances has no root: it ends uniform at beta = 2^100.  Nothing here yields NaN or Inf.
 *   Joint.  P_ij = (p_j|i + p_i|j) / (2 Na), a direction that is in no row counting 0.
 *   At a map Y (2 x N: y_i = Y[2 i], Y[2 i + 1]).  w_ij = 1 / (1 + |y_i - y_j|^2), the differences taken coordinate-wise before
 *   squaring; Z = sum over alive i != j of w_ij; g_i = 4 (a sum_j P_ij w_ij (y_i - y_j) - (1 / Z) sum_j w_ij^2 (y_i - y_j)), a
 *   the exaggeration in force; KL = sum over P_ij > 0 of P_ij log(P_ij Z / w_ij), always with the un-exaggerated P.
 *   Iteration t = 0 .. max_iter - 1, from gain = 1, v = 0: a = exaggeration and mu = 0.5 while t < exag_iters, else a = 1 and
 *   mu = 0.8; step = eta if eta > 0, else max(Na / (4 exaggeration), 50).  Per coordinate: gain = gain + 0.2 if
 *   (g > 0) != (v > 0), else gain * 0.8; gain = max(gain, 0.01); v = mu v - (step gain) g; y = y + v (each product and sum
 *   rounded as written).  Then the mean of the alive points, summed in a fixed order, is subtracted.  There is no early stop.
 *   Records.  kl_traj has max_iter / kl_every + 1 entries: entry j is KL at Y_t, t = j kl_every (Y_max_iter = the returned map);
 *   final_kl is KL at the returned map.  grad (2 x N) and Z are the gradient under a = 1 and Z at the returned map; beta (N) and
 *   p_cond (N x k, open slots exactly 0) the calibration.  beta, p_cond, grad and Z may each be NULL.
 *   Start.  init (2 x N) given: Y_0 = init (the values of dead points are checked but not used); max_iter = 0 then means
 *   "calibrate, and evaluate KL, Z and the gradient at this Y".  init NULL: y_{i,d} = insider_tsne_draw(insider_sample_key(seed,
 *   0), 2 i + d) (include/insider_sample.h): u = h32(key ^ 0x27D4EB2F (2 i + d + 1)), y = ((u + 0.5) 2^-32 - 0.5) 1e-4, uniform
 *   in +-0.5e-4, drawn on the host.
 *   Device.  The alive points are compacted on the host and the pattern of the reverse edges (a stable counting sort of the edges
 *   by target) is built there before the upload; the all-pairs repulsion runs on a grid of row tiles x `slabs` slabs of the
 *   points, whose partial sums are added in slab order (slabs = 0: the library chooses, from Na alone; 1..64: forced).  No
 *   floating-point atomics: the result is a pure function of the arguments and repeated calls return identical bits.  The bits may
 *   depend on `slabs` (it sets where the sums are cut).  Between the upload and the final download nothing crosses the bus.
 *   Device memory is O(N k + slabs N).
 *   INSIDER_ERR_ARG, nothing written: a NULL nbr_idx, nbr_d2, Y, kl_traj or final_kl; N outside 1..2^20; k outside 1..64; a
 *   perplexity that is not finite or < 1; max_iter or exag_iters outside 0..10000; kl_every < 1; an exaggeration that is not finite
 *   or < 1; an eta that is not finite or < 0; slabs outside 0..64; max_iter = 0 without init; an index outside -1..N-1, a row that
 *   names itself or an index twice, a filled slot after an open one; a negative or non-finite d2 in a filled slot; a non-finite
 *   init; Na < 2 (all checked on the host, before a device is opened).
 *   insider_hip_last_tsne_ms: of the calling THREAD's last call, the HIP-event time in ms from its first kernel to its last (the
 *   upload and the download excluded). */
int insider_hip_tsne(const int32_t *nbr_idx, const double *nbr_d2, int64_t N, int k, double perplexity, const double *init,
                     int max_iter, int exag_iters, int kl_every, double exaggeration, double eta, uint64_t seed, int slabs,
                     int device, double *Y, double *kl_traj, double *final_kl, double *beta, double *p_cond, double *grad, double *Z);
double insider_hip_last_tsne_ms(void);

/* Profile of the last insider_hip_optimize() call (option "profile" = 1), HIP-event timed on the library's stream.
 * out[0..11]: {column-side masked-Gram launches, total ms, row-side masked-Gram launches, total ms,
 *  column-solve (CD / ridge) launches, total ms, test-residual launches, total ms,
 *  optimize() wall ms, outer iterations run, elastic-net sweeps total, path flags (1 = factored column statistics, 2 =
 *  merged row update, 4 = the factored column statistics ran in their pair-count form)}. */
int insider_hip_get_profile(insider_hip_handle *h, double *out12);

/* Facts about the handle that measurement code needs (bench.py's roofline): "col_stats_path" (0 = per-entry lists, 1 =
 * look-up form, 2 = pair-count form, as the cost model / options chose for the current K), "col_mfma_per_gene"
 * (v_mfma_f64_16x16x4 instructions the column-side statistics kernel issues per gene), "row_merged", "col_entries",
 * "row_entries" (padded held-out list lengths), "data_bytes_shared" / "data_bytes_own" (insider_hip_remask), "lists_bytes", "pair_count_bytes_per_gene", "stat_doubles", "kp",
 * "cd_ms_steady" / "col_stats_ms_steady" (option "profile": mean HIP-event time per outer iteration from iteration 5 on of
 * the last optimize(), i.e. without the cold start), "cap_hits" / "max_gene_sweeps" (of the last optimize() / optimize_col():
 * elastic-net solves ended by "max_sweeps" instead of convergence — must be 0 to match the reference, which has no cap — and
 * the longest solve in sweeps), "max_sweeps", "col_solver" / "col_eval" (the kernel the last column solve launched for the solve,
 * and for the evaluation pass after it; 0 = none: 1 k_ridge_cols_reg, 2 k_ridge_cols, 3 k_cd_cols_reg with one or two slots,
 * 4 k_cd_cols_reg with three slots, 5 k_cd_cols<16,4>, 6 k_cd_cols<32,2>, 7 k_cd_cols<64,1>, 8 / 9 / 10 k_cd_cols_r16<1 / 2 / 3>),
 * "col_ridge_fallback" (1: the last ridge solve also launched k_ridge_cols for the genes k_ridge_cols_reg marked),
 * "col_stats_kernel" (the kernel the last column-side statistics launch ran, in optimize(), optimize_col() or col_stats(): 0 =
 * none yet, 1 k_list_stats<NB>, 2 k_list_stats4, 3 k_col_factored, 4 k_col_paircnt, 5 k_col_paircnt with real-valued counts
 * (continuous covariates), 6 / 7 k_col_paircnt4 with MAXS = 4 / 8 k-steps, 8 k_col_paircnt4 with MAXS = 4 and real-valued
 * counts; MAXS = 8 with real-valued counts is never launched), "col_stats_tickets" (the ticket counters k_col_paircnt4 drew
 * genes from: 1 or 16; 0 for the other kernels), "col_stats_blocks" (k_col_paircnt4's grid size, 0 for the other kernels: its
 * blocks walk the genes in groups of four when 4 x blocks < p), "col_stats_own_q" (1: that launch formed the genes' rows of S A
 * and S^held A itself, option "stats_own_q", and no product over the genes ran for it; 0: it read the products),
 * "col_q_kernel" (the kernel the last Q = S A or S^held A product ran: 0 = none yet, 1 k_mm_rows<NB>, 2 k_mm_rows2<NB>),
 * "mm_rows2_tiles" (the tiles of 16 rows per wave of the last k_mm_rows2 launch, for S A or for V = C A'; 0 = none yet),
 * "n_simd" (SIMDs of the handle's device, 4 per compute unit),
 * "vd_path" (the form of k_vd_stats the last insider_hip_variance_decomposition() ran: 1 = level tables in LDS, 2 = read from
 * global memory; 0 = none yet),
 * "sd_path" / "sd_slabs" (of the last insider_hip_sample_decomposition(): the form of k_sd_stats, 1 = level tables in LDS, 2 =
 * read from global memory, 0 = none yet; and the gene slabs its grid had),
 * "ls_path" / "ls_slabs" (of the last insider_hip_level_scores(): 1 = one level window, X read once, 2 = several windows of 128
 * levels, X read once per window, 0 = none yet; and the gene slabs its grid had),
 * "glm_slabs" / "glm_form" (of the last insider_hip_interaction_glm(): the gene slabs the grid of k_resid_stats had, and its
 * form 10 NB + GT, NB = ceil(K / 16) blocks of 16 latent dimensions and GT gene tiles per staging round: 18, 24, 32, 42; 0 =
 * none yet),
 * "fd_path" (the form of the heavy pass of the last insider_hip_factor_decomposition(): 1 = one column window, X read once;
 * 2 = several windows of 128 columns of W, X read once per window; 0 = none yet),
 * "rc_slabs" / "rc_ms" (of the last insider_hip_residual_products(): the gene slabs the grid of k_rc_fwd had, 0 = no forward
 * pass or none yet; and the HIP-event time in milliseconds of k_rc_back, k_rc_fwd and k_rc_reduce),
 * "cx_stage_mb" / "cx_stage_ms" / "cx_ms" (of the last insider_hip_coexpression(): the megabytes of the staged standardised
 * residual, the HIP-event time in milliseconds of k_cx_stage and k_cx_norm, and that of k_cx_topk; 0 = none yet; a call of
 * insider_hip_coexpression_pairwise() fills the first two alike and leaves "cx_ms"),
 * "cx_pc_ms" (of the last insider_hip_coexpression_pairwise(): the HIP-event time in milliseconds of k_cx_topk_pc; 0 = none
 * yet),
 * "ls_form" / "fd_form" / "rc_form" / "cx_form" (the template instantiation of the heavy launch of the last
 * insider_hip_level_scores(), _factor_decomposition(), _residual_products() and _coexpression(), set on the host at the launch
 * site; 0 = none yet.  The first three are 10 QT + KS, KS = ceil(K / 16) blocks of 16 latent dimensions and QT tiles of 16
 * columns: k_ls_prod<QT,KS> with QT 1 (at most 16 levels) or 8 (the window form): 11..14, 81..84; k_fd_prod<8,KS,true>: 81..84;
 * k_rc_back<QT,KS> and k_rc_fwd<QT,KS> with QT = ceil(q / 16): 11..14, 21..24, 31..34, 41..44.  "cx_form" is the KS of
 * k_cx_stage<KS>: 1..4),
 * "ol_path" (the form of k_ol_flag the last insider_hip_outliers() ran: 1 = level tables in LDS, 2 = read from global memory;
 * 0 = none yet),
 * "row_kernels" (a bit mask of the row-phase kernel forms the last optimize() / optimize_row() launched, reset at the start of
 * each; set on the host at each launch site.  Level Gram sums: bit 0 wgemm4, 1 wgemm5, 2 wgemm6, 3 wgemm7 (k_wgemm<LT>),
 * 4 wgemm_chunks (a k_wgemm launch with more than one level-tile chunk, grid.z > 1), 5 wsyrk (k_wsyrk<NB>; neither wsyrk nor a
 * wgemm bit: no held-out entry), 6 gram_side (level Gram sums on optimize()'s second side stream).  u: 7 gene_u_cnt
 * (k_gene_u_cnt), 8 gene_u (k_gene_u), 9 gene_uc (k_gene_uc, a continuous column).  Record tail + equations: 10 merged_solve
 * (k_level_merged with the ridge solve), 11 merged (k_level_merged without it), 12 merged_zero (k_level_merged on the zero
 * record of tuning = 0), 13 pack_reduce (k_level_pack + k_level_reduce).  Per-sample path and solves: 14 list_stats4
 * (k_list_stats4, row side), 15 list_stats (k_list_stats<NB>, row side), 16 level_partial (k_level_partial + k_level_sum +
 * k_level_reduce), 17 level_solve (k_level_solve), 18 cont_cd (k_cont_cd).  Products of the row update (not the row prep):
 * V = C A' 19 mm_rows2 (k_mm_rows2), 20 mm_rows (k_mm_rows); Y = U'C 21 mm_reduce2_2 (k_mm_reduce2<NB,2>), 22 mm_reduce2_4
 * (k_mm_reduce2<NB,4>), 23 mm_reduce (k_mm_reduce)),
 * the scalar facts of the resident data set (what insider_hip_create_ex / _remask / _remask_fold built; they describe the
 * arrays of insider_hip_get_array "ds:<name>"): "ds_ldn" / "ds_ldp" (pitch of a gene-major / sample-major line: n / p rounded
 * up to 128), "ds_SLP" (pitch of the level-sum tables: all levels + m, rounded up to 2), "ds_cnt_train" / "ds_cnt_test"
 * (entries whose train / test bit is set), "ds_no_na" (1: every entry is train or test), "ds_merged" / "ds_cont_merged" (the
 * tables of the merged row update exist; also for the continuous columns), "ds_cf_pair_ok" (the pair-count form's tables
 * exist: no cell above 255), "ds_max_chunks", "ds_max_L", "ds_max_items", "ds_nitems:<i>" / "ds_npairs:<i>" (work items and
 * (level, gene) pairs of covariate i's weighted lists),
 * "ds_bytes:<name>" or "ds_bytes:<name>:<i>" (size in bytes of the data-set array of that name, 0 when this data set did not
 * build it; an unknown name returns INSIDER_ERR_ARG; "ds_bytes:cf_geometry" and "ds_bytes:names" likewise). */
int insider_hip_get_info(insider_hip_handle *h, const char *name, double *out);

/* Diagnostics: copy an internal per-gene array to the host: "cd_pass_slot" (uint32 x p: what the last limited pass of a
 * multi-pass column solve left per gene: 0xFFFFFFFF = finished, else estimate bucket << 24 | rank), "gene_perm" (int32 x p:
 * the launch order), "order_table" (the sweep-order table of the last column solve: rows of 448 bytes, one per sweep of the
 * period; bytes 0..K-1 of row s = the coordinates of sweep s in visiting order, include/insider_perm.h).
 * bytes may be at most what exists (else INSIDER_ERR_ARG); the handle's stream is synchronised, nothing is written.
 *
 * "ds:<name>" or "ds:<name>:<i>": a device array of the resident data set, as it lies in memory (the whole allocation:
 * "ds_bytes:<name>" of insider_hip_get_info gives its size).  An array this data set did not build returns INSIDER_ERR_ARG
 * with a message that says so; so does an unknown name.  Names are those of the members:
 *   X (f64, p lines of pitch ds_ldn, pad 0), codes (u8, same layout: bit 0 train, bit 1 test, pad = train), lev (i32, c x n,
 *   0-based), lvl_off_d (i32, c + 1), members_all (i32, c x n: samples by level, ascending inside a level), lvl_ptr_all (i32,
 *   covariate i's L_i + 1 pointers at lvl_off[i] + i), lvl_count_all (i32, per stacked level), Zc (f64, m x n), one_count,
 *   ident_members (i32), S / Strain / Sheld (f64, p x ds_SLP: level sums of X over all / train / held-out entries, continuous
 *   column k at SLcat + k: sums of x z), yy_all / yy_train (f64, p), col_ptr / row_ptr (u32, lines + 1), col_idx / row_idx
 *   (i32), col_val / row_val (f64), col_flag (u8; only with NA entries): the held-out lists, ascending element index inside a
 *   line, each line padded to a multiple of 32 entries with (0x7FFFFF, 0.0, 0); the 64 entries behind the last line are not
 *   defined.  cf_cnt (u8), cf_hn (f32), cf_sq (f64), cf_zt (f64): the packed tables of the factored column statistics,
 *   cont_cnt (f64, m), cont_pair:<k> (f64, SL), fold_id (u8, layout of codes, pad 0).
 *   Per covariate i: chunk_level:<i>, chunk_begin:<i>, chunk_end:<i>, lvl_chunk_ptr:<i> (i32), grp:<i> (u32, p x (L_i + 1)),
 *   slev:<i> (u16, max(c - 1, 1) planes of col_entries + 64; defined at the positions grp addresses), item_begin:<i>,
 *   item_end:<i> (u32), lvl_item_ptr:<i> (i32, L_i + 1), wl_idx:<i> (i32), wl_w:<i> (f64), paircnt:<i> (f64, L_i rows of
 *   pitch SL = all levels + m).  The same members of the continuous columns' tables are "cont.<member>",
 *   "contm.<member>:<k>" (contm.paircnt:<k> is the allocation of cont_pair:<k>) and "contm_lists.<member>".
 * "ds:names": every such name, one per line, ":#" behind a name that takes an index.
 * "ds:cf_geometry": the static part of the factored statistics' arguments as 136 int32: c, nsteps, tab_skip_lo, tab_skip_n,
 *   tab_rows, cnt_stride, hn_stride, zt_stride, sq_stride, m; then nine values each (positions 0..8, descending level count;
 *   position c = the continuous columns) of L, off, nlater, cnt_off, hn_off, zt_off; then pos_cov[8]; then later_plane[8][8]
 *   row by row.  All zero when the data set has no factored tables (more than 8 covariates, or no merged tables). */
int insider_hip_get_array(insider_hip_handle *h, const char *name, void *out, int64_t bytes);

/* Diagnostics: per-gene sweep counts of the last column update (p ints); of the calling THREAD's last
 * insider_hip_strong_cd() / _xy(), the HIP-event time in ms of its solve launches (summed over the chunks of a large
 * batch) and the kernel that ran them, coded as insider_hip_get_info("col_solver") codes it. */
int insider_hip_get_sweeps(insider_hip_handle *h, int32_t *out);
double insider_hip_last_cd_ms(void);
int insider_hip_last_cd_solver(void);

#ifdef __cplusplus
}
#endif
#endif /* INSIDER_HIP_H */
