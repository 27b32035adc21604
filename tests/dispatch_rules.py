"""Which kernel form runs for which call, written out by hand: the tests' independent copy of the rules of
insider_amd/csrc/insider_plan.hpp (build_plan() and the small functions beside it).

The GPU tests assert these against what a call reports it launched (insider_hip_get_info: "col_solver", "col_eval",
"col_stats_kernel", "col_stats_tickets", "col_stats_blocks", "col_q_kernel", "mm_rows2_tiles", "row_kernels");
tests/test_plan_cpu.py asserts them against the plan itself, built on the CPU by tests/plan_driver.cpp.  Pure Python: no
library, no device, no data (what a rule needs from a case's data, such as the largest pair count, comes in as an argument).
"""
import math

MM_FAST_MIN = 16384
MM_SLAB = 128
CF_MAXC = 8
GU_TILE = 512
PERM_PERIOD = 16384


def nb_of(K):
    return (K + 16) // 16


# ----------------------------------------------------------------------------------------------------------------------
# the column solve
# ----------------------------------------------------------------------------------------------------------------------
# (lambda, alpha) of the column update in each regime; the two last leave a near-exact fit on the cd_reg and ridge_reg kernels
REGIMES = {"enet": (30.0, 0.4),     # lambda alpha > 0 and an l2 term
           "lasso": (30.0, 1.0),    # l2 = 0: XtX_kk + l2 = 0 in a zero latent dimension
           "nol1": (0.0, 0.5),      # lambda = 0: alpha > 0 but no l1 term, so not the register-resident kernel
           "ridge": (30.0, 0.0),
           "enet_tiny": (1e-12, 0.4), "ridge_tiny": (1e-12, 0.0)}

# the kernel of the column solve, per (regime, cd_variant), for K in 1..16 | 17..32 | 33..48 | 49..63
SOLVER = {
    ("enet", 0): ("cd_reg", "cd_reg", "cd_reg3", "cd_cols64"),
    ("lasso", 0): ("cd_reg", "cd_reg", "cd_reg3", "cd_cols64"),
    ("nol1", 0): ("cd_cols16", "cd_cols32", "cd_r16_3", "cd_cols64"),
    ("ridge", 0): ("ridge_reg", "ridge_reg", "ridge", "ridge"),
    ("enet", 1): ("cd_cols16", "cd_cols32", "cd_cols64", "cd_cols64"),
    ("lasso", 1): ("cd_cols16", "cd_cols32", "cd_cols64", "cd_cols64"),
    ("ridge", 1): ("ridge", "ridge", "ridge", "ridge"),
    ("enet", 2): ("cd_r16_1", "cd_r16_2", "cd_r16_3", "cd_cols64"),
    ("lasso", 2): ("cd_r16_1", "cd_r16_2", "cd_r16_3", "cd_cols64"),
    ("enet_tiny", 0): ("cd_reg", "cd_reg", "cd_reg3", "cd_cols64"),
    ("ridge_tiny", 0): ("ridge_reg", "ridge_reg", "ridge", "ridge"),
}
# the evaluation launch after the register-resident solves (the three-slot kernel hands it to the row16 kernel)
EVAL = {"cd_reg": "cd_reg", "cd_reg3": "cd_r16_3"}


def col_solver(regime, variant, K):
    return SOLVER[(regime, variant)][(K - 1) // 16]


def col_eval(solver):
    return EVAL.get(solver, "none")


def pass_limits(first, ratio, max_sweeps, period=PERM_PERIOD):
    """The sweep indices at which the passes of a cold column solve stop (options cd_pass1, cd_pass_ratio): none below 32;
    else first, first x ratio, ... (ratio at least 2) while below min(max_sweeps, 4 periods of the order sequence), 16 at most.
    The last pass runs from the last limit to the end."""
    out = []
    if first >= 32:
        limit = first
        while limit < min(max_sweeps, 4 * period) and len(out) < 16:
            out.append(limit)
            limit *= max(ratio, 2)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the per-entry statistics of either side
# ----------------------------------------------------------------------------------------------------------------------
def list_form(K, list_fine=1, fperm=True):
    """k_list_stats4 for 16 <= K <= 31 (NB = 2, NT = 5..8) when the workspace holds the permuted factor rows."""
    return "list4" if list_fine and 16 <= K <= 31 and fperm else "list"


# ----------------------------------------------------------------------------------------------------------------------
# the column statistics (test_gpu_col_stats.py: a case is a dict with K, levels, m, p, opts, cost, walk)
# ----------------------------------------------------------------------------------------------------------------------
COL_OPTS = dict(col_factored=1, col_mfma4=1, list_fine=1)


def lookup_fits(tab_rows, KP):
    """k_col_factored's LDS: (tab_rows + 1) KP doubles of table + 4 x 16 x 17 transpose scratch + 4 x CF_CAP uint16 <= 64 KB,
    i.e. (tab_rows + 1) KP <= 5056: tab_rows <= 315 / 157 / 104 / 78 at KP = 16 / 32 / 48 / 64."""
    return (tab_rows + 1) * KP <= 5056


def pc4_fits(KP, nsteps, quads):
    """k_col_paircnt4's LDS: 1088 + KP^2 + 4 nsteps KP + 4 quads KP <= 8192 doubles (nsteps + quads <= 47 at KP = 32)."""
    return 1088 + KP * KP + 4 * nsteps * KP + 4 * quads * KP <= 8192


def col_structure(c, max_cell):
    """What stage_merged() / stage_factored() / stage_cont_factored() decide for a case's data set.  max_cell: the largest
    dense pair count of any gene."""
    levels, m = c["levels"], c["m"]
    ncov, SLcat = len(levels), sum(levels)
    merged = m <= 4 and SLcat + GU_TILE <= 2048
    tab_rows = SLcat - max(levels)                 # every covariate but the largest (position 0) is in the table
    nsteps = (tab_rows + 3) // 4
    pair_ok = merged and ncov <= CF_MAXC and nsteps <= 8 and max_cell <= 255
    zt = m > 0 and pair_ok and all(SLcat + m + L + L % 2 <= 1536 for L in levels)
    return merged, tab_rows, nsteps, pair_ok, zt


def col_stats_kernel(c, structure):
    """(col_stats_kernel, col_stats_tickets) of one col_stats() call on the case's handle; structure: col_structure(c, .)."""
    o = {**COL_OPTS, **c["opts"]}
    K, levels, m, p = c["K"], c["levels"], c["m"], c["p"]
    NB = (K + 16) // 16
    KP = 16 * NB
    merged, tab_rows, nsteps, pair_ok, zt = structure
    # col_stats_path()
    if not (merged and o["col_factored"] and len(levels) <= CF_MAXC):
        path = "list"
    elif m > 0:
        path = "pair" if pair_ok and zt else "list"
    elif o["col_factored"] == 3 and pair_ok:
        path = "pair"
    elif o["col_factored"] >= 2:
        # (a table too large for the look-up form has more than 78 rows: never a pair-count table, whose limit is 32)
        path = "lookup" if lookup_fits(tab_rows, KP) else ("pair" if pair_ok else "list")
    else:
        path = c["cost"]          # the cost model: pinned by hand per case (COST in test_gpu_col_stats.py)
        assert path in ("list", "lookup", "pair"), c["id"]
    if path == "list":
        return list_form(K, o["list_fine"]), 0
    if path == "lookup":
        return "factored", 0
    # the pair-count form
    quads = 1 + sum(math.ceil(L / 4) for L in levels) + (1 if zt else 0)
    if o["col_mfma4"] and NB <= 2 and not (zt and nsteps > 4) and pc4_fits(KP, nsteps, quads):
        name = "paircnt4_ms4" if nsteps <= 4 else "paircnt4_ms8"
        return name + ("_zt" if zt else ""), 16 if math.ceil(p / 4) >= 16 else 1
    return ("paircnt_zt" if zt else "paircnt"), 0


def check_pc4_blocks(c, kernel, tickets, blocks):
    """The grid of the statistics launch: k_col_paircnt4's blocks are a multiple of its ticket counters, one per group of
    four genes unless the case is written to have fewer resident blocks than groups; 0 for every other kernel."""
    if kernel.startswith("paircnt4"):
        nb = math.ceil(c["p"] / 4)
        assert blocks % tickets == 0 and blocks >= tickets, blocks
        if c["walk"]:                       # fewer resident blocks than groups of four genes: the blocks walk
            assert 4 * blocks < c["p"], (blocks, c["p"])
        else:
            assert blocks == nb - nb % tickets, (blocks, nb)
    else:
        assert blocks == 0


def loss_stats_kernel(paths, K, m=0):
    """The column-statistics kernel of a masked call under PATHS[paths] on the data of test_gpu_loss_checkpoint.py (info
    "col_stats_kernel"), by hand: seven table rows (the smaller covariate) fit the look-up form and two k-steps of the
    pair-count form; the pair counts run on the 4x4x4 instruction up to K = 31; continuous columns take the pair-count form
    with real-valued counts."""
    if paths == "lists":
        return list_form(K)
    if paths == "fast" and m == 0:
        return "factored"
    return ("paircnt4_ms4" if K <= 31 else "paircnt") + ("_zt" if m else "")


# ----------------------------------------------------------------------------------------------------------------------
# the row update (test_gpu_row_update.py: a case is a dict with K, levels, m, p, tuning, opts, overflow, no_heldout,
# cost_merged)
# ----------------------------------------------------------------------------------------------------------------------
# Level Gram sums of a covariate with L levels on the k_wgemm route (row_gemm = 1, dense pair counts, c <= 8): tiles =
# ceil(L / 16) >= 4, split into ceil(tiles / 7) chunks of LT = ceil(tiles / chunks) tiles.  For K <= 31 the cost test
# tiles * ceil(K (K + 1) / 32) < 0.9 L NB (NB + 1) / 2 holds at every L >= 49.
GEMM_BANDS = [((1, 48), {"wsyrk"}),
              ((49, 64), {"wgemm4"}), ((65, 80), {"wgemm5"}), ((81, 96), {"wgemm6"}), ((97, 112), {"wgemm7"}),
              ((113, 128), {"wgemm4", "wgemm_chunks"}), ((129, 160), {"wgemm5", "wgemm_chunks"}),
              ((161, 192), {"wgemm6", "wgemm_chunks"}), ((193, 224), {"wgemm7", "wgemm_chunks"}),
              ((225, 240), {"wgemm5", "wgemm_chunks"}), ((993, 1008), {"wgemm7", "wgemm_chunks"})]
# K >= 32: the cost test decides (written out: tiles * ntile against 0.9 L NBLK)
GEMM_WIDE = {(47, 52): {"wsyrk"},     # 4 * 71 = 284 >= 280.8
             (47, 53): {"wgemm4"},    # 284 < 286.2
             (47, 65): {"wsyrk"},     # 5 * 71 = 355 >= 351
             (63, 55): {"wsyrk"},     # 4 * 126 = 504 >= 495
             (63, 58): {"wgemm4"},    # 504 < 522
             (63, 65): {"wsyrk"}}     # 630 >= 585
# the K sweep's many-level covariate: 60 levels pass the test at every K (K = 47: 284 < 324; K = 63: 504 < 540)
GEMM_WIDE.update({(K, 60): {"wgemm4"} for K in range(32, 64)})


def gemm_forms(K, L):
    if K >= 32 and L >= 49:
        return GEMM_WIDE[(K, L)]
    for (lo, hi), forms in GEMM_BANDS:
        if lo <= L <= hi:
            return forms
    raise KeyError((K, L))


ROW_OPTS = dict(row_merged=1, row_gemm=1, row_counts=1, row_fused=1, list_fine=1, force_allreduce=0, mm_fast=1)


def row_structure(case):
    """(tables, pair, cont_merged) of a case's data set.  insider_hip_create_ex: the merged tables exist for m <= 4 and
    SLcat + 512 <= 2048 (k_gene_u's LDS record); the dense pair counts for c <= 8, at most 32 table rows (levels of all
    covariates but the largest) and no cell over 255."""
    levels, m = case["levels"], case["m"]
    c, SLcat = len(levels), sum(levels)
    tables = m <= 4 and SLcat <= 1536
    pair = tables and c <= 8 and SLcat - max(levels) <= 32 and not case["overflow"]
    cont_merged = m > 0 and pair and all(SLcat + m + L + L % 2 <= 1536 for L in levels)
    return tables, pair, cont_merged


def row_kernels(case, cov):
    """The forms one optimize_row() of covariate `cov` launches (cov >= c: continuous column cov - c)."""
    o = {**ROW_OPTS, **case["opts"]}
    K, levels, m, p, tuning = case["K"], case["levels"], case["m"], case["p"], case["tuning"]
    c, SLcat = len(levels), sum(levels)
    NB = (K + 16) // 16
    cont = cov >= c
    tables, pair, cont_merged = row_structure(case)
    merged = tables and o["row_merged"] != 0 and (m == 0 or cont_merged)
    if o["row_merged"] == 1 and m == 0 and tuning == 1:
        merged = merged and case["cost_merged"]     # use_merged()'s cost model, evaluated by hand for the case
    solve = {"merged_solve"} if NB <= 2 and not o["force_allreduce"] else {"merged", "level_solve"}
    s = set()
    if tuning == 1 and merged:
        s.add("mm_rows2" if o["mm_fast"] and p >= MM_FAST_MIN else "mm_rows")
        if cont:
            return s | {"gene_uc", "mm_reduce", "wsyrk", "merged", "cont_cd"}
        L = levels[cov]
        s.add("gene_u_cnt" if pair and (o["row_counts"] or m > 0) and SLcat + m + L + L % 2 <= 1536 else "gene_u")
        if o["mm_fast"] and p >= MM_FAST_MIN and L > 16:
            s.add("mm_reduce2_2" if (L + 15) // 16 <= 2 or o["mm_fast"] == 2 or NB > 2 else "mm_reduce2_4")
        else:
            s.add("mm_reduce")
        gram = gemm_forms(K, L) if o["row_gemm"] and pair else {"wsyrk"}
        if case["no_heldout"]:
            assert gram == {"wsyrk"}
            gram = set()
        s |= gram
        s |= solve if o["row_fused"] else {"pack_reduce", "level_solve"}
    elif tuning == 1:
        s.add("list_stats4" if list_form(K, o["list_fine"]) == "list4" else "list_stats")
        s |= {"level_partial", "cont_cd" if cont else "level_solve"}
    elif tables and o["row_merged"] and o["row_fused"] and m == 0:
        s |= {"merged_zero"} | solve
    else:
        s |= {"level_partial", "level_solve"}
    return s


# ----------------------------------------------------------------------------------------------------------------------
# the streaming products (test_gpu_stream_products.py)
# ----------------------------------------------------------------------------------------------------------------------
def q_kernel(K, SL, p, mm_fast=1):
    """Q = S A on k_mm_rows2 (2) or k_mm_rows (1): the staged factors, 4 ceil(SL / 16) NB 64 doubles, within 64 KB:
    ceil(SL / 16) NB <= 32 (SLP is even)."""
    return 2 if mm_fast and p >= MM_FAST_MIN and math.ceil(SL / 16) * nb_of(K) <= 32 else 1


def tiles(p, n_simd, mm_tiles=0):
    """Tiles of 16 genes per wave of k_mm_rows2."""
    return mm_tiles if mm_tiles >= 1 else max(1, math.ceil(p / 16) // (2 * n_simd))


def v_nt(N):
    """(NT, grid.y) of V = C A' for N stacked levels."""
    NT = 1 if N <= 16 else 2 if N <= 32 else 4
    return NT, math.ceil(N / (16 * NT))


def reduce2_form(K, L, p, mm_fast=1):
    """(NB, LT) of k_mm_reduce2 for a reduction over p rows into L columns, or None (k_mm_reduce)."""
    if not (mm_fast and p >= MM_FAST_MIN and L > 16):
        return None
    NB = nb_of(K)
    return NB, (2 if math.ceil(L / 16) <= 2 or mm_fast == 2 or NB > 2 else 4)
