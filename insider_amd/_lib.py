"""ctypes binding of libinsider_hip.so (the C ABI declared in include/insider_hip.h).

There is no CPU fallback: every compute entry point raises InsiderError when the
shared library is missing or no HIP device is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("INSIDER_HIP_LIB") or os.path.join(_HERE, "libinsider_hip.so")   # INSIDER_HIP_LIB: another build of the same C ABI

OK, ERR_ARG, ERR_SOLVE, ERR_ALLOC, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_COMM, ERR_UNFINISHED = range(9)
TRAJ_STRIDE = 10
MAX_K = 63

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

# every symbol include/insider_hip.h declares (tests check the library exports all of them)
SYMBOLS = (
    "insider_hip_version", "insider_hip_last_error", "insider_hip_device_count", "insider_hip_create",
    "insider_hip_create_ex",
    "insider_hip_destroy", "insider_hip_set_shard", "insider_hip_set_option", "insider_hip_optimize",
    "insider_hip_optimize_oneshot", "insider_hip_optimize_row", "insider_hip_optimize_col", "insider_hip_strong_cd", "insider_hip_masked_gram_cols",
    "insider_hip_masked_gram_rows", "insider_hip_get_profile", "insider_hip_get_sweeps", "insider_hip_last_cd_ms",
    "insider_hip_optimize_oneshot_ex", "insider_hip_strong_cd_xy", "insider_hip_solve_sympd", "insider_hip_get_info",
    "insider_hip_comm_unique_id", "insider_hip_comm_init", "insider_hip_get_array", "insider_hip_clone",
    "insider_hip_optimize_continuous_v2", "insider_hip_residual", "insider_hip_interaction_glm",
    "insider_hip_variance_decomposition", "insider_hip_sample_decomposition", "insider_hip_col_stats", "insider_hip_last_cd_solver",
    "insider_hip_remask", "insider_hip_set_folds", "insider_hip_remask_fold", "insider_hip_factor_decomposition",
    "insider_hip_outliers", "insider_hip_neighbors", "insider_hip_last_neighbors_ms", "insider_hip_level_scores",
    "insider_hip_enrichment", "insider_hip_last_enrichment_ms", "insider_hip_enrichment_sample",
    "insider_hip_kmeans", "insider_hip_last_kmeans_ms", "insider_hip_residual_products", "insider_hip_solve_sympd_form",
    "insider_hip_tsne", "insider_hip_last_tsne_ms",
    "insider_hip_gram_topk", "insider_hip_last_gram_topk_ms", "insider_hip_coexpression",
    "insider_hip_gram_topk_pairwise", "insider_hip_coexpression_pairwise",
    "insider_hip_hclust", "insider_hip_last_hclust_ms",
)
COMM_ID_BYTES = 128
# insider_hip_outliers (insider_amd/csrc/insider_outliers.hpp): the samples a block of k_ol_flag covers per trip (OL_TRIP) and the
# genes k_ol_scan takes per step (OL_SCAN_CHUNK): the sizes at which the kernels change path
OL_TRIP = 1024
OL_SCAN_CHUNK = 1024
# insider_hip_get_info("col_solver" / "col_eval") and insider_hip_last_cd_solver(): the column-solve kernel behind each code
# (include/insider_hip.h)
COL_SOLVERS = ("none", "ridge_reg", "ridge", "cd_reg", "cd_reg3", "cd_cols16", "cd_cols32", "cd_cols64", "cd_r16_1", "cd_r16_2",
               "cd_r16_3")
# insider_hip_get_info("col_stats_kernel"): the column-side statistics kernel behind each code (include/insider_hip.h)
COL_STATS_KERNELS = ("none", "list", "list4", "factored", "paircnt", "paircnt_zt", "paircnt4_ms4", "paircnt4_ms8",
                     "paircnt4_ms4_zt")
# insider_hip_get_info("col_q_kernel"): the kernel of the last Q = S A product behind each code (include/insider_hip.h)
COL_Q_KERNELS = ("none", "mm_rows", "mm_rows2")
# insider_hip_get_info("row_kernels"): the row-phase kernel form behind each bit, bit 0 first (include/insider_hip.h)
ROW_KERNELS = ("wgemm4", "wgemm5", "wgemm6", "wgemm7", "wgemm_chunks", "wsyrk", "gram_side",
               "gene_u_cnt", "gene_u", "gene_uc",
               "merged_solve", "merged", "merged_zero", "pack_reduce",
               "list_stats4", "list_stats", "level_partial", "level_solve", "cont_cd",
               "mm_rows2", "mm_rows", "mm_reduce2_2", "mm_reduce2_4", "mm_reduce")


class InsiderError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"insider_hip status {status}: {message}")
        self.status = status


_lib = None


def load():
    """Load libinsider_hip.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.environ.get("INSIDER_HIP_LIB"):
        # the in-tree library must be THE build of the sources on disk: compared by content hash (the library carries the
        # hash of what it was compiled from), never by mtime; a stale or missing binary is rebuilt, not run
        from . import _build
        if _build.needs_build(LIB_PATH):
            try:
                _build.build_library()
            except Exception as e:
                raise InsiderError(ERR_NO_DEVICE, f"{LIB_PATH} is missing or was built from other sources (library "
                                                  f"{_build.library_sha(LIB_PATH)}, sources {_build.source_sha()}) and the "
                                                  f"rebuild failed: {e!r} (there is no CPU fallback)")
    if not os.path.exists(LIB_PATH):
        raise InsiderError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                                          f"g.build()'` (there is no CPU fallback)")
    # Concurrent fits on one GPU (insider_hip_clone, tune(concurrent=k)) overlap only as far as their streams land on
    # DIFFERENT hardware queues: the HIP runtime multiplexes all streams of a process onto a fixed number of queues, and two
    # fits whose main streams share a queue run one after the other.  That number belongs to the host's configuration; the
    # library does not change it.
    lib = C.CDLL(LIB_PATH)
    dp, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    lib.insider_hip_version.restype = C.c_char_p
    lib.insider_hip_last_error.restype = C.c_char_p
    lib.insider_hip_device_count.restype = C.c_int
    lib.insider_hip_create.argtypes = [dp, C.c_int64, C.c_int64, i32p, C.c_int, i32p, u8p, u8p, C.c_int,
                                       C.POINTER(C.c_void_p)]
    lib.insider_hip_create_ex.argtypes = [dp, C.c_int64, C.c_int64, i32p, C.c_int, i32p, dp, C.c_int, u8p, u8p, C.c_int,
                                          C.POINTER(C.c_void_p)]
    lib.insider_hip_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.insider_hip_remask.argtypes = [C.c_void_p, u8p, u8p, C.POINTER(C.c_void_p)]
    lib.insider_hip_set_folds.argtypes = [C.c_void_p, u8p, C.c_int]
    lib.insider_hip_remask_fold.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.insider_hip_destroy.argtypes = [C.c_void_p]
    lib.insider_hip_destroy.restype = None
    lib.insider_hip_set_shard.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
    lib.insider_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    lib.insider_hip_optimize.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_double, C.c_double,
                                         C.c_double, C.c_int, C.c_double, C.c_double, C.c_uint32, C.c_uint64, dp, dp,
                                         dp, dp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.insider_hip_optimize_oneshot.argtypes = [dp, C.c_int64, C.c_int64, C.POINTER(dp), dp, i32p, C.c_int, i32p,
                                                 u8p, u8p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                 C.c_int, C.c_double, C.c_double, C.c_uint32, C.c_uint64, dp, dp, dp]
    lib.insider_hip_optimize_oneshot_ex.argtypes = [dp, C.c_int64, C.c_int64, C.POINTER(dp), dp, i32p, C.c_int, i32p, dp,
                                                    C.c_int, u8p, u8p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                    C.c_double, C.c_int, C.c_double, C.c_double, C.c_uint32, C.c_uint64,
                                                    C.c_int, dp, dp, dp]
    lib.insider_hip_strong_cd_xy.argtypes = [dp, dp, C.c_int64, C.c_int, dp, C.c_double, C.c_double, dp, dp, C.c_double,
                                             C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, dp, i32p]
    lib.insider_hip_solve_sympd.argtypes = [dp, dp, C.c_int, C.c_int64, C.c_int, dp, i32p]
    lib.insider_hip_solve_sympd_form.argtypes = [dp, dp, C.c_int, C.c_int64, C.c_double, C.c_int, C.c_int, dp, i32p]
    lib.insider_hip_optimize_continuous_v2.argtypes = [dp, C.c_int64, C.c_int64, u8p, dp, dp, C.c_int, dp, dp, C.c_double,
                                                       C.c_int, C.c_int]
    lib.insider_hip_get_info.argtypes = [C.c_void_p, C.c_char_p, dp]
    lib.insider_hip_get_array.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]
    lib.insider_hip_comm_unique_id.argtypes = [C.c_void_p, C.c_int]
    lib.insider_hip_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.insider_hip_optimize_row.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.insider_hip_optimize_col.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_double, C.c_double,
                                             C.c_int, C.c_double, C.c_uint64, C.c_uint32]
    lib.insider_hip_strong_cd.argtypes = [dp, dp, dp, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double,
                                          C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, dp, i32p]
    lib.insider_hip_masked_gram_cols.argtypes = [C.c_void_p, dp, C.c_int, dp, dp]
    lib.insider_hip_masked_gram_rows.argtypes = [C.c_void_p, dp, C.c_int, dp, dp]
    lib.insider_hip_col_stats.argtypes = [C.c_void_p, C.POINTER(dp), C.c_int, C.c_int, dp, dp, dp]
    lib.insider_hip_residual.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, i32p, C.c_int64, C.c_int64, dp]
    lib.insider_hip_interaction_glm.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, i32p, i32p, C.c_int, dp,
                                                dp, dp]
    lib.insider_hip_variance_decomposition.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp]
    lib.insider_hip_sample_decomposition.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp]
    lib.insider_hip_level_scores.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp,
                                             dp]
    lib.insider_hip_factor_decomposition.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp]
    lib.insider_hip_residual_products.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp, dp, dp, C.c_int, dp,
                                                  dp, dp]
    lib.insider_hip_outliers.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int64,
                                         i32p, i32p, dp, C.POINTER(C.c_int64), i32p, i32p]
    lib.insider_hip_neighbors.argtypes = [dp, C.c_int64, dp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, i32p, dp]
    lib.insider_hip_last_neighbors_ms.restype = C.c_double
    lib.insider_hip_gram_topk.argtypes = [dp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, i32p, dp]
    lib.insider_hip_last_gram_topk_ms.restype = C.c_double
    lib.insider_hip_coexpression.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int,
                                             i32p, dp]
    lib.insider_hip_gram_topk_pairwise.argtypes = [dp, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, i32p,
                                                   dp, i32p]
    lib.insider_hip_coexpression_pairwise.argtypes = [C.c_void_p, C.POINTER(dp), dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int,
                                                      C.c_int64, C.c_int, i32p, dp, i32p]
    lib.insider_hip_enrichment.argtypes = [dp, C.c_int64, C.c_int64, C.POINTER(C.c_int64), i32p, C.c_int64, C.c_int, C.c_int,
                                           C.c_uint64, C.c_int, dp, i32p, i32p, i32p, dp, i32p]
    lib.insider_hip_last_enrichment_ms.restype = C.c_double
    lib.insider_hip_enrichment_sample.argtypes = [C.c_uint64, C.c_uint32, C.c_int64, C.c_int64, i32p]
    lib.insider_hip_kmeans.argtypes = [dp, C.c_int64, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_uint64, C.c_int, dp, i32p,
                                       dp, i32p, dp, i32p, dp, dp, i32p, i32p, i32p]
    lib.insider_hip_last_kmeans_ms.restype = C.c_double
    lib.insider_hip_hclust.argtypes = [dp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, dp, i32p, i32p, i32p,
                                       C.POINTER(C.c_int64), i32p]
    lib.insider_hip_last_hclust_ms.restype = C.c_double
    lib.insider_hip_tsne.argtypes = [i32p, dp, C.c_int64, C.c_int, C.c_double, dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                     C.c_uint64, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp]
    lib.insider_hip_last_tsne_ms.restype = C.c_double
    lib.insider_hip_get_profile.argtypes = [C.c_void_p, dp]
    lib.insider_hip_get_sweeps.argtypes = [C.c_void_p, i32p]
    lib.insider_hip_last_cd_ms.restype = C.c_double
    lib.insider_hip_last_cd_solver.restype = C.c_int
    _lib = lib
    return lib


def library_source_sha():
    """The source hash the LOADED library reports (insider_hip_version(): 'src:<sha16>')."""
    v = load().insider_hip_version().decode()
    return v.rsplit("src:", 1)[1] if "src:" in v else None


def check(status):
    if status != OK:
        raise InsiderError(status, load().insider_hip_last_error().decode(errors="replace"))


def device_count():
    return int(load().insider_hip_device_count())


def f64(a):
    return np.asfortranarray(a, dtype=np.float64)


def ptr(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))
