"""Every row-update kernel form that row_update() and launch_level_gram() can launch, against the CPU oracle.

For each covariate the row update picks its level Gram sums (k_wgemm<4..7> in one or several level-tile chunks, k_wsyrk, or
nothing), its u (k_gene_u_cnt, k_gene_u, k_gene_uc), its record tail / equations / solve (k_level_merged with or without the
solve, k_level_pack + k_level_reduce, k_level_solve, k_cont_cd), the per-sample chain instead (k_list_stats4 / k_list_stats,
k_level_partial ...) and the forms of its products V = C A' and Y = U'C.  insider_hip_get_info("row_kernels") reports the
forms the last optimize() / optimize_row() launched, one bit each (_lib.ROW_KERNELS).  expected() (row_kernels() in
tests/dispatch_rules.py) is that dispatch written out by hand from the call's FitPlan (build_plan() in insider_plan.hpp:
wgemm_plan(), use_merged(), unmasked_fused, fused_solve, row_fused, u_cnt, list4, v_rows2, reduce_form()): every case asserts
the exact set it reached before it compares values, so that a dispatch edit that moves a band to another kernel fails the
case written for the old one instead of quietly testing another kernel.
"""
import numpy as np
import pytest

from insider_amd import _lib, api, workloads
from tests.dispatch_rules import GEMM_WIDE, row_kernels as expected
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

BIT = {name: 1 << i for i, name in enumerate(_lib.ROW_KERNELS)}


def launched(ds):
    mask = int(ds.info("row_kernels"))
    assert mask & ~sum(BIT.values()) == 0, hex(mask)
    return {name for name, b in BIT.items() if mask & b}


@pytest.fixture(scope="module", autouse=True)
def _oracle_chunk(oracle):
    """One gene per OpenMP chunk: the reference's chunk of 100 genes would run these small solves on one thread."""
    oracle.set_col_chunk(1)
    yield
    oracle.set_col_chunk(100)


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
def case(name, K, levels, p=61, n=None, opts=None, tuning=1, lam=2.0, m=0, f=0.2, with_na=False, covs=None,
         overflow=False, no_heldout=False, cost_merged=None):
    return dict(id=name, K=K, levels=tuple(levels), p=p, n=n or max(120, 3 * sum(levels)), opts=opts or {}, tuning=tuning,
                lam=lam, m=m, f=f, with_na=with_na, covs=covs, overflow=overflow, no_heldout=no_heldout,
                cost_merged=cost_merged)


# K: the edges of NB 1..4 and of k_list_stats4's NT = 5..8, and an odd K inside each band
KS = [1, 9, 15, 16, 17, 19, 20, 23, 27, 28, 31, 32, 33, 41, 47, 48, 55, 63]
PS = [64, 61, 63, 131, 201]            # p = 0, 1, 3 mod 4; one slab (<= 64 genes) and three / four with a short last one
CASES = []
for i, K in enumerate(KS):
    p = PS[i % len(PS)]
    CASES.append(case(f"K{K}-merged-p{p}", K, (60, 7), p=p, opts=dict(row_merged=2), with_na=K % 2 == 1))
    CASES.append(case(f"K{K}-lists", K, (60, 7), p=p, opts=dict(row_merged=0)))
    if 16 <= K <= 31:
        CASES.append(case(f"K{K}-lists-coarse", K, (60, 7), p=p, opts=dict(row_merged=0, list_fine=0)))
    CASES.append(case(f"K{K}-unmasked", K, (60, 7), p=p, tuning=0))
for K in (1, 16, 31, 32, 47, 48, 63):
    CASES += [case(f"K{K}-nogemm", K, (60, 7), p=63, opts=dict(row_merged=2, row_gemm=0)),
              case(f"K{K}-nocounts", K, (60, 7), p=63, opts=dict(row_merged=2, row_counts=0)),
              case(f"K{K}-unfused", K, (60, 7), p=63, opts=dict(row_merged=2, row_fused=0)),
              case(f"K{K}-allreduce", K, (60, 7), p=63, opts=dict(row_merged=2, force_allreduce=1)),
              case(f"K{K}-unmasked-unfused", K, (60, 7), p=63, tuning=0, opts=dict(row_fused=0)),
              case(f"K{K}-unmasked-allreduce", K, (60, 7), p=63, tuning=0, opts=dict(force_allreduce=1))]
    for o in (dict(), dict(row_fused=0), dict(force_allreduce=1)):   # lambda = 0: fit_interaction()'s arithmetic
        CASES.append(case(f"K{K}-lambda0-{'-'.join(o) or 'fused'}", K, (60, 7), p=131, lam=0.0, opts=dict(row_merged=2, **o),
                          covs=(0,)))
    CASES.append(case(f"K{K}-lambda0-unmasked", K, (60, 7), p=131, lam=0.0, tuning=0, covs=(0,)))
# level counts: every k_wgemm tile count and chunking (second covariate of 5 levels)
for i, L in enumerate([33, 40, 48, 49, 50, 64, 65, 80, 81, 96, 97, 112, 113, 130, 170, 192, 200, 230]):
    K, p = (9, 24)[i % 2], PS[i % len(PS)]
    CASES.append(case(f"L{L}-K{K}-p{p}", K, (L, 5), p=p, opts=dict(row_merged=2), n=2 * L + 40))
# both sides of wgemm_plan's cost edge, and one slab at large K (row_gemm_waves = 64)
for K, L in sorted(GEMM_WIDE):
    if L != 60:
        CASES.append(case(f"edge-K{K}-L{L}", K, (L, 4), p=64, opts=dict(row_merged=2), covs=(0,)))
CASES.append(case("K63-L60-one-slab", 63, (60, 4), p=201, opts=dict(row_merged=2, row_gemm_waves=64), covs=(0,)))
CASES.append(case("K20-L130-one-slab", 20, (130, 4), p=131, opts=dict(row_merged=2, row_gemm_waves=64), covs=(0,)))
# fallbacks: one-byte count overflow (gene 0 wholly held out: ~267 samples per cell), nine covariates, a covariate too
# large for k_gene_u_cnt's record beside one that fits, no held-out entry at all
CASES += [case("overflow", 5, (3, 2), n=1600, p=40, opts=dict(row_merged=2), overflow=True),
          case("nine-covariates", 6, (3, 2, 2, 2, 2, 2, 2, 2, 3), n=200, p=40, opts=dict(row_merged=2)),
          case("L1000-beside-L30", 6, (1000, 30), n=2100, p=40, opts=dict(row_merged=2)),
          case("L1000-beside-L30-K20", 20, (1000, 30), n=2100, p=41, opts=dict(row_merged=2)),
          case("no-heldout", 9, (40, 6), p=61, opts=dict(row_merged=2), no_heldout=True),
          case("no-heldout-K40", 40, (40, 6), p=61, opts=dict(row_merged=2), no_heldout=True)]
# continuous columns: merged (m <= 4) and per-sample (m = 5), masked and not
for m in (1, 2, 4, 5):
    for K in (7, 20):
        for tuning in (1, 0):
            CASES.append(case(f"ctns{m}-K{K}-t{tuning}", K, (6, 4), p=61, n=150, m=m, tuning=tuning))
CASES.append(case("ctns2-K40", 40, (6, 4), p=64, n=150, m=2))
# streaming products (p >= 16384): V on k_mm_rows2; U'C on k_mm_reduce2<., 4> (L > 32, NB <= 2, mm_fast = 1), <., 2>
# (17..32 levels, mm_fast = 2 or NB > 2) and k_mm_reduce (L <= 16)
for K, mm in ((5, 1), (20, 1), (40, 1), (50, 1), (5, 2), (20, 2)):
    CASES.append(case(f"stream-K{K}-mm{mm}", K, (40, 20, 3), p=16400, n=48, opts=dict(row_merged=2, mm_fast=mm), f=0.15,
                      covs=(0, 1, 2) if K <= 20 else (0,)))
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def data(c):
    """X, level table, masks and random factors of a case (the factors: like test_optimize_row_operator)."""
    w = workloads.small(n=c["n"], p=c["p"], level_counts=c["levels"], K=c["K"], f=c["f"], seed=len(c["id"]) + c["K"],
                        with_na=c["with_na"])
    Mtr, Mte = w.M_train.copy(order="F"), w.M_test.copy(order="F")
    if c["overflow"]:
        Mtr[:, 0], Mte[:, 0] = 0, 1
    if c["no_heldout"]:
        Mtr[:], Mte[:] = 1, 0
    rng = np.random.default_rng(1000 + c["K"] + c["p"])
    A = [np.asfortranarray(rng.standard_normal(a.shape) * 0.5) for a in w.A0]
    C = np.asfortranarray(rng.standard_normal(w.C0.shape) * 0.5)
    Z = np.asfortranarray(rng.standard_normal((c["n"], c["m"]))) if c["m"] else None
    U = np.asfortranarray(rng.standard_normal((c["m"], c["K"])) * 0.3) if c["m"] else None
    return w, Mtr, Mte, A, C, Z, U


def handle(c, w, Mtr, Mte, Z):
    ds = api.InsiderData(w.X, w.levels, Mtr, Mte, ctns_confounder=Z)
    for k, v in c["opts"].items():
        ds.set_option(k, v)
    return ds


def factors(A, U):
    return [a.copy(order="F") for a in A] + ([U.copy(order="F")] if U is not None else [])


def reference(oracle, c, w, M, A, C, Z, U, cov):
    """oracle.optimize_row / optimize_continuous on the residual without the updated covariate's contribution."""
    ncat = len(c["levels"])
    part = sum(A[i][w.levels[:, i] - 1, :] for i in range(ncat) if i != cov)
    if U is not None:
        part = part + sum(np.outer(Z[:, k], U[k]) for k in range(c["m"]) if ncat + k != cov)
    resid = w.X - (part @ C if not np.isscalar(part) else 0.0)
    if cov < ncat:
        return oracle.optimize_row(resid, M, A[cov], C, w.levels[:, cov], C @ C.T, c["lam"], tuning=c["tuning"])
    k = cov - ncat
    return oracle.optimize_continuous(resid, M, U[k], C, Z[:, k], C @ C.T, c["lam"], tuning=c["tuning"])[None, :]


# ----------------------------------------------------------------------------------------------------------------------
# a. operator level, and c. the same update on a handle with history
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASE_BY_ID))
def test_optimize_row_every_kernel(oracle, cid):
    c = CASE_BY_ID[cid]
    w, Mtr, Mte, A, C, Z, U = data(c)
    inc = 1 if c["m"] else 0
    M = Mtr if c["tuning"] == 1 else np.ones_like(Mtr)
    ncov = len(c["levels"]) + c["m"]
    covs = c["covs"] if c["covs"] is not None else range(ncov)
    for cov in covs:
        want = expected(c, cov)
        ds = handle(c, w, Mtr, Mte, Z)      # a fresh handle per update
        try:
            got = ds.optimize_row(factors(A, U), C, cov, lambda_=c["lam"], tuning=c["tuning"], inc_continuous=inc)
            assert launched(ds) == want, (cov, sorted(launched(ds)), sorted(want))
            if cov >= len(c["levels"]):   # (a continuous column's update returns every column's row: its own is row cov - c)
                got = got[[cov - len(c["levels"])]]
        finally:
            ds.close()
        ref = reference(oracle, c, w, M, A, C, Z, U, cov)
        assert relerr(got, ref) < 1e-9, (cov, relerr(got, ref))
        if c["tuning"] == 1 and want & {"mm_rows", "mm_rows2"}:
            # c. merged form: bit-identical on a handle that has just run a masked optimize() (level Gram sums on the side
            # stream, w_ready) and an optimize_row() of another covariate
            ds = handle(c, w, Mtr, Mte, Z)
            try:
                ds.optimize(factors(A, U), C.copy(order="F"), c["K"], 2.0, 2.0, 0.4, tuning=1, max_iter=1, seed=3,
                            inc_continuous=inc)
                assert "gram_side" in launched(ds)
                ds.optimize_row(factors(A, U), C, (cov + 1) % ncov, lambda_=c["lam"], tuning=1, inc_continuous=inc)
                again = ds.optimize_row(factors(A, U), C, cov, lambda_=c["lam"], tuning=1, inc_continuous=inc)
                assert launched(ds) == want
                if cov >= len(c["levels"]):
                    again = again[[cov - len(c["levels"])]]
            finally:
                ds.close()
            assert np.array_equal(again, got), (cov, relerr(again, got))


# ----------------------------------------------------------------------------------------------------------------------
# b. fits: the side-stream level Gram sums of optimize()
# ----------------------------------------------------------------------------------------------------------------------
FITS = {"gemm-cnt": case("fit-gemm-cnt", 9, (70, 5), p=63, opts=dict(row_merged=2)),
        "gemm-chunks": case("fit-gemm-chunks", 20, (130, 4), p=64, n=300, opts=dict(row_merged=2)),
        "gene-u": case("fit-gene-u", 6, (3, 2, 2, 2, 2, 2, 2, 2, 3), p=40, n=200, opts=dict(row_merged=2)),
        "nb3": case("fit-nb3", 40, (60, 7), p=64, opts=dict(row_merged=2)),
        "allreduce": case("fit-allreduce", 9, (60, 7), p=61, opts=dict(row_merged=2, force_allreduce=1)),
        "unfused": case("fit-unfused", 9, (60, 7), p=61, opts=dict(row_merged=2, row_fused=0)),
        "ctns2": case("fit-ctns2", 7, (6, 4), p=61, n=150, m=2),
        "unmasked": case("fit-unmasked", 9, (60, 7), p=61, tuning=0),
        "lists": case("fit-lists", 20, (60, 7), p=61, opts=dict(row_merged=0))}


def fit_expected(c):
    s = set()
    for cov in range(len(c["levels"]) + c["m"]):
        s |= expected(c, cov)
    if c["tuning"] == 1 and ("mm_rows" in s or "mm_rows2" in s):
        s.add("gram_side")
    return s


def _fit_check(oracle, c, w, Mtr, Mte, A, C, Z, U, opts_default=False):
    inc = 1 if c["m"] else 0
    ds = handle(c, w, Mtr, Mte, Z)
    try:
        got = ds.optimize(factors(A, U), C.copy(order="F"), c["K"], 2.0, 2.0, 0.4, tuning=c["tuning"], max_iter=3, seed=19,
                          inc_continuous=inc)
        kernels = launched(ds)
    finally:
        ds.close()
    ref = oracle.optimize(w.X, w.levels, w.n_levels, A + ([U] if U is not None else []), C, Mtr, Mte, 2.0, 2.0, 0.4,
                          tuning=c["tuning"], max_iter=3, seed=19, row_threads=8, col_threads=16,
                          **(dict(ctns=Z) if Z is not None else {}))
    assert got["iters"] == ref["iters"] == 4
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
    assert np.array_equal(got["traj"][:, 9], ref["traj"][:, 9])      # same decay schedule
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-7, i
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-7
    return kernels


@pytest.mark.parametrize("name", list(FITS))
def test_fit_every_merged_form(oracle, name):
    c = FITS[name]
    w, Mtr, Mte, A, C, Z, U = data(c)
    kernels = _fit_check(oracle, c, w, Mtr, Mte, A, C, Z, U)
    assert kernels == fit_expected(c), (sorted(kernels), sorted(fit_expected(c)))


# the benchmark's structures under the default options (64-gene slabs of c3 and c5, all samples): the merged update
# (use_merged()'s cost model picks it: ~90 against ~110 us at c3, ~180 against ~200 us at c5), c3's 100-level covariate on
# k_wgemm<7> beside k_gene_u_cnt; c5's interaction covariate (200 levels: 55 table rows) leaves the pair counts, so k_gene_u and
# k_wsyrk.  (At full size the products are k_mm_rows2 and k_mm_reduce2<2, 4> / k_mm_reduce instead.)
DEFAULT_FITS = {"c3": {"wgemm7", "wsyrk", "gram_side", "gene_u_cnt", "merged_solve", "mm_rows", "mm_reduce"},
                "c5": {"wsyrk", "gram_side", "gene_u", "merged_solve", "mm_rows", "mm_reduce"}}


@pytest.mark.parametrize("name", list(DEFAULT_FITS))
def test_benchmark_structures_default_kernels(oracle, name):
    w = workloads.make(name, gene_range=(0, 64))
    rng = np.random.default_rng(7)
    A = [np.asfortranarray(rng.standard_normal(a.shape) * 0.3) for a in w.A0]
    C = np.asfortranarray(rng.standard_normal(w.C0.shape) * 0.3)
    c = case(f"default-{name}", w.K, [int(L) for L in w.n_levels], p=64, n=w.X.shape[0], cost_merged=True)
    kernels = _fit_check(oracle, c, w, w.M_train, w.M_test, A, C, None, None)
    assert kernels == DEFAULT_FITS[name], sorted(kernels)


# ----------------------------------------------------------------------------------------------------------------------
# d. reach: every form is launched by some case
# ----------------------------------------------------------------------------------------------------------------------
def reach_cases():
    """For each form, the first case of the table expected to launch it (the streaming cases come last), one per form."""
    picked = []
    for name in _lib.ROW_KERNELS:
        for c in CASES:
            covs = c["covs"] if c["covs"] is not None else range(len(c["levels"]) + c["m"])
            if any(name in expected(c, cov) for cov in covs):
                if c not in picked:
                    picked.append(c)
                break
    return picked


def test_every_row_kernel_is_reached():
    union = set()
    for c in reach_cases():
        w, Mtr, Mte, A, C, Z, U = data(c)
        inc = 1 if c["m"] else 0
        ds = handle(c, w, Mtr, Mte, Z)
        try:
            for cov in (c["covs"] if c["covs"] is not None else range(len(c["levels"]) + c["m"])):
                ds.optimize_row(factors(A, U), C, cov, lambda_=c["lam"], tuning=c["tuning"], inc_continuous=inc)
                assert launched(ds) == expected(c, cov), (c["id"], cov)
                union |= launched(ds)
            if c["tuning"] == 1:
                ds.optimize(factors(A, U), C.copy(order="F"), c["K"], 2.0, 2.0, 0.4, tuning=1, max_iter=0, seed=3,
                            inc_continuous=inc)
                union |= launched(ds)
        finally:
            ds.close()
    assert union == set(_lib.ROW_KERNELS), sorted(set(_lib.ROW_KERNELS) - union)
