"""Every column-solver kernel that the column update and the batch entry can launch, against the CPU oracle.

The batch entry (insider_hip_strong_cd) runs the column update's elastic-net kernels with the default cd_variant, and
insider_hip_last_cd_solver() reports which one; its tests assert it as well.

The call's plan (build_plan() in insider_amd/csrc/insider_plan.hpp) picks one of ten kernels from the K band, from whether
lambda alpha > 0, alpha > 0 or alpha == 0, and from the option cd_variant; insider_hip_get_info("col_solver" / "col_eval")
reports which one ran.  SOLVER (tests/dispatch_rules.py) is that choice written out by hand: each test asserts the kernel it
reached, so that a dispatch edit that moves a band to another kernel fails the test written for the old one instead of
quietly testing another kernel.

The operator-level checks cap the solve at three sweeps: every kernel converges to the same minimiser at a tight tol, whatever
its coordinate order, so only a capped solve shows that a kernel reads its row of the sweep-order table correctly.
"""
import numpy as np
import pytest

from insider_amd import _lib, api, workloads
from tests.dispatch_rules import EVAL, SOLVER, col_solver as expected
from tests.dispatch_rules import REGIMES as ALL_REGIMES
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

UNCAPPED = 1 << 24


@pytest.fixture(scope="module", autouse=True)
def _oracle_chunk(oracle):
    """One gene per OpenMP chunk: the reference's chunk of 100 genes would run these 77-gene solves on one thread."""
    oracle.set_col_chunk(1)
    yield
    oracle.set_col_chunk(100)


def solver(ds, key="col_solver"):
    return _lib.COL_SOLVERS[int(ds.info(key))]


# (lambda, alpha) of the column update in each regime of this file
REGIMES = {r: ALL_REGIMES[r] for r in ("enet", "lasso", "nol1", "ridge")}

# the edges of every band and an odd K inside each
KS = [1, 2, 9, 15, 16, 17, 18, 25, 31, 32, 33, 34, 41, 47, 48, 49, 50, 55, 62, 63]
CELLS = [(r, v, K) for (r, v) in SOLVER if r in REGIMES for K in KS
         if not (r == "ridge" and v == 1 and K > 32)]   # (same kernel as cd_variant 0)

# ----------------------------------------------------------------------------------------------------------------------
# a. operator level: optimize_col() against oracle.optimize_col()
# ----------------------------------------------------------------------------------------------------------------------
N, P, LEVELS = 240, 77, (120, 7)   # p = 77: the last wave is partial at 4 and at 16 genes per wave
G_EMPTY, G_HELD = 5, 40            # a gene that is all zero, a gene whose every entry is held out
TOL = 1e-10


def _col_case(K, regime, with_na, seed):
    """Random row factors (R of full column rank: m >= 3K training rows per gene), data that the factors fit, a warm start.
    Outside the lambda = 0 regime: one all-zero gene, and one latent dimension whose column of R is exactly zero."""
    rng = np.random.default_rng(seed)
    levels = workloads.cyclic_levels(N, LEVELS)
    A = [np.asfortranarray(rng.standard_normal((L, K)) * 0.5) for L in LEVELS]
    edge = regime != "nol1"   # (lambda = 0: XtX_j has no penalty, the zero column would leave it singular)
    kz = K // 2
    if edge and K > 1:
        for a in A:
            a[:, kz] = 0.0
    R = sum(A[i][levels[:, i] - 1, :] for i in range(len(LEVELS)))
    Ct = rng.standard_normal((K, P)) * (rng.random((K, P)) < 0.5)
    X = np.asfortranarray(R @ Ct + 0.5 * rng.standard_normal((N, P)))
    if edge:
        X[:, G_EMPTY] = 0.0
    test = rng.random((N, P)) < 0.15
    if edge:
        test[:, G_HELD] = True
    Mte = np.asfortranarray(test.astype(np.uint8))
    Mtr = np.asfortranarray((~test).astype(np.uint8))
    if with_na:   # NA entries: x = 0, neither train nor test
        na = rng.random((N, P)) < 0.05
        na[:, G_HELD] = False   # (its entries stay held out)
        X[na] = 0.0
        Mtr[na] = 0
        Mte[na] = 0
    C0 = np.asfortranarray(rng.standard_normal((K, P)) * 0.3)
    return X, levels, Mtr, Mte, A, R, C0


@pytest.mark.parametrize("data", ["train_test", "na", "unmasked"])
@pytest.mark.parametrize("regime,variant,K", CELLS, ids=[f"{r}-v{v}-K{K}" for r, v, K in CELLS])
def test_optimize_col_every_solver(oracle, regime, variant, K, data):
    lam, alpha = REGIMES[regime]
    X, levels, Mtr, Mte, A, R, C0 = _col_case(K, regime, data == "na", seed=1000 * K + 10 * variant + len(regime))
    tuning = 0 if data == "unmasked" else 1
    M = Mtr if tuning == 1 else np.ones_like(Mtr)
    ds = api.InsiderData(X, levels, Mtr, Mte)
    try:
        ds.set_option("cd_variant", variant)
        if alpha == 0.0:   # one exact solve per gene: no sweeps, no order
            got = ds.optimize_col(A, C0.copy(order="F"), lambda_=lam, alpha=0.0, tuning=tuning)
            assert solver(ds) == expected(regime, variant, K)
            assert ds.info("col_ridge_fallback") == (solver(ds) == "ridge_reg")
            ref, _ = oracle.optimize_col(X, M, R, C0, lam, 0.0, tuning=tuning)
            assert relerr(got, ref) < 1e-10, relerr(got, ref)
            _check_edges(got, regime, tuning)
            return
        # capped: the first sweeps in either order mode, coordinate for coordinate (at K <= 2, with the zero dimension, one
        # coordinate is left, which the second sweep finds converged)
        cap = 1 if K <= 2 else 3
        for mode in (0, 1):
            ds.set_option("order_mode", mode)
            ds.set_option("max_sweeps", cap)
            got = ds.optimize_col(A, C0.copy(order="F"), lambda_=lam, alpha=alpha, tuning=tuning, tol=TOL, seed=77, it=5)
            assert solver(ds) == expected(regime, variant, K)
            assert ds.info("cap_hits") > 0
            sw = ds.sweeps()
            sink = oracle.set_sweep_sink(P)
            try:
                ref, _ = oracle.optimize_col(X, M, R, C0, lam, alpha, tuning=tuning, tol=TOL, seed=77, it=5,
                                             order_mode=mode, max_sweeps=cap)
                osw = sink.copy()
            finally:
                oracle.set_sweep_sink(None)
            assert np.array_equal(sw, osw), (mode, np.nonzero(sw != osw))
            assert relerr(got, ref) < 1e-10, (mode, relerr(got, ref))
        # uncapped to a tight tol: one sweep of slack in the stopping rule (see test_strong_cd_matches_oracle)
        ds.set_option("order_mode", 0)
        ds.set_option("max_sweeps", UNCAPPED)
        got = ds.optimize_col(A, C0.copy(order="F"), lambda_=lam, alpha=alpha, tuning=tuning, tol=TOL, seed=78, it=2)
        assert solver(ds) == expected(regime, variant, K)
        assert ds.info("cap_hits") == 0
        sw = ds.sweeps()
        sink = oracle.set_sweep_sink(P)
        try:
            ref, _ = oracle.optimize_col(X, M, R, C0, lam, alpha, tuning=tuning, tol=TOL, seed=78, it=2)
            osw = sink.copy()
        finally:
            oracle.set_sweep_sink(None)
    finally:
        ds.close()
    for j in range(P):
        assert abs(int(sw[j]) - int(osw[j])) <= 1, (j, sw[j], osw[j])
        err = np.max(np.abs(got[:, j] - ref[:, j]))
        assert err < (1e-9 if sw[j] == osw[j] else 50 * np.sqrt(TOL)), (j, sw[j], osw[j], err)
    assert np.array_equal(got == 0, ref == 0)
    _check_edges(got, regime, tuning)


def _check_edges(got, regime, tuning):
    """The all-zero gene, the gene held out entirely (when the mask is read) and the zero latent dimension solve to 0.  (The
    held-out gene's X'y is the full product less its held-out part: rounding, which only the l1 term sets to exactly 0.)"""
    if regime == "nol1":
        return
    assert not got[:, G_EMPTY].any()
    if tuning == 1:
        assert np.max(np.abs(got[:, G_HELD])) < 1e-13 if regime == "ridge" else not got[:, G_HELD].any()
    if got.shape[0] > 1:
        assert not got[got.shape[0] // 2].any()


# ----------------------------------------------------------------------------------------------------------------------
# b. fit level: the checkpoint branch of each kernel (per-gene loss sums) and the evaluation pass
# ----------------------------------------------------------------------------------------------------------------------
# (kernel, cd_variant, alpha, K): one K at each edge of the kernel's band
FIT_CELLS = [("cd_reg", 0, 0.4, 1), ("cd_reg", 0, 0.4, 32), ("cd_reg3", 0, 0.4, 33), ("cd_reg3", 0, 0.4, 48),
             ("cd_cols64", 0, 0.4, 49), ("cd_cols64", 0, 0.4, 63), ("cd_cols64", 1, 0.4, 33), ("cd_cols64", 1, 0.4, 48),
             ("cd_cols16", 1, 0.4, 1), ("cd_cols16", 1, 0.4, 16), ("cd_cols32", 1, 0.4, 17), ("cd_cols32", 1, 0.4, 32),
             ("cd_r16_1", 2, 0.4, 1), ("cd_r16_1", 2, 0.4, 16), ("cd_r16_2", 2, 0.4, 17), ("cd_r16_2", 2, 0.4, 32),
             ("cd_r16_3", 2, 0.4, 33), ("cd_r16_3", 2, 0.4, 48), ("ridge_reg", 0, 0.0, 1), ("ridge_reg", 0, 0.0, 32),
             ("ridge", 0, 0.0, 33), ("ridge", 0, 0.0, 63), ("ridge", 1, 0.0, 1), ("ridge", 2, 0.0, 32)]
# (EVAL: the evaluation pass after the register-resident solve; the three-slot kernel hands it to the row16 kernel)


@pytest.mark.parametrize("kernel,variant,alpha,K", FIT_CELLS, ids=[f"{k}-v{v}-K{K}" for k, v, _, K in FIT_CELLS])
def test_fit_every_solver(oracle, kernel, variant, alpha, K):
    w = workloads.small(K=K, n=150, p=77, level_counts=(30, 7), seed=200 + K, alpha=alpha, with_na=K % 2 == 1)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        ds.set_option("cd_variant", variant)
        ds.set_option("profile", 1)
        got = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha,
                          max_iter=5, seed=13)
        assert solver(ds) == kernel
        assert solver(ds, "col_eval") == "none"          # outer iteration 5 is no checkpoint
        total = ds.profile()["sweeps"]
        # one outer iteration: the checkpoint of outer iteration 0 is the last column solve
        one = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha,
                          max_iter=0, seed=13)
        assert solver(ds) == kernel
        assert solver(ds, "col_eval") == EVAL.get(kernel, "none")
    finally:
        ds.close()
    ref = oracle.optimize(w.X, w.levels, w.n_levels, w.A0, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, max_iter=5,
                          seed=13)
    assert got["iters"] == ref["iters"] == 6
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-8
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-8
    if alpha > 0:
        assert abs(total - ref["total_sweeps"]) <= max(3, 0.002 * ref["total_sweeps"])
    ref1 = oracle.optimize(w.X, w.levels, w.n_levels, w.A0, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, max_iter=0,
                           seed=13)
    np.testing.assert_allclose(one["traj"][:, 1:8], ref1["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
    assert relerr(one["column_factor"], ref1["column_factor"]) < 1e-9


# ----------------------------------------------------------------------------------------------------------------------
# c. whole fits at K > 48: the NB = 4 statistics and row update with k_cd_cols<64, 1>
# ----------------------------------------------------------------------------------------------------------------------
PATHS = {"fast": dict(row_merged=2, col_factored=2, row_counts=0), "pair": dict(row_merged=2, col_factored=3, row_counts=1),
         "lists": dict(row_merged=0, col_factored=0)}
WIDE = {"k49": dict(K=49), "k56": dict(K=56), "k62": dict(K=62), "k63": dict(K=63),
        "k56_ridge": dict(K=56, alpha=0.0), "k62_na": dict(K=62, with_na=True)}


def _wide(case):
    return workloads.small(n=150, p=60, **WIDE[case])


@pytest.mark.parametrize("paths", list(PATHS))
@pytest.mark.parametrize("case", list(WIDE))
def test_wide_fit_one_iteration(oracle, case, paths):
    w = _wide(case)
    rng = np.random.default_rng(5)
    A = [np.asfortranarray(rng.standard_normal(a.shape) * 0.3) for a in w.A0]
    C = np.asfortranarray(rng.standard_normal(w.C0.shape) * 0.3)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        for k, v in PATHS[paths].items():
            ds.set_option(k, v)
        got = ds.optimize([a.copy(order="F") for a in A], C.copy(order="F"), w.K, w.lam, w.lam, w.alpha, max_iter=0,
                          seed=17)
        assert solver(ds) == ("ridge" if w.alpha == 0 else "cd_cols64")
    finally:
        ds.close()
    ref = oracle.optimize(w.X, w.levels, w.n_levels, A, C, w.M_train, w.M_test, w.lam, w.lam, w.alpha, max_iter=0,
                          seed=17)
    assert got["iters"] == ref["iters"]
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-9
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-9
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)


@pytest.mark.parametrize("paths", list(PATHS))
@pytest.mark.parametrize("case", list(WIDE))
def test_wide_fit_31_iterations(oracle, case, paths):
    w = _wide(case)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        for k, v in PATHS[paths].items():
            ds.set_option(k, v)
        got = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha,
                          max_iter=30, seed=23)
        assert solver(ds) == ("ridge" if w.alpha == 0 else "cd_cols64")
    finally:
        ds.close()
    ref = oracle.optimize(w.X, w.levels, w.n_levels, w.A0, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha,
                          max_iter=30, seed=23)
    assert got["iters"] == ref["iters"] == 31
    assert list(got["traj"][:, 0]) == [-1, 0, 10, 20, 30]
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
    assert np.array_equal(got["traj"][:, 9], ref["traj"][:, 9])
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-6
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-6
    assert got["loss"] == pytest.approx(ref["loss"], rel=1e-9)


# ----------------------------------------------------------------------------------------------------------------------
# d. the batch entry (insider_hip_strong_cd) where lambda alpha = 0, and at K >= 49
# ----------------------------------------------------------------------------------------------------------------------
BATCH = [("alpha0", K) for K in (1, 7, 16, 17, 31, 32, 33, 40, 48, 49, 63, 64)] + \
        [("lambda0", K) for K in (1, 7, 16, 17, 31, 32, 33, 40, 48, 49, 63, 64)] + \
        [("enet", K) for K in (49, 50, 55, 62, 63)]


@pytest.mark.parametrize("regime,K", BATCH, ids=[f"{r}-K{K}" for r, K in BATCH])
def test_strong_cd_batch_every_solver(oracle, regime, K):
    rng = np.random.default_rng(300 + K + len(regime))
    B, m = 9, 3 * K + 20                                 # m >= 3K: G well conditioned for lambda = 0
    Xs = rng.standard_normal((B, m, K))
    bt = rng.standard_normal((B, K)) * (rng.random((B, K)) < 0.5)
    ys = np.einsum("bmk,bk->bm", Xs, bt) + 0.3 * rng.standard_normal((B, m))
    Gs = np.einsum("bmk,bml->bkl", Xs, Xs)
    qs = np.einsum("bmk,bm->bk", Xs, ys)
    ws = 0.1 * rng.standard_normal((B, K))
    lam, alpha = {"alpha0": (3.0, 0.0), "lambda0": (0.0, 0.5), "enet": (0.35 * float(np.max(np.abs(qs))), 0.6)}[regime]
    for mode in (0, 1):
        for cap in (3, UNCAPPED):
            beta, sw = api.strong_coordinate_descent(None, None, ws, lam, alpha, Gs, qs, tol=TOL, seed=5, it=3,
                                                     order_mode=mode, max_sweeps=cap, return_sweeps=True)
            assert _lib.COL_SOLVERS[_lib.load().insider_hip_last_cd_solver()] == \
                expected("enet" if regime == "enet" else "nol1", 0, K), (mode, cap)
            for b in range(B):
                ob, osw = oracle.strong_cd(Xs[b], ys[b], ws[b], lam, alpha, Gs[b], qs[b], tol=TOL, seed=5, unit=b, it=3,
                                           order_mode=mode, max_sweeps=cap)
                if cap == 3:
                    assert sw[b] == osw, (mode, b, sw[b], osw)
                    assert np.max(np.abs(ob - beta[b])) < 1e-10 * max(1.0, np.max(np.abs(ob))), (mode, b)
                else:
                    assert abs(osw - sw[b]) <= 1, (mode, b, osw, sw[b])
                    assert np.max(np.abs(ob - beta[b])) < (1e-9 if osw == sw[b] else 50 * np.sqrt(TOL)), (mode, b)
                    assert np.array_equal(ob == 0, beta[b] == 0)


# ----------------------------------------------------------------------------------------------------------------------
# e. the batch entry past one chunk: strong_cd_device() solves CD_BATCH_DOUBLES / stat_len problems per launch
# ----------------------------------------------------------------------------------------------------------------------
CD_BATCH_DOUBLES = 1 << 26
GEN_BLOCK = 4096                       # problems generated at a time (their design matrices are not kept)
CHUNKED = [(1, "enet"), (17, "enet"), (17, "lambda0"), (49, "enet")]


def _batch_chunk(K):
    """chunk = 2^26 / stat_len, stat_len = NB (NB + 1) / 2 * 256 doubles per record: 262144, 87381 and 26214 problems."""
    NB = (K + 16) // 16
    return CD_BATCH_DOUBLES // (NB * (NB + 1) // 2 * 256)


def _batch_block(K, b, count):
    """Problems b * GEN_BLOCK ... of the batch, built as in test_strong_cd_batch_every_solver from a stream keyed by the block."""
    rng = np.random.default_rng([300 + K, b])
    m = 3 * K + 20
    Xs = rng.standard_normal((count, m, K), dtype=np.float32).astype(np.float64)     # (single-precision draws: half the time)
    bt = rng.standard_normal((count, K)) * (rng.random((count, K)) < 0.5)
    ys = np.matmul(Xs, bt[:, :, None])[:, :, 0] + 0.3 * rng.standard_normal((count, m))
    ws = 0.1 * rng.standard_normal((count, K))
    return Xs, ys, ws


@pytest.mark.parametrize("K,regime", CHUNKED, ids=[f"{r}-K{K}" for K, r in CHUNKED])
def test_strong_cd_batch_past_one_chunk(oracle, K, regime):
    chunk = _batch_chunk(K)
    assert chunk == {1: 262144, 17: 87381, 49: 26214}[K]
    nprob = chunk + 3
    Gs, qs, ws = np.empty((nprob, K, K)), np.empty((nprob, K)), np.empty((nprob, K))
    for b in range(-(-nprob // GEN_BLOCK)):
        lo, hi = b * GEN_BLOCK, min((b + 1) * GEN_BLOCK, nprob)
        Xs, ys, ws[lo:hi] = _batch_block(K, b, hi - lo)
        np.matmul(Xs.transpose(0, 2, 1), Xs, out=Gs[lo:hi])
        qs[lo:hi] = np.matmul(Xs.transpose(0, 2, 1), ys[:, :, None])[:, :, 0]
    lam, alpha = {"lambda0": (0.0, 0.5), "enet": (0.35 * float(np.max(np.abs(qs[:9]))), 0.6)}[regime]
    probe = [0, 1, chunk - 2, chunk - 1, chunk, chunk + 1, chunk + 2]
    alone = np.r_[chunk - 64:chunk + 3]           # the last 64 problems of the first chunk and the 3 of the second
    for cap in (3, UNCAPPED):
        beta, sw = api.strong_coordinate_descent(None, None, ws, lam, alpha, Gs, qs, tol=TOL, seed=5, it=3, max_sweeps=cap,
                                                 return_sweeps=True)
        assert _lib.COL_SOLVERS[_lib.load().insider_hip_last_cd_solver()] == \
            expected("enet" if regime == "enet" else "nol1", 0, K), cap
        # against the oracle: what a wrong offset of a chunk's Gram matrices, solutions or sweep counts would fail
        for j in probe:
            Xs, ys, _ = _batch_block(K, j // GEN_BLOCK, min(GEN_BLOCK, nprob - j // GEN_BLOCK * GEN_BLOCK))
            i = j % GEN_BLOCK
            ob, osw = oracle.strong_cd(Xs[i], ys[i], ws[j], lam, alpha, Gs[j], qs[j], tol=TOL, seed=5, unit=j, it=3,
                                       max_sweeps=cap)
            if cap == 3:
                assert sw[j] == osw, (j, sw[j], osw)
                assert np.max(np.abs(ob - beta[j])) < 1e-10 * max(1.0, np.max(np.abs(ob))), j
            else:
                assert abs(osw - sw[j]) <= 1, (j, osw, sw[j])
                assert np.max(np.abs(ob - beta[j])) < (1e-9 if osw == sw[j] else 50 * np.sqrt(TOL)), j
                assert np.array_equal(ob == 0, beta[j] == 0)
        # across the chunks: the chunking changes no result, so the same problems solved in a call of their own give the same bits
        beta1, sw1 = api.strong_coordinate_descent(None, None, ws[alone], lam, alpha, Gs[alone], qs[alone], tol=TOL, seed=5,
                                                   it=3, max_sweeps=cap, return_sweeps=True)
        assert np.array_equal(sw1, sw[alone]), (cap, np.nonzero(sw1 != sw[alone]))
        assert np.array_equal(beta1, beta[alone]), (cap, np.nonzero((beta1 != beta[alone]).any(1)))


# ----------------------------------------------------------------------------------------------------------------------
# the upper edge of the band
# ----------------------------------------------------------------------------------------------------------------------
def test_k64_is_unsupported_and_leaves_the_factors_untouched():
    w = workloads.small(K=4, n=80, p=40)
    rng = np.random.default_rng(64)
    A = [np.asfortranarray(rng.standard_normal((int(L), 64))) for L in w.n_levels]
    C = np.asfortranarray(rng.standard_normal((64, w.X.shape[1])))
    A0, C0 = [a.copy() for a in A], C.copy()
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        with pytest.raises(_lib.InsiderError) as e:
            ds.optimize(A, C, 64, 1.0, 1.0, 0.4, max_iter=2, copy=False)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.InsiderError) as e:
            ds.optimize_col(A, C, lambda_=1.0, alpha=0.4)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        assert all(np.array_equal(a, a0) for a, a0 in zip(A, A0)) and np.array_equal(C, C0)
        # the handle stays usable
        got = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha,
                          max_iter=1, seed=3)
        assert np.isfinite(got["loss"])
    finally:
        ds.close()
