"""The compiled reference (oracle/_ref/insider_ref: the reference's own translation units, unmodified, over the stand-in of
oracle/ref_shim) against BOTH oracles on identical inputs, with the cyclic sweep order (order_mode = 1) throughout.

Until this file the oracles were pinned to the reference by reading and by mathematics only; here the reference's program
text itself runs.  No tolerance is new: each comparison takes the one tests/test_oracle_cd.py / tests/test_oracle_optimize.py
apply between the C oracle and the numpy oracle for the same entry (cited at each use) -- those two, like the stand-in, do the
same arithmetic in another summation order.  Quantities read from the reference's log carry its 12-digit quantisation on top
(half a unit of the 12th significant digit: 5e-12 relative).

The numpy oracle is pure Python: it is compared where it finishes in seconds (the cases its own tests run); the C oracle
everywhere.  Skips when oracle/_ref/insider_ref is not built (no reference tree or no C++ compiler).
"""
import numpy as np
import pytest

from oracle import numpy_oracle as NO
from oracle import ref
from tests import reference_cases as RC

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/insider_ref not built (reference tree or C++ compiler absent)")

LOG_Q = 5e-12                                  # the log prints 12 significant digits
ORACLE_LOG_COLS = [0, 1, 2, 3, 4, 5, 6, 8]     # c_oracle.TRAJ_COLS -> ref.LOG_COLS (the log has no total-loss and no decay column)
WORST = {}                                     # entry -> largest observed error, printed by the last test


def _note(entry, err):
    WORST[entry] = max(WORST.get(entry, 0.0), float(err))


def test_cases_are_those_of_the_parity_tests():
    from tests.test_gpu_parity import CASES, LONG_CASES, LONG_FIT
    def same(kw, theirs, name):      # the lasso case differs in its seed alone (tests/reference_cases.py says why)
        return (dict(kw, seed=RC.PARITY_LASSO_SEED) if name == "lasso" else kw) == theirs

    for name, kw in RC.SHORT.items():
        assert same(kw, CASES[name], name), name
    for name, kw in RC.LONG.items():
        assert same(kw, LONG_CASES[name][0], name), name
    assert RC.LONG_FIT == {k: v for k, v in LONG_FIT.items() if k != "seed"}        # the seed only feeds the hashed order


# ---- strong_coordinate_descent (src/coordinate_descent.cpp:56-127) --------------------------------------------------------
@pytest.mark.parametrize("K", RC.CD_KS)
def test_strong_cd(oracle, K):
    prob = RC.cd_problem(K, RC.CD_SEEDS[K])
    for name, w0, lam, alpha in RC.cd_variants(prob):
        rb, rs = ref.strong_cd(prob["X"], prob["y"], w0, lam, alpha, prob["XtX"], prob["Xty"], RC.CD_TOL)
        cb, cs = oracle.strong_cd(prob["X"], prob["y"], w0, lam, alpha, prob["XtX"], prob["Xty"], tol=RC.CD_TOL, order_mode=1)
        nb, ns = NO.strong_coordinate_descent(prob["X"], prob["y"], w0, lam, alpha, prob["XtX"], prob["Xty"], tol=RC.CD_TOL,
                                              order_mode=1)
        assert rs == cs == ns, (K, name, rs, cs, ns)                                # tests/test_oracle_cd.py:70
        _note("cd", max(np.abs(rb - cb).max(), np.abs(rb - nb).max()))
        np.testing.assert_allclose(cb, rb, rtol=0, atol=1e-13, err_msg=name)        # tests/test_oracle_cd.py:71
        np.testing.assert_allclose(nb, rb, rtol=0, atol=1e-13, err_msg=name)        # tests/test_oracle_cd.py:71
        assert np.array_equal(rb == 0, cb == 0), (K, name)
        assert rs >= 2 or alpha == 1.0, (K, name)


def test_strong_rule_excludes_and_kkt_loop_readmits(oracle):
    """Asserted on the REFERENCE's result: a coordinate its strong rule (src/coordinate_descent.cpp:74) discards comes back
    non-zero, which only the KKT re-entry (:118-123) can do; the oracles then agree on values and on the sweep count, which
    includes the sweeps of the second round."""
    c = RC.cd_kkt_problem()
    ex = RC.strong_rule_excluded(c["Xty"], c["lam"], c["alpha"])
    assert ex[1] and not ex[0]
    args = (c["X"], c["y"], c["wstart"], c["lam"], c["alpha"], c["XtX"], c["Xty"])
    rb, rs = ref.strong_cd(*args, c["tol"])
    assert rb[1] != 0.0 and rb[0] != 0.0                    # discarded by the rule, re-admitted by the KKT loop
    # without the re-entry the solve ends after the first round: strictly fewer sweeps and beta[1] = 0
    first = NO.strong_coordinate_descent(c["X"][:, ~ex], c["y"], c["wstart"][~ex], c["lam"], c["alpha"], c["XtX"][np.ix_(~ex, ~ex)],
                                         c["Xty"][~ex], tol=c["tol"], order_mode=1)[1]
    assert rs > first
    cb, cs = oracle.strong_cd(*args, tol=c["tol"], order_mode=1)
    nb, ns = NO.strong_coordinate_descent(*args, tol=c["tol"], order_mode=1)
    assert rs == cs == ns                                                           # tests/test_oracle_cd.py:70
    _note("cd", max(np.abs(rb - cb).max(), np.abs(rb - nb).max()))
    np.testing.assert_allclose(cb, rb, rtol=0, atol=1e-13)                          # tests/test_oracle_cd.py:71
    np.testing.assert_allclose(nb, rb, rtol=0, atol=1e-13)                          # tests/test_oracle_cd.py:71


# ---- the block updates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.ROW_CASES))
def test_optimize_row(oracle, name):
    """Tuning 1 and 0, and lambda = 0: the arithmetic of fit_interaction (src/fit_interaction.cpp:37-54,73-82), whose own call
    the stand-in refuses (a K x 1 result assigned to a 1 x K row view)."""
    c = RC.ROW_CASES[name]
    w, A, C = RC.op_workload()
    resid, gram = RC.row_inputs(w, A, C, c["cov"])
    lev = w.levels[:, c["cov"]]
    r = ref.optimize_row(resid, w.M_train, A[c["cov"]], C, lev, gram, c["lam"], c["tuning"])
    a_c = oracle.optimize_row(resid, w.M_train, A[c["cov"]], C, lev, gram, c["lam"], c["tuning"])
    a_n = NO.optimize_row(resid, w.M_train, A[c["cov"]], C, lev, gram, c["lam"], c["tuning"])
    _note("row", max(np.abs(r - a_c).max(), np.abs(r - a_n).max()))
    np.testing.assert_allclose(a_c, r, rtol=1e-10, atol=1e-12)                      # tests/test_oracle_optimize.py:47
    np.testing.assert_allclose(a_n, r, rtol=1e-10, atol=1e-12)                      # tests/test_oracle_optimize.py:47
    assert not np.allclose(r, A[c["cov"]])


@pytest.mark.parametrize("name", list(RC.COL_CASES))
def test_optimize_col(oracle, name):
    c = RC.COL_CASES[name]
    w, A, C = RC.op_workload()
    R = RC.row_factor(w, A)
    r, rs = ref.optimize_col(w.X, w.M_train, R, C, RC.COL_LAM, c["alpha"], c["tuning"], RC.COL_TOL)
    c_c, sw_c = oracle.optimize_col(w.X, w.M_train, R, C, RC.COL_LAM, c["alpha"], c["tuning"], tol=RC.COL_TOL, order_mode=1)
    c_n, sw_n = NO.optimize_col(w.X, w.M_train, R, C, RC.COL_LAM, c["alpha"], c["tuning"], RC.COL_TOL, order_mode=1)
    assert rs == sw_c == sw_n and (rs > 0) == (c["alpha"] != 0.0)                   # tests/test_oracle_optimize.py:57
    _note("col", max(np.abs(r - c_c).max(), np.abs(r - c_n).max()))
    np.testing.assert_allclose(c_c, r, rtol=1e-9, atol=1e-11)                       # tests/test_oracle_optimize.py:58
    np.testing.assert_allclose(c_n, r, rtol=1e-9, atol=1e-11)                       # tests/test_oracle_optimize.py:58


@pytest.mark.parametrize("name", list(RC.CONTINUOUS_CASES))
def test_optimize_continuous_v2(oracle, name):
    """Tuning 1 and 0; tuning 0 with a `gram` that is not C C' (the caller's gram, whatever it holds)."""
    c = RC.continuous_inputs(*RC.CONTINUOUS_CASES[name])
    args = (c["data"], c["indicator"], c["u"], c["c_factor"], c["confd"], c["gram"], c["lam"], c["tuning"])
    r = ref.optimize_continuous(*args)
    uc = oracle.optimize_continuous(*args)
    un = NO.optimize_continuous_v2(*args)
    _note("continuous", max(np.abs(r - uc).max(), np.abs(r - un).max()))
    np.testing.assert_allclose(uc, r, rtol=1e-10, atol=1e-12)                       # tests/test_oracle_optimize.py:156
    np.testing.assert_allclose(un, r, rtol=1e-10, atol=1e-12)                       # tests/test_oracle_optimize.py:156
    assert not np.allclose(r, c["u"])


@pytest.mark.parametrize("tuning", [1, 0])
def test_predict_evaluate_compute_loss_on_a_fixed_state(tuning):
    """predict, evaluate and both compute_loss (src/utils.cpp:46-102) against the numpy oracle's and against direct numpy, at
    the rel 1e-11 tests/test_oracle_optimize.py:95-100 holds the oracle's components to."""
    w, A, C = RC.op_workload()
    R = RC.row_factor(w, A)
    rng = np.random.default_rng(4)
    cd_res, cd_beta = rng.standard_normal(30), rng.standard_normal(w.K) * (rng.random(w.K) < 0.7)
    o = ref.state(w.X, R, A, C, w.M_train, w.M_test, 1.3, 2.1, 0.4, tuning, cd_res, cd_beta)
    pred = R @ C
    assert np.all(np.abs(o["predictions"] - pred) <= 1e-11 * (np.abs(R) @ np.abs(C)))
    resid = w.X - o["predictions"]
    sse, tr, te = NO.evaluate(resid, w.M_train != 0, w.M_test != 0, tuning)[:3]
    assert o["sum_residual"] == pytest.approx(sse, rel=1e-11) and o["train_rmse"] == pytest.approx(tr, rel=1e-11)
    if tuning == 1:
        assert o["test_rmse"] == pytest.approx(te, rel=1e-11)
        assert o["test_rmse"] == pytest.approx(np.sqrt(np.mean(resid[w.M_test != 0] ** 2)), rel=1e-11)
    else:
        assert "test_rmse" not in o             # never written by the reference under tuning = 0 (src/utils.cpp:61-64)
    loss = NO.compute_loss(A, C, 1.3, 2.1, 0.4, o["sum_residual"])
    assert o["loss"] == pytest.approx(loss[0], rel=1e-11)
    assert o["cd_loss"] == pytest.approx(NO.compute_sub_loss(cd_res, cd_beta, 2.1, 0.4), rel=1e-11)
    t = o["traj"][0]                            # what the two functions print, to 12 digits
    comps = [o["sum_residual"] / 2, 1.3 * sum(np.sum(a ** 2) for a in A) / 2, 2.1 * 0.6 * np.sum(C ** 2) / 2, 2.1 * 0.4 * np.abs(C).sum()]
    np.testing.assert_allclose(t[3:7], comps, rtol=1e-11 + LOG_Q)
    assert t[1] == pytest.approx(o["train_rmse"], rel=LOG_Q)
    assert o["loss"] == pytest.approx(sum(comps), rel=1e-11)


# ---- optimize() (src/optimize.cpp:255-422) --------------------------------------------------------------------------------
NUMPY_TOO = ("plain", "unmasked", "na", "ridge", "interaction", "continuous")     # what tests/test_oracle_optimize.py:66-67,159 run


def _fit(oracle, name, which):
    case = RC.optimize_case("optimize_short", name)
    w, A, Z = RC.optimize_inputs(case)
    if which == "ref":
        return ref.optimize(w.X, w.levels, A, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, tuning=w.tuning, ctns=Z, **case["fit"])
    if which == "c":
        return oracle.optimize(w.X, w.levels, w.n_levels, A, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, tuning=w.tuning,
                               order_mode=1, ctns=Z, **case["fit"])
    return NO.optimize(w.X, A, w.C0, w.levels, w.M_train, w.M_test, w.lam, w.lam, w.alpha, tuning=w.tuning, order_mode=1,
                       ctns_confounder=Z, **case["fit"])


def _compare_fit(name, r, o, tuning):
    # iteration count and sweep total: equal, as tests/test_oracle_optimize.py:74 has them
    assert list(r["traj"][:, 0]) == list(o["traj"][:, 0]), name
    assert r["total_sweeps"] == o["total_sweeps"], (name, r["total_sweeps"], o["total_sweeps"])
    if r["iters"] is not None:
        assert r["iters"] == o["iters"], name
    # checkpoint by checkpoint: the four loss components, both RMSEs, delta loss (tests/test_oracle_optimize.py:75, plus the
    # log's quantisation)
    ot = o["traj"][:, ORACLE_LOG_COLS]
    with np.errstate(invalid="ignore", divide="ignore"):
        _note("optimize traj (rel)", np.nanmax(np.abs(ot[:, 1:] - r["traj"][:, 1:]) / np.abs(ot[:, 1:])))
    np.testing.assert_allclose(r["traj"], ot, rtol=1e-9 + LOG_Q, atol=1e-12, equal_nan=True, err_msg=name)
    _note("optimize factors", np.abs(o["column_factor"] - r["column_factor"]).max())
    np.testing.assert_allclose(o["column_factor"], r["column_factor"], rtol=1e-8, atol=1e-10)      # tests/test_oracle_optimize.py:76
    assert len(o["row_matrices"]) == len(r["row_matrices"])
    for a, b in zip(o["row_matrices"], r["row_matrices"]):
        _note("optimize factors", np.abs(a - b).max())
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-10)                                    # tests/test_oracle_optimize.py:78
    assert o["loss"] == pytest.approx(r["loss"], rel=1e-10)                                        # tests/test_oracle_optimize.py:79
    assert o["train_rmse"] == pytest.approx(r["train_rmse"], rel=1e-10)
    if tuning == 1:
        assert o["test_rmse"] == pytest.approx(r["test_rmse"], rel=1e-10)
    else:       # the reference never writes test_rmse under tuning = 0: asserted on our side only (tests/test_oracle_optimize.py:81)
        assert r["test_rmse"] is None and np.isnan(o["test_rmse"])


@pytest.mark.parametrize("name", RC.optimize_names("optimize_short"))
def test_optimize(oracle, name):
    """31 iterations (checkpoints 0, 10, 20, 30 and at least one move of the decay ladder); `early` stops on global_tol."""
    case = RC.optimize_case("optimize_short", name)
    tuning = case["kw"].get("tuning", 1)
    r = _fit(oracle, name, "ref")
    c = _fit(oracle, name, "c")
    if name == "early":
        assert r["iters"] is not None and r["iters"] < case["fit"]["max_iter"]    # the log ends at a checkpoint before max_iter
        assert r["iters"] == c["iters"] == int(r["traj"][-1, 0])
    else:
        assert list(r["traj"][:, 0]) == [-1, 0, 10, 20, 30] and c["iters"] == 31
        if name == "plain":
            assert len(set(c["traj"][:, 9])) > 1                                   # the decay ladder moves within 31 iterations
    if name == "lasso":        # what the case is there for: a latent dimension dead in every gene, in the reference's own result
        assert (~r["column_factor"].any(axis=1)).sum() >= 1
    _compare_fit(name, r, c, tuning)
    if name in NUMPY_TOO:
        _compare_fit(name, r, _fit(oracle, name, "numpy"), tuning)


# ---- the fixtures of tests/golden/reference/ are what the compiled reference writes today -----------------------------------
@pytest.mark.parametrize("group,name", [("cd", "cd_k7"), ("cd", "cd_kkt"), ("row", "row"), ("col", "col"), ("continuous", "continuous_k1_t1"),
                                        ("optimize_short", "optimize_short_plain"), ("optimize_long", "optimize_long_ridge")])
def test_regenerated_fixture_has_the_stored_bytes(group, name):
    """One short case of each group, regenerated (stopping-margin reruns included) and compared array by array, byte for byte
    (the .npz container carries time stamps; the arrays in it are the fixture)."""
    import os

    from tests.golden import make_reference_golden as gen
    [(fname, arrays)] = list(gen.files(group, only=name))
    with np.load(os.path.join(gen.OUT, fname + ".npz"), allow_pickle=False) as z:
        stored = {k: z[k] for k in z.files}
    assert sorted(stored) == sorted(arrays)
    for k, v in arrays.items():
        v = np.asarray(v)
        assert stored[k].dtype == v.dtype and stored[k].shape == v.shape, k
        assert stored[k].tobytes() == v.tobytes(), k


def test_zz_report_largest_errors():
    """Not a check: prints the largest error seen per entry next to the tolerance it was held to (pytest -s)."""
    tol = {"cd": "atol 1e-13", "row": "rtol 1e-10 + atol 1e-12", "col": "rtol 1e-9 + atol 1e-11", "continuous": "rtol 1e-10 + atol 1e-12",
           "optimize traj (rel)": "rtol 1e-9 + 5e-12", "optimize factors": "rtol 1e-8 + atol 1e-10"}
    for k, v in WORST.items():
        print("reference vs oracles, %-22s largest |difference| %.3g   (tolerance %s)" % (k, v, tol[k]))
