"""The HIP library against what the reference's OWN compiled code computed: the fixtures of tests/golden/reference/, written by
tests/golden/make_reference_golden.py from oracle/_ref/insider_ref (the reference's translation units, unmodified, over the
stand-in headers of oracle/ref_shim).  No hand restatement of the algorithm stands between the reference's program text and
these assertions.  Only the fixtures are read: neither the reference tree nor the binary exists where this runs.

Everything runs with the cyclic sweep order (order_mode = 1), the compiled reference's one order.  No tolerance is new: each is
the one the existing GPU tests apply against the oracle for the same entry, cited at its use.  Values that come from the
reference's log carry its 12-digit quantisation (5e-12 relative) on top.
"""
import glob
import json
import os

import numpy as np
import pytest

from insider_amd import _lib, api, workloads
from tests import reference_cases as RC
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
LOG_Q = 5e-12


def _load(name):
    with np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _names(prefix):
    return sorted(os.path.basename(p)[len(prefix):-4] for p in glob.glob(os.path.join(DIR, prefix + "*.npz")))


def test_every_group_has_its_fixtures():
    assert _names("cd_") == sorted(["k%d" % k for k in RC.CD_KS] + ["kkt"])
    assert _names("continuous_") == sorted(RC.CONTINUOUS_CASES)
    assert _names("optimize_short_") == sorted(RC.optimize_names("optimize_short"))
    assert _names("optimize_long_") == sorted(RC.optimize_names("optimize_long"))


# ---- strong_coordinate_descent -------------------------------------------------------------------------------------------
def _cd_variants(f):
    if "variants" in f:
        return [(str(v), f[str(v) + "_wstart"], float(f[str(v) + "_lam"]), float(f[str(v) + "_alpha"]), f[str(v) + "_beta"],
                 int(f[str(v) + "_sweeps"])) for v in f["variants"]]
    return [("kkt", f["wstart"], float(f["lam"]), float(f["alpha"]), f["beta"], int(f["sweeps"]))]


def _check_cd(beta, sw, ref, ref_sw, what):
    assert abs(int(sw) - ref_sw) <= 1, (what, sw, ref_sw)                                       # tests/test_gpu_boundary.py:113
    assert np.max(np.abs(beta - ref)) < 1e-8 * max(1.0, np.max(np.abs(ref))), what               # tests/test_gpu_boundary.py:112
    assert np.array_equal(beta == 0, ref == 0), what                                            # tests/test_gpu_boundary.py:113


@pytest.mark.parametrize("name", ["k%d" % k for k in RC.CD_KS] + ["kkt"])
def test_strong_cd_standalone(name):
    """api.strong_coordinate_descent in its covariance form (XtX, Xty) and its (X, y) form."""
    f = _load("cd_" + name)
    tol = float(f["tol"])
    for v, w0, lam, alpha, ref, ref_sw in _cd_variants(f):
        for args in ((None, None, f["XtX"], f["Xty"]), (f["X"], f["y"], None, None)):
            beta, sw = api.strong_coordinate_descent(args[0], args[1], w0, lam, alpha, args[2], args[3], tol=tol, order_mode=1,
                                                     return_sweeps=True)
            _check_cd(beta, sw, ref, ref_sw, (name, v, args[0] is None))
    if name == "kkt":      # the coordinate the strong rule discards is back in the model
        assert f["excluded"][1] and beta[1] != 0.0


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", ["k%d" % k for k in RC.CD_KS] + ["kkt"])
def test_strong_cd_through_the_column_update(name, variant):
    """The same problems as ONE gene of a data set whose samples each have their own level (row factor = X, data = y), so that the
    column update's kernels solve them under every cd_variant (the stand-alone entry only runs the default one)."""
    f = _load("cd_" + name)
    X, y, tol = f["X"], f["y"], float(f["tol"])
    m, K = X.shape
    levels = np.asfortranarray(np.arange(1, m + 1, dtype=np.int32).reshape(m, 1))
    ones = np.ones((m, 1), dtype=np.uint8, order="F")
    ds = api.InsiderData(np.asfortranarray(y.reshape(m, 1)), levels, ones, np.zeros_like(ones))
    try:
        ds.set_option("cd_variant", variant)
        ds.set_option("order_mode", 1)
        for v, w0, lam, alpha, ref, ref_sw in _cd_variants(f):
            got = ds.optimize_col([np.asfortranarray(X)], np.asfortranarray(w0.reshape(K, 1)), lambda_=lam, alpha=alpha, tuning=0, tol=tol)
            _check_cd(got[:, 0], ds.sweeps()[0], ref, ref_sw, (name, v, variant))
    finally:
        ds.close()


# ---- the block updates ---------------------------------------------------------------------------------------------------
def _op_handle(f):
    return api.InsiderData(f["X"], f["levels"], f["M_train"], f["M_test"])


def test_optimize_row():
    """insider_hip_optimize_row, tuning 1 and 0, lambda = 0 included (fit_interaction's arithmetic)."""
    f = _load("row")
    ds = _op_handle(f)
    try:
        for name in f["cases"]:
            name = str(name)
            cov = int(f[name + "_cov"])
            A = [f["A0"].copy(order="F"), f["A1"].copy(order="F")]
            got = ds.optimize_row(A, f["C"].copy(order="F"), cov, lambda_=float(f[name + "_lam"]), tuning=int(f[name + "_tuning"]))
            assert relerr(got, f[name + "_factor"]) < 1e-9, (name, relerr(got, f[name + "_factor"]))   # tests/test_gpu_row_update.py:244
    finally:
        ds.close()


def test_optimize_col():
    f = _load("col")
    tol, lam = float(f["tol"]), float(f["lam"])
    ds = _op_handle(f)
    try:
        ds.set_option("order_mode", 1)
        for name in f["cases"]:
            name = str(name)
            alpha, ref, ref_sw = float(f[name + "_alpha"]), f[name + "_c_factor"], int(f[name + "_sweeps"])
            got = ds.optimize_col([f["A0"].copy(order="F"), f["A1"].copy(order="F")], f["C"].copy(order="F"), lambda_=lam, alpha=alpha,
                                  tuning=int(f[name + "_tuning"]), tol=tol)
            if alpha == 0.0:
                assert relerr(got, ref) < 1e-10, (name, relerr(got, ref))                          # tests/test_gpu_col_solvers.py:119
                continue
            total = int(ds.sweeps().sum())
            assert abs(total - ref_sw) <= max(3, 0.002 * ref_sw), (name, total, ref_sw)             # tests/test_gpu_parity.py:406
            err = np.max(np.abs(got - ref))
            assert err < (1e-9 if total == ref_sw else 50 * np.sqrt(tol)), (name, err)              # tests/test_gpu_col_solvers.py:159
            assert np.array_equal(got == 0, ref == 0), name                                        # tests/test_gpu_col_solvers.py:160
    finally:
        ds.close()


@pytest.mark.parametrize("name", list(RC.CONTINUOUS_CASES))
def test_optimize_continuous_v2_symbol(name):
    """The raw insider_hip_optimize_continuous_v2 symbol, as tests/test_gpu_boundary.py:137-144 calls it."""
    import ctypes as C
    f = _load("continuous_" + name)
    D, M, Cm, z, gram = (np.asfortranarray(f[k]) for k in ("data", "indicator", "c_factor", "confd", "gram"))
    n, p = D.shape
    K, tuning, lam = Cm.shape[0], int(f["tuning"]), float(f["lam"])
    u = np.ascontiguousarray(f["u"], dtype=np.float64).copy()
    dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    lib = _lib.load()
    rc = lib.insider_hip_optimize_continuous_v2(D.ctypes.data_as(dp), n, p, M.ctypes.data_as(u8) if tuning == 1 else None,
                                                u.ctypes.data_as(dp), Cm.ctypes.data_as(dp), K, z.ctypes.data_as(dp),
                                                gram.ctypes.data_as(dp) if tuning == 0 else None, lam, tuning, 0)
    assert rc == _lib.OK, lib.insider_hip_last_error()
    assert relerr(u, f["u_out"]) < 1e-9 and not np.allclose(u, f["u"])                             # tests/test_gpu_boundary.py:144


# ---- optimize() ----------------------------------------------------------------------------------------------------------
def _ladder(delta):
    """The decay the reference sets at a checkpoint from its delta loss (src/optimize.cpp:389-403)."""
    for d in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1):
        if delta / 1000 <= d:
            return d
    return 1.0


def _fixture_inputs(f):
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(f["kw"])).items()}
    w = workloads.small(**kw)
    A = [a.copy(order="F") for a in w.A0]
    Z = None
    if int(f["continuous"]):
        Z, U0 = RC.continuous_extra(w)
        A.append(U0)
    assert RC.input_hashes(w, A, Z) == json.loads(str(f["hashes"])), "the generated inputs are no longer those the fixture was recorded on"
    return w, A, Z, json.loads(str(f["fit"]))


def _identity_allreduce(ptr, count, stream):
    return None


OPTION_SETS = {"default": {}, "row_lists": dict(row_merged=0), "col_lists": dict(col_factored=0), "allreduce": dict(force_allreduce=1)}


def _fit_and_check(group, name, opts, factor_tol):
    f = _load("%s_%s" % (group, name))
    w, A, Z, fit = _fixture_inputs(f)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, ctns_confounder=Z)
    try:
        ds.set_option("order_mode", 1)
        if opts == "allreduce":      # world of one rank: the sum over ranks is the identity
            ds.set_shard(0, 0, 1, allreduce=_identity_allreduce)
        for k, v in OPTION_SETS[opts].items():
            ds.set_option(k, v)
        got = ds.optimize(A, w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha, tuning=w.tuning, inc_continuous=int(Z is not None), **fit)
    finally:
        ds.close()
    log = f["log"]
    traj = got["traj"]
    # the iterations at which the reference logged, and where it left the loop
    assert list(traj[:, 0]) == list(log[:, 0])
    if int(f["iters"]) >= 0:
        assert got["iters"] == int(f["iters"])
    else:        # the log cannot tell a break at the last checkpoint from running out at max_iter (oracle/ref.py)
        assert got["iters"] in (int(log[-1, 0]), fit["max_iter"] + 1)
    # the decay column: the ladder applied to the reference's own logged delta loss
    assert list(traj[1:, 9]) == [_ladder(d) for d in log[1:, 7]] and traj[0, 9] == 1.0                # tests/test_gpu_parity.py:313,582
    # traj[:, 1:8] against the logged checkpoints (the log has no total: the sum of its four components)
    want = np.column_stack([log[:, 1:7], log[:, 3:7].sum(axis=1)])
    np.testing.assert_allclose(traj[:, 1:8], want, rtol=1e-9 + LOG_Q, equal_nan=True)                 # tests/test_gpu_parity.py:312,583
    n_fac = len(A)
    for i in range(n_fac):
        assert relerr(got["row_matrices"]["factor%d" % i], f["factor%d" % i]) < factor_tol, (i, relerr(got["row_matrices"]["factor%d" % i], f["factor%d" % i]))
    assert relerr(got["column_factor"], f["column_factor"]) < factor_tol, relerr(got["column_factor"], f["column_factor"])
    assert got["loss"] == pytest.approx(float(f["loss"]), rel=1e-9)                                  # tests/test_gpu_parity.py:317,587
    assert got["train_rmse"] == pytest.approx(float(f["train_rmse"]), rel=1e-9)                      # tests/test_gpu_parity.py:687
    if int(f["test_rmse_defined"]):
        assert got["test_rmse"] == pytest.approx(float(f["test_rmse"]), rel=1e-9)                    # tests/test_gpu_parity.py:687
    else:        # never written by the reference under tuning = 0: asserted on the library's side only
        assert w.tuning == 0 and np.isnan(got["test_rmse"])                                          # tests/test_gpu_parity.py:318-319


@pytest.mark.parametrize("name,opts", [(n, "default") for n in RC.optimize_names("optimize_short")]
                         + [(n, o) for n in ("plain", "na", "continuous") for o in ("row_lists", "col_lists", "allreduce")])
def test_optimize_short(name, opts):
    """31 iterations (`early`: until global_tol stops it): factors at 1e-6 (tests/test_gpu_parity.py:315-316; `early` at the 1e-7
    of :529-530)."""
    _fit_and_check("optimize_short", name, opts, 1e-7 if name == "early" else 1e-6)


@pytest.mark.parametrize("name", RC.optimize_names("optimize_long"))
def test_optimize_long(name):
    """400 iterations down the decay ladder (continuous: 200): factors at 1e-7 (tests/test_gpu_parity.py:585-586; continuous at
    the 1e-6 of :613-614)."""
    from tests.test_gpu_parity import LONG_CASES
    log = _load("optimize_long_" + name)["log"]
    lowest = 1e-3 if name == "continuous" else LONG_CASES[name][1]          # tests/test_gpu_parity.py:541-552,608
    assert min(_ladder(d) for d in log[1:, 7]) <= lowest                     # the reference's own fit reaches the case's decay
    _fit_and_check("optimize_long", name, "default", 1e-6 if name == "continuous" else 1e-7)
