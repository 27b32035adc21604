"""What every post-hoc call on the resident data set owes the fit: a sharded handle is refused with ERR_UNSUPPORTED (by the
raw C entry too, with its outputs untouched, where the row has ``raw``), and calls between two fits, one of them refused
half-way, leave the second fit's bits as they are.  One row of CALLS per call:
    invoke(ds, A, C, entries)   the Python call; entries None = the call's defaults, as the sharded handle gets it
    invoke_bad(ds, A, C)        a call the library refuses
    raw(ds, w)                  optional: the C entry on the sharded handle -> (status, sentinel-filled outputs)
    fit                         optional: the workload, max_iter and whether a first fit precedes the calls, where they are
                                not those of the other rows"""
import numpy as np
import pytest

from insider_amd import _lib, api, workloads
from tests.support import need_gpu  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
FIT = dict(small=dict(n=90, p=140, K=6), max_iter=12, prefit=True)


def _kw(entries):
    return {} if entries is None else {"entries": entries}


def _outliers(ds, A, C, entries):
    if entries is None:
        return ds.outliers(A, C, np.ones(ds.p))
    got = ds.outliers(A, C, np.ones(ds.p), threshold=0.5, entries=entries)
    assert got["total"] > 0


def _residual_products(ds, A, C, entries):
    if entries is None:
        return ds.residual_products(A, C, np.asfortranarray(np.ones((ds.n, 2))))
    return ds.residual_products(A, C, np.random.default_rng(0).standard_normal((ds.n, 10)), entries=entries)


def _residual_products_raw(ds, w):
    Q = np.asfortranarray(np.ones((48, 2)))
    _, Cw, Aptrs = ds._marshal(w.A0, w.C0, 3, 0)
    outs = np.full((64, 2), -7.0, order="F"), np.full((48, 2), -7.0, order="F"), np.full(64, -7.0)
    return _lib.load().insider_hip_residual_products(ds._h, Aptrs, _lib.ptr(Cw), 0, 3, 1, None, None, _lib.ptr(Q), 2,
                                                     *(_lib.ptr(o) for o in outs)), outs


def _level_scores(ds, A, C, entries):
    if entries is None:
        return ds.level_scores(A, C, 0)
    for cov in range(ds.c):
        ds.level_scores(A, C, cov, entries=entries)


def _level_scores_raw(ds, w):
    _, Cw, Aptrs = ds._marshal(w.A0, w.C0, 3, 0)
    outs = np.full((48, int(ds.n_levels[0])), -7.0, order="F"), np.full(48, -7.0)
    return _lib.load().insider_hip_level_scores(ds._h, Aptrs, _lib.ptr(Cw), 0, 3, 1, 0, None, 0,
                                                *(_lib.ptr(o) for o in outs)), outs


CALLS = {
    "variance_decomposition": dict(invoke=lambda ds, A, C, e: ds.variance_decomposition(A, C, **_kw(e)),
                                   invoke_bad=lambda ds, A, C: ds.variance_decomposition(A, C, inc_continuous=1)),
    "sample_decomposition": dict(invoke=lambda ds, A, C, e: ds.sample_decomposition(A, C, **_kw(e)),
                                 invoke_bad=lambda ds, A, C: ds.sample_decomposition(A, C, inc_continuous=1)),
    # the one call made on a handle that has not fitted yet: its work space is the first the handle allocates
    "factor_decomposition": dict(invoke=lambda ds, A, C, e: ds.factor_decomposition(A, C, **_kw(e)),
                                 invoke_bad=lambda ds, A, C: ds.factor_decomposition(A, C, inc_continuous=1),
                                 fit=dict(small={}, max_iter=5, prefit=False)),
    "outliers": dict(invoke=_outliers, invoke_bad=lambda ds, A, C: ds.outliers(A, C, np.ones(ds.p), inc_continuous=1)),
    "residual_products": dict(invoke=_residual_products, raw=_residual_products_raw,
                              invoke_bad=lambda ds, A, C: ds.residual_products(
                                  A, C, np.random.default_rng(0).standard_normal((ds.n, 10))[:-1])),
    "level_scores": dict(invoke=_level_scores, raw=_level_scores_raw,
                         invoke_bad=lambda ds, A, C: ds.level_scores(A, C, ds.c)),
}


@pytest.mark.parametrize("call", CALLS)
def test_refuses_a_sharded_handle(call):
    row = CALLS[call]
    w = workloads.small(n=48, p=64, K=3)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        ds.set_shard(0, 0, 2, allreduce=lambda ptr, count, stream: None)
        with pytest.raises(_lib.InsiderError) as e:
            row["invoke"](ds, w.A0, w.C0, None)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        if "raw" in row:
            status, outs = row["raw"](ds, w)
            assert status == _lib.ERR_UNSUPPORTED
            assert all(np.all(o == -7.0) for o in outs)
    finally:
        ds.close()


@pytest.mark.parametrize("call", CALLS)
def test_leaves_optimize_bit_identical(call):
    row = CALLS[call]
    fit = row.get("fit", FIT)
    w = workloads.small(**fit["small"])

    def run(with_calls):
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        try:
            A = [a.copy(order="F") for a in w.A0]
            Cm = w.C0.copy(order="F")
            if fit["prefit"]:
                r1 = ds.optimize(A, Cm, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=fit["max_iter"], seed=3)
                A = [a.copy(order="F") for a in r1["row_matrices"].values()]
                Cm = r1["column_factor"].copy(order="F")
            if with_calls:
                for e in ENTRIES:
                    row["invoke"](ds, A, Cm, e)
                with pytest.raises(_lib.InsiderError):
                    row["invoke_bad"](ds, A, Cm)
            return ds.optimize(A, Cm, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=fit["max_iter"], seed=3)
        finally:
            ds.close()

    ref, got = run(False), run(True)
    for a, b in zip(ref["row_matrices"].values(), got["row_matrices"].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(ref["column_factor"], got["column_factor"])
    assert np.array_equal(ref["traj"], got["traj"], equal_nan=True)
