"""Host-side checks of the outlier calls (insider_hip_outliers): the numpy yardstick posthoc.outliers_host() agrees with a
naive double loop, posthoc.residual_center_scale() gives the mean and the standard deviation of the masked residual, genes
without a usable scale get no call, and the command line accepts --outliers / --outlier-entries."""
import functools

import numpy as np
import pytest

from insider_amd import fit, posthoc
from tests.support import problem

COUNTS = ("gene_low", "gene_high", "sample_low", "sample_high")


_problem = functools.partial(problem, n=7, p=5, counts=(3, 2), m=1, K=3, scale=0.3)


def _residual(X, lev, Z, A, Cm):
    n, p = X.shape
    r = np.empty((n, p))
    for i in range(n):
        for j in range(p):
            f = 0.0
            for b in range(lev.shape[1]):
                f += float(A[b][lev[i, b] - 1] @ Cm[:, j])
            if Z is not None:
                f += float(Z[i] @ (A[lev.shape[1]] @ Cm[:, j]))
            r[i, j] = X[i, j] - f
    return r


def test_host_calls_match_a_naive_double_loop():
    """7 x 5, K = 3, two categorical blocks, one continuous column and a mask: membership, order, z and the four counts."""
    X, lev, Z, mask, A, Cm = _problem(1)
    n, p = X.shape
    rng = np.random.default_rng(2)
    center, scale = 0.1 * rng.standard_normal(p), 0.5 + rng.random(p)
    t = 0.8
    got = posthoc.outliers_host(X, lev, Z, mask, A, Cm, center, scale, t)
    r = _residual(X, lev, Z, A, Cm)
    rows, cols, zs = [], [], []
    want = {k: np.zeros(p if k.startswith("gene") else n, dtype=np.int64) for k in COUNTS}
    for j in range(p):
        for i in range(n):
            z = (r[i, j] - center[j]) / scale[j]
            if mask[i, j] and abs(z) >= t:
                rows.append(i), cols.append(j), zs.append(z)
                side = "low" if z < 0 else "high"
                want["gene_" + side][j] += 1
                want["sample_" + side][i] += 1
    assert 3 < len(rows) < mask.sum()
    assert got["total"] == len(rows)
    assert np.array_equal(got["rows"], rows) and np.array_equal(got["cols"], cols)
    np.testing.assert_allclose(got["z"], zs, rtol=1e-12, atol=1e-14)
    for k in COUNTS:
        assert np.array_equal(got[k], want[k]), k
    # no center = a center of zeros
    a, b = (posthoc.outliers_host(X, lev, Z, mask, A, Cm, ce, scale, t) for ce in (None, np.zeros(p)))
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["cols"], b["cols"]) and np.array_equal(a["z"], b["z"])


def test_center_and_scale_are_the_mean_and_sd_of_the_masked_residual():
    X, lev, Z, mask, A, Cm = _problem(3, n=23, p=9)
    center, scale = posthoc.residual_center_scale(posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm))
    r = _residual(X, lev, Z, A, Cm)
    for j in range(X.shape[1]):
        rj = r[mask[:, j], j]
        assert rj.size >= 2
        assert abs(center[j] - rj.mean()) <= 1e-10 and abs(scale[j] - rj.std(ddof=1)) <= 1e-10


def test_a_gene_with_fewer_than_two_entries_gets_no_call():
    X, lev, Z, mask, A, Cm = _problem(4, n=11, p=6)
    mask[:, 1] = False                       # n_j = 0
    mask[:, 4] = False
    mask[5, 4] = True                        # n_j = 1
    center, scale = posthoc.residual_center_scale(posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm))
    assert np.isnan(scale[1]) and np.isnan(scale[4]) and np.isnan(center[1]) and np.isfinite(center[4])
    assert np.all(np.isfinite(scale[[0, 2, 3, 5]]))
    got = posthoc.outliers_host(X, lev, Z, mask, A, Cm, center, scale, 1e-3)
    assert got["gene_low"][[1, 4]].sum() == 0 and got["gene_high"][[1, 4]].sum() == 0
    assert not np.isin(got["cols"], (1, 4)).any() and got["total"] > 0
    # the same rule for every unusable scale
    bad = np.array([0.0, -1.0, np.nan, np.inf, 1.0, 1.0])
    got = posthoc.outliers_host(X, lev, Z, None, A, Cm, None, bad, 1e-3)
    assert set(got["cols"]) == {4, 5} and got["total"] == got["gene_low"].sum() + got["gene_high"].sum()
    assert got["total"] == got["sample_low"].sum() + got["sample_high"].sum()


def test_cli_parses_the_outlier_options():
    a = fit.parse(["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2", "--outliers", "3",
                   "--outlier-entries", "test"])
    assert a.outliers == 3.0 and a.outlier_entries == "test"
    a = fit.parse(["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"])
    assert a.outliers is None and a.outlier_entries == "train"
    with pytest.raises(SystemExit):
        fit.parse(["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2",
                   "--outlier-entries", "held-out"])
