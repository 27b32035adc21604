"""Host-side checks of the per-factor decomposition (insider_hip_factor_decomposition): the numpy yardstick
posthoc.factor_decomposition_host() agrees with a naive triple loop and, summed over the factors, with the per-gene
yardstick, fd_derived() marks empty genes, factor_summary() pools the genes, and the command line accepts
--factor-decomposition."""
import functools

import numpy as np
import pytest

from insider_amd import fit, posthoc
from tests.support import problem

RAW = ("n", "sum_x", "sum_xx", "rss", "sum_h", "sum_hh", "sum_rh")


_problem = functools.partial(problem, n=7, p=5, counts=(3, 2), m=1, K=3)


def test_host_record_matches_a_naive_triple_loop():
    """7 x 5, K = 3, two categorical blocks, one continuous column and a mask: every slot by loops over i, j, k."""
    X, lev, Z, mask, A, Cm = _problem(1)
    d = posthoc.factor_decomposition_host(X, lev, Z, mask, A, Cm)
    n, p = X.shape
    K, B = Cm.shape[0], 3
    assert d["sum_h"].shape == (B + 1, K, p) and d["explained"].shape == (B + 1, K, p) and d["r2"].shape == (p,)
    want = {k: np.zeros_like(d[k]) for k in RAW}
    for j in range(p):
        for i in range(n):
            if not mask[i, j]:
                continue
            u = [A[0][lev[i, 0] - 1], A[1][lev[i, 1] - 1], Z[i, 0] * A[2][0]]
            u.append(u[0] + u[1] + u[2])
            f = sum(u[B][k] * Cm[k, j] for k in range(K))
            r = X[i, j] - f
            want["n"][j] += 1
            want["sum_x"][j] += X[i, j]
            want["sum_xx"][j] += X[i, j] ** 2
            want["rss"][j] += r * r
            for b in range(B + 1):
                for k in range(K):
                    h = u[b][k] * Cm[k, j]
                    want["sum_h"][b, k, j] += h
                    want["sum_hh"][b, k, j] += h * h
                    want["sum_rh"][b, k, j] += r * h
    assert np.array_equal(d["n"], want["n"])
    for k in RAW[1:]:
        np.testing.assert_allclose(d[k], want[k], rtol=1e-12, atol=1e-13, err_msg=k)
    # the derived values of one gene, directly: drop_one is the rise in RSS when the term leaves the fit
    j = int(np.argmax(d["n"]))
    s = mask[:, j]
    x = X[s, j]
    tss = np.sum((x - x.mean()) ** 2)
    np.testing.assert_allclose(d["tss"][j], tss, rtol=1e-10)
    U = A[0][lev[:, 0] - 1] + A[1][lev[:, 1] - 1] + Z @ A[2]
    r = x - (U @ Cm)[s, j]
    for k in range(K):
        h = U[s, k] * Cm[k, j]
        np.testing.assert_allclose(d["drop_one"][B, k, j] * tss, np.sum((r + h) ** 2) - np.sum(r * r), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(d["explained"][B, k, j], np.var(h) * s.sum() / tss, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("K,m", [(3, 1), (1, 1), (1, 0), (4, 0)])
def test_sums_over_factors_equal_the_variance_decomposition(K, m):
    X, lev, Z, mask, A, Cm = _problem(3, n=23, p=17, counts=(4, 3), m=m, K=K)
    f = posthoc.factor_decomposition_host(X, lev, Z, mask, A, Cm)
    g = posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm)
    B = 2 + (1 if m else 0)
    for k in ("n", "sum_x", "sum_xx", "rss", "tss", "r2", "rmse"):
        np.testing.assert_allclose(f[k], g[k], rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(f["sum_h"][:B].sum(axis=1), g["sum_g"], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(f["sum_rh"][:B].sum(axis=1), g["sum_rg"], rtol=1e-11, atol=1e-12)
    # the total block sums the blocks
    np.testing.assert_allclose(f["sum_h"][B], f["sum_h"][:B].sum(axis=0), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(f["sum_rh"][B], f["sum_rh"][:B].sum(axis=0), rtol=1e-11, atol=1e-12)
    if K == 1:
        np.testing.assert_allclose(f["sum_hh"][:B, 0], g["sum_gg"], rtol=1e-12)
        np.testing.assert_allclose(f["explained"][:B, 0], g["explained"], rtol=1e-9, atol=1e-12)


def test_empty_gene_gives_nan():
    X, lev, Z, mask, A, Cm = _problem(5, n=23, p=17, counts=(4, 3), m=0)
    mask[:, 4] = False
    d = posthoc.factor_decomposition_host(X, lev, None, mask, A, Cm)
    assert d["n"][4] == 0 and d["rss"][4] == 0 and np.all(d["sum_h"][:, :, 4] == 0)
    for k in ("tss", "r2", "rmse"):
        assert np.isnan(d[k][4]) and np.all(np.isfinite(np.delete(d[k], 4)))
    for k in ("explained", "drop_one"):
        assert np.all(np.isnan(d[k][:, :, 4])) and np.all(np.isfinite(np.delete(d[k], 4, axis=2)))
    # on raw sums alone, too
    raw = posthoc.fd_derived({k: d[k] for k in RAW})
    assert np.isnan(raw["r2"][4]) and np.array_equal(raw["explained"], d["explained"], equal_nan=True)


def test_factor_summary_pools_genes_orders_factors_and_counts_loadings():
    X, lev, Z, mask, A, Cm = _problem(7, n=23, p=17, counts=(4, 3), m=2, K=4)
    mask[:, 2] = False                     # an empty gene is left out
    Cm[1, ::2] = 0.0
    Cm[3] = 0.0                            # a dead factor: no share, last in the order (drop_one 0 against positive ones)
    d = posthoc.factor_decomposition_host(X, lev, Z, mask, A, Cm)
    s = posthoc.factor_summary(d, Cm)
    live = np.flatnonzero(d["n"] > 0)
    assert 2 not in live and live.size == 16
    tss = d["tss"][live].sum()
    np.testing.assert_allclose(s["tss"], tss, rtol=1e-12)
    assert s["explained"].shape == (4, 4) and s["drop_one"].shape == (4, 4)
    for b in range(4):
        for k in range(4):
            ex = sum(d["explained"][b, k, j] * d["tss"][j] for j in live) / tss
            do = sum(d["sum_hh"][b, k, j] + 2 * d["sum_rh"][b, k, j] for j in live) / tss
            np.testing.assert_allclose(s["explained"][b, k], ex, rtol=1e-10, atol=1e-14)
            np.testing.assert_allclose(s["drop_one"][b, k], do, rtol=1e-10, atol=1e-14)
    assert np.all(s["explained"][:, 3] == 0) and np.all(s["drop_one"][:, 3] == 0)
    assert sorted(s["order"]) == [0, 1, 2, 3]
    assert np.all(np.diff(s["drop_one"][-1][s["order"]]) <= 0)
    assert np.array_equal(s["order"], np.argsort(-s["drop_one"][-1], kind="stable"))
    assert np.array_equal(s["loading_nnz"], [17, 8, 17, 0])
    assert "loading_nnz" not in posthoc.factor_summary(d)


def test_cli_accepts_factor_decomposition():
    a = fit.parse(["--flat", "d", "--rank", "4", "--lambda", "2", "--alpha", "0.3", "--factor-decomposition"])
    assert a.factor_decomposition is True and a.variance_decomposition is False and a.sample_decomposition is False
    assert fit.parse(["--flat", "d", "--rank", "4", "--lambda", "2", "--alpha", "0.3"]).factor_decomposition is False
