"""Host-side checks of the per-gene variance decomposition (insider_hip_variance_decomposition): the numpy yardstick
posthoc.variance_decomposition_host() agrees with the direct formulas, and the command line accepts
--variance-decomposition."""
import functools

import numpy as np
import pytest

from insider_amd import fit, posthoc
from tests.support import blocks, problem


_problem = functools.partial(problem, n=37, p=23, counts=(4, 3), m=2, K=5)


@pytest.mark.parametrize("seed,m", [(0, 0), (1, 2), (2, 1)])
def test_host_record_matches_direct_formulas(seed, m):
    X, lev, Z, mask, A, Cm = _problem(seed, m=m)
    d = posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm)
    g = blocks(lev, Z, A, Cm)
    R = X - sum(g)
    B = len(g)
    assert d["sum_g"].shape == (B, X.shape[1]) and d["drop_one"].shape == (B, X.shape[1])
    for j in range(X.shape[1]):
        s = mask[:, j]
        x, r = X[s, j], R[s, j]
        assert d["n"][j] == s.sum()
        tss = np.sum((x - x.mean()) ** 2)
        rss = np.sum(r ** 2)
        np.testing.assert_allclose(d["rss"][j], rss, rtol=1e-12)
        np.testing.assert_allclose(d["tss"][j], tss, rtol=1e-10)
        np.testing.assert_allclose(d["r2"][j], 1 - rss / tss, rtol=1e-10)
        np.testing.assert_allclose(d["rmse"][j], np.sqrt(rss / s.sum()), rtol=1e-12)
        for b in range(B):
            gb = g[b][s, j]
            np.testing.assert_allclose(d["explained"][b, j], np.var(gb) * s.sum() / tss, rtol=1e-9)
            rss_without = np.sum((x - (sum(g)[s, j] - gb)) ** 2)      # the fit without block b
            np.testing.assert_allclose(d["drop_one"][b, j] * tss, rss_without - rss, rtol=1e-9, atol=1e-10 * rss)


def test_host_record_every_entry_and_empty_gene():
    X, lev, Z, mask, A, Cm = _problem(5, m=0)
    mask[:, 3] = False
    d = posthoc.variance_decomposition_host(X, lev, None, mask, A, Cm)
    assert d["n"][3] == 0
    for k in ("tss", "r2", "rmse"):
        assert np.isnan(d[k][3]) and np.all(np.isfinite(np.delete(d[k], 3)))
    for k in ("explained", "drop_one"):
        assert np.all(np.isnan(d[k][:, 3])) and np.all(np.isfinite(np.delete(d[k], 3, axis=1)))
    full = posthoc.variance_decomposition_host(X, lev, None, None, A, Cm)
    assert np.all(full["n"] == X.shape[0])
    np.testing.assert_allclose(full["sum_x"], X.sum(axis=0), rtol=1e-12)


def test_vd_derived_on_raw_records():
    rec = dict(n=np.array([4.0, 0.0]), sum_x=np.array([2.0, 0.0]), sum_xx=np.array([3.0, 0.0]),
               rss=np.array([0.5, 0.0]), sum_g=np.array([[1.0, 0.0]]), sum_gg=np.array([[1.5, 0.0]]),
               sum_rg=np.array([[0.25, 0.0]]))
    d = posthoc.vd_derived(rec)
    assert d["tss"][0] == 2.0 and d["r2"][0] == 0.75 and d["rmse"][0] == np.sqrt(0.125)
    assert d["explained"][0, 0] == (1.5 - 0.25) / 2.0 and d["drop_one"][0, 0] == (1.5 + 0.5) / 2.0
    assert all(np.isnan(d[k][..., 1]).all() for k in ("tss", "r2", "rmse", "explained", "drop_one"))


def test_cli_accepts_variance_decomposition():
    a = fit.parse(["--flat", "d", "--rank", "4", "--lambda", "2", "--alpha", "0.3", "--variance-decomposition"])
    assert a.variance_decomposition is True
    assert fit.parse(["--flat", "d", "--rank", "4", "--lambda", "2", "--alpha", "0.3"]).variance_decomposition is False
