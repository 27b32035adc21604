"""Host-side checks of the per-sample fit diagnostics (insider_hip_sample_decomposition): the numpy yardstick
posthoc.sample_decomposition_host() agrees with direct per-sample loops and with the per-gene yardstick's totals,
posthoc.level_decomposition() pools the samples of a level, and the command line accepts --sample-decomposition."""
import functools

import numpy as np
import pytest

from insider_amd import fit, posthoc
from tests.support import blocks, problem

SUMS = ("n", "sum_x", "sum_xx", "rss", "sum_g", "sum_gg", "sum_rg")


_problem = functools.partial(problem, n=23, p=17, counts=(4, 3), m=2, K=5)


def test_host_record_matches_per_sample_loops():
    """23 x 17 with a continuous block and a mask: every slot and every derived value of every sample."""
    X, lev, Z, mask, A, Cm = _problem(1)
    d = posthoc.sample_decomposition_host(X, lev, Z, mask, A, Cm)
    g = blocks(lev, Z, A, Cm)
    R = X - sum(g)
    B, n = len(g), X.shape[0]
    assert B == 3 and d["sum_g"].shape == (B, n) and d["drop_one"].shape == (B, n) and d["r2"].shape == (n,)
    for i in range(n):
        s = mask[i]
        x, r = X[i, s], R[i, s]
        assert d["n"][i] == s.sum()
        np.testing.assert_allclose(d["sum_x"][i], x.sum(), rtol=1e-12)
        np.testing.assert_allclose(d["sum_xx"][i], np.sum(x * x), rtol=1e-12)
        rss, tss = np.sum(r ** 2), np.sum((x - x.mean()) ** 2)
        np.testing.assert_allclose(d["rss"][i], rss, rtol=1e-12)
        np.testing.assert_allclose(d["r2"][i], 1 - rss / tss, rtol=1e-10)
        np.testing.assert_allclose(d["rmse"][i], np.sqrt(rss / s.sum()), rtol=1e-12)
        for b in range(B):
            gb = g[b][i, s]
            np.testing.assert_allclose(d["sum_g"][b, i], gb.sum(), rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(d["sum_gg"][b, i], np.sum(gb * gb), rtol=1e-12)
            np.testing.assert_allclose(d["sum_rg"][b, i], np.sum(r * gb), rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(d["explained"][b, i], np.var(gb) * s.sum() / tss, rtol=1e-9)
            rss_without = np.sum((x - (sum(g)[i, s] - gb)) ** 2)      # the fit without block b
            np.testing.assert_allclose(d["drop_one"][b, i] * tss, rss_without - rss, rtol=1e-9, atol=1e-10 * rss)


@pytest.mark.parametrize("m", [0, 2])
def test_totals_over_samples_equal_totals_over_genes(m):
    X, lev, Z, mask, A, Cm = _problem(3, m=m)
    per_sample = posthoc.sample_decomposition_host(X, lev, Z, mask, A, Cm)
    per_gene = posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm)
    for k in SUMS:
        np.testing.assert_allclose(per_sample[k].sum(axis=-1), per_gene[k].sum(axis=-1), rtol=1e-12, err_msg=k)


def test_empty_sample_gives_nan():
    X, lev, Z, mask, A, Cm = _problem(5, m=0)
    mask[4] = False
    d = posthoc.sample_decomposition_host(X, lev, None, mask, A, Cm)
    assert d["n"][4] == 0 and d["rss"][4] == 0 and np.all(d["sum_g"][:, 4] == 0)
    for k in ("tss", "r2", "rmse"):
        assert np.isnan(d[k][4]) and np.all(np.isfinite(np.delete(d[k], 4)))


def test_level_decomposition_matches_direct_and_marks_empty_levels():
    X, lev, Z, mask, A, Cm = _problem(7, n=23, counts=(4, 3))
    ids = lev[:, 0].copy()
    ids[ids == 2] = 1                      # level 2 of 5 has no sample, level 5 none either
    mask[ids == 3] = False                 # level 3 has samples, none with a selected entry
    rec = posthoc.sample_decomposition_host(X, lev, Z, mask, A, Cm)
    d = posthoc.level_decomposition(rec, ids, 5)
    g = blocks(lev, Z, A, Cm)
    R = X - sum(g)
    assert d["r2"].shape == (5,) and d["explained"].shape == (3, 5)
    for l in (1, 4):
        s = mask & (ids == l)[:, None]
        x, r = X[s], R[s]
        assert d["n"][l - 1] == s.sum() > 0
        tss = np.sum((x - x.mean()) ** 2)
        np.testing.assert_allclose(d["r2"][l - 1], 1 - np.sum(r * r) / tss, rtol=1e-10)
        np.testing.assert_allclose(d["rmse"][l - 1], np.sqrt(np.mean(r * r)), rtol=1e-12)
        for b in range(3):
            gb = g[b][s]
            np.testing.assert_allclose(d["explained"][b, l - 1], np.var(gb) * s.sum() / tss, rtol=1e-9)
            np.testing.assert_allclose(d["drop_one"][b, l - 1] * tss, np.sum((r + gb) ** 2) - np.sum(r * r), rtol=1e-9,
                                       atol=1e-10 * np.sum(r * r))
    for l in (2, 3, 5):
        assert d["n"][l - 1] == 0
        assert all(np.isnan(d[k][..., l - 1]).all() for k in ("r2", "rmse", "explained", "drop_one"))
    with pytest.raises(ValueError):
        posthoc.level_decomposition(rec, ids, 3)


def test_cli_accepts_sample_decomposition():
    a = fit.parse(["--flat", "d", "--rank", "4", "--lambda", "2", "--alpha", "0.3", "--sample-decomposition"])
    assert a.sample_decomposition is True and a.variance_decomposition is False
    assert fit.parse(["--flat", "d", "--rank", "4", "--lambda", "2", "--alpha", "0.3"]).sample_decomposition is False
