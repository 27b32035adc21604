"""Per-gene variance decomposition on the resident data set (insider_hip_variance_decomposition, k_vd_stats) against the
numpy yardstick posthoc.variance_decomposition_host()."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import GENES_3_5, close_resident, factors, planted, resident

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
SUMS = ("n", "sum_x", "sum_xx", "rss", "sum_g", "sum_gg", "sum_rg")


def _data(n, p, counts, m=0, seed=0):
    """A data set with train, test and NA entries; gene 3 has no test entry, gene 5 no train entry."""
    d = planted(n, p, counts, m, seed, empty=GENES_3_5)
    return (resident(*d),) + d


def _scales(X, lev, Z, mask, A, Cm):
    """The absolute sums that bound the rounding error of each signed sum: sum |x|, sum (|x| + |f|)^2, sum |g_b|, sum
    (|x| + |f|) |g_b| over the selected entries."""
    g = [np.abs(A[b][lev[:, b] - 1] @ Cm) for b in range(lev.shape[1])]
    if Z is not None:
        g.append(np.abs(Z @ (A[lev.shape[1]] @ Cm)))
    w = np.ones(X.shape, bool) if mask is None else mask
    a = np.where(w, np.abs(X), 0.0)
    big = a + np.where(w, sum(g), 0.0)
    gs = [np.where(w, gb, 0.0) for gb in g]
    return dict(sum_x=a.sum(0), sum_xx=(a * a).sum(0), rss=(big * big).sum(0), sum_g=np.array([x.sum(0) for x in gs]),
                sum_gg=np.array([(x * x).sum(0) for x in gs]), sum_rg=np.array([(big * x).sum(0) for x in gs]))


def _check(got, X, lev, Z, mask, A, Cm, genes=None):
    if genes is not None:
        X, Cm = X[:, genes], Cm[:, genes]
        mask = None if mask is None else mask[:, genes]
        got = {k: v[..., genes] for k, v in got.items()}
    ref = posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm)
    sc = _scales(X, lev, Z, mask, A, Cm)
    assert np.array_equal(got["n"], ref["n"])
    for k in SUMS[1:]:
        assert got[k].shape == ref[k].shape, k
        err = np.abs(got[k] - ref[k])
        assert np.all(err <= 1e-12 * sc[k]), (k, np.max(err / np.maximum(sc[k], 1e-300)))
    return ref


@pytest.fixture(scope="module")
def two():
    ds, X, lev, Z, masks = _data(203, 157, (5, 3), seed=1)
    yield ds, X, lev, Z, masks
    ds.close()


@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 30, 31, 32, 33, 48, 49, 63])
def test_records_match_host(two, K):
    ds, X, lev, Z, masks = two
    rng = np.random.default_rng(K)
    A, Cm = factors(rng, (5, 3), 0, K, X.shape[1])
    for e in ENTRIES:
        got = ds.variance_decomposition(A, Cm, entries=e)
        assert ds.info("vd_path") == 1
        _check(got, X, lev, Z, masks[e], A, Cm)
        if e == "test":
            assert got["n"][3] == 0 and np.all(got["sum_g"][:, 3] == 0)
            assert np.isnan(posthoc.vd_derived(got)["r2"][3])
        if e == "train":
            assert got["n"][5] == 0


@pytest.mark.parametrize("counts,m", [((7,), 0), ((4, 6), 1), ((3, 5, 2), 3), ((3, 4, 2, 5), 2), ((2, 3, 4, 5, 6), 0)])
def test_blocks_and_continuous_covariates(counts, m):
    """B = 1 .. 6 blocks: windows of one, two and four blocks, and more than one pass for B > 4."""
    ds, X, lev, Z, masks = _data(131, 97, counts, m=m, seed=len(counts) + 10 * m)
    try:
        for K in (5, 33):
            A, Cm = factors(np.random.default_rng(K + m), counts, m, K, X.shape[1])
            for e in ENTRIES:
                got = ds.variance_decomposition(A, Cm, entries=e, inc_continuous=1 if m else 0)
                assert got["sum_g"].shape == (len(counts) + (1 if m else 0), X.shape[1])
                _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()


def test_global_table_form():
    """A covariate with 3500 levels: two genes' tables (56 KB) do not fit the LDS budget, so the tables are read from
    global memory; forcing that form on a small data set gives the same bits as the staged one."""
    ds, X, lev, Z, masks = _data(3701, 45, (3500, 3), seed=4)
    try:
        A, Cm = factors(np.random.default_rng(9), (3500, 3), 0, 17, X.shape[1])
        for e in ENTRIES:
            got = ds.variance_decomposition(A, Cm, entries=e)
            assert ds.info("vd_path") == 2
            _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()
    ds, X, lev, Z, masks = _data(150, 77, (4, 6), m=2, seed=5)
    try:
        A, Cm = factors(np.random.default_rng(2), (4, 6), 2, 31, X.shape[1])
        staged = ds.variance_decomposition(A, Cm, entries="train", inc_continuous=1)
        assert ds.info("vd_path") == 1
        ds.set_option("vd_stage_kb", 0)
        glob = ds.variance_decomposition(A, Cm, entries="train", inc_continuous=1)
        assert ds.info("vd_path") == 2
        for k in SUMS:
            assert np.array_equal(staged[k], glob[k]), k
    finally:
        ds.close()


def test_interaction_column_fit_and_tune_handles():
    rng = np.random.default_rng(8)
    n, p = 240, 151
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    data = rng.standard_normal((n, p))
    data[rng.random((n, p)) < 0.05] = np.nan
    obj = api.insider(data, conf, interaction_idx=[1, 2])
    obj["params"]["max_iter"] = 4
    api.fit(obj, latent_dimension=5, lambda_=1.0, alpha=0.2)
    A = list(obj["cfd_matrices"].values())
    Cm = obj["column_factor"]
    lev = obj["confounder"]
    assert lev.shape[1] == 3
    X = obj["data"]
    tr, te, na = (obj[k].astype(bool) for k in ("train_indicator", "test_indicator", "na_indicator"))
    try:
        for which, e, mask in (("fit", "train", tr | te), ("fit", "test", na), ("fit", "all", None),
                               ("tune", "test", te), ("tune", "train", tr)):
            d = posthoc.variance_decomposition(obj, which=which, entries=e)
            ref = _check(d, X, lev, None, mask, A, Cm)
            # the derived ratios where tss is not degenerate (on the NA set X holds zeros: tss = 0)
            live = ref["tss"] > 1e-6 * ref["sum_xx"]
            assert which == "fit" and e == "test" or live.sum() > 0.9 * live.size
            for k in ("tss", "r2", "rmse", "explained", "drop_one"):
                np.testing.assert_allclose(d[k][..., live], ref[k][..., live], rtol=1e-9, atol=1e-12)
    finally:
        close_resident(obj)


def test_c2_after_fit():
    w = workloads.make("c2")
    obj = api.insider(np.asarray(w.X), np.asarray(w.levels))
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=w.K, lambda_=w.lam, alpha=w.alpha)
    try:
        d = posthoc.variance_decomposition(obj, which="fit", entries="train")
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        genes = np.arange(0, obj["data"].shape[1], 37)
        ref = _check(d, obj["data"], obj["confounder"], None, mask, list(obj["cfd_matrices"].values()),
                     obj["column_factor"], genes=genes)
        np.testing.assert_allclose(d["r2"][genes], ref["r2"], rtol=1e-9, atol=1e-12)
        assert d["r2"].shape == (obj["data"].shape[1],) and d["explained"].shape == (2, obj["data"].shape[1])
    finally:
        close_resident(obj)


def test_repeatable_bits_and_clone(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(21), (5, 3), 0, 30, X.shape[1])
    a = ds.variance_decomposition(A, Cm, entries="test")
    b = ds.variance_decomposition(A, Cm, entries="test")
    cl = ds.clone()
    try:
        c = cl.variance_decomposition(A, Cm, entries="test")
    finally:
        cl.close()
    for k in SUMS:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


def test_argument_errors(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(17), (5, 3), 0, 4, X.shape[1])

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.variance_decomposition(A, Cm, entries="held-out")) == _lib.ERR_ARG
    assert status(lambda: ds.variance_decomposition(A, Cm, inc_continuous=1)) == _lib.ERR_ARG
    assert status(lambda: ds.variance_decomposition(A, Cm, inc_continuous=2)) == _lib.ERR_ARG
    A64, C64 = factors(np.random.default_rng(1), (5, 3), 0, 64, X.shape[1])
    assert status(lambda: ds.variance_decomposition(A64, C64)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly)
    lib = _lib.load()
    _, Cw, Aptrs = ds._marshal(A, Cm, 4, 0)
    out = np.zeros((X.shape[1], 10))
    for entries in (3, -1):
        assert lib.insider_hip_variance_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 0, 4, entries, _lib.ptr(out)) == _lib.ERR_ARG
    assert lib.insider_hip_variance_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 1, 4, 1, _lib.ptr(out)) == _lib.ERR_ARG
    assert lib.insider_hip_variance_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 2, 4, 1, _lib.ptr(out)) == _lib.ERR_ARG
    _, Cw64, Aptrs64 = ds._marshal(A64, C64, 64, 0)
    assert lib.insider_hip_variance_decomposition(ds._h, Aptrs64, _lib.ptr(Cw64), 0, 64, 1,
                                                  _lib.ptr(out)) == _lib.ERR_UNSUPPORTED
    assert lib.insider_hip_variance_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 0, 4, 1, None) == _lib.ERR_ARG
    assert np.all(out == 0)


def test_cli_writes_the_decomposition(tmp_path):
    from insider_amd import fit as fit_cli
    rng = np.random.default_rng(3)
    n, p = 120, 90
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    Zc = rng.standard_normal((n, 2))
    data = rng.standard_normal((n, p))
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    np.save(tmp_path / "Z.npy", Zc)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--ctns",
                         str(tmp_path / "Z.npy"), "--variance-decomposition", "--rank", "4", "--lambda", "1", "--alpha",
                         "0.2", "--max-iter", "3", "--out", str(out)]) == 0
    A = [np.load(out / f"A{i}.npy") for i in range(3)]
    Cm = np.load(out / "C.npy")
    ref = posthoc.variance_decomposition_host(data, conf, Zc, None, A, Cm)
    for name, key in (("vd_r2", "r2"), ("vd_rmse", "rmse"), ("vd_explained", "explained"), ("vd_drop_one", "drop_one")):
        got = np.load(out / f"{name}.npy")
        assert got.shape == ref[key].shape, name
        np.testing.assert_allclose(got, ref[key], rtol=1e-9, atol=1e-12)
