"""Per-sample fit diagnostics on the resident data set (insider_hip_sample_decomposition, k_sd_stats / k_sd_reduce) against
the numpy yardstick posthoc.sample_decomposition_host().

Tolerance: every sum of a record is compared within 1e-12 x its scale, the sum of the absolute terms with |g_b| bounded by
|A_b|[level] @ |C| (absolute values before the product) and |f| by the sum of those bounds.  The bound is derived, not
measured: a term g_b is a K-term dot product and f adds at most B of them (error < (K + B) 2^-53 of the bound), a record
slot adds fewer than p terms in some order on either side (< p 2^-53 of the sum of absolute terms), products and the fma
add a few more units: fewer than (p + K + 8) 2^-53 in all, below 1e-12 for p + K < 9000, which every shape here but c2
satisfies (c2 states its own factor)."""
import ctypes as C
import functools

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import SAMPLES_3_5_7, close_resident, factors, planted, resident, same_bits

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
SUMS = ("n", "sum_x", "sum_xx", "rss", "sum_g", "sum_gg", "sum_rg")


def _data(n, p, counts, m=0, seed=0):
    """A data set with train, test and NA entries; sample 3 has no test entry, sample 5 no train entry, sample 7 is all NA."""
    d = planted(n, p, counts, m, seed, empty=SAMPLES_3_5_7)
    return (resident(*d),) + d


def _scale_terms(X, lev, Z, mask, A, Cm):
    """Per entry: |x| + F, and the bounds G_b >= |g_b|, zero outside the mask (F = sum_b G_b)."""
    aC = np.abs(Cm)
    g = [np.abs(A[b])[lev[:, b] - 1] @ aC for b in range(lev.shape[1])]
    if Z is not None:
        g.append(np.abs(Z) @ (np.abs(A[lev.shape[1]]) @ aC))
    w = np.ones(X.shape, bool) if mask is None else mask
    a = np.where(w, np.abs(X), 0.0)
    gs = [np.where(w, gb, 0.0) for gb in g]
    return a, a + sum(gs), gs


def _scales(X, lev, Z, mask, A, Cm, axis=1):
    a, big, gs = _scale_terms(X, lev, Z, mask, A, Cm)
    return dict(sum_x=a.sum(axis), sum_xx=(a * a).sum(axis), rss=(big * big).sum(axis), sum_g=np.array([x.sum(axis) for x in gs]),
                sum_gg=np.array([(x * x).sum(axis) for x in gs]), sum_rg=np.array([(big * x).sum(axis) for x in gs]))


def _check(got, X, lev, Z, mask, A, Cm, rows=None, factor=1e-12):
    if rows is not None:
        X, lev = X[rows], lev[rows]
        Z = None if Z is None else Z[rows]
        mask = None if mask is None else mask[rows]
        got = {k: v[..., rows] for k, v in got.items()}
    ref = posthoc.sample_decomposition_host(X, lev, Z, mask, A, Cm)
    sc = _scales(X, lev, Z, mask, A, Cm)
    assert np.array_equal(got["n"], ref["n"])
    for k in SUMS[1:]:
        assert got[k].shape == ref[k].shape, k
        err = np.abs(got[k] - ref[k])
        assert np.all(err <= factor * sc[k]), (k, np.max(err / np.maximum(sc[k], 1e-300)))
    return ref


_same_bits = functools.partial(same_bits, keys=SUMS)


@pytest.fixture(scope="module")
def two():
    ds, X, lev, Z, masks = _data(203, 157, (5, 3), seed=1)
    yield ds, X, lev, Z, masks
    ds.close()


@pytest.mark.parametrize("K", [1, 16, 17, 63])
def test_records_match_host(two, K):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(K), (5, 3), 0, K, X.shape[1])
    for e in ENTRIES:
        got = ds.sample_decomposition(A, Cm, entries=e)
        assert ds.info("sd_path") == 1
        assert got["n"].shape == (203,) and got["sum_g"].shape == (2, 203)
        _check(got, X, lev, Z, masks[e], A, Cm)
        empty = {"all": (), "train": (5, 7), "test": (3, 7)}[e]
        for i in empty:
            assert got["n"][i] == 0 and all(np.all(got[k][..., i] == 0) for k in SUMS)
            assert np.isnan(posthoc.vd_derived(got)["r2"][i])


@pytest.mark.parametrize("slabs", [1, 2, 3, 7, 0])
def test_slabs(two, slabs):
    """157 genes in 1, 2, 3, 7 slabs (no even split) and the automatic count: the same sums within the bound, the same
    bits for the same setting."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(40), (5, 3), 0, 9, X.shape[1])
    ds.set_option("sd_slabs", slabs)
    try:
        a = ds.sample_decomposition(A, Cm, entries="train")
        used = ds.info("sd_slabs")
        if slabs:
            assert used == slabs
        else:      # eight blocks per compute unit over one sample tile, at most 256 slabs, then slabs of equal length
            want = min(256, 2 * int(ds.info("n_simd")))
            assert used == -(-157 // -(-157 // want))
        b = ds.sample_decomposition(A, Cm, entries="train")
        assert ds.info("sd_slabs") == used
    finally:
        ds.set_option("sd_slabs", 0)
    _check(a, X, lev, Z, masks["train"], A, Cm)
    _same_bits(a, b)


@pytest.mark.parametrize("n", [65, 257, 515])
def test_partial_waves_and_tiles(n):
    """n = 65: one sample in the second wave's first lane; 257: half a tile with an odd last lane; 515: a second tile of
    three samples."""
    ds, X, lev, Z, masks = _data(n, 61, (4, 3), m=1, seed=n)
    try:
        A, Cm = factors(np.random.default_rng(n), (4, 3), 1, 7, X.shape[1])
        for slabs in (0, 3):
            ds.set_option("sd_slabs", slabs)
            for e in ENTRIES:
                got = ds.sample_decomposition(A, Cm, entries=e, inc_continuous=1)
                _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()


@pytest.mark.parametrize("counts,m", [((7,), 0), ((4, 6), 1), ((3, 5, 2), 3), ((3, 4, 2, 5), 2), ((2, 3, 4, 5, 6), 0)])
def test_blocks_and_continuous_covariates(counts, m):
    """B = 1 .. 6 blocks: windows of one, two and four blocks, and more than one pass for B > 4."""
    ds, X, lev, Z, masks = _data(131, 97, counts, m=m, seed=len(counts) + 10 * m)
    try:
        for K in (5, 33):
            A, Cm = factors(np.random.default_rng(K + m), counts, m, K, X.shape[1])
            for e in ENTRIES:
                got = ds.sample_decomposition(A, Cm, entries=e, inc_continuous=1 if m else 0)
                assert got["sum_g"].shape == (len(counts) + (1 if m else 0), X.shape[0])
                _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()


def test_more_blocks_than_registers_hold():
    """Ten categorical blocks and six continuous columns: the ids and z beyond the register-resident ones are re-read."""
    counts = (2, 3, 2, 4, 2, 3, 2, 2, 3, 2)
    ds, X, lev, Z, masks = _data(90, 41, counts, m=6, seed=77)
    try:
        A, Cm = factors(np.random.default_rng(5), counts, 6, 4, X.shape[1])
        got = ds.sample_decomposition(A, Cm, entries="train", inc_continuous=1)
        _check(got, X, lev, Z, masks["train"], A, Cm)
    finally:
        ds.close()


def test_global_table_form():
    """A covariate with 3500 levels: one load step's tables (four genes, 112 KB) do not fit the LDS budget, so the tables
    are read from global memory; forcing that form on a small data set gives the same bits as the staged one."""
    ds, X, lev, Z, masks = _data(3701, 45, (3500, 3), seed=4)
    try:
        A, Cm = factors(np.random.default_rng(9), (3500, 3), 0, 17, X.shape[1])
        for e in ENTRIES:
            got = ds.sample_decomposition(A, Cm, entries=e)
            assert ds.info("sd_path") == 2
            _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()
    ds, X, lev, Z, masks = _data(150, 77, (4, 6), m=2, seed=5)
    try:
        A, Cm = factors(np.random.default_rng(2), (4, 6), 2, 31, X.shape[1])
        staged = ds.sample_decomposition(A, Cm, entries="train", inc_continuous=1)
        assert ds.info("sd_path") == 1
        ds.set_option("vd_stage_kb", 0)
        glob = ds.sample_decomposition(A, Cm, entries="train", inc_continuous=1)
        assert ds.info("sd_path") == 2
        _same_bits(staged, glob)
        _check(glob, X, lev, Z, masks["train"], A, Cm)
    finally:
        ds.close()


def test_totals_match_the_per_gene_call(two):
    """Slot by slot, the per-sample records summed over samples equal the per-gene records summed over genes, within the
    bound applied to the grand totals: each side is off by fewer than (p + K + 8 + n) 2^-53 of the grand scale (its records'
    error plus the host sum of n or p records), 1e-13 for both sides together at this shape."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(12), (5, 3), 0, 11, X.shape[1])
    for e in ENTRIES:
        s = ds.sample_decomposition(A, Cm, entries=e)
        g = ds.variance_decomposition(A, Cm, entries=e)
        sc = _scales(X, lev, Z, masks[e], A, Cm, axis=None)
        assert s["n"].sum() == g["n"].sum()
        for k in SUMS[1:]:
            err = np.abs(s[k].sum(axis=-1) - g[k].sum(axis=-1))
            assert np.all(err <= 1e-12 * sc[k]), (e, k, err, sc[k])


def test_clone_and_remask_return_the_same_bits(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(21), (5, 3), 0, 30, X.shape[1])
    cl = ds.clone()
    rm = ds.remask(masks["train"], masks["test"])
    try:
        for e in ENTRIES:
            a = ds.sample_decomposition(A, Cm, entries=e)
            _same_bits(a, cl.sample_decomposition(A, Cm, entries=e))
            _same_bits(a, rm.sample_decomposition(A, Cm, entries=e))
    finally:
        cl.close()
        rm.close()


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
    tr, te = (obj[k].astype(bool) for k in ("train_indicator", "test_indicator"))
    derived = ("tss", "r2", "rmse", "explained", "drop_one")
    try:
        for which, e, mask in (("fit", "train", tr | te), ("fit", "all", None), ("tune", "test", te), ("tune", "train", tr)):
            d = posthoc.sample_decomposition(obj, which=which, entries=e)
            ref = _check(d, X, lev, None, mask, A, Cm)
            live = ref["tss"] > 1e-6 * ref["sum_xx"]
            assert live.sum() > 0.9 * live.size
            for k in derived:
                np.testing.assert_allclose(d[k][..., live], ref[k][..., live], rtol=1e-9, atol=1e-12)
            if (which, e) == ("fit", "train"):
                # per level of the donor-like column 0, against the host's records pooled the same way
                L = int(lev[:, 0].max())
                got = posthoc.level_decomposition(d, lev[:, 0], L)
                want = posthoc.level_decomposition(ref, lev[:, 0], L)
                assert got["r2"].shape == (L,) and got["explained"].shape == (3, L)
                assert np.array_equal(got["n"], want["n"])
                for k in derived:
                    np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
                for l in range(1, L + 1):       # and one direct value per level
                    r = (X - sum(A[b][lev[:, b] - 1] @ Cm for b in range(3)))[(lev[:, 0] == l)[:, None] & mask]
                    np.testing.assert_allclose(got["rmse"][l - 1], np.sqrt(np.mean(r * r)), rtol=1e-9)
    finally:
        close_resident(obj)


def test_c2_after_fit():
    w = workloads.make("c2")
    obj = api.insider(np.asarray(w.X), np.asarray(w.levels))
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=w.K, lambda_=w.lam, alpha=w.alpha)
    try:
        d = posthoc.sample_decomposition(obj, which="fit", entries="train")
        n, p = obj["data"].shape
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        rows = np.arange(0, n, 37)
        # p + K = 20020 is above the 9000 the module's 1e-12 covers: the same derivation gives (p + K + 8) 2^-53 per side, so
        # the factor here is (p + K + 8) 2^-52
        ref = _check(d, obj["data"], obj["confounder"], None, mask, list(obj["cfd_matrices"].values()),
                     obj["column_factor"], rows=rows, factor=(p + w.K + 8) * 2.0 ** -52)
        np.testing.assert_allclose(d["rmse"][rows], ref["rmse"], rtol=1e-9, atol=1e-12)
        assert d["r2"].shape == (n,) and d["explained"].shape == (2, n) and d["sum_rg"].shape == (2, n)
    finally:
        close_resident(obj)


def test_argument_errors(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(17), (5, 3), 0, 4, X.shape[1])

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.sample_decomposition(A, Cm, entries="held-out")) == _lib.ERR_ARG
    assert status(lambda: ds.sample_decomposition(A, Cm, inc_continuous=1)) == _lib.ERR_ARG
    assert status(lambda: ds.sample_decomposition(A, Cm, inc_continuous=2)) == _lib.ERR_ARG
    A64, C64 = factors(np.random.default_rng(1), (5, 3), 0, 64, X.shape[1])
    assert status(lambda: ds.sample_decomposition(A64, C64)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly)
    lib = _lib.load()
    _, Cw, Aptrs = ds._marshal(A, Cm, 4, 0)
    out = np.zeros((X.shape[0], 10))
    for entries in (3, -1):
        assert lib.insider_hip_sample_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 0, 4, entries, _lib.ptr(out)) == _lib.ERR_ARG
    assert lib.insider_hip_sample_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 1, 4, 1, _lib.ptr(out)) == _lib.ERR_ARG
    assert lib.insider_hip_sample_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 2, 4, 1, _lib.ptr(out)) == _lib.ERR_ARG
    _, Cw64, Aptrs64 = ds._marshal(A64, C64, 64, 0)
    assert lib.insider_hip_sample_decomposition(ds._h, Aptrs64, _lib.ptr(Cw64), 0, 64, 1,
                                                _lib.ptr(out)) == _lib.ERR_UNSUPPORTED
    assert lib.insider_hip_sample_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 0, 4, 1, None) == _lib.ERR_ARG
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
                         str(tmp_path / "Z.npy"), "--sample-decomposition", "--rank", "4", "--lambda", "1", "--alpha",
                         "0.2", "--max-iter", "3", "--out", str(out)]) == 0
    A = [np.load(out / f"A{i}.npy") for i in range(3)]
    Cm = np.load(out / "C.npy")
    ref = posthoc.sample_decomposition_host(data, conf, Zc, None, A, Cm)
    for name, key in (("sd_r2", "r2"), ("sd_rmse", "rmse"), ("sd_explained", "explained"), ("sd_drop_one", "drop_one")):
        got = np.load(out / f"{name}.npy")
        assert got.shape == ref[key].shape, name
        np.testing.assert_allclose(got, ref[key], rtol=1e-9, atol=1e-12)
    for b, L in ((0, 3), (1, 2)):
        lv = posthoc.level_decomposition(ref, conf[:, b], L)
        for name, key in ((f"sd_level{b}_r2", "r2"), (f"sd_level{b}_rmse", "rmse")):
            got = np.load(out / f"{name}.npy")
            assert got.shape == (L,), name
            np.testing.assert_allclose(got, lv[key], rtol=1e-9, atol=1e-12)
    assert not (out / "vd_r2.npy").exists()
