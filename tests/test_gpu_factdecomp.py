"""Per-factor decomposition on the resident data set (insider_hip_factor_decomposition: k_fd_build_w, k_fd_prod, k_fd_finish)
against the numpy yardstick posthoc.factor_decomposition_host().

Tolerance: every slot of a record is compared within 1e-12 x its scale, the sum of the absolute values of its terms, with
|u_b(i)[k]| bounded by |A_b|[level] (|z| |B_c| for the continuous block, the sum of those bounds for the total block),
|h_{b,k}| by that bound times |C[k][j]| and |r| by |x| + sum_b |A_b|[level] @ |C|.  For sum h and sum h^2 the scale runs over
all n samples of the gene (a complement form of those two stays admissible), for the other slots over the selected entries.
The bound is derived, not measured: an embedding of the continuous block is an m-term dot product and the total adds B of
them, the fit is a K-term dot product per block (error < (B K + m) 2^-53 of the bound on |f|), a slot adds at most n terms
in some order on either side (< n 2^-53 of the sum of absolute terms), the products with C[k][j] and the fma add a few more
units: fewer than (n + B K + m + 8) 2^-53 enter a slot, which is below 1e-12 for n + B K + m < 9000; every shape here has
n + B K + m < 9000 (the largest: n = 3001, B K = 16)."""
import functools

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import GENES_3_5_7, close_resident, factors, planted, resident, same_bits

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
BASE = ("sum_x", "sum_xx", "rss")
SUMS = ("n", "sum_x", "sum_xx", "rss", "sum_h", "sum_hh", "sum_rh")
EMPTY = {"all": (), "train": (5, 7), "test": (3, 7)}


def _data(n, p, counts, m=0, seed=0):
    """A data set with train, test and NA entries; gene 3 has no test entry, gene 5 no train entry, gene 7 is all NA (as far
    as p reaches)."""
    d = planted(n, p, counts, m, seed, empty=GENES_3_5_7)
    return (resident(*d),) + d


def _scales(X, lev, Z, mask, A, Cm):
    """The sum of the absolute values of every slot's terms (module docstring)."""
    aC = np.abs(Cm)
    G = [np.abs(A[b])[lev[:, b] - 1] for b in range(lev.shape[1])]
    if Z is not None:
        G.append(np.abs(Z) @ np.abs(A[lev.shape[1]]))
    G.append(sum(G))
    w = np.ones(X.shape, bool) if mask is None else mask
    a = np.where(w, np.abs(X), 0.0)
    big = np.where(w, np.abs(X) + G[-1] @ aC, 0.0)
    K, p = Cm.shape
    sh, shh, srh = (np.zeros((len(G), K, p)) for _ in range(3))
    for b, g in enumerate(G):
        sh[b] = g.sum(axis=0)[:, None] * aC
        shh[b] = (g * g).sum(axis=0)[:, None] * aC * aC
        srh[b] = (g.T @ big) * aC
    return dict(sum_x=a.sum(0), sum_xx=(a * a).sum(0), rss=(big * big).sum(0), sum_h=sh, sum_hh=shh, sum_rh=srh)


def _check(got, X, lev, Z, mask, A, Cm):
    ref = posthoc.factor_decomposition_host(X, lev, Z, mask, A, Cm)
    sc = _scales(X, lev, Z, mask, A, Cm)
    assert np.array_equal(got["n"], ref["n"])
    for k in SUMS[1:]:
        assert got[k].shape == ref[k].shape, k
        err = np.abs(got[k] - ref[k])
        worst = np.max(err / np.maximum(sc[k], 1e-300))
        print(f"{k}: worst error / scale {worst:.3e}")
        assert np.all(err <= 1e-12 * sc[k]), (k, worst)
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
        got = ds.factor_decomposition(A, Cm, entries=e)
        assert ds.info("fd_path") == 1       # 2 K <= 126 columns: one window
        assert got["n"].shape == (157,) and got["sum_h"].shape == (3, K, 157)
        _check(got, X, lev, Z, masks[e], A, Cm)
        d = posthoc.fd_derived(got)
        for j in EMPTY[e]:
            assert got["n"][j] == 0 and all(np.all(got[k][..., j] == 0) for k in SUMS)
            assert np.isnan(d["r2"][j]) and np.all(np.isnan(d["explained"][..., j])) and np.all(np.isnan(d["drop_one"][..., j]))


@pytest.mark.parametrize("K", [4, 31])
def test_two_continuous_columns(K):
    ds, X, lev, Z, masks = _data(203, 157, (5, 3), m=2, seed=2)
    try:
        A, Cm = factors(np.random.default_rng(K), (5, 3), 2, K, X.shape[1])
        for e in ENTRIES:
            got = ds.factor_decomposition(A, Cm, entries=e, inc_continuous=1)
            assert got["sum_h"].shape == (4, K, 157)
            _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()


@pytest.mark.parametrize("n,p,counts,K", [(203, 1, (5, 3), 6), (5, 157, (2, 3), 6), (64, 70, (5, 3), 9), (65, 70, (5, 3), 9),
                                          (97, 66, (97, 3), 5), (3001, 33, (3000, 2), 8)])
def test_edges(n, p, counts, K):
    """p = 1; n = 5; n = 64 and 65 (a chunk boundary and one sample past it); every sample its own level; a level count far
    past anything a block could stage (the kernel stages rows of the per-sample embeddings, never level tables)."""
    ds, X, lev, Z, masks = _data(n, p, counts, seed=n + p)
    try:
        A, Cm = factors(np.random.default_rng(n), counts, 0, K, p)
        for e in ENTRIES:
            got = ds.factor_decomposition(A, Cm, entries=e)
            assert ds.info("fd_path") == 1
            _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()


def test_five_blocks_at_k63_run_every_column_window():
    """B K = 315 columns: three windows of the heavy pass (128 + 128 + 59 columns), six of the light one."""
    counts = (2, 3, 4, 5, 6)
    ds, X, lev, Z, masks = _data(131, 97, counts, seed=50)
    try:
        A, Cm = factors(np.random.default_rng(63), counts, 0, 63, X.shape[1])
        for e in ENTRIES:
            got = ds.factor_decomposition(A, Cm, entries=e)
            assert ds.info("fd_path") == 2
            assert got["sum_h"].shape == (6, 63, 97)
            _check(got, X, lev, Z, masks[e], A, Cm)
    finally:
        ds.close()


def test_zero_row_of_c_gives_zero_slots(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(33), (5, 3), 0, 7, X.shape[1])
    Cm[2] = 0.0
    Cm[6] = 0.0
    for e in ENTRIES:
        got = ds.factor_decomposition(A, Cm, entries=e)
        for k in (2, 6):
            assert all(np.all(got[s][:, k, :] == 0) for s in ("sum_h", "sum_hh", "sum_rh")), (e, k)
        _check(got, X, lev, Z, masks[e], A, Cm)


def test_repeat_clone_and_remask_return_the_same_bits(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(21), (5, 3), 0, 30, X.shape[1])
    cl = ds.clone()
    rm = ds.remask(masks["train"], masks["test"])
    try:
        for e in ENTRIES:
            a = ds.factor_decomposition(A, Cm, entries=e)
            _same_bits(a, ds.factor_decomposition(A, Cm, entries=e))
            _same_bits(a, cl.factor_decomposition(A, Cm, entries=e))
            _same_bits(a, rm.factor_decomposition(A, Cm, entries=e))
    finally:
        cl.close()
        rm.close()


@pytest.mark.parametrize("K", [1, 11])
def test_sums_over_factors_match_the_variance_decomposition(two, K):
    """sum_k sum_h[b, k] = sum_g[b], sum_k sum_rh[b, k] = sum_rg[b], equal base slots and, with K = 1, sum_hh[b, 0] =
    sum_gg[b].  Bound: each side is within 1e-12 of its own scale of the exact value (module docstring; the per-gene call's
    scale is the sum over k of this one's, taken over the selected entries, so it is no larger) and the host sum over k
    adds fewer than K 2^-53 of the scale: (2e-12 + K 2^-53) x the sum over k of the scales."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(12 + K), (5, 3), 0, K, X.shape[1])
    for e in ENTRIES:
        f = ds.factor_decomposition(A, Cm, entries=e)
        g = ds.variance_decomposition(A, Cm, entries=e)
        sc = _scales(X, lev, Z, masks[e], A, Cm)
        tol = 2e-12 + K * 2.0 ** -53
        assert np.array_equal(f["n"], g["n"])
        for k in BASE:
            assert np.all(np.abs(f[k] - g[k]) <= tol * sc[k]), (e, k)
        for fk, gk in (("sum_h", "sum_g"), ("sum_rh", "sum_rg")) + ((("sum_hh", "sum_gg"),) if K == 1 else ()):
            err = np.abs(f[fk][:2].sum(axis=1) - g[gk])
            assert np.all(err <= tol * sc[fk][:2].sum(axis=1)), (e, fk, np.max(err))
        # the total block: the sum of the blocks' slots
        for fk in ("sum_h", "sum_rh"):
            err = np.abs(f[fk][2] - f[fk][:2].sum(axis=0))
            assert np.all(err <= tol * sc[fk][2]), (e, fk)


def test_after_fit_and_summary():
    w = workloads.small()
    obj = api.insider(np.asarray(w.X), np.asarray(w.levels))
    obj["params"]["max_iter"] = 4
    api.fit(obj, latent_dimension=w.K, lambda_=w.lam, alpha=w.alpha)
    try:
        A = list(obj["cfd_matrices"].values())
        Cm = obj["column_factor"]
        X, lev = obj["data"], obj["confounder"]
        n, p = X.shape
        B = lev.shape[1]
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        d = posthoc.factor_decomposition(obj, which="fit", entries="train")
        ref = _check(d, X, lev, None, mask, A, Cm)
        assert d["explained"].shape == (B + 1, w.K, p) and d["r2"].shape == (p,)
        live = ref["tss"] > 1e-6 * ref["sum_xx"]
        assert live.sum() > 0.9 * live.size
        np.testing.assert_allclose(d["rmse"][live], ref["rmse"][live], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(d["r2"][live], ref["r2"][live], rtol=1e-9, atol=1e-9)
        got, want = posthoc.factor_summary(d, Cm), posthoc.factor_summary(ref, Cm)
        assert got["explained"].shape == (B + 1, w.K) and got["order"].shape == (w.K,)
        for k in ("explained", "drop_one"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
        assert sorted(got["order"]) == list(range(w.K))
        assert np.all(np.diff(got["drop_one"][-1][got["order"]]) <= 0)
        assert np.array_equal(got["loading_nnz"], np.count_nonzero(Cm, axis=1))
    finally:
        close_resident(obj)


def test_argument_errors(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(17), (5, 3), 0, 4, X.shape[1])

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.factor_decomposition(A, Cm, entries="held-out")) == _lib.ERR_ARG
    assert status(lambda: ds.factor_decomposition(A, Cm, inc_continuous=1)) == _lib.ERR_ARG
    assert status(lambda: ds.factor_decomposition(A, Cm, inc_continuous=2)) == _lib.ERR_ARG
    A64, C64 = factors(np.random.default_rng(1), (5, 3), 0, 64, X.shape[1])
    assert status(lambda: ds.factor_decomposition(A64, C64)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly)
    lib = _lib.load()
    _, Cw, Aptrs = ds._marshal(A, Cm, 4, 0)
    out = np.zeros((X.shape[1], 4 + 3 * 3 * 4))
    for entries in (3, -1):
        assert lib.insider_hip_factor_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 0, 4, entries, _lib.ptr(out)) == _lib.ERR_ARG
    assert lib.insider_hip_factor_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 1, 4, 1, _lib.ptr(out)) == _lib.ERR_ARG
    assert lib.insider_hip_factor_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 2, 4, 1, _lib.ptr(out)) == _lib.ERR_ARG
    _, Cw64, Aptrs64 = ds._marshal(A64, C64, 64, 0)
    assert lib.insider_hip_factor_decomposition(ds._h, Aptrs64, _lib.ptr(Cw64), 0, 64, 1,
                                                _lib.ptr(out)) == _lib.ERR_UNSUPPORTED
    assert lib.insider_hip_factor_decomposition(ds._h, Aptrs, _lib.ptr(Cw), 0, 4, 1, None) == _lib.ERR_ARG
    assert np.all(out == 0)


def test_cli_writes_the_decomposition(tmp_path):
    from insider_amd import fit as fit_cli
    rng = np.random.default_rng(3)
    n, p, K = 120, 90, 4
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    Zc = rng.standard_normal((n, 2))
    data = rng.standard_normal((n, p))
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    np.save(tmp_path / "Z.npy", Zc)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--ctns",
                         str(tmp_path / "Z.npy"), "--factor-decomposition", "--rank", str(K), "--lambda", "1", "--alpha",
                         "0.2", "--max-iter", "3", "--out", str(out)]) == 0
    A = [np.load(out / f"A{i}.npy") for i in range(3)]
    Cm = np.load(out / "C.npy")
    ref = posthoc.factor_decomposition_host(data, conf, Zc, None, A, Cm)
    fs = posthoc.factor_summary(ref)
    for name, want in (("fd_summary_explained", fs["explained"]), ("fd_summary_drop_one", fs["drop_one"]),
                       ("fd_explained", ref["explained"].reshape(-1, p).T), ("fd_drop_one", ref["drop_one"].reshape(-1, p).T)):
        got = np.load(out / f"{name}.npy")
        assert got.shape == want.shape, name
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert np.load(out / "fd_summary_explained.npy").shape == (4, K)
    assert np.load(out / "fd_explained.npy").shape == (p, 4 * K)
    order = np.load(out / "fd_order.npy")
    assert order.shape == (K,) and sorted(order.astype(int)) == list(range(K))
    assert not (out / "vd_r2.npy").exists()

