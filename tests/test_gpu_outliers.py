"""Outlier calls on the resident data set (insider_hip_outliers: k_ol_flag, k_ol_scan, k_ol_fill) against the numpy yardstick
posthoc.outliers_host().

The device and numpy round z differently in the last bits, so a threshold never sits on an entry: _gap_threshold() takes it
from the middle of a gap of the sorted reference |z| whose relative width is at least 1e-6 (asserted on the host before the
device is called).  With such a threshold membership and order must match exactly; z must match to
1e-12 (|x| + sum_b |g_b| + |center|) / scale per entry."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import GENES_3_5, close_resident, factors, planted, resident

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
CODE = {"all": 0, "train": 1, "test": 2}
COUNTS = ("gene_low", "gene_high", "sample_low", "sample_high")
LISTS = ("rows", "cols", "z")
SENT_I, SENT_Z = -7, -123.25


def _data(n, p, counts, m=0, seed=0):
    """A data set with train, test and NA entries; gene 3 has no test entry, gene 5 no train entry."""
    d = planted(n, p, counts, m, seed, empty=GENES_3_5)
    return (resident(*d),) + d


def _center_scale(X, lev, Z, mask, A, Cm):
    return posthoc.residual_center_scale(posthoc.variance_decomposition_host(X, lev, Z, mask, A, Cm))


def _zref(X, lev, Z, A, Cm, center, scale):
    """The reference z (n x p) and the bound on |device z - reference z| per entry."""
    g = [A[b][lev[:, b].astype(np.int64) - 1] @ Cm for b in range(lev.shape[1])]
    if Z is not None:
        g.append(Z @ (A[lev.shape[1]] @ Cm))
    f = np.zeros_like(X)
    for gb in g:
        f = f + gb
    ce = np.zeros(X.shape[1]) if center is None else np.asarray(center, dtype=np.float64)
    sc = np.asarray(scale, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((X - f) - ce) / sc
        bound = 1e-12 * (np.abs(X) + sum(np.abs(gb) for gb in g) + np.abs(ce)) / sc
    return z, bound


def _selected_absz(z, mask, scale):
    """|z| of the entries that can be called: selected, in a gene with a usable scale."""
    sc = np.asarray(scale, dtype=np.float64)
    w = np.ones(z.shape, dtype=bool) if mask is None else mask
    return np.abs(z[w & (np.isfinite(sc) & (sc > 0))[None, :]])


def _gap_threshold(absz, target=0.035):
    """The midpoint of a gap of the sorted |z| whose relative width is at least 1e-6, the one whose call rate (the entries
    above it over all of them) is nearest ``target``, the middle of 2 - 5 %; at least one call.  Asserts that such a gap
    exists."""
    a = np.sort(absz)
    assert a.size >= 2 and np.all(np.isfinite(a))
    wide = (a[1:] - a[:-1]) >= 1e-6 * a[1:]                      # gap k lies between a[k] and a[k + 1]
    rate = (a.size - 1 - np.arange(a.size - 1)) / a.size          # ... and leaves a.size - 1 - k calls above it
    assert wide.any(), "no gap of relative width 1e-6 among the reference |z|"
    cand = np.flatnonzero(wide)
    k = cand[np.argmin(np.abs(rate[cand] - target))]
    return 0.5 * (a[k] + a[k + 1])


def _check(got, X, lev, Z, mask, A, Cm, center, scale, t, genes=None):
    """Exact membership, order and counts, z to its bound, consistent count sums.  -> the reference."""
    ref = posthoc.outliers_host(X, lev, Z, mask, A, Cm, center, scale, t)
    _, bound = _zref(X, lev, Z, A, Cm, center, scale)
    assert got["total"] == ref["total"]
    assert np.array_equal(got["rows"], ref["rows"]) and np.array_equal(got["cols"], ref["cols"])
    assert got["rows"].dtype == np.int32 and got["cols"].dtype == np.int32
    for k in COUNTS:
        assert np.array_equal(got[k], ref[k]), k
    assert got["gene_low"].sum() + got["gene_high"].sum() == got["total"]
    assert got["sample_low"].sum() + got["sample_high"].sum() == got["total"]
    err = np.abs(got["z"] - ref["z"])
    assert np.all(err <= bound[ref["rows"], ref["cols"]]), float(np.max(err / bound[ref["rows"], ref["cols"]]))
    return ref


def _run_all_entries(ds, X, lev, Z, masks, A, Cm, inc=0, center_mask="same"):
    """Every entries choice against the host; center / scale from the host record of the same entries (``center_mask`` =
    "same"; genes without two such entries then have no usable scale) or of every entry ("all")."""
    for e in ENTRIES:
        center, scale = _center_scale(X, lev, Z, masks[e] if center_mask == "same" else None, A, Cm)
        z, _ = _zref(X, lev, Z, A, Cm, center, scale)
        t = _gap_threshold(_selected_absz(z, masks[e], scale))
        got = ds.outliers(A, Cm, scale, center=center, threshold=t, entries=e, inc_continuous=inc)
        ref = _check(got, X, lev, Z, masks[e], A, Cm, center, scale, t)
        assert ref["total"] >= 1
        if center_mask == "same" and e == "test":
            assert np.isnan(scale[3]) and got["gene_low"][3] + got["gene_high"][3] == 0
        if center_mask == "same" and e == "train":
            assert np.isnan(scale[5]) and got["gene_low"][5] + got["gene_high"][5] == 0


def _raw(ds, A, Cm, scale, center, t, entries, cap, lists, total, gene, samp, inc=0):
    """The C ABI called directly: lists = (rows, cols, z) arrays or None each; total a c_int64 or None.  -> the status."""
    K = int(Cm.shape[0])
    _, Cw, Aptrs = ds._marshal(A, Cm, K, 1 if len(A) > ds.c else 0)        # (inc itself may be the wrong one on purpose)
    ip = lambda a: None if a is None else _lib.ptr(a, C.c_int32)
    dp = lambda a: None if a is None else _lib.ptr(a)
    return _lib.load().insider_hip_outliers(ds._h, Aptrs, _lib.ptr(Cw), inc, K, entries, dp(center), dp(scale), float(t), cap,
                                            ip(lists[0]), ip(lists[1]), dp(lists[2]),
                                            None if total is None else C.byref(total), ip(gene), ip(samp))


def _sentinels(k, n, p):
    return ((np.full(k, SENT_I, np.int32), np.full(k, SENT_I, np.int32), np.full(k, SENT_Z)), C.c_int64(SENT_I),
            np.full((p, 2), SENT_I, np.int32), np.full((n, 2), SENT_I, np.int32))


@pytest.fixture(scope="module")
def two():
    ds, X, lev, Z, masks = _data(203, 157, (5, 3), seed=1)
    yield ds, X, lev, Z, masks
    ds.close()


@pytest.fixture(scope="module")
def two_ref(two):
    """One set of factors, center / scale and a gap threshold per entries choice on the shared data set, with its reference."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(30), (5, 3), 0, 30, X.shape[1])
    center, scale = _center_scale(X, lev, Z, None, A, Cm)
    z, _ = _zref(X, lev, Z, A, Cm, center, scale)
    out = dict(A=A, Cm=Cm, center=center, scale=scale, z=z)
    for e in ENTRIES:
        t = _gap_threshold(_selected_absz(z, masks[e], scale))
        out[e] = (t, posthoc.outliers_host(X, lev, Z, masks[e], A, Cm, center, scale, t))
    return out


@pytest.mark.parametrize("K", [1, 16, 17, 33, 63])
def test_calls_match_host(two, K):
    """n = 203: the sample trip is only partly filled; p = 157: the last block of the flag pass holds one gene."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(K), (5, 3), 0, K, X.shape[1])
    _run_all_entries(ds, X, lev, Z, masks, A, Cm)
    assert ds.info("ol_path") == 1


@pytest.mark.parametrize("n", [3, _lib.OL_TRIP + 5, 4099])
def test_trip_boundaries(n):
    """Fewer samples than a lane takes; the kernel's samples per trip (OL_TRIP = 1024) + 5: a trip boundary crossed by a few
    samples; several bitmap words per gene and lane step with a partial last word."""
    counts = (2,) if n == 3 else (3, 2)
    ds, X, lev, Z, masks = _data(n, 11, counts, seed=n)
    try:
        A, Cm = factors(np.random.default_rng(n + 1), counts, 0, 7, 11)
        _run_all_entries(ds, X, lev, Z, masks, A, Cm, center_mask="all")
    finally:
        ds.close()


@pytest.mark.parametrize("counts,m", [((7,), 0), ((4, 6), 1), ((3, 5, 2), 3), ((2, 3, 4, 5, 6), 0)])
def test_blocks_and_continuous_covariates(counts, m):
    ds, X, lev, Z, masks = _data(131, 97, counts, m=m, seed=len(counts) + 10 * m)
    try:
        for K in (5, 33):
            A, Cm = factors(np.random.default_rng(K + m), counts, m, K, X.shape[1])
            _run_all_entries(ds, X, lev, Z, masks, A, Cm, inc=1 if m else 0)
    finally:
        ds.close()


def test_scan_boundaries():
    """p = 2 OL_SCAN_CHUNK + 3 (the genes k_ol_scan takes per step, 1024): two full steps and a step of three genes."""
    p = 2 * _lib.OL_SCAN_CHUNK + 3
    assert p >= 2051
    ds, X, lev, Z, masks = _data(9, p, (3, 2), seed=12)
    try:
        A, Cm = factors(np.random.default_rng(13), (3, 2), 0, 4, p)
        _run_all_entries(ds, X, lev, Z, masks, A, Cm, center_mask="all")
    finally:
        ds.close()


def test_dense_and_empty(two, two_ref):
    ds, X, lev, Z, masks = two
    r = two_ref
    n, p = X.shape
    for e in ("train", "test"):
        absz = _selected_absz(r["z"], masks[e], r["scale"])
        assert absz.min() > 0
        t = 0.5 * absz.min()
        got = ds.outliers(r["A"], r["Cm"], r["scale"], center=r["center"], threshold=t, entries=e)
        _check(got, X, lev, Z, masks[e], r["A"], r["Cm"], r["center"], r["scale"], t)
        # every selected entry is a call, the list is S in order
        cols, rows = np.nonzero(masks[e].T)
        assert got["total"] == masks[e].sum() and np.array_equal(got["rows"], rows) and np.array_equal(got["cols"], cols)
        # a threshold above the largest |z|: nothing is called, nothing is written
        lists, total, gene, samp = _sentinels(16, n, p)
        assert _raw(ds, r["A"], r["Cm"], r["scale"], r["center"], 2.0 * absz.max(), CODE[e], 16, lists, total, gene,
                    samp) == _lib.OK
        assert total.value == 0 and not gene.any() and not samp.any()
        assert np.all(lists[0] == SENT_I) and np.all(lists[1] == SENT_I) and np.all(lists[2] == SENT_Z)


def test_unusable_scales(two, two_ref):
    ds, X, lev, Z, masks = two
    r = two_ref
    t, ref = r["train"]
    bad = r["scale"].copy()
    bad[[0, 8, 20, 156]] = (0.0, -1.0, np.nan, np.inf)
    got = ds.outliers(r["A"], r["Cm"], bad, center=r["center"], threshold=t, entries="train")
    _check(got, X, lev, Z, masks["train"], r["A"], r["Cm"], r["center"], bad, t)
    assert not np.isin(got["cols"], (0, 8, 20, 156)).any()
    assert ref["gene_low"][[0, 8, 20, 156]].sum() + ref["gene_high"][[0, 8, 20, 156]].sum() > 0
    keep = ~np.isin(ref["cols"], (0, 8, 20, 156))
    assert np.array_equal(got["rows"], ref["rows"][keep]) and np.array_equal(got["cols"], ref["cols"][keep])
    full = ds.outliers(r["A"], r["Cm"], r["scale"], center=r["center"], threshold=t, entries="train")
    assert np.array_equal(got["z"], full["z"][keep])


def test_cap(two, two_ref):
    ds, X, lev, Z, masks = two
    r = two_ref
    t, ref = r["test"]
    n, p = X.shape
    tot = ref["total"]
    assert tot > 8
    # the first total - 3 calls: the reference prefix, nothing beyond the capacity, complete counts
    lists, total, gene, samp = _sentinels(tot, n, p)
    assert _raw(ds, r["A"], r["Cm"], r["scale"], r["center"], t, 2, tot - 3, lists, total, gene, samp) == _lib.OK
    assert total.value == tot
    assert np.array_equal(lists[0][:tot - 3], ref["rows"][:tot - 3]) and np.array_equal(lists[1][:tot - 3], ref["cols"][:tot - 3])
    assert np.all(lists[0][tot - 3:] == SENT_I) and np.all(lists[1][tot - 3:] == SENT_I) and np.all(lists[2][tot - 3:] == SENT_Z)
    assert np.array_equal(gene[:, 0], ref["gene_low"]) and np.array_equal(gene[:, 1], ref["gene_high"])
    assert np.array_equal(samp[:, 0], ref["sample_low"]) and np.array_equal(samp[:, 1], ref["sample_high"])
    got = ds.outliers(r["A"], r["Cm"], r["scale"], center=r["center"], threshold=t, entries="test", cap=tot - 3)
    assert got["total"] == tot and np.array_equal(got["rows"], ref["rows"][:tot - 3]) and got["z"].shape == (tot - 3,)
    assert np.array_equal(got["z"], lists[2][:tot - 3])
    for k in COUNTS:
        assert np.array_equal(got[k], ref[k]), k
    # counts only: cap = 0 with null list pointers
    _, total, gene, samp = _sentinels(0, n, p)
    assert _raw(ds, r["A"], r["Cm"], r["scale"], r["center"], t, 2, 0, (None, None, None), total, gene, samp) == _lib.OK
    assert total.value == tot
    assert np.array_equal(gene[:, 0], ref["gene_low"]) and np.array_equal(gene[:, 1], ref["gene_high"])
    assert np.array_equal(samp[:, 0], ref["sample_low"]) and np.array_equal(samp[:, 1], ref["sample_high"])
    # ... and without the count arrays: the total alone
    total = C.c_int64(SENT_I)
    assert _raw(ds, r["A"], r["Cm"], r["scale"], r["center"], t, 2, 0, (None, None, None), total, None, None) == _lib.OK
    assert total.value == tot
    got = ds.outliers(r["A"], r["Cm"], r["scale"], center=r["center"], threshold=t, entries="test", cap=0)
    assert got["total"] == tot and got["rows"].size == 0 and np.array_equal(got["sample_high"], ref["sample_high"])


def test_global_table_form():
    """A covariate with 3500 levels: four genes' tables do not fit the LDS budget, so the flag pass reads them from global
    memory; forcing that form on a small data set gives the same bits as the staged one."""
    ds, X, lev, Z, masks = _data(3701, 45, (3500, 3), seed=4)
    try:
        A, Cm = factors(np.random.default_rng(9), (3500, 3), 0, 17, X.shape[1])
        center, scale = _center_scale(X, lev, Z, masks["train"], A, Cm)
        z, _ = _zref(X, lev, Z, A, Cm, center, scale)
        t = _gap_threshold(_selected_absz(z, masks["train"], scale))
        got = ds.outliers(A, Cm, scale, center=center, threshold=t, entries="train")
        assert ds.info("ol_path") == 2
        _check(got, X, lev, Z, masks["train"], A, Cm, center, scale, t)
    finally:
        ds.close()
    ds, X, lev, Z, masks = _data(150, 77, (4, 6), m=2, seed=5)
    try:
        A, Cm = factors(np.random.default_rng(2), (4, 6), 2, 31, X.shape[1])
        center, scale = _center_scale(X, lev, Z, masks["train"], A, Cm)
        z, _ = _zref(X, lev, Z, A, Cm, center, scale)
        t = _gap_threshold(_selected_absz(z, masks["train"], scale))
        assert ds.info("ol_path") == 0
        staged = ds.outliers(A, Cm, scale, center=center, threshold=t, entries="train", inc_continuous=1)
        assert ds.info("ol_path") == 1
        _check(staged, X, lev, Z, masks["train"], A, Cm, center, scale, t)
        ds.set_option("vd_stage_kb", 0)
        glob = ds.outliers(A, Cm, scale, center=center, threshold=t, entries="train", inc_continuous=1)
        assert ds.info("ol_path") == 2
        for k in LISTS + COUNTS + ("total",):
            assert np.array_equal(staged[k], glob[k]), k
    finally:
        ds.close()


def test_repeatable_bits_clone_and_remask(two, two_ref):
    ds, X, lev, Z, masks = two
    r = two_ref
    t, ref = r["test"]
    run = lambda d: d.outliers(r["A"], r["Cm"], r["scale"], center=r["center"], threshold=t, entries="test")
    a, b = run(ds), run(ds)
    cl = ds.clone()
    try:
        c = run(cl)
    finally:
        cl.close()
    rm = ds.remask(np.asfortranarray(masks["train"], dtype=np.uint8), np.asfortranarray(masks["test"], dtype=np.uint8))
    try:
        d = run(rm)
    finally:
        rm.close()
    assert a["total"] == ref["total"] > 0
    for k in LISTS + COUNTS + ("total",):
        for other in (b, c, d):
            assert np.array_equal(a[k], other[k]), k


def test_argument_errors(two):
    ds, X, lev, Z, masks = two
    n, p = X.shape
    A, Cm = factors(np.random.default_rng(17), (5, 3), 0, 4, p)
    A64, C64 = factors(np.random.default_rng(1), (5, 3), 0, 64, p)
    scale = np.ones(p)

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    for t in (0.0, -1.0, np.nan, np.inf):
        assert status(lambda: ds.outliers(A, Cm, scale, threshold=t)) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A, Cm, scale, entries="held-out")) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A, Cm, None)) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A, Cm, scale[:-1])) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A, Cm, scale, cap=-1)) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A, Cm, scale, inc_continuous=1)) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A, Cm, scale, inc_continuous=2)) == _lib.ERR_ARG
    assert status(lambda: ds.outliers(A64, C64, scale)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly); no output is touched
    lists, total, gene, samp = _sentinels(8, n, p)
    call = lambda **kw: _raw(ds, kw.get("A", A), kw.get("Cm", Cm), kw.get("scale", scale), None, kw.get("t", 2.0),
                             kw.get("entries", 1), kw.get("cap", 8), kw.get("lists", lists),
                             kw.get("total", total), gene, samp, inc=kw.get("inc", 0))
    for t in (0.0, -1.0, np.nan, np.inf, -np.inf):
        assert call(t=t) == _lib.ERR_ARG
    for entries in (3, -1):
        assert call(entries=entries) == _lib.ERR_ARG
    assert call(scale=None) == _lib.ERR_ARG
    assert call(total=None) == _lib.ERR_ARG
    assert call(cap=-1) == _lib.ERR_ARG
    for miss in range(3):
        assert call(lists=tuple(None if q == miss else lists[q] for q in range(3))) == _lib.ERR_ARG
    assert call(lists=(None, None, None)) == _lib.ERR_ARG
    assert call(inc=1) == _lib.ERR_ARG and call(inc=2) == _lib.ERR_ARG
    assert call(A=A64, Cm=C64) == _lib.ERR_UNSUPPORTED
    assert total.value == SENT_I and np.all(gene == SENT_I) and np.all(samp == SENT_I)
    assert np.all(lists[0] == SENT_I) and np.all(lists[1] == SENT_I) and np.all(lists[2] == SENT_Z)
    assert call() == _lib.OK and total.value >= 0


def test_end_to_end_finds_planted_spikes():
    rng = np.random.default_rng(8)
    n, p = 240, 151
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    data = rng.standard_normal((n, p))
    data[rng.random((n, p)) < 0.05] = np.nan
    # 12 spikes of +10 per-gene standard deviations at distinct samples and genes, on observed entries
    si, sj = rng.permutation(n)[:12], rng.permutation(p)[:12]
    data[si, sj] = np.nan_to_num(data[si, sj]) + 10.0 * np.nanstd(data[:, sj], axis=0)
    obj = api.insider(data, conf, interaction_idx=[1, 2])
    obj["params"]["max_iter"] = 4
    api.fit(obj, latent_dimension=5, lambda_=1.0, alpha=0.2)
    A = list(obj["cfd_matrices"].values())
    Cm, lev, X = obj["column_factor"], obj["confounder"], obj["data"]
    assert lev.shape[1] == 3 and X.shape == (n, p)
    mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
    assert mask[si, sj].all()
    try:
        first = posthoc.outliers(obj)                                    # derives center and scale (threshold 3)
        center, scale = first["center"], first["scale"]
        z, _ = _zref(X, lev, None, A, Cm, center, scale)
        t = _gap_threshold(_selected_absz(z, mask, scale))
        got = posthoc.outliers(obj, threshold=t)
        assert np.array_equal(got["center"], center) and np.array_equal(got["scale"], scale)
        _check(got, X, lev, None, mask, A, Cm, center, scale, t)
        called = {(int(i), int(j)): float(v) for i, j, v in zip(got["rows"], got["cols"], got["z"])}
        for i, j in zip(si, sj):
            assert called.get((int(i), int(j)), -1.0) >= t               # in the list, as a high call
        # the same with center and scale given
        again = posthoc.outliers(obj, threshold=t, center=center, scale=scale)
        for k in LISTS + COUNTS:
            assert np.array_equal(got[k], again[k]), k
    finally:
        close_resident(obj)


def test_cli_writes_the_calls(tmp_path):
    """The threshold comes from the gap helper on the factors a first run wrote (the fit is deterministic); center and scale
    are derived from sums on either side, as the derived ratios of the other post-hoc tests: 1e-9 relative on top of z's
    bound."""
    from insider_amd import fit as fit_cli
    rng = np.random.default_rng(3)
    n, p = 120, 90
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    Zc = rng.standard_normal((n, 2))
    data = rng.standard_normal((n, p))
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    np.save(tmp_path / "Z.npy", Zc)

    def run(t, name):
        out = tmp_path / name
        assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--ctns",
                             str(tmp_path / "Z.npy"), "--outliers", repr(float(t)), "--rank", "4", "--lambda", "1",
                             "--alpha", "0.2", "--max-iter", "3", "--out", str(out)]) == 0
        return out, [np.load(out / f"A{i}.npy") for i in range(3)], np.load(out / "C.npy")

    _, A, Cm = run(3.0, "first")
    center, scale = _center_scale(data, conf, Zc, None, A, Cm)
    z, bound = _zref(data, conf, Zc, A, Cm, center, scale)
    t = _gap_threshold(_selected_absz(z, None, scale))
    out, A2, C2 = run(t, "second")
    assert all(np.array_equal(a, b) for a, b in zip(A, A2)) and np.array_equal(Cm, C2)
    ref = posthoc.outliers_host(data, conf, Zc, None, A, Cm, center, scale, t)
    rows, cols, zs = (np.load(out / f"ol_{k}.npy") for k in LISTS)
    gene, samp = np.load(out / "ol_gene_counts.npy"), np.load(out / "ol_sample_counts.npy")
    assert ref["total"] > 0 and gene.shape == (p, 2) and samp.shape == (n, 2)
    assert np.array_equal(rows, ref["rows"]) and np.array_equal(cols, ref["cols"])
    assert np.array_equal(gene[:, 0], ref["gene_low"]) and np.array_equal(gene[:, 1], ref["gene_high"])
    assert np.array_equal(samp[:, 0], ref["sample_low"]) and np.array_equal(samp[:, 1], ref["sample_high"])
    assert np.all(np.abs(zs - ref["z"]) <= bound[rows, cols] + 1e-9 * np.abs(ref["z"]))


def test_c2_after_fit():
    w = workloads.make("c2")
    obj = api.insider(np.asarray(w.X), np.asarray(w.levels))
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=w.K, lambda_=w.lam, alpha=w.alpha)
    try:
        X, lev = obj["data"], obj["confounder"]
        n, p = X.shape
        A, Cm = list(obj["cfd_matrices"].values()), obj["column_factor"]
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        genes = np.arange(0, p, 37)
        ds = api._resident(obj, "fit")
        center, scale = posthoc.residual_center_scale(ds.variance_decomposition(A, Cm, entries="train"))
        Xg, Cg, mg, cg, sg = X[:, genes], Cm[:, genes], mask[:, genes], center[genes], scale[genes]
        z, bound = _zref(Xg, lev, None, A, Cg, cg, sg)
        t = _gap_threshold(_selected_absz(z, mg, sg))
        got = posthoc.outliers(obj, threshold=t, center=center, scale=scale)
        ref = posthoc.outliers_host(Xg, lev, None, mg, A, Cg, cg, sg, t)
        assert got["gene_low"].shape == (p,) and got["sample_low"].shape == (n,) and got["rows"].shape == (got["total"],)
        assert np.array_equal(got["gene_low"][genes], ref["gene_low"]) and np.array_equal(got["gene_high"][genes], ref["gene_high"])
        at = np.flatnonzero(np.isin(got["cols"], genes))
        assert ref["total"] > 0 and at.size == ref["total"]
        assert np.array_equal(got["rows"][at], ref["rows"]) and np.array_equal(got["cols"][at], genes[ref["cols"]])
        assert np.all(np.abs(got["z"][at] - ref["z"]) <= bound[ref["rows"], ref["cols"]])
        # ascending gene, then ascending sample, over the whole list; consistent sums
        key = got["cols"].astype(np.int64) * n + got["rows"]
        assert np.all(key[1:] > key[:-1])
        assert got["gene_low"].sum() + got["gene_high"].sum() == got["total"]
        assert got["sample_low"].sum() + got["sample_high"].sum() == got["total"]
        assert np.array_equal(np.bincount(got["cols"], minlength=p), got["gene_low"] + got["gene_high"])
        assert np.array_equal(np.bincount(got["rows"], minlength=n), got["sample_low"] + got["sample_high"])
    finally:
        close_resident(obj)
