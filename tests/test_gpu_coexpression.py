"""insider_hip_coexpression on the device against the numpy yardstick posthoc.coexpression_host().

The tolerance is derived, not fitted.  With D the depth (n for genes, p for samples) the product and the centring cost what
tests/test_gpu_gram_topk.py derives: 4 (D + 8) 2^-52 (1 + 2 kappa_a + 2 kappa_b), kappa = sqrt(D) mean|v| / |v - mean| of the
reference's vector over its selected entries.  The vectors themselves are computed here, not given: an entry of the residual
is x - u . c - centre, times 1 / scale, a K-term dot and two subtractions, so with u = 2^-53 it errs by at most
(K + 2) u E, E_ij = (|x_ij| + sum_k |u_ik| |c_kj| + |centre_j|) / scale_j (|u| summed block by block, as the yardstick adds
the blocks; the device's multiplication by the rounded 1 / scale adds under 2 u |r| <= 2 u E, inside the factor below).  A
vector of D such entries is off by at most sqrt(D) (K + 2) u max E in norm, which relative to the norm of its centred self
is (K + 2) u rho with
    rho = sqrt(D) max_depth E / |centred vector|,
and a relative perturbation of one side moves the score by at most twice that.  Two sides, the device and the yardstick:
    tol = 4 (D + 8) 2^-52 (1 + 2 kappa_a + 2 kappa_b) + 2 (K + 2) 2^-52 (rho_a + rho_b)."""
import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import SAMPLES_3_5_7_GENES_1_3, bits, close_resident, factors, lib, masks, need_gpu, planted, resident  # noqa: F401
from tests.test_gpu_neighbors import check_rule3

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
AXES = ("genes", "samples")
OUT = ("index", "score")
COUNTS = (5, 3)


def reference(X, lev, Z, mask, A, Cm, axis, center=None, scale=None):
    """The float64 score of every pair, its tolerance (N x N each) and who may be whose partner."""
    K = Cm.shape[0]
    r, w = posthoc.coexpression_residual_host(X, lev, Z, mask, A, Cm, center, scale)
    absU = sum(np.abs(np.asarray(A[b])[lev[:, b] - 1]) for b in range(lev.shape[1]))
    if Z is not None:
        absU = absU + np.abs(Z) @ np.abs(np.asarray(A[lev.shape[1]]))
    p = X.shape[1]
    sc = np.ones(p) if scale is None else np.asarray(scale, dtype=np.float64)
    ce = np.zeros(p) if center is None else np.asarray(center, dtype=np.float64)
    usable = np.isfinite(sc) & (sc > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.where(usable[None, :] & w, (np.abs(X) + absU @ np.abs(Cm) + np.abs(ce)[None, :]) / sc[None, :], 0.0)
    if axis == "samples":
        r, w, E = r.T, w.T, E.T
    D = r.shape[0]
    W, alive = posthoc._gram_standardise(r, w, 0)
    S = W.T @ W
    m = np.maximum(w.sum(axis=0), 1)
    mean = r.sum(axis=0) / m
    cen = np.where(w, r - mean[None, :], 0.0)
    nrm = np.sqrt((cen * cen).sum(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(alive, np.sqrt(D) * (np.abs(r).sum(axis=0) / m) / nrm, 0.0)
        rho = np.where(alive, np.sqrt(D) * E.max(axis=0) / nrm, 0.0)
    T = (4.0 * (D + 8) * 2.0 ** -52 * (1.0 + 2.0 * kappa[:, None] + 2.0 * kappa[None, :])
         + 2.0 * (K + 2) * 2.0 ** -52 * (rho[:, None] + rho[None, :]))
    elig = alive[:, None] & alive[None, :] & ~np.eye(S.shape[0], dtype=bool)
    return S, T, elig, alive


def center_scale(rng, p):
    """A centre and a scale per gene; gene 0 has a NaN scale, gene 2 a zero scale: dead genes."""
    ce, sc = 0.3 * rng.standard_normal(p), 0.5 + rng.random(p)
    sc[0], sc[2] = np.nan, 0.0
    return ce, sc


_DATA = {}


def data(n, p, m):
    """The planted data set of a shape and its resident handle, made once and left unchanged."""
    if (n, p, m) not in _DATA:
        d = planted(n, p, COUNTS, m, seed=n + m, empty=SAMPLES_3_5_7_GENES_1_3)
        _DATA[(n, p, m)] = (resident(*d),) + d
    return _DATA[(n, p, m)]


@pytest.fixture(scope="module", autouse=True)
def close_data():
    yield
    for d in _DATA.values():
        d[0].close()
    _DATA.clear()


@pytest.mark.parametrize("K", [1, 7, 30, 48])
@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("shape", [(90, 130), (130, 90)])
def test_scores_match_host(lib, shape, m, K):
    n, p = shape
    ds, X, lev, Z, mk = data(n, p, m)
    rng = np.random.default_rng(1000 * K + n + m)
    A, Cm = factors(rng, COUNTS, m, K, p)
    ce, sc = center_scale(rng, p)
    for entries in ENTRIES:
        for axis in AXES:
            for cs in (False, True):
                kw = dict(center=ce, scale=sc) if cs else {}
                S, T, elig, alive = reference(X, lev, Z, mk[entries], A, Cm, axis, **kw)
                k = 10
                got = ds.coexpression(A, Cm, axis=axis, k=k, entries=entries, inc_continuous=1 if m else 0, **kw)
                assert got["index"].shape == (S.shape[0], k) and got["index"].dtype == np.int32
                check_rule3(got, S, T, k, elig)
                ref = posthoc.coexpression_host(X, lev, Z, mk[entries], A, Cm, axis, k, **kw)
                assert np.array_equal(got["index"] < 0, ref["index"] < 0)
                if axis == "genes" and cs:
                    assert not alive[0] and not alive[2]               # a bad scale gives a dead gene
                    assert np.all(got["index"][[0, 2]] == -1) and not np.isin(got["index"], (0, 2)).any()
                if axis == "genes" and entries == "train":
                    assert not alive[1] and np.all(got["index"][1] == -1)          # gene 1 has no train entry
                if axis == "samples" and entries != "all":
                    assert not alive[7] and np.all(got["index"][7] == -1)          # sample 7 is all NA
            assert ds.info("cx_stage_mb") > 0 and ds.info("cx_stage_ms") >= 0 and ds.info("cx_ms") >= 0


@pytest.mark.parametrize("axis", AXES)
def test_full_selection_agrees_with_gram_topk_of_the_residual(lib, axis):
    n, p, K, k = 90, 130, 7, 10
    ds, X, lev, Z, mk = data(n, p, 0)
    A, Cm = factors(np.random.default_rng(5), COUNTS, 0, K, p)
    S, T, elig, _ = reference(X, lev, Z, None, A, Cm, axis)
    got = ds.coexpression(A, Cm, axis=axis, k=k, entries="all")
    R = ds.residual(A, Cm)
    gram = api.gram_topk(R if axis == "genes" else R.T, k=k, metric="correlation")
    check_rule3(gram, S, T, k, elig)
    rows = np.arange(S.shape[0])[:, None]
    same = got["index"] == gram["index"]
    assert same.mean() > 0.9
    assert np.all(np.abs(got["score"] - gram["score"])[same] <= T[rows, got["index"]][same])
    big = ds.coexpression(A, Cm, axis=axis, k=64, entries="all")           # k = 64: above 64 KB of LDS
    check_rule3(big, S, T, 64, elig)
    assert bits(dict(index=big["index"][:, :k], score=big["score"][:, :k]), OUT) == bits(got, OUT)


def test_repeats_clones_and_remasks(lib):
    n, p, K, k = 130, 90, 30, 10
    ds, X, lev, Z, mk = data(n, p, 0)
    A, Cm = factors(np.random.default_rng(21), COUNTS, 0, K, p)
    tr2, te2 = masks(np.random.default_rng(77), n, p, SAMPLES_3_5_7_GENES_1_3)
    pair = [np.asfortranarray(v, dtype=np.uint8) for v in (tr2, te2)]
    cl, rm, fresh = ds.clone(), ds.remask(*pair), api.InsiderData(X, lev, *pair)
    try:
        for axis in AXES:
            for e in ENTRIES:
                a = ds.coexpression(A, Cm, axis=axis, k=k, entries=e)
                assert bits(a, OUT) == bits(ds.coexpression(A, Cm, axis=axis, k=k, entries=e), OUT)
                assert bits(a, OUT) == bits(cl.coexpression(A, Cm, axis=axis, k=k, entries=e), OUT)
                b = rm.coexpression(A, Cm, axis=axis, k=k, entries=e)
                assert bits(b, OUT) == bits(fresh.coexpression(A, Cm, axis=axis, k=k, entries=e), OUT)
                S, T, elig, _ = reference(X, lev, Z, {"all": None, "train": tr2, "test": te2}[e], A, Cm, axis)
                check_rule3(b, S, T, k, elig)
    finally:
        for h in (cl, rm, fresh):
            h.close()


def test_argument_errors_leave_the_outputs_untouched(lib):
    n, p = 90, 130
    ds, X, lev, Z, mk = data(n, p, 0)
    A, Cm = factors(np.random.default_rng(17), COUNTS, 0, 4, p)

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    bad = _lib.ERR_ARG
    assert status(lambda: ds.coexpression(A, Cm, entries="held-out")) == bad
    assert status(lambda: ds.coexpression(A, Cm, axis="columns")) == bad
    assert status(lambda: ds.coexpression(A, Cm, axis=0)) == bad
    for k in (0, 65, 2.5, True):
        assert status(lambda: ds.coexpression(A, Cm, k=k)) == bad
    assert status(lambda: ds.coexpression(A, Cm, inc_continuous=1)) == bad
    assert status(lambda: ds.coexpression(A, Cm, scale=np.ones(p - 1))) == bad
    A64, C64 = factors(np.random.default_rng(1), COUNTS, 0, 64, p)
    assert status(lambda: ds.coexpression(A64, C64)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly): sentinel-filled outputs stay as they are
    _, Cw, Aptrs = ds._marshal(A, Cm, 4, 0)
    idx, sc = np.full(p * 3 + 5, -77, dtype=np.int32), np.full(p * 3 + 5, -7.0)

    def call(K=4, inc=0, entries=1, axis=0, k=3, i=idx, s=sc, ptrs=Aptrs, cw=Cw):
        import ctypes as C
        opt = lambda a, t=C.c_double: None if a is None else _lib.ptr(a, t)
        return lib.insider_hip_coexpression(ds._h, ptrs, _lib.ptr(cw), inc, K, entries, None, None, axis, k,
                                            opt(i, C.c_int32), opt(s))

    for kw in (dict(entries=3), dict(entries=-1), dict(axis=2), dict(axis=-1), dict(k=0), dict(k=65), dict(inc=1), dict(inc=2),
               dict(i=None), dict(s=None)):
        assert call(**kw) == bad, kw
    _, Cw64, Aptrs64 = ds._marshal(A64, C64, 64, 0)
    assert call(K=64, ptrs=Aptrs64, cw=Cw64) == _lib.ERR_UNSUPPORTED
    assert np.all(idx == -77) and np.all(sc == -7.0)
    assert call() == _lib.OK                                  # and the valid call fills exactly p x 3
    assert np.all(idx[:p * 3] != -77) and np.all(idx[p * 3:] == -77) and np.all(sc[p * 3:] == -7.0)
    assert call(axis=1) == _lib.OK and np.all(idx[n * 3:p * 3 + 5][-5:] == -77)


def test_refuses_a_sharded_handle(lib):
    w = workloads.small(n=48, p=64, K=3)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        ds.set_shard(0, 0, 2, allreduce=lambda ptr, count, stream: None)
        with pytest.raises(_lib.InsiderError) as e:
            ds.coexpression(w.A0, w.C0)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        import ctypes as C
        _, Cw, Aptrs = ds._marshal(w.A0, w.C0, 3, 0)
        idx, sc = np.full(64 * 2, -77, dtype=np.int32), np.full(64 * 2, -7.0)
        assert lib.insider_hip_coexpression(ds._h, Aptrs, _lib.ptr(Cw), 0, 3, 1, None, None, 0, 2, _lib.ptr(idx, C.c_int32),
                                            _lib.ptr(sc)) == _lib.ERR_UNSUPPORTED
        assert np.all(idx == -77) and np.all(sc == -7.0)
    finally:
        ds.close()


def test_leaves_optimize_bit_identical(lib):
    w = workloads.small(n=90, p=140, K=6)

    def run(with_calls):
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        try:
            r1 = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha, tuning=1,
                             max_iter=12, seed=3)
            A = [a.copy(order="F") for a in r1["row_matrices"].values()]
            Cm = r1["column_factor"].copy(order="F")
            if with_calls:
                for e in ENTRIES:
                    for axis in AXES:
                        ds.coexpression(A, Cm, axis=axis, entries=e)
                with pytest.raises(_lib.InsiderError):
                    ds.coexpression(A, Cm, inc_continuous=1)
            return ds.optimize(A, Cm, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=12, seed=3)
        finally:
            ds.close()

    ref, got = run(False), run(True)
    for a, b in zip(ref["row_matrices"].values(), got["row_matrices"].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(ref["column_factor"], got["column_factor"])
    assert np.array_equal(ref["traj"], got["traj"], equal_nan=True)


def test_fitted_object_and_command_line(lib, tmp_path):
    """posthoc.gene_coexpression() / sample_coexpression() on the resident handle of a fitted object against the yardstick on
    its factors, and the two flags of the command line: the four cx_* records with their shapes and element types."""
    rng = np.random.default_rng(8)
    n, p, k = 40, 60, 5
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    data_ = rng.standard_normal((n, p)) + 2.0 * np.outer(rng.standard_normal(n), rng.standard_normal(p))
    obj = api.insider(data_, conf)
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=3, lambda_=1.0, alpha=0.2)
    try:
        A, Cm = list(obj["cfd_matrices"].values()), obj["column_factor"]
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        lev = np.asarray(obj["confounder"])
        g = posthoc.gene_coexpression(obj, k=k)
        S, T, elig, _ = reference(np.asarray(obj["data"]), lev, None, mask, A, Cm, "genes")
        check_rule3(g, S, T, k, elig)
        s = posthoc.sample_coexpression(obj, k=k)
        S, T, elig, _ = reference(np.asarray(obj["data"]), lev, None, mask, A, Cm, "samples", s["center"], s["scale"])
        check_rule3(s, S, T, k, elig)
        raw = posthoc.sample_coexpression(obj, k=k, standardize=False)
        assert raw["center"] is None and raw["index"].shape == (n, k)
    finally:
        close_resident(obj)
    from insider_amd import fit as fit_cli
    np.save(tmp_path / "X.npy", data_)
    np.save(tmp_path / "L.npy", conf)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--rank", "3", "--lambda", "1",
                         "--alpha", "0.2", "--max-iter", "3", "--gene-coexpression", str(k), "--sample-coexpression", str(k),
                         "--out", str(out)]) == 0
    gi, gs = np.load(out / "cx_gene_index.npy"), np.load(out / "cx_gene_score.npy")
    si, ss = np.load(out / "cx_sample_index.npy"), np.load(out / "cx_sample_score.npy")
    assert gi.shape == gs.shape == (p, k) and si.shape == ss.shape == (n, k)
    assert gi.dtype == si.dtype == np.int32 and gs.dtype == ss.dtype == np.float64
    Cm = np.load(out / "C.npy")
    A = [np.load(out / f"A{i}.npy") for i in range(2)]
    full = np.ones((n, p), dtype=bool)
    S, T, elig, _ = reference(data_, conf, None, full, A, Cm, "genes")
    check_rule3(dict(index=gi, score=gs), S, T, k, elig)
    ce, sc = posthoc.residual_center_scale(posthoc._decomposition_host(data_, conf, None, full, A, Cm, 0))
    S, T, elig, _ = reference(data_, conf, None, full, A, Cm, "samples", ce, sc)
    check_rule3(dict(index=si, score=ss), S, T, k, elig)
