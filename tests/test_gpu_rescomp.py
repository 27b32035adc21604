"""The residual products on the resident data set (insider_hip_residual_products: k_rc_back, k_rc_fwd / k_rc_reduce)
against the numpy yardstick posthoc.residual_products_host(), and the subspace iteration on top of them
(posthoc.residual_components) against the same driver on the host operator and against numpy.linalg.svd.

Tolerance of the operator (derived, not measured).  With w the 0/1 selection, a_ij = w_ij (|x_ij| + F_ij + |center_j|) / scale_j
(0 for a gene without a usable scale) and F = sum_b |A_b|[level] @ |C| (+ |Z_c| |B_c| |C|), the bounds of
tests/test_gpu_sampdecomp.py:
    |Z_gpu - Z_host|[j, k]   <= 1e-12 BZ[j, k],  BZ[j, k] = sum_i a_ij |Q_ik|,
    |Y_gpu - Y_host|[i, k]   <= 1e-12 sum_j a_ij BZ[j, k],
    |rss_gpu - rss_host|[j]  <= 1e-12 sum_i a_ij^2.
A residual is a K-term dot product of at most B embeddings, a difference, and one multiplication by the rounded reciprocal
of the scale where the host divides: fewer than (K + 8) 2^-53 of a_ij.  Z and rss add at most n such terms on either side:
fewer than (n + K + 8) 2^-53 of the bound, below 1e-12 while n + K < 9000.  Y multiplies the residual by the device's own Z
(|Z| <= BZ, its error the bound above) and adds at most p terms: fewer than (n + p + 2 K + 16) 2^-53 of its bound, below
1e-12 while n + p + 2 K < 9000.  Every shape here is far inside both.  Each check prints its largest error / bound ratio.

The driver, on the planted case of tests/test_rescomp_cpu.py with the same seed: the device and the host run are two
arithmetic orders of one iteration, so they stop at the same pass and agree far inside the iteration's own error.  Bounds:
sv to 1e-10 relative, scores (relative to the component's largest score) and loadings to 1e-7.  Observed on the MI355X:
see test_driver_matches_host_and_svd's docstring."""
import functools

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from tests.support import SAMPLES_3_5_7_GENES_1_3, close_resident, factors, masks, planted, resident, same_bits

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
TOL = 1e-9


# train, test and NA entries; sample 3 has no test entry, sample 5 no train entry, sample 7 is all NA; gene 1 has no train
# entry, gene 3 no test entry
_masks = functools.partial(masks, empty=SAMPLES_3_5_7_GENES_1_3)


def _data(n, p, counts, m=0, seed=0):
    d = planted(n, p, counts, m, seed, empty=SAMPLES_3_5_7_GENES_1_3)
    return (resident(*d),) + d


def _center_scale(rng, p):
    """A centre and a scale per gene; gene 0 has a NaN scale, gene 2 a zero scale, gene 4 (when there is one) an infinite one."""
    ce, sc = 0.3 * rng.standard_normal(p), 0.5 + rng.random(p)
    sc[0], sc[2] = np.nan, 0.0
    if p > 4:
        sc[4] = np.inf
    return ce, sc


def _bounds(X, lev, Z, mask, A, Cm, Q, center, scale):
    """BZ (p x q), the bound of Y (n x q) and of rss (p) of the module docstring, without the factor 1e-12."""
    aC = np.abs(Cm)
    c = lev.shape[1]
    F = np.zeros(X.shape)
    for b in range(c):
        F = F + np.abs(A[b])[lev[:, b] - 1] @ aC
    if Z is not None:
        F = F + np.abs(Z) @ (np.abs(A[c]) @ aC)
    p = X.shape[1]
    ce = np.zeros(p) if center is None else np.abs(center)
    sc = np.ones(p) if scale is None else scale
    ok = np.isfinite(sc) & (sc > 0)
    w = np.ones(X.shape, bool) if mask is None else mask
    a = np.where(w & ok[None, :], (np.abs(X) + F + ce) / np.where(ok, sc, 1.0), 0.0)
    BZ = a.T @ np.abs(Q)
    return BZ, a @ BZ, (a * a).sum(axis=0)


def _check(got, X, lev, Z, mask, A, Cm, Q, center=None, scale=None, want_y=True):
    ref = posthoc.residual_products_host(X, lev, Z, mask, A, Cm, Q, center, scale)
    bz, by, br = _bounds(X, lev, Z, mask, A, Cm, Q, center, scale)
    worst = 0.0
    for name, bound in (("Z", bz), ("Y", by), ("rss", br)):
        if name == "Y" and not want_y:
            assert got["Y"] is None
            continue
        assert got[name].shape == ref[name].shape, name
        assert np.all(np.isfinite(got[name])), name
        err = np.abs(got[name] - ref[name])
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        assert np.all(err <= 1e-12 * bound), (name, ratio)
    print("max error / bound:", worst)
    return ref


_same_bits = functools.partial(same_bits, keys=("Z", "Y", "rss"))


# n: below one wave tile, no multiple of 16 or 64, three sample tiles of k_rc_fwd (and 5 chunks of k_rc_back, the last of 2 samples);
# p: below one gene group, a ragged last group, three blocks of k_rc_back; q: the four tile counts, with full and ragged last
# tiles; K: the four depths of the fit (1..16, ..32, ..48, ..63), one with K no multiple of 4; every entry set, with and without
# a continuous block (m), with and without centre and scale (cs), slabs forced to 1, 2, 3 and automatic (0)
CASES = [
    # n,  p,   q,  K,  m, entries, cs,    slabs
    (15, 5, 1, 1, 0, "all", False, 0),
    (15, 37, 16, 4, 0, "train", True, 1),
    (15, 150, 17, 5, 2, "test", True, 2),
    (70, 5, 48, 30, 0, "train", True, 3),
    (70, 37, 64, 63, 0, "all", False, 2),
    (70, 150, 1, 4, 2, "test", True, 3),
    (130, 5, 17, 63, 2, "all", True, 1),
    (130, 37, 48, 5, 0, "test", False, 0),
    (130, 150, 64, 30, 2, "train", True, 0),
    (130, 150, 16, 1, 0, "train", False, 3),
    (15, 37, 64, 30, 2, "train", False, 2),
    (70, 37, 17, 1, 0, "test", True, 1),
    (130, 37, 1, 30, 0, "all", True, 2),
    (70, 150, 48, 63, 2, "train", False, 1),
    (15, 150, 16, 63, 0, "all", True, 3),
    (130, 5, 64, 4, 0, "test", True, 2),
    (70, 5, 16, 5, 2, "all", False, 1),
    (15, 5, 48, 4, 0, "train", True, 0),
    (70, 37, 32, 40, 0, "train", True, 0),
    (130, 150, 33, 40, 2, "all", True, 2),
    (15, 5, 64, 63, 2, "test", True, 3),
    (130, 150, 48, 5, 0, "test", True, 1),
]


@pytest.mark.parametrize("n,p,q,K,m,entries,cs,slabs", CASES)
def test_products_match_host(n, p, q, K, m, entries, cs, slabs):
    counts = (4, 3)
    ds, X, lev, Z, masks = _data(n, p, counts, m=m, seed=n + p + q + K)
    try:
        rng = np.random.default_rng(7 * n + p + q)
        A, Cm = factors(rng, counts, m, K, p)
        Q = rng.standard_normal((n, q))
        ce, sc = _center_scale(rng, p) if cs else (None, None)
        ds.set_option("rc_slabs", slabs)
        got = ds.residual_products(A, Cm, Q, entries=entries, center=ce, scale=sc, inc_continuous=1 if m else 0)
        used = ds.info("rc_slabs")
        if slabs:
            assert used == slabs
        else:      # eight blocks per compute unit over the sample tiles, at most 256 slabs, then slabs of equal length
            want = min(256, -(-2 * int(ds.info("n_simd")) // -(-n // 64)))
            assert used == -(-p // -(-p // want))
        assert ds.info("rc_ms") > 0
        _check(got, X, lev, Z, masks[entries], A, Cm, Q, ce, sc)
        mask = np.ones((n, p), bool) if masks[entries] is None else masks[entries]
        dead = ~mask.any(axis=0)
        if cs:
            dead |= ~(np.isfinite(sc) & (sc > 0))
        assert np.all(got["Z"][dead] == 0) and np.all(got["rss"][dead] == 0)      # a gene without an entry or a usable scale
        assert np.all(got["Y"][~mask.any(axis=1)] == 0)                          # a sample without an entry
        if entries != "all":
            assert dead[{"train": 1, "test": 3}[entries]] and not mask[7].any()
    finally:
        ds.close()


@pytest.fixture(scope="module")
def two():
    ds, X, lev, Z, masks = _data(130, 150, (5, 3), seed=1)
    yield ds, X, lev, Z, masks
    ds.close()


def test_repeated_calls_and_the_z_only_form(two):
    """Two identical calls return identical bits; with Y NULL the forward pass is skipped ("rc_slabs" 0) and Z and rss have the
    bits of the full call."""
    ds, X, lev, Z, masks = two
    rng = np.random.default_rng(2)
    A, Cm = factors(rng, (5, 3), 0, 9, 150)
    Q = rng.standard_normal((130, 20))
    ce, sc = _center_scale(rng, 150)
    for slabs in (0, 3):
        ds.set_option("rc_slabs", slabs)
        a = ds.residual_products(A, Cm, Q, entries="train", center=ce, scale=sc)
        used = ds.info("rc_slabs")
        b = ds.residual_products(A, Cm, Q, entries="train", center=ce, scale=sc)
        assert ds.info("rc_slabs") == used
        _same_bits(a, b)
        z = ds.residual_products(A, Cm, Q, entries="train", center=ce, scale=sc, want_y=False)
        assert z["Y"] is None and ds.info("rc_slabs") == 0
        assert np.array_equal(z["Z"], a["Z"]) and np.array_equal(z["rss"], a["rss"])
        _check(z, X, lev, Z, masks["train"], A, Cm, Q, ce, sc, want_y=False)
    ds.set_option("rc_slabs", 0)
    # a vector is a block of one column
    v = ds.residual_products(A, Cm, Q[:, 0], entries="all")
    _same_bits(v, ds.residual_products(A, Cm, Q[:, :1], entries="all"))


def test_clone_and_remask_use_their_own_masks(two):
    ds, X, lev, Z, masks = two
    rng = np.random.default_rng(21)
    A, Cm = factors(rng, (5, 3), 0, 30, 150)
    Q = rng.standard_normal((130, 13))
    tr2, te2 = _masks(np.random.default_rng(77), 130, 150)
    cl = ds.clone()
    rm = ds.remask(np.asfortranarray(tr2, dtype=np.uint8), np.asfortranarray(te2, dtype=np.uint8))
    try:
        for e in ENTRIES:
            a = ds.residual_products(A, Cm, Q, entries=e)
            _same_bits(a, cl.residual_products(A, Cm, Q, entries=e))
            _check(a, X, lev, Z, masks[e], A, Cm, Q)
            _check(rm.residual_products(A, Cm, Q, entries=e), X, lev, Z, {"all": None, "train": tr2, "test": te2}[e], A, Cm, Q)
    finally:
        cl.close()
        rm.close()


def test_argument_errors_leave_the_outputs_untouched(two):
    ds, X, lev, Z, masks = two
    n, p = X.shape
    A, Cm = factors(np.random.default_rng(17), (5, 3), 0, 4, p)
    Q = np.asfortranarray(np.random.default_rng(18).standard_normal((n, 3)))

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.residual_products(A, Cm, Q, entries="held-out")) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, Q, inc_continuous=1)) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, Q, inc_continuous=2)) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, Q[:-1])) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, np.ones((n, 65)))) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, np.ones((n, 0)))) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, np.full((n, 2), np.nan))) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, Q, scale=np.ones(p - 1))) == _lib.ERR_ARG
    assert status(lambda: ds.residual_products(A, Cm, Q, center=np.ones(p + 1))) == _lib.ERR_ARG
    A64, C64 = factors(np.random.default_rng(1), (5, 3), 0, 64, p)
    assert status(lambda: ds.residual_products(A64, C64, Q)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly): sentinel-filled outputs stay as they are
    lib = _lib.load()
    _, Cw, Aptrs = ds._marshal(A, Cm, 4, 0)
    Zo, Yo, ro = np.full((p, 4), -7.0, order="F"), np.full((n, 4), -7.0, order="F"), np.full(p, -7.0)
    bad = {}
    for name, v in (("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf)):
        bad[name] = Q.copy(order="F")
        bad[name][n - 1, 2] = v

    def call(K=4, inc=0, entries=1, Qm=Q, q=3, z=Zo, y=Yo, r=ro, ptrs=Aptrs, cw=Cw, h=None):
        opt = lambda a: None if a is None else _lib.ptr(a)
        return lib.insider_hip_residual_products(ds._h if h is None else h, ptrs, _lib.ptr(cw), inc, K, entries, None, None,
                                                 opt(Qm), q, opt(z), opt(y), opt(r))

    for kw in (dict(entries=3), dict(entries=-1), dict(inc=1), dict(inc=2), dict(Qm=None), dict(z=None), dict(q=0), dict(q=-1),
               dict(q=65), dict(Qm=bad["nan"]), dict(Qm=bad["inf"]), dict(Qm=bad["ninf"])):
        assert call(**kw) == _lib.ERR_ARG, kw
    _, Cw64, Aptrs64 = ds._marshal(A64, C64, 64, 0)
    assert call(K=64, ptrs=Aptrs64, cw=Cw64) == _lib.ERR_UNSUPPORTED
    assert np.all(Zo == -7.0) and np.all(Yo == -7.0) and np.all(ro == -7.0)
    assert call() == _lib.OK                                  # and the valid call fills exactly p x 3, n x 3 and p
    assert np.all(Zo[:, :3] != -7.0) and np.all(Zo[:, 3] == -7.0) and np.all(Yo[:, 3] == -7.0) and np.all(ro >= 0)
    assert call(y=None, r=None) == _lib.OK                    # Y and rss are optional


def _planted(seed=11):
    """The planted case of tests/test_rescomp_cpu.py: n = 120, p = 300, K = 4, two covariates, an exact fit, plus a rank-3 term
    with singular values 60 / 40 / 25 and noise of sd 0.1; 70 % of the entries kept."""
    rng = np.random.default_rng(seed)
    n, p, K, counts = 120, 300, 4, (4, 3)
    lev = np.column_stack([rng.permutation(np.arange(n) % L) + 1 for L in counts]).astype(np.int32)
    A = [rng.standard_normal((L, K)) for L in counts]
    Cm = rng.standard_normal((K, p))
    fitted = sum(A[b][lev[:, b] - 1] for b in range(2)) @ Cm
    U3 = np.linalg.qr(rng.standard_normal((n, 3)))[0]
    V3 = np.linalg.qr(rng.standard_normal((p, 3)))[0]
    X = fitted + (U3 * np.array([60.0, 40.0, 25.0])) @ V3.T + 0.1 * rng.standard_normal((n, p))
    mask = rng.random((n, p)) < 0.7
    return X, lev, mask, A, Cm, np.where(mask, X - fitted, 0.0)


def test_driver_matches_host_and_svd():
    """Device and host driver on the planted case, same seed: the same number of passes, sv within 1e-10 relative, scores
    (relative to the component's largest) and loadings within 1e-7; and the device record within 10 tol of numpy.linalg.svd
    of the zero-filled residual (singular values relative, 1 - |u . u_ref| and 1 - |v . v_ref|), tol = 1e-9.
    Observed on the MI355X: both stop after 7 passes (last change 8.2e-11); device against host sv 1.3e-15, scores 2.1e-15,
    loadings 2.2e-16 — rounding of two summation orders, far inside the bounds, which are kept as the distance two correct
    implementations may show on other inputs; device against the SVD: sv 5.0e-16 / 6.1e-16 / 9.7e-13,
    1 - |u . u_ref| up to 1.1e-12, 1 - |v . v_ref| up to 1.2e-13, against the bound 1e-8."""
    X, lev, mask, A, Cm, Rz = _planted()
    ds = api.InsiderData(np.asfortranarray(X), np.asfortranarray(lev), np.asfortranarray(mask, dtype=np.uint8),
                         np.asfortranarray(~mask, dtype=np.uint8))
    try:
        dev = posthoc.residual_components_resident(ds, A, Cm, r=3, entries="train", tol=TOL)
        std = posthoc.residual_components_resident(ds, A, Cm, r=2, entries="train", standardize=True, tol=TOL)
    finally:
        ds.close()
    host = posthoc.residual_components_host(X, lev, None, mask, A, Cm, r=3, tol=TOL)
    assert dev["converged"] and host["converged"] and dev["iters"] == host["iters"] < 30
    d_sv = np.max(np.abs(dev["sv"] - host["sv"]) / host["sv"])
    d_sc = np.max(np.abs(dev["sample_scores"] - host["sample_scores"]) / np.abs(host["sample_scores"]).max(axis=0))
    d_ld = np.max(np.abs(dev["gene_loadings"] - host["gene_loadings"]))
    print("iters:", dev["iters"], "device vs host: sv", d_sv, "scores", d_sc, "loadings", d_ld, "last change", dev["last_change"])
    assert d_sv <= 1e-10 and d_sc <= 1e-7 and d_ld <= 1e-7
    assert np.allclose(dev["share"], host["share"], rtol=1e-9)
    Ur, sr, Vtr = np.linalg.svd(Rz, full_matrices=False)
    rel = np.abs(dev["sv"] - sr[:3]) / sr[:3]
    du = 1.0 - np.abs(np.sum(dev["sample_scores"] / dev["sv"] * Ur[:, :3], axis=0))
    dv = 1.0 - np.abs(np.sum(dev["gene_loadings"] * Vtr[:3].T, axis=0))
    print("device vs svd: sv", rel, "1 - |u.u_ref|", du, "1 - |v.v_ref|", dv)
    assert np.all(rel <= 10 * TOL) and np.all(du <= 10 * TOL) and np.all(dv <= 10 * TOL)
    lead = np.argmax(np.abs(dev["sample_scores"]), axis=0)
    assert np.all(dev["sample_scores"][lead, np.arange(3)] > 0)
    hstd = posthoc.residual_components_host(X, lev, None, mask, A, Cm, r=2, standardize=True, tol=TOL)
    assert std["converged"] and std["iters"] == hstd["iters"]
    assert np.max(np.abs(std["sv"] - hstd["sv"]) / hstd["sv"]) <= 1e-10


def test_fitted_object_and_command_line(tmp_path):
    """posthoc.residual_components() on the resident handle of a fitted object against the host driver on its factors, and
    --residual-components of the command line: the five rc_* records with their shapes."""
    rng = np.random.default_rng(8)
    n, p = 40, 60
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    hidden = np.outer(rng.standard_normal(n), rng.standard_normal(p))          # a factor no covariate knows
    data = rng.standard_normal((n, p)) + 2.0 * hidden
    obj = api.insider(data, conf)
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=3, lambda_=1.0, alpha=0.2)
    try:
        d = posthoc.residual_components(obj, r=2, which="fit", entries="train", tol=TOL)
        A, Cm = list(obj["cfd_matrices"].values()), obj["column_factor"]
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        h = posthoc.residual_components_host(obj["data"], obj["confounder"], None, mask, A, Cm, r=2, tol=TOL)
        assert d["converged"] and d["iters"] == h["iters"]
        assert np.max(np.abs(d["sv"] - h["sv"]) / h["sv"]) <= 1e-10
        assert d["sample_scores"].shape == (n, 2) and d["gene_loadings"].shape == (p, 2)
    finally:
        close_resident(obj)
    from insider_amd import fit as fit_cli
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--residual-components", "2",
                         "--rank", "3", "--lambda", "1", "--alpha", "0.2", "--max-iter", "3", "--out", str(out)]) == 0
    shapes = dict(rc_sv=(2,), rc_share=(2,), rc_sample_scores=(n, 2), rc_gene_loadings=(p, 2), rc_assoc=(2, 2))
    rec = {k: np.load(out / f"{k}.npy") for k in shapes}
    for k, shape in shapes.items():
        assert rec[k].shape == shape and np.all(np.isfinite(rec[k])), k
    A = [np.load(out / f"A{i}.npy") for i in range(2)]
    ref = posthoc.residual_components_host(data, conf, None, None, A, np.load(out / "C.npy"), r=2)
    assert np.max(np.abs(rec["rc_sv"] - ref["sv"]) / ref["sv"]) <= 1e-9
    assert rec["rc_sv"][0] > rec["rc_sv"][1] and 0 < rec["rc_share"].sum() < 1
    assert np.all((rec["rc_assoc"] >= 0) & (rec["rc_assoc"] <= 1))
