"""Host-side checks of the hidden-factor analysis (insider_hip_residual_products, posthoc.residual_components): the numpy
operator posthoc.residual_products_host() agrees with a literal per-entry loop; the subspace iteration
posthoc.residual_components_host() recovers a planted rank-3 term against numpy.linalg.svd of the zero-filled residual; the
sign convention, the clamp of the block size, posthoc.component_associations() and the argument checks of the Python layer."""
import numpy as np
import pytest

from insider_amd import _lib, fit, posthoc

TOL = 1e-9


def test_products_host_equals_a_literal_loop():
    """9 x 7, two covariates and a continuous block, a mask, a centre, and a scale with one NaN and one 0: the matrix form
    against one scalar expression per entry.  Either side adds at most 9 products per sum: 1e-13 of the sum of the absolute
    terms covers any order (9 x 2^-53 is 1e-15)."""
    rng = np.random.default_rng(5)
    n, p, K, counts, m, q = 9, 7, 3, (3, 2), 2, 4
    X = rng.standard_normal((n, p)) + 0.5
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    Zc = rng.standard_normal((n, m))
    A = [0.3 * rng.standard_normal((L, K)) for L in counts] + [0.3 * rng.standard_normal((m, K))]
    Cm = rng.standard_normal((K, p))
    mask = rng.random((n, p)) < 0.7
    center = 0.2 * rng.standard_normal(p)
    scale = 0.5 + rng.random(p)
    scale[2], scale[5] = np.nan, 0.0
    Q = rng.standard_normal((n, q))
    r = np.zeros((n, p))
    for i in range(n):
        for j in range(p):
            if not mask[i, j] or not (np.isfinite(scale[j]) and scale[j] > 0):
                continue
            f = 0.0
            for b in range(len(counts)):
                f += float(A[b][lev[i, b] - 1] @ Cm[:, j])
            f += float(Zc[i] @ (A[2] @ Cm[:, j]))
            r[i, j] = (X[i, j] - f - center[j]) / scale[j]
    Z = np.array([[sum(r[i, j] * Q[i, k] for i in range(n)) for k in range(q)] for j in range(p)])
    Y = np.array([[sum(r[i, j] * Z[j, k] for j in range(p)) for k in range(q)] for i in range(n)])
    rss = np.array([sum(r[i, j] ** 2 for i in range(n)) for j in range(p)])
    got = posthoc.residual_products_host(X, lev, Zc, mask, A, Cm, Q, center, scale)
    aZ = np.abs(r).T @ np.abs(Q)
    assert got["Z"].shape == (p, q) and got["Y"].shape == (n, q) and got["rss"].shape == (p,)
    assert np.all(np.abs(got["Z"] - Z) <= 1e-13 * aZ + 1e-300)
    assert np.all(np.abs(got["Y"] - Y) <= 1e-13 * (np.abs(r) @ aZ) + 1e-300)
    assert np.all(np.abs(got["rss"] - rss) <= 1e-13 * rss)
    assert np.all(got["Z"][[2, 5]] == 0) and np.all(got["rss"][[2, 5]] == 0) and np.all(rss[[0, 1, 3, 4, 6]] > 0)
    # no centre and no scale: the plain masked residual
    plain = posthoc.residual_products_host(X, lev, Zc, mask, A, Cm, Q)
    full = posthoc.residual_products_host(X, lev, Zc, mask, A, Cm, Q, np.zeros(p), np.ones(p))
    for k in ("Z", "Y", "rss"):
        assert np.array_equal(plain[k], full[k])


def planted(seed=11):
    """n = 120, p = 300, K = 4, two covariates, an exact fit, plus a rank-3 term with singular values 60 / 40 / 25 and noise of
    sd 0.1; 70 % of the entries kept."""
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


def check_against_svd(rec, Rz, r=3, bound=10 * TOL):
    """The record of a residual_components run against numpy.linalg.svd of the zero-filled residual."""
    Ur, sr, Vtr = np.linalg.svd(Rz, full_matrices=False)
    rel = np.abs(rec["sv"] - sr[:r]) / sr[:r]
    U = rec["sample_scores"] / rec["sv"]
    du = 1.0 - np.abs(np.sum(U * Ur[:, :r], axis=0))
    dv = 1.0 - np.abs(np.sum(rec["gene_loadings"] * Vtr[:r].T, axis=0))
    print("sv relative error:", rel, "1 - |u.u_ref|:", du, "1 - |v.v_ref|:", dv)
    assert np.all(rel <= bound) and np.all(du <= bound) and np.all(dv <= bound)
    return sr


def test_components_host_recover_the_planted_term():
    X, lev, mask, A, Cm, Rz = planted()
    rec = posthoc.residual_components_host(X, lev, None, mask, A, Cm, r=3, tol=TOL)
    assert rec["sv"].shape == (3,) and rec["sample_scores"].shape == (120, 3) and rec["gene_loadings"].shape == (300, 3)
    assert rec["converged"] and rec["iters"] < 30 and rec["last_change"] < TOL
    sr = check_against_svd(rec, Rz)
    # the shares are those of the residual sum of squares, and three components do not make all of it
    assert np.allclose(rec["share"], sr[:3] ** 2 / np.sum(Rz * Rz), rtol=1e-7)
    assert 0.5 < rec["share"].sum() < 1.0 and np.all(np.diff(rec["share"]) < 0)
    # sign: the entry of largest magnitude of every score column is positive
    S = rec["sample_scores"]
    lead = np.argmax(np.abs(S), axis=0)
    assert np.all(S[lead, np.arange(3)] > 0)
    # U has orthonormal columns, and R'u = sv v ties the loadings' sign to the scores'
    U = S / rec["sv"]
    assert np.allclose(U.T @ U, np.eye(3), atol=1e-12)
    assert np.allclose(Rz.T @ U, rec["gene_loadings"] * rec["sv"], atol=1e-5)
    # the same seed gives the same record; max_iter = 1 stops unconverged after one pass
    again = posthoc.residual_components_host(X, lev, None, mask, A, Cm, r=3, tol=TOL)
    assert all(np.array_equal(rec[k], again[k]) for k in ("sv", "sample_scores", "gene_loadings", "share"))
    one = posthoc.residual_components_host(X, lev, None, mask, A, Cm, r=3, tol=TOL, max_iter=1)
    assert one["iters"] == 1 and not one["converged"] and one["last_change"] == np.inf


def test_standardize_uses_the_residual_center_and_scale():
    X, lev, mask, A, Cm, Rz = planted()
    ce, sc = posthoc.residual_center_scale(posthoc.variance_decomposition_host(X, lev, None, mask, A, Cm))
    Rs = np.where(mask, (Rz - ce) / sc, 0.0)
    rec = posthoc.residual_components_host(X, lev, None, mask, A, Cm, r=2, standardize=True, tol=TOL)
    assert rec["converged"]
    sr = np.linalg.svd(Rs, compute_uv=False)
    assert np.all(np.abs(rec["sv"] - sr[:2]) <= 10 * TOL * sr[:2])


def test_sign_tie_goes_to_the_lowest_index():
    U = np.array([[0.5, -0.5, 0.1, 0.0], [-0.5, 0.5, -0.7, 0.0], [0.2, -0.1, 0.7, -0.0]])
    assert np.array_equal(posthoc.component_signs(U), [1.0, -1.0, -1.0, 1.0])
    # a rank-1 residual u v' with v > 0 and the largest entry of u negative: the scores flip, and the loadings with them
    n, p = 6, 5
    u = np.array([0.1, -0.9, 0.3, 0.2, 0.1, 0.2])
    X = np.outer(u, np.arange(1.0, p + 1))
    lev = np.ones((n, 1), dtype=np.int32)
    rec = posthoc.residual_components_host(X, lev, None, None, [np.zeros((1, 1))], np.zeros((1, p)), r=1, oversample=0)
    assert rec["sample_scores"][1, 0] > 0 and np.all(rec["gene_loadings"][:, 0] < 0)
    assert np.allclose(np.outer(rec["sample_scores"][:, 0], rec["gene_loadings"][:, 0]), X, atol=1e-12)


def test_block_size_clamps_to_n():
    rng = np.random.default_rng(3)
    n, p = 6, 40
    X = rng.standard_normal((n, p))
    lev = np.ones((n, 1), dtype=np.int32)
    A, Cm = [np.zeros((1, 2))], np.zeros((2, p))
    seen = []

    def apply(Q):
        seen.append(Q.shape)
        return posthoc.residual_products_host(X, lev, None, None, A, Cm, Q)

    rec = posthoc.residual_components_driver(apply, n, r=5, oversample=8, tol=TOL)
    assert set(seen) == {(n, n)}                                    # q = min(r + oversample, 64, n)
    assert rec["sv"].shape == (5,) and rec["converged"] and rec["iters"] == 2      # the block spans everything: exact at once
    assert np.allclose(rec["sv"], np.linalg.svd(X, compute_uv=False)[:5], rtol=1e-12)
    wide = posthoc.residual_components_host(X, lev, None, None, A, Cm, r=9, oversample=0, tol=TOL)
    assert wide["sv"].shape == (n,) and wide["sample_scores"].shape == (n, n)      # r itself clamps to the block
    assert abs(wide["share"].sum() - 1.0) < 1e-12


def test_component_associations():
    n = 24
    lev = np.column_stack([np.arange(n) % 3 + 1, np.arange(n) // 12 + 1]).astype(np.int32)
    ind = (lev[:, 0] == 2).astype(np.float64)                      # an indicator of a level of covariate 0
    bal = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)        # sums to 0 inside every level of both covariates
    z = np.linspace(-1.0, 1.0, n)
    S = np.column_stack([ind, bal, 3.0 * z + 1.0])
    T = posthoc.component_associations(S, lev, ctns=z.reshape(-1, 1))
    assert T.shape == (3, 3)
    assert abs(T[0, 0] - 1.0) < 1e-12                               # the indicator is its covariate's
    for b in (0, 1):
        assert abs(np.sum(bal[lev[:, b] == 1])) == 0 and abs(T[b, 1]) < 1e-12
    assert abs(T[2, 2] - 1.0) < 1e-12 and T[2, 0] < 0.2            # the continuous block explains its own line
    assert np.all((T >= -1e-12) & (T <= 1 + 1e-12))
    assert posthoc.component_associations(S, lev).shape == (2, 3)
    assert np.all(np.isnan(posthoc.component_associations(np.ones((n, 1)), lev)))


def test_argument_errors_raise_without_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    X, lev, mask, A, Cm, _ = planted()
    host = lambda **kw: posthoc.residual_components_host(X, lev, None, mask, A, Cm, **kw)
    for kw in (dict(r=0), dict(r=65), dict(r=2.5), dict(r=True), dict(oversample=-1), dict(max_iter=0), dict(tol=0.0),
               dict(tol=np.nan), dict(tol=np.inf), dict(seed=-1)):
        with pytest.raises(ValueError):
            host(**kw)
        with pytest.raises(ValueError):
            posthoc.residual_components({}, **kw)                  # (checked before the object is looked at)
    with pytest.raises(ValueError):
        posthoc.residual_components({}, entries="held-out")
    Q = np.ones((120, 2))
    prod = lambda Qm, **kw: posthoc.residual_products_host(X, lev, None, mask, A, Cm, Qm, **kw)
    for bad in (np.ones((119, 2)), np.ones((120, 0)), np.ones((120, 65)), np.where(np.arange(240).reshape(120, 2) == 7, np.nan, 1.0),
                np.where(np.arange(240).reshape(120, 2) == 7, np.inf, 1.0)):
        with pytest.raises(ValueError):
            prod(bad)
    for kw in (dict(center=np.zeros(299)), dict(scale=np.ones(301))):
        with pytest.raises(ValueError):
            prod(Q, **kw)
    with pytest.raises(ValueError):
        posthoc.component_associations(np.ones((5, 2)), np.ones((4, 1), dtype=np.int32))
    with pytest.raises(ValueError):
        posthoc.component_associations(np.ones((5, 2)), np.ones((5, 1), dtype=np.int32), ctns=np.ones((4, 1)))


def test_command_line_accepts_the_option():
    a = fit.parse(["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2",
                   "--residual-components", "2", "--rc-standardize", "--rc-entries", "all"])
    assert a.residual_components == 2 and a.rc_standardize and a.rc_entries == "all"
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    assert fit.parse(base).residual_components is None and fit.parse(base).rc_entries == "train"
    for bad in (["--residual-components", "0"], ["--residual-components", "65"], ["--rc-standardize"],
                ["--residual-components", "2", "--tune"]):
        with pytest.raises(SystemExit):
            fit.parse(base + bad)
