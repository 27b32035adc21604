"""glm_interaction() on the resident data set (insider_hip_residual / insider_hip_interaction_glm) against numpy: the
residual X - sum_b u_b C and posthoc.glm_interaction() (the closed form of R/glm_interaction.R) on it."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import SPLIT_80_20, close_resident, factors, planted, resident

pytestmark = pytest.mark.gpu


def _data(n, p, counts, m=0, seed=0):
    d = planted(n, p, counts, m, seed, offset=0.0, empty=SPLIT_80_20)
    return (resident(*d),) + d[:3]


def _np_resid(X, lev, Z, A, Cm, sub):
    U = np.zeros((X.shape[0], Cm.shape[0]))
    for b in range(lev.shape[1]):
        if sub[b]:
            U += A[b][lev[:, b] - 1]
    if Z is not None and sub[lev.shape[1]]:
        U += Z @ A[lev.shape[1]]
    return X - U @ Cm


def _maxrel(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


@pytest.fixture(scope="module")
def cat():
    ds, X, lev, Z = _data(133, 203, (5, 3), seed=1)
    yield ds, X, lev, Z
    ds.close()


@pytest.mark.parametrize("K", [1, 7, 16, 30, 31, 48, 63])
def test_residual_matches_numpy(cat, K):
    ds, X, lev, Z = cat
    rng = np.random.default_rng(K)
    A, Cm = factors(rng, (5, 3), 0, K, X.shape[1])
    for sub in ([1, 1], [1, 0], [0, 1], [0, 0]):
        ref = _np_resid(X, lev, Z, A, Cm, sub)
        for rows in ((0, 133), (5, 37), (17, 18), (120, 133), (3, 131)):
            got = ds.residual(A, Cm, subtract=sub, rows=rows)
            assert got.shape == (rows[1] - rows[0], X.shape[1])
            assert _maxrel(got, ref[rows[0]:rows[1]]) < 1e-12, (K, sub, rows)
    assert ds.residual(A, Cm, rows=(7, 7)).shape == (0, X.shape[1])


def test_residual_with_continuous_covariates():
    ds, X, lev, Z = _data(150, 181, (4, 6), m=2, seed=2)
    try:
        rng = np.random.default_rng(3)
        for K in (5, 33):
            A, Cm = factors(rng, (4, 6), 2, K, X.shape[1])
            for sub in ([1, 1, 1], [1, 0, 1], [0, 0, 1], [1, 1, 0]):
                ref = _np_resid(X, lev, Z, A, Cm, sub)
                got = ds.residual(A, Cm, subtract=sub, rows=(9, 141), inc_continuous=1)
                assert _maxrel(got, ref[9:141]) < 1e-12, (K, sub)
    finally:
        ds.close()


def test_residual_streams_through_several_staging_slabs(cat):
    ds, X, lev, Z = cat
    rng = np.random.default_rng(9)
    A, Cm = factors(rng, (5, 3), 0, 12, X.shape[1])
    ref = _np_resid(X, lev, Z, A, Cm, [1, 1])
    try:
        for mb in (0.0, 0.05):        # 16 genes per slab; 48 genes per slab
            ds.set_option("resid_stage_mb", mb)
            assert _maxrel(ds.residual(A, Cm), ref) < 1e-12
            assert _maxrel(ds.residual(A, Cm, rows=(1, 132)), ref[1:132]) < 1e-12
    finally:
        ds.set_option("resid_stage_mb", 256)


def _check_glm(coeff, se, dof, ref_c, ref_p, p):
    pval = posthoc.t_pvalues(coeff, se, dof)
    np.testing.assert_allclose(coeff, ref_c, rtol=1e-9, atol=0)
    np.testing.assert_allclose(pval, ref_p, rtol=1e-7, atol=1e-300)


@pytest.fixture(scope="module")
def big():
    ds, X, lev, Z = _data(1100, 301, (7, 130), seed=4)
    yield ds, X, lev, Z
    ds.close()


@pytest.mark.parametrize("G", [2, 17, 130])
def test_interaction_glm_matches_glm_interaction(big, G):
    ds, X, lev, Z = big
    rng = np.random.default_rng(G)
    K = 7
    A, Cm = factors(rng, (7, 130), 0, K, X.shape[1])
    group = rng.permutation(np.concatenate([np.arange(1, G + 1), rng.integers(1, G + 1, size=X.shape[0] - G)]))
    group = group.astype(np.int32)
    sub = [1, 0]
    R = _np_resid(X, lev, Z, A, Cm, sub)
    ref_c, ref_p = posthoc.glm_interaction(R, None, group, Cm)
    coeff, se, dof = ds.interaction_glm(A, Cm, group, subtract=sub)
    assert coeff.shape == (G, K) and dof.shape == (G,)
    counts = np.bincount(group, minlength=G + 1)[1:]
    np.testing.assert_array_equal(dof, counts * X.shape[1] - K)
    _check_glm(coeff, se, dof, ref_c, ref_p, X.shape[1])


def test_interaction_glm_group_ids_with_gaps_and_zero(big):
    ds, X, lev, Z = big
    rng = np.random.default_rng(21)
    K = 9
    A, Cm = factors(rng, (7, 130), 0, K, X.shape[1])
    G = 10
    group = rng.choice(np.array([0, 1, 3, 4, 7, 10], dtype=np.int32), size=X.shape[0])
    R = _np_resid(X, lev, Z, A, Cm, [1, 1])
    coeff, se, dof = ds.interaction_glm(A, Cm, group, n_groups=G)
    pval = posthoc.t_pvalues(coeff, se, dof)
    for g in range(1, G + 1):
        rows = np.flatnonzero(group == g)
        if rows.size == 0:
            assert np.all(coeff[g - 1] == 0) and np.all(se[g - 1] == 0) and dof[g - 1] == 0 and np.all(pval[g - 1] == 0)
            continue
        ref_c, ref_p = posthoc.glm_interaction(R[rows], None, np.ones(rows.size, dtype=np.int32), Cm)
        np.testing.assert_allclose(coeff[g - 1], ref_c[0], rtol=1e-9, atol=0)
        np.testing.assert_allclose(pval[g - 1], ref_p[0], rtol=1e-7, atol=1e-300)


def test_interaction_glm_aliased_dimensions(big):
    ds, X, lev, Z = big
    rng = np.random.default_rng(5)
    K = 8
    A, Cm = factors(rng, (7, 130), 0, K, X.shape[1])
    group = lev[:, 0]
    for zero in ([3], [0, 6]):
        Cz = Cm.copy(order="F")
        Cz[zero] = 0.0
        keep = [k for k in range(K) if k not in zero]
        R = _np_resid(X, lev, Z, A, Cz, [0, 1])
        coeff, se, dof = ds.interaction_glm(A, Cz, group, subtract=[0, 1])
        assert np.all(np.isnan(coeff[:, zero])) and np.all(np.isnan(se[:, zero]))
        counts = np.bincount(group)[1:]
        np.testing.assert_array_equal(dof, counts * X.shape[1] - len(keep))
        ref_c, ref_p = posthoc.glm_interaction(R, None, group, Cz[keep])
        _check_glm(coeff[:, keep], se[:, keep], dof, ref_c, ref_p, X.shape[1])
    # nearly collinear rows that are not zero: singular to working precision
    Cc = Cm.copy(order="F")
    Cc[2] = 2.0 * Cc[1] + 1e-13 * rng.standard_normal(X.shape[1])
    with pytest.raises(_lib.InsiderError) as e:
        ds.interaction_glm(A, Cc, group)
    assert e.value.status == _lib.ERR_SOLVE


def test_interaction_glm_c2_after_optimize():
    w = workloads.make("c2")
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        A = [a.copy(order="F") for a in w.A0]
        Cm = w.C0.copy(order="F")
        res = ds.optimize(A, Cm, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=3)
        A = list(res["row_matrices"].values())
        Cm = res["column_factor"]
        group = np.asarray(w.levels)[:, 0]
        coeff, se, dof = ds.interaction_glm(A, Cm, group, subtract=[0, 1])
        R = _np_resid(np.asarray(w.X), np.asarray(w.levels), None, A, Cm, [0, 1])
        zero = np.flatnonzero(~Cm.any(axis=1))
        keep = np.flatnonzero(Cm.any(axis=1))
        assert np.all(np.isnan(coeff[:, zero]))
        ref_c, ref_p = posthoc.glm_interaction(R, None, group, Cm[keep])
        _check_glm(coeff[:, keep], se[:, keep], dof, ref_c, ref_p, Cm.shape[1])
        got = ds.residual(A, Cm, subtract=[0, 1], rows=(1000, 1517))
        assert _maxrel(got, R[1000:1517]) < 1e-12
    finally:
        ds.close()


def test_glm_interaction_resident_end_to_end(tmp_path):
    rng = np.random.default_rng(8)
    n, p = 240, 150
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    data = rng.standard_normal((n, p))
    obj = api.insider(data, conf, interaction_idx=[1, 2])
    obj["params"]["max_iter"] = 4
    api.fit(obj, latent_dimension=5, lambda_=1.0, alpha=0.2)
    coeff, pval = posthoc.glm_interaction_resident(obj, 1)
    A = list(obj["cfd_matrices"].values())
    Cm = obj["column_factor"]
    lev = obj["confounder"]
    R = _np_resid(obj["data"], lev, None, A, Cm, [1, 0, 1])
    keep = np.flatnonzero(Cm.any(axis=1))
    ref_c, ref_p = posthoc.glm_interaction(R, None, lev[:, 1], Cm[keep])
    assert coeff.shape == (lev[:, 1].max(), 5)
    np.testing.assert_allclose(coeff[:, keep], ref_c, rtol=1e-9, atol=0)
    np.testing.assert_allclose(pval[:, keep], ref_p, rtol=1e-7, atol=1e-300)
    close_resident(obj)
    # the command line: --interaction-glm writes the two matrices next to the factors
    from insider_amd import fit as fit_cli
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--interaction", "1", "2",
                         "--interaction-glm", "1", "--rank", "4", "--lambda", "1", "--alpha", "0.2", "--max-iter", "3",
                         "--out", str(out)]) == 0
    A = [np.load(out / f"A{i}.npy") for i in range(3)]
    Cm = np.load(out / "C.npy")
    lev = workloads.interaction_indicator(conf, (1, 2))
    R = _np_resid(data, lev, None, A, Cm, [1, 0, 1])
    keep = np.flatnonzero(Cm.any(axis=1))
    ref_c, ref_p = posthoc.glm_interaction(R, None, lev[:, 1], Cm[keep])
    np.testing.assert_allclose(np.load(out / "interaction_coeff.npy")[:, keep], ref_c, rtol=1e-9, atol=0)
    np.testing.assert_allclose(np.load(out / "interaction_pval.npy")[:, keep], ref_p, rtol=1e-7, atol=1e-300)


def test_posthoc_calls_leave_optimize_bit_identical():
    w = workloads.small(n=90, p=140, K=6)

    def run(with_glm):
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        try:
            A = [a.copy(order="F") for a in w.A0]
            Cm = w.C0.copy(order="F")
            r1 = ds.optimize(A, Cm, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=12, seed=3)
            A1 = [a.copy(order="F") for a in r1["row_matrices"].values()]
            C1 = r1["column_factor"].copy(order="F")
            outs = []
            if with_glm:
                group = np.asarray(w.levels)[:, 0]
                outs = [ds.interaction_glm(A1, C1, group, subtract=[0, 1]) for _ in range(2)]
                ds.residual(A1, C1, rows=(3, 50))
                Cbad = np.asfortranarray(np.random.default_rng(0).standard_normal(C1.shape))
                Cbad[1] = Cbad[0]
                with pytest.raises(_lib.InsiderError):
                    ds.interaction_glm(A1, Cbad, group)        # a call that fails inside the library on the way
            r2 = ds.optimize(A1, C1, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=12, seed=3)
            return r2, outs
        finally:
            ds.close()

    ref, _ = run(False)
    got, outs = run(True)
    for a, b in zip(ref["row_matrices"].values(), got["row_matrices"].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(ref["column_factor"], got["column_factor"])
    assert np.array_equal(ref["traj"], got["traj"], equal_nan=True)
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x, y, equal_nan=True)


def test_posthoc_on_a_clone(cat):
    ds, X, lev, Z = cat
    rng = np.random.default_rng(13)
    A, Cm = factors(rng, (5, 3), 0, 4, X.shape[1])
    cl = ds.clone()
    try:
        assert np.array_equal(cl.residual(A, Cm), ds.residual(A, Cm))
        a = cl.interaction_glm(A, Cm, lev[:, 1], subtract=[1, 0])
        b = ds.interaction_glm(A, Cm, lev[:, 1], subtract=[1, 0])
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    finally:
        cl.close()


def test_posthoc_argument_errors(cat):
    ds, X, lev, Z = cat
    rng = np.random.default_rng(17)
    A, Cm = factors(rng, (5, 3), 0, 4, X.shape[1])
    group = lev[:, 0]

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.interaction_glm(A, Cm[:3], group)) == _lib.ERR_ARG                 # K mismatch
    assert status(lambda: ds.interaction_glm(A, Cm, group, n_groups=4)) == _lib.ERR_ARG         # id 5 > G
    assert status(lambda: ds.interaction_glm(A, Cm, np.where(group == 2, -1, group))) == _lib.ERR_ARG
    assert status(lambda: ds.interaction_glm(A, Cm, group, subtract=[1, 1, 1])) == _lib.ERR_ARG
    assert status(lambda: ds.residual(A, Cm, rows=(0, X.shape[0] + 1))) == _lib.ERR_ARG
    # the same checks inside the library (the C ABI called directly)
    lib = _lib.load()
    K = 4
    _, Cw, Aptrs = ds._marshal(A, Cm, K, 0)
    sub = np.ones(2, dtype=np.int32)
    g32 = np.ascontiguousarray(group, dtype=np.int32)
    co, se, dof = np.zeros((5, K)), np.zeros((5, K)), np.zeros(5)
    rc = lib.insider_hip_interaction_glm(ds._h, Aptrs, _lib.ptr(Cw), 0, K, _lib.ptr(sub, C.c_int32),
                                         _lib.ptr(g32, C.c_int32), 4, _lib.ptr(co), _lib.ptr(se), _lib.ptr(dof))
    assert rc == _lib.ERR_ARG
    bad = g32.copy()
    bad[7] = -2
    rc = lib.insider_hip_interaction_glm(ds._h, Aptrs, _lib.ptr(Cw), 0, K, _lib.ptr(sub, C.c_int32),
                                         _lib.ptr(bad, C.c_int32), 5, _lib.ptr(co), _lib.ptr(se), _lib.ptr(dof))
    assert rc == _lib.ERR_ARG
    out = np.zeros((X.shape[0] + 1) * X.shape[1])
    rc = lib.insider_hip_residual(ds._h, Aptrs, _lib.ptr(Cw), 0, K, _lib.ptr(sub, C.c_int32), 0, X.shape[0] + 1,
                                  _lib.ptr(out))
    assert rc == _lib.ERR_ARG
    rc = lib.insider_hip_residual(ds._h, Aptrs, _lib.ptr(Cw), 0, 64, _lib.ptr(sub, C.c_int32), 0, 1, _lib.ptr(out))
    assert rc == _lib.ERR_UNSUPPORTED


def test_posthoc_refuses_a_sharded_handle():
    w = workloads.small(n=48, p=64, K=3)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        ds.set_shard(0, 0, 2, allreduce=lambda ptr, count, stream: None)
        with pytest.raises(_lib.InsiderError) as e:
            ds.interaction_glm(w.A0, w.C0, np.asarray(w.levels)[:, 0])
        assert e.value.status == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.InsiderError) as e:
            ds.residual(w.A0, w.C0)
        assert e.value.status == _lib.ERR_UNSUPPORTED
    finally:
        ds.close()
