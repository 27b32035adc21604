"""Host-side checks of the post-hoc interaction GLM (no GPU needed): argument validation before the library is called,
the C ABI's own checks on a null handle, and the p-value helper."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, fit, posthoc
from tests.support import lib  # noqa: F401  (fixture)


def _fake(n=20, p=12, n_levels=(3, 2), m=0):
    """An InsiderData with the shape facts of a resident data set but no handle: every check below must fire before the
    library is reached."""
    ds = object.__new__(api.InsiderData)
    ds.n, ds.p, ds.c, ds.m = n, p, len(n_levels), m
    ds.n_levels = np.asarray(n_levels, dtype=np.int32)
    ds._h = C.c_void_p()
    return ds


def _status(fn):
    with pytest.raises(_lib.InsiderError) as e:
        fn()
    return e.value.status


def test_python_side_argument_checks():
    ds = _fake()
    K = 4
    A = [np.zeros((3, K), order="F"), np.zeros((2, K), order="F")]
    Cm = np.ones((K, 12), order="F")
    group = np.tile([1, 2], 10)
    assert _status(lambda: ds.interaction_glm([a[:, :3] for a in A], Cm, group)) == _lib.ERR_ARG      # K mismatch
    assert _status(lambda: ds.interaction_glm(A, Cm, group, subtract=[1])) == _lib.ERR_ARG            # subtract length
    assert _status(lambda: ds.interaction_glm(A, Cm, group, subtract=[1, 0, 1])) == _lib.ERR_ARG
    assert _status(lambda: ds.interaction_glm(A, Cm, group, n_groups=1)) == _lib.ERR_ARG              # id 2 > G
    assert _status(lambda: ds.interaction_glm(A, Cm, np.where(group == 2, -1, group))) == _lib.ERR_ARG
    assert _status(lambda: ds.interaction_glm(A, Cm, np.zeros(20, dtype=int))) == _lib.ERR_ARG         # no group at all
    assert _status(lambda: ds.interaction_glm(A, Cm, group[:-1])) == _lib.ERR_ARG
    assert _status(lambda: ds.interaction_glm(A, Cm, group + 0.5)) == _lib.ERR_ARG
    assert _status(lambda: ds.residual(A, Cm, rows=(0, 21))) == _lib.ERR_ARG                          # row_end > n
    assert _status(lambda: ds.residual(A, Cm, rows=(5, 4))) == _lib.ERR_ARG
    assert _status(lambda: ds.residual(A, Cm, rows=slice(0, 10, 2))) == _lib.ERR_ARG
    assert _status(lambda: ds.residual(A, Cm, inc_continuous=2)) == _lib.ERR_ARG


def test_c_abi_rejects_a_null_handle(lib):
    K = 3
    a = np.zeros((2, K))
    Aptrs = (C.POINTER(C.c_double) * 1)(_lib.ptr(a))
    Cm = np.zeros((K, 4))
    sub = np.ones(1, dtype=np.int32)
    grp = np.ones(2, dtype=np.int32)
    out = np.zeros(64)
    assert lib.insider_hip_residual(None, Aptrs, _lib.ptr(Cm), 0, K, _lib.ptr(sub, C.c_int32), 0, 1, _lib.ptr(out)) == \
        _lib.ERR_ARG
    assert b"null handle" in lib.insider_hip_last_error()
    assert lib.insider_hip_interaction_glm(None, Aptrs, _lib.ptr(Cm), 0, K, _lib.ptr(sub, C.c_int32),
                                           _lib.ptr(grp, C.c_int32), 1, _lib.ptr(out), _lib.ptr(out),
                                           _lib.ptr(out)) == _lib.ERR_ARG


def test_t_pvalues():
    from scipy import stats
    coeff = np.array([[1.0, -2.0, np.nan], [0.0, 0.0, 0.0]])
    se = np.array([[0.5, 1.0, np.nan], [0.0, 0.0, 0.0]])
    dof = np.array([30.0, 0.0])
    pv = posthoc.t_pvalues(coeff, se, dof)
    np.testing.assert_allclose(pv[0, :2], 2 * stats.t.sf([2.0, 2.0], 30.0), rtol=1e-15)
    assert np.isnan(pv[0, 2])
    assert np.all(pv[1] == 0)                                # empty group: the reference's matrix(0, ...) rows


def test_glm_interaction_resident_checks_the_covariate():
    obj = api.Insider(inc_continuous=0, _resident_fit=_fake())
    with pytest.raises(ValueError, match="group_cov"):
        posthoc.glm_interaction_resident(obj, 2)


def test_cli_accepts_interaction_glm():
    a = fit.parse(["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.1",
                   "--interaction-glm", "1"])
    assert a.interaction_glm == 1
    assert fit.parse(["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.1"]).interaction_glm \
        is None


def test_longdouble_reference_agrees_with_glm_interaction():
    """tests/glm_reference.py (the yardstick of tests/test_gpu_glm_forms.py) against the host closed form at K = 7, p = 301:
    coefficients to 1e-12 of each level's largest, p-values through t_pvalues() to 1e-9."""
    from tests import glm_reference as gr
    rng = np.random.default_rng(11)
    n, p, K, G = 90, 301, 7, 6
    R = rng.standard_normal((n, p))
    Cm = rng.standard_normal((K, p))
    group = rng.permutation(np.concatenate([np.arange(1, G + 1), rng.integers(1, G + 1, size=n - G)]))
    ref_c, ref_p = posthoc.glm_interaction(R, None, group, Cm)
    got = gr.glm_reference(R, group, G, Cm)
    assert got["coeff"].dtype == np.longdouble
    assert gr.EXTENDED == (np.finfo(np.longdouble).eps < np.finfo(np.float64).eps)
    coeff = got["coeff"].astype(np.float64)
    assert np.all(np.abs(coeff - ref_c) <= 1e-12 * np.abs(ref_c).max(axis=1, keepdims=True))
    counts = np.bincount(group, minlength=G + 1)[1:]
    np.testing.assert_array_equal(got["m"], counts)
    np.testing.assert_array_equal(got["dof"].astype(np.float64), counts * p - K)
    pv = posthoc.t_pvalues(coeff, got["se"].astype(np.float64), got["dof"].astype(np.float64))
    np.testing.assert_allclose(pv, ref_p, rtol=1e-9, atol=0)
    # the direct RSS and the expanded form the device uses agree; ss and cond are what they say
    np.testing.assert_allclose(got["ss"].astype(np.float64), [np.sum(R[group == g] ** 2) for g in range(1, G + 1)], rtol=1e-13)
    assert abs(got["cond"] - np.linalg.cond(Cm @ Cm.T)) <= 1e-9 * got["cond"]
    np.testing.assert_allclose(got["dinv"].astype(np.float64), np.diag(np.linalg.inv(Cm @ Cm.T)), rtol=1e-12)
    # a zero row of C is dropped: NaN columns, rank K - 1, an empty group gives zero rows
    Cz = Cm.copy()
    Cz[2] = 0.0
    gz = np.where(group == 3, 0, group)
    got = gr.glm_reference(R, gz, G, Cz)
    keep = [0, 1, 3, 4, 5, 6]
    assert list(got["keep"]) == keep
    assert np.all(np.isnan(got["coeff"][[0, 1, 3, 4, 5], 2])) and np.isnan(got["dinv"][2])
    assert np.all(got["coeff"][2] == 0) and np.all(got["se"][2] == 0) and got["dof"][2] == 0 and got["m"][2] == 0
    live = [0, 1, 3, 4, 5]
    ref_c, _ = posthoc.glm_interaction(R[gz > 0], None, np.searchsorted(np.unique(gz[gz > 0]), gz[gz > 0]) + 1, Cz[keep])
    c = got["coeff"].astype(np.float64)[np.ix_(live, keep)]
    assert np.all(np.abs(c - ref_c) <= 1e-12 * np.abs(ref_c).max(axis=1, keepdims=True))


def test_glm_option_and_info_keys_are_declared():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "insider_hip.h")).read()
    src = open(os.path.join(root, "insider_amd", "csrc", "insider_hip.hip")).read()
    for key in ("glm_slabs", "glm_form"):
        assert f'"{key}"' in hdr and f's == "{key}"' in src, key
    assert src.count('s == "glm_slabs"') == 2                 # an option and an info key
    for key in ("ls_form", "fd_form", "rc_form", "cx_form"):  # the forms tests/test_gpu_posthoc_forms.py asserts
        assert f'"{key}"' in hdr and src.count(f's == "{key}"') == 1 and f"h->{key} = " in src, key


_FIT_CALLS = {
    "variance_decomposition": lambda ds, A, Cm, kw: ds.variance_decomposition(A, Cm, **kw),
    "sample_decomposition": lambda ds, A, Cm, kw: ds.sample_decomposition(A, Cm, **kw),
    "level_scores": lambda ds, A, Cm, kw: ds.level_scores(A, Cm, 99, **kw),                          # (cov is bad as well)
    "factor_decomposition": lambda ds, A, Cm, kw: ds.factor_decomposition(A, Cm, **kw),
    "residual_products": lambda ds, A, Cm, kw: ds.residual_products(A, Cm, np.ones((19, 2)), **kw),  # (so is Q)
    "outliers": lambda ds, A, Cm, kw: ds.outliers(A, Cm, None, cap=-1, **kw),                        # (so are scale and cap)
}


@pytest.mark.parametrize("name", sorted(_FIT_CALLS))
def test_calls_on_a_fit_report_entries_first_then_inc_continuous(name, monkeypatch):
    """The order of the shared checks: a bad ``entries`` wins over a bad ``inc_continuous``, which wins over the call's own
    arguments and over factors of the wrong shape; nothing reaches the library."""
    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    ds = _fake()
    K = 4
    A = [np.zeros((3, K), order="F"), np.zeros((2, K + 1), order="F")]   # (the second block's K is wrong)
    Cm = np.ones((K, 12), order="F")
    call = _FIT_CALLS[name]
    with pytest.raises(_lib.InsiderError) as e:
        call(ds, A, Cm, dict(entries="held-out", inc_continuous=2))
    assert e.value.status == _lib.ERR_ARG and "entries must be one of ['all', 'test', 'train'], got 'held-out'" in str(e.value)
    with pytest.raises(_lib.InsiderError) as e:
        call(ds, A, Cm, dict(entries="test", inc_continuous=2))
    assert e.value.status == _lib.ERR_ARG and "inc_continuous can only be 0 or 1" in str(e.value)
    with pytest.raises(_lib.InsiderError) as e:
        call(ds, A, Cm, dict(entries="test", inc_continuous=0))
    own = {"level_scores": "cov must be", "residual_products": "Q must be n x q", "outliers": "scale is required"}
    assert e.value.status == _lib.ERR_ARG and own.get(name, "cfd_factors[1] must be 2 x 4") in str(e.value)


def test_optimize_continuous_v2_updates_a_non_contiguous_view_in_place(monkeypatch):
    """``updating_factor`` is the reference's ``rowvec&``: a row of a column-major matrix (a strided float64 view) is written
    through, not a temporary copy of it.  The library is a stand-in that doubles the vector it is handed."""
    K, n, p = 3, 4, 5

    class Stub:
        @staticmethod
        def insider_hip_optimize_continuous_v2(D, n_, p_, M, u, Cm, K_, z, g, lam, tuning, device):
            for k in range(K_):
                u[k] = 2.0 * u[k]
            return _lib.OK

    monkeypatch.setattr(_lib, "load", lambda: Stub)
    W = np.asfortranarray(np.arange(2.0 * K).reshape(2, K) + 1.0)
    row = W[1]
    assert not row.flags.c_contiguous and not row.flags.f_contiguous
    before = W.copy()
    got = api.optimize_continuous_v2(np.zeros((n, p)), None, row, np.ones((K, p)), np.ones(n), np.eye(K), 1.0, 0)
    assert np.array_equal(got, 2.0 * before[1])
    assert np.array_equal(W[1], 2.0 * before[1]) and np.array_equal(W[0], before[0])
