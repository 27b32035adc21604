"""The stand-in headers of oracle/ref_shim on their own: the driver's `selftest` entry applies every primitive the
reference's translation units use to arrays read from files, and each result is compared with numpy.

  * to the bit where the operation is exact or a single rounding (indexing, find, unique, element-wise arithmetic, relational
    operators, views and their assignment);
  * within n 2**-52 of the sum of absolute values of the terms for the reductions (n terms, any summation order: Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2), plus the single rounding of a final division or square root;
  * by backward error for solve(), at K (3K + 1) 2**-52 (the cap tests/test_solve_reference_cpu.py:99-106 holds the float64
    Cholesky yardstick to; rho = 1 on the Cholesky route), and against tests/solve_reference.py's longdouble Cholesky.

Shapes: 1 x 1, a single row, a single column, non-square both ways; index vectors in non-monotone order with repeats.
Skips when oracle/_ref/insider_ref is not built (no reference tree or no C++ compiler)."""
import numpy as np
import pytest

from oracle import ref
from tests import solve_reference as sr

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/insider_ref not built (reference tree or C++ compiler absent)")

EPS = 2.0 ** -52
SHAPES = [(1, 1), (1, 6), (7, 1), (5, 8), (9, 4)]


def _inputs(r, c, seed):
    rng = np.random.default_rng([r, c, seed])
    k = min(r, c)
    A = rng.standard_normal((r, c))
    B = rng.standard_normal((r, c))
    ind = (rng.random((r, c)) < 0.6).astype(np.float64)
    ind.flat[0] = 0.0                                   # at least one zero and (below) one non-zero where the size allows
    if r * c > 1:
        ind.flat[-1] = 1.0
    S = sr.spd(rng, c, 1e4) * 3.0
    Um = rng.integers(1, 4, size=(max(r, 2), 2)).astype(np.uint32)
    Um[1] = Um[0] if r % 2 else Um[0] + 1
    return dict(A=A, B=B, P=rng.standard_normal((r, c)), S=S, RHS=rng.standard_normal((c, 2)), I=ind,
                v=rng.standard_normal(r), w=rng.standard_normal(r),
                ri=rng.integers(0, r, size=r + 2).astype(np.uint32)[::-1].copy(),          # non-monotone, with repeats
                ci=rng.permutation(k).astype(np.uint32)[::-1].copy(),
                ei=np.concatenate([rng.permutation(r * c)[: max(1, (r * c) // 2)], [0]]).astype(np.uint32),
                lv=rng.integers(1, 5, size=r).astype(np.uint32), Um=Um), dict(sc=0.7, r0=r - 1, c0=c // 2)


@pytest.fixture(scope="module", params=SHAPES, ids=["%dx%d" % s for s in SHAPES])
def run(request):
    r, c = request.param
    arrays, scalars = _inputs(r, c, 3)
    return arrays, scalars, ref.run_case("selftest", scalars, arrays, timeout=60)


def _col(x):
    return np.asarray(x).reshape(-1, 1)


def _find(x):
    return _col(np.flatnonzero(np.asarray(x).reshape(-1, order="F")).astype(np.uint32))


def test_exact_primitives(run):
    a, s, out = run
    A, B, P, S, ind, v, w, ri, ci, ei, lv, Um = (a[k] for k in ("A", "B", "P", "S", "I", "v", "w", "ri", "ci", "ei", "lv", "Um"))
    sc, r0, c0 = s["sc"], s["r0"], s["c0"]
    r, c = A.shape
    W = A.copy()
    W[r0, :] = 2.0 * A[r0, :]
    W[:, c0] = A[:, c0] - B[:, c0]
    Z = A.copy(order="F")
    Z.reshape(-1, order="F")[ei] = 0.0          # a view: Z is F-contiguous
    o = v.copy()
    o[ci] = 1.0
    o[np.flatnonzero(np.abs(v) > sc)] = 0.0
    D = S.copy()
    D[np.diag_indices(c)] += sc
    Af = A.reshape(-1, order="F")
    expect = {
        "dims": np.array([[r, c, r * c, r * c, 0, 1]], dtype=np.float64),
        "zeros_rc": np.zeros((r, c)), "zeros_size": np.zeros((r, c)), "zeros_vec": np.zeros((r, 1)),
        "zeros_uvec": np.zeros((r, 1), dtype=np.uint32), "ones_n": np.ones((r, 1)),
        "find_I": _find(ind), "find_row_eq0": _find(ind[r0, :] == 0), "find_col_eq0": _find(ind[:, c0] == 0),
        "find_trow": _find(ind[r0, :]), "find_lv_eq": _find(lv == lv[0]), "find_Um_col_eq": _find(Um[:, 0] == Um[0, 0]),
        "unique_lv": _col(np.unique(lv)), "unique_Um_col": _col(np.unique(Um[:, 0])),
        "lt": _col(np.abs(v) < sc).astype(np.uint32), "gt": _col(np.abs(v) > sc).astype(np.uint32),
        "trans_A": A.T, "t_A": A.T, "trans_v": v.reshape(1, -1), "trans_row": _col(A[r0, :]), "row_t": _col(A[r0, :]),
        "square_A": A * A, "pow_A_2": A * A, "pow_v_2": _col(v * v), "abs_A": np.abs(A), "max_abs_v": np.abs(v).max(),
        "sign": np.array([[-1.0, 0.0, 1.0]]),
        "approx_equal": np.array([[1.0, float(np.array_equal(Um[0], Um[1])), 1.0]]),
        "randperm": _col(np.arange(7, dtype=np.uint32)),
        "row_r0": A[r0:r0 + 1, :], "col_c0": A[:, c0:c0 + 1], "rows_ri": A[ri, :], "cols_ci": A[:, ci], "Um_rows": Um[ri, :],
        "elem_ei": _col(Af[ei]), "paren_ei": _col(v[ci]), "sub_ri_ci": A[np.ix_(ri, ci)], "ei_of_ci": _col(ei[np.flatnonzero(ei > 0)]),
        "at": np.array([[A[r0, c0], A[r0, c0]]]),
        "assign_rowcol": W, "elem_zeros": Z, "elem_ones": _col(o), "diag_plus": D, "zeros_member": np.zeros((r, c)),
        "ones_member": np.ones((r, 1)), "field_1": B, "mat_ptr": A, "plus": A + B, "minus": A - B, "schur": A * B,
        "outer": np.outer(v, w), "scal_l": sc * A, "scal_r": A * sc, "uw_scal": float(len(ri)) * A, "plus_eq": A + B,
        "minus_eq": A - sc * B, "uvec_minus_1": _col(lv - 1), "rcpp_roundtrip": A, "rcpp_scalar": sc,
    }
    for name, e in expect.items():
        got = out[name]
        if np.ndim(e) == 0:
            assert got == e, name
        else:
            assert got.shape == e.shape and got.dtype == e.dtype, (name, got.shape, e.shape, got.dtype)
            assert np.array_equal(got, e), name
    assert out["sweeps"] == 1                                         # the one randperm call was counted
    assert out["log"] == "selftest %d\n" % r                          # cout / endl reach the log


def test_reductions_within_n_eps_of_the_absolute_sum(run):
    a, s, out = run
    A, B, P, v, w, ri = (a[k] for k in ("A", "B", "P", "v", "w", "ri"))
    r0, c0 = s["r0"], s["c0"]
    r, c = A.shape
    LD = np.longdouble

    def close(name, exact, n, abs_sum, extra=0.0):
        got = np.asarray(out[name], dtype=LD)
        tol = n * EPS * np.asarray(abs_sum, dtype=np.float64) + extra
        assert np.all(np.abs(got - exact) <= tol), (name, float(np.max(np.abs(got - exact) - tol)))

    Aq, Bq, Pq, vq, wq = (np.asarray(x, dtype=LD) for x in (A, B, P, v, w))
    close("sum_v", vq.sum(), r, np.abs(v).sum())
    close("sum_row", Aq[r0].sum(), c, np.abs(A[r0]).sum())
    close("sum_A_1", Aq.sum(axis=1).reshape(-1, 1), c, np.abs(A).sum(axis=1).reshape(-1, 1))
    close("sum_A_0", Aq.sum(axis=0).reshape(1, -1), r, np.abs(A).sum(axis=0).reshape(1, -1))
    close("sum_sum_abs", np.abs(Aq).sum(), r * c, np.abs(A).sum())
    close("accu_A", Aq.sum(), r * c, np.abs(A).sum())
    close("mean_v", vq.sum() / r, r, np.abs(v).sum() / r, extra=EPS * abs(float(v.mean())))
    close("dot_vw", (vq * wq).sum(), r + 1, np.abs(v * w).sum())
    close("dot_col", (vq * Aq[:, c0]).sum(), r + 1, np.abs(v * A[:, c0]).sum())
    nA, nr = np.sqrt((Aq * Aq).sum()), np.sqrt((Aq[r0] * Aq[r0]).sum())
    close("norm_A", nA, r * c + 2, float(nA))
    close("norm_row", nr, c + 2, float(nr))
    close("as_scalar", vq @ Aq @ Pq[0], r + c + 2, np.abs(v) @ np.abs(A) @ np.abs(P[0]))
    close("matmul", Aq @ Bq.T, c + 1, np.abs(A) @ np.abs(B).T)
    close("matvec", (Aq.T @ vq).reshape(-1, 1), r + 1, (np.abs(A).T @ np.abs(v)).reshape(-1, 1))
    outer = np.einsum("ia,ib->iab", Pq, Pq)
    close("cube_sum", outer[ri].sum(axis=0), len(ri) + 1, np.abs(np.asarray(outer, dtype=np.float64))[ri].sum(axis=0))


def test_solve_is_a_cholesky_solve_by_backward_error(run):
    a, _, out = run
    S, RHS = a["S"], a["RHS"]
    K = S.shape[0]
    cap = K * (3 * K + 1) * EPS                                       # tests/test_solve_reference_cpu.py:99-106, rho = 1
    assert out["solve_vec"].shape == (K, 1) and out["solve_mat"].shape == (K, 2)
    assert np.array_equal(out["solve_vec"][:, 0], out["solve_mat"][:, 0])
    cond = np.linalg.cond(S)
    for j in range(2):
        x = out["solve_mat"][:, j]
        assert sr.backward_error(S, RHS[:, j], x) <= cap, (K, j)
        xr = sr.cholesky_solve(S, RHS[:, j])
        # forward, as tests/test_gpu_solve_forms.py:23 has it: 4 K^2 2**-52 rho cond_2(A) ||x_ref||_inf
        assert float(np.abs(x - xr).max()) <= 4 * K * K * EPS * cond * float(np.abs(xr).max())


def test_refused_constructs_abort_with_a_message():
    """Where Armadillo's behaviour is not settled the stand-in aborts and names the construct: a gene with no
    held-out entry reaches sum(cube.slices(empty), 2) at src/optimize.cpp:218; a matrix that is not positive definite reaches
    solve(); mean() of no test entries (src/utils.cpp:67)."""
    rng = np.random.default_rng(0)
    n, p, K = 6, 3, 2
    X, R, C = rng.standard_normal((n, p)), rng.standard_normal((n, K)), rng.standard_normal((K, p))
    M = np.ones((n, p))
    M[0, 1:] = 0                                                      # gene 0 keeps every entry
    with pytest.raises(ref.RefError, match=r"refuses: sum\(cube.slices\(idx\), 2\) with an empty index selection"):
        ref.optimize_col(X, M, R, C, 1.0, 0.4, tuning=1)
    with pytest.raises(ref.RefError, match="refuses: solve.*not positive definite"):
        ref.optimize_col(X, M, np.zeros((n, K)), C, 0.0, 0.0, tuning=0)
    with pytest.raises(ref.RefError, match="refuses: mean.*no elements"):
        ref.state(X, R, [rng.standard_normal((2, K))], C, M, np.zeros((n, p)), 1.0, 1.0, 0.4, 1, np.zeros(3), np.zeros(2))
    with pytest.raises(ref.RefError, match="index out of bounds"):     # bounds-checked: a level id beyond the factor's rows
        ref.optimize_row(X, M, rng.standard_normal((2, K)), C, np.array([1, 2, 3, 1, 2, 3]), C @ C.T, 1.0, tuning=1)
