"""tests/solve_reference.py checked on its own, without a GPU: it agrees with np.linalg.solve, its backward error stays
below 2**-60 on every family the GPU tests use, the route it reports follows the sign of the smallest eigenvalue, a zero
column is reported singular, and the float64 yardsticks solve what they are given."""
import numpy as np
import pytest

from tests import solve_reference as sr

KS = [1, 15, 31, 47, 63]


def _systems(K):
    """(family, A, b) over the symmetric families and the non-symmetric one."""
    rng = np.random.default_rng(50 + K)
    for name, systems in sr.families(K).items():
        for A, _ in systems:
            yield name, A, rng.standard_normal(K)
    for pos in sr.indefinite_positions(K):
        yield "nonsymmetric", sr.nonsymmetric(rng, K, pos), rng.standard_normal(K)


@pytest.mark.parametrize("K", KS)
def test_agrees_with_numpy(K):
    for name, A, b in _systems(K):
        x, route = sr.solve_likely_sympd(A, b)
        want = np.linalg.solve(A, b)
        # LAPACK's own forward error: a few K eps cond
        tol = 64 * K * 2.0 ** -52 * np.linalg.cond(A)
        assert np.abs(x.astype(np.float64) - want).max() <= tol * np.abs(want).max(), (K, name, route)


@pytest.mark.parametrize("K", KS)
def test_backward_error_below_2_to_minus_60(K):
    """(Where long double is no wider than double, the refined solution is held to one rounding of double instead.)"""
    worst = {}
    for name, A, b in _systems(K):
        x, _ = sr.solve_likely_sympd(A, b)
        worst[name] = max(worst.get(name, 0.0), sr.backward_error(A, b, x))
    print(f"solve-reference K={K} backward error by family: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < (2.0 ** -60 if sr.EXTENDED else 2.0 ** -52), worst


@pytest.mark.parametrize("K", KS)
def test_route_follows_the_smallest_eigenvalue(K):
    for name, A, b in _systems(K):
        if name == "nonsymmetric":
            assert sr.solve_likely_sympd(A, b)[1] == 1
            continue
        d = np.diag(A)
        if np.all(d > 0):       # the same inertia (Sylvester), without the scaling of family ii
            A_ev = A / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
        else:
            A_ev = A
        ev = np.linalg.eigvalsh(A_ev)
        assert abs(ev[0]) > 1e-14 * np.abs(ev).max(), (K, name, ev[0])      # the sign is not a coin toss
        assert sr.solve_likely_sympd(A, b)[1] == (0 if ev[0] > 0 else 1), (K, name, ev[0])
        assert (sr.cholesky_solve(A, b) is None) == (ev[0] <= 0), (K, name)


def test_first_failing_pivot_is_where_it_was_put():
    """Family iii: the Cholesky factorisation of the leading pos x pos block succeeds, that of the leading (pos + 1) block
    does not — at pos = K - 1 the positive-definite route fails at its final pivot."""
    for K in (2, 16, 31, 33, 63):
        rng = np.random.default_rng(K)
        for pos in sr.indefinite_positions(K):
            A = sr.indefinite(rng, K, pos)
            assert pos == 0 or sr.chol_f64(A[:pos, :pos], np.ones(pos)) is not None, (K, pos)
            assert sr.chol_f64(A[:pos + 1, :pos + 1], np.ones(pos + 1)) is None, (K, pos)
            assert sr.cholesky_solve(A[:pos + 1, :pos + 1], np.ones(pos + 1)) is None, (K, pos)


@pytest.mark.parametrize("K", [1, 2, 17, 63])
def test_zero_column_is_singular(K):
    rng = np.random.default_rng(K)
    A = sr.spd(rng, K, 10.0)
    z = K // 2
    A[:, z] = 0.0
    b = rng.standard_normal(K)
    assert sr.gepp_solve(A, b)[0] is None                   # non-symmetric: the column alone
    assert sr.solve_likely_sympd(A, b) == (None, -1)
    A[z, :] = 0.0                                           # symmetric: row and column
    assert sr.solve_likely_sympd(A, b) == (None, -1)
    assert sr.gj_rowpivot_f64(A, b) is None and sr.chol_f64(A, b) is None


def test_growth_factor():
    # no growth on a diagonal matrix; the classical 2^(K-1) matrix grows to exactly that
    assert sr.gepp_solve(np.diag([3.0, -2.0, 5.0]), np.ones(3))[1] == 1
    K = 8
    W = np.eye(K) - np.tril(np.ones((K, K)), -1)
    W[:, -1] = 1.0
    x, rho = sr.gepp_solve(W, np.ones(K))
    assert rho == 2.0 ** (K - 1)
    assert sr.backward_error(W, np.ones(K), x) < 2.0 ** -60 or not sr.EXTENDED


@pytest.mark.parametrize("K", KS)
def test_yardsticks_solve(K):
    """Each float64 yardstick stays under the textbook cap K (3K + 1) 2**-52 rho on the systems of its route."""
    for name, A, b in _systems(K):
        info = {}
        x, route = sr.solve_likely_sympd(A, b, info)
        cap = K * (3 * K + 1) * 2.0 ** -52 * info["rho"]
        if route == 0:
            for f in (sr.gj_nopivot_f64, sr.chol_f64):
                assert sr.backward_error(A, b, f(A, b)) <= cap, (K, name, f.__name__)
        else:
            assert sr.backward_error(A, b, sr.gj_rowpivot_f64(A, b)) <= cap, (K, name)


def test_backward_error_definition():
    A = np.array([[2.0, 0.0], [0.0, 4.0]])
    b = np.array([2.0, 4.0])
    assert sr.backward_error(A, b, np.array([1.0, 1.0])) == 0.0
    # residual (0, 4); ||A||_inf = 4, ||x||_inf = 1, ||b||_inf = 4
    assert sr.backward_error(A, b, np.array([1.0, 0.0])) == 4.0 / 8.0
