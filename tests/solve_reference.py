"""A plain high-precision reference of solve(A, b, solve_opts::likely_sympd) for the tests that compare the device solves
form by form (tests/test_gpu_solve_forms.py): numpy ``longdouble``, no LAPACK, nothing of the product imported.

Reference (longdouble):
    cholesky_solve(A, b)        -> x, or None when a pivot is not > 0 ("not positive definite")
    gepp_solve(A, b)            -> (x, rho), x None when a pivot column is exactly zero ("singular"); rho is the growth
                                   factor max_k max_ij |a_ij^(k)| / max_ij |a_ij| of the elimination
    solve_likely_sympd(A, b)    -> (x, route): Cholesky first (route 0; symmetric A only), else the general route (1), each
                                   followed by three steps of iterative refinement with the residual in longdouble;
                                   route -1 and x = None when the system is singular
    backward_error(A, b, x)     = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), in longdouble

Yardsticks (float64, plain numpy loops; only to size the bounds of the tests, never a reference):
    gj_nopivot_f64(A, b)        pivot-free Gauss-Jordan, one reciprocal per column (the register route of the level solve)
    chol_f64(A, b)              Cholesky with forward and back substitution (the LDS route)
    gj_rowpivot_f64(A, b)       Gauss-Jordan with row pivoting (the general route)

Test systems: the families of tests/test_gpu_solve_forms.py, shared with tests/test_solve_reference_cpu.py.

EXTENDED tells whether the host's long double is wider than double; the 2**-60 condition on the reference's own backward
error is asserted only where it is."""
import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps < np.finfo(np.float64).eps)
U = 2.0 ** -53          # unit roundoff of float64; the bounds of the tests are written with 2**-52 = 2 U


# ----------------------------------------------------------------------------------------------------------------------
# reference, longdouble
# ----------------------------------------------------------------------------------------------------------------------
def _chol_factor(A):
    """L (lower, longdouble) with L L' = A from the lower triangle of A, or None at a pivot that is not > 0."""
    K = A.shape[0]
    L = np.zeros((K, K), dtype=LD)
    for j in range(K):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < K:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _chol_apply(L, b):
    K = L.shape[0]
    y = np.array(b, dtype=LD)
    for j in range(K):
        y[j] = (y[j] - np.dot(L[j, :j], y[:j])) / L[j, j]
    for j in range(K - 1, -1, -1):
        y[j] = (y[j] - np.dot(L[j + 1:, j], y[j + 1:])) / L[j, j]
    return y


def cholesky_solve(A, b):
    """x with A x = b by Cholesky in longdouble; None when A is not positive definite (a pivot not > 0)."""
    L = _chol_factor(np.asarray(A, dtype=LD))
    return None if L is None else _chol_apply(L, b)


def _gepp_factor(A):
    """(LU packed, perm, rho) of P A = L U by Gaussian elimination with partial pivoting (lowest row on ties), or
    (None, None, rho) when a pivot column is exactly zero."""
    M = np.array(A, dtype=LD)
    K = M.shape[0]
    perm = np.arange(K)
    amax = np.abs(M).max() if K else LD(0)
    gmax = amax
    for j in range(K):
        r = j + int(np.argmax(np.abs(M[j:, j])))
        if M[r, j] == 0:
            return None, None, (gmax / amax if amax > 0 else LD(1))
        if r != j:
            M[[j, r]] = M[[r, j]]
            perm[[j, r]] = perm[[r, j]]
        if j + 1 < K:
            M[j + 1:, j] /= M[j, j]
            M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:])
            gmax = max(gmax, np.abs(M[j + 1:, j + 1:]).max())
    return M, perm, gmax / amax


def _gepp_apply(M, perm, b):
    K = M.shape[0]
    y = np.array(b, dtype=LD)[perm]
    for j in range(K):
        y[j] -= np.dot(M[j, :j], y[:j])
    for j in range(K - 1, -1, -1):
        y[j] = (y[j] - np.dot(M[j, j + 1:], y[j + 1:])) / M[j, j]
    return y


def gepp_solve(A, b):
    """(x, rho): Gaussian elimination with partial pivoting in longdouble; x is None when A is singular (an exactly zero
    pivot column)."""
    M, perm, rho = _gepp_factor(np.asarray(A, dtype=LD))
    return (None if M is None else _gepp_apply(M, perm, b)), rho


def solve_likely_sympd(A, b, info=None, refine=3):
    """(x, route) as Armadillo's solve(A, b, likely_sympd) decides: the Cholesky route (0) when A is symmetric and every
    pivot is > 0, else the general route (1); (None, -1) when that finds a zero pivot column.  ``info`` (a dict, optional)
    receives rho, the growth factor of the general route (1 on route 0)."""
    Aq = np.asarray(A, dtype=LD)
    bq = np.asarray(b, dtype=LD)
    L = _chol_factor(Aq) if np.array_equal(Aq, Aq.T) else None
    rho = LD(1)
    if L is not None:
        route, apply = 0, (lambda r: _chol_apply(L, r))
    else:
        M, perm, rho = _gepp_factor(Aq)
        if M is None:
            if info is not None:
                info["rho"] = float(rho)
            return None, -1
        route, apply = 1, (lambda r: _gepp_apply(M, perm, r))
    x = apply(bq)
    for _ in range(refine):
        x = x + apply(bq - Aq @ x)
    if info is not None:
        info["rho"] = float(rho)
    return x, route


def backward_error(A, b, x):
    """||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) in longdouble (0 for a zero system with a zero solution)."""
    Aq, bq, xq = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD), np.asarray(x, dtype=LD)
    num = np.abs(bq - Aq @ xq).max()
    den = np.abs(Aq).sum(axis=1).max() * np.abs(xq).max() + np.abs(bq).max()
    return float(num / den) if den > 0 else float(num)


# ----------------------------------------------------------------------------------------------------------------------
# yardsticks, float64
# ----------------------------------------------------------------------------------------------------------------------
def gj_nopivot_f64(A, b):
    """Gauss-Jordan elimination without pivoting: one reciprocal per column, every other row reduced by its multiple of the
    pivot row, the solution b_i / pivot_i at the end.  Returns x (non-finite when a pivot is zero)."""
    M = np.array(A, dtype=np.float64)
    y = np.array(b, dtype=np.float64)
    K = M.shape[0]
    piv = np.ones(K)
    with np.errstate(all="ignore"):
        for j in range(K):
            piv[j] = M[j, j]
            rp = 1.0 / M[j, j]
            f = M[:, j] * rp
            f[j] = 0.0
            for c in range(j + 1, K):
                M[:, c] = M[:, c] - f * M[j, c]
            y = y - f * y[j]
        return y / piv


def chol_f64(A, b):
    """Cholesky (column by column, trailing updates) with forward and back substitution; None when not positive definite."""
    M = np.array(A, dtype=np.float64)
    y = np.array(b, dtype=np.float64)
    K = M.shape[0]
    for j in range(K):
        if not M[j, j] > 0.0:
            return None
        s = np.sqrt(M[j, j])
        M[j, j] = s
        M[j + 1:, j] = M[j + 1:, j] / s
        for c in range(j + 1, K):
            M[c:, c] = M[c:, c] - M[c:, j] * M[c, j]
    for j in range(K):
        y[j] = y[j] / M[j, j]
        y[j + 1:] = y[j + 1:] - M[j + 1:, j] * y[j]
    for j in range(K - 1, -1, -1):
        y[j] = y[j] / M[j, j]
        y[:j] = y[:j] - M[j, :j] * y[j]
    return y


def gj_rowpivot_f64(A, b):
    """Gauss-Jordan elimination with row pivoting (the largest entry of the column among the rows not yet used, lowest row
    on ties; no row is moved).  None when a pivot column is exactly zero."""
    M = np.array(A, dtype=np.float64)
    y = np.array(b, dtype=np.float64)
    K = M.shape[0]
    used = np.zeros(K, dtype=bool)
    col_of = np.full(K, -1)
    for j in range(K):
        cand = np.where(used, -1.0, np.abs(M[:, j]))
        pr = int(np.argmax(cand))
        if not cand[pr] > 0.0:
            return None
        f = M[:, j] / M[pr, j]
        f[pr] = 0.0
        for c in range(j + 1, K):
            M[:, c] = M[:, c] - f * M[pr, c]
        y = y - f * y[pr]
        used[pr] = True
        col_of[pr] = j
    x = np.empty(K)
    for r in range(K):
        x[col_of[r]] = y[r] / M[r, col_of[r]]
    return x


# ----------------------------------------------------------------------------------------------------------------------
# test systems
# ----------------------------------------------------------------------------------------------------------------------
def _sym(A):
    """Exactly symmetric: the upper triangle mirrored."""
    return np.triu(A) + np.triu(A, 1).T


def _orth(rng, K):
    Q, R = np.linalg.qr(rng.standard_normal((K, K)))
    return Q * np.sign(np.diag(R))


def spd(rng, K, cond):
    """Family i: Q diag(s) Q', s log-spaced from 1 down to 1 / cond."""
    Q = _orth(rng, K)
    s = np.logspace(0.0, -np.log10(cond), K) if K > 1 else np.ones(1)
    return _sym((Q * s) @ Q.T)


def spd_scaled(rng, K, cond):
    """Family ii: D A D, A of family i, D = diag(10**u), u uniform in [-3, 3]."""
    d = 10.0 ** rng.uniform(-3.0, 3.0, K)
    return _sym(spd(rng, K, cond) * d[:, None] * d[None, :])


def indefinite(rng, K, pos):
    """Family iii: symmetric, the leading pos x pos block positive definite and pivot `pos` of the elimination = -1 (up to
    rounding): M = [[B, V], [V', V' B^-1 V + S]] with S = diag(-1, 1, ..., 1).  pos = K - 1 is [[B, v], [v', v' B^-1 v - 1]]."""
    assert 0 <= pos < K
    S = np.ones(K - pos)
    S[0] = -1.0
    A = np.zeros((K, K))
    if pos:
        B = spd(rng, pos, 100.0)
        V = rng.standard_normal((pos, K - pos)) / np.sqrt(K)
        A[:pos, :pos] = B
        A[:pos, pos:] = V
        A[pos:, pos:] = V.T @ np.linalg.solve(B, V)
    T = rng.standard_normal((K - pos, K - pos)) * 0.3 / np.sqrt(K)
    Lt = np.tril(T, -1) + np.eye(K - pos)
    A[pos:, pos:] += (Lt * S) @ Lt.T
    return _sym(A)


def zero_diagonal(rng, K, tie=False):
    """Family iv (K >= 2; tie: K >= 3): symmetric, a_00 = 0 with a non-zero column below it, so the general route has to
    exchange rows at its first step.  tie: the two largest entries of column 0 have the same magnitude and opposite signs."""
    A = _sym(rng.standard_normal((K, K)))
    A[0, 0] = 0.0
    if K > 2:
        A[K // 2, K // 2] = 0.0
    if tie:
        A[1, 0] = A[0, 1] = 4.0
        A[2, 0] = A[0, 2] = -4.0
    return A


def nonsymmetric(rng, K, pos):
    """Family v: the upper triangle of indefinite(K, pos), an unrelated lower triangle."""
    A = np.triu(indefinite(rng, K, pos)) + np.tril(rng.standard_normal((K, K)), -1) / np.sqrt(K)
    if K > 1:
        A[K - 1, 0] += 1.0      # never symmetric by accident
    return A


def indefinite_positions(K):
    return sorted({0, K // 2, K - 1})


def families(K, seed=0):
    """{name: list of (A, cond)} — the symmetric families i-iv at rank K; cond is the condition number the family was built
    for (None where it was not controlled).  Five to nine systems per family."""
    rng = np.random.default_rng(1000 * K + seed)
    conds = (1.0, 1e4, 1e8, 1e12)
    pos = indefinite_positions(K)
    out = {"spd": [(spd(rng, K, c), c) for c in conds for _ in range(2)],
           "scaled": [(spd_scaled(rng, K, c), None) for c in conds for _ in range(2)],
           "indefinite": [(indefinite(rng, K, pos[t % len(pos)]), None) for t in range(6 if len(pos) < 3 else 9)]}
    if K >= 2:
        out["zero_diag"] = [(zero_diagonal(rng, K, tie=(K >= 3 and t % 2 == 1)), None) for t in range(6)]
    return out
