"""A plain high-precision reference of the per-group regression of insider_hip_interaction_glm() (the closed form stated in
include/insider_hip.h), for the tests that compare the device path form by form: every quantity in ``np.longdouble``, the
normal equations solved by a Cholesky factorisation written out here, RSS in its direct form (the residual of the fit,
squared and summed: no cancellation).  Nothing of the product is imported.

EXTENDED tells whether the host's long double is wider than double.  Where it is not (a 64-bit long double), the
reference carries double rounding itself, of the order of K eps cond(G); the GPU tests' bounds are stated against the exact
result and hold against it all the same (they leave a factor 64 over that)."""
import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps < np.finfo(np.float64).eps)


def cholesky_lower(G):
    """L (lower triangular, longdouble) with L L' = G; ValueError at a pivot that is not positive."""
    r = G.shape[0]
    L = np.zeros((r, r), dtype=LD)
    for j in range(r):
        d = G[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise ValueError(f"pivot {j + 1} of {r} is not positive")
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, r):
            L[i, j] = (G[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def lower_inverse(L):
    """L^-1 (lower triangular) by forward substitution on the identity, column by column."""
    r = L.shape[0]
    Li = np.zeros((r, r), dtype=LD)
    for c in range(r):
        Li[c, c] = LD(1) / L[c, c]
        for i in range(c + 1, r):
            Li[i, c] = -np.dot(L[i, c:i], Li[c:i, c]) / L[i, i]
    return Li


def glm_reference(R, group, G, C):
    """R: n x p residual rows; group: n ids in 0..G (0 = in no group); C: K x p column factor.  Per group g (row g - 1) over
    the rows of C that are not entirely zero (``keep``, rank r): beta_g = (C C')^-1 C mean(r_i), RSS_g = sum_i ||r_i -
    C' beta_g||^2, dof_g = m_g p - r, se_g = sqrt(RSS_g / dof_g diag((C C')^-1) / m_g).  -> dict of
        coeff, se (G x K, NaN in the dropped columns, zero rows for empty groups), dof, rss, ss (= sum_i ||r_i||^2), m (G),
        dinv (K: diag((C C')^-1), NaN where dropped), keep (indices), cond (the 2-norm condition number of the reduced C C').
    coeff, se, dof, rss, ss and dinv are longdouble."""
    R = np.asarray(R, dtype=LD)
    Cm = np.asarray(C, dtype=LD)
    grp = np.asarray(group).ravel().astype(np.int64)
    n, p = R.shape
    K = Cm.shape[0]
    if Cm.shape[1] != p or grp.shape != (n,):
        raise ValueError("shapes of R, group and C do not agree")
    keep = np.flatnonzero((Cm != 0).any(axis=1))
    r = keep.size
    Ck = Cm[keep]
    Gm = Ck @ Ck.T
    Li = lower_inverse(cholesky_lower(Gm))
    dinv = np.full(K, np.nan, dtype=LD)
    dinv[keep] = (Li * Li).sum(axis=0)
    coeff = np.zeros((G, K), dtype=LD)
    se = np.zeros((G, K), dtype=LD)
    dof, rss, ss = (np.zeros(G, dtype=LD) for _ in range(3))
    m = np.zeros(G, dtype=np.int64)
    for g in range(1, G + 1):
        rows = np.flatnonzero(grp == g)
        m[g - 1] = rows.size
        if rows.size == 0:
            continue
        Rg = R[rows]
        beta = Li.T @ (Li @ (Ck @ (Rg.sum(axis=0) / LD(rows.size))))
        E = Rg - beta @ Ck
        rss[g - 1] = (E * E).sum()
        ss[g - 1] = (Rg * Rg).sum()
        dof[g - 1] = LD(rows.size) * LD(p) - LD(r)
        coeff[g - 1] = np.nan
        se[g - 1] = np.nan
        coeff[g - 1, keep] = beta
        se[g - 1, keep] = np.sqrt(rss[g - 1] / dof[g - 1] * dinv[keep] / LD(rows.size))
    cond = float(np.linalg.cond(Gm.astype(np.float64), 2)) if r else 1.0
    return dict(coeff=coeff, se=se, dof=dof, rss=rss, ss=ss, m=m, dinv=dinv, keep=keep, cond=cond)
