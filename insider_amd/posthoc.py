"""Post-hoc per-interaction-level regression of the reference (R/glm_interaction.R:2-30): for every level of the
interaction indicator, the residual rows of its samples are regressed on the column factor,
``glm(response ~ . - 1, family = gaussian())`` with response = the stacked residual rows and features = t(column_factor)
repeated once per sample; coefficients and two-sided t-test p-values are returned per level.

Closed form of that stacked least-squares problem (m samples in the level, p genes, K latent dimensions):
    beta = (C C')^-1 C mean_k(residual[k, :]),   RSS = sum_k ||residual[k, :] - C' beta||^2,
    Var(beta) = RSS / (m p - K) * (m C C')^-1,   p-value = 2 * P(T_{m p - K} > |beta / se|).
glm_interaction() below is that closed form in plain numpy on a host residual matrix (the yardstick);
glm_interaction_resident() runs the same arithmetic on the device from the resident data set of a fitted object
(InsiderData.interaction_glm: one streaming pass over X, the residual never leaves the GPU).
"""
import numpy as np


def glm_interaction(residual, train_indicator, interaction_indicator, column_factor, tol=1e-10, n_cores=10):
    """-> (coeff_matrix, pval_matrix), each (#levels) x K, row i-1 for level i (R/glm_interaction.R:4-5,26-27).
    ``train_indicator``, ``tol`` and ``n_cores`` are accepted and unused, exactly like the reference's signature."""
    from scipy import stats
    residual = np.asarray(residual, dtype=np.float64)
    Cm = np.asarray(column_factor, dtype=np.float64)
    ind = np.asarray(interaction_indicator).ravel()
    K, p = Cm.shape
    levels = np.unique(ind)
    coeff = np.zeros((len(levels), K))
    pval = np.zeros((len(levels), K))
    G = Cm @ Cm.T
    Ginv = np.linalg.inv(G)
    for i in levels:
        ids = np.flatnonzero(ind == i)
        m = ids.size
        beta = Ginv @ (Cm @ residual[ids].mean(axis=0))
        rss = float(np.sum((residual[ids] - beta @ Cm) ** 2))
        dof = m * p - K
        se = np.sqrt(rss / dof * np.diag(Ginv) / m)
        coeff[int(i) - 1] = beta
        pval[int(i) - 1] = 2.0 * stats.t.sf(np.abs(beta / se), dof)
    return coeff, pval


def t_pvalues(coeff, se, dof):
    """Two-sided t-test p-values 2 P(T_dof > |coeff / se|) per row (dof per row); rows with dof 0 (empty groups) give 0,
    like the reference's matrix(0, ...) initialisation, NaN coefficients give NaN."""
    from scipy import stats
    coeff = np.asarray(coeff, dtype=np.float64)
    dof = np.asarray(dof, dtype=np.float64).reshape(-1, 1)
    pval = np.zeros_like(coeff)
    live = dof[:, 0] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        pval[live] = 2.0 * stats.t.sf(np.abs(coeff[live] / np.asarray(se)[live]), dof[live])
    return pval


def glm_interaction_resident(obj, group_cov, subtract=None):
    """glm_interaction() of a fitted ``Insider`` object (api.insider + api.fit) on the device: the interaction levels are
    column ``group_cov`` (0-based) of obj["confounder"] (insider(interaction_idx=...) puts its indicator in column 1), the
    residual is X minus the blocks flagged in ``subtract`` (default: every covariate block except ``group_cov``: the
    main-effects residual, so that the coefficients are interaction effects), the factors obj["cfd_matrices"] /
    obj["column_factor"].  -> (coeff_matrix, pval_matrix), each L x K, row l-1 for level l, like glm_interaction()."""
    from . import api
    ds = api._resident(obj, "fit")
    inc = int(obj["inc_continuous"])
    group_cov = int(group_cov)
    if not 0 <= group_cov < ds.c:
        raise ValueError(f"group_cov must be a categorical covariate column in 0..{ds.c - 1}")
    if subtract is None:
        subtract = [b != group_cov for b in range(ds.c + inc)]
    cfd = list(obj["cfd_matrices"].values())
    group = np.asarray(obj["confounder"])[:, group_cov]
    coeff, se, dof = ds.interaction_glm(cfd, obj["column_factor"], group, subtract=subtract, inc_continuous=inc,
                                        n_groups=int(ds.n_levels[group_cov]))
    return coeff, t_pvalues(coeff, se, dof)
