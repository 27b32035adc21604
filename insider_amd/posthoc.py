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

variance_decomposition() answers a different question per gene: how much of its variance each covariate block carries
and how well the model fits it (InsiderData.variance_decomposition: the level table [A_stack; B_c] C, then one streaming
pass over X); variance_decomposition_host() is the same record in plain numpy (the yardstick).

sample_decomposition() is the same record per sample instead of per gene (InsiderData.sample_decomposition: how well the
model fits each sample, which samples are outliers, what each block carries of a sample's variance), with
sample_decomposition_host() as its yardstick; level_decomposition() pools the samples of each level of a covariate
(per donor, per tissue).

factor_decomposition() splits the per-gene record along the K latent factors (InsiderData.factor_decomposition: which
factors matter, which covariate drives factor k, in which genes it acts), with factor_decomposition_host() as its
yardstick, fd_derived() for the per-gene shares and factor_summary() for the (B + 1) x K tables pooled over genes.

outliers() lists the entries themselves: the (sample, gene) entries whose standardised residual the model cannot explain
(InsiderData.outliers: a flag pass over X into a bitmap, a scan, a fill pass over the bitmap), with outliers_host() as its
yardstick and residual_center_scale() for the per-gene center and scale from a variance-decomposition record.

level_scores() asks whether each sample's label of a covariate is right: every sample scored against every level's embedding
(InsiderData.level_scores: the candidate table cand C, then one streaming pass over X as two masked products over the genes),
with level_scores_host() as its yardstick and ls_derived() for best / second / margin / flagged / confusion.

residual_components() asks what the model has left behind across samples and genes at once: the leading singular directions
of the masked (optionally standardised) residual, by a block subspace iteration whose two thin products per step run on the
device (InsiderData.residual_products: R never exists), with residual_products_host() / residual_components_host() as the
yardsticks (the same driver on the numpy operator) and component_associations() to tell a component tied to a known
covariate (misfit, a missing interaction) from one tied to none (an unknown factor).

gene_coexpression() / sample_coexpression() ask the pairwise question about the same residual: which genes still move
together, which samples' residuals correlate (InsiderData.coexpression: the standardised residual staged once on the device,
then an n- or p-deep product with the top-k selection fused behind it; the zero-filled correlation, not the pairwise-complete
one, where entries are missing; missing="pairwise" asks for the pairwise-complete one, InsiderData.coexpression_pairwise: six
products); coexpression_host() is the yardstick, gram_topk_host() / gram_topk_pairwise_host() those of the handle-free
api.gram_topk() / api.gram_topk_pairwise().

gene_neighbors() / sample_neighbors() ask the latent representations themselves which genes lie next to a gene and which
samples next to a sample (api.neighbors: a K-deep product on the device with the top-k selection fused behind it, the
similarity matrix never exists), on column_factor and on sample_embeddings(); neighbors_host() is the yardstick.
gene_modules() / sample_clusters() partition the same two embeddings (api.kmeans: the whole Lloyd loop on the device, cosine or
Euclidean, restarts); kmeans_host() is the yardstick, module_overrepresentation() / module_summary() read the modules.
gene_map() / sample_map() draw them: the exact t-SNE map of the embeddings' cosine neighbour graph (embedding_graph(), api.tsne:
the whole optimisation on the device, the all-pairs repulsion summed in fp64, the same map to the bit from run to run);
tsne_host() is the yardstick.
gene_tree() / sample_tree() / level_tree() build their dendrograms (api.hclust: average linkage of cosine distances or Ward's
linkage, rounds of reciprocal nearest neighbours on the device, the N x N distances never exist); hclust_host() is the
yardstick, cut_tree() cuts a tree into flat clusters, tree_overrepresentation() reads the modules of a cut.

factor_enrichment() / level_enrichment() ask what a factor or a level effect means: a preranked gene-set enrichment of the
rows of column_factor, or of A_b @ column_factor, with a permutation null of random gene sets of equal size
(api.enrichment: per (profile, set) a sort and a scan on the device, the null table never exists); enrichment_host() is the
yardstick, gs_derived() gives p, NES, FDR and the hypergeometric p, leading_edge() a set's leading genes.
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


def _fitted(obj, which):
    """What every call on a fitted ``Insider`` object starts from: its resident data set ``which`` ("fit" or "tune"), the
    list of its row factors, its column factor and its inc_continuous flag."""
    from . import api
    return api._resident(obj, which), list(obj["cfd_matrices"].values()), obj["column_factor"], int(obj["inc_continuous"])


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


def vd_derived(rec):
    """The raw per-gene sums of a variance decomposition (InsiderData.variance_decomposition) plus
        tss = sum x^2 - (sum x)^2 / n,  r2 = 1 - rss / tss,  rmse = sqrt(rss / n),
        explained[b] = (sum g_b^2 - (sum g_b)^2 / n) / tss   (the share of the gene's variance block b carries),
        drop_one[b] = (sum g_b^2 + 2 sum r g_b) / tss         (the rise in RSS, over tss, when block b leaves the fit).
    tss is formed from the raw sums (one pass, no centring): for a gene whose mean is large against its spread it loses
    digits to cancellation.  The explained shares do not add up to r2: the cross terms between blocks (and between the
    fit and the residual) are not split among them.  A gene with n = 0 gets NaN in every derived value."""
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    n = out["n"]
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = np.where(n > 0, n, np.nan)
        tss = out["sum_xx"] - out["sum_x"] ** 2 / nn
        out["tss"] = tss
        out["r2"] = 1.0 - out["rss"] / tss
        out["rmse"] = np.sqrt(out["rss"] / nn)
        out["explained"] = (out["sum_gg"] - out["sum_g"] ** 2 / nn) / tss
        out["drop_one"] = (out["sum_gg"] + 2.0 * out["sum_rg"]) / tss
    return out


def _decomposition_host(X, levels, ctns, mask, A, C, axis):
    """The raw sums of the decomposition record over ``axis`` of the n x p terms (0: per gene, 1: per sample)."""
    X = np.asarray(X, dtype=np.float64)
    Cm = np.asarray(C, dtype=np.float64)
    lev = np.asarray(levels).reshape(X.shape[0], -1)
    c = lev.shape[1]
    g = [np.asarray(A[b], dtype=np.float64)[lev[:, b].astype(np.int64) - 1] @ Cm for b in range(c)]
    if ctns is not None:
        Z = np.asarray(ctns, dtype=np.float64).reshape(X.shape[0], -1)
        g.append(Z @ (np.asarray(A[c], dtype=np.float64) @ Cm))
    f = np.zeros_like(X)
    for gb in g:
        f = f + gb
    w = np.ones(X.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    r = np.where(w, X - f, 0.0)
    xs = np.where(w, X, 0.0)
    gs = [np.where(w, gb, 0.0) for gb in g]
    return dict(n=w.sum(axis=axis).astype(np.float64), sum_x=xs.sum(axis=axis), sum_xx=(xs * xs).sum(axis=axis),
                rss=(r * r).sum(axis=axis), sum_g=np.array([gb.sum(axis=axis) for gb in gs]).reshape(len(g), -1),
                sum_gg=np.array([(gb * gb).sum(axis=axis) for gb in gs]).reshape(len(g), -1),
                sum_rg=np.array([(r * gb).sum(axis=axis) for gb in gs]).reshape(len(g), -1))


def variance_decomposition_host(X, levels, ctns, mask, A, C):
    """The variance-decomposition record in plain numpy (the yardstick of the device path).  X: n x p; levels: n x c level
    ids 1..L_b; ctns: n x m or None; mask: n x p (entries that count) or None (every entry); A: the c categorical row
    factors (L_b x K), then B_c (m x K) when ctns is given; C: K x p.  -> vd_derived() of the raw sums."""
    return vd_derived(_decomposition_host(X, levels, ctns, mask, A, C, 0))


def variance_decomposition(obj, which="fit", entries="train"):
    """Per-gene variance decomposition of a fitted ``Insider`` object (api.insider + api.fit / tune) on the device, over
    the entries ``entries`` of the resident data set ``which`` ("fit": train = the observed entries, test = NA; "tune": the
    ratio_splitter split, so entries="test" gives each gene's held-out error).  Blocks: the columns of obj["confounder"],
    then the continuous block.  -> vd_derived() of the raw sums: n, sum_x, sum_xx, rss (p), sum_g, sum_gg, sum_rg (B x p),
    tss, r2, rmse (p), explained, drop_one (B x p)."""
    ds, cfd, col, inc = _fitted(obj, which)
    rec = ds.variance_decomposition(cfd, col, entries=entries, inc_continuous=inc)
    return vd_derived(rec)


def sample_decomposition_host(X, levels, ctns, mask, A, C):
    """The per-sample record in plain numpy (the yardstick of InsiderData.sample_decomposition): the terms of
    variance_decomposition_host(), summed over the genes of every sample.  -> vd_derived() of the raw sums, each of length
    n (B x n per block)."""
    return vd_derived(_decomposition_host(X, levels, ctns, mask, A, C, 1))


def sample_decomposition(obj, which="fit", entries="train"):
    """Per-sample fit diagnostics of a fitted ``Insider`` object on the device: variance_decomposition() along the other
    axis, with the same ``which`` / ``entries``.  -> vd_derived() of the raw sums: n, sum_x, sum_xx, rss, tss, r2, rmse (n),
    sum_g, sum_gg, sum_rg, explained, drop_one (B x n).  A sample's tss is its spread across genes."""
    ds, cfd, col, inc = _fitted(obj, which)
    rec = ds.sample_decomposition(cfd, col, entries=entries, inc_continuous=inc)
    return vd_derived(rec)


RAW_SUMS = ("n", "sum_x", "sum_xx", "rss", "sum_g", "sum_gg", "sum_rg")


def level_decomposition(rec, level_ids, n_levels):
    """The per-sample records pooled per level of a covariate: the raw sums of ``rec`` (sample_decomposition() or
    InsiderData.sample_decomposition()) of the samples with level id l (1-based ``level_ids``, length n) are added up, row
    l - 1 of the result for level l, then vd_derived() gives per level n, r2, rmse, explained, drop_one (L and B x L).  A
    level without selected entries gets NaN in every derived value."""
    ids = np.asarray(level_ids).ravel().astype(np.int64) - 1
    L = int(n_levels)
    if ids.size and (ids.min() < 0 or ids.max() >= L):
        raise ValueError(f"level ids must be within 1..{L}")
    pooled = {}
    for k in RAW_SUMS:
        v = np.asarray(rec[k], dtype=np.float64)
        if v.shape[-1] != ids.size:
            raise ValueError(f"rec[{k!r}] holds {v.shape[-1]} samples, level_ids {ids.size}")
        out = np.zeros(v.shape[:-1] + (L,))
        np.add.at(out.reshape(-1, L).T, ids, v.reshape(-1, ids.size).T)
        pooled[k] = out
    return vd_derived(pooled)


def factor_decomposition_host(X, levels, ctns, mask, A, C):
    """The per-factor record in plain numpy (the yardstick of InsiderData.factor_decomposition); arguments as in
    variance_decomposition_host().  Blocks: the categorical covariates, the continuous block when ctns is given, then the
    total (the sum of the blocks' embeddings: the row factor).  Loops over the blocks and k: no n x p x K array is formed.
    -> fd_derived() of the raw sums n, sum_x, sum_xx, rss (p) and sum_h, sum_hh, sum_rh ((B + 1) x K x p)."""
    X = np.asarray(X, dtype=np.float64)
    Cm = np.asarray(C, dtype=np.float64)
    lev = np.asarray(levels).reshape(X.shape[0], -1)
    c = lev.shape[1]
    U = [np.asarray(A[b], dtype=np.float64)[lev[:, b].astype(np.int64) - 1] for b in range(c)]
    if ctns is not None:
        U.append(np.asarray(ctns, dtype=np.float64).reshape(X.shape[0], -1) @ np.asarray(A[c], dtype=np.float64))
    tot = np.zeros_like(U[0])
    for u in U:
        tot = tot + u
    U.append(tot)
    K, p = Cm.shape
    w = np.ones(X.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    r = np.where(w, X - tot @ Cm, 0.0)
    xs = np.where(w, X, 0.0)
    sum_h, sum_hh, sum_rh = (np.zeros((len(U), K, p)) for _ in range(3))
    for b, u in enumerate(U):
        for k in range(K):
            h = np.where(w, np.outer(u[:, k], Cm[k]), 0.0)
            sum_h[b, k], sum_hh[b, k], sum_rh[b, k] = h.sum(axis=0), (h * h).sum(axis=0), (r * h).sum(axis=0)
    return fd_derived(dict(n=w.sum(axis=0).astype(np.float64), sum_x=xs.sum(axis=0), sum_xx=(xs * xs).sum(axis=0),
                           rss=(r * r).sum(axis=0), sum_h=sum_h, sum_hh=sum_hh, sum_rh=sum_rh))


def fd_derived(rec):
    """The raw per-gene sums of a factor decomposition plus tss, r2, rmse as in vd_derived() and, per (block, factor, gene),
        explained[b, k] = (sum h^2 - (sum h)^2 / n) / tss   (the share of the gene's variance factor k carries through b),
        drop_one[b, k] = (sum h^2 + 2 sum r h) / tss         (the rise in RSS, over tss, when that term leaves the fit).
    A gene with n = 0 gets NaN in every derived value."""
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    n = out["n"]
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = np.where(n > 0, n, np.nan)
        tss = out["sum_xx"] - out["sum_x"] ** 2 / nn
        out["tss"] = tss
        out["r2"] = 1.0 - out["rss"] / tss
        out["rmse"] = np.sqrt(out["rss"] / nn)
        out["explained"] = (out["sum_hh"] - out["sum_h"] ** 2 / nn) / tss
        out["drop_one"] = (out["sum_hh"] + 2.0 * out["sum_rh"]) / tss
    return out


def factor_summary(rec, column_factor=None):
    """The (B + 1) x K tables of a factor decomposition pooled over genes: the numerators of fd_derived()'s explained and
    drop_one summed over the genes with n > 0, over the sum of their tss.  -> dict of ``explained``, ``drop_one``
    ((B + 1) x K), ``tss`` (the denominator), ``order`` (the factors by descending pooled drop_one of the total block) and,
    with ``column_factor`` (K x p) given, ``loading_nnz`` (the non-zero loadings of every factor)."""
    d = fd_derived({k: rec[k] for k in ("n", "sum_x", "sum_xx", "rss", "sum_h", "sum_hh", "sum_rh")})
    live = d["n"] > 0
    nn = d["n"][live]
    tss = float(d["tss"][live].sum())
    sh, shh, srh = (d[k][:, :, live] for k in ("sum_h", "sum_hh", "sum_rh"))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(explained=(shh - sh ** 2 / nn).sum(axis=2) / tss, drop_one=(shh + 2.0 * srh).sum(axis=2) / tss, tss=tss)
    out["order"] = np.argsort(-out["drop_one"][-1], kind="stable")
    if column_factor is not None:
        out["loading_nnz"] = np.count_nonzero(np.asarray(column_factor), axis=1)
    return out


def factor_decomposition(obj, which="fit", entries="train"):
    """Per-factor decomposition of a fitted ``Insider`` object on the device, with the ``which`` / ``entries`` of
    variance_decomposition().  -> fd_derived() of the raw sums: n, sum_x, sum_xx, rss, tss, r2, rmse (p), sum_h, sum_hh,
    sum_rh, explained, drop_one ((B + 1) x K x p; the last block is the total)."""
    ds, cfd, col, inc = _fitted(obj, which)
    rec = ds.factor_decomposition(cfd, col, entries=entries, inc_continuous=inc)
    return fd_derived(rec)


def level_scores_host(X, levels, ctns, mask, A, C, cov, candidates=None):
    """The level scores in plain numpy (the yardstick of InsiderData.level_scores); X, levels, ctns, mask, A, C as in
    variance_decomposition_host(), ``cov`` the 0-based categorical covariate, ``candidates`` (L x K) or None = A[cov].  The
    direct form: d = x - (every block but cov), sse[i, l] = sum over the entries of sample i that count of
    (d - candidates[l] . C)^2.  -> dict(sse=(n, L), n=(n,))."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    Cm = np.asarray(C, dtype=np.float64)
    lev = np.asarray(levels).reshape(n, -1)
    c = lev.shape[1]
    if not 0 <= cov < c:
        raise ValueError(f"cov must be a categorical covariate in 0..{c - 1}")
    d = X.copy()
    for b in range(c):
        if b != cov:
            d = d - np.asarray(A[b], dtype=np.float64)[lev[:, b].astype(np.int64) - 1] @ Cm
    if ctns is not None:
        d = d - np.asarray(ctns, dtype=np.float64).reshape(n, -1) @ (np.asarray(A[c], dtype=np.float64) @ Cm)
    E = np.asarray(A[cov] if candidates is None else candidates, dtype=np.float64).reshape(-1, Cm.shape[0])
    w = np.ones(X.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    sse = np.empty((n, E.shape[0]))
    for l in range(E.shape[0]):
        r = np.where(w, d - E[l] @ Cm, 0.0)
        sse[:, l] = (r * r).sum(axis=1)
    return dict(sse=sse, n=w.sum(axis=1).astype(np.float64))


def ls_derived(rec, assigned=None):
    """The scores of level_scores() / InsiderData.level_scores() (``sse`` n x L, ``n``) plus, per sample,
        mse = sse / n                                  (NaN where n = 0),
        best, second                                   the 1-based levels of the smallest and second smallest sse, ties to
                                                       the lowest id; 0 where n = 0 (second also 0 when L = 1),
        margin = (sse[assigned] - sse[best]) / sse[assigned]   (0 when the assigned level is best or ties with the best —
                                                       also when both are 0 — NaN where n = 0 or without ``assigned``),
        flagged = best != assigned                     (False where n = 0 or without ``assigned``),
        confusion                                      L x L counts, assigned x best, over the samples with n > 0 (None
                                                       without ``assigned``).
    ``assigned`` holds the 1-based ids of the scored covariate's column (length n), or None when the candidates are foreign
    embeddings.  A sample's own level was fitted WITH that sample, so on the entries the fit used the assigned level is
    favoured (a level with one sample fits itself); nothing here corrects for that."""
    sse = np.asarray(rec["sse"], dtype=np.float64)
    cnt = np.asarray(rec["n"], dtype=np.float64)
    n, L = sse.shape
    live = cnt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = sse / np.where(live, cnt, np.nan)[:, None]
    order = np.argsort(sse, axis=1, kind="stable")          # stable: ties to the lowest id
    best = np.where(live, order[:, 0] + 1, 0).astype(np.int64)
    second = np.where(live, order[:, 1] + 1, 0).astype(np.int64) if L > 1 else np.zeros(n, dtype=np.int64)
    out = dict(sse=sse, n=cnt, mse=mse, best=best, second=second)
    if assigned is None:
        out.update(margin=np.full(n, np.nan), flagged=np.zeros(n, dtype=bool), confusion=None)
        return out
    ids = np.asarray(assigned).ravel().astype(np.int64)
    if ids.shape != (n,) or (n and (ids.min() < 1 or ids.max() > L)):
        raise ValueError(f"assigned must hold n = {n} level ids within 1..{L}")
    rows = np.arange(n)
    own, low = sse[rows, ids - 1], sse[rows, np.maximum(best, 1) - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where((best == ids) | (own <= low), 0.0, (own - low) / np.where(own > low, own, 1.0))
    out["margin"] = np.where(live, margin, np.nan)
    out["flagged"] = live & (best != ids)
    conf = np.zeros((L, L), dtype=np.int64)
    np.add.at(conf, (ids[live] - 1, best[live] - 1), 1)
    out["confusion"] = conf
    return out


def level_scores(obj, cov, which="fit", entries="train", candidates=None):
    """Every sample of a fitted ``Insider`` object scored against every level of covariate column ``cov`` (0-based column of
    obj["confounder"]) on the device, with the ``which`` / ``entries`` of variance_decomposition(): is each sample's label
    right, and what should a sample with a placeholder label be called?  ``candidates`` (L x K): score against those
    embeddings instead of the covariate's own.  -> ls_derived() of the scores against the column's ids (against None with
    ``candidates``): sse, mse (n x L), n, best, second, margin, flagged (n), confusion (L x L).
    A sample's own level was fitted WITH that sample: on which="fit" / entries="train" the assigned level is favoured, most
    for levels with few samples (a level with one sample fits itself); which="tune", entries="test" scores on held-out
    entries no embedding has seen.  Nothing is reported or corrected for it."""
    ds, cfd, col, inc = _fitted(obj, which)
    rec = ds.level_scores(cfd, col, int(cov), entries=entries, candidates=candidates, inc_continuous=inc)
    return ls_derived(rec, None if candidates is not None else np.asarray(obj["confounder"])[:, int(cov)])


def residual_center_scale(rec):
    """Per-gene mean and standard deviation of the residual r = x - f over S_j, from the raw sums of a variance
    decomposition (InsiderData.variance_decomposition / variance_decomposition_host):
        center = (sum_x - sum_b sum_g_b) / n,   scale = sqrt((rss - n center^2) / (n - 1)).
    A gene with n < 2 gets a NaN scale (and with n = 0 a NaN center): outliers() gives it no call.  -> (center, scale)."""
    n = np.asarray(rec["n"], dtype=np.float64)
    sum_r = np.asarray(rec["sum_x"], dtype=np.float64) - np.asarray(rec["sum_g"], dtype=np.float64).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        center = sum_r / np.where(n > 0, n, np.nan)
        var = (np.asarray(rec["rss"], dtype=np.float64) - n * center * center) / np.where(n > 1, n - 1.0, np.nan)
        scale = np.sqrt(np.maximum(var, 0.0))
    return center, scale


def outliers_host(X, levels, ctns, mask, A, C, center, scale, threshold):
    """The outlier calls in plain numpy (the yardstick of InsiderData.outliers); X, levels, ctns, mask, A, C as in
    variance_decomposition_host(), ``center`` (None = 0) and ``scale`` of length p.  An entry that counts is a call when
    |z| >= threshold, z = (x - f - center[j]) / scale[j], f the sum of the blocks in block order; a gene whose scale is not
    finite or not > 0 has none.  -> dict of rows, cols (int32), z in ascending gene, then ascending sample, total, and the
    counts gene_low, gene_high (p), sample_low, sample_high (n) (low: z < 0, high: z > 0)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Cm = np.asarray(C, dtype=np.float64)
    lev = np.asarray(levels).reshape(n, -1)
    c = lev.shape[1]
    f = np.zeros_like(X)
    for b in range(c):
        f = f + np.asarray(A[b], dtype=np.float64)[lev[:, b].astype(np.int64) - 1] @ Cm
    if ctns is not None:
        f = f + np.asarray(ctns, dtype=np.float64).reshape(n, -1) @ (np.asarray(A[c], dtype=np.float64) @ Cm)
    sc = np.asarray(scale, dtype=np.float64).ravel()
    ce = np.zeros(p) if center is None else np.asarray(center, dtype=np.float64).ravel()
    usable = np.isfinite(sc) & (sc > 0)
    w = np.ones(X.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((X - f) - ce) / sc
        call = w & usable[None, :] & (np.abs(z) >= threshold)
    cols, rows = np.nonzero(call.T)                       # gene-major: ascending gene, then ascending sample
    low, high = call & (z < 0), call & (z > 0)
    return dict(rows=rows.astype(np.int32), cols=cols.astype(np.int32), z=z[rows, cols], total=int(call.sum()),
                gene_low=low.sum(axis=0).astype(np.int32), gene_high=high.sum(axis=0).astype(np.int32),
                sample_low=low.sum(axis=1).astype(np.int32), sample_high=high.sum(axis=1).astype(np.int32))


def outliers(obj, which="fit", entries="train", threshold=3.0, center=None, scale=None, cap=None):
    """The aberrant entries of a fitted ``Insider`` object on the device, with the ``which`` / ``entries`` of
    variance_decomposition().  ``center`` / ``scale`` (length p) not given: variance_decomposition() runs on the same entries
    first and residual_center_scale() supplies each gene's residual mean and standard deviation.  -> the dict of
    InsiderData.outliers() (rows, cols, z, total, gene_low, gene_high, sample_low, sample_high) plus the ``center`` and
    ``scale`` that were used."""
    ds, cfd, col, inc = _fitted(obj, which)
    if center is None or scale is None:
        ce, sc = residual_center_scale(ds.variance_decomposition(cfd, col, entries=entries, inc_continuous=inc))
        center = ce if center is None else center
        scale = sc if scale is None else scale
    out = ds.outliers(cfd, col, scale, center=center, threshold=threshold, entries=entries, inc_continuous=inc, cap=cap)
    out["center"], out["scale"] = np.asarray(center, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    return out


# ---- hidden factors: the leading components of the masked residual ------------------------------------------------------------
def residual_products_host(X, levels, ctns, mask, A, C, Q, center=None, scale=None):
    """The residual products in plain numpy (the yardstick of InsiderData.residual_products); X, levels, ctns, mask, A, C as
    in variance_decomposition_host(), ``Q`` n x q, ``center`` (None = 0) and ``scale`` (None = 1) of length p.  The direct
    form: r = ((x - f) - center[j]) / scale[j] on the entries that count and 0 elsewhere, f the sum of the blocks in block
    order; a gene whose scale is not finite or not > 0 is an all-zero column.  -> dict(Z = r'Q (p x q), Y = r Z (n x q),
    rss (p))."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be an n x p matrix")
    n, p = X.shape
    Qm = np.asarray(Q, dtype=np.float64)
    if Qm.ndim == 1:
        Qm = Qm.reshape(-1, 1)
    if Qm.ndim != 2 or Qm.shape[0] != n or not 1 <= Qm.shape[1] <= 64:
        raise ValueError(f"Q must be n x q with n = {n} and q in 1..64")
    if not np.all(np.isfinite(Qm)):
        raise ValueError("Q holds a value that is not finite")
    sc = np.ones(p) if scale is None else np.asarray(scale, dtype=np.float64).ravel()
    ce = np.zeros(p) if center is None else np.asarray(center, dtype=np.float64).ravel()
    if sc.shape != (p,) or ce.shape != (p,):
        raise ValueError(f"center and scale must hold p = {p} values")
    Cm = np.asarray(C, dtype=np.float64)
    lev = np.asarray(levels).reshape(n, -1)
    c = lev.shape[1]
    f = np.zeros_like(X)
    for b in range(c):
        f = f + np.asarray(A[b], dtype=np.float64)[lev[:, b].astype(np.int64) - 1] @ Cm
    if ctns is not None:
        f = f + np.asarray(ctns, dtype=np.float64).reshape(n, -1) @ (np.asarray(A[c], dtype=np.float64) @ Cm)
    usable = np.isfinite(sc) & (sc > 0)
    w = np.ones(X.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(w & usable[None, :], ((X - f) - ce) / sc, 0.0)
    Z = r.T @ Qm
    return dict(Z=Z, Y=r @ Z, rss=(r * r).sum(axis=0))


def _rc_check(r, oversample, max_iter, tol, seed):
    for name, v, low in (("r", r, 1), ("oversample", oversample, 0), ("max_iter", max_iter, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
            raise ValueError(f"{name} must be an integer >= {low}, got {v!r}")
    if r > 64:
        raise ValueError("r must be at most 64 (the block of one operator application)")
    if not (isinstance(tol, (int, float, np.floating)) and np.isfinite(tol) and tol > 0):
        raise ValueError(f"tol must be finite and > 0, got {tol!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError(f"seed must be a non-negative integer, got {seed!r}")


def component_signs(U):
    """The sign convention of the components: +1 / -1 per column of U so that, multiplied by it, the column's entry of largest
    magnitude is positive (equal magnitudes: the entry of lowest index decides)."""
    U = np.asarray(U, dtype=np.float64)
    lead = np.argmax(np.abs(U), axis=0)                               # (the first of equal magnitudes: the lowest index)
    return np.where(U[lead, np.arange(U.shape[1])] < 0, -1.0, 1.0)


def residual_components_driver(apply, n, r=5, oversample=8, max_iter=30, tol=1e-10, seed=0x1D5EED):
    """The block subspace iteration behind residual_components() and residual_components_host(), written once against the
    operator ``apply(Q) -> dict(Z = R'Q, Y = R Z, rss)``.  Block size q = min(r + oversample, 64, n) (r itself is clamped to
    q); Q0 = qr(gaussian(n, q)) from numpy.random.default_rng(seed); each pass applies the operator, takes svd(Z') = W S V'
    — with Q orthonormal, R ~ Q Q'R = (Q W) S V' — and sets U = Q W, sv, V, then Q <- qr(Y).  It stops when the largest
    relative change of the top-r singular values between two passes is below ``tol`` (converged), or after ``max_iter``
    passes.  Sign: each component's entry of U with the largest magnitude is positive (ties: the lowest index).
    -> dict(sv (r), sample_scores = U sv (n x r), gene_loadings = V (p x r), share = sv^2 / sum(rss), iters, converged,
    last_change (inf after a single pass))."""
    _rc_check(r, oversample, max_iter, tol, seed)
    n = int(n)
    q = max(1, min(int(r) + int(oversample), 64, n))
    r = min(int(r), q)
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, q)))[0]
    prev, change, converged, iters = None, np.inf, False, 0
    while iters < max_iter:
        out = apply(np.asfortranarray(Q))
        iters += 1
        Z = np.asarray(out["Z"], dtype=np.float64)
        W, sv, Vt = np.linalg.svd(Z.T, full_matrices=False)
        if prev is not None:
            top = sv[:r]
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(top > 0, np.abs(top - prev[:r]) / top, np.where(prev[:r] > 0, np.inf, 0.0))
            change = float(rel.max())
            if change < tol:
                converged = True
                break
        prev = sv
        if iters < max_iter:
            Q = np.linalg.qr(np.asarray(out["Y"], dtype=np.float64))[0]
    U, V = (Q @ W)[:, :r], Vt[:r].T
    sign = component_signs(U)
    U, V = U * sign, V * sign
    total = float(np.sum(out["rss"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = sv[:r] ** 2 / total
    return dict(sv=sv[:r].copy(), sample_scores=U * sv[:r], gene_loadings=V, share=share, iters=iters, converged=converged,
                last_change=change)


def residual_components_host(X, levels, ctns, mask, A, C, r=5, standardize=False, oversample=8, max_iter=30, tol=1e-10,
                             seed=0x1D5EED):
    """residual_components() in plain numpy (the yardstick of the device path): residual_components_driver() on
    residual_products_host(); X, levels, ctns, mask, A, C as in variance_decomposition_host().  standardize=True takes each
    gene's centre and scale from residual_center_scale() of the host variance decomposition under the same mask."""
    _rc_check(r, oversample, max_iter, tol, seed)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be an n x p matrix")
    center = scale = None
    if standardize:
        center, scale = residual_center_scale(_decomposition_host(X, levels, ctns, mask, A, C, 0))
    return residual_components_driver(lambda Q: residual_products_host(X, levels, ctns, mask, A, C, Q, center, scale),
                                      X.shape[0], r, oversample, max_iter, tol, seed)


def residual_components_resident(ds, cfd_factors, column_factor, inc_continuous=0, r=5, entries="train", standardize=False,
                                 oversample=8, max_iter=30, tol=1e-10, seed=0x1D5EED):
    """residual_components() on a resident data set and explicit factors (the command line's entry):
    residual_components_driver() on InsiderData.residual_products."""
    _rc_check(r, oversample, max_iter, tol, seed)
    if entries not in ds.VD_ENTRIES:
        raise ValueError(f"entries must be one of {sorted(ds.VD_ENTRIES)}, got {entries!r}")
    center = scale = None
    if standardize:
        center, scale = residual_center_scale(ds.variance_decomposition(cfd_factors, column_factor, entries=entries,
                                                                        inc_continuous=inc_continuous))
    return residual_components_driver(
        lambda Q: ds.residual_products(cfd_factors, column_factor, Q, entries=entries, center=center, scale=scale,
                                       inc_continuous=inc_continuous), ds.n, r, oversample, max_iter, tol, seed)


def residual_components(obj, r=5, which="fit", entries="train", standardize=False, oversample=8, max_iter=30, tol=1e-10,
                        seed=0x1D5EED):
    """The hidden factors of a fitted ``Insider`` object: the r leading singular directions of its masked residual
    R = M .* (X - fit) on the device, with the ``which`` / ``entries`` of variance_decomposition().  standardize=True centres
    and scales every gene's residual first (residual_center_scale() of a variance decomposition on the same entries), so
    that a few high-variance genes do not own the leading components.  A block subspace iteration
    (residual_components_driver) whose two thin products per step, R'Q and R Z, are streaming passes over the resident X:
    the residual never exists, on the device or the host.  -> dict(sv, sample_scores (n x r), gene_loadings (p x r), share
    (of the residual sum of squares), iters, converged, last_change); component_associations() relates the scores to the
    known covariates."""
    _rc_check(r, oversample, max_iter, tol, seed)
    if entries not in ("all", "train", "test"):
        raise ValueError(f"entries must be one of ['all', 'test', 'train'], got {entries!r}")
    ds, cfd, col, inc = _fitted(obj, which)
    return residual_components_resident(ds, cfd, col, inc, r, entries, standardize, oversample, max_iter, tol, seed)


def component_associations(sample_scores, levels, ctns=None):
    """How much of every component the known covariates explain, on the host: row b < c holds eta-squared of the r columns of
    ``sample_scores`` (n x r) on categorical covariate b (between-level over total sum of squares about the mean), and with
    ``ctns`` (n x m) a last row holds R-squared of the least-squares fit on [1, ctns].  A component tied to a known
    covariate points at misfit or a missing interaction, one tied to none at an unknown factor.  A constant component
    gives NaN.  -> (B x r)."""
    S = np.asarray(sample_scores, dtype=np.float64)
    if S.ndim == 1:
        S = S.reshape(-1, 1)
    if S.ndim != 2:
        raise ValueError("sample_scores must be n x r")
    n = S.shape[0]
    lev = np.asarray(levels)
    if lev.ndim < 1 or lev.ndim > 2 or lev.shape[0] != n or lev.size == 0:
        raise ValueError(f"levels must hold n = {n} rows")
    lev = lev.reshape(n, -1)
    dev = S - S.mean(axis=0)
    tss = (dev * dev).sum(axis=0)
    rows = []
    for b in range(lev.shape[1]):
        ids = np.unique(lev[:, b], return_inverse=True)[1].ravel()
        cnt = np.bincount(ids).astype(np.float64)
        sums = np.zeros((cnt.size, S.shape[1]))
        np.add.at(sums, ids, dev)
        rows.append((sums * sums / cnt[:, None]).sum(axis=0))
    if ctns is not None:
        Zc = np.asarray(ctns, dtype=np.float64)
        if Zc.shape[0] != n:
            raise ValueError(f"ctns must hold n = {n} rows")
        D = np.column_stack([np.ones(n), Zc.reshape(n, -1)])
        res = dev - D @ np.linalg.lstsq(D, dev, rcond=None)[0]
        rows.append(tss - (res * res).sum(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array(rows).reshape(len(rows), S.shape[1]) / np.where(tss > 0, tss, np.nan)


def neighbors_host(query, base=None, k=10, metric="cosine", exclude_self=None, device=0, chunk=512):
    """api.neighbors() in plain numpy (the yardstick of the device path): the same arguments, checks and result.  Scores are
    float64, q.b or q.b / (|q| |b|); per query the eligible base columns are ordered by np.lexsort on (index, -score):
    descending score, equal scores (-0.0 == 0.0) by ascending index.  Not eligible: the query's own column under
    exclude_self and, under cosine, zero-norm base columns; a zero-norm query has no candidate at all.  Rows with fewer than
    k candidates end in -1 / NaN.  Queries are taken ``chunk`` at a time: no nq x nb array is formed (``device`` is accepted
    for the common signature and not used)."""
    from . import api
    Q, B, k, code, off = api.neighbor_args(query, base, k, metric, exclude_self)
    nq, nb = Q.shape[1], B.shape[1]
    index = np.full((nq, k), -1, dtype=np.int32)
    score = np.full((nq, k), np.nan)
    ids = np.arange(nb)
    nrm_b = np.sqrt((B * B).sum(axis=0))
    for c0 in range(0, nq, chunk):
        Qc = Q[:, c0:c0 + chunk]
        S = Qc.T @ B
        ok = np.ones(S.shape, dtype=bool)
        if code == 0:
            nrm_q = np.sqrt((Qc * Qc).sum(axis=0))
            with np.errstate(divide="ignore", invalid="ignore"):
                S = S / (nrm_q[:, None] * nrm_b[None, :])
            ok &= (nrm_q > 0)[:, None] & (nrm_b > 0)[None, :]
        if off >= 0:
            own = off + c0 + np.arange(Qc.shape[1])
            ok[np.arange(Qc.shape[1]), own] = False
        for i in range(Qc.shape[1]):
            cand = ids[ok[i]]
            sc = S[i, cand] + 0.0                                   # (-0.0 + 0.0 = 0.0: one zero for the sort key)
            order = np.lexsort((cand, -sc))[:k]
            index[c0 + i, :order.size] = cand[order]
            score[c0 + i, :order.size] = sc[order]
    return dict(index=index, score=score)


# ---- residual co-expression: the top-k correlated partners of deep vectors -----------------------------------------------------
def _gram_standardise(R, sel, code):
    """The device's standardisation of the columns of ``R`` (depth x N) in numpy, every sum in index order (np.cumsum runs
    sequentially, np.sum would not): ``code`` 0 centres the selected entries (``sel``: a boolean depth x N array, None = all) by
    their mean and divides by the root of the centred sum of squares, 1 divides by the root of the sum of squares, 2 copies.
    Unselected entries are 0.  -> (the standardised matrix, alive (N,) bool): a column with fewer than two selected entries
    (code 0) or a sum of squares that is not > 0 is dead and all zero."""
    R = np.asarray(R, dtype=np.float64)
    depth, N = R.shape
    sel = np.ones(R.shape, dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    if code == 2:
        return np.where(sel, R, 0.0), np.ones(N, dtype=bool)
    Rz = np.where(sel, R, 0.0)
    m = sel.sum(axis=0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.cumsum(Rz, axis=0)[-1] / m if code == 0 else np.zeros(N)
        cen = np.where(sel, Rz - mean[None, :], 0.0)
        ss = np.cumsum(cen * cen, axis=0)[-1]
        alive = (ss > 0) & ((m >= 2) if code == 0 else True)
        out = np.where(alive[None, :], cen / np.sqrt(ss)[None, :], 0.0)
    return out, alive


def _gram_select(W, alive, k, first, count, chunk):
    """The selection of neighbors_host() on the scores W' W of the standardised columns ``W``: per query of the window the
    alive columns other than itself by descending score, equal scores (-0.0 == 0.0) by ascending index; a dead query has none."""
    N = W.shape[1]
    index = np.full((count, k), -1, dtype=np.int32)
    score = np.full((count, k), np.nan)
    ids = np.arange(N)
    for c0 in range(first, first + count, chunk):
        c1 = min(c0 + chunk, first + count)
        S = W[:, c0:c1].T @ W
        for i in range(c1 - c0):
            if not alive[c0 + i]:
                continue
            ok = alive.copy()
            ok[c0 + i] = False
            cand = ids[ok]
            sc = S[i, cand] + 0.0                                   # (-0.0 + 0.0 = 0.0: one zero for the sort key)
            order = np.lexsort((cand, -sc))[:k]
            index[c0 + i - first, :order.size] = cand[order]
            score[c0 + i - first, :order.size] = sc[order]
    return dict(index=index, score=score)


def gram_topk_host(V, k=10, metric="correlation", first=0, count=None, chunk=512):
    """api.gram_topk() in plain numpy (the yardstick of the device path): the same arguments, checks and result.  float64, the
    device's standardisation with its sums in index order (_gram_standardise), scores W' W of the standardised vectors taken
    ``chunk`` queries at a time (no N x N array is formed) and the selection of neighbors_host()."""
    from . import api
    V, k, code, first, count = api.gram_topk_args(V, k, metric, first, count)
    W, alive = _gram_standardise(V, None, code)
    return _gram_select(W, alive, k, first, count, chunk)


def _pairwise_sums(Z, M, alive, min_overlap, c0, c1):
    """The pairwise-complete score of the queries c0 .. c1 - 1 against every vector (include/insider_hip.h,
    insider_hip_gram_topk_pairwise): ``Z`` (depth x N) the standardised vectors, 0 where unselected, ``M`` the selection as
    0 / 1 doubles.  -> dict of (c1 - c0) x N arrays: score, eligible, N (int64) and the six sums' va, vb, Saa, Sbb."""
    depth = Z.shape[0]
    floor = 16.0 * (depth + 8) * 2.0 ** -52
    Zc, Mc, Q = Z[:, c0:c1], M[:, c0:c1], Z * Z
    N = Mc.T @ M
    Sab, Sa, Sb, Saa, Sbb = Zc.T @ Z, Zc.T @ M, Mc.T @ Z, Q[:, c0:c1].T @ M, Mc.T @ Q
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = Sab - Sa * Sb / N
        va = Saa - Sa * Sa / N
        vb = Sbb - Sb * Sb / N
        score = cov / np.sqrt(va * vb)
    own = np.arange(c0, c1)[:, None] == np.arange(Z.shape[1])[None, :]
    eligible = (alive[c0:c1, None] & alive[None, :] & ~own & (N >= min_overlap) & (va > floor * Saa) & (vb > floor * Sbb))
    return dict(score=score, eligible=eligible, N=np.rint(N).astype(np.int64), va=va, vb=vb, Saa=Saa, Sbb=Sbb)


def _gram_select_pairwise(R, sel, k, min_overlap, first, count, chunk):
    """The pairwise-complete selection on the columns of ``R`` (depth x N) with the boolean selection ``sel``: every vector
    standardised over its own selected entries first (_gram_standardise), the six sums over the joint entries, the eligible
    partners of every query of the window by descending score, equal scores (-0.0 == 0.0) by ascending index."""
    Z, alive = _gram_standardise(R, sel, 0)
    M = (np.asarray(sel, dtype=bool) & alive[None, :]).astype(np.float64)
    index = np.full((count, k), -1, dtype=np.int32)
    score = np.full((count, k), np.nan)
    overlap = np.full((count, k), -1, dtype=np.int32)
    ids = np.arange(Z.shape[1])
    for c0 in range(first, first + count, chunk):
        c1 = min(c0 + chunk, first + count)
        t = _pairwise_sums(Z, M, alive, min_overlap, c0, c1)
        for i in range(c1 - c0):
            cand = ids[t["eligible"][i]]
            sc = t["score"][i, cand] + 0.0                          # (-0.0 + 0.0 = 0.0: one zero for the sort key)
            order = np.lexsort((cand, -sc))[:k]
            index[c0 + i - first, :order.size] = cand[order]
            score[c0 + i - first, :order.size] = sc[order]
            overlap[c0 + i - first, :order.size] = t["N"][i, cand[order]]
    return dict(index=index, score=score, overlap=overlap)


def gram_topk_pairwise_host(V, k=10, min_overlap=None, first=0, count=None, chunk=512):
    """api.gram_topk_pairwise() in plain numpy (the yardstick of the device path): the same arguments, checks, definition
    (standardise first, the six sums, the variance floor 16 (depth + 8) 2^-52) and result."""
    from . import api
    V, k, min_overlap, first, count = api.gram_topk_pairwise_args(V, k, min_overlap, first, count)
    sel = ~np.isnan(V)
    return _gram_select_pairwise(np.where(sel, V, 0.0), sel, k, min_overlap, first, count, chunk)


def coexpression_residual_host(X, levels, ctns, mask, A, C, center=None, scale=None):
    """The working residual of coexpression_host() and the entries that count: r = ((x - f) - center[j]) / scale[j], f the
    sum of the blocks in block order (residual_products_host()'s definition); a gene whose scale is not finite or not > 0 is
    an all-zero column whose entries still count.  -> (r (n x p, 0 where the mask is off), selected (n x p bool))."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be an n x p matrix")
    n, p = X.shape
    sc = np.ones(p) if scale is None else np.asarray(scale, dtype=np.float64).ravel()
    ce = np.zeros(p) if center is None else np.asarray(center, dtype=np.float64).ravel()
    if sc.shape != (p,) or ce.shape != (p,):
        raise ValueError(f"center and scale must hold p = {p} values")
    Cm = np.asarray(C, dtype=np.float64)
    lev = np.asarray(levels).reshape(n, -1)
    c = lev.shape[1]
    f = np.zeros_like(X)
    for b in range(c):
        f = f + np.asarray(A[b], dtype=np.float64)[lev[:, b].astype(np.int64) - 1] @ Cm
    if ctns is not None:
        f = f + np.asarray(ctns, dtype=np.float64).reshape(n, -1) @ (np.asarray(A[c], dtype=np.float64) @ Cm)
    usable = np.isfinite(sc) & (sc > 0)
    w = np.ones(X.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(w & usable[None, :], ((X - f) - ce) / sc, 0.0)
    return r, w


def coexpression_host(X, levels, ctns, mask, A, C, axis, k, center=None, scale=None, chunk=512, missing="zero",
                      min_overlap=None):
    """InsiderData.coexpression() in plain numpy (the yardstick of the device path); X, levels, ctns, mask, A, C, center and
    scale as in residual_products_host(), ``axis`` "genes" (the p columns of the residual, correlated over the samples) or
    "samples" (its n rows, over the genes).  Every vector is centred by its mean over its selected entries (unselected stay
    0) and divided by the root of its centred sum of squares; fewer than two selected entries or no variance: dead.  The
    score is the plain sum of products over the whole depth: Pearson's r under a full selection, the zero-filled correlation
    (NOT the pairwise-complete one) under a mask.  -> dict(index=(N, k) int32, score=(N, k)), the order and open slots of
    neighbors_host().  missing="pairwise": InsiderData.coexpression_pairwise() instead, the pairwise-complete score of
    gram_topk_pairwise_host() on the same standardised vectors with ``min_overlap`` (None = max(3, ceil(depth / 4))), and an
    ``overlap`` (N, k) int32 in the result."""
    if axis not in ("genes", "samples"):
        raise ValueError(f"axis must be 'genes' or 'samples', got {axis!r}")
    if missing not in COEXPR_MISSING:
        raise ValueError(f"missing must be one of {COEXPR_MISSING}, got {missing!r}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 64:
        raise ValueError("k must be an integer in 1..64")
    r, w = coexpression_residual_host(X, levels, ctns, mask, A, C, center, scale)
    if axis == "samples":
        r, w = r.T, w.T
    if missing == "pairwise":
        from . import api
        return _gram_select_pairwise(r, w, int(k), api.pairwise_min_overlap(min_overlap, r.shape[0]), 0, r.shape[1], chunk)
    W, alive = _gram_standardise(r, w, 0)
    return _gram_select(W, alive, int(k), 0, W.shape[1], chunk)


COEXPR_MISSING = ("zero", "pairwise")


def _coexpression(ds, cfd, col, axis, k, entries, inc, missing, min_overlap, **kw):
    """ds.coexpression() (missing="zero": min_overlap must be None) or ds.coexpression_pairwise() (missing="pairwise")."""
    if missing not in COEXPR_MISSING:
        raise ValueError(f"missing must be one of {COEXPR_MISSING}, got {missing!r}")
    if missing == "pairwise":
        return ds.coexpression_pairwise(cfd, col, axis=axis, k=k, min_overlap=min_overlap, entries=entries, inc_continuous=inc,
                                        **kw)
    if min_overlap is not None:
        raise ValueError('min_overlap belongs to missing="pairwise"')
    return ds.coexpression(cfd, col, axis=axis, k=k, entries=entries, inc_continuous=inc, **kw)


def gene_coexpression(obj, k=10, which="fit", entries="train", missing="zero", min_overlap=None):
    """The k most correlated genes of every gene in the residual of a fitted ``Insider`` object (InsiderData.coexpression,
    axis "genes"), with the ``which`` / ``entries`` of variance_decomposition(): the co-expression network on corrected
    expression.  The correlation of two genes does not depend on their scales, so no centre or scale is passed.
    missing="zero": missing entries make it the zero-filled correlation; missing="pairwise": the pairwise-complete one
    (InsiderData.coexpression_pairwise) over the samples both genes have, at least ``min_overlap`` of them (None =
    max(3, ceil(n / 4))), with an ``overlap`` (p, k) int32 in the result.  -> dict(index=(p, k) int32 0-based genes,
    score=(p, k)); open slots -1 / NaN."""
    ds, cfd, col, inc = _fitted(obj, which)
    return _coexpression(ds, cfd, col, "genes", k, entries, inc, missing, min_overlap)


def sample_coexpression(obj, k=10, which="fit", entries="train", standardize=True, missing="zero", min_overlap=None):
    """The k most correlated samples of every sample in the residual of a fitted ``Insider`` object (InsiderData.coexpression,
    axis "samples"): duplicated libraries, cross-contamination, relatedness.  standardize=True centres and scales every
    gene's residual first (residual_center_scale() of a variance decomposition on the same entries), so that a few
    high-variance genes do not own the sample correlation.  ``missing`` / ``min_overlap`` as in gene_coexpression(): the
    zero-filled correlation by default, the pairwise-complete one (and an ``overlap``) with "pairwise".
    -> dict(index=(n, k) int32 0-based samples, score=(n, k)) plus the ``center`` and ``scale`` used (None without
    standardize)."""
    ds, cfd, col, inc = _fitted(obj, which)
    center = scale = None
    if standardize:
        center, scale = residual_center_scale(ds.variance_decomposition(cfd, col, entries=entries, inc_continuous=inc))
    out = _coexpression(ds, cfd, col, "samples", k, entries, inc, missing, min_overlap, center=center, scale=scale)
    out["center"], out["scale"] = center, scale
    return out


def gene_neighbors(column_factor, k=10, metric="cosine", device=0):
    """The k nearest genes of every gene in the latent space: one api.neighbors() call on C (K x p) against itself, a gene
    never its own neighbour.  -> dict(index=(p, k) int32 0-based genes, score=(p, k)); open slots -1 / NaN (under cosine
    an all-zero column of C, which elastic-net fits do produce, has no neighbours and is nobody's)."""
    from . import api
    return api.neighbors(column_factor, None, k=k, metric=metric, device=device)


def sample_embeddings(cfd_factors, levels, ctns_confounder=None):
    """The K x n per-sample row embedding of a fit: column i is the sum over the covariates b of row levels[i, b] (1-based)
    of cfd_factors[b], plus ctns_confounder[i] @ cfd_factors[c] when the continuous block is given: the total block of
    factor_decomposition_host(), summed in block order."""
    lev = np.asarray(levels)
    lev = lev.reshape(lev.shape[0], -1)
    A = [np.asarray(a, dtype=np.float64) for a in cfd_factors]
    c = lev.shape[1]
    if len(A) != c + (0 if ctns_confounder is None else 1):
        raise ValueError(f"{len(A)} factor matrices for {c} covariates" + ("" if ctns_confounder is None else " + the continuous block"))
    tot = np.zeros((lev.shape[0], A[0].shape[1]))
    for b in range(c):
        ids = lev[:, b].astype(np.int64) - 1
        if ids.size and (ids.min() < 0 or ids.max() >= A[b].shape[0]):
            raise ValueError(f"level ids of covariate {b} must be within 1..{A[b].shape[0]}")
        tot = tot + A[b][ids]
    if ctns_confounder is not None:
        tot = tot + np.asarray(ctns_confounder, dtype=np.float64).reshape(lev.shape[0], -1) @ A[c]
    return np.asfortranarray(tot.T)


def sample_neighbors(cfd_factors, levels, ctns_confounder=None, k=10, metric="cosine", device=0):
    """The k nearest samples of every sample: api.neighbors() on sample_embeddings() against itself.  Samples that share
    every level have equal embeddings: they tie, and ties list by ascending sample.  -> dict(index=(n, k) int32 0-based
    samples, score=(n, k)); open slots -1 / NaN."""
    from . import api
    return api.neighbors(sample_embeddings(cfd_factors, levels, ctns_confounder), None, k=k, metric=metric, device=device)


# ---- gene-set enrichment (include/insider_hip.h states the definitions) ----------------------------------------------------
def _h32(x):
    """insider_h32 (include/insider_perm.h) on a uint32 array."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def gs_sample_host(seed, perm, m, p):
    """Null draw ``perm`` under ``seed``: phi(0 .. m - 1) on [0, p), the numpy mirror of include/insider_sample.h (uint32
    arithmetic that wraps; the Feistel network is walked until every value is below p).  -> int64 (m)."""
    half = 1
    while half < 16 and (1 << (2 * half)) < p:
        half += 1
    h, mask = np.uint32(half), np.uint32((1 << half) - 1)
    with np.errstate(over="ignore"):
        key = _h32(np.array([(seed & 0xFFFFFFFF) ^ 0x9E3779B9], dtype=np.uint32))
        key = _h32(key ^ np.uint32((seed >> 32) & 0xFFFFFFFF) ^ np.uint32((0x85EBCA6B * perm) & 0xFFFFFFFF))
        x = np.arange(m, dtype=np.uint32)
        todo = np.ones(m, dtype=bool)
        while todo.any():
            L, Rr = x[todo] >> h, x[todo] & mask
            for i in range(1, 9):
                t = L ^ (_h32(Rr ^ key ^ np.uint32((0xC2B2AE35 * i) & 0xFFFFFFFF)) & mask)
                L, Rr = Rr, t
            x[todo] = (L << h) | Rr
            todo = x >= p
    return x.astype(np.int64)


def gs_deviations(aw, T, weight):
    """The deviations of the position sets T (ascending; (m) for all profiles or (R, m) per profile) on the profiles whose
    |score| by rank position is aw (R x p): (P_i / N - miss_i / (p - m), P_{i-1} / N - miss_i / (p - m)), each R x m, every
    term in exactly that form; rows with N == 0 use w = 1."""
    R, p = aw.shape
    T = np.broadcast_to(T, (R, np.shape(T)[-1]))
    m = T.shape[1]
    i = np.arange(m)
    miss = (T - i).astype(np.float64) / float(p - m)
    if weight:
        P = np.cumsum(np.take_along_axis(aw, T, axis=1), axis=1)
        N = P[:, -1:].copy()
        zero = N[:, 0] == 0.0
        P[zero] = i + 1.0
        N[zero] = float(m)
    else:
        P = np.broadcast_to(i + 1.0, (R, m))
        N = float(m)
    Pprev = np.concatenate([np.zeros((R, 1)), P[:, :-1]], axis=1)
    return P / N - miss, Pprev / N - miss


def gs_pick(dh, dl, T):
    """(ES, peak) per row from the deviations: ES = hi if hi >= -lo else lo, peak the smallest position at the extreme."""
    T = np.broadcast_to(T, dh.shape)
    ihi, ilo = dh.argmax(axis=1), dl.argmin(axis=1)
    rows = np.arange(dh.shape[0])
    hi, lo = dh[rows, ihi], dl[rows, ilo]
    up = hi >= -lo
    return np.where(up, hi, lo), T[rows, np.where(up, ihi, ilo)].astype(np.int32)


def enrichment_host(scores, set_ptr, set_genes, nperm=1000, weight=1, seed=0x1D5EED, device=0, return_null=False):
    """api.enrichment() in plain numpy (the yardstick of the device path): the same arguments and record, vectorised over
    the profiles.  return_null: the record also holds ``null`` (R x distinct sizes x nperm, the score of every draw) and
    ``null_sizes`` (``device`` is accepted for the common signature and not used; the arguments are assumed valid)."""
    from . import api
    sc, ptr, genes, nperm, weight, seed = api.enrichment_args(scores, set_ptr, set_genes, nperm, weight, seed)
    R, p = sc.shape
    S = ptr.size - 1
    order = np.argsort(-sc, axis=1, kind="stable")                 # descending score, ties by ascending gene
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(p), (R, p)), axis=1)
    aw = np.abs(np.take_along_axis(sc, order, axis=1))
    size = np.diff(ptr).astype(np.int32)
    rec = dict(es=np.zeros((R, S)), sum_same=np.zeros((R, S)))
    for name in ("peak", "n_ge", "n_same", "hits_nonzero"):
        rec[name] = np.zeros((R, S), dtype=np.int32)
    for s in range(S):
        g = genes[ptr[s]:ptr[s + 1]]
        T = np.sort(rank[:, g], axis=1)
        rec["es"][:, s], rec["peak"][:, s] = gs_pick(*gs_deviations(aw, T, weight), T)
        rec["hits_nonzero"][:, s] = np.count_nonzero(sc[:, g], axis=1)
    usizes = np.unique(size)
    null = np.zeros((R, usizes.size, nperm))
    for b in range(nperm if S and R else 0):
        pos = gs_sample_host(seed, b, int(usizes[-1]), p)
        for z, m in enumerate(usizes):
            T = np.sort(pos[:m])
            null[:, z, b] = gs_pick(*gs_deviations(aw, T, weight), T)[0]
    for s in range(S):
        nb = null[:, np.searchsorted(usizes, size[s]), :]
        obs = rec["es"][:, s:s + 1]
        same = (nb >= 0.0) == (obs >= 0.0)
        rec["n_same"][:, s] = same.sum(axis=1)
        rec["n_ge"][:, s] = (same & (np.abs(nb) >= np.abs(obs))).sum(axis=1)
        total, comp = np.zeros(R), np.zeros(R)                     # a compensated (Neumaier) sum in draw order
        for b in range(nperm):
            e = np.where(same[:, b], nb[:, b], 0.0)
            t = total + e
            comp += np.where(np.abs(total) >= np.abs(e), (total - t) + e, (e - t) + total)
            total = t
        rec["sum_same"][:, s] = total + comp
    rec.update(size=size, nonzero=np.count_nonzero(sc, axis=1).astype(np.int64), nperm=nperm, weight=weight, seed=seed,
               scores=sc, set_ptr=ptr, set_genes=genes)
    if return_null:
        rec.update(null=null, null_sizes=usizes)
    return rec


def _hyper_tail(k, M, n, N):
    """P(X >= k), X hypergeometric: N draws without replacement from M genes of which n are marked (math.lgamma)."""
    import math
    lo, hi = max(k, 0, N - (M - n)), min(n, N)
    if lo > hi:
        return 0.0
    lc = lambda a, b: math.lgamma(a + 1) - math.lgamma(b + 1) - math.lgamma(a - b + 1)
    den = lc(M, N)
    return min(1.0, math.fsum(math.exp(lc(n, x) + lc(M - n, N - x) - den) for x in range(lo, hi + 1)))


def gs_derived(rec):
    """From an enrichment record: pval = (n_ge + 1) / (n_same + 1); nes = ES / (sum_same / n_same), NaN where no draw fell
    on the observed side; fdr = Benjamini-Hochberg over the sets of each profile; hyper_p = the hypergeometric upper tail of
    hits_nonzero among the set's genes against the profile's non-zero count (the over-representation test of a sparse
    factor's support).  All R x S."""
    es, n_same = rec["es"], rec["n_same"].astype(np.float64)
    R, S = es.shape
    pval = (rec["n_ge"] + 1.0) / (n_same + 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        nes = np.where(n_same > 0, es / (rec["sum_same"] / n_same), np.nan)
    fdr = np.ones((R, S))
    if S:
        o = np.argsort(pval, axis=1, kind="stable")
        q = np.take_along_axis(pval, o, axis=1) * S / np.arange(1, S + 1)
        q = np.minimum(np.minimum.accumulate(q[:, ::-1], axis=1)[:, ::-1], 1.0)
        np.put_along_axis(fdr, o, q, axis=1)
    p = rec["scores"].shape[1]
    hyper = np.array([[_hyper_tail(int(rec["hits_nonzero"][r, s]), p, int(rec["nonzero"][r]), int(rec["size"][s]))
                       for s in range(S)] for r in range(R)], dtype=np.float64).reshape(R, S)
    return dict(pval=pval, nes=nes, fdr=fdr, hyper_p=hyper)


def leading_edge(rec, r, s):
    """The genes of set s that make the score of profile r: those ranked at or before the peak when ES >= 0, at or after it
    otherwise, in rank order (int64 gene indices, 0-based)."""
    sc = rec["scores"][r]
    g = rec["set_genes"][rec["set_ptr"][s]:rec["set_ptr"][s + 1]].astype(np.int64)
    rank = np.empty(sc.size, dtype=np.int64)
    rank[np.argsort(-sc, kind="stable")] = np.arange(sc.size)
    t = rank[g]
    keep = t <= rec["peak"][r, s] if rec["es"][r, s] >= 0.0 else t >= rec["peak"][r, s]
    return g[keep][np.argsort(t[keep])]


def _enrich(profiles, sets, nperm, weight, seed, device):
    from . import api
    ptr, genes = sets[-2], sets[-1]                               # (set_ptr, set_genes) or flatio.read_gmt()'s triple
    rec = api.enrichment(profiles, ptr, genes, nperm=nperm, weight=weight, seed=seed, device=device)
    rec.update(gs_derived(rec))
    if len(sets) == 3:
        rec["names"] = list(sets[0])
    return rec


def factor_enrichment(column_factor, sets, abs=True, nperm=1000, weight=1, seed=0x1D5EED, device=0):
    """Gene-set enrichment of every factor's loadings: the profiles are the rows of column_factor (K x p).  abs=True ranks by
    |loading|: a factor's sign is arbitrary and, after the elastic net, most loadings are 0.  ``sets`` is
    (set_ptr, set_genes) or what flatio.read_gmt() returns.  -> the api.enrichment() record with gs_derived() merged in
    (K x S)."""
    Cm = np.asarray(column_factor, dtype=np.float64)
    return _enrich(np.abs(Cm) if abs else Cm, sets, nperm, weight, seed, device)


def level_enrichment(cfd_factor, column_factor, sets, nperm=1000, weight=1, seed=0x1D5EED, device=0):
    """Gene-set enrichment of every level's per-gene effect A_b[l] . C of one covariate: the profiles are the rows of
    cfd_factor (L x K) @ column_factor (K x p), signed.  -> as factor_enrichment(), L x S."""
    return _enrich(np.asarray(cfd_factor, dtype=np.float64) @ np.asarray(column_factor, dtype=np.float64), sets, nperm,
                   weight, seed, device)


# ---- k-means (include/insider_hip.h states the definitions) ------------------------------------------------------------------
def _sumsq(M):
    """The sum of squares of every column, taken in index order."""
    ss = np.zeros(M.shape[1])
    for d in range(M.shape[0]):
        ss = ss + M[d] * M[d]
    return ss


def kmeans_host(points, k, metric="cosine", init=None, restarts=8, max_iter=100, seed=0x1D5EED, device=0, chunk=4096,
                blas=False):
    """api.kmeans() in plain numpy float64 (the yardstick of the device path): the same arguments, checks and record, following
    the definitions of include/insider_hip.h line by line.  The record also holds ``score`` / ``score2`` (N: the best and the
    runner-up score of the last assignment, NaN for a dead point and for k = 1) and ``min_gap``: over every assignment of the
    returned restart, the smallest (best - runner-up) score of an alive point divided by the largest |best score| of that
    assignment (inf when k = 1): how far the run is from a tie that rounding could decide.  Points are scored ``chunk`` at a
    time; a score adds its D products in index order, so equal points and equal centres tie exactly and the tie rule decides
    (blas=True takes the matrix product instead: faster, and equal columns may then differ in the last bit).  A cluster's sum
    runs over its members in ascending index (``device`` is accepted for the common signature and not used; ``ms`` is the wall
    time)."""
    import time
    from . import api
    t_start = time.perf_counter()
    P, k, code, init, restarts, max_iter, seed = api.kmeans_args(points, k, metric, init, restarts, max_iter, seed)
    D, N = P.shape
    if code == 0:                                                   # working points: x = p / |p|, a zero column is dead
        nrm = np.sqrt(_sumsq(P))
        alive = nrm > 0
        X = np.where(alive, P / np.where(alive, nrm, 1.0), 0.0)
    else:
        X, alive = P, np.ones(N, dtype=bool)
    xx = _sumsq(X)
    ids = np.flatnonzero(alive)

    def assign(Cm):
        h = 0.5 * _sumsq(Cm) if code == 1 else np.zeros(k)
        label, second = np.full(N, -1, dtype=np.int32), np.full(N, -1, dtype=np.int32)
        s1, s2 = np.full(N, np.nan), np.full(N, np.nan)
        for c0 in range(0, N, chunk):
            Xc = X[:, c0:c0 + chunk]
            if blas:
                S = Xc.T @ Cm
            else:
                S = np.zeros((Xc.shape[1], k))
                for d in range(D):
                    S = S + Xc[d][:, None] * Cm[d][None, :]
            S = (S - h) + 0.0                                       # (-0.0 + 0.0 = 0.0: one zero)
            rows = np.arange(S.shape[0])
            l1 = S.argmax(axis=1)                                   # the first of equal scores: the lowest centre index
            label[c0:c0 + chunk], s1[c0:c0 + chunk] = l1, S[rows, l1]
            if k > 1:
                S[rows, l1] = -np.inf
                l2 = S.argmax(axis=1)
                second[c0:c0 + chunk], s2[c0:c0 + chunk] = l2, S[rows, l2]
        if code == 0:
            d1, d2 = 1.0 - s1, 1.0 - s2
        else:
            d1, d2 = np.maximum(0.0, xx - 2.0 * s1), np.where(np.isnan(s2), np.nan, np.maximum(0.0, xx - 2.0 * s2))
        label[~alive], second[~alive] = -1, -1
        d1[~alive], d2[~alive] = np.nan, np.nan
        gap = np.inf
        if k > 1 and ids.size:
            top = float(np.abs(s1[ids]).max())
            gap = float((s1[ids] - s2[ids]).min()) / top if top > 0 else 0.0
        s1[~alive], s2[~alive] = np.nan, np.nan
        return label, second, d1, d2, float(d1[ids].sum()), gap, s1, s2

    def update(Cm, label):
        Cm = Cm.copy(order="F")
        for j in range(k):
            members = X[:, label == j]                              # (dead points carry -1)
            if members.shape[1] == 0:
                continue                                            # an empty cluster keeps its centre
            tot = np.cumsum(members, axis=1)[:, -1]                 # (one after the other, in member order)
            den = float(members.shape[1]) if code == 1 else float(np.sqrt(_sumsq(tot[:, None]))[0])
            if den > 0.0:                                           # (cosine: a sum of norm 0 keeps the centre too)
                Cm[:, j] = tot / den
        return Cm

    runs = []
    for r in range(restarts):
        if init is not None:
            Cm = np.asfortranarray(init / np.sqrt(_sumsq(init)) if code == 0 else init.copy())
        else:
            Cm = np.asfortranarray(X[:, ids[gs_sample_host(seed, r, k, ids.size)]])
        traj = np.full(max_iter + 1, np.nan)
        label, second, d1, d2, traj[0], gap, s1, s2 = assign(Cm)
        t, conv = 0, 0
        while t < max_iter:
            Cm = update(Cm, label)
            new, second, d1, d2, J, g, s1, s2 = assign(Cm)
            t += 1
            traj[t], gap = J, min(gap, g)
            same = np.array_equal(new, label)
            label = new
            if same:
                conv = 1
                break
        runs.append(dict(centers=Cm, label=label, dist=d1, second=second, dist2=d2,
                         sizes=np.bincount(label[label >= 0], minlength=k).astype(np.int32), traj=traj, iters=t, converged=conv,
                         final=traj[t], min_gap=gap, score=s1, score2=s2))
    final = np.array([q["final"] for q in runs])
    best = int(np.argmin(final))                                    # (the first of equal minima: the lowest r)
    rec = {name: runs[best][name] for name in ("centers", "label", "dist", "second", "dist2", "sizes", "traj", "min_gap", "score",
                                               "score2")}
    rec.update(final_inertia=final, iters=np.array([q["iters"] for q in runs], dtype=np.int32),
               converged=np.array([q["converged"] for q in runs], dtype=np.int32), best=best,
               ms=(time.perf_counter() - t_start) * 1e3)
    return rec


def gene_modules(column_factor, k, metric="cosine", init=None, restarts=8, max_iter=100, seed=0x1D5EED, device=0):
    """Gene modules: api.kmeans() on the columns of C (K x p), genes with the same loading pattern share a module.  Under
    cosine (the default) an all-zero column of C, which elastic-net fits do produce, is dead: label -1, in no module.  -> the
    api.kmeans() record (label: p, 0-based modules)."""
    from . import api
    return api.kmeans(column_factor, k, metric=metric, init=init, restarts=restarts, max_iter=max_iter, seed=seed, device=device)


def sample_clusters(cfd_factors, levels, ctns_confounder=None, k=8, metric="cosine", init=None, restarts=8, max_iter=100,
                    seed=0x1D5EED, device=0):
    """Sample clusters: api.kmeans() on sample_embeddings().  Samples that share every level (and, with a continuous block,
    its values) are EQUAL points: they always fall into one cluster, and when two of them are drawn as starting centres the
    tie rule leaves the higher-indexed centre empty (size 0).  -> the api.kmeans() record (label: n)."""
    from . import api
    return api.kmeans(sample_embeddings(cfd_factors, levels, ctns_confounder), k, metric=metric, init=init, restarts=restarts,
                      max_iter=max_iter, seed=seed, device=device)


def assign_to_centers(points, centers, metric="cosine", device=0):
    """The points (D x N) assigned to given centres (D x k): the max_iter = 0 call of api.kmeans() (label, second, dist, dist2
    and sizes against ``centers``, normalised under cosine)."""
    from . import api
    Cm = np.asarray(centers, dtype=np.float64)
    if Cm.ndim != 2:
        raise api.InsiderError(api._lib.ERR_ARG, "centers must be a D x k array")
    return api.kmeans(points, int(Cm.shape[1]), metric=metric, init=Cm, restarts=1, max_iter=0, device=device)


# ---- t-SNE (include/insider_hip.h states the definitions) --------------------------------------------------------------------
TSNE_U = 2.0 ** -52


def tsne_draw_host(seed, N):
    """The drawn start of insider_hip_tsne (insider_tsne_draw, include/insider_sample.h) -> (N, 2) float64, to the bit."""
    with np.errstate(over="ignore"):
        key = _h32(np.array([(seed & 0xFFFFFFFF) ^ 0x9E3779B9], dtype=np.uint32))
        key = _h32(key ^ np.uint32((seed >> 32) & 0xFFFFFFFF))      # insider_sample_key(seed, 0)
        e = np.arange(2 * N, dtype=np.uint32)
        u = _h32(key ^ (np.uint32(0x27D4EB2F) * (e + np.uint32(1))))
    return ((((u.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)) - 0.5) * 1e-4).reshape(N, 2)


def tsne_calibrate_host(idx, d2, perplexity):
    """The calibration of every row: (beta (N), p_cond (N x k)); the 100 fixed steps, all rows at once, sums in slot order."""
    N, k = idx.shape
    filled = idx >= 0
    m = filled.sum(axis=1)
    d = np.where(filled, d2, np.inf)
    d = np.where(filled, d - np.where(m > 0, d.min(axis=1), 0.0)[:, None], 0.0)
    search = (m > 0) & (perplexity < m)
    target = np.log(perplexity)
    b, lo, hi = np.ones(N), np.zeros(N), np.full(N, np.inf)

    def sums(b):
        S, T = np.zeros(N), np.zeros(N)
        for s in range(k):
            e = np.where(filled[:, s], np.exp(-b * d[:, s]), 0.0)
            S, T = S + e, T + d[:, s] * e
        return S, T
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for _ in range(100):
            S, T = sums(b)
            up = np.log(S) + b * T / S > target
            lo, hi = np.where(up, b, lo), np.where(up, hi, b)
            b = np.where(up, np.where(np.isinf(hi), b * 2.0, (b + hi) * 0.5), (lo + b) * 0.5)
        b = np.where(search, b, 1.0)
        S, _ = sums(b)
        pc = np.where(filled, np.exp(-b[:, None] * d) / S[:, None], 0.0)
        pc = np.where(search[:, None], pc, np.where(filled, 1.0 / np.maximum(m, 1)[:, None], 0.0))
    return np.where(m > 0, b, 1.0), pc


def tsne_joint_host(idx, pc, n_alive):
    """The joint P as ordered pairs: (ii, jj, PP), every pair (i, j) with an edge in either direction once, and its mirror."""
    N = idx.shape[0]
    src, slot = np.nonzero(idx >= 0)
    dst = idx[src, slot].astype(np.int64)
    keys = np.concatenate([src * N + dst, dst * N + src])
    uniq, inv = np.unique(keys, return_inverse=True)
    PP = np.bincount(inv.ravel(), weights=np.concatenate([pc[src, slot]] * 2), minlength=uniq.size) / (2.0 * n_alive)
    return uniq // N, uniq % N, PP


def tsne_eval_host(Y, ii, jj, PP, alive, a=1.0, chunk=1024):
    """Z, KL, the gradient (N x 2, under exaggeration a) and the sums the error bound of the gradient is made of at the map Y
    (N x 2): dense O(N^2) repulsion, ``chunk`` rows at a time.  -> dict(z, kl, grad, attr_abs, rep_abs, rep, terms)."""
    N = Y.shape[0]
    ids = np.flatnonzero(alive)
    Ya = Y[ids]
    sw, rep, rep_abs = np.zeros(ids.size), np.zeros((ids.size, 2)), np.zeros((ids.size, 2))
    for c0 in range(0, ids.size, chunk):
        dx = Ya[c0:c0 + chunk, 0][:, None] - Ya[None, :, 0]
        dy = Ya[c0:c0 + chunk, 1][:, None] - Ya[None, :, 1]
        w = 1.0 / (1.0 + dx * dx + dy * dy)
        r = np.arange(dx.shape[0])
        w[r, c0 + r] = 0.0                                          # the self pair
        sw[c0:c0 + chunk] = w.sum(axis=1)
        w2 = w * w
        rep[c0:c0 + chunk, 0], rep[c0:c0 + chunk, 1] = (w2 * dx).sum(axis=1), (w2 * dy).sum(axis=1)
        rep_abs[c0:c0 + chunk, 0], rep_abs[c0:c0 + chunk, 1] = (w2 * np.abs(dx)).sum(axis=1), (w2 * np.abs(dy)).sum(axis=1)
    z = float(sw.sum())
    dlt = Y[ii] - Y[jj]
    d = 1.0 + dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]
    t = (PP / d)[:, None] * dlt
    attr = np.column_stack([np.bincount(ii, weights=t[:, c], minlength=N) for c in range(2)])
    attr_abs = np.column_stack([np.bincount(ii, weights=np.abs(t[:, c]), minlength=N) for c in range(2)])
    pos = PP > 0
    kl = float((PP[pos] * np.log(PP[pos] * z * d[pos])).sum())
    full = np.zeros((N, 2))
    full_abs = np.zeros((N, 2))
    full[ids], full_abs[ids] = rep, rep_abs
    grad = 4.0 * (a * attr - full / z)
    grad[~alive] = np.nan
    return dict(z=z, kl=kl, grad=grad, attr_abs=a * attr_abs, rep_abs=full_abs, rep=full,
                terms=np.bincount(ii, minlength=N).astype(np.float64))


def tsne_grad_bound(ev, n_alive, slabs):
    """The derived bound on the error of a gradient component of the device (or of the yardstick) against the exact value, from
    tsne_eval_host()'s sums: a sum of m terms in any order errs by at most (m - 1) u sum |terms| to first order, u = 2^-53; the
    constant 8 covers the terms' own roundings (the differences, d, a reciprocal good to 2 ulp, the products) at 2^-52:
        4 [ (m + 8) 2^-52 sum |attractive terms| + (Na + slabs + 8) 2^-52 sum_j |w^2 delta| / Z + |repulsive part| rz ],
    rz = (Na + slabs + 8) 2^-52 the bound on the relative error of Z.  -> (N x 2)."""
    rz = (n_alive + slabs + 8) * TSNE_U
    return 4.0 * ((ev["terms"][:, None] + 8) * TSNE_U * ev["attr_abs"] + rz * ev["rep_abs"] / ev["z"]
                  + np.abs(ev["rep"]) / ev["z"] * rz)


def tsne_host(nbr_idx, nbr_d2, perplexity=20.0, init=None, max_iter=1000, exag_iters=250, kl_every=50, exaggeration=12.0, eta=0.0,
              seed=0x1D5EED, slabs=0, device=0, chunk=1024, perturb_seed=None):
    """api.tsne() in plain numpy float64 (the yardstick of the device path): the same arguments, checks, draw, schedule and
    record over the same sparse definitions, with a dense O(N^2) repulsion ``chunk`` rows at a time.  The record also holds, over
    the run's sign decisions of alive points, ``min_abs_g`` / ``min_abs_v`` (the smallest |g| and the smallest |v| from iteration
    1 on: v is exactly 0 at iteration 0 on every side) and ``min_g_margin`` / ``min_v_margin``: the smallest |g| / bound and
    |v| / (step gain bound), bound = tsne_grad_bound() with max(slabs, 1): a run whose margins exceed 1 takes the same decisions
    under any evaluation that meets the bound.  perturb_seed: every gradient component is moved by + or - its bound (random
    signs from that seed) before it is used: how far rounding-sized errors move the map.  (``device`` is accepted for the
    common signature and not used; ``ms`` is the wall time.)"""
    import time
    from . import api
    t_start = time.perf_counter()
    idx, d2, perplexity, init, max_iter, exag_iters, kl_every, exaggeration, eta, seed, slabs, alive = api.tsne_args(
        nbr_idx, nbr_d2, perplexity, init, max_iter, exag_iters, kl_every, exaggeration, eta, seed, slabs)
    N, k = idx.shape
    na = int(alive.sum())
    beta, pc = tsne_calibrate_host(idx, d2, perplexity)
    ii, jj, PP = tsne_joint_host(idx, pc, na)
    Y = (tsne_draw_host(seed, N) if init is None else init.copy())
    step = eta if eta > 0 else max(na / (4.0 * exaggeration), 50.0)
    gain, v = np.ones((N, 2)), np.zeros((N, 2))
    traj = np.full(max_iter // kl_every + 1, np.nan)
    rng = None if perturb_seed is None else np.random.default_rng(perturb_seed)
    mins = dict(min_abs_g=np.inf, min_abs_v=np.inf, min_g_margin=np.inf, min_v_margin=np.inf)
    for t in range(max_iter):
        a, mu = (exaggeration, 0.5) if t < exag_iters else (1.0, 0.8)
        ev = tsne_eval_host(Y, ii, jj, PP, alive, a, chunk)
        if t % kl_every == 0:
            traj[t // kl_every] = ev["kl"]
        g, bound = ev["grad"], tsne_grad_bound(ev, na, max(slabs, 1))
        if rng is not None:
            g = g + np.where(rng.random((N, 2)) < 0.5, -1.0, 1.0) * bound
        ga, ba = np.abs(g[alive]), bound[alive]
        mins["min_abs_g"] = min(mins["min_abs_g"], float(ga.min()))
        with np.errstate(divide="ignore", invalid="ignore"):
            mins["min_g_margin"] = min(mins["min_g_margin"], float(np.min(np.where(ba > 0, ga / ba, np.inf))))
            if t > 0:
                va = np.abs(v[alive])
                mins["min_abs_v"] = min(mins["min_abs_v"], float(va.min()))
                vb = step * gain[alive] * ba
                mins["min_v_margin"] = min(mins["min_v_margin"], float(np.min(np.where(vb > 0, va / vb, np.inf))))
        g = np.where(alive[:, None], g, 0.0)
        gain = np.maximum(np.where((g > 0) != (v > 0), gain + 0.2, gain * 0.8), 0.01)
        v = mu * v - (step * gain) * g
        Y = Y + v
        Y = Y - Y[alive].sum(axis=0) / float(na)
    ev = tsne_eval_host(Y, ii, jj, PP, alive, 1.0, chunk)
    if max_iter % kl_every == 0:
        traj[max_iter // kl_every] = ev["kl"]
    Y = np.where(alive[:, None], Y, np.nan)
    rec = dict(y=Y, kl_traj=traj, final_kl=ev["kl"], beta=np.where(alive, beta, np.nan), p_cond=pc, grad=ev["grad"], z=ev["z"],
               alive=alive, grad_bound=tsne_grad_bound(ev, na, max(slabs, 1)), ms=(time.perf_counter() - t_start) * 1e3)
    rec.update(mins)
    return rec


def embedding_graph(points, k, metric="cosine", device=0):
    """The neighbour graph of the columns of ``points`` (D x N) for tsne(): api.neighbors() of the points against themselves
    -> (nbr_idx (N x k int32, -1 = open slot), nbr_d2 (N x k): d2 = max(0, 2 - 2 score), the squared distance of the unit
    vectors, NaN at open slots).  Only the cosine score is a distance this way; api.tsne() itself takes any graph."""
    from . import api
    if metric != "cosine":
        raise api.InsiderError(api._lib.ERR_ARG, "embedding_graph offers the cosine metric only")
    nn = api.neighbors(points, None, k=k, metric=metric, device=device)
    idx, sc = nn["index"], nn["score"]
    with np.errstate(invalid="ignore"):
        return idx, np.where(idx >= 0, np.maximum(0.0, 2.0 - 2.0 * sc), np.nan)


def tsne_defaults(n_alive, n_points, perplexity=None, k=None):
    """The maps' defaults: perplexity = min(20, (Na - 1) / 3) (at least 1), k = min(64, N - 1, ceil(3 perplexity))."""
    if perplexity is None:
        perplexity = max(1.0, min(20.0, (n_alive - 1) / 3.0))
    if k is None:
        k = int(max(1, min(64, n_points - 1, np.ceil(3.0 * perplexity))))
    return float(perplexity), int(k)


def embedding_map(points, perplexity=None, k=None, metric="cosine", max_iter=1000, seed=0x1D5EED, device=0, **kw):
    """The t-SNE map of the columns of ``points`` (D x N): embedding_graph() and api.tsne() with tsne_defaults() (Na counted as
    the columns that are not all zero).  -> the api.tsne() record plus nbr_idx, nbr_d2, perplexity and k."""
    from . import api
    P = np.asarray(points, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] < 2:
        raise api.InsiderError(api._lib.ERR_ARG, "points must be a D x N array of at least 2 columns")
    perplexity, k = tsne_defaults(int(np.count_nonzero((P * P).sum(axis=0) > 0)), P.shape[1], perplexity, k)
    idx, d2 = embedding_graph(P, k, metric=metric, device=device)
    rec = api.tsne(idx, d2, perplexity=perplexity, max_iter=max_iter, seed=seed, device=device, **kw)
    rec.update(nbr_idx=idx, nbr_d2=d2, perplexity=perplexity, k=k)
    return rec


def gene_map(column_factor, perplexity=None, k=None, metric="cosine", max_iter=1000, seed=0x1D5EED, device=0, **kw):
    """The two-dimensional map of the genes: embedding_map() of the columns of C (K x p).  An all-zero column, which elastic-net
    fits do produce, has no neighbours under cosine and is nobody's: it is dead (y = NaN).  -> the api.tsne() record (y: p x 2)."""
    return embedding_map(column_factor, perplexity, k, metric, max_iter, seed, device, **kw)


def sample_map(cfd_factors, levels, ctns_confounder=None, perplexity=None, k=None, metric="cosine", max_iter=1000, seed=0x1D5EED,
               device=0, **kw):
    """The two-dimensional map of the samples: embedding_map() of sample_embeddings().  Samples that share every level are equal
    points at distance 0: they stay neighbours of each other.  -> the api.tsne() record (y: n x 2)."""
    return embedding_map(sample_embeddings(cfd_factors, levels, ctns_confounder), perplexity, k, metric, max_iter, seed, device,
                         **kw)


def module_overrepresentation(label, sets, k=None):
    """Over-representation of gene sets in gene modules, on the host.  ``label``: a module per gene, -1 = dead (the record of
    gene_modules()); ``sets``: (set_ptr, set_genes) or what flatio.read_gmt() returns.  The universe is the alive genes
    (label >= 0), M of them; set s marks its alive genes (size[s]); module j draws its n_j genes.  -> dict(overlap (k x S
    int32: the genes of set s in module j), hyper_p (k x S: the hypergeometric upper tail P(X >= overlap)), hyper_fdr
    (Benjamini-Hochberg over the sets of each module), size (S), module_size (k), and names when the sets carry them)."""
    lab = np.asarray(label).astype(np.int64).ravel()
    ptr, genes = np.asarray(sets[-2], dtype=np.int64), np.asarray(sets[-1], dtype=np.int64)
    S = ptr.size - 1
    k = int(lab.max()) + 1 if k is None else int(k)
    alive = lab >= 0
    M = int(alive.sum())
    module_size = np.bincount(lab[alive], minlength=k).astype(np.int32)
    overlap, size = np.zeros((k, S), dtype=np.int32), np.zeros(S, dtype=np.int32)
    for s in range(S):
        g = lab[genes[ptr[s]:ptr[s + 1]]]
        g = g[g >= 0]
        size[s] = g.size
        overlap[:, s] = np.bincount(g, minlength=k)
    hyper = np.array([[_hyper_tail(int(overlap[j, s]), M, int(size[s]), int(module_size[j])) for s in range(S)]
                      for j in range(k)], dtype=np.float64).reshape(k, S)
    fdr = np.ones((k, S))
    if S:
        o = np.argsort(hyper, axis=1, kind="stable")
        q = np.take_along_axis(hyper, o, axis=1) * S / np.arange(1, S + 1)
        q = np.minimum(np.minimum.accumulate(q[:, ::-1], axis=1)[:, ::-1], 1.0)
        np.put_along_axis(fdr, o, q, axis=1)
    rec = dict(overlap=overlap, hyper_p=hyper, hyper_fdr=fdr, size=size, module_size=module_size)
    if len(sets) == 3:
        rec["names"] = list(sets[0])
    return rec


# ---- agglomerative clustering (include/insider_hip.h states the definitions and the tie rule) ---------------------------------
def hclust_points(P, code):
    """The working points of insider_hip_hclust -> (X D x N, alive): cosine x = p / |p| (a zero column is dead), Euclidean
    x = p - m with the grand mean m summed in the header's order (256 interleaved partials, then the partials in order)."""
    D, N = P.shape
    if code == 0:
        nrm = np.sqrt(_sumsq(P))
        alive = nrm > 0
        return np.where(alive, P / np.where(alive, nrm, 1.0), 0.0), alive
    pad = np.zeros((D, -(-N // 256) * 256))
    pad[:, :N] = P
    pad = pad.reshape(D, -1, 256)
    part = np.zeros((D, 256))
    for r in range(pad.shape[1]):
        part = part + pad[:, r, :]
    tot = np.zeros(D)
    for e in range(256):
        tot = tot + part[:, e]
    return P - (tot / float(N))[:, None], np.ones(N, dtype=bool)


def hclust_state(X, alive):
    """The state of a run before its first round: per cluster id (0 .. 2 N - 2) the sum S, the size n, alive, nn (-1: none) and
    nn_d; the emitted records; the counters."""
    D, N = X.shape
    M = 2 * N - 1
    S = np.zeros((M, D))
    S[:N] = X.T
    al = np.zeros(M, dtype=bool)
    al[:N] = alive
    n = np.zeros(M, dtype=np.int64)
    n[:N] = 1
    return dict(N=N, S=S, n=n, alive=al, nn=np.full(M, -1, dtype=np.int64), nn_d=np.full(M, np.inf), ra=[], rb=[], rd=[], rn=[],
                scale=[], rounds=0, queries=0, min_gap=np.inf)


def hclust_round(st, code, force=False, chunk=512, blas=False):
    """One round of the run on the state ``st`` (hclust_state()), as include/insider_hip.h states it -> the number of merges.
    Every stale cluster (every alive one when ``force``) takes its first candidate in the order (d ascending, id ascending);
    the reciprocal pairs a < b are merged in ascending a.  A product adds its D terms in index order (blas=True: the matrix
    product).  st["min_gap"] keeps the smallest (runner-up d - best d) / scale over all queries so far, scale = the larger
    n_A n_B / (n_A + n_B) (h_A + h_B) of the two pairs under Ward and 1 under cosine: how far the run is from a choice that
    rounding could make; st["scale"] the same scale of every merged pair."""
    N, S, n, alive, nn = st["N"], st["S"], st["n"], st["alive"], st["nn"]
    act = np.flatnonzero(alive)
    stale_mask = np.ones(act.size, dtype=bool) if force else (nn[act] < 0) | ~alive[np.maximum(nn[act], 0)]
    stale = act[stale_mask]
    mu = S[act] / n[act][:, None].astype(np.float64)
    h = _sumsq(mu.T)
    nc = n[act].astype(np.float64)
    pos = np.flatnonzero(stale_mask)
    for c0 in range(0, stale.size, chunk):
        qp = pos[c0:c0 + chunk]
        Q = mu[qp]
        if blas:
            Pr = Q @ mu.T
        else:
            Pr = np.zeros((qp.size, act.size))
            for d in range(mu.shape[1]):
                Pr = Pr + Q[:, d][:, None] * mu[:, d][None, :]
        if code == 1:
            w = (nc[qp][:, None] * nc[None, :]) / (nc[qp][:, None] + nc[None, :])
            sc = w * (h[qp][:, None] + h[None, :])
            dist = np.maximum(0.0, w * ((h[qp][:, None] + h[None, :]) - 2.0 * Pr))
        else:
            sc = np.ones_like(Pr)
            dist = 1.0 - Pr
        rows = np.arange(qp.size)
        dist[rows, qp] = np.inf                                    # (itself)
        b1 = dist.argmin(axis=1)                                    # the first of equal distances: the lowest id
        d1 = dist[rows, b1]
        ok = np.isfinite(d1)
        nn[act[qp]] = np.where(ok, act[b1], -1)
        st["nn_d"][act[qp]] = d1
        if act.size > 2:
            s1 = sc[rows, b1]
            dist[rows, b1] = np.inf
            b2 = dist.argmin(axis=1)
            gap = (dist[rows, b2] - d1) / np.maximum(np.maximum(s1, sc[rows, b2]), 1e-300)
            st["min_gap"] = min(st["min_gap"], float(gap[ok].min()) if ok.any() else np.inf)
    st["rounds"] += 1
    st["queries"] += int(stale.size)
    b = nn[act]
    pair = (b > act) & (nn[np.maximum(b, 0)] == act)
    base = len(st["ra"])
    hpos = {int(c): i for i, c in enumerate(act)} if code == 1 else None
    for r, a in enumerate(act[pair]):
        a, bb = int(a), int(nn[a])
        c = N + base + r
        S[c] = S[a] + S[bb]
        n[c] = n[a] + n[bb]
        alive[a] = alive[bb] = False
        alive[c] = True
        nn[c] = -1
        st["ra"].append(a), st["rb"].append(bb), st["rd"].append(float(st["nn_d"][a])), st["rn"].append(int(n[c]))
        st["scale"].append(float(n[a] * n[bb]) / float(n[a] + n[bb]) * (h[hpos[a]] + h[hpos[bb]]) if code == 1 else 1.0)
    return int(pair.sum())


def hclust_finish(N, pt_alive, code, ra, rb, rd, rn):
    """The emitted records in the order and the numbering of the result -> (merge, height, size, order, perm): heights made
    monotone along the tree, a stable sort by height, row r creates id N + r, the lower id first; perm[r] = the emission index
    of row r."""
    R = len(ra)
    h = np.zeros(R)
    for r in range(R):
        v = np.sqrt(2.0 * rd[r]) if code == 1 else rd[r]
        for c in (ra[r], rb[r]):
            if c >= N:
                v = max(v, h[c - N])
        h[r] = v
    perm = np.argsort(h, kind="stable")
    row = np.empty(R, dtype=np.int64)
    row[perm] = np.arange(R)
    merge = np.full((max(N - 1, 0), 2), -1, dtype=np.int32)
    height, size = np.full(max(N - 1, 0), np.nan), np.full(max(N - 1, 0), -1, dtype=np.int32)
    for r in range(R):
        e = perm[r]
        x, y = (c if c < N else N + row[c - N] for c in (ra[e], rb[e]))
        merge[r] = min(x, y), max(x, y)
        height[r], size[r] = h[e], rn[e]
    order, stack = [], [N + R - 1] if R else [int(i) for i in np.flatnonzero(pt_alive)[::-1]]
    while stack:
        c = stack.pop()
        if c < N:
            order.append(c)
        else:
            stack.append(int(merge[c - N, 1]))
            stack.append(int(merge[c - N, 0]))
    order += [int(i) for i in np.flatnonzero(~np.asarray(pt_alive, dtype=bool))]
    return merge, height, size, np.array(order, dtype=np.int32), perm


def hclust_host(points, metric="cosine", linkage=None, max_rounds=None, chunk=512, blas=False):
    """api.hclust() in plain numpy float64 (the yardstick of the device path): the same arguments, checks, rule and record,
    following include/insider_hip.h line by line: rounds of reciprocal nearest neighbours over stale clusters only, sums and
    merges in the device's order.  The record also holds ``min_gap`` (hclust_round()), ``scale`` (per row, what the error bound
    of a height scales with) and ``d`` (per row, the linkage distance the height was made from).  A run that max_rounds cuts
    short raises InsiderError(ERR_UNFINISHED).  ``ms`` is the wall time."""
    import time
    from . import api
    t_start = time.perf_counter()
    P, code, _, max_rounds = api.hclust_args(points, metric, linkage, max_rounds)
    N = P.shape[1]
    X, pt_alive = hclust_points(P, code)
    st = hclust_state(X, pt_alive)
    force = False
    while int(st["alive"].sum()) > 1:
        if st["rounds"] == max_rounds:
            raise api.InsiderError(api._lib.ERR_UNFINISHED, "max_rounds reached before one cluster was left")
        force = hclust_round(st, code, force=force, chunk=chunk, blas=blas) == 0
    merge, height, size, order, perm = hclust_finish(N, pt_alive, code, st["ra"], st["rb"], st["rd"], st["rn"])
    R = len(st["ra"])
    scale, d = np.full(max(N - 1, 0), np.nan), np.full(max(N - 1, 0), np.nan)
    scale[:R], d[:R] = np.asarray(st["scale"], dtype=np.float64)[perm], np.asarray(st["rd"], dtype=np.float64)[perm]
    return dict(merge=merge, height=height, size=size, order=order, rounds=st["rounds"], queries=st["queries"],
                alive=int(pt_alive.sum()), min_gap=st["min_gap"], scale=scale, d=d, ms=(time.perf_counter() - t_start) * 1e3)


def cut_tree(rec, k=None, height=None):
    """Flat clusters of an hclust() record, on the host: the first alive - k merges (``k`` clusters), or every merge of height
    <= ``height``.  -> labels (N int32), 0-based in the order of every cluster's lowest point index, -1 for a dead point."""
    from . import api
    merge, hts = np.asarray(rec["merge"]), np.asarray(rec["height"])
    N, alive = int(np.asarray(rec["order"]).size), int(rec["alive"])
    R = max(alive - 1, 0)
    if (k is None) == (height is None):
        raise api.InsiderError(api._lib.ERR_ARG, "give exactly one of k and height")
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not (1 <= k <= alive or (alive == 0 and k == 0)):
            raise api.InsiderError(api._lib.ERR_ARG, f"k must be an integer in 1..{alive} (the alive points)")
        take = alive - int(k)
    else:
        take = int(np.searchsorted(hts[:R], float(height), side="right"))
    low = np.arange(N + R, dtype=np.int64)                          # the lowest point index under every id
    parent = np.arange(N + R, dtype=np.int64)
    for r in range(take):
        x, y = int(merge[r, 0]), int(merge[r, 1])
        low[N + r] = min(low[x], low[y])
        parent[x] = parent[y] = N + r
    label = np.full(N, -1, dtype=np.int32)
    dead = np.ones(N, dtype=bool)
    dead[np.asarray(rec["order"])[:alive]] = False
    root = np.arange(N + R)
    for c in range(N + take - 1, -1, -1):                           # (parents have higher ids: their roots are final)
        if parent[c] != c:
            root[c] = root[parent[c]]
    lows = low[root[:N]]
    lows[dead] = -1
    _, inv = np.unique(lows[~dead], return_inverse=True)
    label[~dead] = inv.astype(np.int32)
    return label


def tree_overrepresentation(rec, k, sets):
    """Over-representation of gene sets in the k modules a gene tree is cut into: module_overrepresentation() of
    cut_tree(rec, k)."""
    return module_overrepresentation(cut_tree(rec, k=k), sets, k=k)


def gene_tree(column_factor, metric="cosine", linkage=None, max_rounds=None, device=0):
    """The dendrogram of the genes: api.hclust() on the columns of C (K x p).  Under cosine (the default) an all-zero column of
    C is dead: in no cluster, last in ``order``.  -> the api.hclust() record (order: the gene order of a heat map)."""
    from . import api
    return api.hclust(column_factor, metric=metric, linkage=linkage, max_rounds=max_rounds, device=device)


def sample_tree(cfd_factors, levels, ctns_confounder=None, metric="cosine", linkage=None, max_rounds=None, device=0):
    """The dendrogram of the samples: api.hclust() on sample_embeddings().  Samples that share every level are equal points:
    they merge first, at height 0, in ascending index (the tie rule).  -> the api.hclust() record."""
    from . import api
    return api.hclust(sample_embeddings(cfd_factors, levels, ctns_confounder), metric=metric, linkage=linkage,
                      max_rounds=max_rounds, device=device)


def level_tree(cfd_factor, metric="cosine", linkage=None, max_rounds=None, device=0):
    """The dendrogram of one covariate's levels (which tissues, phenotypes or donors go together): api.hclust() on the rows of
    its L x K matrix.  -> the api.hclust() record (leaves: 0-based levels)."""
    from . import api
    return api.hclust(np.asarray(cfd_factor, dtype=np.float64).T, metric=metric, linkage=linkage, max_rounds=max_rounds,
                      device=device)


def module_summary(rec, column_factor):
    """What the modules of a gene_modules() record look like: mean_abs_loading (k x K: per module the mean |loading| of its
    genes on every factor, NaN for an empty module) and members (k arrays of 0-based genes by ascending dist, equal distances by
    ascending gene: the most typical gene first)."""
    Cm = np.abs(np.asarray(column_factor, dtype=np.float64))
    lab, k = np.asarray(rec["label"]), int(np.asarray(rec["sizes"]).size)
    mean_abs, members = np.full((k, Cm.shape[0]), np.nan), []
    for j in range(k):
        g = np.flatnonzero(lab == j)
        members.append(g[np.argsort(np.asarray(rec["dist"])[g], kind="stable")])
        if g.size:
            mean_abs[j] = Cm[:, g].mean(axis=1)
    return dict(mean_abs_loading=mean_abs, members=members)
