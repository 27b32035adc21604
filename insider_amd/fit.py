"""Command-line driver: the INSIDER fit on the MI355X from files, no R and no .RData.

    python -m insider_amd.fit --flat DIR                     # inputs written by r/insider_hip.R:insider_write_flat
    python -m insider_amd.fit --x X.npy --levels L.npy [--train-mask M.npy --test-mask T.npy] [--ctns Z.npy]
        --rank K --lambda 5 --alpha 0.4 [--partition 0|1] [--max-iter N] [--out DIR] [--out-format npy|flat]
    ... --tune --ranks 10 12 14 --lambdas 1 3 5 --alphas 0.2 0.4   # tune()'s rank sweep + lambda x alpha grid
    ... --tune --folds 5 ...                    # k-fold cross-validated tune(): mean / pooled / per-fold RMSE per grid point
    ... --interaction 1 2 --interaction-glm 1   # then glm_interaction() on the device for covariate column 1 (0-based)
    ... --variance-decomposition                # then the per-gene variance decomposition on the device
    ... --sample-decomposition                  # then the per-sample and per-level fit diagnostics on the device
    ... --factor-decomposition                  # then the per-factor decomposition (which factor, through which covariate)
    ... --outliers 3 [--outlier-entries train]  # then the entries whose standardised residual has |z| >= 3, on the device
    ... --gene-neighbors 10 --sample-neighbors 10 [--neighbor-metric cosine]   # then each gene's / sample's nearest in latent space
    ... --gene-coexpression 10 --sample-coexpression 10   # then each gene's / sample's most correlated partners in the residual
    ... --gene-coexpression 10 --coexpression-missing pairwise [--coexpression-min-overlap 30]   # ... pairwise-complete
    ... --gene-modules 20 --sample-clusters 6 [--cluster-metric cosine]        # then k-means of the genes / samples in latent space
    ... --gene-map --sample-map [--map-perplexity 20] [--map-neighbors 60]     # then the t-SNE map of the genes / samples
    ... --gene-tree --sample-tree [--tree-metric cosine] [--tree-cut 20]       # then the dendrogram of the genes / samples
    ... --level-scores 1 [--level-score-entries train]   # then every sample against every level of covariate column 1 (1-based)
    ... --residual-components 5 [--rc-standardize] [--rc-entries train]   # then the hidden factors: what the model left behind
    ... --gene-sets SETS.gmt [--gene-names NAMES.txt] [--enrich-perms 1000] [--enrich-levels 1]   # then what each factor means

Semantics are those of insider_amd.api (the mirror of R/insider.R): with masks given, `--partition 1` fits on the
train entries (optimize(tuning = 1)) and reports the test RMSE; without masks (or `--partition 0`) every non-NA entry is
used (fit()'s default, R/insider.R:190-216; NaN entries of X are the NA set).  Inits are N(0, 0.001^2)
(R/utils.R:40-43) from --seed.  --interaction-glm COV adds interaction_coeff / interaction_pval (L_COV x K, glm_interaction()
on the device against the residual of every other block); --variance-decomposition adds vd_r2 / vd_rmse (p) and
vd_explained / vd_drop_one (B x p, posthoc.vd_derived) over the entries the fit used; --sample-decomposition adds the same per
sample, sd_r2 / sd_rmse (n) and sd_explained / sd_drop_one (B x n), and per level of every categorical covariate b,
sd_level<b>_r2 / sd_level<b>_rmse (L_b, posthoc.level_decomposition); --factor-decomposition adds the tables pooled over genes
fd_summary_explained / fd_summary_drop_one ((B + 1) x K, the last block the total; posthoc.factor_summary), fd_order (the
factors by descending pooled drop_one of the total) and per gene fd_explained / fd_drop_one (p x (B + 1) K, block-major
columns); --outliers T adds the calls |z| >= T among the --outlier-entries (z standardised by each gene's residual mean and
standard deviation over those entries, posthoc.residual_center_scale): ol_rows, ol_cols (0-based sample and gene), ol_z (in
ascending gene, then sample), ol_gene_counts (p x 2) and ol_sample_counts (n x 2), columns {low, high};
--gene-neighbors N / --sample-neighbors N add each gene's N nearest genes by its column of C and each sample's N nearest
samples by its row embedding (posthoc.gene_neighbors / sample_neighbors, --neighbor-metric cosine or dot): nn_gene_index /
nn_gene_score (p x N) and nn_sample_index / nn_sample_score (n x N), 0-based, descending score, ties by ascending index, open
slots -1 / NaN; --gene-coexpression N / --sample-coexpression N add each gene's N most correlated genes and each sample's N most
correlated samples in the residual of the fit over the entries it used (posthoc.gene_coexpression / sample_coexpression; the
samples after every gene's residual is centred and scaled, posthoc.residual_center_scale): cx_gene_index / cx_gene_score
(p x N) and cx_sample_index / cx_sample_score (n x N), indices int32 and 0-based, descending score, ties by ascending index,
open slots -1 / NaN; --coexpression-missing says what a missing entry does to them: "zero" (the default) the zero-filled
correlation (a missing entry counts as the vector's mean, scores shrink towards 0 with missingness, one product), "pairwise"
the pairwise-complete correlation (Pearson's r of each pair over the entries both have, six products; a pair needs
--coexpression-min-overlap M joint entries, default max(3, ceil(depth / 4)), and variance in both on them), which also writes
cx_gene_overlap / cx_sample_overlap (int32: the joint entries of each listed pair, -1 in open slots);
--gene-modules K / --sample-clusters K add the k-means partition of the genes by their columns of C and of the
samples by their row embeddings (posthoc.gene_modules / sample_clusters; --cluster-metric cosine or euclidean, the best of
--cluster-restarts drawn starts from --cluster-seed, at most --cluster-iters updates each): km_gene_label / km_gene_second (p,
0-based, -1 = an all-zero column under cosine, or no second centre), km_gene_dist / km_gene_dist2 (p), km_gene_center (K x k),
km_gene_size (k), km_gene_traj (the inertia before every update, NaN beyond the last) and the same under km_sample_*; with
--gene-sets also km_gene_overlap / km_gene_hyper_p / km_gene_hyper_fdr (k x S, posthoc.module_overrepresentation);
--gene-map / --sample-map add the exact t-SNE map of the genes by their columns of C and of the samples by their row embeddings
(posthoc.gene_map / sample_map: the cosine neighbour graph of --map-neighbors neighbours, --map-perplexity, --map-iters
iterations from the start drawn from --map-seed; the defaults follow posthoc.tsne_defaults): ts_gene_y (p x 2, NaN for an
all-zero column), ts_gene_kl (KL every 50 iterations and at the end), ts_gene_beta (p) and the same under ts_sample_*;
--gene-tree / --sample-tree add the dendrogram of the genes by their columns of C and of the samples by their row embeddings
(posthoc.gene_tree / sample_tree; --tree-metric cosine: average linkage, the default, or euclidean: Ward's linkage):
hc_gene_merge (p - 1 x 2 int32, scipy's numbering: row r creates id p + r), hc_gene_height, hc_gene_size (p - 1), hc_gene_order
(p: the leaf order, points in no cluster last; rows beyond the alive points hold -1 / NaN), with --tree-cut K hc_gene_label (p,
0-based by the lowest member, -1 = in no cluster) and the same under hc_sample_*; with --gene-sets and --tree-cut also
hc_gene_overlap / hc_gene_hyper_p / hc_gene_hyper_fdr (K x S, posthoc.tree_overrepresentation);
--level-scores COV adds, for covariate column COV (1-based), ls_sse (n x L: the residual sum of squares of every
sample over the --level-score-entries with its embedding for COV replaced by each level's), ls_n, ls_best (1-based, 0 = no
entry), ls_margin (n) and ls_confusion (L x L, assigned x best; posthoc.ls_derived) — a sample's own level was fitted with that
sample, so on the entries the fit used the assigned level is favoured, most for levels with few samples;
--residual-components R adds the R leading singular directions of the masked residual over the --rc-entries
(posthoc.residual_components: a subspace iteration whose products stream over the resident X; --rc-standardize centres and
scales every gene's residual first): rc_sv, rc_share (R), rc_sample_scores (n x R), rc_gene_loadings (p x R) and rc_assoc
(blocks x R: eta-squared of every component on every categorical covariate, R-squared on the continuous block;
posthoc.component_associations); --gene-sets FILE (GMT;
tokens are the lines of --gene-names, else 0-based gene columns; sets outside --enrich-min-size..--enrich-max-size are dropped)
adds the preranked gene-set enrichment of every factor's |loadings| against every set with --enrich-perms random sets of equal
size as the null (posthoc.factor_enrichment): gs_factor_es / gs_factor_nes / gs_factor_pval / gs_factor_fdr / gs_factor_peak
(K x S), gs_size (S) and gs_set_names.txt, and with --enrich-levels B the same for the signed per-gene effect of every level of
covariate column B (1-based), gs_level<B>_es / _nes / _pval / _fdr / _peak (L_B x S; posthoc.level_enrichment).  Output: A<i> (L_i x K), C (K x p) and result.json {train_rmse, test_rmse, loss,
iters, traj} in --out.  There is no CPU fallback: without a visible MI355X the command fails with the library's status.
"""
import argparse
import json
import os
import sys

import numpy as np


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="python -m insider_amd.fit", description=__doc__.split("\n\n")[0])
    ap.add_argument("--flat", help="directory in the insider-flat-1 layout (X.f64, levels.i32, train.u8, test.u8, manifest.json)")
    ap.add_argument("--x", help="n x p expression matrix (.npy / .csv); NaN = NA")
    ap.add_argument("--levels", help="n x c categorical covariates, 1-based level ids (.npy / .csv)")
    ap.add_argument("--ctns", help="n x m continuous covariates (.npy / .csv)")
    ap.add_argument("--train-mask", help="n x p 0/1 (.npy)")
    ap.add_argument("--test-mask", help="n x p 0/1 (.npy)")
    ap.add_argument("--interaction", type=int, nargs="+", help="1-based covariate columns to interact (R/insider.R:28-40)")
    ap.add_argument("--rank", type=int, help="latent dimension K")
    ap.add_argument("--lambda", dest="lam", type=float)
    ap.add_argument("--alpha", type=float)
    ap.add_argument("--partition", type=int, default=None, choices=(0, 1))
    ap.add_argument("--max-iter", type=int, default=50000)
    ap.add_argument("--global-tol", type=float, default=1e-9)
    ap.add_argument("--sub-tol", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=0x1D5EED)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tune", action="store_true")
    ap.add_argument("--ranks", type=int, nargs="+")
    ap.add_argument("--lambdas", type=float, nargs="+")
    ap.add_argument("--alphas", type=float, nargs="+")
    ap.add_argument("--tuning-iter", type=int, default=30)
    ap.add_argument("--warm-start", action="store_true",
                    help="--tune: start every (lambda, alpha) grid point from its nearest finished neighbour's factors "
                         "(opt-in; the reference draws fresh inits per point, R/insider.R:152-161)")
    ap.add_argument("--folds", type=int, default=None, metavar="K",
                    help="--tune: K-fold cross-validation (every grid point fitted once per fold on re-masks of the one "
                         "resident matrix); tune.json gains the per-fold tables, tune_folds.csv holds them")
    ap.add_argument("--split-ratio", type=float, default=0.1)
    ap.add_argument("--out", default="insider_fit_out")
    ap.add_argument("--out-format", choices=("npy", "flat"), default=None)
    ap.add_argument("--interaction-glm", type=int, default=None, metavar="COV",
                    help="after the fit, glm_interaction() on the device for the levels of covariate column COV (0-based, "
                         "after --interaction: its indicator is column 1) against the residual of every other block; "
                         "writes interaction_coeff / interaction_pval (L x K) next to the factors")
    ap.add_argument("--variance-decomposition", action="store_true",
                    help="after the fit, the per-gene variance decomposition on the device over the entries the fit used; "
                         "writes vd_r2, vd_rmse (p) and vd_explained, vd_drop_one (blocks x p) next to the factors")
    ap.add_argument("--sample-decomposition", action="store_true",
                    help="after the fit, the per-sample fit diagnostics on the device over the entries the fit used; writes "
                         "sd_r2, sd_rmse (n), sd_explained, sd_drop_one (blocks x n) and, per categorical covariate b, "
                         "sd_level<b>_r2, sd_level<b>_rmse (its levels) next to the factors")
    ap.add_argument("--factor-decomposition", action="store_true",
                    help="after the fit, the per-factor decomposition on the device over the entries the fit used; writes "
                         "fd_summary_explained, fd_summary_drop_one ((blocks + 1) x K), fd_order (K) and fd_explained, "
                         "fd_drop_one (p x (blocks + 1) K, block-major columns) next to the factors")
    ap.add_argument("--outliers", type=float, default=None, metavar="T",
                    help="after the fit, the entries whose standardised residual has |z| >= T, on the device; writes ol_rows, "
                         "ol_cols, ol_z (ascending gene, then sample), ol_gene_counts (p x 2) and ol_sample_counts (n x 2; "
                         "columns low, high) next to the factors")
    ap.add_argument("--outlier-entries", choices=("all", "train", "test"), default="train",
                    help="--outliers: the entries that can be called (default: train, the entries the fit used)")
    ap.add_argument("--level-scores", type=int, default=None, metavar="COV",
                    help="after the fit, every sample scored against every level of covariate column COV (1-based like "
                         "--interaction, counted after it), on the device; writes ls_sse (n x L), ls_n, ls_best, ls_margin (n) "
                         "and ls_confusion (L x L, assigned x best) next to the factors.  A sample's own level was fitted with "
                         "that sample: on the entries the fit used the assigned level is favoured")
    ap.add_argument("--level-score-entries", choices=("all", "train", "test"), default="train",
                    help="--level-scores: the entries that are scored (default: train, the entries the fit used)")
    ap.add_argument("--residual-components", type=int, default=None, metavar="R",
                    help="after the fit, the R leading singular directions of the masked residual (hidden factors: an "
                         "unmodelled batch, a missing interaction), on the device; writes rc_sv, rc_share (R), rc_sample_scores "
                         "(n x R), rc_gene_loadings (p x R) and rc_assoc (blocks x R: how much of each component every known "
                         "covariate explains) next to the factors")
    ap.add_argument("--rc-standardize", action="store_true",
                    help="--residual-components: centre and scale every gene's residual first")
    ap.add_argument("--rc-entries", choices=("all", "train", "test"), default="train",
                    help="--residual-components: the entries of the residual (default: train, the entries the fit used)")
    ap.add_argument("--gene-neighbors", type=int, default=None, metavar="N",
                    help="after the fit, every gene's N nearest genes in the latent space (columns of C), on the device; "
                         "writes nn_gene_index, nn_gene_score (p x N; 0-based, open slots -1 / NaN) next to the factors")
    ap.add_argument("--sample-neighbors", type=int, default=None, metavar="N",
                    help="after the fit, every sample's N nearest samples by its row embedding (the sum of its levels' rows), "
                         "on the device; writes nn_sample_index, nn_sample_score (n x N) next to the factors")
    ap.add_argument("--neighbor-metric", choices=("cosine", "dot"), default="cosine",
                    help="--gene-neighbors / --sample-neighbors: the score (default: cosine)")
    ap.add_argument("--gene-coexpression", type=int, default=None, metavar="N",
                    help="after the fit, every gene's N most correlated genes in the residual over the entries the fit used, on "
                         "the device; writes cx_gene_index (int32, 0-based, open slots -1), cx_gene_score (p x N, open slots NaN) "
                         "next to the factors")
    ap.add_argument("--sample-coexpression", type=int, default=None, metavar="N",
                    help="after the fit, every sample's N most correlated samples in the residual (every gene's residual centred "
                         "and scaled first), on the device; writes cx_sample_index, cx_sample_score (n x N) next to the factors")
    ap.add_argument("--coexpression-missing", choices=("zero", "pairwise"), default="zero",
                    help="--gene-coexpression / --sample-coexpression: what a missing entry does.  zero (default): the "
                         "zero-filled correlation, a missing entry counts as the vector's mean and scores shrink with "
                         "missingness; pairwise: the pairwise-complete correlation, Pearson's r of each pair over the entries "
                         "both have, which also writes cx_gene_overlap / cx_sample_overlap (int32)")
    ap.add_argument("--coexpression-min-overlap", type=int, default=None, metavar="M",
                    help="--coexpression-missing pairwise: the joint entries a pair needs, at least 3 (default "
                         "max(3, ceil(depth / 4)))")
    ap.add_argument("--gene-modules", type=int, default=None, metavar="K",
                    help="after the fit, the k-means partition of the genes into K modules by their columns of C, on the device; "
                         "writes km_gene_label, km_gene_dist, km_gene_second, km_gene_dist2 (p), km_gene_center (rank x K), "
                         "km_gene_size (K) and km_gene_traj next to the factors; with --gene-sets also km_gene_overlap, "
                         "km_gene_hyper_p, km_gene_hyper_fdr (K x S)")
    ap.add_argument("--sample-clusters", type=int, default=None, metavar="K",
                    help="after the fit, the k-means partition of the samples into K clusters by their row embeddings, on the "
                         "device; writes the km_sample_* records (samples that share every level are equal points)")
    ap.add_argument("--cluster-metric", choices=("cosine", "euclidean"), default="cosine",
                    help="--gene-modules / --sample-clusters: spherical (cosine, the default: all-zero columns of C form no "
                         "module) or Euclidean k-means")
    ap.add_argument("--cluster-restarts", type=int, default=8, metavar="R",
                    help="--gene-modules / --sample-clusters: drawn starts, the lowest final inertia is kept (default 8)")
    ap.add_argument("--cluster-iters", type=int, default=100, metavar="I",
                    help="--gene-modules / --sample-clusters: updates per start at most (default 100)")
    ap.add_argument("--cluster-seed", type=int, default=0x1D5EED, metavar="S",
                    help="--gene-modules / --sample-clusters: the seed of the drawn starts")
    ap.add_argument("--gene-tree", action="store_true",
                    help="after the fit, the dendrogram of the genes by their columns of C (agglomerative clustering on the "
                         "device); writes hc_gene_merge (p - 1 x 2), hc_gene_height, hc_gene_size (p - 1), hc_gene_order (p: the "
                         "leaf order of a heat map) next to the factors; with --tree-cut K also hc_gene_label (p) and, with "
                         "--gene-sets, hc_gene_overlap, hc_gene_hyper_p, hc_gene_hyper_fdr (K x S)")
    ap.add_argument("--sample-tree", action="store_true",
                    help="after the fit, the dendrogram of the samples by their row embeddings, on the device; writes the "
                         "hc_sample_* records")
    ap.add_argument("--tree-metric", choices=("cosine", "euclidean"), default=None,
                    help="--gene-tree / --sample-tree: cosine (the default: average linkage, all-zero columns of C are in no "
                         "cluster) or euclidean (Ward's linkage)")
    ap.add_argument("--tree-cut", type=int, default=None, metavar="K",
                    help="--gene-tree / --sample-tree: also the labels of the tree cut into K clusters (hc_gene_label / "
                         "hc_sample_label, -1 for a point in no cluster)")
    ap.add_argument("--gene-map", action="store_true",
                    help="after the fit, the exact t-SNE map of the genes by their columns of C, on the device; writes ts_gene_y "
                         "(p x 2; NaN for an all-zero column), ts_gene_kl and ts_gene_beta (p) next to the factors")
    ap.add_argument("--sample-map", action="store_true",
                    help="after the fit, the exact t-SNE map of the samples by their row embeddings, on the device; writes the "
                         "ts_sample_* records")
    ap.add_argument("--map-perplexity", type=float, default=None, metavar="P",
                    help="--gene-map / --sample-map: the perplexity (default min(20, (points - 1) / 3))")
    ap.add_argument("--map-neighbors", type=int, default=None, metavar="N",
                    help="--gene-map / --sample-map: neighbours per point of the graph, 1..64 (default ceil(3 perplexity))")
    ap.add_argument("--map-iters", type=int, default=1000, metavar="I",
                    help="--gene-map / --sample-map: iterations (default 1000, the first 250 exaggerated)")
    ap.add_argument("--map-seed", type=int, default=0x1D5EED, metavar="S", help="--gene-map / --sample-map: the seed of the start")
    ap.add_argument("--gene-sets", default=None, metavar="FILE",
                    help="after the fit, the gene-set enrichment of every factor's |loadings| on the device against the sets of "
                         "this GMT file (name, description, genes; tab-separated); writes gs_factor_es, gs_factor_nes, "
                         "gs_factor_pval, gs_factor_fdr, gs_factor_peak (K x S), gs_size (S) and gs_set_names.txt next to the "
                         "factors")
    ap.add_argument("--gene-names", default=None, metavar="FILE",
                    help="--gene-sets: one gene name per line, in the order of the columns of X (default: the GMT tokens are "
                         "0-based column indices)")
    ap.add_argument("--enrich-perms", type=int, default=1000, metavar="N",
                    help="--gene-sets: random gene sets of equal size per (factor, set size) (default 1000, at most 65536)")
    ap.add_argument("--enrich-min-size", type=int, default=15, help="--gene-sets: smallest set kept (default 15)")
    ap.add_argument("--enrich-max-size", type=int, default=500, help="--gene-sets: largest set kept (default 500, at most 4096)")
    ap.add_argument("--enrich-levels", type=int, default=None, metavar="B",
                    help="--gene-sets: also the enrichment of every level's signed per-gene effect of covariate column B "
                         "(1-based like --level-scores); writes gs_level<B>_es / _nes / _pval / _fdr / _peak (L x S)")
    a = ap.parse_args(argv)
    if a.gene_sets is None and (a.gene_names is not None or a.enrich_levels is not None):
        ap.error("--gene-names and --enrich-levels go with --gene-sets")
    if a.gene_sets is not None:
        if a.tune:
            ap.error("--gene-sets interprets a fit: it does not go with --tune")
        if not 1 <= a.enrich_perms <= 65536:
            ap.error("--enrich-perms must be in 1..65536")
        if not 1 <= a.enrich_min_size <= a.enrich_max_size <= 4096:
            ap.error("--enrich-min-size / --enrich-max-size must satisfy 1 <= min <= max <= 4096")
        if a.enrich_levels is not None and a.enrich_levels < 1:
            ap.error("--enrich-levels: B is 1-based")
    for name in ("gene_neighbors", "sample_neighbors", "gene_coexpression", "sample_coexpression"):
        v = getattr(a, name)
        if v is not None and not 1 <= v <= 64:
            ap.error(f"--{name.replace('_', '-')} must be in 1..64")
        if v is not None and a.tune and name.endswith("coexpression"):
            ap.error(f"--{name.replace('_', '-')} reads a fit: it does not go with --tune")
    if a.coexpression_missing == "pairwise" and a.gene_coexpression is None and a.sample_coexpression is None:
        ap.error("--coexpression-missing goes with --gene-coexpression or --sample-coexpression")
    if a.coexpression_min_overlap is not None:
        if a.coexpression_missing != "pairwise":
            ap.error("--coexpression-min-overlap goes with --coexpression-missing pairwise")
        if a.coexpression_min_overlap < 3:
            ap.error("--coexpression-min-overlap must be >= 3")
    for name in ("gene_modules", "sample_clusters"):
        v = getattr(a, name)
        if v is not None and not 1 <= v <= 4096:
            ap.error(f"--{name.replace('_', '-')} must be in 1..4096")
        if v is not None and a.tune:
            ap.error(f"--{name.replace('_', '-')} partitions a fit: it does not go with --tune")
    if a.gene_tree or a.sample_tree:
        if a.tune:
            ap.error("--gene-tree / --sample-tree cluster a fit: they do not go with --tune")
        if a.tree_cut is not None and a.tree_cut < 1:
            ap.error("--tree-cut must be at least 1")
    elif a.tree_metric is not None or a.tree_cut is not None:
        ap.error("--tree-metric and --tree-cut go with --gene-tree or --sample-tree")
    if a.gene_map or a.sample_map:
        if a.tune:
            ap.error("--gene-map / --sample-map draw a fit: they do not go with --tune")
    elif a.map_perplexity is not None or a.map_neighbors is not None:
        ap.error("--map-perplexity and --map-neighbors go with --gene-map or --sample-map")
    if a.map_perplexity is not None and not (np.isfinite(a.map_perplexity) and a.map_perplexity >= 1.0):
        ap.error("--map-perplexity must be finite and >= 1")
    if a.map_neighbors is not None and not 1 <= a.map_neighbors <= 64:
        ap.error("--map-neighbors must be in 1..64")
    if not 1 <= a.map_iters <= 10000:
        ap.error("--map-iters must be in 1..10000")
    if not 0 <= a.map_seed < 2 ** 64:
        ap.error("--map-seed must fit 64 bits")
    if not 1 <= a.cluster_restarts <= 256:
        ap.error("--cluster-restarts must be in 1..256")
    if not 0 <= a.cluster_iters <= 10000:
        ap.error("--cluster-iters must be in 0..10000")
    if not 0 <= a.cluster_seed < 2 ** 64:
        ap.error("--cluster-seed must fit 64 bits")
    if a.level_scores is not None and a.level_scores < 1:
        ap.error("--level-scores: COV is 1-based")
    if not a.flat and not (a.x and a.levels):
        ap.error("give --flat DIR or --x and --levels")
    if not a.tune and (a.rank is None or a.lam is None or a.alpha is None):
        ap.error("a fit needs --rank, --lambda and --alpha (or use --tune)")
    if a.tune and a.level_scores is not None:
        ap.error("--level-scores scores a fit: it does not go with --tune")
    if a.residual_components is None and a.rc_standardize:
        ap.error("--rc-standardize goes with --residual-components")
    if a.residual_components is not None:
        if a.tune:
            ap.error("--residual-components reads a fit: it does not go with --tune")
        if not 1 <= a.residual_components <= 64:
            ap.error("--residual-components must be in 1..64")
    if a.folds is not None and not a.tune:
        ap.error("--folds goes with --tune")
    if a.folds is not None and a.warm_start:
        ap.error("--folds and --warm-start exclude each other")
    return a


def load_inputs(a):
    from . import flatio
    if a.flat:
        d = flatio.read_flat(a.flat)
        X, lev, tr, te, Z = d["X"], d["levels"], d["train"], d["test"], d["ctns"]
    else:
        X = flatio.load_matrix(a.x, np.float64)
        lev = flatio.load_matrix(a.levels).astype(np.int32).reshape(X.shape[0], -1)
        tr = flatio.load_matrix(a.train_mask) if a.train_mask else None
        te = flatio.load_matrix(a.test_mask) if a.test_mask else None
        Z = flatio.load_matrix(a.ctns, np.float64) if a.ctns else None
    return X, lev, tr, te, Z


def km_records(prefix, rec):
    """The records of one api.kmeans() result under <prefix>_label, _dist, _second, _dist2, _center, _size and _traj."""
    names = dict(label="label", dist="dist", second="second", dist2="dist2", center="centers", size="sizes", traj="traj")
    return {f"{prefix}_{out}": rec[key] for out, key in names.items()}


def ts_records(prefix, rec):
    """The records of one api.tsne() result under <prefix>_y, _kl (the recorded KL, then the final one) and _beta."""
    return {f"{prefix}_y": rec["y"], f"{prefix}_kl": np.append(rec["kl_traj"], rec["final_kl"]), f"{prefix}_beta": rec["beta"]}


def main(argv=None):
    a = parse(argv)
    from . import api, flatio
    X, lev, tr, te, Z = load_inputs(a)
    X = np.array(X, dtype=np.float64, order="F")
    na = np.isnan(X)
    X[na] = 0.0                                                           # R/insider.R:26
    if a.interaction:
        from .workloads import interaction_indicator
        lev = interaction_indicator(np.asarray(lev, dtype=np.int32), tuple(a.interaction))
    n, p = X.shape
    if a.level_scores is not None and not 1 <= a.level_scores <= np.asarray(lev).reshape(n, -1).shape[1]:
        raise SystemExit(f"--level-scores: COV must be in 1..{np.asarray(lev).reshape(n, -1).shape[1]}")
    if a.enrich_levels is not None and not 1 <= a.enrich_levels <= np.asarray(lev).reshape(n, -1).shape[1]:
        raise SystemExit(f"--enrich-levels: B must be in 1..{np.asarray(lev).reshape(n, -1).shape[1]}")
    fmt = a.out_format or ("flat" if a.flat else "npy")
    if a.tune:
        # the caller-level path: insider() draws its own hold-out (R/utils.R:78-117) unless masks were given
        obj = api.insider(np.where(na, np.nan, X), lev, ctns_confounder=Z, split_ratio=a.split_ratio, global_tol=a.global_tol,
                          sub_tol=a.sub_tol, tuning_iter=a.tuning_iter, max_iter=a.max_iter, device=a.device, seed=a.seed,
                          folds=a.folds)
        if tr is not None and te is not None and a.folds is None:
            obj["train_indicator"] = np.asfortranarray(np.asarray(tr) != 0, dtype=np.uint8)
            obj["test_indicator"] = np.asfortranarray(np.asarray(te) != 0, dtype=np.uint8)
        res = api.tune(obj, latent_dimension=np.array(a.ranks if a.ranks else [a.rank]),
                       lambda_=a.lambdas if a.lambdas else (a.lam if a.lam is not None else 0.1),
                       alpha=a.alphas if a.alphas else (a.alpha if a.alpha is not None else 0.0), out_dir=None,
                       rng=np.random.default_rng(a.seed), warm_start=a.warm_start, folds=True if a.folds else None)
        os.makedirs(a.out, exist_ok=True)
        if a.folds:
            # the per-fold table next to tune.json: one row per fitted point (the rank sweep first) — latent rank, lambda,
            # alpha (NaN in the rank sweep's rows: tune() fixes them there), then the F per-fold test RMSEs
            blocks = []
            if res["rank_tuning"] is not None:
                k_col = res["rank_tuning"][:, :1]
                blocks.append(np.column_stack([k_col, np.full((len(k_col), 2), np.nan), res["rank_tuning_folds"]]))
            if res["reg_tuning"] is not None:
                g2 = res["reg_tuning"][:, :2]
                blocks.append(np.column_stack([np.full(len(g2), float(res["latent_rank"])), g2, res["reg_tuning_folds"]]))
            np.savetxt(os.path.join(a.out, "tune_folds.csv"), np.vstack(blocks), delimiter=",")
        out = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
        with open(os.path.join(a.out, "tune.json"), "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps({"latent_rank": res["latent_rank"], "out": a.out}))
        return 0
    if tr is None:
        tr = ~na
    if te is None:
        te = np.zeros((n, p), dtype=bool)
    tr = np.asfortranarray(np.asarray(tr) != 0, dtype=np.uint8)
    te = np.asfortranarray(np.asarray(te) != 0, dtype=np.uint8)
    partition = a.partition if a.partition is not None else (1 if te.any() else 0)
    if partition == 0:                                                    # R/insider.R:207-208: train + test, "test" = NA
        tr, te = np.asfortranarray((tr | te) & ~na, dtype=np.uint8), np.asfortranarray(na, dtype=np.uint8)
    ds = api.InsiderData(X, lev, tr, te, device=a.device, ctns_confounder=Z)
    ds_levels = np.asarray(lev, dtype=np.int32).reshape(n, -1)
    rng = np.random.default_rng(a.seed)
    K = a.rank
    A0 = [np.asfortranarray(api.init_parameters(int(L) * K, rng=rng).reshape((-1, K), order="F")) for L in ds.n_levels]
    if Z is not None:
        A0.append(np.asfortranarray(api.init_parameters(ds.m * K, rng=rng).reshape((-1, K), order="F")))
    C0 = np.asfortranarray(api.init_parameters(K * p, rng=rng).reshape((K, -1), order="F"))
    res = ds.optimize(A0, C0, K, a.lam, a.lam, a.alpha, tuning=partition, global_tol=a.global_tol, sub_tol=a.sub_tol,
                      max_iter=a.max_iter, seed=a.seed, inc_continuous=1 if Z is not None else 0)
    glm = None
    if a.interaction_glm is not None:
        from .posthoc import t_pvalues
        cov = a.interaction_glm
        if not 0 <= cov < ds.c:
            raise SystemExit(f"--interaction-glm: COV must be in 0..{ds.c - 1}")
        rows = list(res["row_matrices"].values())
        coeff, se, dof = ds.interaction_glm(rows, res["column_factor"], ds_levels[:, cov],
                                            subtract=[b != cov for b in range(len(rows))],
                                            inc_continuous=1 if Z is not None else 0, n_groups=int(ds.n_levels[cov]))
        glm = (coeff, t_pvalues(coeff, se, dof))
    vd = None
    if a.variance_decomposition:
        from .posthoc import vd_derived
        d = vd_derived(ds.variance_decomposition(list(res["row_matrices"].values()), res["column_factor"], entries="train",
                                                 inc_continuous=1 if Z is not None else 0))
        vd = {"vd_r2": d["r2"], "vd_rmse": d["rmse"], "vd_explained": d["explained"], "vd_drop_one": d["drop_one"]}
    if a.sample_decomposition:
        from .posthoc import level_decomposition, vd_derived
        rec = ds.sample_decomposition(list(res["row_matrices"].values()), res["column_factor"], entries="train",
                                      inc_continuous=1 if Z is not None else 0)
        d = vd_derived(rec)
        vd = dict(vd or {}, sd_r2=d["r2"], sd_rmse=d["rmse"], sd_explained=d["explained"], sd_drop_one=d["drop_one"])
        for b in range(ds.c):
            lv = level_decomposition(rec, ds_levels[:, b], int(ds.n_levels[b]))
            vd[f"sd_level{b}_r2"], vd[f"sd_level{b}_rmse"] = lv["r2"], lv["rmse"]
    if a.factor_decomposition:
        from .posthoc import factor_summary, fd_derived
        rec = ds.factor_decomposition(list(res["row_matrices"].values()), res["column_factor"], entries="train",
                                      inc_continuous=1 if Z is not None else 0)
        d, fs = fd_derived(rec), factor_summary(rec)
        vd = dict(vd or {}, fd_summary_explained=fs["explained"], fd_summary_drop_one=fs["drop_one"],
                  fd_order=fs["order"].astype(np.float64), fd_explained=d["explained"].reshape(-1, p).T,
                  fd_drop_one=d["drop_one"].reshape(-1, p).T)
    if a.outliers is not None:
        from .posthoc import residual_center_scale
        rows_, inc = list(res["row_matrices"].values()), 1 if Z is not None else 0
        ce, sc = residual_center_scale(ds.variance_decomposition(rows_, res["column_factor"], entries=a.outlier_entries,
                                                                 inc_continuous=inc))
        ol = ds.outliers(rows_, res["column_factor"], sc, center=ce, threshold=a.outliers, entries=a.outlier_entries,
                         inc_continuous=inc)
        vd = dict(vd or {}, ol_rows=ol["rows"], ol_cols=ol["cols"], ol_z=ol["z"],
                  ol_gene_counts=np.column_stack([ol["gene_low"], ol["gene_high"]]),
                  ol_sample_counts=np.column_stack([ol["sample_low"], ol["sample_high"]]))
    if a.level_scores is not None:
        from .posthoc import ls_derived
        cov = a.level_scores - 1
        ls = ls_derived(ds.level_scores(list(res["row_matrices"].values()), res["column_factor"], cov,
                                        entries=a.level_score_entries, inc_continuous=1 if Z is not None else 0),
                        ds_levels[:, cov])
        vd = dict(vd or {}, ls_sse=ls["sse"], ls_n=ls["n"], ls_best=ls["best"].astype(np.float64), ls_margin=ls["margin"],
                  ls_confusion=ls["confusion"].astype(np.float64))
    if a.residual_components is not None:
        from .posthoc import component_associations, residual_components_resident
        rcs = residual_components_resident(ds, list(res["row_matrices"].values()), res["column_factor"],
                                           1 if Z is not None else 0, r=a.residual_components, entries=a.rc_entries,
                                           standardize=a.rc_standardize, seed=a.seed)
        vd = dict(vd or {}, rc_sv=rcs["sv"], rc_share=rcs["share"], rc_sample_scores=rcs["sample_scores"],
                  rc_gene_loadings=rcs["gene_loadings"], rc_assoc=component_associations(rcs["sample_scores"], ds_levels, Z))
    if a.gene_neighbors is not None:
        from .posthoc import gene_neighbors
        nn = gene_neighbors(res["column_factor"], k=a.gene_neighbors, metric=a.neighbor_metric, device=a.device)
        vd = dict(vd or {}, nn_gene_index=nn["index"], nn_gene_score=nn["score"])
    if a.sample_neighbors is not None:
        from .posthoc import sample_neighbors
        nn = sample_neighbors(list(res["row_matrices"].values()), ds_levels, Z, k=a.sample_neighbors, metric=a.neighbor_metric,
                              device=a.device)
        vd = dict(vd or {}, nn_sample_index=nn["index"], nn_sample_score=nn["score"])
    pairwise = a.coexpression_missing == "pairwise"

    def coexpression(axis, k, **kw):
        """The cx_<axis>_* records of one axis: the zero-filled call, or the pairwise-complete one with its overlap."""
        rows_, inc = list(res["row_matrices"].values()), 1 if Z is not None else 0
        if pairwise:
            cx = ds.coexpression_pairwise(rows_, res["column_factor"], axis=axis + "s", k=k, entries="train", inc_continuous=inc,
                                          min_overlap=a.coexpression_min_overlap, **kw)
        else:
            cx = ds.coexpression(rows_, res["column_factor"], axis=axis + "s", k=k, entries="train", inc_continuous=inc, **kw)
        return {f"cx_{axis}_{name}": v for name, v in cx.items()}

    if a.gene_coexpression is not None:
        vd = dict(vd or {}, **coexpression("gene", a.gene_coexpression))
    if a.sample_coexpression is not None:
        from .posthoc import residual_center_scale
        rows_, inc = list(res["row_matrices"].values()), 1 if Z is not None else 0
        ce, sc = residual_center_scale(ds.variance_decomposition(rows_, res["column_factor"], entries="train", inc_continuous=inc))
        vd = dict(vd or {}, **coexpression("sample", a.sample_coexpression, center=ce, scale=sc))
    km_gene = None
    km = dict(metric=a.cluster_metric, restarts=a.cluster_restarts, max_iter=a.cluster_iters, seed=a.cluster_seed, device=a.device)
    if a.gene_modules is not None:
        from .posthoc import gene_modules
        km_gene = gene_modules(res["column_factor"], a.gene_modules, **km)
        vd = dict(vd or {}, **km_records("km_gene", km_gene))
    if a.sample_clusters is not None:
        from .posthoc import sample_clusters
        vd = dict(vd or {}, **km_records("km_sample", sample_clusters(list(res["row_matrices"].values()), ds_levels, Z,
                                                                      k=a.sample_clusters, **km)))
    ts = dict(perplexity=a.map_perplexity, k=a.map_neighbors, max_iter=a.map_iters, seed=a.map_seed, device=a.device)
    if a.gene_map:
        from .posthoc import gene_map
        vd = dict(vd or {}, **ts_records("ts_gene", gene_map(res["column_factor"], **ts)))
    if a.sample_map:
        from .posthoc import sample_map
        vd = dict(vd or {}, **ts_records("ts_sample", sample_map(list(res["row_matrices"].values()), ds_levels, Z, **ts)))
    hc_gene = None

    def hc_records(prefix, rec):
        """The hc_<axis>_* records of one tree, with the labels of --tree-cut."""
        out = {f"{prefix}_{name}": rec[name] for name in ("merge", "height", "size", "order")}
        if a.tree_cut is not None:
            from .posthoc import cut_tree
            if a.tree_cut > rec["alive"]:
                raise SystemExit(f"--tree-cut {a.tree_cut}: the {prefix[3:]} tree has {rec['alive']} leaves")
            out[f"{prefix}_label"] = cut_tree(rec, k=a.tree_cut)
        return out

    if a.gene_tree:
        from .posthoc import gene_tree
        hc_gene = gene_tree(res["column_factor"], metric=a.tree_metric or "cosine", device=a.device)
        vd = dict(vd or {}, **hc_records("hc_gene", hc_gene))
    if a.sample_tree:
        from .posthoc import sample_tree
        vd = dict(vd or {}, **hc_records("hc_sample", sample_tree(list(res["row_matrices"].values()), ds_levels, Z,
                                                                  metric=a.tree_metric or "cosine", device=a.device)))
    gs_names = None
    if a.gene_sets is not None:
        from .posthoc import factor_enrichment, level_enrichment
        gene_names = None
        if a.gene_names is not None:
            with open(a.gene_names) as f:
                gene_names = [ln.strip() for ln in f if ln.strip()]
            if len(gene_names) != p:
                raise SystemExit(f"--gene-names: {len(gene_names)} names for {p} genes")
        sets = flatio.read_gmt(a.gene_sets, gene_names, min_size=a.enrich_min_size, max_size=min(a.enrich_max_size, p - 1))
        if not sets[0]:
            raise SystemExit("--gene-sets: no set is left within the size window")
        gs_names = sets[0]
        keys = ("es", "nes", "pval", "fdr", "peak")
        gs = factor_enrichment(res["column_factor"], sets, nperm=a.enrich_perms, seed=a.seed, device=a.device)
        vd = dict(vd or {}, gs_size=gs["size"], **{f"gs_factor_{k}": gs[k] for k in keys})
        if a.enrich_levels is not None:
            gs = level_enrichment(list(res["row_matrices"].values())[a.enrich_levels - 1], res["column_factor"], sets,
                                  nperm=a.enrich_perms, seed=a.seed, device=a.device)
            vd.update({f"gs_level{a.enrich_levels}_{k}": gs[k] for k in keys})
        if km_gene is not None:
            from .posthoc import module_overrepresentation
            ora = module_overrepresentation(km_gene["label"], sets, k=a.gene_modules)
            vd.update(km_gene_overlap=ora["overlap"], km_gene_hyper_p=ora["hyper_p"], km_gene_hyper_fdr=ora["hyper_fdr"])
        if hc_gene is not None and a.tree_cut is not None:
            from .posthoc import tree_overrepresentation
            ora = tree_overrepresentation(hc_gene, a.tree_cut, sets)
            vd.update(hc_gene_overlap=ora["overlap"], hc_gene_hyper_p=ora["hyper_p"], hc_gene_hyper_fdr=ora["hyper_fdr"])
    ds.close()
    summary = dict(train_rmse=res["train_rmse"], test_rmse=None if np.isnan(res["test_rmse"]) else res["test_rmse"],
                   loss=res["loss"], iters=res["iters"], rank=K, **{"lambda": a.lam}, alpha=a.alpha, partition=partition,
                   n=n, p=p, n_levels=[int(v) for v in ds.n_levels], traj=np.where(np.isnan(res["traj"]), None, res["traj"]).tolist())
    flatio.write_result(a.out, fmt, list(res["row_matrices"].values()), res["column_factor"], summary)
    if glm is not None:
        for name, v in zip(("interaction_coeff", "interaction_pval"), glm):
            if fmt == "npy":
                np.save(os.path.join(a.out, name + ".npy"), np.asfortranarray(v))
            else:
                flatio.write_raw(os.path.join(a.out, name + ".f64"), v)
    flatio.write_records(a.out, fmt, vd or {})
    if gs_names is not None:
        with open(os.path.join(a.out, "gs_set_names.txt"), "w") as f:
            f.write("".join(name + "\n" for name in gs_names))
    print(json.dumps({k: summary[k] for k in ("train_rmse", "test_rmse", "loss", "iters")} | {"out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
