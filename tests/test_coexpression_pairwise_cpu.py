"""The pairwise-complete co-expression without a device: the numpy yardsticks posthoc.gram_topk_pairwise_host() and
coexpression_host(missing="pairwise") against a brute-force Pearson's r, the eligibility rules at their edges, the argument
checks of the Python wrappers, the command line's flags and the contract on the source tree.

reference() is shared with tests/test_gpu_coexpression_pairwise.py; its tolerance is derived there."""
import os
import re

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from insider_amd import fit as fit_cli
from tests.support import problem
from tests.test_gpu_neighbors import check_rule3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("insider_hip_gram_topk_pairwise", "insider_hip_coexpression_pairwise")


def reference(R, sel, min_overlap):
    """Of the vectors R (depth x N) with the boolean selection sel, by the definition of include/insider_hip.h on the
    standardised values: the float64 score of every pair, its tolerance T = 4 (3 D + 16) 2^-52 (kappa_a + kappa_b) with
    kappa = Saa / va of the pair, who may be whose partner, the pairs' joint counts, and kappa_a, kappa_b (N x N each)."""
    depth, N = R.shape
    Z, alive = posthoc._gram_standardise(R, sel, 0)
    M = (np.asarray(sel, dtype=bool) & alive[None, :]).astype(np.float64)
    t = posthoc._pairwise_sums(Z, M, alive, min_overlap, 0, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        ka, kb = t["Saa"] / t["va"], t["Sbb"] / t["vb"]
        T = 4.0 * (3 * depth + 16) * 2.0 ** -52 * (ka + kb)
    # (a pair that is not eligible has no score to compare: 0 and an infinite tolerance keep NaN out of check_rule3)
    return np.where(t["eligible"], t["score"], 0.0), np.where(t["eligible"], T, np.inf), t["eligible"], t["N"], ka, kb


def vectors(depth, N, missing, seed, shift=3.0):
    """depth x N normal vectors, a tenth scaled down and a tenth up by 10^3, a fifth moved off zero by ``shift`` standard
    deviations; NaN in a share ``missing`` of the entries."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((depth, N))
    V[:, rng.random(N) < 0.1] *= 1e-3
    V[:, rng.random(N) < 0.1] *= 1e3
    moved = rng.random(N) < 0.2
    V[:, moved] += shift * V[:, moved].std(axis=0)
    if missing:
        V[rng.random((depth, N)) < missing] = np.nan
    return np.asfortranarray(V)


def brute_force(V, a, b):
    """Pearson's r of the columns a and b over their joint entries: two passes in long double on the raw values."""
    J = ~np.isnan(V[:, a]) & ~np.isnan(V[:, b])
    x, y = V[J, a].astype(np.longdouble), V[J, b].astype(np.longdouble)
    x, y = x - x.sum() / x.size, y - y.sum() / y.size
    return float((x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum())), int(J.sum())


@pytest.mark.parametrize("case", [(37, 40, 0.3, 3.0), (37, 40, 0.6, 3.0), (65, 30, 0.3, 1e4), (90, 25, 0.0, 3.0)])
def test_yardstick_matches_a_brute_force_pearson(case):
    depth, N, missing, shift = case
    V = vectors(depth, N, missing, 11 * depth + N, shift)
    k, mo = min(N - 1, 64), 5
    got = posthoc.gram_topk_pairwise_host(V, k=k, min_overlap=mo)
    sel = ~np.isnan(V)
    S, T, elig, Nn, _, _ = reference(np.where(sel, V, 0.0), sel, mo)
    check_rule3(got, S, T, k, elig)
    assert got["overlap"].dtype == np.int32 and np.array_equal(got["overlap"] < 0, got["index"] < 0)
    worst, seen = 0.0, 0
    for a in range(N):
        for slot in range(k):
            b = got["index"][a, slot]
            if b < 0:
                continue
            want, n_joint = brute_force(V, a, b)
            assert got["overlap"][a, slot] == n_joint == Nn[a, b] and n_joint >= mo
            worst = max(worst, abs(got["score"][a, slot] - want) / T[a, b])
            seen += 1
    print("pairs", seen, "max error / T", worst)
    assert seen > N and worst <= 1.0
    # every pair left out is one the rules exclude
    for a in range(N):
        listed = set(got["index"][a][got["index"][a] >= 0])
        if len(listed) == k:
            continue
        for b in set(range(N)) - listed - {a}:
            assert not elig[a, b]


def test_pairwise_differs_from_zero_filled():
    """The figure of the issue: on 37 x 40 data with 30 % missing the two scores of a pair differ by tenths."""
    V = vectors(37, 40, 0.3, 5)
    sel = ~np.isnan(V)
    S, _, elig, _, _, _ = reference(np.where(sel, V, 0.0), sel, 3)
    W, _ = posthoc._gram_standardise(np.where(sel, V, 0.0), sel, 0)
    assert np.max(np.abs(S - W.T @ W)[elig]) > 0.1


def edge_vectors():
    """depth 12.  0: entries 0..6; 1: entries 2..11 (joint with 0: five); 2: everywhere, constant on 0..6 and varying on
    7..11 (constant on its joint set with 0, not on its own entries, nor on its joint set with 1); 3: all missing;
    4: one entry; 5: everywhere."""
    rng = np.random.default_rng(3)
    V = np.full((12, 6), np.nan, order="F")
    V[0:7, 0] = rng.standard_normal(7)
    V[2:12, 1] = rng.standard_normal(10)
    V[:, 2] = 2.0
    V[7:12, 2] = rng.standard_normal(5)
    V[4, 4] = 1.5
    V[:, 5] = rng.standard_normal(12)
    return V


def partners(got, a):
    return {int(b): int(n) for b, n in zip(got["index"][a], got["overlap"][a]) if b >= 0}


def test_eligibility_at_its_edges():
    V = edge_vectors()
    at = posthoc.gram_topk_pairwise_host(V, k=5, min_overlap=5)        # the overlap of 0 and 1 is exactly min_overlap
    below = posthoc.gram_topk_pairwise_host(V, k=5, min_overlap=6)     # ... and exactly min_overlap - 1
    assert partners(at, 0) == {1: 5, 5: 7} and partners(at, 1) == {0: 5, 2: 10, 5: 10}
    assert partners(below, 0) == {5: 7} and partners(below, 1) == {2: 10, 5: 10}
    # 2 is constant where 0 has entries: no pair with 0, but it is alive and pairs with 1 and 5
    assert partners(at, 2) == {1: 10, 5: 12}
    for got in (at, below):
        for dead in (3, 4):                                            # all missing; one entry
            assert np.all(got["index"][dead] == -1) and np.all(np.isnan(got["score"][dead])) and np.all(got["overlap"][dead] == -1)
            assert not np.isin(got["index"], dead).any()
    # min_overlap above the depth: every row open
    none = posthoc.gram_topk_pairwise_host(V, k=5, min_overlap=13)
    assert np.all(none["index"] == -1) and np.all(np.isnan(none["score"])) and np.all(none["overlap"] == -1)
    # the default is max(3, ceil(depth / 4))
    assert api.pairwise_min_overlap(None, 12) == 3 and api.pairwise_min_overlap(None, 13) == 4 and api.pairwise_min_overlap(None, 1) == 3
    # a window lists the rows of the full call (the host's products may round differently from shape to shape)
    full = posthoc.gram_topk_pairwise_host(V, k=5)
    part = posthoc.gram_topk_pairwise_host(V, k=5, first=1, count=2)
    assert np.array_equal(part["index"], full["index"][1:3]) and np.array_equal(part["overlap"], full["overlap"][1:3])
    assert np.allclose(part["score"], full["score"][1:3], rtol=0, atol=1e-14, equal_nan=True)


@pytest.mark.parametrize("shape", [(37, 70), (300, 25)])
def test_nothing_missing_agrees_with_the_correlation_yardstick(shape):
    from tests.test_gpu_gram_topk import COR, reference_scores
    depth, N = shape
    V = vectors(depth, N, 0.0, 7 * depth + N)
    S, T, elig = reference_scores(V, COR)                               # tests/test_gpu_gram_topk.py's correlation tolerance
    for k in (1, 10):
        got = posthoc.gram_topk_pairwise_host(V, k=k, min_overlap=3)
        check_rule3(got, S, T, k, elig)
        assert np.all(got["overlap"] == depth)


def test_coexpression_host_pairwise_keyword():
    X, lev, Z, mask, A, Cm = problem(4, 30, 22, (3, 2), 0, 3)
    zero = posthoc.coexpression_host(X, lev, Z, mask, A, Cm, "genes", 5)
    assert set(zero) == {"index", "score"}                              # the default is unchanged
    assert all(np.array_equal(zero[n], posthoc.coexpression_host(X, lev, Z, mask, A, Cm, "genes", 5, missing="zero")[n],
                              equal_nan=True) for n in zero)
    r, w = posthoc.coexpression_residual_host(X, lev, Z, mask, A, Cm)
    for axis, (R, sel) in (("genes", (r, w)), ("samples", (r.T, w.T))):
        got = posthoc.coexpression_host(X, lev, Z, mask, A, Cm, axis, 5, missing="pairwise")
        want = posthoc.gram_topk_pairwise_host(np.where(sel, R, np.nan), k=5)
        for name in ("index", "score", "overlap"):
            assert np.array_equal(got[name], want[name], equal_nan=True), (axis, name)
        few = posthoc.coexpression_host(X, lev, Z, mask, A, Cm, axis, 5, missing="pairwise", min_overlap=R.shape[0] + 1)
        assert np.all(few["index"] == -1)
    with pytest.raises(ValueError):
        posthoc.coexpression_host(X, lev, Z, mask, A, Cm, "genes", 5, missing="complete")


def test_wrappers_refuse_bad_arguments_without_the_library():
    V = np.random.default_rng(7).standard_normal((9, 12))

    def status(fn, *a, **kw):
        with pytest.raises(_lib.InsiderError) as e:
            fn(*a, **kw)
        return e.value.status

    bad, args = _lib.ERR_ARG, api.gram_topk_pairwise_args
    assert status(args, V[0], 3, None, 0, None) == bad                  # not two-dimensional
    assert status(args, np.zeros((0, 4)), 3, None, 0, None) == bad
    assert status(args, np.zeros((4, 0)), 3, None, 0, None) == bad
    for k in (0, 65, -1, 2.0, True):
        assert status(args, V, k, None, 0, None) == bad
    for mo in (2, 0, -1, 3.0, True, "3"):
        assert status(args, V, 3, mo, 0, None) == bad
        assert status(api.pairwise_min_overlap, mo, 9) == bad
    for first, count in ((-1, 2), (0, -1), (0, 13), (12, 1), (5, 8), (1.0, 2), (0, 2.0)):
        assert status(args, V, 3, None, first, count) == bad
    for val in (np.inf, -np.inf):
        W = V.copy()
        W[4, 11] = val
        assert status(args, W, 3, None, 0, None) == bad
        assert status(api.gram_topk_pairwise, W, k=3) == bad            # refused before the library is touched
    W = V.copy()
    W[4, 11] = np.nan                                                   # a NaN is a missing entry
    Vf, k, mo, first, count = args(W, 3, None, 2, None)
    assert Vf.flags.f_contiguous and (k, mo, first, count) == (3, 3, 2, 10)
    assert args(V, 64, 100, 12, 0)[1:] == (64, 100, 12, 0)               # min_overlap above the depth is allowed
    # posthoc: the keyword is checked before the handle is looked at
    for fn in (posthoc.gene_coexpression, posthoc.sample_coexpression):
        assert "missing" in fn.__code__.co_varnames and "min_overlap" in fn.__code__.co_varnames
    with pytest.raises(ValueError):
        posthoc._coexpression(None, None, None, "genes", 5, "train", 0, "complete", None)
    with pytest.raises(ValueError):
        posthoc._coexpression(None, None, None, "genes", 5, "train", 0, "zero", 4)
    assert "coexpression_pairwise" in api.InsiderData.coexpression.__doc__
    assert api.InsiderData.coexpression_pairwise.__code__.co_varnames[:10] == (
        "self", "cfd_factors", "column_factor", "axis", "k", "min_overlap", "entries", "center", "scale", "inc_continuous")


def test_cli_flags_parse():
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    a = fit_cli.parse(base + ["--gene-coexpression", "10"])
    assert a.coexpression_missing == "zero" and a.coexpression_min_overlap is None
    a = fit_cli.parse(base + ["--gene-coexpression", "10", "--coexpression-missing", "pairwise"])
    assert a.coexpression_missing == "pairwise" and a.coexpression_min_overlap is None
    a = fit_cli.parse(base + ["--sample-coexpression", "4", "--coexpression-missing", "pairwise", "--coexpression-min-overlap", "3"])
    assert a.coexpression_min_overlap == 3
    refused = (
        ["--gene-coexpression", "10", "--coexpression-missing", "complete"],                              # an unknown choice
        ["--coexpression-missing", "pairwise"],                                                          # nothing to apply it to
        ["--gene-coexpression", "10", "--coexpression-min-overlap", "5"],                                 # belongs to pairwise
        ["--gene-coexpression", "10", "--coexpression-missing", "zero", "--coexpression-min-overlap", "5"],
        ["--gene-coexpression", "10", "--coexpression-missing", "pairwise", "--coexpression-min-overlap", "2"],
        ["--gene-coexpression", "10", "--coexpression-missing", "pairwise", "--coexpression-min-overlap", "x"],
    )
    for extra in refused:
        with pytest.raises(SystemExit):
            fit_cli.parse(base + extra)
    for word in ("--coexpression-missing", "--coexpression-min-overlap", "cx_gene_overlap", "cx_sample_overlap", "zero-filled",
                 "pairwise-complete"):
        assert word in fit_cli.__doc__, word


def test_contract_on_the_source_tree():
    hdr = open(os.path.join(ROOT, "include", "insider_hip.h")).read()
    src = open(os.path.join(ROOT, "insider_amd", "csrc", "insider_hip.hip")).read()
    for name in NEW:
        assert re.search(rf"^int {name}\(", hdr, re.M) and re.search(rf"^int {name}\(", src, re.M), name
        assert name in _lib.SYMBOLS
    assert '"cx_pc_ms"' in hdr and 's == "cx_pc_ms"' in src
    from insider_amd import _build
    assert os.path.join(_build.CSRC, "insider_coexpr_pc.hpp") in _build.source_files()
    kern = open(os.path.join(ROOT, "insider_amd", "csrc", "insider_coexpr_pc.hpp")).read()
    for name in ("k_cx_std_pc", "k_cx_topk_pc"):
        assert re.search(rf"\b{name}\b", kern) and re.search(rf"\b{name}\b", src), name
    assert "nn_merge_t<true>(" in kern and "nn_before" not in kern      # the selection is reused, not copied
    assert "atomic" not in kern.replace("No floating-point atomics", "")
    assert re.search(r"constexpr int CXP_BT = \d+;", kern)               # a base step of its own
