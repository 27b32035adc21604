"""Host-side checks of the agglomerative clustering call (insider_hip_hclust): the numpy yardstick posthoc.hclust_host() builds
the tree scipy's linkage builds, the tie rule orders exact ties, dead points and degenerate sizes give the documented padding,
the round function's no-pair guard works on a hand-made state, cut_tree() and the leaf order are consistent with the merges,
api.hclust_args() refuses every bad argument before it reaches the library, the driver's flags parse, and the header, the
symbol table, the source hash and the Python-side size constant agree.  The error bounds are derived in tests/hclust_cases.py."""
import os
import re

import numpy as np
import pytest

from insider_amd import _build, _lib, api, fit, posthoc
from tests import hclust_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def members(rec, N):
    """The point set under every id of a record."""
    under = {i: [i] for i in range(N)}
    for r in range(rec["alive"] - 1):
        under[N + r] = under[int(rec["merge"][r, 0])] + under[int(rec["merge"][r, 1])]
    return under


# ---- the yardstick against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("D", [1, 3, 30])
@pytest.mark.parametrize("N", [2, 3, 17, 300])
def test_yardstick_builds_scipys_tree(N, D, metric):
    """Child pairs and sizes identical, heights within scipy_bound().  Where scipy's own heights tie exactly the tree is not
    unique (cosine with D = 1: every point is +1 or -1 and every distance 0 or 2) and scipy's order among the ties is its
    own: there the heights and every cut between two distinct heights are compared instead of the rows."""
    linkage = pytest.importorskip("scipy.cluster.hierarchy").linkage
    P = hc.planted(N, D, hc.seed_of(N, D))
    rec = posthoc.hclust_host(P, metric)
    Z = linkage(P.T, method=hc.SCIPY_METHOD[metric], metric=metric)
    assert rec["alive"] == N and rec["merge"].shape == (N - 1, 2)
    dz, do = hc.linkage_d(metric, Z[:, 2]), hc.linkage_d(metric, rec["height"])
    bound = hc.scipy_bound(metric, D, N, rec["scale"], dz)
    print(f"N={N} D={D} {metric}: max error / bound = {np.max(np.abs(do - dz) / bound):.3g}, rounds {rec['rounds']}, "
          f"queries / N = {rec['queries'] / N:.2f}")
    assert np.all(np.abs(do - dz) <= bound)
    if np.all(np.diff(Z[:, 2]) > 0):
        assert np.array_equal(rec["merge"], np.sort(Z[:, :2].astype(np.int64), axis=1))
        assert np.array_equal(rec["size"], Z[:, 3].astype(np.int64))
    else:
        fcluster = pytest.importorskip("scipy.cluster.hierarchy").fcluster
        levels = np.unique(Z[:, 2])
        for lo, hi in zip(levels[:-1], levels[1:]):
            mine, theirs = posthoc.cut_tree(rec, height=(lo + hi) / 2), fcluster(Z, (lo + hi) / 2, criterion="distance")
            pairs = {(int(a), int(b)) for a, b in zip(mine, theirs)}
            assert len(pairs) == len(set(mine.tolist())) == len(set(theirs.tolist()))      # the same partition


# ---- the tie rule ------------------------------------------------------------------------------------------------------------
def test_exact_ties_merge_in_ascending_order():
    P = hc.ties()
    rec = posthoc.hclust_host(P, "euclidean")
    nz = len(hc.TIE_ZERO)
    assert np.array_equal(rec["height"][:nz], np.zeros(nz)) and rec["height"][nz] > 0
    assert [tuple(r) for r in rec["merge"][:nz].tolist()] == hc.TIE_ZERO          # ascending a; the triple as ((0, 5), 9)
    assert rec["size"][:nz].tolist() == [2] * (nz - 1) + [3]
    assert np.all(np.diff(rec["height"]) >= 0) and rec["size"][-1] == 16


# ---- dead points and degenerate sizes ----------------------------------------------------------------------------------------
def test_dead_points_are_in_no_cluster():
    P = hc.planted(12, 3, 5)
    dead = [2, 7, 11]
    P[:, dead] = 0.0
    rec = posthoc.hclust_host(P, "cosine")
    assert rec["alive"] == 9
    assert np.all(rec["merge"][8:] == -1) and np.all(np.isnan(rec["height"][8:])) and np.all(rec["size"][8:] == -1)
    assert np.all(rec["merge"][:8] >= 0) and rec["size"][7] == 9
    assert rec["order"][9:].tolist() == dead and sorted(rec["order"].tolist()) == list(range(12))
    assert not set(dead) & set(rec["merge"][:8].ravel().tolist())
    alive = np.delete(np.arange(12), dead)
    sub = posthoc.hclust_host(P[:, alive], "cosine")                             # the same tree over the alive points alone
    assert np.array_equal(sub["height"], rec["height"][:8]) and np.array_equal(sub["size"], rec["size"][:8])
    assert np.array_equal(alive[sub["order"]], rec["order"][:9])
    assert posthoc.cut_tree(rec, k=2)[dead].tolist() == [-1, -1, -1]
    assert posthoc.hclust_host(P, "euclidean")["alive"] == 12                    # every point is alive under Euclid


@pytest.mark.parametrize("metric", hc.METRICS)
def test_one_point_and_no_point_give_no_merge(metric):
    rec = posthoc.hclust_host(np.ones((3, 1)), metric)
    assert rec["merge"].shape == (0, 2) and rec["height"].shape == (0,) and rec["order"].tolist() == [0]
    assert (rec["alive"], rec["rounds"], rec["queries"]) == (1, 0, 0)
    if metric == "cosine":
        rec = posthoc.hclust_host(np.zeros((3, 4)), metric)                      # all dead
        assert rec["alive"] == 0 and rec["rounds"] == 0 and np.all(rec["merge"] == -1) and rec["order"].tolist() == [0, 1, 2, 3]
        P = np.zeros((3, 4))
        P[:, 2] = 1.0                                                             # one alive point among dead ones
        rec = posthoc.hclust_host(P, metric)
        assert rec["alive"] == 1 and np.all(rec["merge"] == -1) and rec["order"].tolist() == [2, 0, 1, 3]


# ---- rounds ------------------------------------------------------------------------------------------------------------------
def test_the_chain_takes_many_rounds_and_finishes():
    linkage = pytest.importorskip("scipy.cluster.hierarchy").linkage
    P = hc.chain()
    rec = posthoc.hclust_host(P, "euclidean")
    assert rec["rounds"] >= 10 and rec["size"][-1] == 40
    assert rec["queries"] < 40 * rec["rounds"] / 2                               # stale clusters only, not everybody every round
    Z = linkage(P.T, method="ward")
    assert np.array_equal(rec["merge"], np.sort(Z[:, :2].astype(np.int64), axis=1))
    with pytest.raises(api.InsiderError) as e:
        posthoc.hclust_host(P, "euclidean", max_rounds=rec["rounds"] - 1)
    assert e.value.status == _lib.ERR_UNFINISHED
    assert posthoc.hclust_host(P, "euclidean", max_rounds=rec["rounds"])["rounds"] == rec["rounds"]


@pytest.mark.parametrize("code", [0, 1])
def test_a_round_without_a_pair_merges_nothing_and_the_forced_round_does(code):
    """A hand-made state no run reaches in exact arithmetic: nobody is stale, and the stored neighbours form a cycle, so no
    two clusters name each other.  The round merges nothing and asks nobody; the forced round asks everybody and merges."""
    X, alive = posthoc.hclust_points(np.array([[1.0, 2.0, 4.0, 8.0], [0.5, 0.1, 0.3, 0.2]]), code)
    st = posthoc.hclust_state(X, alive)
    st["nn"][:4] = [1, 2, 3, 0]
    assert posthoc.hclust_round(st, code) == 0
    assert (st["rounds"], st["queries"]) == (1, 0) and st["nn"][:4].tolist() == [1, 2, 3, 0] and st["alive"][:4].all()
    assert posthoc.hclust_round(st, code, force=True) >= 1
    assert (st["rounds"], st["queries"]) == (2, 4) and st["alive"].sum() < 4
    a, b = st["ra"][0], st["rb"][0]
    assert a < b and not st["alive"][a] and not st["alive"][b] and st["alive"][4] and st["nn"][4] == -1
    assert np.array_equal(st["S"][4], st["S"][a] + st["S"][b]) and st["n"][4] == 2


# ---- host helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", hc.METRICS)
def test_cut_tree_and_leaf_order(metric):
    N = 60
    rec = posthoc.hclust_host(hc.planted(N, 5, 9, centres=4), metric)
    assert posthoc.cut_tree(rec, k=1).tolist() == [0] * N
    assert posthoc.cut_tree(rec, k=N).tolist() == list(range(N))
    under = members(rec, N)
    for k in (2, 4, 7):
        lab = posthoc.cut_tree(rec, k=k)
        assert sorted(set(lab.tolist())) == list(range(k))
        first = [int(np.flatnonzero(lab == j)[0]) for j in range(k)]
        assert first == sorted(first)                                            # 0-based by the lowest member's index
        h = (rec["height"][N - k - 1] + rec["height"][N - k]) / 2
        assert np.array_equal(posthoc.cut_tree(rec, height=h), lab)
        roots = set(range(N + N - 1 - (k - 1))) - set(rec["merge"][:N - k].ravel().tolist())   # ids the first N - k rows leave
        assert sorted(sorted(under[c]) for c in roots) == sorted(np.flatnonzero(lab == j).tolist() for j in range(k))
    assert posthoc.cut_tree(rec, height=-1.0).tolist() == list(range(N))
    assert posthoc.cut_tree(rec, height=rec["height"][-1]).tolist() == [0] * N
    for bad in (dict(), dict(k=2, height=1.0), dict(k=0), dict(k=N + 1), dict(k=2.5)):
        with pytest.raises(api.InsiderError):
            posthoc.cut_tree(rec, **bad)
    order = rec["order"].tolist()
    assert sorted(order) == list(range(N))
    where = np.argsort(rec["order"])
    for r in range(N - 1):
        at = np.sort(where[under[N + r]])
        assert at[-1] - at[0] == len(at) - 1                                     # the members of every merge are contiguous
        lo, hi = (where[under[int(c)]] for c in rec["merge"][r])
        assert lo.max() < hi.min()                                               # the lower id's leaves come first
    sets = (np.array([0, 10, 30]), np.arange(30))
    ora = posthoc.tree_overrepresentation(rec, 4, sets)
    ref = posthoc.module_overrepresentation(posthoc.cut_tree(rec, k=4), sets, k=4)
    assert ora["overlap"].shape == (4, 2) and np.array_equal(ora["overlap"], ref["overlap"])


def test_hclust_args_refuses_bad_arguments():
    P = hc.planted(10, 3, 1)
    Q, m, l, r = api.hclust_args(P, "cosine", None, None)
    assert (m, l, r) == (0, 0, 20) and Q.flags.f_contiguous
    assert api.hclust_args(P, "euclidean", None, 5)[1:] == (1, 1, 5)
    assert api.hclust_args(P, "euclidean", "ward", None)[1:] == (1, 1, 20)
    nan, inf = P.copy(), P.copy()
    nan[1, 4], inf[0, 0] = np.nan, np.inf
    for args in ((np.zeros((64, 5)) + 1, "cosine", None, None), (np.zeros((0, 5)), "cosine", None, None),
                 (np.zeros((3, 0)), "cosine", None, None), (np.zeros(5), "cosine", None, None), (nan, "cosine", None, None),
                 (inf, "euclidean", None, None), (P, "cosine", "ward", None), (P, "euclidean", "average", None),
                 (P, "dot", None, None), (P, "cosine", "single", None), (P, "euclidean", "centroid", None),
                 (P, "cosine", None, 0), (P, "cosine", None, -3), (P, "cosine", None, 1.5), (P, "cosine", None, True)):
        with pytest.raises(api.InsiderError) as e:
            api.hclust_args(*args)
        assert e.value.status == _lib.ERR_ARG
    for combo in (("cosine", "ward"), ("euclidean", "average")):
        with pytest.raises(api.InsiderError, match=combo[0]) as e:                 # refused by name
            api.hclust_args(P, *combo, None)
        assert combo[1] in str(e.value)
    assert api.hclust_args(np.ones((63, 2)), "cosine", None, None)[0].shape == (63, 2)


# ---- the driver --------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_tree_options():
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    a = fit.parse(base + ["--gene-tree", "--sample-tree", "--tree-metric", "euclidean", "--tree-cut", "12"])
    assert (a.gene_tree, a.sample_tree, a.tree_metric, a.tree_cut) == (True, True, "euclidean", 12)
    a = fit.parse(base + ["--gene-tree"])
    assert (a.gene_tree, a.sample_tree, a.tree_metric, a.tree_cut) == (True, False, None, None)
    a = fit.parse(base)
    assert not a.gene_tree and not a.sample_tree
    for extra in (["--tree-metric", "cosine"], ["--tree-cut", "3"], ["--gene-tree", "--tree-metric", "dot"],
                  ["--gene-tree", "--tree-cut", "0"], ["--sample-tree", "--tree-cut", "-2"]):
        with pytest.raises(SystemExit):
            fit.parse(base + extra)
    with pytest.raises(SystemExit):
        fit.parse(["--x", "X.npy", "--levels", "L.npy", "--tune", "--gene-tree"])


# ---- the contract ------------------------------------------------------------------------------------------------------------
def test_header_symbols_sources_and_constants_agree():
    hdr = " ".join(open(os.path.join(ROOT, "include", "insider_hip.h")).read().split())
    assert "int insider_hip_hclust(" in hdr and "double insider_hip_last_hclust_ms(void)" in hdr
    assert "insider_hip_hclust" in _lib.SYMBOLS and "insider_hip_last_hclust_ms" in _lib.SYMBOLS
    assert re.search(r"#define INSIDER_ERR_UNFINISHED (\d+)", hdr).group(1) == str(_lib.ERR_UNFINISHED)
    kernels = os.path.join(ROOT, "insider_amd", "csrc", "insider_hclust.hpp")
    assert kernels in _build.source_files()
    src = open(kernels).read()
    assert int(re.search(r"constexpr int HC_MAX_D = (\d+);", src).group(1)) == api.HCLUST_MAX_D
    assert '#include "insider_hclust.hpp"' in open(os.path.join(ROOT, "insider_amd", "csrc", "insider_hip.hip")).read()
    for word in ("single", "complete", "centroid", "median", "reducible"):       # the header says what is not offered, and why
        assert word in hdr.lower(), word
