"""The numpy yardsticks of the co-expression calls (posthoc.gram_topk_host / coexpression_host), the argument checks of
api.gram_topk_args and the contract on the source tree: no library build, no GPU."""
import os
import re

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from insider_amd import fit as fit_cli
from tests.support import problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(V, k, metric):
    """The definition, one pair at a time: sums in index order, python floats."""
    depth, N = V.shape
    W, alive = np.zeros((depth, N)), np.ones(N, dtype=bool)
    for j in range(N):
        v = [float(x) for x in V[:, j]]
        if metric == "dot":
            W[:, j] = v
            continue
        mean = 0.0
        if metric == "correlation":
            s = 0.0
            for x in v:
                s += x
            mean = s / depth
        ss = 0.0
        for x in v:
            ss += (x - mean) * (x - mean)
        alive[j] = ss > 0
        if alive[j]:
            W[:, j] = [(x - mean) / np.sqrt(ss) for x in v]
    index, score = np.full((N, k), -1, dtype=np.int32), np.full((N, k), np.nan)
    for i in range(N):
        if not alive[i]:
            continue
        cand = [(-(float(W[:, i] @ W[:, j]) + 0.0), j) for j in range(N) if j != i and alive[j]]
        for slot, (neg, j) in enumerate(sorted(cand)[:k]):
            index[i, slot], score[i, slot] = j, -neg
    return dict(index=index, score=score)


@pytest.mark.parametrize("metric", ["correlation", "cosine", "dot"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (2, 7), (9, 40), (33, 17)])
def test_gram_topk_host_against_the_definition(metric, shape):
    depth, N = shape
    rng = np.random.default_rng(depth * 100 + N)
    V = rng.standard_normal((depth, N))
    if N > 4:
        V[:, 3] = 0.0                      # dead under correlation and cosine
        V[:, 4] = 2.5                      # constant: dead under correlation
    for k in (1, 3, 64):
        ref = brute(V, k, metric)
        got = posthoc.gram_topk_host(V, k=k, metric=metric, chunk=7)
        assert np.array_equal(got["index"], ref["index"])
        assert np.allclose(got["score"], ref["score"], rtol=0, atol=1e-13, equal_nan=True)
    win = posthoc.gram_topk_host(V, k=3, metric=metric, first=N // 2, count=N - N // 2)
    full = posthoc.gram_topk_host(V, k=3, metric=metric)
    assert np.array_equal(win["index"], full["index"][N // 2:])
    assert np.allclose(win["score"], full["score"][N // 2:], rtol=0, atol=1e-14, equal_nan=True)   # (BLAS blocks by shape)


def test_tie_rule_and_self_exclusion_on_integer_data():
    rng = np.random.default_rng(5)
    V = rng.integers(-2, 3, (6, 30)).astype(np.float64)
    V[:, 11] = V[:, 2]                                        # duplicates: exactly equal scores
    V[:, 19] = V[:, 2]
    got = posthoc.gram_topk_host(V, k=29, metric="dot")
    ref = brute(V, 29, "dot")
    assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["score"], ref["score"])
    S = V.T @ V
    for i in range(30):
        assert i not in got["index"][i] and sorted(got["index"][i]) == [j for j in range(30) if j != i]
        sc = S[i, got["index"][i]]
        assert np.all(np.diff(sc) <= 0) and np.all(np.diff(got["index"][i])[np.diff(sc) == 0] > 0)
    # all vectors equal: the tie rule alone decides
    got = posthoc.gram_topk_host(np.ones((3, 8)), k=4, metric="dot")
    assert got["index"].tolist() == [[j for j in range(8) if j != i][:4] for i in range(8)]
    # -0.0 == 0.0
    got = posthoc.gram_topk_host(np.array([[1.0, 0.0, -0.0, 0.0, -1.0]]), k=4, metric="dot")
    assert got["index"][0].tolist() == [1, 2, 3, 4] and got["index"][4].tolist() == [1, 2, 3, 0]   # products 0.0 and -0.0 tie


def test_dead_vectors():
    rng = np.random.default_rng(6)
    V = rng.standard_normal((12, 9))
    V[:, 2] = 4.0
    V[:, 5] = 0.0
    cor = posthoc.gram_topk_host(V, k=8, metric="correlation")
    for dead in (2, 5):
        assert np.all(cor["index"][dead] == -1) and np.all(np.isnan(cor["score"][dead])) and dead not in cor["index"]
    assert np.all(cor["index"][0, :6] >= 0) and np.all(cor["index"][0, 6:] == -1)      # 9 - 1 - 2 partners
    cos = posthoc.gram_topk_host(V, k=8, metric="cosine")
    assert np.all(cos["index"][5] == -1) and 5 not in cos["index"] and 2 in cos["index"]
    dot = posthoc.gram_topk_host(V, k=8, metric="dot")
    assert np.all(dot["index"] >= 0)                                                   # nothing is dead under dot
    one = posthoc.gram_topk_host(rng.standard_normal((1, 4)), k=2, metric="correlation")   # depth 1: every centred vector is 0
    assert np.all(one["index"] == -1)


def _case(seed=3, n=24, p=31, K=3, m=2):
    return problem(seed, n, p, (4, 3), m, K, scale=0.4)


def test_full_selection_is_pearson():
    X, lev, Z, _, A, Cm = _case()
    r, w = posthoc.coexpression_residual_host(X, lev, Z, None, A, Cm)
    assert w.all()
    for axis, R in (("genes", r), ("samples", r.T)):
        N = R.shape[1]
        got = posthoc.coexpression_host(X, lev, Z, None, A, Cm, axis, N - 1)
        cc = np.corrcoef(R, rowvar=False)
        rows = np.arange(N)[:, None]
        assert np.all(got["index"] >= 0)
        assert np.max(np.abs(got["score"] - cc[rows, got["index"]])) <= 1e-12
        assert np.all(np.diff(got["score"], axis=1) <= 0)
        for i in range(N):
            assert sorted(got["index"][i]) == [j for j in range(N) if j != i]


def test_masked_scores_stay_within_one_and_dead_rules():
    X, lev, Z, mask, A, Cm = _case(seed=4)
    mask = mask.copy()
    mask[:, 0] = False                     # gene 0: no entry
    mask[:, 1] = False
    mask[5, 1] = True                      # gene 1: m = 1
    mask[2, :] = False                     # sample 2: no entry
    mask[3, :] = False
    mask[3, 7] = True                      # sample 3: m = 1
    sc = np.ones(X.shape[1])
    sc[4], sc[6] = 0.0, np.nan             # bad scales: all-zero columns, dead genes
    for axis, dead in (("genes", (0, 1, 4, 6)), ("samples", (2, 3))):
        N = X.shape[1] if axis == "genes" else X.shape[0]
        got = posthoc.coexpression_host(X, lev, Z, mask, A, Cm, axis, 10, scale=sc)
        ok = np.isfinite(got["score"])
        assert np.all(np.abs(got["score"][ok]) <= 1 + 1e-12)
        for d in dead:
            assert np.all(got["index"][d] == -1) and d not in got["index"]
        alive = [i for i in range(N) if i not in dead]
        assert np.all(got["index"][alive] >= 0)
    # the zero-filled definition, written out for one pair of genes
    got = posthoc.coexpression_host(X, lev, Z, mask, A, Cm, "genes", X.shape[1] - 1)
    r, w = posthoc.coexpression_residual_host(X, lev, Z, mask, A, Cm)
    a, b = 8, 9
    za = np.where(w[:, a], r[:, a] - r[w[:, a], a].mean(), 0.0)
    zb = np.where(w[:, b], r[:, b] - r[w[:, b], b].mean(), 0.0)
    want = za @ zb / np.sqrt((za @ za) * (zb @ zb))
    assert abs(got["score"][a][list(got["index"][a]).index(b)] - want) <= 1e-13


def test_gram_topk_args_refuses_bad_arguments():
    V = np.random.default_rng(7).standard_normal((5, 12))

    def status(*a):
        with pytest.raises(_lib.InsiderError) as e:
            api.gram_topk_args(*a)
        return e.value.status

    bad = _lib.ERR_ARG
    assert status(V[0], 3, "dot", 0, None) == bad                      # not two-dimensional
    assert status(np.zeros((0, 4)), 3, "dot", 0, None) == bad          # depth < 1
    assert status(np.zeros((4, 0)), 3, "dot", 0, None) == bad          # N < 1
    for k in (0, 65, -1, 2.0, True):
        assert status(V, k, "dot", 0, None) == bad
    for metric in ("pearson", 0, None):
        assert status(V, 3, metric, 0, None) == bad
    for first, count in ((-1, 2), (0, -1), (0, 13), (12, 1), (5, 8), (1.0, 2), (0, 2.0)):
        assert status(V, 3, "dot", first, count) == bad
    for val in (np.nan, np.inf, -np.inf):
        W = V.copy()
        W[4, 11] = val
        assert status(W, 3, "dot", 0, None) == bad
    Vf, k, code, first, count = api.gram_topk_args(V, 3, "correlation", 2, None)
    assert Vf.flags.f_contiguous and (k, code, first, count) == (3, 0, 2, 10)
    assert api.gram_topk_args(V, 64, "cosine", 12, 0)[2:] == (1, 12, 0)
    assert api.GRAM_METRICS == {"correlation": 0, "cosine": 1, "dot": 2}


def test_contract_on_the_source_tree():
    hdr = open(os.path.join(ROOT, "include", "insider_hip.h")).read()
    src = open(os.path.join(ROOT, "insider_amd", "csrc", "insider_hip.hip")).read()
    for name in ("insider_hip_gram_topk", "insider_hip_last_gram_topk_ms", "insider_hip_coexpression"):
        assert re.search(rf"^(int|double) {name}\(", hdr, re.M), name
        assert re.search(rf"^(int|double) {name}\(", src, re.M), name
        assert name in _lib.SYMBOLS
    for key in ("cx_stage_mb", "cx_stage_ms", "cx_ms"):
        assert f'"{key}"' in hdr and f's == "{key}"' in src, key
    assert "zero-filled" in hdr.lower() and "pairwise-complete" in hdr
    kern = open(os.path.join(ROOT, "insider_amd", "csrc", "insider_coexpr.hpp")).read()
    for name in ("k_cx_prep", "k_cx_stage", "k_cx_norm", "k_cx_topk"):
        assert re.search(rf"\b{name}\b", kern) and re.search(rf"\b{name}\b", src), name
    assert "nn_merge(" in kern and "nn_before" not in kern.replace("nn_before /", "")      # reused, not copied


def test_cli_flags_parse():
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    a = fit_cli.parse(base + ["--gene-coexpression", "10", "--sample-coexpression", "7"])
    assert (a.gene_coexpression, a.sample_coexpression) == (10, 7)
    a = fit_cli.parse(base)
    assert a.gene_coexpression is None and a.sample_coexpression is None
    for flag in ("--gene-coexpression", "--sample-coexpression"):
        for v in ("0", "65"):
            with pytest.raises(SystemExit):
                fit_cli.parse(base + [flag, v])
        with pytest.raises(SystemExit):
            fit_cli.parse(["--x", "X.npy", "--levels", "L.npy", "--tune", flag, "5"])
    assert "--gene-coexpression" in fit_cli.__doc__ and "cx_sample_index" in fit_cli.__doc__
