"""Host-side checks of the nearest-neighbour call (insider_hip_neighbors): the numpy yardstick posthoc.neighbors_host() agrees
with a brute force over the full score matrix (Python ``sorted`` with the key (-score, index)), api.neighbors() refuses bad
arguments before it reaches the library, posthoc.sample_embeddings() is the explicit sum over the covariate blocks, and the
driver's flags parse and its records round-trip through flatio."""
import math

import numpy as np
import pytest

from insider_amd import _lib, api, fit, flatio, posthoc


def brute(Q, B, k, metric, off):
    """The full score matrix and Python's sort: the ten-line reference of the yardstick."""
    nq, nb = Q.shape[1], B.shape[1]
    idx, sc = np.full((nq, k), -1, dtype=np.int32), np.full((nq, k), np.nan)
    for i in range(nq):
        cand = []
        for j in range(nb):
            s = float(Q[:, i] @ B[:, j])
            if metric == "cosine":
                nq_, nb_ = math.sqrt(float(Q[:, i] @ Q[:, i])), math.sqrt(float(B[:, j] @ B[:, j]))
                if nq_ == 0.0 or nb_ == 0.0:
                    continue
                s = s / (nq_ * nb_)
            if off is not None and j == off + i:
                continue
            cand.append((-s, j))
        for slot, (ms, j) in enumerate(sorted(cand)[:k]):
            idx[i, slot], sc[i, slot] = j, -ms
    return idx, sc


def same(got, idx, sc):
    assert got["index"].dtype == np.int32 and got["score"].dtype == np.float64
    assert np.array_equal(got["index"], idx)
    assert np.array_equal(np.isnan(got["score"]), np.isnan(sc)) and np.array_equal(got["index"] < 0, np.isnan(sc))
    assert np.allclose(got["score"], sc, rtol=0, atol=1e-15, equal_nan=True)


def tiny(seed, K=3, n=9):
    rng = np.random.default_rng(seed)
    B = rng.integers(-2, 3, (K, n)).astype(np.float64)
    B[:, 4] = B[:, 1]          # duplicate columns: equal scores, the lower index first
    B[:, 7] = B[:, 1]
    B[:, 2] = 0.0              # zero columns
    B[:, 6] = 0.0
    return B


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("k", [1, 3, 9, 12])
def test_host_yardstick_matches_brute_force(metric, k):
    B = tiny(1)
    same(posthoc.neighbors_host(B, None, k=k, metric=metric), *brute(B, B, k, metric, 0))               # self call
    same(posthoc.neighbors_host(B, B, k=k, metric=metric, exclude_self=False), *brute(B, B, k, metric, None))
    Q = B[:, 3:7]                                                                                       # a window start
    same(posthoc.neighbors_host(Q, B, k=k, metric=metric, exclude_self=3), *brute(Q, B, k, metric, 3))
    rng = np.random.default_rng(2)
    Q = rng.standard_normal((3, 5))
    same(posthoc.neighbors_host(Q, B, k=k, metric=metric, chunk=2), *brute(Q, B, k, metric, None))      # several chunks


def test_host_yardstick_open_slots_and_signed_zero():
    B = tiny(3)
    got = posthoc.neighbors_host(B, None, k=12, metric="cosine")
    live = [j for j in range(9) if j not in (2, 6)]
    assert np.all(got["index"][[2, 6]] == -1) and np.all(np.isnan(got["score"][[2, 6]]))     # zero-norm queries
    assert not np.isin(got["index"], (2, 6)).any()                                           # zero-norm base columns
    for i in live:
        assert np.sum(got["index"][i] >= 0) == len(live) - 1
    got = posthoc.neighbors_host(B, None, k=12, metric="dot")                                # k >= nb: nb - 1 candidates
    assert np.all(np.sum(got["index"] >= 0, axis=1) == 8) and np.all(got["index"][:, 8:] == -1)
    assert list(got["index"][2][:8]) == [0, 1, 3, 4, 5, 6, 7, 8] and np.all(got["score"][2][:8] == 0.0)
    # -0.0 and 0.0 are one number: the lower index first whichever sign a zero entry carries
    Q = np.array([[1.0]])
    Bz = np.array([[0.0, -0.0, 0.0, -0.0]])
    got = posthoc.neighbors_host(Q, Bz, k=4, metric="dot")
    assert list(got["index"][0]) == [0, 1, 2, 3] and np.all(got["score"][0] == 0.0)
    same(got, *brute(Q, Bz, 4, "dot", None))


def test_wrapper_refuses_bad_arguments():
    B = tiny(4)
    bad = [
        dict(query=B[0]),                                       # not K x nq
        dict(query=B, base=B[:2]),                              # another K
        dict(query=B, base=B[0]),                               # base not 2-D
        dict(query=np.zeros((64, 3))),                          # K > 63
        dict(query=np.zeros((0, 3))),                           # K < 1
        dict(query=B[:, :2], base=np.zeros((3, 0))),            # an empty base
        dict(query=np.zeros((3, 0))),                           # base = the (empty) queries
        dict(query=B, metric="euclidean"),
        dict(query=B, k=0),
        dict(query=B, k=65),
        dict(query=B, k=2.5),
        dict(query=B, k=True),
        dict(query=B[:, :3], base=B, exclude_self=-1),
        dict(query=B[:, :3], base=B, exclude_self=7),           # 7 + 3 > 9
        dict(query=B[:, :3], base=B, exclude_self=1.0),
        dict(query=B[:, :3], base=B, exclude_self=True),
    ]
    for kw in bad:
        for fn in (api.neighbors, posthoc.neighbors_host):
            with pytest.raises(_lib.InsiderError) as e:
                fn(**kw)
            assert e.value.status == _lib.ERR_ARG, kw
    # what is allowed: the last window, and no queries at all
    got = posthoc.neighbors_host(B[:, 6:], B, k=2, exclude_self=6)
    assert got["index"].shape == (3, 2)
    got = api.neighbors(np.zeros((3, 0)), B, k=2)              # (nothing to compute: no device is touched)
    assert got["index"].shape == (0, 2) and got["score"].shape == (0, 2)


def test_sample_embeddings_is_the_sum_over_the_blocks():
    rng = np.random.default_rng(5)
    n, K, counts, m = 13, 4, (3, 5), 2
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    A = [rng.standard_normal((L, K)) for L in counts]
    Bc = rng.standard_normal((m, K))
    Z = rng.standard_normal((n, m))
    for ctns, fac in ((None, A), (Z, A + [Bc])):
        E = posthoc.sample_embeddings(fac, lev, ctns)
        assert E.shape == (K, n) and E.flags.f_contiguous
        for i in range(n):
            want = np.zeros(K)
            for b in range(len(counts)):
                want = want + A[b][lev[i, b] - 1]
            if ctns is not None:
                want = want + sum(Z[i, j] * Bc[j] for j in range(m))
            assert np.allclose(E[:, i], want, rtol=0, atol=1e-14)
    assert posthoc.sample_embeddings([A[0]], lev[:, 0]).shape == (K, n)      # one covariate given as a vector
    with pytest.raises(ValueError):
        posthoc.sample_embeddings(A, lev, Z)                                   # the continuous block's factor is missing
    with pytest.raises(ValueError):
        posthoc.sample_embeddings(A, lev + 5)
    # samples with the same levels share their embedding: sample_neighbors' ties
    E = posthoc.sample_embeddings(A, lev)
    i, j = 0, int(np.flatnonzero((lev == lev[0]).all(axis=1))[-1])
    assert np.array_equal(E[:, i], E[:, j])


def test_cli_parses_the_neighbor_options():
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    a = fit.parse(base + ["--gene-neighbors", "5", "--sample-neighbors", "7", "--neighbor-metric", "dot"])
    assert a.gene_neighbors == 5 and a.sample_neighbors == 7 and a.neighbor_metric == "dot"
    a = fit.parse(base)
    assert a.gene_neighbors is None and a.sample_neighbors is None and a.neighbor_metric == "cosine"
    for extra in (["--neighbor-metric", "euclidean"], ["--gene-neighbors", "0"], ["--sample-neighbors", "65"]):
        with pytest.raises(SystemExit):
            fit.parse(base + extra)


@pytest.mark.parametrize("fmt", ["flat", "npy"])
def test_records_round_trip_through_flatio(tmp_path, fmt):
    B = tiny(6, K=3, n=9)
    E = np.asfortranarray(B[:, :5] + 0.25)
    g, s = posthoc.neighbors_host(B, None, k=10, metric="cosine"), posthoc.neighbors_host(E, None, k=3, metric="dot")
    assert (g["index"] == -1).any() and np.isnan(g["score"]).any()           # open slots are part of the record
    rec = dict(nn_gene_index=g["index"], nn_gene_score=g["score"], nn_sample_index=s["index"], nn_sample_score=s["score"])
    flatio.write_records(str(tmp_path), fmt, rec)
    for name, v in rec.items():
        if fmt == "npy":
            back = np.load(tmp_path / (name + ".npy"))
            assert back.dtype == v.dtype
        else:
            back = flatio.read_raw(str(tmp_path / (name + ".f64")), v.shape)
            assert back.dtype == np.float64
        assert back.shape == v.shape and np.array_equal(back, v, equal_nan=True)
    idx = np.load(tmp_path / "nn_gene_index.npy") if fmt == "npy" else flatio.read_raw(str(tmp_path / "nn_gene_index.f64"), (9, 10))
    assert idx.min() == -1 and idx.max() == 8                                 # 0-based, -1 = open
