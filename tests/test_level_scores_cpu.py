"""CPU-side checks of the level scores: the numpy yardstick posthoc.level_scores_host() agrees with a naive triple loop;
posthoc.ls_derived() handles ties, samples without entries, foreign candidates and the confusion table; the command line
knows the new flags."""
import numpy as np
import pytest

from insider_amd import fit as fit_cli, posthoc


def _naive(X, lev, Z, mask, A, Cm, cov, cand):
    n, p = X.shape
    K = Cm.shape[0]
    E = A[cov] if cand is None else cand
    sse = np.zeros((n, E.shape[0]))
    cnt = np.zeros(n)
    for i in range(n):
        for j in range(p):
            if mask is not None and not mask[i, j]:
                continue
            cnt[i] += 1
            d = X[i, j]
            for b in range(lev.shape[1]):
                if b != cov:
                    d -= sum(A[b][lev[i, b] - 1, k] * Cm[k, j] for k in range(K))
            if Z is not None:
                for q in range(Z.shape[1]):
                    d -= Z[i, q] * sum(A[lev.shape[1]][q, k] * Cm[k, j] for k in range(K))
            for l in range(E.shape[0]):
                r = d - sum(E[l, k] * Cm[k, j] for k in range(K))
                sse[i, l] += r * r
    return sse, cnt


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("foreign", [False, True])
def test_host_yardstick_against_a_triple_loop(m, foreign):
    rng = np.random.default_rng(3 + m)
    n, p, K, counts = 7, 5, 3, (3, 2)
    X = rng.standard_normal((n, p))
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    Z = rng.standard_normal((n, m)) if m else None
    A = [rng.standard_normal((L, K)) for L in counts] + ([rng.standard_normal((m, K))] if m else [])
    Cm = rng.standard_normal((K, p))
    mask = rng.random((n, p)) < 0.7
    mask[2] = False
    cand = rng.standard_normal((4, K)) if foreign else None
    for cov in (0, 1):
        for w in (None, mask):
            got = posthoc.level_scores_host(X, lev, Z, w, A, Cm, cov, candidates=cand)
            sse, cnt = _naive(X, lev, Z, w, A, Cm, cov, cand)
            assert got["sse"].shape == (n, 4 if foreign else counts[cov])
            np.testing.assert_allclose(got["sse"], sse, rtol=1e-12, atol=1e-13)
            assert np.array_equal(got["n"], cnt)
            if w is not None:
                assert got["n"][2] == 0 and np.all(got["sse"][2] == 0)
    with pytest.raises(ValueError):
        posthoc.level_scores_host(X, lev, Z, None, A, Cm, 2)


def test_ls_derived():
    sse = np.array([[4.0, 1.0, 2.0],      # assigned 1, best 2, second 3
                    [3.0, 3.0, 5.0],      # a tie: the lowest id is best, the other one second
                    [0.0, 0.0, 0.0],      # no entries
                    [2.0, 8.0, 1.0],      # assigned 3 = best
                    [0.0, 1.0, 1.0]])     # assigned 1 = best with sse 0: margin 0, not 0 / 0
    cnt = np.array([2.0, 4.0, 0.0, 1.0, 5.0])
    d = posthoc.ls_derived(dict(sse=sse, n=cnt), np.array([1, 2, 3, 3, 1]))
    assert d["best"].tolist() == [2, 1, 0, 3, 1]
    assert d["second"].tolist() == [3, 2, 0, 1, 2]
    np.testing.assert_array_equal(d["mse"][0], [2.0, 0.5, 1.0])
    assert np.all(np.isnan(d["mse"][2]))
    np.testing.assert_array_equal(d["margin"][[0, 1, 3, 4]], [0.75, 0.0, 0.0, 0.0])
    assert np.isnan(d["margin"][2])
    assert d["flagged"].tolist() == [True, True, False, False, False]
    want = np.zeros((3, 3), dtype=np.int64)
    want[0, 1] = want[1, 0] = want[2, 2] = want[0, 0] = 1
    assert np.array_equal(d["confusion"], want) and d["confusion"].sum() == 4
    # the assigned level ties with a lower id at sse 0: flagged, margin 0 (not 0 / 0)
    z = posthoc.ls_derived(dict(sse=np.array([[0.0, 0.0, 1.0]]), n=np.array([3.0])), np.array([2]))
    assert z["best"].tolist() == [1] and z["flagged"].tolist() == [True] and z["margin"].tolist() == [0.0]
    # foreign candidates: no assigned level
    f = posthoc.ls_derived(dict(sse=sse, n=cnt), None)
    assert f["best"].tolist() == [2, 1, 0, 3, 1] and f["confusion"] is None
    assert np.all(np.isnan(f["margin"])) and not f["flagged"].any()
    # one candidate: no second
    one = posthoc.ls_derived(dict(sse=sse[:, :1], n=cnt), None)
    assert one["best"].tolist() == [1, 1, 0, 1, 1] and one["second"].tolist() == [0] * 5
    with pytest.raises(ValueError):
        posthoc.ls_derived(dict(sse=sse, n=cnt), np.array([1, 2, 4, 3, 1]))
    with pytest.raises(ValueError):
        posthoc.ls_derived(dict(sse=sse, n=cnt), np.array([1, 2, 3]))


def test_command_line_flags(tmp_path):
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "2", "--lambda", "1", "--alpha", "0.1"]
    a = fit_cli.parse(base + ["--level-scores", "2", "--level-score-entries", "test"])
    assert a.level_scores == 2 and a.level_score_entries == "test"
    a = fit_cli.parse(base + ["--level-scores", "1"])
    assert a.level_scores == 1 and a.level_score_entries == "train"
    assert fit_cli.parse(base).level_scores is None
    for bad in (["--level-scores", "1", "--tune"], ["--level-scores", "0"], ["--level-scores", "-1"], ["--level-scores", "1", "--level-score-entries", "held"]):
        with pytest.raises(SystemExit):
            fit_cli.parse(base + bad)
    # COV beyond the covariate columns of the input is refused when the inputs are read, before any device work
    rng = np.random.default_rng(0)
    np.save(tmp_path / "X.npy", rng.standard_normal((6, 4)))
    np.save(tmp_path / "L.npy", np.column_stack([rng.integers(1, 3, 6), rng.integers(1, 3, 6)]).astype(np.int32))
    with pytest.raises(SystemExit) as e:
        fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--rank", "2", "--lambda", "1",
                      "--alpha", "0.1", "--level-scores", "3", "--out", str(tmp_path / "out")])
    assert "--level-scores" in str(e.value)
