"""Host-side checks of the k-means call (insider_hip_kmeans): the numpy yardstick posthoc.kmeans_host() agrees with a brute
force built from Python loops and ``sorted`` with the key (-score, index), the Forgy start is the draw
insider_hip_enrichment_sample names, api.kmeans() refuses every bad argument before it reaches the library,
module_overrepresentation() counts what a hand count gives, and the driver's flags parse and its records round-trip through
flatio."""
import ctypes as C
import math

import numpy as np
import pytest

from insider_amd import _lib, api, fit, flatio, posthoc
from tests.support import lib  # noqa: F401  (fixture)


# ---- the yardstick against a brute force -------------------------------------------------------------------------------------
def brute(P, k, metric, init, max_iter):
    """Lloyd's loop of include/insider_hip.h in Python floats: loops, and ``sorted`` with the key (-score, index)."""
    cos = metric == "cosine"
    ss = lambda v: sum((a * a for a in v), 0.0)
    unit = lambda v: [a / math.sqrt(ss(v)) for a in v]
    pts = [[float(a) for a in P[:, i]] for i in range(P.shape[1])]
    alive = [ss(p) > 0 or not cos for p in pts]
    X = [unit(p) if cos and ok else p for p, ok in zip(pts, alive)]
    Cm = [unit(c) if cos else c for c in ([float(a) for a in init[:, j]] for j in range(k))]
    dist = lambda x, s: 1.0 - s if cos else max(0.0, ss(x) - 2.0 * s)

    def assign():
        rows = []
        for x, ok in zip(X, alive):
            order = sorted((-(sum((a * b for a, b in zip(x, c)), 0.0) - (0.0 if cos else 0.5 * ss(c))), j) for j, c in enumerate(Cm))
            one = (order[0][1], dist(x, -order[0][0]))
            two = (order[1][1], dist(x, -order[1][0])) if k > 1 else (-1, math.nan)
            rows.append((one, two) if ok else ((-1, math.nan), (-1, math.nan)))
        return rows

    rows = assign()
    traj, t, conv = [sum(r[0][1] for r, ok in zip(rows, alive) if ok)], 0, 0
    while t < max_iter:
        for j in range(k):
            mem = [x for x, r, ok in zip(X, rows, alive) if ok and r[0][0] == j]
            tot = [sum(col, 0.0) for col in zip(*mem)]
            den = (math.sqrt(ss(tot)) if cos else float(len(mem))) if mem else 0.0
            if den > 0.0:
                Cm[j] = [a / den for a in tot]
        new = assign()
        t += 1
        traj.append(sum(r[0][1] for r, ok in zip(new, alive) if ok))
        same = [r[0][0] for r in new] == [r[0][0] for r in rows]
        rows = new
        if same:
            conv = 1
            break
    return dict(centers=np.array(Cm).T, label=np.array([r[0][0] for r in rows]), dist=np.array([r[0][1] for r in rows]),
                second=np.array([r[1][0] for r in rows]), dist2=np.array([r[1][1] for r in rows]),
                sizes=np.array([sum(1 for r in rows if r[0][0] == j) for j in range(k)]), traj=np.array(traj), iters=t,
                converged=conv)


def same(got, ref, max_iter):
    assert got["label"].dtype == got["second"].dtype == got["sizes"].dtype == np.int32
    for name in ("label", "second", "sizes"):
        assert np.array_equal(got[name], ref[name]), name
    assert got["iters"][0] == ref["iters"] and got["converged"][0] == ref["converged"] and got["best"] == 0
    for name in ("dist", "dist2", "centers"):
        assert np.allclose(got[name], ref[name], rtol=0, atol=1e-14, equal_nan=True), name
    assert got["traj"].shape == (max_iter + 1,)
    assert np.allclose(got["traj"][:ref["iters"] + 1], ref["traj"], rtol=1e-13, atol=0)
    assert np.all(np.isnan(got["traj"][ref["iters"] + 1:])) and got["final_inertia"][0] == got["traj"][ref["iters"]]


def tiny(seed, D=3, n=14):
    rng = np.random.default_rng(seed)
    P = rng.integers(-2, 3, (D, n)).astype(np.float64)
    P[:, 1] = [1, -2, 2][:D]
    P[:, 4] = P[:, 1]          # duplicate columns
    P[:, 9] = P[:, 1]
    P[:, 2] = 0.0              # zero columns: dead under cosine
    P[:, 6] = 0.0
    P[:, n - 1] = 0.0
    return P


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("max_iter", [0, 1, 20])
def test_host_yardstick_matches_brute_force(metric, k, max_iter):
    for seed in (1, 2, 3):
        P = tiny(seed)
        init = P[:, [0, 1, 3, 5, 7][:k]] + np.array([[0.0], [0.0], [1.0]])        # (never a zero column)
        got = posthoc.kmeans_host(P, k, metric=metric, init=init, restarts=1, max_iter=max_iter)
        same(got, brute(P, k, metric, init, max_iter), max_iter)
        again = posthoc.kmeans_host(P, k, metric=metric, init=init, restarts=1, max_iter=max_iter, chunk=5)
        for name in ("label", "second", "dist", "dist2", "centers", "traj"):
            assert np.array_equal(got[name], again[name], equal_nan=True)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_empty_cluster_and_dead_point_rules(metric):
    P = tiny(4)
    init = np.array([[1.0, 1.0, -1.0, 1.0], [-2.0, -2.0, 0.0, -2.0], [2.0, 2.0, 1.0, 2.0]])   # centres 0, 1 and 3 are one point
    for max_iter in (0, 1, 20):
        got = posthoc.kmeans_host(P, 4, metric=metric, init=init, restarts=1, max_iter=max_iter)
        same(got, brute(P, 4, metric, init, max_iter), max_iter)
        if max_iter == 0:   # the tie rule leaves the higher-indexed duplicates empty
            assert got["sizes"][1] == 0 and got["sizes"][3] == 0 and not np.isin(got["label"], (1, 3)).any()
            assert np.all(got["label"][[1, 4, 9]] == 0) and np.all(got["second"][[1, 4, 9]] == 1)
        if max_iter <= 1:   # and a cluster that was empty keeps its centre through the update
            want = init[:, 1] / (3.0 if metric == "cosine" else 1.0)
            assert np.allclose(got["centers"][:, 1], want, rtol=0, atol=1e-15)
            assert np.array_equal(got["centers"][:, 1], got["centers"][:, 3])
        dead = [2, 6, 13]
        if metric == "cosine":
            assert np.all(got["label"][dead] == -1) and np.all(got["second"][dead] == -1)
            assert np.all(np.isnan(got["dist"][dead])) and np.all(np.isnan(got["dist2"][dead]))
            assert got["sizes"].sum() == P.shape[1] - 3
            assert got["final_inertia"][0] == got["dist"][got["label"] >= 0].sum()
        else:
            assert np.all(got["label"][dead] >= 0) and got["sizes"].sum() == P.shape[1]
    # -0.0 and 0.0 are one number: equal scores go to the lowest centre whichever sign a zero carries
    got = posthoc.kmeans_host(np.array([[1.0, 2.0, 3.0]]), 3, metric="euclidean", init=np.array([[-0.0, 0.0, -0.0]]), restarts=1,
                              max_iter=0)
    assert list(got["label"]) == [0, 0, 0] and list(got["second"]) == [1, 1, 1]


def test_forgy_start_is_the_named_draw(lib):
    P = tiny(5, n=40)
    rng = np.random.default_rng(5)
    P[:, 10:] = rng.integers(-2, 3, (3, 30))
    P[:, [11, 20, 39]] = 0.0
    seed, k = 0xABCDEF0123, 6
    for metric in ("cosine", "euclidean"):
        alive = np.flatnonzero((P * P).sum(axis=0) > 0) if metric == "cosine" else np.arange(P.shape[1])
        for r in range(3):
            out = np.full(k, -1, dtype=np.int32)
            assert lib.insider_hip_enrichment_sample(seed, r, k, alive.size, _lib.ptr(out, C.c_int32)) == _lib.OK
            assert np.array_equal(out, posthoc.gs_sample_host(seed, r, k, alive.size))
        got = posthoc.kmeans_host(P, k, metric=metric, restarts=1, max_iter=0, seed=seed)
        out = posthoc.gs_sample_host(seed, 0, k, alive.size)
        X = P[:, alive[out]] / (np.sqrt((P[:, alive[out]] ** 2).sum(axis=0)) if metric == "cosine" else 1.0)
        assert np.allclose(got["centers"], X, rtol=0, atol=1e-15) and len(set(out.tolist())) == k
        assert not np.isin(alive[out], (2, 6, 11, 20, 39)).any() or metric == "euclidean"


# ---- the wrapper's refusals --------------------------------------------------------------------------------------------------
def test_wrapper_refuses_bad_arguments_before_the_library(monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", never)
    P = tiny(6)
    init = P[:, [0, 1]] + 1.0
    inf, nan = P.copy(), init.copy()
    inf[1, 3], nan[0, 1] = np.inf, np.nan
    zero_init = init.copy()
    zero_init[:, 1] = 0.0
    one_alive = np.zeros((3, 5))
    one_alive[:, 2] = 1.0
    bad = [
        dict(points=P[0], k=2),                                   # not D x N
        dict(points=np.zeros((64, 5)) + 1.0, k=2),                # D > 63
        dict(points=np.zeros((0, 5)), k=1),                       # D < 1
        dict(points=np.zeros((3, 0)), k=1),                       # N < 1
        dict(points=P, k=0), dict(points=P, k=4097), dict(points=P, k=2.0), dict(points=P, k=True),
        dict(points=P, k=2, metric="dot"),
        dict(points=P, k=2, restarts=0), dict(points=P, k=2, restarts=257),
        dict(points=P, k=2, init=init, restarts=2),               # restarts != 1 with init
        dict(points=P, k=2, max_iter=-1), dict(points=P, k=2, max_iter=10001), dict(points=P, k=2, max_iter=1.5),
        dict(points=P, k=2, seed=-1), dict(points=P, k=2, seed=2 ** 64),
        dict(points=inf, k=2), dict(points=P, k=2, init=nan, restarts=1),
        dict(points=P, k=2, init=init[:, :1], restarts=1),        # init is not D x k
        dict(points=P, k=2, init=init[:2], restarts=1),
        dict(points=P, k=2, init=zero_init, restarts=1, metric="cosine"),
        dict(points=P, k=12, metric="cosine"),                    # k > Na = 11
        dict(points=P, k=15, metric="euclidean"),                 # k > N
        dict(points=one_alive, k=1, metric="cosine"),             # a drawn start with Na < 2
        dict(points=np.ones((3, 1)), k=1, metric="euclidean"),
    ]
    for kw in bad:
        for fn in (api.kmeans, posthoc.kmeans_host):
            with pytest.raises(_lib.InsiderError) as e:
                fn(**kw)
            assert e.value.status == _lib.ERR_ARG, kw
    # what is allowed (the yardstick needs no library): k = Na, one point with init, a zero init column under Euclidean
    assert posthoc.kmeans_host(P, 11, metric="cosine", restarts=2, max_iter=3)["sizes"].sum() == 11
    assert posthoc.kmeans_host(np.ones((3, 1)), 1, metric="cosine", init=np.ones((3, 1)), restarts=1)["label"][0] == 0
    assert posthoc.kmeans_host(P, 2, metric="euclidean", init=zero_init, restarts=1, max_iter=0)["sizes"].sum() == 14


# ---- host-only follow-ups ----------------------------------------------------------------------------------------------------
def test_module_overrepresentation_on_a_hand_countable_case():
    # 10 genes: modules {0, 1, 2, 3}, {4, 5, 6}, gene 7 and 8 in module 2, gene 9 dead
    label = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, -1], dtype=np.int32)
    names = ["a", "b"]
    ptr, genes = np.array([0, 4, 7], dtype=np.int64), np.array([0, 1, 2, 9, 3, 4, 5], dtype=np.int32)
    rec = posthoc.module_overrepresentation(label, (names, ptr, genes))
    assert rec["names"] == names and list(rec["module_size"]) == [4, 3, 2] and list(rec["size"]) == [3, 3]   # gene 9 is not counted
    assert rec["overlap"].tolist() == [[3, 1], [0, 2], [0, 0]] and rec["overlap"].dtype == np.int32
    c = math.comb
    # P(X >= 3): all 3 marked genes among the module's 4 of 9; P(X >= 1) = 1 - P(0); P(X >= 2) among 3 of 9
    want = np.array([[c(6, 1) / c(9, 4), 1 - c(6, 4) / c(9, 4)],
                     [1.0, (c(3, 2) * c(6, 1) + c(3, 3)) / c(9, 3)],
                     [1.0, 1.0]])
    assert np.allclose(rec["hyper_p"], want, rtol=1e-12, atol=0)
    p0 = want[0]
    assert np.allclose(rec["hyper_fdr"][0], [min(p0[0] * 2, p0[1]), p0[1]], rtol=1e-12)       # Benjamini-Hochberg, S = 2
    assert np.allclose(rec["hyper_fdr"][2], [1.0, 1.0])
    rec = posthoc.module_overrepresentation(label, (ptr, genes), k=4)                         # an empty fourth module
    assert rec["overlap"].shape == (4, 2) and rec["module_size"][3] == 0 and np.all(rec["hyper_p"][3] == 1.0)
    assert "names" not in rec


def test_module_summary():
    Cm = np.array([[1.0, -3.0, 0.0, 2.0], [0.0, 1.0, 0.0, -4.0]])
    rec = dict(label=np.array([0, 1, -1, 1]), sizes=np.array([1, 2, 0]), dist=np.array([0.5, 0.25, np.nan, 0.125]))
    out = posthoc.module_summary(rec, Cm)
    assert np.array_equal(out["mean_abs_loading"][:2], [[1.0, 0.0], [2.5, 2.5]]) and np.all(np.isnan(out["mean_abs_loading"][2]))
    assert [m.tolist() for m in out["members"]] == [[0], [3, 1], []]


def test_gmt_sets_feed_the_overrepresentation(tmp_path):
    path = tmp_path / "sets.gmt"
    path.write_text("s1\tna\t0\t1\t2\ns2\tna\t3\t4\n")
    sets = flatio.read_gmt(str(path), min_size=1, max_size=10)
    rec = posthoc.module_overrepresentation(np.array([0, 0, 1, 1, 1]), sets)
    assert rec["names"] == ["s1", "s2"] and rec["overlap"].tolist() == [[2, 0], [1, 2]]


# ---- the driver --------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_cluster_options():
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    a = fit.parse(base + ["--gene-modules", "20", "--sample-clusters", "6", "--cluster-metric", "euclidean", "--cluster-restarts",
                          "3", "--cluster-iters", "50", "--cluster-seed", "11"])
    assert (a.gene_modules, a.sample_clusters, a.cluster_metric, a.cluster_restarts, a.cluster_iters, a.cluster_seed) == \
        (20, 6, "euclidean", 3, 50, 11)
    a = fit.parse(base)
    assert a.gene_modules is None and a.sample_clusters is None and a.cluster_metric == "cosine"
    assert (a.cluster_restarts, a.cluster_iters, a.cluster_seed) == (8, 100, 0x1D5EED)
    for extra in (["--cluster-metric", "dot"], ["--gene-modules", "0"], ["--sample-clusters", "4097"], ["--cluster-restarts", "0"],
                  ["--cluster-restarts", "257"], ["--cluster-iters", "-1"], ["--cluster-iters", "10001"], ["--cluster-seed", "-1"]):
        with pytest.raises(SystemExit):
            fit.parse(base + extra)
    with pytest.raises(SystemExit):
        fit.parse(["--x", "X.npy", "--levels", "L.npy", "--tune", "--gene-modules", "3"])


@pytest.mark.parametrize("fmt", ["flat", "npy"])
def test_records_round_trip_through_flatio(tmp_path, fmt):
    P = tiny(7)
    km = posthoc.kmeans_host(P, 3, metric="cosine", restarts=2, max_iter=5, seed=3)
    assert (km["label"] == -1).any() and np.isnan(km["dist"]).any()            # dead points are part of the record
    rec = dict(fit.km_records("km_gene", km), **fit.km_records("km_sample", posthoc.kmeans_host(P[:, :5] + 0.25, 2, restarts=1)))
    assert sorted(rec) == sorted(f"km_{w}_{n}" for w in ("gene", "sample")
                                 for n in ("label", "dist", "second", "dist2", "center", "size", "traj"))
    ora = posthoc.module_overrepresentation(km["label"], (np.array([0, 3, 7]), np.array([0, 1, 2, 3, 4, 5, 6])), k=3)
    rec.update(km_gene_overlap=ora["overlap"], km_gene_hyper_p=ora["hyper_p"], km_gene_hyper_fdr=ora["hyper_fdr"])
    flatio.write_records(str(tmp_path), fmt, rec)
    for name, v in rec.items():
        v = np.asarray(v)
        if fmt == "npy":
            back = np.load(tmp_path / (name + ".npy"))
            assert back.dtype == v.dtype
        else:
            back = flatio.read_raw(str(tmp_path / (name + ".f64")), v.shape)
            assert back.dtype == np.float64
        assert back.shape == v.shape and np.array_equal(back, v, equal_nan=True), name
    lab = np.load(tmp_path / "km_gene_label.npy") if fmt == "npy" else flatio.read_raw(str(tmp_path / "km_gene_label.f64"), (14,))
    assert lab.min() == -1 and lab.max() <= 2                                 # 0-based, -1 = dead
