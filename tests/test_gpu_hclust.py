"""insider_hip_hclust on the device against the numpy yardstick posthoc.hclust_host(): identical merges, sizes, leaf order and
counters at the tile, wave and block edges of 16 and 64 and at every K-block form, heights within the per-merge bound derived
in tests/hclust_cases.py; then what the yardstick does not give (repeats, monotone heights, translation, exact ties, the slow
chain, dead columns), the refusals through the raw C entry and through api.hclust(), and the users' calls.

Equal topology is only meaningful where the yardstick's own choices are separated: every case asserts that the smallest gap
between a query's best and runner-up distance, over all queries of all rounds, exceeds four times the bound."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests import hclust_cases as hc
from tests.support import bits, lib, need_gpu, same_bits  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 257, 2000)      # the edges of 16 (tile), 64 (block of queries), 256 (list blocks)
DS = (1, 3, 4, 5, 16, 17, 30, 48, 63)                        # every KS = 1..4 and the K4 padding
RECORD = ("merge", "size", "order")
COUNTERS = ("alive", "rounds", "queries")
NAMES = RECORD + ("height",)


def follows(got, ref, metric, D, what="", exact=False):
    """got (the device) against ref (the yardstick): the separation of the inputs first, then the records.  exact: a case whose
    every distance is computed without rounding on both sides (no gap can be asked of it: the tie rule alone decides, and the
    heights must then agree to the bit)."""
    N = ref["order"].size
    if exact:
        assert np.array_equal(got["height"], ref["height"], equal_nan=True)
    elif N > 2 and np.isfinite(ref["min_gap"]):
        print(f"{what}: smallest gap / (4 bound) = {ref['min_gap'] / (4 * hc.gap_bound(D)):.3g}")
        assert ref["min_gap"] > 4 * hc.gap_bound(D)
    for k in COUNTERS:
        assert got[k] == ref[k], k
    for k in RECORD:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    R = max(ref["alive"] - 1, 0)
    assert np.all(np.isnan(got["height"][R:])) and got["height"].shape == (max(N - 1, 0),)
    if R:
        err = np.abs(hc.linkage_d(metric, got["height"][:R]) - ref["d"][:R])
        bound = hc.pair_bound(metric, D, ref["scale"][:R], ref["d"][:R])
        print(f"{what}: max height error / bound = {np.max(err / bound):.3g} over {R} merges, rounds {got['rounds']}, "
              f"queries / N = {got['queries'] / N:.2f}")
        assert np.all(err <= bound)


@pytest.fixture(scope="module")
def yardsticks():
    """hclust_host() of a planted case, computed once per (N, D, metric)."""
    cache = {}

    def get(N, D, metric):
        if (N, D, metric) not in cache:
            P = hc.planted(N, D, hc.seed_of(N, D))
            cache[N, D, metric] = P, posthoc.hclust_host(P, metric)
        return cache[N, D, metric]
    return get


# ---- 1. against the yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("N", NS)
def test_sizes_follow_the_yardstick(lib, yardsticks, N, metric):
    P, ref = yardsticks(N, 30, metric)
    follows(api.hclust(P, metric), ref, metric, 30, f"N={N} D=30 {metric}")


@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("D", DS)
def test_depths_follow_the_yardstick(lib, yardsticks, D, metric):
    """Under cosine with D = 1 every working point is +1 or -1, every mean +1 or -1 and every distance 0 or 2, all exact: no
    planted data can separate the choices there, and none is needed."""
    for N in (65, 257):
        P, ref = yardsticks(N, D, metric)
        follows(api.hclust(P, metric), ref, metric, D, f"N={N} D={D} {metric}", exact=metric == "cosine" and D == 1)


# ---- 2. what the yardstick does not give -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", hc.METRICS)
def test_repeats_heights_and_sizes(lib, metric):
    P = hc.planted(300, 30, 11)
    runs = [api.hclust(P, metric) for _ in range(3)]
    assert bits(runs[0], NAMES) == bits(runs[1], NAMES) == bits(runs[2], NAMES)
    assert all(runs[0][k] == r[k] for r in runs for k in COUNTERS)
    got = runs[0]
    assert np.all(np.diff(got["height"]) >= 0) and got["size"][-1] == got["alive"] == 300
    assert got["ms"] > 0.0 and lib.insider_hip_last_hclust_ms() == runs[2]["ms"]
    assert sorted(got["order"].tolist()) == list(range(300))
    assert np.all(got["merge"][:, 0] < got["merge"][:, 1]) and np.all(got["merge"] < 300 + np.arange(299)[:, None])


def test_ward_does_not_see_a_translation(lib):
    P = hc.planted(257, 30, 12)
    a, b = api.hclust(P, "euclidean"), api.hclust(P + 1e3, "euclidean")
    same_bits(a, b, RECORD)
    assert np.allclose(a["height"], b["height"], rtol=1e-9, atol=0)


def test_exact_ties_give_the_yardsticks_records(lib):
    P = hc.ties()
    got, ref = api.hclust(P, "euclidean"), posthoc.hclust_host(P, "euclidean")
    nz = len(hc.TIE_ZERO)
    assert [tuple(r) for r in got["merge"][:nz].tolist()] == hc.TIE_ZERO and np.array_equal(got["height"][:nz], np.zeros(nz))
    same_bits(got, ref, RECORD)
    assert all(got[k] == ref[k] for k in COUNTERS)
    assert np.all(np.abs(hc.linkage_d("euclidean", got["height"]) - ref["d"]) <= hc.pair_bound("euclidean", 2, ref["scale"], ref["d"]))


def test_the_chain_finishes_and_agrees(lib):
    P = hc.chain()
    ref = posthoc.hclust_host(P, "euclidean")
    got = api.hclust(P, "euclidean")
    assert got["rounds"] >= 10
    follows(got, ref, "euclidean", 2, "chain")


def test_dead_columns_under_cosine(lib):
    N, D = 300, 9
    P = hc.planted(N, D, 13)
    dead = np.random.default_rng(13).random(N) < 0.3
    P[:, dead] = 0.0
    ref = posthoc.hclust_host(P, "cosine")
    got = api.hclust(P, "cosine")
    follows(got, ref, "cosine", D, "30 % dead")
    na = int((~dead).sum())
    assert got["alive"] == na and got["order"][na:].tolist() == np.flatnonzero(dead).tolist()
    assert np.all(got["merge"][na - 1:] == -1) and np.all(got["size"][na - 1:] == -1) and got["size"][na - 2] == na
    assert not set(np.flatnonzero(dead).tolist()) & set(got["merge"][:na - 1].ravel().tolist())
    allzero = api.hclust(np.zeros((D, 20)), "cosine")
    assert (allzero["alive"], allzero["rounds"]) == (0, 0) and np.all(allzero["merge"] == -1)
    assert allzero["order"].tolist() == list(range(20))


# ---- 3. refusals and housekeeping --------------------------------------------------------------------------------------------
def raw(lib, P, metric=0, linkage=0, max_rounds=100, D=None, N=None, null=()):
    """The C entry with sentinel-filled outputs -> (status, outputs)."""
    P = np.asfortranarray(P, dtype=np.float64)
    D = P.shape[0] if D is None else D
    N = P.shape[1] if N is None else N
    n = P.shape[1]
    outs = [np.full((max(n - 1, 1), 2), -7, dtype=np.int32), np.full(max(n - 1, 1), -7.0), np.full(max(n - 1, 1), -7, dtype=np.int32),
            np.full(n, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int64),
            np.full(1, -7, dtype=np.int32)]
    types = [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    ptrs = [None if 1 + i in null else _lib.ptr(o, t) for i, (o, t) in enumerate(zip(outs, types))]
    status = lib.insider_hip_hclust(None if 0 in null else _lib.ptr(P), N, D, metric, linkage, max_rounds, 0, *ptrs)
    return status, outs


def test_bad_arguments_are_refused_and_write_nothing(lib):
    P = hc.planted(17, 5, 14)
    bad = _lib.ERR_ARG

    def refused(status_outs, expect=bad):
        status, outs = status_outs
        assert status == expect and all(np.all(o == -7) for o in outs)

    for pos in range(8):                                                         # P and every output
        refused(raw(lib, P, null=(pos,)))
    refused(raw(lib, np.ones((64, 17))))                                         # D = 64
    refused(raw(lib, P, D=0))
    refused(raw(lib, P, N=0))
    refused(raw(lib, P, N=-2))
    refused(raw(lib, P, N=2 ** 30 + 1))                                          # (refused before P is read)
    for metric, linkage in ((0, 1), (1, 0), (2, 0), (0, 2), (-1, 0), (1, -1)):   # the two unoffered pairs and unknown codes
        refused(raw(lib, P, metric=metric, linkage=linkage))
    refused(raw(lib, P, max_rounds=0))
    refused(raw(lib, P, max_rounds=-1))
    for val in (np.nan, np.inf, -np.inf):
        Pn = P.copy(order="F")
        Pn[4, 16] = val
        refused(raw(lib, Pn))
        refused(raw(lib, Pn, metric=1, linkage=1))
    assert b"finite" in lib.insider_hip_last_error()
    refused(raw(lib, P, max_rounds=1), expect=_lib.ERR_UNFINISHED)               # N = 17 needs more than one round
    refused(raw(lib, P, metric=1, linkage=1, max_rounds=1), expect=_lib.ERR_UNFINISHED)
    assert b"max_rounds" in lib.insider_hip_last_error() and lib.insider_hip_last_hclust_ms() > 0.0
    status, outs = raw(lib, P)                                                   # and the same call with room finishes
    assert status == _lib.OK and outs[2][15] == 17 and outs[6][0] == 17
    with pytest.raises(_lib.InsiderError) as e:
        api.hclust(P, "cosine", max_rounds=1)
    assert e.value.status == _lib.ERR_UNFINISHED
    for kw in (dict(metric="cosine", linkage="ward"), dict(metric="euclidean", linkage="average"), dict(max_rounds=0),
               dict(metric="dot")):
        with pytest.raises(_lib.InsiderError) as e:
            api.hclust(P, **kw)
        assert e.value.status == _lib.ERR_ARG
    with pytest.raises(_lib.InsiderError):
        api.hclust(np.ones((64, 4)))
    assert api.hclust(P, "cosine", max_rounds=2 * 17)["alive"] == 17             # the process goes on


def test_a_fit_keeps_its_bits_around_a_call(lib):
    w = workloads.small(n=90, p=140, K=6)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        def fit():
            return ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha, tuning=1,
                               max_iter=8, seed=3)
        before = fit()
        tree = api.hclust(before["column_factor"], "cosine")
        assert tree["alive"] >= 2 and tree["size"][tree["alive"] - 2] == tree["alive"]
        with pytest.raises(_lib.InsiderError):
            api.hclust(before["column_factor"], "euclidean", max_rounds=1)
        after = fit()
    finally:
        ds.close()
    same_bits(before, after, ("column_factor",))
    same_bits(before["row_matrices"], after["row_matrices"], tuple(before["row_matrices"]))
    assert np.array_equal(before["traj"], after["traj"], equal_nan=True)


# ---- 4. users' calls ---------------------------------------------------------------------------------------------------------
def test_gene_tree_recovers_planted_modules(lib):
    rng = np.random.default_rng(15)
    K, p, modules = 9, 300, 6
    centres = rng.standard_normal((K, modules))
    truth = np.concatenate([np.arange(modules), rng.integers(0, modules, p - modules)])
    Cm = np.asfortranarray(centres[:, truth] + 0.1 * rng.standard_normal((K, p)))
    for metric in hc.METRICS:
        rec = posthoc.gene_tree(Cm, metric=metric)
        ref = posthoc.hclust_host(Cm, metric)
        follows(rec, ref, metric, K, f"gene_tree {metric}")
        lab = posthoc.cut_tree(rec, k=modules)
        pairs = {(int(a), int(b)) for a, b in zip(lab, truth)}
        assert len(pairs) == modules                                             # the planted partition, up to the labels' names
        assert rec["height"][p - modules] > 2 * rec["height"][p - modules - 1]   # and the tree says "six" by itself
    assert min(np.bincount(truth)) >= 30
    sets = (np.array([0, 30, 60]), np.concatenate([np.flatnonzero(truth == 0)[:30], np.flatnonzero(truth == 1)[:30]]))
    ora = posthoc.tree_overrepresentation(rec, modules, sets)
    assert ora["overlap"].shape == (modules, 2) and ora["overlap"].max(axis=0).tolist() == [30, 30]


def test_sample_and_level_trees(lib):
    rng = np.random.default_rng(16)
    K, n, counts = 5, 80, (7, 3)
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    A = [rng.standard_normal((L, K)) for L in counts]
    rec = posthoc.sample_tree(A, lev)
    combos = len({tuple(r) for r in lev.tolist()})
    assert rec["alive"] == n and np.count_nonzero(rec["height"] < 1e-12) == n - combos   # equal samples merge first, at 0
    lab = posthoc.cut_tree(rec, k=combos)
    assert len({(int(a), tuple(r)) for a, r in zip(lab, lev.tolist())}) == combos
    rec = posthoc.level_tree(A[0], metric="euclidean")
    ref = posthoc.hclust_host(A[0].T, "euclidean")
    assert rec["order"].size == 7 and np.array_equal(rec["merge"], ref["merge"])


def test_cli_writes_the_tree_records(tmp_path):
    from insider_amd import fit as fit_cli
    rng = np.random.default_rng(17)
    n, p, K = 60, 45, 4
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    np.save(tmp_path / "X.npy", rng.standard_normal((n, p)))
    np.save(tmp_path / "L.npy", conf)
    (tmp_path / "sets.gmt").write_text("".join(f"set{s}\tna\t" + "\t".join(str(g) for g in range(5 * s, 5 * s + 10)) + "\n"
                                               for s in range(6)))
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--rank", str(K), "--lambda", "1",
                         "--alpha", "0.2", "--max-iter", "3", "--gene-tree", "--sample-tree", "--tree-cut", "3", "--gene-sets",
                         str(tmp_path / "sets.gmt"), "--enrich-min-size", "5", "--enrich-perms", "10", "--out", str(out)]) == 0
    for who, count in (("gene", p), ("sample", n)):
        rec = {name: np.load(out / f"hc_{who}_{name}.npy") for name in ("merge", "height", "size", "order", "label")}
        assert rec["merge"].shape == (count - 1, 2) and rec["height"].shape == rec["size"].shape == (count - 1,)
        assert rec["merge"].dtype == rec["size"].dtype == rec["order"].dtype == rec["label"].dtype == np.int32
        assert sorted(rec["order"].tolist()) == list(range(count)) and rec["label"].shape == (count,)
        assert set(rec["label"].tolist()) - {-1} == {0, 1, 2}
    tree = posthoc.hclust_host(np.load(out / "C.npy"), "cosine")
    assert np.array_equal(np.load(out / "hc_gene_merge.npy"), tree["merge"])
    assert np.load(out / "hc_gene_overlap.npy").shape == np.load(out / "hc_gene_hyper_p.npy").shape == (3, 6)
