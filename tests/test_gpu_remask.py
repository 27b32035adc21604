"""Re-masked data sets (insider_hip_remask, insider_hip_set_folds, insider_hip_remask_fold) and tune(folds=True) on the GPU.

A re-masked handle shares the resident X with its source and builds everything that depends on the masks with the stages
insider_hip_create_ex runs, so whatever it computes must equal, BIT FOR BIT, what a data set created from the same X and
the same masks computes.  Against the CPU oracle the tolerances are those of tests/test_gpu_parity.py
(test_optimize_one_iteration: rel 1e-9 on factors and trajectory; test_optimize_31_iterations: rel 1e-6 on the factors,
1e-9 on the trajectory and the loss)."""
import ctypes
import threading

import numpy as np
import pytest

from insider_amd import _lib, api, workloads
from insider_amd._lib import InsiderError
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

CHUNK = 128          # line pitch of the resident matrix: ldn = n rounded up to it (insider_kernels.hpp)


# the data sets of check 1: two covariates; NA entries; continuous covariates (m = 1, m = 2); one many-level covariate
# (>= 49 levels: the level Gram sums run as one GEMM over genes, k_wgemm)
DATA = {
    "two_cov": (dict(n=70, p=90, level_counts=(5, 4)), 0),
    "na": (dict(n=70, p=90, level_counts=(5, 4), with_na=True), 0),
    "cont1": (dict(n=70, p=90, level_counts=(5, 4)), 1),
    "cont2": (dict(n=64, p=75, level_counts=(6, 3), with_na=True), 2),
    "many_level": (dict(n=170, p=110, level_counts=(56, 3)), 0),
}


def _workload(case, K):
    kw, m = DATA[case]
    w = workloads.small(K=K, **kw)
    na = (w.M_train == 0) & (w.M_test == 0)
    Z = np.asfortranarray(np.random.default_rng(8).standard_normal((w.n, m))) if m else None
    # the second pair of masks: another draw, another held-out share; the NA set belongs to X and stays
    tr2, te2 = workloads.holdout_masks(w.n, w.p, 0.22, seed=977)
    tr2, te2 = np.asfortranarray(tr2 * ~na, dtype=np.uint8), np.asfortranarray(te2 * ~na, dtype=np.uint8)
    return w, Z, m, tr2, te2


def _inits(w, m, K, seed=3, scale=1e-3):
    rng = np.random.default_rng(seed)
    A = [np.asfortranarray(rng.standard_normal((int(L), K)) * scale) for L in w.n_levels]
    if m:
        A.append(np.asfortranarray(rng.standard_normal((m, K)) * scale))
    return A, np.asfortranarray(rng.standard_normal((K, w.p)) * scale)


def _fit(hd, w, m, K, tuning=1, max_iter=12, lam=2.0, seed=3):
    A, C = _inits(w, m, K, seed)
    return hd.optimize(A, C, K, lam, lam, 0.4, tuning=tuning, max_iter=max_iter, seed=3, inc_continuous=1 if m else 0)


def _assert_same_fit(got, ref):
    assert got["iters"] == ref["iters"]
    assert np.array_equal(got["column_factor"], ref["column_factor"])
    assert set(got["row_matrices"]) == set(ref["row_matrices"])
    for k in ref["row_matrices"]:
        assert np.array_equal(got["row_matrices"][k], ref["row_matrices"][k]), k
    assert np.array_equal(got["traj"], ref["traj"], equal_nan=True)
    assert got["loss"] == ref["loss"] and got["train_rmse"] == ref["train_rmse"]
    assert got["test_rmse"] == ref["test_rmse"] or (np.isnan(got["test_rmse"]) and np.isnan(ref["test_rmse"]))


def _assert_same_handle(b, ref, w, m, K, options=()):
    """Everything the issue lists: optimize() with tuning 1 and 0, col_stats, variance decomposition, interaction GLM and
    the facts that describe the lists and the statistics kernel — bit for bit."""
    for hd in (b, ref):
        for name, v in options:
            hd.set_option(name, v)
    inc = 1 if m else 0
    for tuning in (1, 0):
        got, want = _fit(b, w, m, K, tuning), _fit(ref, w, m, K, tuning)
        _assert_same_fit(got, want)
    for key in ("col_stats_kernel", "col_stats_path", "col_entries", "row_entries"):
        assert b.info(key) == ref.info(key), key
    A, C = _inits(w, m, K, seed=9, scale=0.3)
    for x, y in zip(b.col_stats(A, inc_continuous=inc), ref.col_stats(A, inc_continuous=inc)):
        assert np.array_equal(x, y)
    assert b.info("col_stats_kernel") == ref.info("col_stats_kernel")
    for entries in ("train", "test", "all"):
        vb = b.variance_decomposition(A, C, entries=entries, inc_continuous=inc)
        vr = ref.variance_decomposition(A, C, entries=entries, inc_continuous=inc)
        for k in vr:
            assert np.array_equal(vb[k], vr[k], equal_nan=True), (entries, k)
    sub = [i != 1 for i in range(len(A))]
    for x, y in zip(b.interaction_glm(A, C, w.levels[:, 1], subtract=sub, inc_continuous=inc),
                    ref.interaction_glm(A, C, w.levels[:, 1], subtract=sub, inc_continuous=inc)):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("K", [7, 20, 30, 33, 48])
@pytest.mark.parametrize("case", list(DATA))
def test_remask_equals_create_by_bits(case, K):
    w, Z, m, tr2, te2 = _workload(case, K)
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, ctns_confounder=Z)
    b = a.remask(tr2, te2)
    ref = api.InsiderData(w.X, w.levels, tr2, te2, ctns_confounder=Z)
    try:
        assert a.info("data_bytes_shared") == 0 and b.info("data_bytes_shared") > 0
        assert b.info("data_bytes_shared") + b.info("data_bytes_own") == ref.info("data_bytes_own")
        _assert_same_handle(b, ref, w, m, K)
    finally:
        for hd in (a, b, ref):
            hd.close()


@pytest.mark.parametrize("col_factored", [0, 2, 3])
@pytest.mark.parametrize("case", ["two_cov", "na", "cont1", "many_level"])
def test_remask_equals_create_with_the_statistics_form_forced(case, col_factored):
    K = 20
    w, Z, m, tr2, te2 = _workload(case, K)
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, ctns_confounder=Z)
    b = a.remask(tr2, te2)
    ref = api.InsiderData(w.X, w.levels, tr2, te2, ctns_confounder=Z)
    try:
        _assert_same_handle(b, ref, w, m, K, options=(("col_factored", col_factored),))
    finally:
        for hd in (a, b, ref):
            hd.close()


def _fold_ids(w, F, seed=41):
    """Fold ids of a workload: its NA entries (neither train nor test) get id 0."""
    na = (w.M_train == 0) & (w.M_test == 0)
    return api.fold_splitter(np.where(na, np.nan, w.X), folds=F, rm_na_col=False, seed=seed)["fold_id"]


def _fold_masks(ids, f):
    return (np.asfortranarray((ids != f) & (ids != 0), dtype=np.uint8), np.asfortranarray(ids == f, dtype=np.uint8))


FOLD_DATA = [(dict(n=70, p=90, level_counts=(5, 4)), 0),
             (dict(n=131, p=77, level_counts=(6, 3), with_na=True), 0),     # n not a multiple of CHUNK, NA
             (dict(n=128, p=50, level_counts=(4, 4)), 1),                   # n a multiple: no pad elements
             (dict(n=300, p=40, level_counts=(5, 2), with_na=True), 0)]     # more than one 16-byte step per lane
P_PAST_GRID = 32805    # k_fold_codes runs min(ceil(p / 4), 8 n_simd) blocks of four genes: past 32 n_simd genes the blocks stride
                       # (32 * 1024 + 37 on 256 compute units)
FOLD_CASES = [pytest.param(kw, m, F, id=f"kw{i}-{m}-{F}") for F in (3, 5) for i, (kw, m) in enumerate(FOLD_DATA)] + \
             [pytest.param(dict(n=21, p=P_PAST_GRID, level_counts=(4, 3)), 0, 3, id="kw4-0-3")]


@pytest.mark.parametrize("kw,m,F", FOLD_CASES)
def test_fold_equals_create_by_bits(kw, m, F):
    K = 9
    w = workloads.small(K=K, **kw)
    Z = np.asfortranarray(np.random.default_rng(8).standard_normal((w.n, m))) if m else None
    ids = _fold_ids(w, F)
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, ctns_confounder=Z)
    if w.p == P_PAST_GRID:
        assert 4 * 8 * a.info("n_simd") < w.p
    a.set_folds(ids, F)
    try:
        for f in range(1, F + 1):
            tr, te = _fold_masks(ids, f)
            b = a.fold(f)
            ref = api.InsiderData(w.X, w.levels, tr, te, ctns_confounder=Z)
            try:
                assert b.info("col_entries") == ref.info("col_entries") and b.info("row_entries") == ref.info("row_entries")
                _assert_same_fit(_fit(b, w, m, K), _fit(ref, w, m, K))
                A, C = _inits(w, m, K, seed=9, scale=0.3)
                for x, y in zip(b.col_stats(A, inc_continuous=1 if m else 0), ref.col_stats(A, inc_continuous=1 if m else 0)):
                    assert np.array_equal(x, y)
                for ent in ("train", "test"):      # the codes themselves: entry counts per gene over each bit
                    vb = b.variance_decomposition(A, C, entries=ent, inc_continuous=1 if m else 0)
                    vr = ref.variance_decomposition(A, C, entries=ent, inc_continuous=1 if m else 0)
                    assert np.array_equal(vb["n"], vr["n"]) and np.array_equal(vb["rss"], vr["rss"])
                    assert vb["n"].sum() == (te if ent == "test" else tr).sum()
            finally:
                b.close()
                ref.close()
    finally:
        a.close()


@pytest.mark.parametrize("case", ["two_cov", "na", "cont1"])
def test_fold_handle_against_the_oracle(oracle, case):
    """One fold handle per data set against the CPU oracle driven with the fold's masks written out on the host: one outer
    iteration from a non-trivial start and 31 iterations from the usual inits, at the tolerances of
    tests/test_gpu_parity.py::test_optimize_one_iteration / test_optimize_31_iterations."""
    K = 4
    w, Z, m, _, _ = _workload(case, K)
    ids = _fold_ids(w, 4)
    tr, te = _fold_masks(ids, 2)
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, ctns_confounder=Z)
    a.set_folds(ids)
    b = a.fold(2)
    a.close()
    inc = 1 if m else 0
    A, C = _inits(w, m, K, seed=5, scale=0.3)
    got = b.optimize([x.copy(order="F") for x in A], C.copy(order="F"), K, w.lam, w.lam, w.alpha, tuning=1, max_iter=0,
                     seed=17, inc_continuous=inc)
    ref = oracle.optimize(w.X, w.levels, w.n_levels, A, C, tr, te, w.lam, w.lam, w.alpha, tuning=1, max_iter=0, seed=17,
                          **(dict(ctns=Z) if m else {}))
    assert got["iters"] == ref["iters"]
    for i, x in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], x) < 1e-9
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-9
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
    A, C = _inits(w, m, K, seed=6)
    got = b.optimize([x.copy(order="F") for x in A], C.copy(order="F"), K, w.lam, w.lam, w.alpha, tuning=1, max_iter=30,
                     seed=23, inc_continuous=inc)
    b.close()
    ref = oracle.optimize(w.X, w.levels, w.n_levels, A, C, tr, te, w.lam, w.lam, w.alpha, tuning=1, max_iter=30, seed=23,
                          **(dict(ctns=Z) if m else {}))
    assert got["iters"] == ref["iters"] == 31
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
    assert np.array_equal(got["traj"][:, 9], ref["traj"][:, 9])
    for i, x in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], x) < 1e-6
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-6
    assert got["loss"] == pytest.approx(ref["loss"], rel=1e-9)


def test_source_is_untouched_and_lifetimes():
    K = 12
    w = workloads.small(n=150, p=400, level_counts=(7, 5), K=K, f=0.12, seed=77, with_na=True)
    na = (w.M_train == 0) & (w.M_test == 0)
    tr2, te2 = workloads.holdout_masks(w.n, w.p, 0.2, seed=5)
    tr2, te2 = np.asfortranarray(tr2 * ~na, dtype=np.uint8), np.asfortranarray(te2 * ~na, dtype=np.uint8)
    ids = _fold_ids(w, 3)
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    before = _fit(a, w, 0, K)
    b = a.remask(tr2, te2)
    used = _fit(b, w, 0, K)
    b.close()
    _assert_same_fit(_fit(a, w, 0, K), before)                  # the source after a re-mask was made, used and closed
    # a re-mask of a clone and a clone of a re-mask
    cl = a.clone()
    b = cl.remask(tr2, te2)
    cl.close()
    bc = b.clone()
    _assert_same_fit(_fit(b, w, 0, K), used)
    _assert_same_fit(_fit(bc, w, 0, K), used)
    # a re-mask of a re-mask: back to the first masks
    back = b.remask(w.M_train, w.M_test)
    _assert_same_fit(_fit(back, w, 0, K), before)
    back.close()
    # four threads at once: the source, the re-mask, its clone, a fold handle — each bit-identical to its fit alone
    a.set_folds(ids, 3)
    f2 = a.fold(2)
    handles = [a, b, bc, f2]
    lams = [1.0, 3.0, 5.0, 2.0]
    alone = [_fit(hd, w, 0, K, lam=lam) for hd, lam in zip(handles, lams)]
    out, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                out[i] = _fit(handles[i], w, 0, K, lam=lams[i])
        except Exception as e:
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for got, ref in zip(out, alone):
        _assert_same_fit(got, ref)
    a.close()                                                   # the source goes first: the others keep the shared arrays
    _assert_same_fit(_fit(b, w, 0, K), used)
    f2b = f2.fold(2)                                            # a derived handle carries the fold ids
    _assert_same_fit(_fit(f2b, w, 0, K, lam=2.0), alone[3])
    for hd in (b, bc, f2, f2b):
        hd.close()


def _free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_remask_shares_x_and_returns_its_memory():
    w = workloads.small(n=2000, p=6000, level_counts=(12, 5), K=8, f=0.1, seed=31, with_na=True)
    na = (w.M_train == 0) & (w.M_test == 0)
    tr2, te2 = workloads.holdout_masks(w.n, w.p, 0.15, seed=6)
    tr2, te2 = np.asfortranarray(tr2 * ~na, dtype=np.uint8), np.asfortranarray(te2 * ~na, dtype=np.uint8)
    ldn = (w.n + CHUNK - 1) // CHUNK * CHUNK
    x_bytes, slack = 8 * w.p * ldn, 32 << 20
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    _fit(a, w, 0, 8, max_iter=2)         # (the runtime's first launches have allocated what they allocate)
    f0 = _free_bytes()
    b = a.remask(tr2, te2)
    f1 = _free_bytes()
    ref = api.InsiderData(w.X, w.levels, tr2, te2)
    f2 = _free_bytes()
    print(f"free-memory drop: remask {(f0 - f1) / 2 ** 20:.1f} MB, create {(f1 - f2) / 2 ** 20:.1f} MB, X {x_bytes / 2 ** 20:.1f} MB; "
          f"shared {b.info('data_bytes_shared') / 2 ** 20:.1f} MB, own {b.info('data_bytes_own') / 2 ** 20:.1f} MB, "
          f"created own {ref.info('data_bytes_own') / 2 ** 20:.1f} MB")
    assert b.info("data_bytes_shared") >= x_bytes
    assert b.info("data_bytes_own") <= ref.info("data_bytes_own") - x_bytes
    assert ref.info("data_bytes_shared") == 0
    assert (f1 - f2) - (f0 - f1) >= x_bytes - slack
    for hd in (a, b, ref):
        hd.close()
    ids = _fold_ids(w, 3)
    free = []
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2], [2, 3, 0, 1]):
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        ds.set_folds(ids, 3)
        hs = [ds] + [ds.fold(f) for f in (1, 2, 3)]
        for hd in hs:
            _fit(hd, w, 0, 8, max_iter=2)
        for i in order:
            hs[i].close()
        free.append(_free_bytes())
    print("free memory after each round (MB):", [round(v / 2 ** 20, 1) for v in free])
    assert abs(free[-1] - free[0]) < slack, free


def _cv_object(folds=3):
    rng = np.random.default_rng(4)
    conf = workloads.cyclic_levels(60, (5, 3))
    A = [rng.standard_normal((5, 4)), rng.standard_normal((3, 4))]
    data = sum(A[i][conf[:, i] - 1] for i in range(2)) @ rng.standard_normal((4, 80)) + 0.5 * rng.standard_normal((60, 80))
    data[rng.random(data.shape) < 0.03] = np.nan
    return api.insider(data, conf, split_ratio=0.15, tuning_iter=8, max_iter=15, seed=99, folds=folds)


def test_tune_with_folds_equals_the_hand_written_loop(tmp_path):
    obj = _cv_object(3)
    lat, lam, alp = np.array([3, 4]), [1.0, 3.0], [0.2, 0.5]
    out = api.tune(obj, latent_dimension=lat, lambda_=lam, alpha=alp, rng=np.random.default_rng(7), folds=True,
                   out_dir=str(tmp_path))
    conc = api.tune(obj, latent_dimension=lat, lambda_=lam, alpha=alp, rng=np.random.default_rng(7), folds=True, concurrent=2)
    for k in ("rank_tuning", "reg_tuning", "rank_tuning_folds", "reg_tuning_folds", "rank_tuning_test_sd", "reg_tuning_test_sd"):
        np.testing.assert_array_equal(conc[k], out[k], err_msg=k)
    assert conc["latent_rank"] == out["latent_rank"]
    # by hand: created data set, folds derived from it, the reference's order of draws, copies of the inits per fold
    ds = api.InsiderData(obj["data"], obj["confounder"], obj["train_indicator"], obj["test_indicator"])
    ds.set_folds(obj["fold_id"], 3)
    hs = [ds.fold(f) for f in (1, 2, 3)]
    n_f = np.array([(obj["fold_id"] == f).sum() for f in (1, 2, 3)], dtype=np.float64)
    rng = np.random.default_rng(7)
    prm = obj["params"]

    def point(K, l_, a_):
        cfd, col = api._fresh_inits(obj, K, rng)
        r = [hd.optimize([x.copy(order="F") for x in cfd], col.copy(order="F"), K, l_, l_, a_, 1, prm["global_tol"],
                         prm["sub_tol"], prm["tuning_iter"], seed=99) for hd in hs]
        return [v["train_rmse"] for v in r], [v["test_rmse"] for v in r]

    rank_rows = [point(int(K), 0.1, 0.0) for K in lat]
    te = np.array([r[1] for r in rank_rows])
    np.testing.assert_array_equal(out["rank_tuning_folds"], te)
    np.testing.assert_array_equal(out["rank_tuning"][:, 1], np.array([r[0] for r in rank_rows]).mean(axis=1))
    np.testing.assert_array_equal(out["rank_tuning"][:, 2], np.sqrt((te * te * n_f).sum(axis=1) / n_f.sum()))
    K = int(lat[int(np.argmin(out["rank_tuning"][:, 2]))])
    assert out["latent_rank"] == K
    grid_rows = [point(K, l_, a_) for a_ in alp for l_ in lam]
    te = np.array([r[1] for r in grid_rows])
    np.testing.assert_array_equal(out["reg_tuning_folds"], te)
    np.testing.assert_array_equal(out["reg_tuning"][:, 2], np.array([r[0] for r in grid_rows]).mean(axis=1))
    np.testing.assert_array_equal(out["reg_tuning"][:, 3], np.sqrt((te * te * n_f).sum(axis=1) / n_f.sum()))
    np.testing.assert_array_equal(out["reg_tuning_test_sd"], te.std(axis=1, ddof=1))
    for hd in hs + [ds]:
        hd.close()
    assert np.loadtxt(tmp_path / f"insider_R{K}_reg_tuning_result_folds.csv", delimiter=",").shape == (4, 5)
    assert np.loadtxt(tmp_path / f"insider_R{K}_reg_tuning_result.csv", delimiter=",").shape == (4, 4)


def test_tune_then_fit_on_a_remask_equals_two_separate_creates(monkeypatch):
    """fit() after tune() now re-masks the tune data set (api._resident) instead of uploading X again: the tables and the
    fitted model must equal, bit for bit, those of two separately created data sets."""
    def run():
        obj = _cv_object(None)
        t = api.tune(obj, latent_dimension=np.array([4]), lambda_=[1.0, 3.0], alpha=[0.2, 0.5], rng=np.random.default_rng(7))
        obj = api.fit(obj, latent_dimension=4, lambda_=3.0, alpha=0.2, partition=1, rng=np.random.default_rng(11))
        return t, obj

    t1, o1 = run()
    assert o1["_resident_fit"].info("data_bytes_shared") > 0        # it IS a re-mask

    def separate(obj, which):
        key = "_resident_" + which
        if key not in obj:
            if which == "tune":
                tr, te = obj["train_indicator"], obj["test_indicator"]
            else:
                tr, te = obj["train_indicator"] + obj["test_indicator"], obj["na_indicator"]
            obj[key] = api.InsiderData(obj["data"], obj["confounder"], tr, te)
        return obj[key]

    monkeypatch.setattr(api, "_resident", separate)
    t2, o2 = run()
    assert o2["_resident_fit"].info("data_bytes_shared") == 0
    np.testing.assert_array_equal(t1["reg_tuning"], t2["reg_tuning"])
    assert np.array_equal(o1["column_factor"], o2["column_factor"]) and o1["loss"] == o2["loss"]
    for k in o2["cfd_matrices"]:
        assert np.array_equal(o1["cfd_matrices"][k], o2["cfd_matrices"][k])
    assert np.array_equal(o1["traj"], o2["traj"], equal_nan=True)
    assert o1["test_rmse"] == o2["test_rmse"] and o1["train_rmse"] == o2["train_rmse"]
    # the other order: fit() first, tune() re-masks the fit data set
    monkeypatch.undo()
    obj = _cv_object(None)
    obj = api.fit(obj, latent_dimension=4, lambda_=3.0, alpha=0.2, partition=1, rng=np.random.default_rng(11))
    t3 = api.tune(obj, latent_dimension=np.array([4]), lambda_=[1.0, 3.0], alpha=[0.2, 0.5], rng=np.random.default_rng(7))
    assert obj["_resident_tune"].info("data_bytes_shared") > 0
    np.testing.assert_array_equal(t3["reg_tuning"], t2["reg_tuning"])
    assert np.array_equal(obj["column_factor"], o2["column_factor"])


def test_errors_leave_the_source_usable():
    K = 5
    w = workloads.small(n=50, p=60, K=K)
    a = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    before = _fit(a, w, 0, K)
    lib = _lib.load()

    def status(fn):
        with pytest.raises(InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: a.remask(w.M_train[:, :-1], w.M_test[:, :-1])) == _lib.ERR_ARG      # wrong mask shape
    assert status(lambda: a.remask(w.M_train.T, w.M_test.T)) == _lib.ERR_ARG
    assert status(lambda: a.fold(1)) == _lib.ERR_ARG                                          # fold() before set_folds()
    out = ctypes.c_void_p()
    assert lib.insider_hip_remask_fold(a._h, 1, ctypes.byref(out)) == _lib.ERR_ARG and not out  # ... in the library too
    ids = _fold_ids(w, 3)
    assert status(lambda: a.set_folds(ids, 2)) == _lib.ERR_ARG                                # ids above F
    assert status(lambda: a.set_folds(ids[:-1], 3)) == _lib.ERR_ARG
    u8 = np.asfortranarray(ids, dtype=np.uint8)
    assert lib.insider_hip_set_folds(a._h, _lib.ptr(u8, ctypes.c_uint8), 2) == _lib.ERR_ARG   # ... in the library too
    assert lib.insider_hip_set_folds(a._h, _lib.ptr(u8, ctypes.c_uint8), 0) == _lib.ERR_ARG
    assert lib.insider_hip_remask(a._h, None, None, ctypes.byref(out)) == _lib.ERR_ARG
    a.set_folds(ids, 3)
    assert status(lambda: a.fold(0)) == _lib.ERR_ARG and status(lambda: a.fold(4)) == _lib.ERR_ARG
    for f in (0, 4):
        assert lib.insider_hip_remask_fold(a._h, f, ctypes.byref(out)) == _lib.ERR_ARG and not out
    # a gene-sharded source
    a.set_shard(0, 0, 2, lambda ptr, count, stream: None)
    assert status(lambda: a.remask(w.M_train, w.M_test)) == _lib.ERR_UNSUPPORTED
    assert status(lambda: a.fold(1)) == _lib.ERR_UNSUPPORTED
    a.set_shard(0, 0, 1)
    _assert_same_fit(_fit(a, w, 0, K), before)
    b = a.fold(3)
    assert b.info("data_bytes_shared") > 0
    b.close()
    a.close()


def test_cli_tune_with_folds_writes_the_per_fold_table(tmp_path):
    from insider_amd import fit as cli
    rng = np.random.default_rng(4)
    conf = workloads.cyclic_levels(60, (5, 3))
    A = [rng.standard_normal((5, 4)), rng.standard_normal((3, 4))]
    data = sum(A[i][conf[:, i] - 1] for i in range(2)) @ rng.standard_normal((4, 50)) + 0.5 * rng.standard_normal((60, 50))
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    out = tmp_path / "out"
    assert cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--tune", "--folds", "3", "--ranks",
                     "3", "4", "--lambdas", "1", "3", "--alphas", "0.2", "--tuning-iter", "5", "--out", str(out)]) == 0
    tab = np.loadtxt(out / "tune_folds.csv", delimiter=",")
    assert tab.shape == (2 + 2, 3 + 3)                      # two ranks, then two grid points: rank, lambda, alpha, 3 folds
    assert list(tab[:2, 0]) == [3.0, 4.0] and np.isnan(tab[:2, 1:3]).all()
    assert list(tab[2:, 1]) == [1.0, 3.0] and list(tab[2:, 2]) == [0.2, 0.2]
    assert np.isfinite(tab[:, 3:]).all() and (tab[:, 3:] > 0).all()
    import json
    res = json.load(open(out / "tune.json"))
    assert np.array(res["reg_tuning_folds"]).shape == (2, 3) and np.array(res["reg_tuning"]).shape == (2, 4)
    np.testing.assert_array_equal(np.array(res["reg_tuning_folds"]), tab[2:, 3:])
