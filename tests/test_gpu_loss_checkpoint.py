"""The loss checkpoint, evaluator by evaluator, against a direct residual sum (tests/loss_reference.py, longdouble).

Every number a caller judges a fit by (train_rmse, test_rmse, loss, the trajectory rows, the global_tol stop, the decay
ladder, tune()'s choice) comes from per-gene sums that the column kernels write as a difference of sums of squares,
sse_train[j] = yy[j] - b'(q + g), and on data without NA entries sse_test[j] = ss_held + b'(R'R b - (q - g) - 2 qc); with NA
entries k_test_sse_list forms the test residuals directly from the held-out lists' flags.  k_loss_reduce sums them.  The
identity is written out in k_cd_cols<W, WPB>, k_ridge_cols, k_cd_cols_reg (nine instantiations), k_cd_cols_r16 and
k_ridge_cols_reg (nine instantiations); which copy runs follows the K band, lambda alpha and cd_variant.

Driver: optimize(max_iter = 0) from planted factors.  Trajectory row 0 (iter -1) is the evaluation of exactly the caller's
(A, C) (a column solve that only evaluates), compared with evaluate() of the inputs; row 1 (iter 0) is the checkpoint taken by
or after the first solve, compared with evaluate() of the returned factors.  The kernels are asserted by name from the
tables of tests/dispatch_rules.py, written out by hand.

Contract checked on both rows (u = 2^-53; loss_reference.bounds() derives the bounds):
    every value finite where the contract says a number, NaN exactly where it says NaN (test_rmse: tuning = 0, no test entry)
    sse_half >= 0, both RMSEs >= 0
    |2 sse_half - sse_train_ref| <= bound_stats,   |train_rmse^2 cnt_train - sse_train_ref| <= bound_stats + 4u sse
    the test sum the same, against bound_stats (no NA: from statistics) or bound_direct (NA: explicit residuals)
    the three penalties within (max(sum L, p) K + 16) u relative
    loss = the sum of the device's own four components to 4u relative
A handle serves the calls that share a data set, and the references (longdouble, on the CPU) are computed by a few threads
while the next call runs on the GPU.  The last test prints the largest error / bound per evaluator.
"""
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from insider_amd import _lib, api
from tests import dispatch_rules as dr
from tests import loss_reference as lr
from tests.dispatch_rules import REGIMES, SOLVER
from tests.dispatch_rules import loss_stats_kernel as stats_kernel
from tests.support import need_gpu  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

U = lr.U
LD = lr.LD
WORST = {}     # (evaluator, which sum) -> largest error / bound seen
REACHED = []   # (col_solver, col_eval) of every call of test a
TIMES = {"create": 0.0, "optimize": 0.0, "reference (CPU seconds, on threads)": 0.0}
POOL = ThreadPoolExecutor(8)
LOCK = threading.Lock()


def names(ds):
    return _lib.COL_SOLVERS[int(ds.info("col_solver"))], _lib.COL_SOLVERS[int(ds.info("col_eval"))]


# (REGIMES: (lambda, alpha) of the column update; the two last leave row 1 a near-exact fit on the cd_reg and ridge_reg evaluators)
# lambda1 of the row update: the column update's lambda, and 30 where that is 0
LAM1 = {"enet": 30.0, "lasso": 30.0, "nol1": 30.0, "ridge": 30.0, "enet_tiny": 1e-12, "ridge_tiny": 1e-12}
# a gene held out entirely has the system 0 b = 0: solvable only under a penalty that is not vanishing
HELD_GENE = {"enet": True, "lasso": True, "nol1": False, "ridge": True, "enet_tiny": False, "ridge_tiny": False}


def expected(regime, variant, K):
    """(col_solver, col_eval) of the call."""
    s = dr.col_solver(regime, variant, K)
    return s, dr.col_eval(s)


# the statistics paths (the PATHS options of test_gpu_col_solvers.py; every option set in every call: a handle serves several)
PATHS = {"fast": dict(row_merged=2, col_factored=2, row_counts=0), "pair": dict(row_merged=2, col_factored=3, row_counts=1),
         "lists": dict(row_merged=0, col_factored=0, row_counts=1)}


# ----------------------------------------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------------------------------------
def _note(evaluator, which, err, bound):
    ratio = float(err / bound) if bound > 0 else (0.0 if err == 0 else float("inf"))
    with LOCK:
        WORST[(evaluator, which)] = max(WORST.get((evaluator, which), 0.0), ratio)
    return ratio


def _sums(d, A, C):
    """The residual sums and the bounds of (A, C) on data set d: what does not depend on the penalties."""
    t = time.perf_counter()
    out = lr.residual_sums(d["Xl"], d["levels"], d["n_levels"], A, C, d["M_train"], d["M_test"], d["tuning"], ctns=d["ctns"],
                           with_bounds=True)
    with LOCK:
        TIMES["reference (CPU seconds, on threads)"] += time.perf_counter() - t
    return out


def check_row(row, ref, bnd, d, evaluator, tag):
    """One trajectory row against the reference of the factors it evaluates (module docstring)."""
    train_rmse, test_rmse, sse_half, row_reg, col_reg, l1_reg, loss = (float(v) for v in row[1:8])
    na = d["tuning"] == 1 and lr.has_na(d["M_train"], d["M_test"])
    for name, v in (("train_rmse", train_rmse), ("sse_half", sse_half), ("row_reg_half", row_reg), ("col_reg_half", col_reg),
                    ("l1_reg", l1_reg), ("loss", loss)):
        assert np.isfinite(v), (tag, name, v)
    assert np.isnan(test_rmse) == np.isnan(ref["test_rmse"]), (tag, test_rmse, ref["test_rmse"], ref["cnt_test"])
    assert sse_half >= 0 and train_rmse >= 0 and (np.isnan(test_rmse) or test_rmse >= 0), (tag, sse_half, train_rmse, test_rmse)
    bs = bnd["bound_stats"]
    # the train sum, as sse_half and through train_rmse
    e1 = abs(2 * LD(sse_half) - ref["sse_train"])
    e2 = abs(LD(train_rmse) ** 2 * ref["cnt_train"] - ref["sse_train"])
    r1 = _note(evaluator, "train", e1, bs)
    assert e1 <= bs, (tag, evaluator, "train sum", 2 * sse_half, float(ref["sse_train"]), "error / bound", r1)
    assert e2 <= bs + 4 * U * ref["sse_train"], (tag, evaluator, float(e2), float(bs))
    # the test sum through test_rmse
    if not np.isnan(test_rmse):
        bt, who, which = (bnd["bound_direct"], "test_sse_list", "test_direct") if na else (bs, evaluator, "test_stats")
        e3 = abs(LD(test_rmse) ** 2 * ref["cnt_test"] - ref["sse_test"])
        bt = bt + 4 * U * ref["sse_test"]
        r3 = _note(who, which, e3, bt)
        assert e3 <= bt, (tag, who, "test sum", test_rmse ** 2 * ref["cnt_test"], float(ref["sse_test"]), "error / bound", r3)
    # the penalties, and the loss as the sum of the device's own components
    for name, v in (("row_reg_half", row_reg), ("col_reg_half", col_reg), ("l1_reg", l1_reg)):
        assert abs(LD(v) - ref[name]) <= bnd["rel_penalty"] * ref[name], (tag, name, v, float(ref[name]))
    parts = sse_half + row_reg + col_reg + l1_reg
    assert abs(loss - parts) <= 4 * U * parts, (tag, loss, parts)


def launch(ds, d, lam1, lam2, alpha, options=(), want=None, want_stats=None, tag="", record=None):
    """One call on an open data set; the kernels asserted by name.  -> what finish() checks"""
    A = [a.copy(order="F") for a in d["A"]]
    C = d["C"].copy(order="F")
    for k, v in options:
        ds.set_option(k, v)
    t = time.perf_counter()
    got = ds.optimize(A, C, d["K"], lam1, lam2, alpha, tuning=d["tuning"], max_iter=0, seed=11,
                      inc_continuous=1 if d["ctns"] is not None else 0)
    TIMES["optimize"] += time.perf_counter() - t
    reached = names(ds)
    if record is not None:
        record.append(reached)
    if want is not None:
        assert reached == want, (tag, reached, want)
    if want_stats is not None and d["tuning"] == 1:
        stats = _lib.COL_STATS_KERNELS[int(ds.info("col_stats_kernel"))]
        assert stats == want_stats, (tag, stats, want_stats)
    assert got["traj"].shape[0] == 2 and list(got["traj"][:, 0]) == [-1, 0], got["traj"][:, 0]
    return got, reached[1] if reached[1] != "none" else reached[0], (lam1, lam2, alpha), tag


def finish(d, got, evaluator, pen, tag):
    """Both rows of a call against their references (on a thread of POOL).  -> the two trajectory rows"""
    traj = got["traj"]
    ref0 = lr.with_penalties(d["ref0"].result(), d["A"], d["C"], *pen)
    check_row(traj[0], ref0, ref0["bounds"], d, evaluator, tag + " row 0")
    A1 = [got["row_matrices"][f"factor{i}"] for i in range(len(d["A"]))]
    ref1 = lr.with_penalties(_sums(d, A1, got["column_factor"]), A1, got["column_factor"], *pen)
    check_row(traj[1], ref1, ref1["bounds"], d, evaluator, tag + " row 1")
    assert got["train_rmse"] == traj[1, 1] and got["loss"] == traj[1, 7]
    assert got["test_rmse"] == traj[1, 2] or (np.isnan(got["test_rmse"]) and np.isnan(traj[1, 2]))
    return traj


def run_groups(groups):
    """groups: (data set, calls) pairs; every call of ``calls`` (keyword arguments of launch()) runs on one handle of its data
    set (creating it costs more than a call), and each is checked whatever the others did; the references are awaited after the
    last call.  -> the trajectory rows of each call"""
    failed, jobs = [], []
    for d, calls in groups:
        d["Xl"] = np.asarray(d["X"], dtype=LD)
        d["ref0"] = POOL.submit(_sums, d, d["A"], d["C"])   # the reference of the planted factors: row 0 of every call
        t = time.perf_counter()
        ds = api.InsiderData(d["X"], d["levels"], d["M_train"], d["M_test"], ctns_confounder=d["ctns"])
        TIMES["create"] += time.perf_counter() - t
        try:
            for kw in calls:
                try:
                    jobs.append(POOL.submit(finish, d, *launch(ds, d, **kw)))
                except AssertionError as e:
                    failed.append(str(e))
        finally:
            ds.close()
    trajs = []
    for job in jobs:
        try:
            trajs.append(job.result())
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    return trajs


def run_all(d, calls):
    return run_groups([(d, calls)])


# ----------------------------------------------------------------------------------------------------------------------
# a. every evaluator: rows 0 and 1 on every (regime, cd_variant, K) cell, data kind and condition
# ----------------------------------------------------------------------------------------------------------------------
# The K inside a band are there for the (SLOTS, KMAX) instantiations of REG_DISPATCH, which cd_variant 0 alone launches: the other
# variants run the band edges.  (ridge, 1) at K > 32 is the same kernel as cd_variant 0.
MIDDLE = (18, 20, 22, 24, 25, 26, 28, 30)
CELLS = [(r, v, K) for (r, v) in SOLVER for K in lr.KS
         if not (v != 0 and K in MIDDLE) and not (r == "ridge" and v == 1 and K > 32)]


@pytest.mark.parametrize("cond", lr.CONDITIONS, ids=[f"s{s:g}-o{o:g}" for s, o in lr.CONDITIONS])
@pytest.mark.parametrize("data", lr.DATA)
@pytest.mark.parametrize("K", lr.KS)
def test_initial_and_first_checkpoint_every_evaluator(K, data, cond):
    """Every (regime, cd_variant) cell of this K, one call each, on one handle per data set (the data with and without the
    wholly held-out gene)."""
    groups = []
    for held in (True, False):
        d = lr.planted(K, *cond, data, lr.case_seed(K, cond), held_gene=held)
        cells = [(r, v) for r, v, k in CELLS if k == K and HELD_GENE[r] == held]
        groups.append((d, [dict(lam1=LAM1[r], lam2=REGIMES[r][0], alpha=REGIMES[r][1], options=[("cd_variant", v)],
                                want=expected(r, v, K), tag=f"{r}-v{v}-K{K}-{data}-{cond}", record=REACHED) for r, v in cells]))
    run_groups(groups)


# ----------------------------------------------------------------------------------------------------------------------
# b. an exact fit: the sums are rounding of either sign per gene; no row may be NaN or negative
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", lr.DATA)
@pytest.mark.parametrize("K", lr.EXACT_KS)
@pytest.mark.parametrize("seed", lr.EXACT_SEEDS)
@pytest.mark.parametrize("offset", lr.EXACT_OFFSETS, ids=["o0", "o100"])
def test_exact_fit_is_never_nan(offset, seed, K, data):
    """sigma = 0 under a vanishing penalty, so that both rows are exact fits; the three statistics paths on one handle.  Before
    k_loss_reduce took a negative per-gene value as 0 the summed value could come out negative and the RMSE NaN: the sign is
    luck of the summation order per seed.  (On the MI355X, 425 of these 576 calls reported a NaN without that rule.)"""
    lam, alpha = REGIMES["enet_tiny"]
    d = lr.planted(K, 0.0, offset, data, seed, held_gene=False)
    run_all(d, [dict(lam1=LAM1["enet_tiny"], lam2=lam, alpha=alpha, options=list(PATHS[paths].items()),
                     want=expected("enet_tiny", 0, K), want_stats=stats_kernel(paths, K),
                     tag=f"exact-o{offset:g}-seed{seed}-K{K}-{data}-{paths}") for paths in PATHS])


# ----------------------------------------------------------------------------------------------------------------------
# c. the test sum from the held-out lists' flags (data with NA entries)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", lr.LIST_MASKS)
@pytest.mark.parametrize("cond", lr.LIST_CONDITIONS, ids=["s0.5-o0", "s0-o100"])
@pytest.mark.parametrize("K", lr.LIST_KS)
def test_test_sum_from_flagged_lists(K, cond, masks):
    d = lr.list_case(K, cond, masks)
    g = len(lr.LIST_LENGTHS)
    if masks == "lists":
        held = (d["M_train"] == 0).sum(axis=0)
        assert tuple(held[:g]) == lr.LIST_LENGTHS and held[g] == 40
        assert not d["M_test"][:, g].any() and d["M_test"][:, g + 1].all()
    lam, alpha = REGIMES["enet"]
    traj, = run_all(d, [dict(lam1=LAM1["enet"], lam2=lam, alpha=alpha, want=expected("enet", 0, K),
                             tag=f"lists-K{K}-{cond}-{masks}")])
    if masks == "lists":
        assert np.isfinite(traj[:, 2]).all()
    else:   # no test entry anywhere: NaN, and the train value is the reference's all the same (checked in finish())
        assert np.isnan(traj[:, 2]).all()


# ----------------------------------------------------------------------------------------------------------------------
# d. shapes: k_loss_reduce's stride of 256 below, at and above one and two trips; the partial last block of the launches of
#    four genes per block
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", lr.SHAPE_DATA)
@pytest.mark.parametrize("n", list(lr.SHAPE_LEVELS))
@pytest.mark.parametrize("p", lr.SHAPE_PS)
def test_shape_edges(p, n, data):
    lam, alpha = REGIMES["enet"]
    run_groups([(lr.shape_case(p, n, data, cond), [dict(lam1=LAM1["enet"], lam2=lam, alpha=alpha, want=expected("enet", 0, lr.SHAPE_K),
                                                        tag=f"shape-p{p}-n{n}-{data}-{cond}")]) for cond in lr.SHAPE_CONDITIONS])


# ----------------------------------------------------------------------------------------------------------------------
# e. a continuous block: R carries Z A_c
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", lr.CTNS_DATA)
@pytest.mark.parametrize("cond", lr.CTNS_CONDITIONS, ids=["s0.5-o0", "s1e-06-o100"])
@pytest.mark.parametrize("K", lr.CTNS_KS)
def test_continuous_block(K, cond, data):
    lam, alpha = REGIMES["enet"]
    run_all(lr.ctns_case(K, cond, data),
            [dict(lam1=LAM1["enet"], lam2=lam, alpha=alpha, options=list(PATHS[paths].items()), want=expected("enet", 0, K),
                  want_stats=stats_kernel(paths, K, m=2), tag=f"ctns-K{K}-{cond}-{data}-{paths}") for paths in ("pair", "lists")])


# ----------------------------------------------------------------------------------------------------------------------
# f. the checkpoint is a fixed-order computation: a repeat gives the same bits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", lr.DATA)
@pytest.mark.parametrize("regime,K", [("enet", 9), ("enet", 40), ("enet", 56), ("ridge", 20), ("ridge", 40), ("enet_tiny", 30)])
def test_repeat_is_bit_identical(regime, K, data):
    lam, alpha = REGIMES[regime]
    d = lr.planted(K, 0.0 if regime == "enet_tiny" else 0.5, 0.0, data, 900 + K, held_gene=HELD_GENE[regime])

    def call(ds):
        return ds.optimize([a.copy(order="F") for a in d["A"]], d["C"].copy(order="F"), K, LAM1[regime], lam, alpha,
                           tuning=d["tuning"], max_iter=0, seed=11)["traj"][:, 1:8].copy()

    rows = []
    for calls in (2, 1):   # twice on one handle, once on a fresh one
        ds = api.InsiderData(d["X"], d["levels"], d["M_train"], d["M_test"])
        try:
            rows += [call(ds) for _ in range(calls)]
        finally:
            ds.close()
    for other in rows[1:]:
        assert rows[0].shape == other.shape == (2, 7)
        assert np.array_equal(rows[0].view(np.uint64), other.view(np.uint64)), (rows[0], other)


# ----------------------------------------------------------------------------------------------------------------------
def test_zz_every_evaluator_reached_and_report():
    for key in sorted(WORST):
        print(f"loss checkpoint, largest error / bound: {key[0]:>14s} {key[1]:<12s} {WORST[key]:.2e}")
    print("loss checkpoint, seconds: " + ", ".join(f"{k} {v:.1f}" for k, v in TIMES.items()))
    assert all(v <= 1 for v in WORST.values())
    table = {expected(r, v, K) for r, v, K in CELLS}
    assert set(REACHED) <= table
    if len(REACHED) == len(CELLS) * len(lr.DATA) * len(lr.CONDITIONS):   # (the whole of test a ran in this session)
        assert set(REACHED) == table, table - set(REACHED)
