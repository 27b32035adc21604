"""k_col_paircnt4 forming each gene's rows of Q = S A and Qheld = S^held A itself (option "stats_own_q", FitPlan::stats_own_q):
the option on against the option off in the same build, the on-path against the float64 reference and the oracle.

With the option on the two products over the genes (k_mm_rows2 / k_mm_rows) and their stream joins are not launched; the
statistics kernel sums a_l S[j][l] over the levels in two free columns of its second product, quad of levels by quad, instead
of the products' order, so Q and Qheld — hence q of the densified record and the fits — agree with the off-path to rounding,
not by bits.  The Gram part of the record does not depend on the option: it is compared by bits.  (K = 15 and 31 have one
free column only and keep the products: not among this file's K.)

Shapes: two covariates, so that the merged row update and the pair-count statistics are what runs (asserted through
info("col_stats_path") / info("row_merged") / info("col_stats_kernel") / info("col_stats_own_q"), not assumed); n = 150; p in
{5, 37, 130} (not a multiple of 4, fewer genes than one block, more than one block of the statistics kernel); level counts
(17, 3) and (33, 16); K in {1, 7, 16, 17, 30}; 10 % and 50 % held out; gene 0 has no held-out entry, gene 2 keeps every sample
of level 1 of covariate 0 in training (no gene at p = 5 beyond those of test_gpu_col_stats.data()).

Bounds.  The statistics: G and the corner never see the option, and wherever the larger covariate comes first q does not
either — below 16384 genes the products run on k_mm_rows, which adds the levels up in stacked order as one chain of fused
multiply-adds, and so does the kernel's second product when its covariate order is the stacked order: these cases are compared
BY BITS, so that one level in a wrong quad cannot pass.  With the larger covariate second the kernel's order is not the stacked
order; there dq is held against the distance between two EXISTING forms on the same inputs with no factor: look-up against
pair-count (both with the products; they differ in G alone, |dG| / |R'R|), the larger over all cases.  The unit of dq in those
two cases is |dq| / | |X_j|' |R| |: both distances are those of re-ordered sums, whose rounding error scales with the sum of
the MAGNITUDES of the terms (|fl(sum) - sum| <= gamma_n sum |t_i|), not with the value of the sum.  For G = sum r_i r_i'
(positive semi-definite terms) that sum is |R'R|, the yardstick's unit; for q = sum x_ij r_i, whose terms change sign, it is
| |X_j|' |R| |.  In check_values' unit |dq| / |X_j'R| this build measures 1.08e-15 (K = 7) and 6.2e-16 (K = 30) on the two
cases against the yardstick's 1.417e-16: a distance in that unit says how far the signed sum cancels (about 1 / sqrt(n) of its
terms on this file's data), and the yardstick, taken on sums that do not cancel, does not carry over to it.  In the terms' unit
the two cases measure 1.025e-16 and 7.18e-17.  Both units are printed; the on-path passes check_values' own 1e-12 in |X_j'R| in every case.  The fits: the larger of look-up against pair-count and row_merged = 0 against 2, as relerr of each factor, the
larger over all fits; the fits with the larger covariate first are compared by bits as well.  Each test prints its figures.

Serial against concurrent: the kernel deals its genes by ticket, so which wave forms which gene's Q depends on what runs
beside it.  A clone fits in a second thread at the same time as its source, and tune(concurrent = 2) is compared with the
serial tune(), all by bits.

Measured on MI355X: profiles/handoff_fused/README.md.  At the benchmark's size the products run on k_mm_rows2 in another
order: the fitted factors of the two builds differ by 5.5e-13 (column factor) and 2.3e-13 (row factors) after 31 iterations.
"""
import numpy as np
import pytest

import threading

from insider_amd import api, workloads
from tests import test_gpu_col_stats as cs
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

KS = (1, 7, 16, 17, 30)
LEVELS = ((17, 3), (33, 16))
PS = (5, 37, 130)
N = 150

PAIR_OFF = dict(col_factored=3, stats_own_q=0)
PAIR_ON = dict(col_factored=3, stats_own_q=2)
LOOKUP = dict(col_factored=2, stats_own_q=0)


# ----------------------------------------------------------------------------------------------------------------------
# a. the densified record: insider_hip_col_stats
# ----------------------------------------------------------------------------------------------------------------------
def stats_cases():
    out = []
    for i, K in enumerate(KS):
        for j, lv in enumerate(LEVELS):
            for k, p in enumerate(PS):
                f = 0.1 if (i + j + k) % 2 == 0 else 0.5
                out.append(cs.case(f"hf-K{K}-L{lv[0]}x{lv[1]}-p{p}-f{int(100 * f)}", K, lv, p=p, n=N, f=f))
    # the larger covariate second: the kernel walks the covariates by decreasing level count, not in stacked order
    out += [cs.case(f"hf-K{K}-L16x33-p37-f50", K, (16, 33), p=37, n=N, f=0.5) for K in (7, 30)]
    return out


STATS_CASES = stats_cases()
STATS_BY_ID = {c["id"]: c for c in STATS_CASES}
assert len(STATS_BY_ID) == len(STATS_CASES)
assert {c["f"] for c in STATS_CASES if c["K"] == 30} == {0.1, 0.5}


def run_stats(c, opts, A, own_q):
    ds = cs.handle(dict(c, opts=opts))
    try:
        got = ds.col_stats(A)
        assert int(ds.info("col_stats_path")) == (1 if opts["col_factored"] == 2 else 2), c["id"]
        kernel = cs.launched(ds)[0]
        assert kernel == ("factored" if opts["col_factored"] == 2 else "paircnt4_ms4"), (c["id"], kernel)
        assert int(ds.info("col_stats_own_q")) == own_q, c["id"]
        assert (int(ds.info("col_q_kernel")) == 0) == bool(own_q), c["id"]      # on: no product over the genes was launched
        return got
    finally:
        ds.close()


def stacked_order(c):
    """The kernel walks the covariates by decreasing level count: is that the stacked order?"""
    return list(c["levels"]) == sorted(c["levels"], reverse=True)


def term_scale(c, A):
    """| |X_j|' |R| | per gene: the sum of the magnitudes of the terms of q (module docstring)."""
    lev, X, Mtr, Mte, Z = cs.data(c)
    R = sum(A[t][lev[:, t] - 1] for t in range(len(c["levels"])))
    return np.linalg.norm(np.abs(X).T @ np.abs(R), axis=1)


def stats_dist(got, want, ref, sq=None):
    """max over genes of |dG| / |R'R| and of |dq| / |X_j'R| (the units of test_gpu_col_stats.check_values); sq: dq's divisor
    instead."""
    sG, sq = ref[3], ref[4] if sq is None else sq
    eG = np.linalg.norm(got[0] - want[0], axis=(1, 2)) / sG
    eq = np.linalg.norm(got[1] - want[1], axis=1) / sq
    return float(eG.max()), float(eq.max())


@pytest.fixture(scope="module")
def stats_runs():
    """Every case under the three forms, once: {id: (A, reference, lookup, pair off, pair on)}."""
    runs = {}
    for c in STATS_CASES:
        A = cs.factors(c, np.random.default_rng(c["seed"] + 1))
        runs[c["id"]] = (A, cs.reference(c, A), run_stats(c, LOOKUP, A, 0), run_stats(c, PAIR_OFF, A, 0), run_stats(c, PAIR_ON, A, 1))
    return runs


@pytest.fixture(scope="module")
def stats_bound(stats_runs):
    """The yardstick: look-up form against pair-count form, the larger of the two normalised distances over all cases."""
    worst = 0.0
    for cid, (A, ref, look, off, on) in stats_runs.items():
        worst = max(worst, *stats_dist(look, off, ref))
    print(f"\nstatistics yardstick (look-up vs pair-count, max over {len(stats_runs)} cases): {worst:.3e}")
    return worst


@pytest.mark.parametrize("cid", list(STATS_BY_ID))
def test_stats_on_against_off_and_reference(cid, stats_runs, stats_bound):
    """G and the corner by bits; q by bits in stacked order, else within the yardstick; the on-path within check_values' bounds
    of the float64 reference."""
    c = STATS_BY_ID[cid]
    A, ref, look, off, on = stats_runs[cid]
    dG, dq = stats_dist(on, off, ref)
    print(f"\n{cid}: on vs off dG {dG:.3e} dq {dq:.3e}; look-up vs off {stats_dist(look, off, ref)}; bound {stats_bound:.3e}")
    assert np.array_equal(on[0], off[0]), cid            # the Gram part does not see the option
    assert np.array_equal(on[2], off[2]), cid            # ... nor does the corner
    if stacked_order(c):
        assert np.array_equal(on[1], off[1]), (cid, dq)
    else:
        dq_terms = stats_dist(on, off, ref, term_scale(c, A))[1]
        print(f"{cid}: dq / | |X_j|' |R| | {dq_terms:.3e}")
        assert 0.0 < dq_terms <= stats_bound, (cid, dq_terms, dq, stats_bound)
    cs.check_values(dict(c, opts=PAIR_ON), on, A, "stats_own_q", ref=ref)


def beside(jobs, rounds=4):
    """Run the jobs at the same time, each in its own thread, `rounds` times each after a common start: {index: [results]}."""
    gate, out, errs = threading.Barrier(len(jobs)), {i: [] for i in range(len(jobs))}, []

    def work(i):
        try:
            gate.wait(timeout=60)
            for _ in range(rounds):
                out[i].append(jobs[i]())
        except Exception as e:      # (reported by the caller: an assertion in a thread is lost)
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errs and not any(t.is_alive() for t in ts), errs
    return out


def test_stats_on_a_clone_beside_its_source_by_bits(stats_runs):
    """The source and a clone form the statistics at the same time from two threads: the bits of a launch alone."""
    c = STATS_BY_ID["hf-K30-L33x16-p130-f50"]
    A, want = stats_runs[c["id"]][0], stats_runs[c["id"]][4]
    ds = cs.handle(dict(c, opts=PAIR_ON))
    twin = ds.clone()
    try:
        got = beside([lambda: ds.col_stats(A), lambda: twin.col_stats(A)])
        assert int(ds.info("col_stats_own_q")) == 1 and int(twin.info("col_stats_own_q")) == 1
    finally:
        twin.close()
        ds.close()
    for runs in got.values():
        assert len(runs) == 4
        for r in runs:
            for x, y in zip(r, want):
                assert np.array_equal(x, y)


# ----------------------------------------------------------------------------------------------------------------------
# b. fits: 1, 2 and 12 outer iterations from the cold inits and from a non-trivial start
# ----------------------------------------------------------------------------------------------------------------------
FIT_FORMS = {"on": dict(row_merged=2, col_factored=3, stats_own_q=1), "off": dict(row_merged=2, col_factored=3, stats_own_q=0),
             "lookup": dict(row_merged=2, col_factored=2, stats_own_q=0), "unmerged": dict(row_merged=0, col_factored=3, stats_own_q=0)}
ITERS = (1, 2, 12)


def fit_cases():
    out = []
    for i, K in enumerate(KS):
        lv, p = LEVELS[i % 2], PS[(i + 1) % 3]
        for it in ITERS:
            for start in ("cold", "warm"):
                out.append(dict(id=f"hf-fit-K{K}-L{lv[0]}x{lv[1]}-p{p}-it{it}-{start}", K=K, levels=lv, p=p, iters=it, start=start,
                                f=0.1 if (i + it) % 2 == 0 else 0.5, seed=100 + 7 * i))
    # the larger covariate second (the kernel's order of the levels is not the products'): here on and off differ
    for K, it, start in ((7, 12, "cold"), (30, 12, "cold"), (30, 2, "warm"), (17, 1, "warm")):
        out.append(dict(id=f"hf-fit-K{K}-L16x33-p37-it{it}-{start}", K=K, levels=(16, 33), p=37, iters=it, start=start, f=0.5,
                        seed=200 + K))
    return out


FIT_CASES = fit_cases()
FIT_BY_ID = {c["id"]: c for c in FIT_CASES}
_FIT_DATA = {}


def fit_data(c):
    key = (c["K"], c["levels"], c["p"], c["f"], c["seed"], c["start"])
    if key not in _FIT_DATA:
        w = workloads.small(seed=c["seed"], n=N, p=c["p"], level_counts=c["levels"], K=c["K"], f=c["f"])
        w.M_test[:, 0] = 0                                   # gene 0: no held-out entry
        w.M_train[:, 0] = 1
        if c["p"] >= 3:                                      # gene 2: level 1 of covariate 0 wholly in training
            rows = w.levels[:, 0] == 1
            w.M_test[rows, 2] = 0
            w.M_train[rows, 2] = 1
        if c["start"] == "warm":
            rng = np.random.default_rng(c["seed"] + 5)
            w.A0 = [np.asfortranarray(rng.standard_normal(a.shape) * 0.3) for a in w.A0]
            w.C0 = np.asfortranarray(rng.standard_normal(w.C0.shape) * 0.3)
        _FIT_DATA[key] = w
    return _FIT_DATA[key]


def run_fit(c, form, ds=None):
    w = fit_data(c)
    own = ds is None
    if own:
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        for k, v in FIT_FORMS[form].items():
            ds.set_option(k, v)
    try:
        got = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha, tuning=1,
                          max_iter=c["iters"] - 1, seed=4)
        if form in ("on", "off"):
            assert int(ds.info("col_stats_path")) == 2 and int(ds.info("row_merged")) == 1, c["id"]
            assert cs.launched(ds)[0] == "paircnt4_ms4", c["id"]
            assert int(ds.info("col_stats_own_q")) == (1 if form == "on" else 0), c["id"]
        return got
    finally:
        if own:
            ds.close()


def fit_dist(a, b):
    d = [relerr(a["column_factor"], b["column_factor"])]
    d += [relerr(a["row_matrices"][k], b["row_matrices"][k]) for k in sorted(a["row_matrices"])]
    return max(d)


@pytest.fixture(scope="module")
def fit_runs():
    return {c["id"]: {form: run_fit(c, form) for form in FIT_FORMS} for c in FIT_CASES}


@pytest.fixture(scope="module")
def fit_bound(fit_runs):
    """The yardstick: the larger of look-up against pair-count and row_merged = 0 against 2 (all with the products), over all fits."""
    look = max(fit_dist(r["lookup"], r["off"]) for r in fit_runs.values())
    unm = max(fit_dist(r["unmerged"], r["off"]) for r in fit_runs.values())
    print(f"\nfit yardstick: look-up vs pair-count {look:.3e}, row_merged 0 vs 2 {unm:.3e}")
    return max(look, unm)


@pytest.mark.parametrize("cid", list(FIT_BY_ID))
def test_fit_on_against_off_and_oracle(oracle, cid, fit_runs, fit_bound):
    """Tolerances against the oracle: test_gpu_stream_products.py::test_fit_with_three_tiles_per_wave."""
    c = FIT_BY_ID[cid]
    w = fit_data(c)
    r = fit_runs[cid]
    d = fit_dist(r["on"], r["off"])
    print(f"\n{cid}: on vs off {d:.3e}; look-up vs off {fit_dist(r['lookup'], r['off']):.3e}; unmerged vs off "
          f"{fit_dist(r['unmerged'], r['off']):.3e}; bound {fit_bound:.3e}")
    assert r["on"]["iters"] == r["off"]["iters"]
    if stacked_order(c):
        assert d == 0.0, (cid, d)
    else:
        assert d <= fit_bound, (cid, d, fit_bound)
    ref = oracle.optimize(w.X, w.levels, w.n_levels, w.A0, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, tuning=1,
                          max_iter=c["iters"] - 1, seed=4)
    got = r["on"]
    assert got["iters"] == ref["iters"]
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-8, equal_nan=True)
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-6
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-6, i


def same_fit(got, want):
    assert np.array_equal(got["column_factor"], want["column_factor"])
    for k in want["row_matrices"]:
        assert np.array_equal(got["row_matrices"][k], want["row_matrices"][k]), k
    assert np.array_equal(got["traj"], want["traj"], equal_nan=True)


def test_fit_on_a_clone_beside_its_source_by_bits(fit_runs):
    """The source and a clone fit at the same time from two threads, three times each; then the source again, alone: every
    result has the bits of the fit on a fresh handle (no dependence on what runs beside it or on the handle's history)."""
    c = FIT_BY_ID[[k for k in FIT_BY_ID if "K30" in k and "L17x3" in k and "it12-cold" in k][0]]
    w = fit_data(c)
    want = fit_runs[c["id"]]["on"]
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    for k, v in FIT_FORMS["on"].items():
        ds.set_option(k, v)
    twin = ds.clone()
    try:
        got = beside([lambda: run_fit(c, "on", ds), lambda: run_fit(c, "on", twin)], rounds=3)
        again = run_fit(c, "on", ds)
    finally:
        twin.close()
        ds.close()
    for runs in got.values():
        assert len(runs) == 3
        for r in runs:
            same_fit(r, want)
    same_fit(again, want)


TUNE_CASE = dict(n=96, p=140, level_counts=(17, 3), K=6, f=0.15, seed=31)


def tune_tables(concurrent):
    w = workloads.small(**TUNE_CASE)
    obj = api.Insider(data=w.X, confounder=w.levels, inc_continuous=0, ctns_confounder=None, train_indicator=w.M_train,
                      test_indicator=w.M_test, seed=13, params=dict(global_tol=1e-9, sub_tol=1e-5, tuning_iter=6, max_iter=50))
    ds = api._resident(obj, "tune")                        # (tune() fits on this handle and on clones of it: they copy its options)
    for k, v in FIT_FORMS["on"].items():
        ds.set_option(k, v)
    try:
        out = api.tune(obj, latent_dimension=np.array([4, 6]), lambda_=[1.0, 2.0, 4.0], alpha=[0.2, 0.5],
                       rng=np.random.default_rng(5), concurrent=concurrent)
        assert int(ds.info("col_stats_path")) == 2 and int(ds.info("row_merged")) == 1
        assert int(ds.info("col_stats_own_q")) == 1
        clones = obj.get("_tune_clones", [])
        assert len(clones) == concurrent - 1 and all(int(hd.info("col_stats_own_q")) == 1 for hd in clones)
    finally:
        for hd in obj.get("_tune_clones", []):
            hd.close()
        ds.close()
    return out


def test_tune_serial_and_two_at_a_time_by_bits():
    """tune(concurrent = 2) — two grid points at a time on one device, each on its own handle — against the serial tune()."""
    serial, conc = tune_tables(1), tune_tables(2)
    assert conc["latent_rank"] == serial["latent_rank"]
    np.testing.assert_array_equal(conc["rank_tuning"], serial["rank_tuning"])
    np.testing.assert_array_equal(conc["reg_tuning"], serial["reg_tuning"])
    assert np.all(np.isfinite(serial["reg_tuning"]))
