"""tests/loss_reference.py checked on its own, without a GPU: it agrees with both oracles on benign data, an exact fit
evaluates to (almost) nothing, the float64 emulation of the device's identities stays within the derived bounds on every
cell the GPU tests use (so a GPU failure against them is the kernel's), and the hazard the clamp in k_loss_reduce answers
is on record: at sigma = 0 the identity's sum does come out negative."""
import numpy as np
import pytest

from oracle import numpy_oracle
from tests import loss_reference as lr


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("data,m", [("train_test", 0), ("na", 0), ("unmasked", 0), ("train_test", 2), ("na", 2)])
@pytest.mark.parametrize("K", [3, 17])
def test_agrees_with_both_oracles(oracle, data, m, K):
    lam1, lam2, alpha = 3.0, 2.0, 0.4
    d = lr.planted(K, 0.5, 0.0, data, seed=40 + K + m, n=90, p=33, level_counts=(9, 4), m=m)
    ref = lr.evaluate(d["X"], d["levels"], d["n_levels"], d["A"], d["C"], d["M_train"], d["M_test"], lam1, lam2, alpha,
                      d["tuning"], ctns=d["ctns"])
    R = lr.row_factor(d["levels"], d["A"], d["ctns"], dtype=np.float64)
    s, tr, te = numpy_oracle.evaluate(d["X"] - R @ d["C"], d["M_train"], d["M_test"], d["tuning"])
    loss, comps = numpy_oracle.compute_loss(d["A"], d["C"], lam1, lam2, alpha, s)
    row = oracle.optimize(d["X"], d["levels"], d["n_levels"], d["A"], d["C"], d["M_train"], d["M_test"], lam1, lam2, alpha,
                          tuning=d["tuning"], max_iter=0, seed=1, ctns=d["ctns"])["traj"][0]
    assert row[0] == -1
    want = [ref[k] for k in ("train_rmse", "test_rmse", "sse_half", "row_reg_half", "col_reg_half", "l1_reg", "loss")]
    for name, w, a, b in zip(("train_rmse", "test_rmse", "sse_half", "row_reg_half", "col_reg_half", "l1_reg", "loss"), want,
                             (tr, te, *comps, loss), row[1:8]):
        if name == "test_rmse" and d["tuning"] == 0:
            assert np.isnan(w) and np.isnan(b)          # (the reference's value is uninitialised there)
            continue
        assert np.isfinite(float(w))
        assert _rel(a, w) < 1e-12 and _rel(b, w) < 1e-12, (name, float(w), a, b)
    assert _rel(s, ref["sse_train"]) < 1e-12
    assert ref["cnt_train"] == (d["X"].size if d["tuning"] == 0 else np.count_nonzero(d["M_train"]))
    assert ref["cnt_test"] == (0 if d["tuning"] == 0 else np.count_nonzero(d["M_test"]))


def test_no_test_entry_is_nan():
    d = lr.planted(4, 0.5, 0.0, "train_test", seed=3, n=30, p=12, level_counts=(5, 3))
    d["M_train"][:], d["M_test"][:] = 1, 0
    ref = lr.evaluate(d["X"], d["levels"], d["n_levels"], d["A"], d["C"], d["M_train"], d["M_test"], 1.0, 1.0, 0.4, 1)
    assert ref["cnt_test"] == 0 and np.isnan(ref["test_rmse"]) and ref["sse_test"] == 0 and np.isfinite(ref["train_rmse"])


@pytest.mark.parametrize("offset", lr.EXACT_OFFSETS)
@pytest.mark.parametrize("K", lr.EXACT_KS)
def test_exact_fit_evaluates_to_rounding_of_the_data(K, offset):
    """X = fl(R C) in float64: an entry is within a few roundings of the exact product where its terms are of one size, far
    below the stated cap.  (Where long double is no wider than double the reference's own product carries K + 2 roundings
    more, and the cap is held to that.)"""
    for data in lr.DATA:
        d = lr.planted(K, 0.0, offset, data, seed=7)
        ref = lr.evaluate(d["X"], d["levels"], d["n_levels"], d["A"], d["C"], d["M_train"], d["M_test"], 1.0, 1.0, 0.4,
                          d["tuning"])
        cap = d["X"].size * (2.0 ** -52 * np.abs(d["X"]).max()) ** 2 * (1 if lr.EXTENDED else (K + 2) ** 2)
        assert 0 <= ref["sse_train"] < cap and 0 <= ref["sse_test"] < cap, (data, float(ref["sse_train"]), cap)


def _ratios(d):
    """|emulation - reference| / bound for the train sum and the test sum of one data set (test: None when there is none)."""
    args = (d["X"], d["levels"])
    ref = lr.evaluate(*args, d["n_levels"], d["A"], d["C"], d["M_train"], d["M_test"], 1.0, 1.0, 0.4, d["tuning"], ctns=d["ctns"])
    bnd = lr.bounds(*args, d["n_levels"], d["A"], d["C"], d["M_train"], d["M_test"], d["tuning"], ctns=d["ctns"])
    emu = lr.emulate_identity(*args, d["A"], d["C"], d["M_train"], d["M_test"], d["tuning"], ctns=d["ctns"])
    r_train = float(abs(emu["sse_train"] - ref["sse_train"]) / bnd["bound_stats"])
    r_unit = float(abs(emu["sse_train"] - ref["sse_train"]) / (2.0 ** -52 * bnd["scale"]))
    r_test = None
    if d["tuning"] == 1:
        b = bnd["bound_direct"] if lr.has_na(d["M_train"], d["M_test"]) else bnd["bound_stats"]
        r_test = float(abs(emu["sse_test"] - ref["sse_test"]) / b) if b > 0 else 0.0
        assert b > 0 or emu["sse_test"] == ref["sse_test"] == 0
    return r_train, r_test, r_unit, emu


_worst = {"train": 0.0, "test_stats": 0.0, "test_direct": 0.0, "unit": 0.0}


def _record(d, data):
    r_train, r_test, r_unit, emu = _ratios(d)
    _worst["train"] = max(_worst["train"], r_train)
    _worst["unit"] = max(_worst["unit"], r_unit)
    if r_test is not None:
        key = "test_direct" if data == "na" else "test_stats"
        _worst[key] = max(_worst[key], r_test)
    assert r_train <= 1 and (r_test is None or r_test <= 1), (data, r_train, r_test)
    return emu


@pytest.mark.parametrize("K", lr.KS)
def test_emulation_within_bounds_on_the_evaluator_grid(K):
    for cond in lr.CONDITIONS:
        for data in lr.DATA:
            for held in (True, False):
                _record(lr.planted(K, *cond, data, lr.case_seed(K, cond), held_gene=held), data)


@pytest.mark.parametrize("K", lr.EXACT_KS)
def test_emulation_within_bounds_on_the_exact_fit_grid(K):
    for offset in lr.EXACT_OFFSETS:
        for seed in lr.EXACT_SEEDS:
            for data in lr.DATA:
                _record(lr.planted(K, 0.0, offset, data, seed, held_gene=False), data)


def test_emulation_within_bounds_on_the_list_shape_and_continuous_cells():
    for K in lr.LIST_KS:
        for cond in lr.LIST_CONDITIONS:
            for masks in lr.LIST_MASKS:
                _record(lr.list_case(K, cond, masks), "train_test" if masks == "all_train" else "na")
    for p in lr.SHAPE_PS:
        for n in lr.SHAPE_LEVELS:
            for data in lr.SHAPE_DATA:
                for cond in lr.SHAPE_CONDITIONS:
                    _record(lr.shape_case(p, n, data, cond), data)
    for K in lr.CTNS_KS:
        for cond in lr.CTNS_CONDITIONS:
            for data in lr.CTNS_DATA:
                _record(lr.ctns_case(K, cond, data), data)


def test_the_identity_goes_negative_at_sigma_zero():
    """The hazard on record: on noiseless data the float64 identity's train sum is negative for some of the eight seeds
    (which ones is luck of the summation order), where the direct sum is a tiny positive number."""
    neg, genes = [], []
    for seed in lr.EXACT_SEEDS:
        d = lr.planted(9, 0.0, 0.0, "train_test", seed, held_gene=False)
        emu = lr.emulate_identity(d["X"], d["levels"], d["A"], d["C"], d["M_train"], d["M_test"], 1)
        neg.append(emu["sse_train"] < 0)
        genes.append(emu["negative"])
    print(f"sigma = 0, K = 9: emulated train sum negative for seeds {[s for s, f in zip(lr.EXACT_SEEDS, neg) if f]}, "
          f"genes with a negative value per seed {genes}")
    assert any(neg), genes
    assert all(g > 0 for g in genes)


def test_zz_report_ratios():
    print("loss-reference emulation error / bound, largest: " + ", ".join(f"{k} {v:.2e}" for k, v in _worst.items())
          + "  (unit = error / (2^-52 scale))")
    assert max(v for k, v in _worst.items() if k != "unit") <= 1
