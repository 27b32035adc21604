"""K-fold cross-validated tune(): the host side (no GPU) — fold_splitter, the pooled RMSE, the exported symbols and the
order in which tune(folds=True) draws its inits."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from insider_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("insider_hip_remask", "insider_hip_set_folds", "insider_hip_remask_fold")


def _data(n=37, p=23, seed=3, na=0.08):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, p))
    d[rng.random((n, p)) < na] = np.nan
    return d


@pytest.mark.parametrize("F", [2, 3, 5, 7])
def test_fold_splitter_deals_every_entry_to_exactly_one_fold(F):
    d = _data()
    s = api.fold_splitter(d, folds=F, rm_na_col=False, seed=11)
    ids, na = s["fold_id"], np.isnan(d)
    assert ids.shape == d.shape and ids.dtype == np.uint8
    assert np.array_equal(s["na_indicator"], na) and s["kept_columns"].all()
    assert (ids[na] == 0).all()                                   # NA entries: fold 0 ...
    assert ((ids[~na] >= 1) & (ids[~na] <= F)).all()              # ... every other entry in exactly one of 1..F
    sizes = np.array([(ids == f).sum() for f in range(1, F + 1)])
    assert sizes.sum() == (~na).sum() and sizes.max() - sizes.min() <= 1
    assert np.array_equal(s["data"], np.where(na, 0.0, d))        # NA -> 0
    assert np.array_equal(api.fold_splitter(d, folds=F, rm_na_col=False, seed=11)["fold_id"], ids)   # same seed, same ids
    assert not np.array_equal(api.fold_splitter(d, folds=F, rm_na_col=False, seed=12)["fold_id"], ids)


def test_fold_splitter_keeps_a_column_whose_nonzeros_lie_in_two_folds():
    """The reference drops a column whose train set is all zero (R/utils.R:102-109).  The train set of fold f is every
    other fold: it is non-zero for every f exactly when the column's non-zero entries lie in at least two folds."""
    n, F = 30, 3
    d = np.zeros((n, 6))
    d[:, 0] = 1.0                       # dense: kept
    d[4, 1] = 2.0                       # one non-zero entry: it lies in one fold, whose train set is all zero -> dropped
    d[:, 2] = np.nan                    # all NA -> dropped
    d[[3, 17], 3] = 5.0                 # two non-zero entries: kept only if they fall in different folds
    d[[1, 2, 9, 20], 4] = -1.0
    d[:, 5] = 0.0                       # all zero -> dropped
    full = api.fold_splitter(d, folds=F, rm_na_col=False, seed=5)["fold_id"]
    s = api.fold_splitter(d, folds=F, seed=5)
    want = np.array([len(set(full[d[:, j] != 0, j]) - {0}) >= 2 if not np.isnan(d[:, j]).all() else False
                     for j in range(d.shape[1])])
    assert np.array_equal(s["kept_columns"], want)
    assert list(want[[0, 1, 2, 5]]) == [True, False, False, False]
    assert s["fold_id"].shape == (n, int(want.sum())) and np.array_equal(s["fold_id"], full[:, want])
    # the rule, fold by fold: every kept column has a non-zero train entry in every fold
    for f in range(1, F + 1):
        train = (s["fold_id"] != f) & (s["fold_id"] != 0)
        assert ((s["data"] != 0) & train).any(axis=0).all()


def test_fold_rule_drops_a_column_with_all_nonzeros_in_one_fold():
    n, F = 12, 3
    d = np.ones((n, 2))
    ids = api.fold_splitter(d, folds=F, rm_na_col=False, seed=1)["fold_id"]
    d[:, 1] = 0.0
    d[ids[:, 1] == 2, 1] = 3.0          # column 1: non-zero only where its entries are in fold 2
    s = api.fold_splitter(d, folds=F, seed=1)
    assert list(s["kept_columns"]) == [True, False]


def test_pooled_rmse_is_the_rmse_over_all_held_out_entries():
    rng = np.random.default_rng(2)
    n, p, F = 14, 9, 4
    truth, pred = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    ids = api.fold_splitter(truth, folds=F, rm_na_col=False, seed=8)["fold_id"]
    rm = np.array([np.sqrt(np.mean((truth - pred)[ids == f] ** 2)) for f in range(1, F + 1)])
    n_f = np.array([(ids == f).sum() for f in range(1, F + 1)])
    assert len(set(n_f)) > 1            # unequal folds: the weights matter
    direct = np.sqrt(np.mean((truth - pred) ** 2))
    assert api.pooled_rmse(rm, n_f) == pytest.approx(direct, rel=1e-14)
    assert api.pooled_rmse(np.stack([rm, 2 * rm]), n_f) == pytest.approx([direct, 2 * direct], rel=1e-14)


def test_new_symbols_are_declared_and_exported():
    ge.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "insider_hip.h")).read()
    declared = set(re.findall(r"\b(insider_hip_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SYMBOLS, s
        assert getattr(lib, s) is not None
    for key in ("data_bytes_shared", "data_bytes_own"):
        assert f'"{key}"' in hdr


class _StubData:
    """Stands in for InsiderData: records the calls tune(folds=True) makes, returns RMSEs that depend on (fold, inits)."""

    def __init__(self, log, fold=0):
        self.log, self.fold_no, self._h = log, fold, True

    def set_folds(self, ids, F):
        self.log.append(("set_folds", int(F)))

    def fold(self, f):
        self.log.append(("fold", f))
        return _StubData(self.log, f)

    def clone(self):
        self.log.append(("clone", self.fold_no))
        return _StubData(self.log, self.fold_no)

    def profile(self):
        return dict(wall_ms=0.0)

    def optimize(self, cfd, col, K, l1, l2, a, tuning, gt, st, iters, seed=None, inc_continuous=0, copy=True):
        key = float(sum(np.abs(x).sum() for x in cfd) + np.abs(col).sum())
        self.log.append(("fit", self.fold_no, K, l1, a, key))
        for x in cfd:                   # a fit updates its arguments in place: the next fold must not see that
            x += 1.0
        col += 1.0
        return dict(train_rmse=key + self.fold_no, test_rmse=key * (1 + self.fold_no) + l1 + a, row_matrices={},
                    column_factor=col)


def _obj(folds=3):
    rng = np.random.default_rng(1)
    conf = np.column_stack([np.arange(40) % 4 + 1, np.arange(40) % 3 + 1])
    data = rng.standard_normal((40, 30))
    data[rng.random(data.shape) < 0.05] = np.nan
    return api.insider(data, conf, tuning_iter=3, seed=5, folds=folds)


def test_insider_with_folds_carries_fold_ids_over_the_kept_columns():
    obj, plain = _obj(4), _obj(None)
    assert "fold_id" not in plain
    assert obj["fold_id"].shape == obj["data"].shape == obj["train_indicator"].shape
    assert np.array_equal(obj["fold_id"] == 0, obj["na_indicator"] != 0)
    assert set(np.unique(obj["fold_id"])) == {0, 1, 2, 3, 4}


def test_tune_with_folds_and_warm_start_raises():
    obj = _obj()
    with pytest.raises(ValueError):
        api.tune(obj, latent_dimension=np.array([3, 4]), folds=True, warm_start=True)
    with pytest.raises(ValueError):
        api.tune(_obj(None), latent_dimension=np.array([3, 4]), folds=True)      # no fold ids on the object


@pytest.mark.parametrize("concurrent", [1, 3])
def test_tune_with_folds_draws_inits_once_per_point(monkeypatch, tmp_path, concurrent):
    obj, F = _obj(3), 3
    log = []
    stub = _StubData(log)
    monkeypatch.setattr(api, "_resident", lambda o, which: stub)
    lat, lam, alp = np.array([3, 5]), [1.0, 2.0], [0.1, 0.3]
    rng = np.random.default_rng(42)
    out = api.tune(obj, latent_dimension=lat, lambda_=lam, alpha=alp, rng=rng, folds=True, concurrent=concurrent,
                   out_dir=str(tmp_path))
    # the same generator after the same calls without folds: the stub's single fit per point draws nothing either
    ref_rng = np.random.default_rng(42)
    ref_log = []
    monkeypatch.setattr(api, "_resident", lambda o, which: _StubData(ref_log))
    api.tune(_obj(3), latent_dimension=lat, lambda_=lam, alpha=alp, rng=ref_rng)
    assert rng.bit_generator.state == ref_rng.bit_generator.state
    # every point: F fits, one per fold, all from THE SAME inits (equal keys), which are the no-fold run's inits
    fits = [e for e in log if e[0] == "fit"]
    ref_fits = [e for e in ref_log if e[0] == "fit"]
    assert len(fits) == F * len(ref_fits) == F * (2 + 4)
    by_point = {}
    for _, f, K, l1, a, key in fits:
        by_point.setdefault((K, l1, a, key), []).append(f)
    assert len(by_point) == len(ref_fits)
    for (_, _, K, l1, a, key) in ref_fits:
        assert sorted(by_point[(K, l1, a, key)]) == [1, 2, 3]
    assert [e for e in log if e[0] == "fold"] == [("fold", 1), ("fold", 2), ("fold", 3)]       # derived once
    # tables: columns as without folds; train = mean, test = pooled over the fold sizes; per-fold table and its spread
    n_f = np.array([(obj["fold_id"] == f).sum() for f in (1, 2, 3)])
    assert out["rank_tuning"].shape == (2, 3) and out["reg_tuning"].shape == (4, 4)
    assert out["rank_tuning_folds"].shape == (2, F) and out["reg_tuning_folds"].shape == (4, F)
    np.testing.assert_array_equal(out["reg_tuning"][:, 3], api.pooled_rmse(out["reg_tuning_folds"], n_f))
    np.testing.assert_array_equal(out["reg_tuning_test_sd"], out["reg_tuning_folds"].std(axis=1, ddof=1))
    assert [tuple(r[:2]) for r in out["reg_tuning"]] == [(1.0, 0.1), (2.0, 0.1), (1.0, 0.3), (2.0, 0.3)]
    K = out["latent_rank"]
    assert np.loadtxt(tmp_path / f"insider_R{K}_reg_tuning_result.csv", delimiter=",").shape == (4, 4)
    assert np.loadtxt(tmp_path / f"insider_R{K}_reg_tuning_result_folds.csv", delimiter=",").shape == (4, 2 + F)
    assert np.loadtxt(tmp_path / "insider_rank_tuning_result_folds.csv", delimiter=",").shape == (2, 1 + F)
    # a second call reuses the fold handles
    n_fold_calls = len([e for e in log if e[0] == "fold"])
    monkeypatch.setattr(api, "_resident", lambda o, which: stub)
    again = api.tune(obj, latent_dimension=lat, lambda_=lam, alpha=alp, rng=np.random.default_rng(42), folds=True)
    assert len([e for e in log if e[0] == "fold"]) == n_fold_calls
    np.testing.assert_array_equal(again["reg_tuning"], out["reg_tuning"])
    np.testing.assert_array_equal(again["rank_tuning_folds"], out["rank_tuning_folds"])
