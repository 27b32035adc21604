"""bench.py --dump-outputs: what the timed call returned, as float64 .npy files within the 64 MB budget (CPU: the writer
alone, on arrays shaped like an optimize() result)."""
import os

import numpy as np

import bench


def _result(K, p, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return {"row_matrices": {"factor0": np.asfortranarray(rng.random((100, K))), "factor1": np.asfortranarray(rng.random((10, K)))},
            "column_factor": np.asfortranarray(rng.random((K, p))), "loss": 1.5, "train_rmse": 0.3, "test_rmse": 0.4,
            "traj": np.vstack([np.r_[-1.0, rng.random(7), np.nan, 1.0], rng.random((2, 10))]), "iters": 20}


def _bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_whole_result_written_as_float64(tmp_path):
    res = _result(30, 50000)
    d = str(tmp_path / "dump")
    files = bench.dump_outputs(d, res, 0, 50000, 0, 1)
    assert sorted(files) == ["column_factor", "factor0", "factor1", "loss", "test_rmse", "train_rmse", "traj"]
    for name in files:
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float64 and np.all(np.isfinite(a)), name
    # the row of the inits has no delta_loss (NaN in the library's trajectory): that column is left out, the rest kept
    assert np.array_equal(np.load(os.path.join(d, "traj.npy")), np.delete(res["traj"], 8, axis=1))
    assert np.array_equal(np.load(os.path.join(d, "column_factor.npy")), res["column_factor"])
    assert np.array_equal(np.load(os.path.join(d, "factor1.npy")), res["row_matrices"]["factor1"])
    assert np.load(os.path.join(d, "loss.npy"))[0] == res["loss"]
    assert _bytes(d) <= bench.DUMP_BUDGET_BYTES


def test_nothing_held_out_leaves_out_test_rmse(tmp_path):
    """tuning = 0: no held-out set, test_rmse is NaN by definition (scalar and trajectory column 2) and is not written."""
    res = _result(23, 5000)
    res["test_rmse"] = np.nan
    res["traj"][:, 2] = np.nan
    d = str(tmp_path / "dump")
    files = bench.dump_outputs(d, res, 0, 5000, 0, 1, tuning=0)
    assert "test_rmse" not in files
    for name in files:
        assert np.all(np.isfinite(np.load(os.path.join(d, name + ".npy")))), name
    assert np.array_equal(np.load(os.path.join(d, "traj.npy")), np.delete(res["traj"], [2, 8], axis=1))


def test_large_column_factor_is_a_fixed_sample_within_budget(tmp_path):
    res = _result(63, 200000)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, res, 0, 200000, 0, 1)
    bench.dump_outputs(d2, res, 0, 200000, 0, 1)
    assert _bytes(d1) <= bench.DUMP_BUDGET_BYTES
    genes = np.load(os.path.join(d1, "column_factor_genes.npy"))
    assert np.array_equal(genes, np.load(os.path.join(d2, "column_factor_genes.npy")))
    assert np.all(np.diff(genes) > 0) and genes[-1] < 200000
    assert np.array_equal(np.load(os.path.join(d1, "column_factor.npy")), res["column_factor"][:, genes.astype(np.int64)])


def test_ranks_write_their_slabs_of_the_same_sample(tmp_path):
    res = _result(63, 200000)
    one = str(tmp_path / "one")
    bench.dump_outputs(one, res, 0, 200000, 0, 1)
    two = str(tmp_path / "two")
    C = res["column_factor"]
    for rank, (lo, hi) in enumerate(((0, 100000), (100000, 200000))):
        bench.dump_outputs(two, dict(res, column_factor=np.asfortranarray(C[:, lo:hi])), lo, 200000, rank, 2)
    assert _bytes(two) <= bench.DUMP_BUDGET_BYTES
    genes = np.concatenate([np.load(os.path.join(two, f"column_factor_genes_rank{r}.npy")) for r in (0, 1)])
    cols = np.concatenate([np.load(os.path.join(two, f"column_factor_rank{r}.npy")) for r in (0, 1)], axis=1)
    assert np.array_equal(genes, np.load(os.path.join(one, "column_factor_genes.npy")))
    assert np.array_equal(cols, np.load(os.path.join(one, "column_factor.npy")))
