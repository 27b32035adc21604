"""The gene-sharded HIP path with TWO processes on ONE GPU: each rank holds a gene slab on cuda:0,
the per-level normal equations and the loss terms cross ranks between kernels through the all-reduce callback of the
C ABI — here a host-staged gloo all-reduce (RCCL refuses two ranks on one device; on a multi-GPU node the same callback
slot carries the stream-ordered RCCL all-reduce of insider_amd/dist.py).  The sharded fit must reproduce the
single-process fit: row factors, the gathered gene factors and the loss trajectory, to summation-order tolerance.
"""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from insider_amd import workloads

pytestmark = pytest.mark.gpu

CASE = dict(n=120, p=150, level_counts=(7, 4), K=9, f=0.15, seed=23, with_na=True)
ITERS = 12


def _fit(rank, world, staged, opts=None, device=0, mode=None):
    from insider_amd import api, dist as idist
    w = workloads.small(**CASE)
    lo, hi = idist.shard_range(w.p, rank, world)
    ds = api.InsiderData(w.X[:, lo:hi], w.levels, w.M_train[:, lo:hi], w.M_test[:, lo:hi], device=device)
    opts = dict(opts or {})
    tuning = int(opts.pop("tuning", 1))      # (not a library option: the fit's own argument)
    for k, v in opts.items():
        ds.set_option(k, v)
    ar = idist.attach(ds, lo, rank, world, device=device, staged=staged, mode=mode)
    A = [a.copy(order="F") for a in w.A0]
    C = w.C0[:, lo:hi].copy(order="F")
    res = ds.optimize(A, C, w.K, w.lam, w.lam, w.alpha, tuning=tuning, max_iter=ITERS, global_tol=-1.0, seed=5)
    ds.close()
    return dict(A=[np.array(a) for a in res["row_matrices"].values()], C=res["column_factor"], traj=res["traj"],
                loss=res["loss"], test_rmse=res["test_rmse"], lo=lo, hi=hi,
                calls=len(ar.calls) if hasattr(ar, "calls") else 0)


def _worker(rank, world, port, q, opts):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _fit(rank, world, staged=True, opts=opts)))
    except Exception as e:   # surface the failure in the parent instead of a hang
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("opts", [dict(row_merged=2, col_factored=2, row_counts=0), dict(row_merged=2, col_factored=3), dict(row_merged=0, col_factored=0),
                                  dict(tuning=0), dict(tuning=0, row_fused=0)],
                         ids=["merged-factored", "merged-paircount", "per-entry", "unmasked", "unmasked-per-sample"])
def test_two_ranks_on_one_gpu_match_single_rank(opts):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, opts)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in (0, 1):
        assert isinstance(out[r], dict), out[r]
    single = _fit(0, 1, staged=False, opts=opts)

    # one all-reduce per covariate per outer iteration + one per loss checkpoint (initial fit, iterations 0 and 10)
    n_cov = len(CASE["level_counts"])
    assert out[0]["calls"] == out[1]["calls"] == n_cov * (ITERS + 1) + 3

    def relerr(a, b):
        return np.linalg.norm(a - b) / np.linalg.norm(b)

    for i in range(n_cov):                                   # row factors: replicated, bit-identical across ranks
        assert np.array_equal(out[0]["A"][i], out[1]["A"][i])
        assert relerr(out[0]["A"][i], single["A"][i]) < 1e-9
    C = np.concatenate([out[0]["C"], out[1]["C"]], axis=1)    # gene factors: gathered slabs
    assert out[0]["hi"] == out[1]["lo"] and C.shape == single["C"].shape
    assert relerr(C, single["C"]) < 1e-9
    assert np.allclose(out[0]["traj"], out[1]["traj"], rtol=0, atol=0, equal_nan=True)
    np.testing.assert_allclose(out[0]["traj"][:, 1:8], single["traj"][:, 1:8], rtol=1e-10, equal_nan=True)
    assert out[0]["loss"] == pytest.approx(single["loss"], rel=1e-11)
    if opts.get("tuning", 1) == 1:           # (tuning = 0 has no test RMSE: NaN, src/optimize.cpp:264)
        assert out[0]["test_rmse"] == pytest.approx(single["test_rmse"], rel=1e-11)


# ---- two ranks on TWO GPUs: the real exchange (needs a multi-GPU node; skipped on the one-GPU test box) ---------------
def _worker_2gpu(rank, world, port, q, mode):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        q.put((rank, _fit(rank, world, staged=False, device=rank, mode=mode)))
    except Exception as e:
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.multi_gpu
@pytest.mark.parametrize("mode", ["rccl", "torch"])
def test_two_ranks_on_two_gpus_rccl(mode):
    """One rank per GPU, backend nccl (= RCCL over xGMI): "rccl" = the library's own communicator and ncclAllReduce on its
    stream (insider_hip_comm_init), "torch" = the stream-ordered torch.distributed callback (dist.DeviceAllreduce)."""
    from insider_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("needs two GPUs (the driver's 8-GPU node; the -m gpu box has one)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_2gpu, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in (0, 1):
        assert isinstance(out[r], dict), out[r]
    single = _fit(0, 1, staged=False)
    for i in range(len(CASE["level_counts"])):
        assert np.array_equal(out[0]["A"][i], out[1]["A"][i])
        assert np.linalg.norm(out[0]["A"][i] - single["A"][i]) / np.linalg.norm(single["A"][i]) < 1e-9
    C = np.concatenate([out[0]["C"], out[1]["C"]], axis=1)
    assert np.linalg.norm(C - single["C"]) / np.linalg.norm(single["C"]) < 1e-9
    np.testing.assert_allclose(out[0]["traj"][:, 1:8], single["traj"][:, 1:8], rtol=1e-10)


def test_bench_two_rank_rehearsal_on_one_gpu():
    """bench.py's N > 1 path end to end from a PLAIN invocation (`python bench.py --gpus 2`: the script starts its ranks
    itself as a torch.distributed.run child process before touching the GPU; gene sharding, max-over-ranks timing, rank
    0's JSON line) with two ranks time-sharing the one GPU (INSIDER_BENCH_ONE_GPU=1: host-staged all-reduce; the timing is
    then not a scaling figure).  The sharded problem's loss must equal the single-process run's."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "c2", "--steps", "6", "--warmup", "1", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["INSIDER_BENCH_ONE_GPU"] = "1"
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", *common],
                        cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stderr[-3000:]
    two = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *common], cwd=root, capture_output=True, text=True,
                        timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][-1])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["steps"] == 6 and two["config"]["genes_per_gpu"] == 10000
    assert "2000 x 20000" in two["metric"] and two["unit"] == "outer-iterations/s" and two["value"] > 0
    assert two["loss"] == pytest.approx(one["loss"], rel=1e-10) and two["test_rmse"] == pytest.approx(one["test_rmse"], rel=1e-10)
    for key in ("roofline", "masked_gram", "cd_kernel"):
        assert key in two and two["roofline"]["frac"] <= 1.0


def test_bench_exchange_vote_rehearsal_one_rank_cannot_join():
    """`bench.py --gpus 2` with the in-library RCCL exchange ATTEMPTED (INSIDER_BENCH_REHEARSE_VOTE=1) and rank 1 made to fail
    before the join (INSIDER_FAIL_COMM_RANK=1): every rank must take the fall-back exchange TOGETHER — nobody enters the
    blocking ncclCommInitRank — and the job finishes with the single-process loss.  (Two ranks on the one GPU: the fall-back
    there is the host-staged exchange; on a multi-GPU node it is the torch.distributed callback, same vote.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "c2", "--steps", "4", "--warmup", "1", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(INSIDER_BENCH_ONE_GPU="1", INSIDER_BENCH_REHEARSE_VOTE="1", INSIDER_FAIL_COMM_RANK="1")
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", *common],
                        cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stderr[-3000:]
    two = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    vote = two["config"]["exchange_vote"]
    assert vote["attempted"] == "rccl" and vote["ready_min"] == 0 and vote["joined_min"] is None and vote["path"] == "staged", vote
    assert "StagedHostAllreduce" in two["config"]["parallelism"]
    assert "fall back to the staged exchange together" in r2.stderr and "injected failure on rank 1" in r2.stderr
    env1 = {k: v for k, v in env.items() if not k.startswith("INSIDER_")}
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *common], cwd=root, env=env1, capture_output=True, text=True,
                        timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][-1])
    assert two["loss"] == pytest.approx(one["loss"], rel=1e-10)


@pytest.mark.multi_gpu
@pytest.mark.parametrize("fail_rank", [None, 1])
def test_bench_gpus_2_rccl_on_two_gpus(fail_rank):
    """`python bench.py --gpus 2` as the driver launches it on a multi-GPU node: the in-library RCCL exchange (both votes 1,
    exchange "rccl"), and with one rank kept from joining, the torch.distributed callback on both ranks; the sharded
    problem's loss equals the single-GPU run's either way."""
    from insider_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("needs two GPUs (the driver's multi-GPU node)")
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "c2", "--steps", "4", "--warmup", "1", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK") and not k.startswith("INSIDER_")}
    if fail_rank is not None:
        env["INSIDER_FAIL_COMM_RANK"] = str(fail_rank)
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", *common], cwd=root, env=env,
                        capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stderr[-3000:]
    two = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    vote = two["config"]["exchange_vote"]
    if fail_rank is None:
        assert vote["ready_min"] == 1 and vote["joined_min"] == 1 and vote["path"] == "rccl", vote
        assert "exchange: rccl" in two["config"]["parallelism"]
    else:
        assert vote["ready_min"] == 0 and vote["path"] == "torch" and "DeviceAllreduce" in two["config"]["parallelism"], vote
    env.pop("INSIDER_FAIL_COMM_RANK", None)
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *common], cwd=root, env=env, capture_output=True, text=True,
                        timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][-1])
    assert two["n_gpus"] == 2 and two["loss"] == pytest.approx(one["loss"], rel=1e-10)


def test_bench_grid_parallel_rehearsal_on_one_gpu():
    """`bench.py --gpus 2 --grid`: config 3's 40 grid points dealt over the ranks (every rank keeps the whole c3 data set
    resident, api.tune(rank, world), one all-reduce of the result table), reported as the `grid_parallel` block next to the
    unchanged strong-scaling line.  Rehearsed with two ranks on the one GPU (gloo): the table equals the one-process grid's."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["INSIDER_BENCH_ONE_GPU"] = "1"
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--grid", "--workload", "c2", "--steps", "4",
                         "--warmup", "1", "--no-cpu-baseline"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stderr[-3000:]
    two = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    gp = two["grid_parallel"]
    assert "failed" not in gp, gp
    assert gp["points"] == 40 and gp["points_per_rank"] == 20 and gp["table_complete"] and gp["mean_outer_iterations_per_s"] > 0
    assert two["n_gpus"] == 2 and "2000 x 20000" in two["metric"]          # the strong-scaling line itself is unchanged
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--grid", "--steps", "4", "--warmup", "1", "--no-cpu-baseline"],
                        cwd=root, capture_output=True, text=True, timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][-1])
    np.testing.assert_array_equal(np.array(gp["table"]), np.array(one["grid"]["table"]))


# ---- grid-parallel tune() on real handles: every rank keeps the WHOLE data set resident on the GPU and
# fits the grid points g % world == rank; the result tables are summed over torch.distributed -----------------------------
TUNE_CASE = dict(n=96, p=140, level_counts=(6, 4), K=6, f=0.15, seed=31)


def _tune_real(rank, world, warm_start=False, concurrent=1):
    from insider_amd import api
    w = workloads.small(**TUNE_CASE)
    obj = api.Insider(data=w.X, confounder=w.levels, inc_continuous=0, ctns_confounder=None, train_indicator=w.M_train,
                      test_indicator=w.M_test, seed=13,
                      params=dict(global_tol=1e-9, sub_tol=1e-5, tuning_iter=6, max_iter=50))
    out = api.tune(obj, latent_dimension=np.array([4, 6]), lambda_=[1.0, 2.0, 4.0], alpha=[0.2, 0.5],
                   rng=np.random.default_rng(5), rank=rank, world=world, warm_start=warm_start, concurrent=concurrent)
    for hd in obj.get("_tune_clones", []):
        hd.close()
    obj["_resident_tune"].close()
    return out


def _tune_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = _tune_real(rank, world)
        q.put((rank, dict(rank_tuning=out["rank_tuning"], latent_rank=out["latent_rank"], reg_tuning=out["reg_tuning"])))
    except Exception as e:
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_grid_parallel_tune_on_real_handles_matches_serial():
    """Two processes, each with its own resident InsiderData on the one GPU, split tune()'s rank sweep and lambda x alpha
    grid between them (gloo sum of the tables): both end with exactly the serial run's tables, because every rank draws
    every point's fresh inits in the reference's order and each fit is an independent, deterministic call."""
    serial = _tune_real(0, 1)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tune_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in (0, 1):
        assert isinstance(out[r], dict), out[r]
        assert out[r]["latent_rank"] == serial["latent_rank"]
        np.testing.assert_array_equal(out[r]["rank_tuning"], serial["rank_tuning"])
        np.testing.assert_array_equal(out[r]["reg_tuning"], serial["reg_tuning"])
    assert serial["reg_tuning"].shape == (6, 4) and np.all(np.isfinite(serial["reg_tuning"]))


def test_tune_warm_start_is_opt_in_and_close_to_cold():
    """warm_start=True starts each grid point from its nearest finished neighbour: the first point is identical to the cold
    run (it has no neighbour), the others are further along (lower train RMSE) within the same iteration budget, and the
    default stays the reference's fresh inits."""
    cold = _tune_real(0, 1)
    cold2 = _tune_real(0, 1)
    warm = _tune_real(0, 1, warm_start=True)
    np.testing.assert_array_equal(cold["reg_tuning"], cold2["reg_tuning"])              # default path: deterministic
    np.testing.assert_array_equal(warm["rank_tuning"], cold["rank_tuning"])            # the rank sweep is not warm-started
    np.testing.assert_array_equal(warm["reg_tuning"][0], cold["reg_tuning"][0])
    assert not np.array_equal(warm["reg_tuning"][1:], cold["reg_tuning"][1:])
    # within the same iteration budget a warm-started point is further along than a cold one: lower train RMSE
    assert np.all(warm["reg_tuning"][1:, 2] < cold["reg_tuning"][1:, 2]) and np.all(np.isfinite(warm["reg_tuning"]))


# ---- several fits of one resident data set at the same time (insider_hip_clone) ----------------------
def test_concurrent_tune_is_bit_identical():
    """tune(concurrent=3): three grid points at a time on the one GPU, each on its own handle of the shared data set, from
    three host threads.  The tables equal the serial grid's to the last bit: the inits are drawn by one generator in the
    reference's order and a fit does not depend on the handle that runs it or on what runs beside it."""
    serial = _tune_real(0, 1)
    conc = _tune_real(0, 1, concurrent=3)
    np.testing.assert_array_equal(conc["rank_tuning"], serial["rank_tuning"])
    np.testing.assert_array_equal(conc["reg_tuning"], serial["reg_tuning"])
    with pytest.raises(ValueError):
        _tune_real(0, 1, warm_start=True, concurrent=2)


def test_clones_share_the_data_set_and_outlive_their_source():
    """insider_hip_clone: same resident device arrays, private workspace.  Four threads fit four different (lambda, K)
    points at once on the source and three clones; each result is bit-identical to the same fit run alone, and a clone keeps
    working after its source handle has been destroyed (the data set goes with the LAST handle)."""
    import threading
    from insider_amd import api
    w = workloads.small(n=150, p=400, level_counts=(7, 5), K=12, f=0.12, seed=77, with_na=True)
    points = [(1.0, 12), (3.0, 12), (5.0, 9), (2.0, 17)]

    def inits(K, seed):
        rs = np.random.default_rng(seed)
        A = [np.asfortranarray(rs.standard_normal((int(L), K)) * 1e-3) for L in w.n_levels]
        return A, np.asfortranarray(rs.standard_normal((K, w.p)) * 1e-3)

    def fit(hd, lam, K):
        A, C = inits(K, K)
        return hd.optimize(A, C, K, lam, lam, 0.4, tuning=1, max_iter=12, seed=3)

    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    alone = [fit(ds, lam, K) for lam, K in points]
    handles = [ds] + [ds.clone() for _ in range(3)]
    out, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):          # repeated: the fits overlap in different phases
                out[i] = fit(handles[i], *points[i])
        except Exception as e:
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for got, ref in zip(out, alone):
        assert np.array_equal(got["column_factor"], ref["column_factor"]) and got["loss"] == ref["loss"]
        for k in ref["row_matrices"]:
            assert np.array_equal(got["row_matrices"][k], ref["row_matrices"][k])
        assert np.array_equal(got["traj"], ref["traj"], equal_nan=True)
    ds.close()                          # the source goes first
    again = fit(handles[1], *points[0])
    assert np.array_equal(again["column_factor"], alone[0]["column_factor"])
    for hd in handles[1:]:
        hd.close()


def test_clones_leak_no_device_memory_and_start_without_diagnostics():
    """Handles of one data set own their memory by type: four rounds of create, two clones, fits at K = 8 and K = 20 on
    every handle (the workspace is rebuilt), residual, interaction GLM and variance decomposition on a clone, then the
    source destroyed first and the clones after it.  The data set is n = 2000 x p = 6000 (X alone is 96 MB on the device,
    the workspace at K = 20 over 40 MB): free device memory (hipMemGetInfo) after the last round must be within 32 MB of
    the figure after the first round, where one leaked data set or workspace per round would have cost 120 MB or more by then.  A new
    clone reports zero for the diagnostics of the last call ("col_solver", "col_eval", "col_ridge_fallback", "row_kernels",
    "vd_path") while its source reports its own."""
    import ctypes
    from insider_amd import api
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    w = workloads.small(n=2000, p=6000, level_counts=(12, 5), K=8, f=0.1, seed=31, with_na=True)
    keys = ("col_solver", "col_eval", "col_ridge_fallback", "row_kernels", "vd_path")
    rng = np.random.default_rng(5)
    inits = {K: ([np.asfortranarray(rng.standard_normal((int(L), K)) * 1e-2) for L in w.n_levels],
                 np.asfortranarray(rng.standard_normal((K, w.p)) * 1e-2)) for K in (8, 20)}

    def fit(hd, K):
        A, C = inits[K]
        return hd.optimize([a.copy(order="F") for a in A], C.copy(order="F"), K, 2.0, 2.0, 0.4, tuning=1, max_iter=3,
                           global_tol=-1.0, seed=3)

    free = []
    for _ in range(4):
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        fit(ds, 8)
        ds.variance_decomposition(list(fit(ds, 20)["row_matrices"].values()), inits[20][1])
        assert ds.info("col_solver") != 0 and ds.info("row_kernels") != 0 and ds.info("vd_path") != 0
        clones = [ds.clone(), ds.clone()]
        for cl in clones:
            assert [cl.info(k) for k in keys] == [0.0] * len(keys)
        for hd in [ds] + clones:
            fit(hd, 8)
            r = fit(hd, 20)
        A = list(r["row_matrices"].values())
        cl = clones[0]
        assert cl.residual(A, r["column_factor"]).shape == (w.n, w.p)
        cl.interaction_glm(A, r["column_factor"], w.levels[:, 1], subtract=[1, 0])
        cl.variance_decomposition(A, r["column_factor"])
        ds.close()
        for cl in clones:
            cl.close()
        free.append(free_bytes())
    assert abs(free[-1] - free[0]) < (32 << 20), free
