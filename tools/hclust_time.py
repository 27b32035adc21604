"""Measurement (GPU box): agglomerative clustering of a synthetic column factor on the device (insider_hip_hclust), its first
round next to a k = 1 neighbours call of the same shape, and the whole call next to the numpy yardstick and scipy on the host.

    python tools/hclust_time.py [--shapes 50000x30] [--reps 5] [--host-n 50000] [--scipy-n 20000] [--out FILE]

Points, per shape N x D: "random" = the seeded C0 of workloads.init_factors (D x N); "planted" = 12 standard-normal centres,
noise 0.3, labels drawn by a seeded generator.  Nothing is downloaded.  Per (shape, points, metric), in one process:
  A  after one warm-up call, --reps times api.hclust(points, metric): the wall time of the call and insider_hip_last_hclust_ms()
     (every kernel and the per-round records; the upload and the final download excluded), rounds and queries / N.
  B  --reps times in turn: the first round alone (max_rounds = 1: the call stops with ERR_UNFINISHED after its first round, all N
     clusters stale, and reports its kernels' time) against api.neighbors(points, k=1, metric="dot"):
     insider_hip_last_neighbors_ms() (k_nn_prep twice, k_nn_topk).  Medians, minima and all values.
  C  for N <= --host-n (0: never): posthoc.hclust_host(blas=True) on the host's threads, its wall time, and whether merges, sizes,
     rounds and queries equal the device's.
  D  on the first --scipy-n points (0: never): scipy.cluster.hierarchy.linkage, its wall time (the condensed matrix included)
     next to the device's on the same points.
Prints one JSON line per (shape, points, metric)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def points_of(kind, N, D):
    from insider_amd import workloads
    if kind == "random":
        return np.asfortranarray(workloads.init_factors((), D, N)[1])
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((D, 12))
    return np.asfortranarray(centres[:, rng.integers(0, 12, N)] + 0.3 * rng.standard_normal((D, N)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["50000x30"], help="N x D")
    ap.add_argument("--points", nargs="+", default=["random", "planted"], choices=("random", "planted"))
    ap.add_argument("--metrics", nargs="+", default=["cosine", "euclidean"], choices=("cosine", "euclidean"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=50000)
    ap.add_argument("--scipy-n", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from insider_amd import _lib, api, posthoc
    lib = _lib.load()
    lines = []
    for shape in a.shapes:
        N, D = (int(v) for v in shape.split("x"))
        for kind in a.points:
            P = points_of(kind, N, D)
            for metric in a.metrics:
                api.hclust(P, metric)                                             # warm-up: code object load
                api.neighbors(P, k=1, metric="dot")
                wall, ms, r1_ms, nn_ms = [], [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    run = api.hclust(P, metric)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(run["ms"])
                for _ in range(a.reps):
                    try:
                        api.hclust(P, metric, max_rounds=1)
                    except api.InsiderError as e:
                        assert e.status == _lib.ERR_UNFINISHED
                    r1_ms.append(float(lib.insider_hip_last_hclust_ms()))
                    api.neighbors(P, k=1, metric="dot")
                    nn_ms.append(float(lib.insider_hip_last_neighbors_ms()))
                rec = dict(N=N, D=D, points=kind, metric=metric, reps=a.reps, rounds=run["rounds"], queries=run["queries"],
                           queries_per_point=run["queries"] / N, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_all=ms,
                           wall_ms_median=float(np.median(wall)), wall_ms_all=wall,
                           round1_ms_median=float(np.median(r1_ms)), round1_ms_all=r1_ms,
                           neighbors_ms_median=float(np.median(nn_ms)), neighbors_ms_all=nn_ms,
                           round1_over_neighbors=float(np.median(r1_ms) / np.median(nn_ms)),
                           ms_per_query_pass=float(np.median(ms)) / (run["queries"] / N), source_sha=_lib.library_source_sha())
                if N <= a.host_n or a.scipy_n > 0:
                    print("device:", json.dumps(rec), flush=True)                 # (the host parts below take minutes)
                if 0 < N <= a.host_n:
                    ref = posthoc.hclust_host(P, metric, blas=True, chunk=1024)
                    rec.update(host_wall_ms=ref["ms"], host_over_device=ref["ms"] / float(np.median(wall)),
                               host_threads=os.environ.get("OMP_NUM_THREADS"), host_min_gap=ref["min_gap"],
                               same_tree=bool(np.array_equal(ref["merge"], run["merge"]) and np.array_equal(ref["size"], run["size"])),
                               same_counters=bool(ref["rounds"] == run["rounds"] and ref["queries"] == run["queries"]))
                if a.scipy_n > 0:
                    from scipy.cluster.hierarchy import linkage
                    n = min(N, a.scipy_n)
                    Q = np.asfortranarray(P[:, :n])
                    api.hclust(Q, metric)
                    t0 = time.perf_counter()
                    sub = api.hclust(Q, metric)
                    dev = (time.perf_counter() - t0) * 1e3
                    t0 = time.perf_counter()
                    Z = linkage(Q.T, method="average" if metric == "cosine" else "ward", metric=metric)
                    sp = (time.perf_counter() - t0) * 1e3
                    rec.update(scipy_n=n, scipy_wall_ms=sp, scipy_device_wall_ms=dev, scipy_over_device=sp / dev,
                               scipy_same_tree=bool(np.array_equal(np.sort(Z[:, :2].astype(np.int64), axis=1), sub["merge"])),
                               scipy_max_height_relerr=float(np.max(np.abs(Z[:, 2] - sub["height"]) / np.maximum(Z[:, 2], 1e-300))))
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
