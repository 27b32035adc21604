"""Measurement (GPU box): k-means of a synthetic column factor on the device (insider_hip_kmeans), its assignment step next to
the parent's only way to do one (api.neighbors with k = 1), and the whole call next to the numpy yardstick on the host.

    python tools/kmeans_time.py [--shapes 50000x30x200 200000x30x500] [--reps 5] [--max-iter 100] [--host-shapes 1] [--out FILE]

Points: the seeded C0 of workloads.init_factors (D x N), 30 % of its columns set to zero as an elastic-net fit leaves them
(dead under cosine); init: k alive columns by a seeded choice.  Nothing is downloaded.  Per shape, after one warm-up call of each
kind, --reps times in turn in one process:
  A  api.kmeans(C, k, init=init, restarts=1, max_iter=0): insider_hip_last_kmeans_ms() (k_nn_prep, k_km_points, k_km_cprep,
     k_km_assign, k_km_reduce and the size count), against api.neighbors(C, init, k=1, metric="dot"):
     insider_hip_last_neighbors_ms() (k_nn_prep twice, k_nn_topk).  Medians, minima and all values.
  then once the whole run, max_iter = --max-iter: iters, converged and ms per Lloyd iteration = last_kmeans_ms / (iters + 1).
  B  for the first --host-shapes shapes: the wall time of that api.kmeans call against the wall time of
     posthoc.kmeans_host(blas=True) with the same arguments on the host's threads, as a whole-call ratio, and whether both took
     the same number of updates and the same labels.
Prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["50000x30x200", "200000x30x500"], help="N x D x k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--host-shapes", type=int, default=1)
    ap.add_argument("--metric", default="cosine", choices=("cosine", "euclidean"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from insider_amd import _lib, api, posthoc, workloads
    lib = _lib.load()
    lines = []
    for pos, shape in enumerate(a.shapes):
        N, D, k = (int(v) for v in shape.split("x"))
        Cm = workloads.init_factors((), D, N)[1]
        rng = np.random.default_rng(7)
        Cm[:, rng.random(N) < 0.3] = 0.0
        alive = np.flatnonzero((Cm * Cm).sum(axis=0) > 0)
        init = np.asfortranarray(Cm[:, rng.choice(alive, k, replace=False)])
        kw = dict(metric=a.metric, init=init, restarts=1)
        api.kmeans(Cm, k, max_iter=0, **kw)                                   # warm-up: code object load
        api.neighbors(Cm, init, k=1, metric="dot")
        km_ms, nn_ms = [], []
        for _ in range(a.reps):
            km_ms.append(api.kmeans(Cm, k, max_iter=0, **kw)["ms"])
            api.neighbors(Cm, init, k=1, metric="dot")
            nn_ms.append(float(lib.insider_hip_last_neighbors_ms()))
        t0 = time.perf_counter()
        run = api.kmeans(Cm, k, max_iter=a.max_iter, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        it = int(run["iters"][0])
        rec = dict(N=N, D=D, k=k, metric=a.metric, alive=int(alive.size), reps=a.reps,
                   assign_ms_median=float(np.median(km_ms)), assign_ms_min=float(np.min(km_ms)), assign_ms_all=km_ms,
                   neighbors_ms_median=float(np.median(nn_ms)), neighbors_ms_min=float(np.min(nn_ms)), neighbors_ms_all=nn_ms,
                   assign_over_neighbors=float(np.median(km_ms) / np.median(nn_ms)),
                   run_iters=it, run_converged=int(run["converged"][0]), run_ms=run["ms"], run_wall_ms=wall,
                   ms_per_iteration=run["ms"] / (it + 1), inertia_first=float(run["traj"][0]), inertia_last=float(run["traj"][it]),
                   source_sha=_lib.library_source_sha())
        if pos < a.host_shapes:
            ref = posthoc.kmeans_host(Cm, k, max_iter=a.max_iter, blas=True, **kw)
            rec.update(host_wall_ms=ref["ms"], host_iters=int(ref["iters"][0]), host_over_device=ref["ms"] / wall,
                       host_threads=os.environ.get("OMP_NUM_THREADS"), host_min_gap=ref["min_gap"],
                       same_labels=bool(np.array_equal(ref["label"], run["label"])))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
