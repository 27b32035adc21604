"""Measurement (GPU box): the exact t-SNE map of a synthetic column factor on the device (insider_hip_tsne).

    python tools/tsne_time.py [--shapes 10000x64 50000x64] [--max-iter 1000] [--slabs 0] [--dim 30] [--out FILE]

Points: the seeded C0 of workloads.init_factors (D x N), 10 % of its columns set to zero as an elastic-net fit leaves them
(dead under cosine); the graph is posthoc.embedding_graph(k) under cosine (its time is reported apart), perplexity k / 3.  Per
shape, after a warm-up call of 2 iterations: one call of --max-iter iterations, insider_hip_last_tsne_ms() (every kernel from
the calibration to the final evaluation; the host's transpose, the upload and the download are in wall_ms only) and a second
call of 0 iterations at the returned map (calibration + one evaluation), so that
    ms_per_iteration = (run_ms - eval_ms) / max_iter,   pairs_per_s = Na^2 / ms_per_iteration.
Under `rocprofv3 --kernel-trace --stats -- python tools/tsne_time.py --shapes 50000x64 --max-iter 100` the per-kernel split comes
from the trace.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000x64", "50000x64"], help="N x k")
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--slabs", type=int, default=0)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from insider_amd import _lib, api, posthoc, workloads
    lines = []
    for shape in a.shapes:
        N, k = (int(v) for v in shape.split("x"))
        Cm = workloads.init_factors((), a.dim, N)[1]
        Cm[:, np.random.default_rng(7).random(N) < 0.1] = 0.0
        t0 = time.perf_counter()
        idx, d2 = posthoc.embedding_graph(Cm, k)
        graph_wall = (time.perf_counter() - t0) * 1e3
        kw = dict(perplexity=k / 3.0, slabs=a.slabs)
        api.tsne(idx, d2, max_iter=2, **kw)                                   # warm-up: code object load
        t0 = time.perf_counter()
        run = api.tsne(idx, d2, max_iter=a.max_iter, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        ev = api.tsne(idx, d2, max_iter=0, init=np.nan_to_num(run["y"]), **kw)
        na = int(run["alive"].sum())
        per_iter = (run["ms"] - ev["ms"]) / max(a.max_iter, 1)
        rec = dict(N=N, k=k, alive=na, max_iter=a.max_iter, slabs=a.slabs, graph_wall_ms=graph_wall, run_ms=run["ms"],
                   run_wall_ms=wall, eval_ms=ev["ms"], ms_per_iteration=per_iter, pairs_per_s=na * float(na) / (per_iter * 1e-3),
                   kl_first=float(run["kl_traj"][0]), kl_last=run["final_kl"], finite=bool(np.isfinite(run["y"][run["alive"]]).all()),
                   source_sha=_lib.library_source_sha())
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
