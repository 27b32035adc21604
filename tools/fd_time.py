"""Measurement (GPU box): the per-factor decomposition on the resident data set, next to the per-gene variance decomposition
on the same handle, at workloads of insider_amd/workloads.py (default c3 and c5).

    python tools/fd_time.py [--configs c3 c5] [--reps 5] [--entries train]

InsiderData.factor_decomposition() and InsiderData.variance_decomposition(), after one warm-up call each (workspace
allocation, code object load), alternating, each timed with HIP events on the null stream around the (synchronous) call: a
figure includes the factor uploads and the copy of the records back to the host (p (4 + 3 (B + 1) K) doubles for the factor
decomposition, 110 MB at c3).  `rocprofv3 --kernel-trace --stats -- python tools/fd_time.py --configs c3` splits a call
into kernels (k_fd_build_w, k_fd_prod<QT, KS, true> the heavy pass, k_fd_prod<QT, 1, false> the light one, k_fd_finish).
Flop count: the three products, 3 x 2 n p (B + 1) K.  Prints one JSON line per workload."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--entries", default="train", choices=("all", "train", "test"))
    a = ap.parse_args()
    import torch
    from insider_amd import api, workloads
    for cfg in a.configs:
        w = workloads.make(cfg)
        X = np.asarray(w.X)
        n, p = X.shape
        K = w.K
        rng = np.random.default_rng(1)
        A = [np.asfortranarray(rng.standard_normal((int(L), K))) for L in w.n_levels]
        Cm = np.asfortranarray(rng.standard_normal((K, p)))
        ds = api.InsiderData(X, np.asarray(w.levels), w.M_train, w.M_test)
        calls = dict(fd=ds.factor_decomposition, vd=ds.variance_decomposition)
        for fn in calls.values():
            fn(A, Cm, entries=a.entries)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = dict(fd=[], vd=[])
        for _ in range(a.reps):
            for name, fn in calls.items():
                torch.cuda.synchronize()
                ev0.record()
                fn(A, Cm, entries=a.entries)
                ev1.record()
                ev1.synchronize()
                ms[name].append(ev0.elapsed_time(ev1))
        B = len(A)
        flops = 6.0 * n * p * (B + 1) * K
        fd, vd = float(np.median(ms["fd"])), float(np.median(ms["vd"]))
        path = int(ds.info("fd_path"))
        heavy_tiles = -(-B * K // 16)
        print(json.dumps(dict(config=cfg, n=n, p=p, K=K, blocks=B, entries=a.entries, fd_path=path,
                              x_reads=1 if path == 1 else -(-heavy_tiles // 8), vd_path=int(ds.info("vd_path")),
                              fd_call_ms_median=fd, fd_call_ms_min=float(np.min(ms["fd"])), vd_call_ms_median=vd,
                              vd_call_ms_min=float(np.min(ms["vd"])), fd_over_vd=fd / vd, flops=flops,
                              fd_tflops_of_call=flops / (fd * 1e-3) / 1e12,
                              record_mb=p * (4 + 3 * (B + 1) * K) * 8 / 1e6)), flush=True)
        ds.close()
        del ds, X, w


if __name__ == "__main__":
    main()
