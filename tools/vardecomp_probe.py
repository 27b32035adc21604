"""Measurement (GPU box): the per-gene variance decomposition on the resident data set against the numpy path, at a workload
of insider_amd/workloads.py (default c3, K = 30: 10000 x 50000, X = 4 GB, codes 0.5 GB).

    python tools/vardecomp_probe.py [--config c3] [--reps 5] [--host-genes 5000] [--entries train]

Device: InsiderData.variance_decomposition() timed with HIP events on the null stream around the (synchronous) call, so the
figure includes the factor uploads, the level table product and the copy of the records back; `rocprofv3 --kernel-trace
--stats -- python tools/vardecomp_probe.py --host-genes 0` splits it into kernels (k_mm_rows builds the table, k_vd_stats
is the one pass over X and the codes).  Host: posthoc.variance_decomposition_host() on the first --host-genes genes, wall
clock, scaled linearly to p (the whole matrix does not fit a host path's temporaries), and the largest difference of the
device records from it relative to the record's scale.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-genes", type=int, default=5000)
    ap.add_argument("--entries", default="train", choices=("all", "train", "test"))
    a = ap.parse_args()
    import torch
    from insider_amd import api, posthoc, workloads
    w = workloads.make(a.config)
    X = np.asarray(w.X)
    lev = np.asarray(w.levels)
    n, p = X.shape
    K = w.K
    rng = np.random.default_rng(1)
    A = [np.asfortranarray(rng.standard_normal((int(L), K))) for L in w.n_levels]
    Cm = np.asfortranarray(rng.standard_normal((K, p)))
    ds = api.InsiderData(X, lev, w.M_train, w.M_test)
    ds.variance_decomposition(A, Cm, entries=a.entries)      # workspace allocation, code object load
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        ev0.record()
        rec = ds.variance_decomposition(A, Cm, entries=a.entries)
        ev1.record()
        ev1.synchronize()
        dev_ms.append(ev0.elapsed_time(ev1))
    path = ds.info("vd_path")
    ds.close()
    out = dict(config=a.config, n=n, p=p, K=K, blocks=len(A), entries=a.entries, vd_path=int(path),
               stream_gb=n * p * 9 / 1e9, device_call_ms_median=float(np.median(dev_ms)),
               device_call_ms_min=float(np.min(dev_ms)))
    if a.host_genes > 0:
        g = np.arange(min(a.host_genes, p))
        mask = {"all": None, "train": np.asarray(w.M_train).astype(bool), "test": np.asarray(w.M_test).astype(bool)}[a.entries]
        t0 = time.perf_counter()
        ref = posthoc.variance_decomposition_host(X[:, g], lev, None, None if mask is None else mask[:, g], A, Cm[:, g])
        t1 = time.perf_counter()
        err = 0.0
        for k in ("sum_x", "sum_xx", "rss", "sum_g", "sum_gg", "sum_rg"):
            d = np.abs(rec[k][..., g] - ref[k])
            err = max(err, float(np.max(d / np.maximum(np.abs(ref[k]), 1e-300))))
        out.update(host_genes=int(g.size), host_s=t1 - t0, host_s_scaled_to_p=(t1 - t0) * p / g.size,
                   n_equal=bool(np.array_equal(rec["n"][g], ref["n"])), max_rel_diff=err)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
