"""Measurement (GPU box): the outlier calls on the resident data set, next to the per-gene variance decomposition on the same
handle, at a workload of insider_amd/workloads.py (default c3: 10000 x 50000, K = 30).

    python tools/ol_time.py [--configs c3] [--reps 5] [--entries train] [--threshold 3]

One process, one handle.  InsiderData.variance_decomposition(entries) and InsiderData.outliers(..., threshold, cap=None) with
the center and scale of that record (posthoc.residual_center_scale), after one warm-up call each (workspace allocation, code
object load), alternating, each timed with HIP events on the null stream around the (synchronous) call: a figure includes the
factor uploads and the copy of the results back to the host (the list is 16 bytes per call).  Both calls stream X and the mask
codes once; the outlier call adds the n p / 8-byte bitmap, the scan and the fill pass over the calls.
`rocprofv3 --kernel-trace --stats -- python tools/ol_time.py` (a run of its own) splits a call into kernels (k_ol_flag,
k_ol_scan, k_ol_fill next to k_vd_stats).  Prints one JSON line per workload."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--entries", default="train", choices=("all", "train", "test"))
    ap.add_argument("--threshold", type=float, default=3.0)
    a = ap.parse_args()
    import torch
    from insider_amd import api, posthoc, workloads
    for cfg in a.configs:
        w = workloads.make(cfg)
        X = np.asarray(w.X)
        n, p = X.shape
        K = w.K
        rng = np.random.default_rng(1)
        A = [np.asfortranarray(rng.standard_normal((int(L), K))) for L in w.n_levels]
        Cm = np.asfortranarray(rng.standard_normal((K, p)))
        ds = api.InsiderData(X, np.asarray(w.levels), w.M_train, w.M_test)
        center, scale = posthoc.residual_center_scale(ds.variance_decomposition(A, Cm, entries=a.entries))
        calls = dict(vd=lambda: ds.variance_decomposition(A, Cm, entries=a.entries),
                     ol=lambda: ds.outliers(A, Cm, scale, center=center, threshold=a.threshold, entries=a.entries, cap=None))
        out = {name: fn() for name, fn in calls.items()}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = dict(vd=[], ol=[])
        for _ in range(a.reps):
            for name, fn in calls.items():
                torch.cuda.synchronize()
                ev0.record()
                fn()
                ev1.record()
                ev1.synchronize()
                ms[name].append(ev0.elapsed_time(ev1))
        vd, ol = float(np.median(ms["vd"])), float(np.median(ms["ol"]))
        total = int(out["ol"]["total"])
        print(json.dumps(dict(config=cfg, n=n, p=p, K=K, blocks=len(A), entries=a.entries, threshold=a.threshold,
                              vd_path=int(ds.info("vd_path")), ol_path=int(ds.info("ol_path")), total=total,
                              call_rate=total / float(out["vd"]["n"].sum()), vd_call_ms_median=vd,
                              vd_call_ms_min=float(np.min(ms["vd"])), ol_call_ms_median=ol,
                              ol_call_ms_min=float(np.min(ms["ol"])), ol_over_vd=ol / vd, bitmap_mb=n * p / 8 / 1e6,
                              list_mb=16 * total / 1e6)), flush=True)
        ds.close()
        del ds, X, w


if __name__ == "__main__":
    main()
