"""Measurement (GPU box): glm_interaction() on the resident data set against the host path it replaces, at a workload of
insider_amd/workloads.py (default c3, K = 30: 10000 x 50000, X = 4 GB).

    python tools/posthoc_probe.py [--config c3] [--reps 5] [--no-host]

Device: InsiderData.interaction_glm() for the levels of covariate 0 against the residual of covariate 1, timed with HIP
events on the null stream around the (synchronous) call, so the figure includes the factor uploads and the host-built group
tables; `rocprofv3 --kernel-trace --stats -- python tools/posthoc_probe.py --no-host` splits it into kernels (k_resid_stats
is the one pass over X).  Host: the same residual in numpy (X - U C) plus posthoc.glm_interaction() on it, wall clock.
Prints one JSON line."""
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
    ap.add_argument("--no-host", action="store_true")
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
    group = lev[:, 0]
    sub = [0] + [1] * (lev.shape[1] - 1)
    ds = api.InsiderData(X, lev, w.M_train, w.M_test)
    ds.interaction_glm(A, Cm, group, subtract=sub)      # workspace allocation, code object load
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        ev0.record()
        coeff, se, dof = ds.interaction_glm(A, Cm, group, subtract=sub)
        ev1.record()
        ev1.synchronize()
        dev_ms.append(ev0.elapsed_time(ev1))
    ds.close()
    out = dict(config=a.config, n=n, p=p, K=K, groups=int(group.max()), x_gb=n * p * 8 / 1e9,
               device_call_ms_median=float(np.median(dev_ms)), device_call_ms_min=float(np.min(dev_ms)))
    if not a.no_host:
        t0 = time.perf_counter()
        U = sum(A[b][lev[:, b] - 1] for b in range(lev.shape[1]) if sub[b])
        R = X - U @ Cm
        t1 = time.perf_counter()
        ref_c, _ = posthoc.glm_interaction(R, None, group, Cm)
        t2 = time.perf_counter()
        out.update(host_residual_s=t1 - t0, host_glm_s=t2 - t1, host_total_s=t2 - t0,
                   max_rel_coeff_diff=float(np.max(np.abs(coeff - ref_c)) / np.max(np.abs(ref_c))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
