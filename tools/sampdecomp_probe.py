"""Measurement (GPU box): the per-sample fit diagnostics on the resident data set, next to the per-gene variance decomposition
in the same process, at a workload of insider_amd/workloads.py (default c3, K = 30: 10000 x 50000, X = 4 GB, codes 0.5 GB).

    python tools/sampdecomp_probe.py [--config c3] [--reps 5] [--host-samples 200] [--entries train] [--slabs 0]

Device: InsiderData.sample_decomposition() and InsiderData.variance_decomposition(), alternating, each timed with HIP events
on the null stream around the (synchronous) call, so a figure includes the factor uploads, the level table product and the
copy of the records back; `rocprofv3 --kernel-trace --stats -- python tools/sampdecomp_probe.py --host-samples 0` splits
them into kernels (k_mm_rows builds the table, k_sd_stats is the pass over X and the codes, k_sd_reduce sums the slabs;
k_vd_stats is the per-gene pass).  Host: posthoc.sample_decomposition_host() on every (n / --host-samples)-th sample, wall
clock, scaled linearly to n, and the largest difference of the device records from it relative to the reference's size.
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
    ap.add_argument("--host-samples", type=int, default=200)
    ap.add_argument("--entries", default="train", choices=("all", "train", "test"))
    ap.add_argument("--slabs", type=int, default=0, help="option sd_slabs (0 = automatic)")
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
    ds.set_option("sd_slabs", a.slabs)
    calls = dict(sd=ds.sample_decomposition, vd=ds.variance_decomposition)
    for fn in calls.values():                                # workspace allocation, code object load
        fn(A, Cm, entries=a.entries)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = dict(sd=[], vd=[])
    rec = None
    for _ in range(a.reps):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            ev0.record()
            r = fn(A, Cm, entries=a.entries)
            ev1.record()
            ev1.synchronize()
            ms[name].append(ev0.elapsed_time(ev1))
            if name == "sd":
                rec = r
    out = dict(config=a.config, n=n, p=p, K=K, blocks=len(A), entries=a.entries, sd_path=int(ds.info("sd_path")),
               sd_slabs=int(ds.info("sd_slabs")), vd_path=int(ds.info("vd_path")), stream_gb=n * p * 9 / 1e9,
               sd_call_ms_median=float(np.median(ms["sd"])), sd_call_ms_min=float(np.min(ms["sd"])),
               vd_call_ms_median=float(np.median(ms["vd"])), vd_call_ms_min=float(np.min(ms["vd"])))
    ds.close()
    if a.host_samples > 0:
        rows = np.arange(0, n, max(1, n // a.host_samples))
        mask = {"all": None, "train": np.asarray(w.M_train).astype(bool), "test": np.asarray(w.M_test).astype(bool)}[a.entries]
        t0 = time.perf_counter()
        ref = posthoc.sample_decomposition_host(X[rows], lev[rows], None, None if mask is None else mask[rows], A, Cm)
        t1 = time.perf_counter()
        err = 0.0
        for k in ("sum_x", "sum_xx", "rss", "sum_g", "sum_gg", "sum_rg"):
            d = np.abs(rec[k][..., rows] - ref[k])
            err = max(err, float(np.max(d / np.maximum(np.abs(ref[k]), 1e-300))))
        out.update(host_samples=int(rows.size), host_s=t1 - t0, host_s_scaled_to_n=(t1 - t0) * n / rows.size,
                   n_equal=bool(np.array_equal(rec["n"][rows], ref["n"])), max_rel_diff=err)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
