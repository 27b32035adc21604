"""Measurement (GPU box): the level scores on the resident data set, next to the per-sample decomposition on the same
handle (one pass over the same bytes), at workloads of insider_amd/workloads.py (default c3 and c1), scoring covariate 0
and covariate 1.

    python tools/ls_time.py [--configs c3 c1] [--covs 0 1] [--reps 5] [--entries train]

InsiderData.level_scores() and InsiderData.sample_decomposition(), after one warm-up call each (workspace allocation, code
object load), alternating, each timed with HIP events on the null stream around the (synchronous) call: a figure includes
the factor uploads and the copy of the n x L scores back to the host.  `rocprofv3 --kernel-trace --stats -- python
tools/ls_time.py --configs c3` splits a call into kernels (k_build_R and k_ph_pack_c of the preparation, k_mm_rows the
candidate table, k_ls_prod<QT, KS> the pass, k_ls_reduce the slab sum; k_sd_stats for comparison).  Flop count: the two
products, 4 n p L, and the fit of the tiles, 2 n p K.  Prints one JSON line per workload and covariate."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c1"])
    ap.add_argument("--covs", nargs="+", type=int, default=[0, 1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--entries", default="train", choices=("all", "train", "test"))
    ap.add_argument("--slabs", type=int, default=0, help="option ls_slabs (0 = automatic)")
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
        ds.set_option("ls_slabs", a.slabs)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for cov in a.covs:
            if cov >= ds.c:
                continue
            calls = dict(ls=lambda: ds.level_scores(A, Cm, cov, entries=a.entries),
                         sd=lambda: ds.sample_decomposition(A, Cm, entries=a.entries))
            for fn in calls.values():
                fn()
            ms = dict(ls=[], sd=[])
            for _ in range(a.reps):
                for name, fn in calls.items():
                    torch.cuda.synchronize()
                    ev0.record()
                    fn()
                    ev1.record()
                    ev1.synchronize()
                    ms[name].append(ev0.elapsed_time(ev1))
            L = int(ds.n_levels[cov])
            flops = 4.0 * n * p * L + 2.0 * n * p * K
            ls, sd = float(np.median(ms["ls"])), float(np.median(ms["sd"]))
            path = int(ds.info("ls_path"))
            print(json.dumps(dict(config=cfg, n=n, p=p, K=K, blocks=len(A), cov=cov, L=L, entries=a.entries, ls_path=path,
                                  x_reads=-(-(-(-L // 16)) // 8), ls_slabs=int(ds.info("ls_slabs")),
                                  sd_slabs=int(ds.info("sd_slabs")), ls_call_ms_median=ls,
                                  ls_call_ms_min=float(np.min(ms["ls"])), sd_call_ms_median=sd,
                                  sd_call_ms_min=float(np.min(ms["sd"])), ls_over_sd=ls / sd, flops=flops,
                                  ls_tflops_of_call=flops / (ls * 1e-3) / 1e12, stream_gb=n * p * 9 / 1e9,
                                  partial_mb=int(ds.info("ls_slabs")) * n * (-(-L // 16) * 16) * 8 / 1e6)), flush=True)
        ds.close()
        del ds, X, w


if __name__ == "__main__":
    main()
