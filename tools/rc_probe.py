"""Measurement (GPU box): one application of the residual operator (InsiderData.residual_products: Z = R'Q, Y = R Z) at
the c3 shape of insider_amd/workloads.py (10000 x 50000, K = 30) for q = 16 / 32 / 64, next to one level-scores pass over the
same bytes on the same handle in the same process.

    python tools/rc_probe.py [--config c3] [--qs 16 32 64] [--reps 5] [--entries train] [--slabs 0]

Per q, after one warm-up call (workspace allocation, code object load): info "rc_ms", the HIP-event time of the kernels of the
call (k_rc_back, k_rc_fwd, k_rc_reduce), median and minimum over --reps calls, and the whole (synchronous) call timed with HIP
events on the null stream, which adds the factor uploads, the packing of Q and the copies of Z, Y and rss back to the host;
and "rc_ms" of a call without Y (k_rc_back alone), so that the difference is the forward pass.
The level-scores call (covariate 0) is timed the same way, alternating with the operator: its figure is a whole call too (there
is no kernel-only figure for it; `rocprofv3 --kernel-trace --stats -- python tools/rc_probe.py` splits both into kernels).  The
operator streams X and the mask codes twice: bytes = 2 x 9 B x n x p, and "rc_gbs" is that over rc_ms.  Prints one JSON line
per q."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--qs", nargs="+", type=int, default=[16, 32, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--entries", default="train", choices=("all", "train", "test"))
    ap.add_argument("--slabs", type=int, default=0, help="option rc_slabs (0 = automatic)")
    a = ap.parse_args()
    import torch
    from insider_amd import api, workloads
    w = workloads.make(a.config)
    X = np.asarray(w.X)
    n, p = X.shape
    K = w.K
    rng = np.random.default_rng(1)
    A = [np.asfortranarray(rng.standard_normal((int(L), K))) for L in w.n_levels]
    Cm = np.asfortranarray(rng.standard_normal((K, p)))
    ds = api.InsiderData(X, np.asarray(w.levels), w.M_train, w.M_test)
    ds.set_option("rc_slabs", a.slabs)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        ev0.record()
        fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    ls = lambda: ds.level_scores(A, Cm, 0, entries=a.entries)
    ls()
    for q in a.qs:
        Q = np.linalg.qr(rng.standard_normal((n, q)))[0]
        rc = lambda: ds.residual_products(A, Cm, Q, entries=a.entries)
        rc()
        slabs = int(ds.info("rc_slabs"))
        kern, call, lsc, back = [], [], [], []
        for _ in range(a.reps):
            call.append(timed(rc))
            kern.append(ds.info("rc_ms"))
            lsc.append(timed(ls))
            ds.residual_products(A, Cm, Q, entries=a.entries, want_y=False)      # the backward pass alone
            back.append(ds.info("rc_ms"))
        ms = float(np.median(kern))
        nbytes = 2.0 * 9.0 * n * p
        print(json.dumps(dict(config=a.config, n=n, p=p, K=K, blocks=len(A), q=q, entries=a.entries,
                              rc_slabs=slabs, rc_ms_median=ms, rc_ms_min=float(np.min(kern)),
                              rc_back_ms_median=float(np.median(back)),
                              rc_call_ms_median=float(np.median(call)), ls_levels=int(ds.n_levels[0]),
                              ls_slabs=int(ds.info("ls_slabs")), ls_call_ms_median=float(np.median(lsc)),
                              ls_call_ms_min=float(np.min(lsc)), stream_gb=nbytes / 1e9, rc_gbs=nbytes / (ms * 1e-3) / 1e9,
                              flops=4.0 * n * p * (q + K), rc_tflops=4.0 * n * p * (q + K) / (ms * 1e-3) / 1e12)), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
