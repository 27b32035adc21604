"""Batch-entry results of the K <= 30 sweep kernels as one build computes them, for tests/test_gpu_cd_deferred.py.
    python tools/cd_deferred_golden.py [OUT.npz]        (GPU box; default tests/golden/cd_deferred_parent.npz)
The committed file was written by the build BEFORE the coefficient increments moved from the step into the sweep's exit block
(insider_cd_reg.hpp): the test recomputes every case with the library in the tree and demands the same bits.

Cases (cases() below, shared with the test): problems built like tests/test_gpu_col_solvers.py's _batch_block, half of the true
coefficients zero, one problem with an all-zero Gram column; K at the edges of the one-slot loop, of KMAX = 18 / 20 / 30 and at
odd K under an even KMAX; B = 33 (a last wave with one gene and three empty rows) and B = 3; enet and lasso (l2 = 0); both
order modes; solves capped at 1 and 3 sweeps and uncapped at tol 1e-10."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cd_deferred_parent.npz")

KS = (1, 15, 16, 17, 19, 20, 29, 30)
BS = (33, 3)
REGIMES = {"enet": 0.6, "lasso": 1.0}          # alpha; lambda = 0.35 max |Xty| of the batch
MODES = (0, 1)
UNCAPPED = 1 << 24
CAPS = (1, 3, UNCAPPED)
TOL = 1e-10
ZERO_PROBLEM = 1                               # the problem whose Gram column K // 2 is exactly zero


def problems(K, B):
    """Xs, ys, Gs, qs, ws of a batch: _batch_block's recipe from a stream keyed by (K, B)."""
    rng = np.random.default_rng([900 + K, B])
    m = 3 * K + 20
    Xs = rng.standard_normal((B, m, K), dtype=np.float32).astype(np.float64)
    Xs[ZERO_PROBLEM, :, K // 2] = 0.0
    bt = rng.standard_normal((B, K)) * (rng.random((B, K)) < 0.5)
    ys = np.matmul(Xs, bt[:, :, None])[:, :, 0] + 0.3 * rng.standard_normal((B, m))
    ws = 0.1 * rng.standard_normal((B, K))
    Gs = np.matmul(Xs.transpose(0, 2, 1), Xs)
    qs = np.matmul(Xs.transpose(0, 2, 1), ys[:, :, None])[:, :, 0]
    return Xs, ys, Gs, qs, ws


def cases(K):
    """(key, B, regime, lambda, alpha, order mode, cap, problem arrays) of every run at this K."""
    for B in BS:
        P = problems(K, B)
        lam = 0.35 * float(np.max(np.abs(P[3])))
        for regime, alpha in REGIMES.items():
            for mode in MODES:
                for cap in CAPS:
                    yield f"K{K}_B{B}_{regime}_m{mode}_c{cap}", B, regime, lam, alpha, mode, cap, P


def solve(lam, alpha, mode, cap, P):
    from insider_amd import api
    _, _, Gs, qs, ws = P
    return api.strong_coordinate_descent(None, None, ws, lam, alpha, Gs, qs, tol=TOL, seed=5, it=3, order_mode=mode,
                                         max_sweeps=cap, return_sweeps=True)


def main(path):
    sys.path.insert(0, ROOT)
    out = {}
    for K in KS:
        for key, B, regime, lam, alpha, mode, cap, P in cases(K):
            beta, sw = solve(lam, alpha, mode, cap, P)
            out[key + "_beta"] = beta
            out[key + "_sweeps"] = np.asarray(sw, dtype=np.int32)
        print(f"K={K}: last run's sweeps mean {np.mean(sw):.1f} max {np.max(sw)}", flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
