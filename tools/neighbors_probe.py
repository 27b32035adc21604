"""Measurement (GPU box): the top-k nearest-neighbour self call (insider_hip_neighbors) on a random column factor of the c3
shape, next to the same job done with torch on the same GPU.

    python tools/neighbors_probe.py [--K 30] [--p 50000] [--k 20] [--metric cosine] [--reps 5] [--out FILE.json]

Library: api.neighbors(C) (the self call: every gene against all genes, itself excluded); the figure is
insider_hip_last_neighbors_ms(), the HIP-event time of the call's kernels (k_nn_prep twice, k_nn_topk; the upload of C and the
copy of the nq x k result are outside it), after one warm-up call, the median and the minimum of --reps calls.
torch yardstick: C resident on the device, columns normalised once under cosine, then per chunk of queries
torch.matmul(Qc.T, C) in fp64, the query's own column set to -inf, torch.topk(k); the chunk is sized so that the score block
stays under 1 GB; timed with device events around the whole loop after one warm-up pass, alternating with the library's calls.
The two agree on the neighbours up to ties and rounding (reported: the share of equal index rows).
fraction of the fp64 MFMA rate: 2 K nq nb flops over the time, over the 78.6 TFLOP/s matrix peak.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--p", type=int, default=50000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--metric", default="cosine", choices=("cosine", "dot"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from insider_amd import _lib, api
    if not torch.cuda.is_available():
        raise SystemExit("neighbors_probe: no GPU visible (there is no CPU fallback and no CPU figure)")
    rng = np.random.default_rng(1)
    Cm = np.asfortranarray(rng.standard_normal((a.K, a.p)))
    lib = _lib.load()
    dev = torch.device("cuda:0")
    Ct = torch.from_numpy(np.ascontiguousarray(Cm.T)).to(dev)             # p x K, one embedding per row
    if a.metric == "cosine":
        Ct = Ct / Ct.norm(dim=1, keepdim=True)
    chunk = max(1, min(a.p, (1 << 30) // (8 * a.p)))                      # score block chunk x p doubles < 1 GB

    def torch_job():
        idx = torch.empty((a.p, a.k), dtype=torch.int64, device=dev)
        val = torch.empty((a.p, a.k), dtype=torch.float64, device=dev)
        for c0 in range(0, a.p, chunk):
            S = torch.matmul(Ct[c0:c0 + chunk], Ct.T)
            S[torch.arange(S.shape[0], device=dev), torch.arange(c0, c0 + S.shape[0], device=dev)] = float("-inf")
            v, i = torch.topk(S, a.k, dim=1)
            idx[c0:c0 + chunk], val[c0:c0 + chunk] = i, v
        return idx, val

    got = api.neighbors(Cm, None, k=a.k, metric=a.metric)                  # warm-up: code object load
    ti, _ = torch_job()
    torch.cuda.synchronize()
    same_rows = float(np.mean(np.all(ti.cpu().numpy() == got["index"], axis=1)))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib_ms, torch_ms = [], []
    for _ in range(a.reps):
        api.neighbors(Cm, None, k=a.k, metric=a.metric)
        lib_ms.append(float(lib.insider_hip_last_neighbors_ms()))
        torch.cuda.synchronize()
        ev0.record()
        torch_job()
        ev1.record()
        ev1.synchronize()
        torch_ms.append(float(ev0.elapsed_time(ev1)))
    flops = 2.0 * a.K * a.p * a.p
    lm, tm = float(np.median(lib_ms)), float(np.median(torch_ms))
    rec = dict(K=a.K, p=a.p, k=a.k, metric=a.metric, reps=a.reps, torch_chunk=chunk,
               neighbors_ms_median=lm, neighbors_ms_min=float(np.min(lib_ms)), neighbors_ms_all=lib_ms,
               torch_ms_median=tm, torch_ms_min=float(np.min(torch_ms)), torch_ms_all=torch_ms,
               neighbors_over_torch=lm / tm, flops=flops,
               neighbors_mfma_frac=flops / (lm * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
               torch_mfma_frac=flops / (tm * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
               equal_index_rows=same_rows, source_sha=_lib.library_source_sha())
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
