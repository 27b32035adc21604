"""Set-up time of a re-masked data set against a created one.

    python tools/remask_setup.py --workload c2 [--folds 5] [--repeat 5] [--out FILE.json]

For one workload of insider_amd/workloads.py: wall time around InsiderData(...) (insider_hip_create_ex), a.remask(...) and
a.fold(1) of the same data and the same masks, each followed by a device synchronise; median of --repeat after one warm-up.
The host-to-device bytes are what each call uploads by construction (X: 8 n p; each mask: n p; the fold ids: n p, once per
data set).  A device-to-device copy of p x ldn bytes (what k_fold_codes reads and writes) is timed as the yardstick of a
byte stream; the kernel's own time comes from running this script under `rocprofv3 --kernel-trace --stats`.
Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from insider_amd import api, workloads  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    hip = ctypes.CDLL("libamdhip64.so")
    w = workloads.make(a.workload)
    n, p = w.n, w.p
    ids = api.fold_splitter(w.X, folds=a.folds, rm_na_col=False)["fold_id"]
    tr2 = np.asfortranarray(ids != 1, dtype=np.uint8)
    te2 = np.asfortranarray(ids == 1, dtype=np.uint8)

    def timed(fn, keep=False):
        ts, last = [], None
        for i in range(a.repeat + 1):
            t0 = time.perf_counter()
            hd = fn()
            assert hip.hipDeviceSynchronize() == 0
            dt = time.perf_counter() - t0
            if i > 0:
                ts.append(dt)
            if keep and i == a.repeat:
                last = hd
            else:
                hd.close()
        return statistics.median(ts), last

    t_create, src = timed(lambda: api.InsiderData(w.X, w.levels, tr2, te2), keep=True)
    t_remask, _ = timed(lambda: src.remask(tr2, te2))
    t0 = time.perf_counter()
    src.set_folds(ids, a.folds)
    assert hip.hipDeviceSynchronize() == 0
    t_set_folds = time.perf_counter() - t0
    t_fold, b = timed(lambda: src.fold(1), keep=True)
    # the yardstick of a byte stream: a device-to-device copy of p x ldn bytes (what k_fold_codes reads and writes)
    ldn = (n + 127) // 128 * 128
    nbytes = p * ldn
    d_src, d_dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_src), ctypes.c_size_t(nbytes)) == 0
    assert hip.hipMalloc(ctypes.byref(d_dst), ctypes.c_size_t(nbytes)) == 0
    cp = []
    for i in range(6):
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        assert hip.hipMemcpyDtoD(d_dst, d_src, ctypes.c_size_t(nbytes)) == 0
        assert hip.hipDeviceSynchronize() == 0
        if i:
            cp.append(time.perf_counter() - t0)
    hip.hipFree(d_src)
    hip.hipFree(d_dst)
    res = dict(workload=a.workload, n=n, p=p, folds=a.folds, repeat=a.repeat,
               create_s=t_create, remask_s=t_remask, fold_s=t_fold, set_folds_once_s=t_set_folds,
               h2d_bytes=dict(create=8 * n * p + 2 * n * p, remask=2 * n * p, fold=0, set_folds_once=n * p),
               data_bytes=dict(created_own=src.info("data_bytes_own"), fold_shared=b.info("data_bytes_shared"),
                               fold_own=b.info("data_bytes_own")),
               codes_bytes=nbytes, d2d_copy_s=statistics.median(cp), d2d_copy_gbps=2 * nbytes / statistics.median(cp) / 1e9)
    b.close()
    src.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
