"""Times InsiderData.coexpression_pairwise() next to InsiderData.coexpression() on the same resident workload in one session
(README.md in this directory): k = 10, entries = train, the workload's initial factors, one warm-up call then three, HIP-event
times from the handle's info.  python profiles/coexpression/probe_pairwise.py OUT.json [workload:axis ...]"""
import json
import sys
import time

from insider_amd import api, workloads

CASES = sys.argv[2:] or ["c1:genes", "c1:samples", "c3:genes"]
out = {}


def log(*a):
    print(*a, flush=True)


def timed(ds, call, keys):
    runs = []
    for rep in range(4):
        t = time.time()
        call()
        runs.append(dict(wall_s=time.time() - t, **{k: ds.info(k) for k in keys}))
        log("   ", rep, runs[-1])
    return runs


for name in dict.fromkeys(c.split(":")[0] for c in CASES):
    t0 = time.time()
    w = workloads.make(name)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    log(name, w.X.shape, "resident after", round(time.time() - t0, 1), "s")
    for axis in (c.split(":")[1] for c in CASES if c.split(":")[0] == name):
        N, depth = (w.p, w.n) if axis == "genes" else (w.n, w.p)
        log(name, axis, "zero-filled")
        zero = timed(ds, lambda: ds.coexpression(w.A0, w.C0, axis=axis, k=10, entries="train"), ("cx_stage_ms", "cx_ms"))
        log(name, axis, "pairwise")
        pair = timed(ds, lambda: ds.coexpression_pairwise(w.A0, w.C0, axis=axis, k=10, entries="train"),
                     ("cx_stage_ms", "cx_pc_ms", "cx_stage_mb"))
        cx, pc = min(r["cx_ms"] for r in zero[1:]), min(r["cx_pc_ms"] for r in pair[1:])
        out[f"{name}:{axis}"] = dict(N=N, depth=depth, min_overlap=api.pairwise_min_overlap(None, depth), zero=zero, pairwise=pair,
                                     ratio=pc / cx, zero_tflops=2.0 * depth * N * N / (cx * 1e-3) / 1e12,
                                     pairwise_tflops=12.0 * depth * N * N / (pc * 1e-3) / 1e12)
        log(name, axis, {k: v for k, v in out[f"{name}:{axis}"].items() if k not in ("zero", "pairwise")})
        json.dump(out, open(sys.argv[1], "w"), indent=1)
    ds.close()
log("done")
