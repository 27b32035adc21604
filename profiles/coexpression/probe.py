import json, sys, time
import numpy as np
from insider_amd import api, workloads

out = {}
def log(*a):
    print(*a, flush=True)

def run(name, axes):
    t0 = time.time()
    w = workloads.make(name)
    log(name, "made in", round(time.time() - t0, 1), "s", w.X.shape)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    log(name, "resident", round(time.time() - t0, 1))
    A, Cm = w.A0, w.C0
    rec = {}
    for axis in axes:
        N, depth = (w.p, w.n) if axis == "genes" else (w.n, w.p)
        runs = []
        for rep in range(4):
            t = time.time()
            ds.coexpression(A, Cm, axis=axis, k=10, entries="train")
            wall = time.time() - t
            runs.append(dict(wall_s=wall, cx_ms=ds.info("cx_ms"), cx_stage_ms=ds.info("cx_stage_ms"), cx_stage_mb=ds.info("cx_stage_mb")))
            log(name, axis, rep, runs[-1])
        best = min(r["cx_ms"] for r in runs[1:])
        rec[axis] = dict(N=N, depth=depth, runs=runs, tflops=2.0 * depth * N * N / (best * 1e-3) / 1e12)
        log(name, axis, "TFLOP/s", rec[axis]["tflops"])
    Q = np.asfortranarray(np.random.default_rng(0).standard_normal((w.n, 64)))
    rp = []
    for rep in range(4):
        t = time.time()
        ds.residual_products(A, Cm, Q, entries="train", want_y=False)
        rp.append(dict(wall_s=time.time() - t, rc_ms=ds.info("rc_ms")))
        log(name, "residual_products", rep, rp[-1])
    rec["residual_products_q64"] = rp
    ds.close()
    out[name] = rec
    json.dump(out, open("profiles/coexpression/probe_c1_c3.json", "w"), indent=1)

run("c1", ("genes", "samples"))
run("c3", ("genes", "samples"))
log("done")
