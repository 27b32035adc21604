"""Measurement (GPU box): the gene-set enrichment call at the size of a real analysis, next to the numpy yardstick.

    python tools/enrichment_time.py [--profiles 30] [--genes 50000] [--sets 5000] [--perms 1000] [--reps 3]
                                    [--host-sets 10] [--host-perms 20] [--out FILE]

Profiles: standard normal with 60 % exact zeros in absolute value (what |column_factor| of an elastic-net fit looks like);
sets: --sets random gene sets of sizes uniform in 15..500; weight 1.  api.enrichment() once to warm up (code object load), then
--reps times: insider_hip_last_enrichment_ms() (HIP events around the call's kernels; the host-side ranking and the transfers
are outside) and the wall time of the whole call.  The yardstick posthoc.enrichment_host() is too slow to run at that size: it
is timed on the first --host-sets sets with 1 and with --host-perms draws, which splits its time into the ranking (timed alone),
the observed scores (per set) and the null (per draw and distinct set size: it scores a draw once per size, for all profiles);
the extrapolation scales each part by its own count.  The device's counts on those sets are compared with the yardstick's at
the same draws.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", type=int, default=30)
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--sets", type=int, default=5000)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sets", type=int, default=10)
    ap.add_argument("--host-perms", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from insider_amd import _lib, api, posthoc
    rng = np.random.default_rng(1)
    R, p, S = a.profiles, a.genes, a.sets
    sc = np.abs(rng.standard_normal((R, p)))
    sc[rng.random((R, p)) < 0.6] = 0.0
    sizes = rng.integers(15, 501, S)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    genes = np.concatenate([rng.choice(p, m, replace=False) for m in sizes]).astype(np.int32)
    lib = _lib.load()
    api.enrichment(sc[:1], ptr[:3], genes[:ptr[2]], nperm=2)                     # warm-up
    kernel_ms, call_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rec = api.enrichment(sc, ptr, genes, nperm=a.perms, weight=1)
        call_s.append(time.perf_counter() - t0)
        kernel_ms.append(float(lib.insider_hip_last_enrichment_ms()))
    # the yardstick on a fraction: t(1 draw) and t(hp draws) on the first hs sets split its time into the ranking (timed alone),
    # the observed scores (per set) and the null (per draw and distinct size); each part is scaled by its own count
    hs, hp = min(a.host_sets, S), max(2, min(a.host_perms, a.perms))
    t0 = time.perf_counter()
    np.argsort(-sc, axis=1, kind="stable")
    rank_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    posthoc.enrichment_host(sc, ptr[:hs + 1], genes[:ptr[hs]], nperm=1, weight=1)
    t1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = posthoc.enrichment_host(sc, ptr[:hs + 1], genes[:ptr[hs]], nperm=hp, weight=1)
    thp = time.perf_counter() - t0
    hsz, nsz = int(np.unique(sizes[:hs]).size), int(np.unique(sizes).size)
    per_draw_size = (thp - t1) / ((hp - 1) * hsz)
    per_set = max(t1 - rank_s - per_draw_size * hsz, 0.0) / hs
    host_full = rank_s + per_set * S + per_draw_size * nsz * a.perms
    got = api.enrichment(sc, ptr[:hs + 1], genes[:ptr[hs]], nperm=hp, weight=1)
    line = dict(profiles=R, genes=p, sets=S, distinct_sizes=nsz, perms=a.perms, weight=1,
                kernel_ms_median=float(np.median(kernel_ms)), kernel_ms_min=float(np.min(kernel_ms)), kernel_ms_all=kernel_ms,
                call_s_median=float(np.median(call_s)), host_sets=hs, host_distinct_sizes=hsz, host_perms=hp,
                host_fraction_of_null=hsz * hp / (nsz * a.perms), host_s_measured=thp, host_s_one_draw=t1, host_rank_s=rank_s,
                host_s_per_draw_and_size=per_draw_size, host_s_per_set=per_set, host_s_extrapolated=host_full,
                counts_equal_on_host_sets=bool(np.array_equal(got["n_ge"], ref["n_ge"]) and
                                               np.array_equal(got["n_same"], ref["n_same"])),
                es_max_abs_diff_on_host_sets=float(np.abs(got["es"] - ref["es"]).max()),
                smallest_pval=float(((rec["n_ge"] + 1.0) / (rec["n_same"] + 1.0)).min()),
                source_sha=_lib.library_source_sha())
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
