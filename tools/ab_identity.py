"""A/B (GPU box): fits of one library build dumped for a bit-for-bit comparison with another build's.
    INSIDER_HIP_LIB=<build> python tools/ab_identity.py run <tag>     factors, sweep counts, trajectory -> gpurun_out/ab/<tag>.npz
    python tools/ab_identity.py cmp <tagA> <tagB>                     every array equal, bit for bit?
Cases: c2 in full (K = 20: the four-wave kernel), a 10000 x 8192 slab of c3 (K = 30), a K = 16 and a K = 32 fit, 31 outer
iterations each from the N(0, 1e-6) inits (cold multi-pass iterations included), and one deep fit (sub_tol 1e-7, 61 iterations);
then the batch entry (insider_hip_strong_cd: solutions and sweep counts) in every K band up to K = 64, with an l1 term (enet),
lambda = 0 and alpha = 0, on exactly symmetric XtX (the entry reads one triangle); then the fit's kernel paths on small data
(paths() below)."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.environ.get("GRAFT_REPO_ROOT", "/root/repo"), "gpurun_out", "ab")


def run(tag):
    from insider_amd import api, workloads
    os.makedirs(OUT, exist_ok=True)
    out = {}
    cases = [("c2", dict(), 31, 1e-5), ("c3", dict(p=8192), 31, 1e-5), ("c3", dict(p=4096, K=16), 31, 1e-5),
             ("c3", dict(p=4096, K=32), 21, 1e-5), ("c2", dict(p=4096), 61, 1e-7)]
    for ci, (name, kw, iters, sub_tol) in enumerate(cases):
        w = workloads.make(name, **kw)
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        A = [a.copy(order="F") for a in w.A0]
        C = w.C0.copy(order="F")
        res = ds.optimize(A, C, w.K, w.lam, w.lam, w.alpha, tuning=w.tuning, max_iter=iters - 1, global_tol=-1.0, seed=11,
                          sub_tol=sub_tol)
        sw = ds.sweeps()
        out[f"{ci}_C"] = C
        for i, a in enumerate(A):
            out[f"{ci}_A{i}"] = a
        out[f"{ci}_sweeps"] = np.asarray(sw)
        out[f"{ci}_traj"] = np.asarray(res["traj"])
        print(f"{tag} case {ci} {name} {kw}: K={w.K} iters={res['iters']} last-iteration sweeps mean {np.mean(sw):.1f} max {np.max(sw)}",
              flush=True)
        ds.close()
    for K in (1, 7, 16, 17, 24, 30, 31, 32, 33, 40, 47, 48, 49, 63, 64):
        rng = np.random.default_rng(700 + K)
        B, m = 33, 3 * K + 20                                # a partial last wave at 4 and at 16 problems per wave
        Xs = rng.standard_normal((B, m, K))
        ys = np.einsum("bmk,bk->bm", Xs, rng.standard_normal((B, K)) * (rng.random((B, K)) < 0.5)) + 0.3 * rng.standard_normal((B, m))
        Gs = np.einsum("bmk,bml->bkl", Xs, Xs)
        Gs = 0.5 * (Gs + Gs.transpose(0, 2, 1))
        qs = np.einsum("bmk,bm->bk", Xs, ys)
        ws = 0.1 * rng.standard_normal((B, K))
        for regime, (lam, alpha) in (("enet", (0.35 * float(np.max(np.abs(qs))), 0.6)), ("lambda0", (0.0, 0.5)), ("alpha0", (3.0, 0.0))):
            for mode, cap in ((0, 1 << 24), (1, 1 << 24), (0, 3)):
                beta, sw = api.strong_coordinate_descent(None, None, ws, lam, alpha, Gs, qs, tol=1e-10, seed=5, it=3, order_mode=mode,
                                                         max_sweeps=cap, return_sweeps=True)
                out[f"cd_K{K}_{regime}_m{mode}_c{cap}_beta"] = beta
                out[f"cd_K{K}_{regime}_m{mode}_c{cap}_sweeps"] = sw
        print(f"{tag} strong_cd K={K}: 3 regimes x 3 runs, last sweeps mean {np.mean(sw):.1f}", flush=True)
    paths(tag, out)
    np.savez(os.path.join(OUT, tag + ".npz"), **out)


PATH_KEYS = ("row_merged", "col_stats_path", "col_mfma_per_gene", "row_kernels", "col_stats_kernel", "col_solver", "col_eval",
             "col_q_kernel")
OPTION_SETS = {"fast": dict(row_merged=2, col_factored=2, row_counts=0), "pair": dict(row_merged=2, col_factored=3, row_counts=1),
               "lists": dict(row_merged=0, col_factored=0), "unfused": dict(row_fused=0), "nogemm": dict(row_gemm=0),
               "allreduce": dict(force_allreduce=1), "cd1": dict(cd_variant=1), "cd2": dict(cd_variant=2), "ridge": dict(alpha=0.0)}


def paths(tag, out):
    """The fit's kernel paths on small data: every K band, masked and not, with and without continuous covariates, under each
    option set — the path keys as the handle answers them BEFORE its first call (an error: its status) and after the fit, the
    profile's path flags, and the fit itself.  Then the streaming forms (p = 16400, mm_fast 0 / 1 / 2) and a 60-level covariate."""
    from insider_amd import _lib, api, workloads

    def info(ds):
        vals = []
        for k in PATH_KEYS:
            try:
                vals.append(ds.info(k))
            except _lib.InsiderError as e:
                vals.append(-1000.0 - e.status)
        return np.asarray(vals)

    def one(key, K, tuning, m, opts, n=120, p=61, levels=(6, 4), iters=4):
        opts = dict(opts)
        alpha = opts.pop("alpha", 0.4)
        w = workloads.small(n=n, p=p, level_counts=levels, K=K, f=0.2, tuning=tuning, seed=K + m)
        rng = np.random.default_rng(50 + K + m)
        Z = np.asfortranarray(rng.standard_normal((n, m))) if m else None
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, ctns_confounder=Z)
        try:
            for k, v in opts.items():
                ds.set_option(k, v)
            ds.set_option("profile", 1)
            out[key + "_before"] = info(ds)
            A = [a.copy(order="F") for a in w.A0] + ([np.asfortranarray(rng.standard_normal((m, K)) * 1e-3)] if m else [])
            C = w.C0.copy(order="F")
            try:
                res = ds.optimize(A, C, K, w.lam, w.lam, alpha, tuning=tuning, max_iter=iters - 1, global_tol=-1.0, seed=11,
                                  inc_continuous=1 if m else 0, copy=False)
                out[key + "_traj"] = np.asarray(res["traj"])
                out[key + "_sweeps"] = np.asarray(ds.sweeps())
                prof = ds.profile()
                out[key + "_prof"] = np.asarray([prof[k] for k in ("col_factored", "row_merged", "col_pair", "iters", "col_stats_launches",
                                                                   "row_stats_launches", "cd_launches", "test_launches")], dtype=float)
            except _lib.InsiderError as e:
                out[key + "_status"] = np.asarray([e.status])
            out[key + "_C"] = C
            for i, a in enumerate(A):
                out[f"{key}_A{i}"] = a
            out[key + "_after"] = info(ds)
        finally:
            ds.close()

    count = 0
    for K in (7, 20, 33, 63):
        for tuning in (1, 0):
            for m in (0, 2):
                for name, opts in OPTION_SETS.items():
                    one(f"path_K{K}_t{tuning}_m{m}_{name}", K, tuning, m, opts)
                    count += 1
        print(f"{tag} paths K={K}: {count} fits so far", flush=True)
    for mm in (0, 1, 2):
        one(f"path_stream_mm{mm}", 20, 1, 0, dict(row_merged=2, mm_fast=mm), n=48, p=16400, levels=(40, 20, 3), iters=3)
    for K in (20, 63):
        one(f"path_L60_K{K}", K, 1, 0, dict(row_merged=2), n=201, levels=(60, 7))
    print(f"{tag} paths: {count + 5} fits", flush=True)


def cmp(a, b):
    A, B = np.load(os.path.join(OUT, a + ".npz")), np.load(os.path.join(OUT, b + ".npz"))
    bad = len(set(A.files) ^ set(B.files))      # an array only one build dumped
    for k in set(A.files) & set(B.files):
        same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()
        if not same:
            bad += 1
            d = np.max(np.abs(A[k].astype(float) - B[k].astype(float))) if A[k].shape == B[k].shape else float("nan")
            print(f"DIFFERENT {k}: max abs diff {d}")
    print(f"ab_identity {a} vs {b}: {len(A.files)} arrays, {bad} different -> {'IDENTICAL' if bad == 0 else 'NOT IDENTICAL'}")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(1 if cmp(sys.argv[2], sys.argv[3]) else 0)
