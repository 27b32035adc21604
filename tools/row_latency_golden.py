"""Row updates and short fits as one build computes them, for tests/test_gpu_row_latency.py.
    python tools/row_latency_golden.py [OUT.npz]        (GPU box; default tests/golden/row_latency_parent.npz)
The committed file was written by the build BEFORE k_level_merged requested its global loads in batches ahead of its sums
(insider_row_merged.hpp): every sum kept its order on its operands, so the test recomputes every case with the library in the
tree and demands the same bits.  (The same change to the earlier-table part of k_gene_u_cnt, insider_col_factored.hpp, was
measured slower and is not in the tree — profiles/row_latency/README.md; its cases stay, for the next attempt.)

Per case: optimize_row() of every covariate from the same random factors, then one optimize(max_iter = 2) (the side streams'
level sums and the once-per-iteration join behind C'C).  Arrays of more than RAW_MAX elements are kept as their SHA-256.

Cases (CASES below, shared with the test), the smallest shapes at which batched loops can go wrong:
  k_gene_u_cnt, tables of earlier covariates — the covariate with the most levels comes first in the kernel's order, so it is
    the earlier table of every other one: its level count Lp on both sides of a block of 16 and of one and two batches of
    GU_BATCH = 8 blocks; the other covariates with <= 16 table rows (4 count bytes per lane and block) and with more (8);
    three covariates (two earlier tables, the order of out[l] +=); a continuous column; p with a partial last block of waves.
  k_level_merged — gene counts that give 1, 15, 16, 17, 33 slabs of U'C partial sums, 512 and 513 (both sides of LM_YCH = 32
    partial sums per group of 16), none (row_fused = 0); stacked levels SL on both sides of a wave's first step, of one and of
    two operand sets of LM_SCH = 16 steps x 4 waves; K at the edges of the padded lengths and of the in-kernel solve; a level
    without samples; tuning = 0 (the all-zero record); force_allreduce = 1 (no in-kernel solve)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "row_latency_parent.npz")
RAW_MAX = 64
FIT = dict(lambda1=2.0, lambda2=2.0, alpha=0.4, max_iter=2, seed=3)


def case(name, levels, K=5, p=61, n=None, m=0, tuning=1, opts=None, empty_level=False, expect=()):
    return dict(id=name, levels=tuple(levels), K=K, p=p, n=n or 2 * max(levels) + 40, m=m, tuning=tuning,
                opts=dict(row_merged=2, **(opts or {})) if tuning == 1 else dict(opts or {}), empty_level=empty_level,
                expect=tuple(expect))


GU = ("gene_u_cnt",)
CASES = []
for Lp in (1, 15, 16, 17, 128, 129, 257):
    CASES.append(case(f"gu-L{Lp}-rows4", (Lp, min(Lp, 4)), p=5, expect=GU))
for Lp in (17, 128, 129, 257):
    CASES.append(case(f"gu-L{Lp}-rows17", (Lp, 17), p=64, expect=GU))
CASES += [case("gu-three-bpl4", (16, 9, 7), p=130, expect=GU),
          case("gu-three-bpl8", (129, 17, 5), p=130, expect=GU),
          case("gu-three-L257", (257, 16, 15), p=5, expect=GU),
          case("gu-ctns", (17, 4), p=64, m=1, n=150, expect=GU),
          case("gu-ctns-three", (129, 17, 5), p=5, m=2, expect=GU)]
for p in (100, 1920, 2048, 2049, 4100):
    CASES.append(case(f"lm-p{p}", (6, 4), p=p, n=40, expect=("merged_solve",)))
for p in (65536, 65537):
    CASES.append(case(f"lm-p{p}", (3, 2), K=3, p=p, n=24, expect=("merged_solve",)))
CASES.append(case("lm-unfused", (6, 4), p=2049, n=40, opts=dict(row_fused=0), expect=("pack_reduce",)))
for lv in ((1,), (2, 1), (3, 1), (3, 2), (60, 3), (60, 4), (60, 5), (120, 8), (120, 9)):
    CASES.append(case(f"lm-SL{sum(lv)}", lv, K=4, p=130, expect=("merged_solve",)))
for K in (1, 15, 16, 17, 30, 31, 32, 33, 63):
    CASES.append(case(f"lm-K{K}", (6, 4), K=K, p=131, expect=("merged_solve" if K <= 31 else "merged",)))
CASES += [case("lm-empty-level", (6, 4), K=7, p=131, empty_level=True, expect=("merged_solve",)),
          case("lm-empty-level-K30", (60, 5), K=30, p=300, empty_level=True, expect=("merged_solve",)),
          case("lm-tuning0", (6, 4), K=7, p=131, tuning=0, expect=("merged_zero",)),
          case("lm-tuning0-K30", (60, 5), K=30, p=300, tuning=0, expect=("merged_zero",)),
          case("lm-allreduce", (6, 4), K=7, p=131, opts=dict(force_allreduce=1), expect=("merged", "level_solve")),
          case("lm-allreduce-K30", (60, 5), K=30, p=300, opts=dict(force_allreduce=1), expect=("merged", "level_solve"))]
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def data(c):
    """X, levels, masks of the case (workloads.small keyed by its position) and random factors of a usual size."""
    from insider_amd import workloads
    seed = 40 + list(CASE_BY_ID).index(c["id"])
    w = workloads.small(n=c["n"], p=c["p"], level_counts=c["levels"], K=c["K"], f=0.2, seed=seed, tuning=c["tuning"])
    n_levels = np.array(w.n_levels, dtype=np.int32)
    if c["empty_level"]:
        n_levels[0] += 1          # one more level than any sample carries
    rng = np.random.default_rng(7000 + seed)
    A = [np.asfortranarray(rng.standard_normal((int(L), c["K"])) * 0.5) for L in n_levels]
    C = np.asfortranarray(rng.standard_normal((c["K"], c["p"])) * 0.5)
    Z = np.asfortranarray(rng.standard_normal((c["n"], c["m"]))) if c["m"] else None
    if c["m"]:
        A.append(np.asfortranarray(rng.standard_normal((c["m"], c["K"])) * 0.3))
    return w, n_levels, A, C, Z


def keep(a):
    a = np.ascontiguousarray(a)
    return a if a.size <= RAW_MAX else np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def run(c):
    """{key: array} of the case with the library that is loaded, and the row-kernel names every call launched."""
    from insider_amd import _lib, api
    w, n_levels, A, C, Z = data(c)
    inc = 1 if c["m"] else 0
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test, n_levels=n_levels, ctns_confounder=Z)
    out, names = {}, set()

    def launched():
        mask = int(ds.info("row_kernels"))
        return {name for i, name in enumerate(_lib.ROW_KERNELS) if mask >> i & 1}

    try:
        for k, v in c["opts"].items():
            ds.set_option(k, v)
        for cov in range(len(A)):
            got = ds.optimize_row([a.copy(order="F") for a in A], C, cov, lambda_=2.0, tuning=c["tuning"], inc_continuous=inc)
            names |= launched()
            out[f"{c['id']}/row{cov}"] = keep(got)
        r = ds.optimize([a.copy(order="F") for a in A], C.copy(order="F"), c["K"], tuning=c["tuning"], inc_continuous=inc, **FIT)
        names |= launched()
        out[f"{c['id']}/fit_C"] = keep(r["column_factor"])
        for i in range(len(A)):
            out[f"{c['id']}/fit_A{i}"] = keep(r["row_matrices"][f"factor{i}"])
        out[f"{c['id']}/fit_traj"] = keep(r["traj"])
        out[f"{c['id']}/fit_loss"] = np.array([r["loss"], r["train_rmse"], r["test_rmse"]])
    finally:
        ds.close()
    return out, names


def main(path):
    sys.path.insert(0, ROOT)
    out = {}
    for c in CASES:
        o, names = run(c)
        missing = set(c["expect"]) - names
        print(f"{c['id']}: {len(o)} arrays, kernels {sorted(names)}" + (f"  MISSING {sorted(missing)}" if missing else ""), flush=True)
        out.update(o)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
