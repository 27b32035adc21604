"""The cases on which the compiled reference (oracle/_ref/insider_ref: the reference's own translation units over the
stand-in of oracle/ref_shim) is compared with the two oracles (tests/test_ref_vs_oracle_cpu.py) and recorded for the HIP
library (tests/golden/make_reference_golden.py -> tests/golden/reference/ -> tests/test_gpu_reference.py).

Pure numpy: every array is a function of the arguments alone.  Everything runs with the cyclic sweep order (order_mode = 1),
the one order the compiled reference has (its randperm is 0..n-1).
"""
import hashlib
import json

import numpy as np

from insider_amd import workloads

CD_KS = (1, 2, 7, 16, 30, 33, 48, 63)
CD_ALPHAS = (0.4, 1.0, 0.05)          # elastic net, pure lasso, near-ridge
CD_TOL = 1e-7
# design seed per K: the first that meets the stopping-margin condition of tests/golden/make_reference_golden.py in all six
# variants (a seed above 0 is a replaced candidate)
CD_SEEDS = {1: 0, 2: 0, 7: 0, 16: 0, 30: 0, 33: 0, 48: 1, 63: 1}

# the CASES / LONG_CASES / LONG_FIT of tests/test_gpu_parity.py that the compiled reference runs (kept equal to them by
# tests/test_ref_vs_oracle_cpu.py::test_cases_are_those_of_the_parity_tests)
SHORT = {
    "plain": dict(),
    "unmasked": dict(tuning=0),
    "interaction": dict(interaction_idx=(1, 2)),
    "na": dict(with_na=True),
    "ridge": dict(alpha=0.0),
    "three_cov": dict(level_counts=(4, 3, 5), n=120, p=100),
    # the parity tests' lasso case has seed 962864; its masks leave genes with no held-out entry, which reach a construct the
    # stand-in refuses (sum of an empty cube selection, src/optimize.cpp:218).  962881 is the next seed whose masks do not and
    # whose fit keeps what the case is there for: a latent dimension dies in every gene, and the 400-iteration fit reaches the
    # decay 1e-4 that tests/test_gpu_parity.py:548 asserts of it.
    "lasso": dict(n=78, p=43, level_counts=(3, 9, 2, 8), K=13, f=0.07, lam=7.0, alpha=1.0, seed=962881),
    "k17": dict(K=17, n=90, p=120),
}
PARITY_LASSO_SEED = 962864
SHORT_FIT = dict(max_iter=30)             # checkpoints 0, 10, 20, 30
EARLY_FIT = dict(max_iter=200, global_tol=1e-3)     # stops on global_tol at a checkpoint (tests/test_gpu_parity.py:517-523)
LONG = dict(SHORT, k30=dict(K=30, n=150, p=40), k40=dict(K=40, n=150, p=30))
LONG_FIT = dict(max_iter=400, global_tol=1e-9)
CONTINUOUS_LONG_FIT = dict(max_iter=200, global_tol=1e-9)


def sha(a):
    a = np.asarray(a)
    return hashlib.sha256(np.asfortranarray(a).tobytes(order="F") + str((a.dtype.str, a.shape)).encode()).hexdigest()


# ---- strong_coordinate_descent -------------------------------------------------------------------------------------------
def cd_problem(K, seed):
    rng = np.random.default_rng([K, seed])
    m = min(130, max(40, 2 * K + 10))
    X = np.asfortranarray(rng.standard_normal((m, K)) @ (np.eye(K) + 0.2 * rng.standard_normal((K, K))))
    bt = rng.standard_normal(K) * (rng.random(K) < 0.6)
    y = X @ bt + 0.5 * rng.standard_normal(m)
    return dict(X=X, y=y, XtX=np.asfortranarray(X.T @ X), Xty=X.T @ y, warm=0.1 * rng.standard_normal(K))


def cd_variants(prob):
    """(name, wstart, lambda, alpha) of one problem: every alpha from a cold and from a warm start."""
    K = prob["Xty"].shape[0]
    out = []
    for alpha in CD_ALPHAS:
        lam = (0.15 if alpha >= 0.4 else 0.5) * float(np.max(np.abs(prob["Xty"])))
        for start in ("cold", "warm"):
            out.append(("a%g_%s" % (alpha, start), np.zeros(K) if start == "cold" else prob["warm"], lam, alpha))
    return out


CD_KKT_SEED = 0       # as CD_SEEDS


def cd_kkt_problem(seed=None):
    """A problem on which the strong rule (src/coordinate_descent.cpp:74) discards a coordinate that the KKT check (:118-123)
    must re-admit: y = a (x0 - rho x1) with x0, x1 correlated rho, so x1'y ~ 0 although x1 carries signal once x0 is fitted."""
    rng = np.random.default_rng([77, CD_KKT_SEED if seed is None else seed])
    m, K, rho, a = 100, 6, 0.9, 3.0
    Z = rng.standard_normal((m, K))
    Z, _ = np.linalg.qr(Z)
    Z *= np.sqrt(m)
    X = Z.copy()
    X[:, 1] = rho * Z[:, 0] + np.sqrt(1 - rho * rho) * Z[:, 1]
    X = np.asfortranarray(X)
    y = a * (X[:, 0] - rho * X[:, 1]) + 0.01 * rng.standard_normal(m)
    q = X.T @ y
    alpha, lam = 0.5, 0.6 * float(np.max(np.abs(q)))
    return dict(X=X, y=y, XtX=np.asfortranarray(X.T @ X), Xty=q, wstart=np.zeros(K), lam=lam, alpha=alpha, tol=CD_TOL)


def strong_rule_excluded(Xty, lam, alpha):
    """The coordinates src/coordinate_descent.cpp:74 discards."""
    a = np.abs(Xty)
    return a < alpha * (2 * lam - a.max())


# ---- the block updates ---------------------------------------------------------------------------------------------------
OP_SEED = 4           # seed of the factors below; as CD_SEEDS, counted from 2


def op_workload():
    """The data set of the row / column update cases: NA entries, every gene with a held-out entry."""
    w = workloads.small(n=36, p=50, with_na=True)
    rng = np.random.default_rng(OP_SEED)
    A = [np.asfortranarray(rng.standard_normal(a.shape) * 0.5) for a in w.A0]
    C = np.asfortranarray(rng.standard_normal(w.C0.shape) * 0.5)
    return w, A, C


def row_factor(w, A):
    return sum(A[i][w.levels[:, i] - 1, :] for i in range(w.levels.shape[1]))


ROW_CASES = {"t1": dict(tuning=1, lam=1.7, cov=0), "t0": dict(tuning=0, lam=1.7, cov=0), "t1_cov1": dict(tuning=1, lam=1.7, cov=1),
             "t1_lam0": dict(tuning=1, lam=0.0, cov=0), "t0_lam0": dict(tuning=0, lam=0.0, cov=1)}
COL_CASES = {"t1_a0.4": dict(tuning=1, alpha=0.4), "t1_a0": dict(tuning=1, alpha=0.0), "t0_a0.4": dict(tuning=0, alpha=0.4),
             "t0_a0": dict(tuning=0, alpha=0.0), "t1_a1": dict(tuning=1, alpha=1.0)}
COL_LAM, COL_TOL = 2.0, 1e-7


def row_inputs(w, A, C, cov):
    """What optimize() hands optimize_row (src/optimize.cpp:338-339): the residual with covariate `cov` added back."""
    resid = w.X - row_factor(w, A) @ C + A[cov][w.levels[:, cov] - 1, :] @ C
    return np.asfortranarray(resid), np.asfortranarray(C @ C.T)


CONTINUOUS_CASES = {"k1_t1": (37, 50, 1, 1), "k1_t0": (37, 50, 1, 0), "k7_t1": (120, 131, 7, 1), "k7_t0": (120, 131, 7, 0),
                    "k30_t1": (64, 90, 30, 1), "k30_t0": (64, 90, 30, 0)}


def continuous_inputs(n, p, K, tuning):
    """As tests/test_gpu_boundary.py:125-135: an arbitrary data matrix, a gene with no held-out entry, a sample held out
    everywhere, and under tuning = 0 a `gram` that is NOT C C' (the reference reads the caller's gram, whatever it holds)."""
    rng = np.random.default_rng(1000 * K + n + tuning)
    Cm = np.asfortranarray(rng.standard_normal((K, p)) * 0.4)
    z = rng.standard_normal(n)
    D = np.asfortranarray(np.outer(z, rng.standard_normal(K) @ Cm) + 0.3 * rng.standard_normal((n, p)))
    M = np.asfortranarray(rng.random((n, p)) > 0.1, dtype=np.uint8)
    M[:, 0] = 1
    M[0, :] = 0
    gram = np.asfortranarray(Cm @ Cm.T) * (1.0 if tuning == 1 else 1.3)
    return dict(data=D, indicator=M, u=rng.standard_normal(K) * 0.05, c_factor=Cm, confd=z, gram=gram, lam=2.5, tuning=tuning)


# ---- optimize() ----------------------------------------------------------------------------------------------------------
def continuous_extra(w):
    """The m = 2 continuous covariates of tests/test_gpu_parity.py:597-600."""
    rng = np.random.default_rng(8)
    Z = np.asfortranarray(rng.standard_normal((w.n, 2)))
    U0 = np.asfortranarray(rng.normal(0.0, 0.001, size=(2, w.K)))
    return Z, U0


def optimize_case(group, name):
    """-> dict(kw (workloads.small keywords), fit (optimize keywords), continuous (bool))."""
    if name == "continuous":
        return dict(kw=dict(with_na=True), fit=dict(SHORT_FIT if group == "optimize_short" else CONTINUOUS_LONG_FIT), continuous=True)
    if name == "early":
        return dict(kw=dict(), fit=dict(EARLY_FIT), continuous=False)
    table, fit = (SHORT, SHORT_FIT) if group == "optimize_short" else (LONG, LONG_FIT)
    return dict(kw=dict(table[name]), fit=dict(fit), continuous=False)


def optimize_names(group):
    return list(SHORT) + ["continuous", "early"] if group == "optimize_short" else list(LONG) + ["continuous"]


def optimize_inputs(case):
    """-> (workload, factor list, Z or None): everything optimize() reads."""
    w = workloads.small(**case["kw"])
    A = [a.copy(order="F") for a in w.A0]
    Z = None
    if case["continuous"]:
        Z, U0 = continuous_extra(w)
        A.append(U0)
    return w, A, Z


def input_hashes(w, A, Z):
    h = dict(X=sha(w.X), levels=sha(w.levels), M_train=sha(w.M_train), M_test=sha(w.M_test), C0=sha(w.C0))
    for i, a in enumerate(A):
        h["A%d" % i] = sha(a)
    if Z is not None:
        h["Z"] = sha(Z)
    return h


def dumps(obj):
    return json.dumps(obj, sort_keys=True)
