"""insider_hip_kmeans on the device against the numpy yardstick posthoc.kmeans_host().

Every call goes through ctypes with outputs prefilled with sentinels and NGUARD guard elements past every array's end; the
guards must be unchanged after every call, and after a refused call the whole output is.

Bounds are derived, not fitted.  With u = 2^-53 a D-term fp64 dot in any order errs by at most D u |x| |c| to first order, the
normalisation and h add a few u, so one score of the device and one of the yardstick differ by at most
tol = 4 (D + 4) 2^-52 (cosine, unit vectors) or 4 (D + 4) 2^-52 (|x| |c| + h) (Euclidean).  A point whose best and runner-up
scores in the yardstick differ by more than 2 tol (the larger tol of the two pairs) is DECIDED: both sides must label it alike.
A sum of n terms in any order errs by at most (n - 1) u sum |x|, so a centre coordinate of the device and of the yardstick
differ by at most (n_j + 4) 2^-52 sum_members |x_d| on the sum, divided by n_j (Euclidean).  Under cosine the sum is not
returned; c = S / |S|, so c_dev |S_ref| - S_ref carries the sum's error b_d plus S_d times the relative error of |S_dev|
against |S_ref|, which is at most |b|_2 / |S| from the sums and (D + 4) 2^-52 from forming the norm: the bound used is
b_d + |S_d| (|b|_2 / |S| + (D + 4) 2^-52)."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from tests.support import bits, lib  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu

NGUARD = 7
INT_SENTINEL = -77
DBL_SENTINEL = 12345.678
COS, EUC = 0, 1
METRIC = {COS: "cosine", EUC: "euclidean"}
U52 = 2.0 ** -52
NAMES_D = ("centers", "dist", "dist2", "traj", "final_inertia")
NAMES_I = ("label", "second", "sizes", "iters", "converged", "best")
NAMES = NAMES_D + NAMES_I


def call(lib, P, k, metric, init=None, restarts=1, max_iter=0, seed=0x1D5EED, N=None, D=None, expect=_lib.OK, null=(),
         pptr=None):
    """One guarded call.  P: column-major D x N; pptr: a raw address for the points (a window of a larger matrix).  N, D, k,
    restarts and max_iter are passed as given; the arrays are sized from what is sane of them."""
    Dp, Np = P.shape
    N = Np if N is None else N
    D = Dp if D is None else D
    kk, rr, mm = min(max(k, 1), 5000), min(max(restarts, 1), 300), min(max(max_iter, 0), 10001)
    size = dict(centers=Dp * kk, dist=Np, dist2=Np, traj=mm + 1, final_inertia=rr, label=Np, second=Np, sizes=kk, iters=rr,
                converged=rr, best=1)
    out = {n: np.full(size[n] + NGUARD, DBL_SENTINEL) for n in NAMES_D}
    out.update({n: np.full(size[n] + NGUARD, INT_SENTINEL, dtype=np.int32) for n in NAMES_I})
    dp, i32 = C.POINTER(C.c_double), C.c_int32
    pp = C.cast(pptr, dp) if pptr is not None else _lib.ptr(P)
    ip = None if init is None else _lib.ptr(init)
    args = [pp, N, D, k, metric, ip, restarts, max_iter, seed, 0, _lib.ptr(out["centers"]), _lib.ptr(out["label"], i32),
            _lib.ptr(out["dist"]), _lib.ptr(out["second"], i32), _lib.ptr(out["dist2"]), _lib.ptr(out["sizes"], i32),
            _lib.ptr(out["traj"]), _lib.ptr(out["final_inertia"]), _lib.ptr(out["iters"], i32),
            _lib.ptr(out["converged"], i32), _lib.ptr(out["best"], i32)]
    for pos in null:
        args[pos] = None
    status = lib.insider_hip_kmeans(*args)
    assert status == expect, (status, lib.insider_hip_last_error().decode(errors="replace"))
    for n in NAMES_D + NAMES_I:
        used = size[n] if status == _lib.OK else 0
        sentinel = DBL_SENTINEL if n in NAMES_D else INT_SENTINEL
        assert np.all(out[n][used:] == sentinel), n
    if status != _lib.OK:
        return None
    rec = {n: out[n][:size[n]] for n in NAMES_D + NAMES_I}
    rec["centers"] = rec["centers"].reshape((Dp, kk), order="F")
    rec["best"] = int(rec["best"][0])
    return rec


def host(P, k, metric, **kw):
    return posthoc.kmeans_host(P, k, metric=METRIC[metric], **kw)


def window(P, s):
    """The address of column s of the column-major P."""
    assert P.flags.f_contiguous
    return P.ctypes.data + s * P.shape[0] * 8


def rows_equal(got, ref):
    for n in ("label", "second"):
        assert np.array_equal(got[n], ref[n]), n
    for n in ("dist", "dist2"):
        assert np.array_equal(got[n], ref[n], equal_nan=True), n


# ---- 1. exact arithmetic (Euclidean) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 63])
def test_exact_integers_equal_the_yardstick(lib, D):
    """Entries in -2..2: every score is exact in fp64 in any order and ties are everywhere, so this is the test of the tie rule,
    of the K4 padding and of the tile edges.  After one update the centres are integer sums over one division: bit for bit."""
    rng = np.random.default_rng(200 + D)
    for N, k in ((1, 1), (15, 2), (16, 16), (17, 17), (250, 33), (1030, 65), (64, 64)):
        P = np.asfortranarray(rng.integers(-2, 3, (D, N)).astype(np.float64))
        init = np.asfortranarray(rng.integers(-2, 3, (D, k)).astype(np.float64))
        got, ref = call(lib, P, k, EUC, init=init), host(P, k, EUC, init=init, restarts=1, max_iter=0)
        rows_equal(got, ref)
        assert np.array_equal(got["sizes"], ref["sizes"]) and np.array_equal(got["centers"], init)
        assert got["traj"][0] == ref["traj"][0] == got["final_inertia"][0] and got["iters"][0] == 0 and got["converged"][0] == 0
        got, ref = call(lib, P, k, EUC, init=init, max_iter=1), host(P, k, EUC, init=init, restarts=1, max_iter=1)
        assert np.array_equal(got["centers"], ref["centers"]) and got["iters"][0] == 1
        assert got["traj"][0] == ref["traj"][0]


# ---- 2. / 3. real-valued inputs: one assignment, one update ---------------------------------------------------------------------
def decided(ref, P, Cm, metric):
    """Per point: the tolerance of its best score and whether the yardstick's best and runner-up differ by more than 2 tol."""
    D = P.shape[0]
    eps = 4.0 * (D + 4) * U52
    if metric == COS:
        tol1 = tol2 = np.full(P.shape[1], eps)
    else:
        nx, nc = np.sqrt((P * P).sum(axis=0)), np.sqrt((Cm * Cm).sum(axis=0))
        tol1 = eps * (nx * nc[ref["label"]] + 0.5 * nc[ref["label"]] ** 2)
        tol2 = eps * (nx * nc[ref["second"]] + 0.5 * nc[ref["second"]] ** 2)
    return tol1, ref["score"] - ref["score2"] > 2.0 * np.maximum(tol1, tol2)


def center_check(got_c, P, label, metric):
    """The device's centres against the sums of the members (float64 and its bound, module docstring)."""
    D, k = got_c.shape
    X = P / np.sqrt((P * P).sum(axis=0)) if metric == COS else P
    worst = 0.0
    for j in range(k):
        M = X[:, label == j]
        n = M.shape[1]
        if n == 0:
            continue
        S, b = M.sum(axis=1), (n + 4) * U52 * np.abs(M).sum(axis=1)
        if metric == EUC:
            err, bound = np.abs(got_c[:, j] - S / n), b / n
        else:
            nS = np.sqrt((S * S).sum())
            err = np.abs(got_c[:, j] * nS - S)
            bound = b + np.abs(S) * (np.sqrt((b * b).sum()) / nS + (D + 4) * U52)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (j, n)
    print("centres: max error / bound", worst)


@pytest.fixture(scope="module")
def real_cases():
    """Gaussian points and centres and the yardstick's assignment and first update, computed once."""
    cases = {}
    for D in (5, 30, 63):
        for N, k in ((1000, 33), (4096, 257)):
            rng = np.random.default_rng(1000 * D + k)
            P, init = np.asfortranarray(rng.standard_normal((D, N))), np.asfortranarray(rng.standard_normal((D, k)))
            for metric in (COS, EUC):
                cases[D, N, k, metric] = (P, init, host(P, k, metric, init=init, restarts=1, max_iter=0),
                                          host(P, k, metric, init=init, restarts=1, max_iter=1))
    return cases


@pytest.mark.parametrize("metric", [COS, EUC])
@pytest.mark.parametrize("shape", [(1000, 33), (4096, 257)])
@pytest.mark.parametrize("D", [5, 30, 63])
def test_real_inputs_one_assignment(lib, real_cases, D, shape, metric):
    P, init, ref, _ = real_cases[(D,) + shape + (metric,)]
    Cm = init / np.sqrt((init * init).sum(axis=0)) if metric == COS else init
    tol, ok = decided(ref, P, Cm, metric)
    print("undecided share", 1.0 - ok.mean())
    assert 1.0 - ok.mean() <= 0.01
    got = call(lib, P, shape[1], metric, init=init)
    assert np.array_equal(got["label"][ok], ref["label"][ok])
    err = np.abs(got["dist"] - ref["dist"])[ok]
    print("max dist error / tol", float(np.max(err / tol[ok])))
    assert np.all(err <= tol[ok])
    assert np.all((got["label"] >= 0) & (got["label"] < shape[1]) & (got["second"] >= 0) & (got["second"] != got["label"]))
    assert np.array_equal(got["sizes"], np.bincount(got["label"], minlength=shape[1]))


@pytest.mark.parametrize("metric", [COS, EUC])
@pytest.mark.parametrize("shape", [(1000, 33), (4096, 257)])
@pytest.mark.parametrize("D", [5, 30, 63])
def test_real_inputs_one_update(lib, real_cases, D, shape, metric):
    P, init, ref0, ref1 = real_cases[(D,) + shape + (metric,)]
    Cm = init / np.sqrt((init * init).sum(axis=0)) if metric == COS else init
    assert decided(ref0, P, Cm, metric)[1].all()                  # so the first labels are equal on both sides
    got = call(lib, P, shape[1], metric, init=init, max_iter=1)
    assert got["iters"][0] == ref1["iters"][0] == 1
    center_check(got["centers"], P, ref0["label"], metric)
    empty = np.flatnonzero(ref0["sizes"] == 0)
    assert np.allclose(got["centers"][:, empty], Cm[:, empty], rtol=0, atol=4 * U52)   # (an empty cluster keeps its centre)


# ---- 4. whole runs -----------------------------------------------------------------------------------------------------------
def mixture(N, D, k, seed):
    rng = np.random.default_rng(seed)
    mu = 1.5 * rng.standard_normal((D, k))
    P = np.asfortranarray(mu[:, rng.integers(0, k, N)] + rng.standard_normal((D, N)))
    return P, np.asfortranarray(P[:, rng.choice(N, k, replace=False)])


@pytest.fixture(scope="module")
def runs():
    out = {}
    for N, D, k in ((1000, 30, 33), (257, 5, 17), (2000, 63, 65), (500, 3, 16)):
        P, init = mixture(N, D, k, 31 * N + k)
        for metric in (COS, EUC):
            out[N, D, k, metric] = (P, init, host(P, k, metric, init=init, restarts=1, max_iter=100))
    return out


@pytest.mark.parametrize("metric", [COS, EUC])
@pytest.mark.parametrize("shape", [(1000, 30, 33), (257, 5, 17), (2000, 63, 65), (500, 3, 16)])
def test_whole_runs_follow_the_yardstick(lib, runs, shape, metric):
    N, D, k = shape
    P, init, ref = runs[shape + (metric,)]
    print("yardstick: min gap", ref["min_gap"], "iters", ref["iters"][0])
    assert ref["min_gap"] > 1e-9 and ref["converged"][0] == 1
    got = call(lib, P, k, metric, init=init, max_iter=100)
    assert got["iters"][0] == ref["iters"][0] and got["converged"][0] == 1 and got["best"] == 0
    assert np.array_equal(got["label"], ref["label"]) and np.array_equal(got["sizes"], ref["sizes"])
    it = int(ref["iters"][0])
    rel = np.abs(got["traj"][:it + 1] - ref["traj"][:it + 1]) / ref["traj"][:it + 1]
    print("traj: max relative error / bound", float(rel.max() / (N * (D + 4) * U52)))
    assert np.all(rel <= N * (D + 4) * U52) and np.all(np.isnan(got["traj"][it + 1:]))
    assert got["final_inertia"][0] == got["traj"][it]
    center_check(got["centers"], P, ref["label"], metric)        # converged: the last update ran on these labels


# ---- 5. invariants of any run --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, EUC])
def test_invariants_of_a_drawn_run(lib, runs, metric):
    N, D, k = 1000, 30, 33
    P = runs[N, D, k, metric][0]
    seed, R = 0xC0FFEE, 5
    got = call(lib, P, k, metric, restarts=R, max_iter=100, seed=seed)
    it = int(got["iters"][got["best"]])
    tr = got["traj"][:it + 1]
    slack = N * (D + 4) * U52 * tr[0]
    assert np.all(np.isfinite(tr)) and np.all(np.diff(tr) <= slack) and np.all(np.isnan(got["traj"][it + 1:]))
    assert np.array_equal(got["sizes"], np.bincount(got["label"], minlength=k))
    assert got["best"] == int(np.argmin(got["final_inertia"])) and got["final_inertia"][got["best"]] == tr[-1]
    assert np.all(got["converged"] == 1) and np.all(got["iters"] >= 1)
    # restart r starts from the points the draw names: its first inertia is that of the call given those points as init
    start = call(lib, P, k, metric, restarts=R, max_iter=0, seed=seed)
    for r in range(R):
        pick = np.full(k, -1, dtype=np.int32)
        assert lib.insider_hip_enrichment_sample(seed, r, k, N, _lib.ptr(pick, C.c_int32)) == _lib.OK
        named = call(lib, P, k, metric, init=np.asfortranarray(P[:, pick]))
        assert named["traj"][0] == start["final_inertia"][r]
        if r == start["best"]:
            assert bits(named, ("centers", "label", "second", "dist", "dist2", "sizes")) == \
                bits(start, ("centers", "label", "second", "dist", "dist2", "sizes"))
    # the returned labels are the assignment to the returned centres
    again = call(lib, P, k, metric, init=np.asfortranarray(got["centers"]))
    assert np.array_equal(again["label"], got["label"])


# ---- 6. dead points and empty clusters --------------------------------------------------------------------------------------------
def test_dead_points_and_empty_clusters(lib):
    rng = np.random.default_rng(6)
    D, N, k = 7, 300, 6
    P = np.asfortranarray(rng.standard_normal((D, N)))
    dead = [0, 15, 16, 63, 64, 255, 256, 299]                       # the edges of a 16-tile and of a block of 64 points
    P[:, dead] = 0.0
    init = np.asfortranarray(P[:, [3, 40, 3, 100, 200, 280]] * 2.5)  # centre 2 repeats centre 0
    first = call(lib, P, k, COS, init=init)
    for max_iter in (0, 3):
        got = call(lib, P, k, COS, init=init, max_iter=max_iter)
        assert np.all(got["label"][dead] == -1) and np.all(got["second"][dead] == -1)
        assert np.all(np.isnan(got["dist"][dead])) and np.all(np.isnan(got["dist2"][dead]))
        alive = np.setdiff1d(np.arange(N), dead)
        assert np.all(got["label"][alive] >= 0) and np.all(np.isfinite(got["dist"][alive]))
        assert got["sizes"].sum() == N - len(dead) and np.array_equal(got["sizes"], np.bincount(got["label"][alive], minlength=k))
        assert got["final_inertia"][0] <= first["traj"][0] * (1 + 1e-12)
    # at the first assignment the tie rule empties the repeat; one update later it still has its (normalised) centre
    assert first["sizes"][2] == 0 and first["label"][3] == 0 and first["second"][3] == 2
    assert np.array_equal(first["centers"][:, 0], first["centers"][:, 2])
    assert np.allclose(np.sqrt((first["centers"] ** 2).sum(axis=0)), 1.0, rtol=0, atol=4 * U52)
    one = call(lib, P, k, COS, init=init, max_iter=1)
    assert np.array_equal(one["centers"][:, 2], first["centers"][:, 2])
    assert not np.array_equal(one["centers"][:, 0], first["centers"][:, 0])
    ref = host(P, k, COS, init=init, restarts=1, max_iter=0)
    assert np.array_equal(first["label"], ref["label"]) and np.array_equal(first["sizes"], ref["sizes"])
    # k = 1: no second centre
    got = call(lib, P, 1, COS, init=np.asfortranarray(P[:, 3:4]), max_iter=2)
    assert np.all(got["second"] == -1) and np.all(np.isnan(got["dist2"])) and got["sizes"][0] == N - len(dead)


# ---- 7. windows and repeats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, EUC])
def test_windows_and_repeats_are_bit_identical(lib, metric):
    rng = np.random.default_rng(77)
    D, N, k = 30, 250, 20
    P = np.asfortranarray(rng.standard_normal((D, N)))
    P[:, [5, 40, 41]] = 0.0
    init = np.asfortranarray(rng.standard_normal((D, k)))
    full = call(lib, P, k, metric, init=init)
    rows = ("label", "second", "dist", "dist2")
    for s, m in ((0, 250), (0, 33), (16, 234), (16, 100), (37, 213), (37, 64)):
        Q = np.asfortranarray(P[:, s:s + m])
        part = call(lib, Q, k, metric, init=init, pptr=window(P, s))
        assert bits(part, rows) == bits({n: full[n][s:s + m] for n in rows}, rows), (s, m)
        copy = call(lib, Q, k, metric, init=init)                               # the same window from a buffer of its own
        assert bits(copy, NAMES) == bits(part, NAMES)
    runs3 = [call(lib, P, k, metric, restarts=3, max_iter=50, seed=5) for _ in range(3)]
    assert bits(runs3[0], NAMES) == bits(runs3[1], NAMES) == bits(runs3[2], NAMES)
    assert lib.insider_hip_last_kmeans_ms() > 0.0


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(lib):
    rng = np.random.default_rng(8)
    D, N, k = 5, 40, 3
    P = np.asfortranarray(rng.standard_normal((D, N)))
    init = np.asfortranarray(rng.standard_normal((D, k)))
    bad = _lib.ERR_ARG
    for pos in (0, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20):                 # P and every output
        call(lib, P, k, COS, init=init, expect=bad, null=(pos,))
    call(lib, np.zeros((64, N), order="F") + 1.0, k, EUC, expect=bad)          # D = 64
    call(lib, P, k, COS, D=0, expect=bad)
    call(lib, P, k, COS, D=-1, expect=bad)
    call(lib, P, 0, COS, expect=bad)
    call(lib, P, 4097, EUC, expect=bad)
    call(lib, P, k, COS, N=0, expect=bad)
    call(lib, P, k, COS, N=-3, expect=bad)
    call(lib, P, k, COS, N=2 ** 31, expect=bad)                                 # (refused before P is read)
    call(lib, P, k, 2, expect=bad)
    call(lib, P, k, -1, expect=bad)
    call(lib, P, k, COS, restarts=0, expect=bad)
    call(lib, P, k, COS, restarts=257, expect=bad)
    call(lib, P, k, COS, init=init, restarts=2, expect=bad)
    call(lib, P, k, COS, max_iter=-1, expect=bad)
    call(lib, P, k, COS, max_iter=10001, expect=bad)
    for val in (np.nan, np.inf, -np.inf):
        Pn, In = P.copy(order="F"), init.copy(order="F")
        Pn[4, 39], In[0, 2] = val, val
        call(lib, Pn, k, EUC, expect=bad)
        call(lib, P, k, EUC, init=In, expect=bad)
    assert b"finite" in lib.insider_hip_last_error()
    Z = P.copy(order="F")
    Z[:, 2:] = 0.0                                                              # two alive points under cosine
    call(lib, Z, 3, COS, expect=bad)                                            # k > Na
    call(lib, Z, 3, COS, init=init, expect=bad)
    call(lib, P, N + 1, EUC, expect=bad)
    Z[:, 1] = 0.0
    call(lib, Z, 1, COS, expect=bad)                                            # a drawn start with Na < 2
    call(lib, np.ones((D, 1), order="F"), 1, EUC, expect=bad)
    In = init.copy(order="F")
    In[:, 1] = 0.0
    call(lib, P, k, COS, init=In, expect=bad)                                   # a zero-norm init column under cosine
    # what is allowed: that init under Euclidean, one alive point with init, k = Na
    assert call(lib, P, k, EUC, init=In)["sizes"].sum() == N
    assert call(lib, Z, 1, COS, init=np.asfortranarray(P[:, :1]))["sizes"][0] == 1
    assert call(lib, P, N, EUC, max_iter=2)["sizes"].sum() == N
    # the wrapper reports its own refusal, and the library's when its check is bypassed
    with pytest.raises(_lib.InsiderError) as e:
        api.kmeans(P, k, init=init, restarts=2)
    assert e.value.status == _lib.ERR_ARG


# ---- 9. users' calls -------------------------------------------------------------------------------------------------------------
def layer_equal(got, ref):
    print("yardstick: min gap", ref["min_gap"])
    assert ref["min_gap"] > 1e-9
    b = ref["best"]                                                             # (min_gap speaks of the returned restart)
    assert got["best"] == b and got["iters"][b] == ref["iters"][b] and got["converged"][b] == ref["converged"][b]
    assert np.array_equal(got["label"], ref["label"]) and np.array_equal(got["sizes"], ref["sizes"])
    assert got["label"].dtype == np.int32 and got["ms"] > 0.0


def test_gene_modules_and_sample_clusters_on_random_factors(lib):
    rng = np.random.default_rng(9)
    K, p, n, counts, m = 9, 300, 90, (4, 3), 2
    Cm = np.asfortranarray(rng.standard_normal((K, p)))
    zero = rng.random(p) < 0.3                                                  # the elastic net's all-zero columns
    Cm[:, zero] = 0.0
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    A = [rng.standard_normal((L, K)) for L in counts] + [rng.standard_normal((m, K))]
    Z = rng.standard_normal((n, m))                                             # (continuous values: no two samples are equal)
    E = posthoc.sample_embeddings(A, lev, Z)
    for metric in ("cosine", "euclidean"):
        # (seed 13: under seed 12 the Euclidean draw takes two all-zero columns as centres, an exact tie of two centres, and
        # the yardstick's own precondition fails)
        kw = dict(metric=metric, restarts=3, max_iter=100, seed=13)
        got = posthoc.gene_modules(Cm, 6, **kw)
        layer_equal(got, posthoc.kmeans_host(Cm, 6, **kw))
        assert np.array_equal(got["label"] == -1, zero if metric == "cosine" else np.zeros(p, dtype=bool))
        got = posthoc.sample_clusters(A, lev, Z, k=4, **kw)
        layer_equal(got, posthoc.kmeans_host(E, 4, **kw))
        back = posthoc.assign_to_centers(E, got["centers"], metric=metric)
        assert np.array_equal(back["label"], got["label"]) and back["iters"][0] == 0
    summary = posthoc.module_summary(posthoc.gene_modules(Cm, 6, restarts=2, seed=12), Cm)
    assert summary["mean_abs_loading"].shape == (6, K) and sum(len(g) for g in summary["members"]) == p - zero.sum()


def test_cli_writes_the_cluster_records(tmp_path):
    from insider_amd import fit as fit_cli
    rng = np.random.default_rng(10)
    n, p, K = 60, 45, 4
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    np.save(tmp_path / "X.npy", rng.standard_normal((n, p)))
    np.save(tmp_path / "L.npy", conf)
    (tmp_path / "sets.gmt").write_text("".join(f"set{s}\tna\t" + "\t".join(str(g) for g in range(5 * s, 5 * s + 10)) + "\n"
                                               for s in range(6)))
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--rank", str(K), "--lambda", "1",
                         "--alpha", "0.2", "--max-iter", "3", "--gene-modules", "5", "--sample-clusters", "3",
                         "--cluster-restarts", "2", "--cluster-iters", "20", "--gene-sets", str(tmp_path / "sets.gmt"),
                         "--enrich-min-size", "5", "--enrich-perms", "10", "--out", str(out)]) == 0
    for who, count, k, emb in (("gene", p, 5, np.load(out / "C.npy")),
                               ("sample", n, 3, posthoc.sample_embeddings([np.load(out / f"A{i}.npy") for i in range(2)], conf))):
        rec = {name: np.load(out / f"km_{who}_{name}.npy") for name in ("label", "dist", "second", "dist2", "center", "size", "traj")}
        assert rec["label"].shape == rec["second"].shape == rec["dist"].shape == rec["dist2"].shape == (count,)
        assert rec["label"].dtype == rec["size"].dtype == np.int32 and rec["center"].shape == (K, k) and rec["traj"].shape == (21,)
        alive = rec["label"] >= 0
        assert np.array_equal(rec["size"], np.bincount(rec["label"][alive], minlength=k))
        back = posthoc.assign_to_centers(emb, rec["center"], metric="cosine")
        assert np.array_equal(back["label"], rec["label"])
    assert np.load(out / "km_gene_overlap.npy").shape == np.load(out / "km_gene_hyper_p.npy").shape == (5, 6)
    assert np.load(out / "km_gene_hyper_fdr.npy").shape == (5, 6)
