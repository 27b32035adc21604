"""insider_hip_gram_topk_pairwise and insider_hip_coexpression_pairwise on the device against the numpy yardsticks
posthoc.gram_topk_pairwise_host() and coexpression_host(missing="pairwise").

Every call goes through ctypes with outputs prefilled with sentinels and NGUARD guard elements past rows * k; the guards must
be unchanged after every call, and after a refused call the whole output is.

The tolerance is derived, not fitted.  With u = 2^-53 and D the depth, a pair's score is cov / sqrt(va vb) with
cov = Sab - Sa Sb / N, va = Saa - Sa Sa / N, vb = Sbb - Sb Sb / N, every S a D-term sum of products in some order.  A D-term
sum of products errs by at most D u times the sum of the absolute products to first order; the product Sa Sb, the quotient
by the exact N and the difference add one u each, so each of cov, va and vb errs by at most (3 D + 3) u times its uncentred
counterpart: sqrt(Saa Sbb) >= |Sab|, |Sa Sb| / N for cov (Cauchy-Schwarz), Saa for va, Sbb for vb.  Relative to the centred
quantities that is (3 D + 3) u kappa with kappa_a = Saa / va, kappa_b = Sbb / vb, and for cov, relative to sqrt(va vb),
(3 D + 3) u sqrt(kappa_a kappa_b) <= (3 D + 3) u (kappa_a + kappa_b) / 2.  With |score| <= 1 the quotient moves by the error
of cov plus half that of va plus half that of vb: at most (3 D + 3) u (kappa_a + kappa_b), and the root, the product va vb and
the last quotient add 3 u.  The vectors are first standardised over their own entries; the score is invariant under that
affine map, so the 2 u per element of the map (a subtraction and a quotient, the same mean and norm for the whole vector up
to their own rounding, which is again an affine map) only adds 2 u to every product, inside the 3 D + 16 below.  The device
and the yardstick together:
    T = 4 (3 D + 16) 2^-52 (kappa_a + kappa_b),
kappa = Saa / va taken from the reference on the standardised values (tests/test_coexpression_pairwise_cpu.py: reference()).
The same formula evaluated in another summation order stayed below 0.002 T on the CPU, vector means of 10^4 standard
deviations and 60 % missing included.  Every test asserts on its reference that no eligible pair has kappa >= 10^6 and that
every pair ineligible by variance is constant by construction, so no pair is near the floor 16 (D + 8) 2^-52."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc, workloads
from tests.support import SAMPLES_3_5_7_GENES_1_3, bits, factors, lib, masks, need_gpu, planted, resident  # noqa: F401
from tests.test_coexpression_pairwise_cpu import reference, vectors
from tests.test_gpu_neighbors import check_rule3

pytestmark = pytest.mark.gpu

NGUARD = 7
IDX_SENTINEL = -77
SCORE_SENTINEL = 12345.678
OUT = ("index", "score", "overlap")
QB = api.CX_QB


def outputs(rows, k):
    size = rows * max(k, 1) + NGUARD
    return (np.full(size, IDX_SENTINEL, dtype=np.int32), np.full(size, SCORE_SENTINEL), np.full(size, IDX_SENTINEL, dtype=np.int32))


def finish(lib, status, expect, rows, k, idx, sc, ov):
    assert status == expect, (status, lib.insider_hip_last_error().decode(errors="replace"))
    used = rows * k if status == _lib.OK else 0
    assert np.all(idx[used:] == IDX_SENTINEL) and np.all(sc[used:] == SCORE_SENTINEL) and np.all(ov[used:] == IDX_SENTINEL)
    if status != _lib.OK:
        assert lib.insider_hip_last_error() != b""
        return None
    return dict(index=idx[:used].reshape(rows, k), score=sc[:used].reshape(rows, k), overlap=ov[:used].reshape(rows, k))


def call(lib, V, k, min_overlap=3, first=0, count=None, depth=None, N=None, expect=_lib.OK, null=()):
    """One guarded call of the handle-free form.  V: column-major depth x N, NaN = missing."""
    d_, n_ = V.shape
    depth = d_ if depth is None else depth
    N = n_ if N is None else N
    count = n_ - first if count is None else count
    rows = max(count, 0) if count <= n_ else n_
    idx, sc, ov = outputs(rows, k)
    args = [_lib.ptr(V), depth, N, min_overlap, k, first, count, 0, _lib.ptr(idx, C.c_int32), _lib.ptr(sc), _lib.ptr(ov, C.c_int32)]
    for pos in null:
        args[pos] = None
    return finish(lib, lib.insider_hip_gram_topk_pairwise(*args), expect, rows, k, idx, sc, ov)


def call_resident(lib, ds, A, Cm, axis, k, min_overlap, entries, expect=_lib.OK, null=(), inc=0):
    """One guarded call of the handle form."""
    K = Cm.shape[0]
    _, Cw, Aptrs = ds._marshal(A, Cm, K, inc)
    rows = ds.p if axis == "genes" else ds.n
    idx, sc, ov = outputs(rows, k)
    args = [ds._h, Aptrs, _lib.ptr(Cw), inc, K, ds.VD_ENTRIES[entries], None, None, ds.COEXPR_AXES[axis], min_overlap, k,
            _lib.ptr(idx, C.c_int32), _lib.ptr(sc), _lib.ptr(ov, C.c_int32)]
    for pos in null:
        args[pos] = None
    return finish(lib, lib.insider_hip_coexpression_pairwise(*args), expect, rows, k, idx, sc, ov)


def planted_constant(V):
    """Vector 5 constant on the first half of the depth and varying on the second, vector 6 missing on the second half: the
    pair is constant on its joint entries by construction (where the shape has room for it)."""
    depth, N = V.shape
    if depth < 8 or N < 7:
        return V
    h = depth // 2
    rng = np.random.default_rng(depth + N)
    V[:h, 5], V[h:, 5] = 0.75, rng.standard_normal(depth - h)
    V[:h, 6], V[h:, 6] = rng.standard_normal(h), np.nan
    return V


def checked_reference(V, min_overlap):
    """reference() of V with NaN = missing, after the two assertions that keep every pair away from the floor."""
    sel = ~np.isnan(V)
    S, T, elig, Nn, ka, kb = reference(np.where(sel, V, 0.0), sel, min_overlap)
    assert np.all(ka[elig] < 1e6) and np.all(kb[elig] < 1e6) and np.all(np.isfinite(T[elig]))
    alive = posthoc._gram_standardise(np.where(sel, V, 0.0), sel, 0)[1]
    by_variance = alive[:, None] & alive[None, :] & ~np.eye(V.shape[1], dtype=bool) & (Nn >= min_overlap) & ~elig
    for a, b in zip(*np.nonzero(by_variance)):
        J = sel[:, a] & sel[:, b]
        assert np.ptp(V[J, a]) == 0.0 or np.ptp(V[J, b]) == 0.0, (a, b)
    return S, T, elig, Nn


def check(got, S, T, elig, Nn, k):
    check_rule3(got, S, T, k, elig)
    slot = got["index"] >= 0
    rows = np.arange(S.shape[0])[:, None]
    assert got["overlap"].dtype == np.int32 and np.all(got["overlap"][~slot] == -1)
    assert np.array_equal(got["overlap"][slot], Nn[rows, np.where(slot, got["index"], 0)][slot])


# ---- 1. against the yardstick -------------------------------------------------------------------------------------------------
SHAPES = [(33, N) for N in (1, 2, 15, 16, 17, 63, 64, 65, 129)] + [(d, 65) for d in (1, 3, 31, 32, 65)]


@pytest.mark.parametrize("missing", [0.0, 0.3])
@pytest.mark.parametrize("shape", SHAPES)
def test_scores_and_overlaps_match_the_yardstick(lib, shape, missing):
    depth, N = shape
    V = vectors(depth, N, missing, 13 * depth + N)
    if missing:
        V = planted_constant(V)
    S, T, elig, Nn = checked_reference(V, 3)
    for k in (1, 10, 64):
        check(call(lib, V, k), S, T, elig, Nn, k)
    if missing and depth >= 8 and N >= 7:
        assert not elig[5, 6] and Nn[5, 6] == depth // 2                   # the planted pair: alive, overlapping, constant
    host = posthoc.gram_topk_pairwise_host(V, k=10, min_overlap=3)
    assert np.array_equal(call(lib, V, 10)["index"] < 0, host["index"] < 0)


# ---- 2. padding -----------------------------------------------------------------------------------------------------------------
def test_padded_positions_are_unselected(lib):
    """depth 35 (padded to 64) and N = 21 (padded to 64): vector 0's entries are all selected and 0 beyond its first three,
    as the padding was under the zero-filled form.  No pair gains overlap from the padded depth, nobody pairs with a padded
    vector."""
    depth, N, k = 35, 21, 20
    V = vectors(depth, N, 0.3, 77)
    V[:, 0] = 0.0
    V[:3, 0] = (1.0, -2.0, 0.5)
    V[:, 1] = np.random.default_rng(1).standard_normal(depth)              # a full partner: overlap exactly the depth
    S, T, elig, Nn = checked_reference(V, 3)
    got = call(lib, V, k)
    check(got, S, T, elig, Nn, k)
    assert Nn.max() == depth and got["overlap"].max() == depth and got["index"].max() < N
    assert got["overlap"][0][list(got["index"][0]).index(1)] == depth
    assert np.array_equal(np.sort(got["overlap"][0][got["index"][0] >= 0]), np.sort(Nn[0][elig[0]]))


# ---- 3. symmetry and determinism ---------------------------------------------------------------------------------------------------
def test_symmetric_bits_windows_and_repeats(lib):
    depth, N, k = 40, QB + 1, 64                                           # k >= N - 1: every eligible pair is listed
    V = planted_constant(vectors(depth, N, 0.3, 31))
    got = call(lib, V, k)
    sc = np.full((N, N), np.nan)
    ov = np.full((N, N), -1, dtype=np.int64)
    rows = np.repeat(np.arange(N), k)[(got["index"] >= 0).ravel()]
    cols = got["index"][got["index"] >= 0]
    sc[rows, cols] = got["score"][got["index"] >= 0]
    ov[rows, cols] = got["overlap"][got["index"] >= 0]
    assert rows.size > N and sc.tobytes() == sc.T.copy().tobytes() and np.array_equal(ov, ov.T)
    depth, N, k = 70, 2 * QB + 2, 10
    V = vectors(depth, N, 0.3, 55)
    full = call(lib, V, k)
    assert bits(full, OUT) == bits(call(lib, V, k), OUT)
    for s, m in ((0, 1), (0, 16), (15, 2), (1, 16), (QB - 1, 2), (QB, QB), (2 * QB - 3, 5), (N - 17, 17), (N - 1, 1)):
        part = call(lib, V, k, first=s, count=m)
        assert bits(part, OUT) == bits({n: full[n][s:s + m] for n in OUT}, OUT), (s, m)


# ---- 4. it is a different answer ------------------------------------------------------------------------------------------------
def test_differs_from_the_zero_filled_call_and_agrees_without_missing(lib):
    from tests.test_gpu_gram_topk import COR, call as call_zero, reference_scores
    rng = np.random.default_rng(9)
    depth, N, k = 37, 40, 10
    full = np.asfortranarray(rng.standard_normal((depth, 4)) @ rng.standard_normal((4, N)) + rng.standard_normal((depth, N)))
    V = full.copy(order="F")
    V[rng.random(V.shape) < 0.3] = np.nan
    S, T, elig, Nn = checked_reference(V, 3)
    pc = call(lib, V, k)
    check(pc, S, T, elig, Nn, k)
    zero = call_zero(lib, np.asfortranarray(np.where(np.isnan(V), 0.0, V)), k, COR)
    assert np.any(np.any(pc["index"] != zero["index"], axis=1))
    # nothing missing: one reference for both calls.  Its scores err by half the zero-filled call's tolerance, the pairwise
    # call by half its own, so the pairwise call is held to the larger of the two.
    Sz, Tz, eligz = reference_scores(full, COR)
    _, Tp, eligp, Nn = checked_reference(full, 3)
    assert np.array_equal(eligz, eligp)
    check_rule3(call_zero(lib, full, k, COR), Sz, Tz, k, eligz)
    check(call(lib, full, k), Sz, np.maximum(Tz, Tp), eligz, Nn, k)


# ---- 5. the resident form ---------------------------------------------------------------------------------------------------------
COUNTS = (5, 3)
N_, P_ = 37, 130
_DATA = {}


def data():
    """The planted data set and its resident handle, made once and left unchanged."""
    if not _DATA:
        d = planted(N_, P_, COUNTS, 0, seed=N_ + P_, empty=SAMPLES_3_5_7_GENES_1_3)
        _DATA[0] = (resident(*d),) + d
    return _DATA[0]


@pytest.fixture(scope="module", autouse=True)
def close_data():
    yield
    for d in _DATA.values():
        d[0].close()
    _DATA.clear()


def resident_reference(X, lev, Z, mask, A, Cm, axis, min_overlap):
    r, w = posthoc.coexpression_residual_host(X, lev, Z, mask, A, Cm)
    if axis == "samples":
        r, w = r.T, w.T
    return checked_reference(np.where(w, r, np.nan), min_overlap)


@pytest.mark.parametrize("K", [3, 17])
def test_resident_form_matches_host(lib, K):
    ds, X, lev, Z, mk = data()
    A, Cm = factors(np.random.default_rng(100 + K), COUNTS, 0, K, P_)
    k = 10
    for entries in ("train", "all"):
        for axis in ("genes", "samples"):
            depth = N_ if axis == "genes" else P_
            mo = api.pairwise_min_overlap(None, depth)
            S, T, elig, Nn = resident_reference(X, lev, Z, mk[entries], A, Cm, axis, mo)
            got = call_resident(lib, ds, A, Cm, axis, k, mo, entries)
            check(got, S, T, elig, Nn, k)
            host = posthoc.coexpression_host(X, lev, Z, mk[entries], A, Cm, axis, k, missing="pairwise")
            assert np.array_equal(got["index"] < 0, host["index"] < 0)
            py = ds.coexpression_pairwise(A, Cm, axis=axis, k=k, entries=entries)
            assert py["overlap"].dtype == np.int32 and bits(py, OUT) == bits(got, OUT)
            if axis == "genes" and entries == "train":
                assert np.all(got["index"][1] == -1) and not np.isin(got["index"], 1).any()     # gene 1 has no train entry
            if axis == "samples" and entries != "all":
                assert np.all(got["index"][7] == -1) and not np.isin(got["index"], 7).any()     # sample 7 is all NA
            assert ds.info("cx_form") == (K + 15) // 16
            assert ds.info("cx_stage_mb") > 0 and ds.info("cx_stage_ms") >= 0 and ds.info("cx_pc_ms") >= 0


def test_resident_clones_remasks_and_k64(lib):
    ds, X, lev, Z, mk = data()
    K, k = 3, 10
    A, Cm = factors(np.random.default_rng(21), COUNTS, 0, K, P_)
    tr2, te2 = masks(np.random.default_rng(77), N_, P_, SAMPLES_3_5_7_GENES_1_3)
    pair = [np.asfortranarray(v, dtype=np.uint8) for v in (tr2, te2)]
    cl, rm, fresh = ds.clone(), ds.remask(*pair), api.InsiderData(X, lev, *pair)
    try:
        for axis in ("genes", "samples"):
            mo = api.pairwise_min_overlap(None, N_ if axis == "genes" else P_)
            a = call_resident(lib, ds, A, Cm, axis, k, mo, "train")
            assert bits(a, OUT) == bits(call_resident(lib, ds, A, Cm, axis, k, mo, "train"), OUT)
            assert bits(a, OUT) == bits(call_resident(lib, cl, A, Cm, axis, k, mo, "train"), OUT)
            b = call_resident(lib, rm, A, Cm, axis, k, mo, "train")
            assert bits(b, OUT) == bits(call_resident(lib, fresh, A, Cm, axis, k, mo, "train"), OUT)
            S, T, elig, Nn = resident_reference(X, lev, Z, tr2, A, Cm, axis, mo)
            check(b, S, T, elig, Nn, k)
            big = call_resident(lib, ds, A, Cm, axis, 64, mo, "train")                         # k = 64: above 64 KB of LDS
            assert bits({n: big[n][:, :k] for n in OUT}, OUT) == bits(a, OUT)
    finally:
        for h in (cl, rm, fresh):
            h.close()


def test_resident_form_refuses_bad_arguments(lib):
    ds, X, lev, Z, mk = data()
    A, Cm = factors(np.random.default_rng(17), COUNTS, 0, 4, P_)
    bad = _lib.ERR_ARG
    for pos in (11, 12, 13):                                                 # idx_out, score_out, overlap_out
        call_resident(lib, ds, A, Cm, "genes", 3, 5, "train", expect=bad, null=(pos,))
    for mo in (2, 0, -1):
        call_resident(lib, ds, A, Cm, "genes", 3, mo, "train", expect=bad)
    for k in (0, 65):
        call_resident(lib, ds, A, Cm, "genes", k, 5, "train", expect=bad)
    assert call_resident(lib, ds, A, Cm, "genes", 3, N_ + 1, "train")["index"].max() == -1     # allowed: every row open

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.coexpression_pairwise(A, Cm, entries="held-out")) == bad
    assert status(lambda: ds.coexpression_pairwise(A, Cm, axis="columns")) == bad
    assert status(lambda: ds.coexpression_pairwise(A, Cm, k=65)) == bad
    assert status(lambda: ds.coexpression_pairwise(A, Cm, min_overlap=2)) == bad


def test_refuses_a_sharded_handle(lib):
    w = workloads.small(n=48, p=64, K=3)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        ds.set_shard(0, 0, 2, allreduce=lambda ptr, count, stream: None)
        with pytest.raises(_lib.InsiderError) as e:
            ds.coexpression_pairwise(w.A0, w.C0)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        call_resident(lib, ds, w.A0, w.C0, "genes", 2, 5, "train", expect=_lib.ERR_UNSUPPORTED)
    finally:
        ds.close()


def test_leaves_optimize_bit_identical(lib):
    w = workloads.small(n=90, p=140, K=6)

    def run(with_calls):
        ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
        try:
            r1 = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha, tuning=1,
                             max_iter=12, seed=3)
            A = [a.copy(order="F") for a in r1["row_matrices"].values()]
            Cm = r1["column_factor"].copy(order="F")
            if with_calls:
                for e in ("train", "all"):
                    for axis in ("genes", "samples"):
                        ds.coexpression_pairwise(A, Cm, axis=axis, entries=e)
                with pytest.raises(_lib.InsiderError):
                    ds.coexpression_pairwise(A, Cm, min_overlap=1)
            return ds.optimize(A, Cm, w.K, w.lam, w.lam, w.alpha, tuning=1, max_iter=12, seed=3)
        finally:
            ds.close()

    ref, got = run(False), run(True)
    for a, b in zip(ref["row_matrices"].values(), got["row_matrices"].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(ref["column_factor"], got["column_factor"])
    assert np.array_equal(ref["traj"], got["traj"], equal_nan=True)


def test_fitted_object_and_command_line(lib, tmp_path):
    """posthoc.gene_coexpression() / sample_coexpression() with missing="pairwise" on a fitted object whose data has NA
    entries, and the command line's --coexpression-missing pairwise: the six cx_* records."""
    from tests.support import close_resident
    rng = np.random.default_rng(8)
    n, p, k = 40, 60, 5
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    X = rng.standard_normal((n, p)) + 2.0 * np.outer(rng.standard_normal(n), rng.standard_normal(p))
    X[rng.random(X.shape) < 0.2] = np.nan
    obj = api.insider(X, conf)
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=3, lambda_=1.0, alpha=0.2)
    try:
        A, Cm = list(obj["cfd_matrices"].values()), obj["column_factor"]
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        assert np.array_equal(mask, ~np.isnan(X))
        lev, X0 = np.asarray(obj["confounder"]), np.where(mask, X, 0.0)
        zero = posthoc.gene_coexpression(obj, k=k)
        assert set(zero) == {"index", "score"}                              # the default is the zero-filled call
        g = posthoc.gene_coexpression(obj, k=k, missing="pairwise")
        S, T, elig, Nn = resident_reference(X0, lev, None, mask, A, Cm, "genes", api.pairwise_min_overlap(None, n))
        check(g, S, T, elig, Nn, k)
        assert 0 <= g["overlap"].max() < n
        s = posthoc.sample_coexpression(obj, k=k, standardize=False, missing="pairwise", min_overlap=20)
        S, T, elig, Nn = resident_reference(X0, lev, None, mask, A, Cm, "samples", 20)
        check(s, S, T, elig, Nn, k)
        assert s["center"] is None and s["overlap"][s["index"] >= 0].min() >= 20
    finally:
        close_resident(obj)
    from insider_amd import fit as fit_cli
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "L.npy", conf)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--rank", "3", "--lambda", "1",
                         "--alpha", "0.2", "--max-iter", "3", "--gene-coexpression", str(k), "--sample-coexpression", str(k),
                         "--coexpression-missing", "pairwise", "--coexpression-min-overlap", "12", "--out", str(out)]) == 0
    Cm = np.load(out / "C.npy")
    A = [np.load(out / f"A{i}.npy") for i in range(2)]
    gi, gs, go = (np.load(out / f"cx_gene_{name}.npy") for name in OUT)
    si, ss, so = (np.load(out / f"cx_sample_{name}.npy") for name in OUT)
    assert gi.shape == gs.shape == go.shape == (p, k) and si.shape == ss.shape == so.shape == (n, k)
    assert gi.dtype == go.dtype == si.dtype == so.dtype == np.int32 and gs.dtype == ss.dtype == np.float64
    S, T, elig, Nn = resident_reference(np.where(np.isnan(X), 0.0, X), conf, None, ~np.isnan(X), A, Cm, "genes", 12)
    check(dict(index=gi, score=gs, overlap=go), S, T, elig, Nn, k)
    assert go.max() < n and so[si >= 0].min() >= 12


# ---- 6. refused arguments ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(lib):
    rng = np.random.default_rng(6)
    V = np.asfortranarray(rng.standard_normal((5, 20)))
    bad = _lib.ERR_ARG
    for pos in (0, 8, 9, 10):                                                # V, idx_out, score_out, overlap_out
        call(lib, V, 3, expect=bad, null=(pos,))
    for mo in (2, 0, -1):
        call(lib, V, 3, min_overlap=mo, expect=bad)
    assert b"min_overlap" in lib.insider_hip_last_error()
    call(lib, V, 0, expect=bad)
    call(lib, V, 65, expect=bad)
    call(lib, V, 3, depth=0, expect=bad)
    call(lib, V, 3, N=0, count=0, expect=bad)
    call(lib, V, 3, N=2 ** 31, expect=bad)                                   # (refused before V is read)
    call(lib, V, 3, first=-1, count=2, expect=bad)
    call(lib, V, 3, first=0, count=-1, expect=bad)
    call(lib, V, 3, first=17, count=4, expect=bad)                           # 17 + 4 > 20
    call(lib, V, 3, first=21, count=0, expect=bad)
    for val in (np.inf, -np.inf):
        Vn = V.copy(order="F")
        Vn[4, 19] = val
        call(lib, Vn, 3, expect=bad)
    assert b"finite" in lib.insider_hip_last_error()
    # what is allowed: a NaN (a missing entry); min_overlap above the depth (every slot open); an empty window
    Vn = V.copy(order="F")
    Vn[4, 19] = np.nan
    S, T, elig, Nn = checked_reference(Vn, 3)
    check(call(lib, Vn, 3), S, T, elig, Nn, 3)
    none = call(lib, V, 3, min_overlap=6)
    assert np.all(none["index"] == -1) and np.all(np.isnan(none["score"])) and np.all(none["overlap"] == -1)
    assert call(lib, V, 3, first=16, count=4)["index"].shape == (4, 3)
    assert call(lib, V, 3, first=20, count=0)["index"].shape == (0, 3)
    assert call(lib, V, 3, first=0, count=0)["index"].shape == (0, 3)
    # the wrapper answers like the guarded call
    got = api.gram_topk_pairwise(Vn, k=3, first=16)
    assert got["index"].dtype == got["overlap"].dtype == np.int32
    assert bits(got, OUT) == bits(call(lib, Vn, 3, first=16, count=4), OUT)
    assert lib.insider_hip_last_gram_topk_ms() >= 0.0


# ---- 7. the contract on the built library ---------------------------------------------------------------------------------------
def test_contract_on_the_built_library(lib):
    for name in ("insider_hip_gram_topk_pairwise", "insider_hip_coexpression_pairwise"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert len(lib.insider_hip_gram_topk_pairwise.argtypes) == 11
    assert len(lib.insider_hip_coexpression_pairwise.argtypes) == 14
    assert len(lib.insider_hip_gram_topk.argtypes) == 10 and len(lib.insider_hip_coexpression.argtypes) == 12
