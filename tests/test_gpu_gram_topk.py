"""insider_hip_gram_topk on the device against the numpy yardstick posthoc.gram_topk_host().

Every call goes through ctypes with outputs prefilled with sentinels and NGUARD guard elements past count * k; the guards
must be unchanged after every call, and after a refused call the whole output is.

Where the arithmetic is exact (integer entries, metric dot: every score is exact in fp64 whatever the summation order)
indices and scores must EQUAL the yardstick's.

The tolerance of the real-valued tests is derived, not fitted.  With u = 2^-53 a D-term fp64 dot in any order errs by at
most D u |a| |b| to first order.  Under cosine the two vectors are first divided by their norms, each known to a few u, so
the score (|a| = |b| = 1) errs by (D + a few) u.  Under correlation each vector is centred first: the computed mean errs by
at most D u mean|v| (a D-term sum divided by D), so every centred element errs by that much and the centred vector by
sqrt(D) D u mean|v| in norm, which relative to its own norm |v - mean| is D u kappa with
    kappa = sqrt(D) mean|v| / |v - mean|
(a vector with mean / sd = 3 has kappa of about 3).  A relative perturbation e of one side moves the normalised score by at
most 2 e (once through the numerator, once through the norm).  Hence
    tol = 4 (D + 8) 2^-52 (1 + 2 kappa_a + 2 kappa_b)     correlation,
    tol = 4 (D + 8) 2^-52                                 cosine,
    tol = 4 (D + 8) 2^-52 |a| |b|                         dot,
kappa taken from the reference; the leading 4 = 2 x 2 turns u into 2^-52 and covers the device and the yardstick together,
the 8 the handful of roundings of the normalisation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from insider_amd import _build, _lib, api, posthoc
from tests.support import bits, lib  # noqa: F401  (lib: fixture)
from tests.test_gpu_neighbors import check_rule3

pytestmark = pytest.mark.gpu

NGUARD = 7
IDX_SENTINEL = -77
SCORE_SENTINEL = 12345.678
COR, COS, DOT = 0, 1, 2
METRIC = {COR: "correlation", COS: "cosine", DOT: "dot"}
OUT = ("index", "score")
DC, QB, BG = api.CX_DC, api.CX_QB, api.CX_BG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call(lib, V, k, metric, first=0, count=None, depth=None, N=None, expect=_lib.OK, null=()):
    """One guarded call.  V: column-major depth x N."""
    d_, n_ = V.shape
    depth = d_ if depth is None else depth
    N = n_ if N is None else N
    count = n_ - first if count is None else count
    rows = max(count, 0) if count <= n_ else n_
    idx = np.full(rows * max(k, 1) + NGUARD, IDX_SENTINEL, dtype=np.int32)
    sc = np.full(rows * max(k, 1) + NGUARD, SCORE_SENTINEL)
    args = [_lib.ptr(V), depth, N, metric, k, first, count, 0, _lib.ptr(idx, C.c_int32), _lib.ptr(sc)]
    for pos in null:
        args[pos] = None
    status = lib.insider_hip_gram_topk(*args)
    assert status == expect, (status, lib.insider_hip_last_error().decode(errors="replace"))
    used = rows * k if status == _lib.OK else 0
    assert np.all(idx[used:] == IDX_SENTINEL) and np.all(sc[used:] == SCORE_SENTINEL)
    if status != _lib.OK:
        return None
    return dict(index=idx[:used].reshape(rows, k), score=sc[:used].reshape(rows, k))


def equal(got, ref):
    assert np.array_equal(got["index"], ref["index"])
    assert np.array_equal(got["score"], ref["score"], equal_nan=True)


def sizes():
    """N at the edges of a tile, of a query group and of a base group."""
    return sorted({1, 2, 15, 16, 17, QB - 1, QB, QB + 1, 2 * QB + 1, BG - 1, BG, BG + 1, 2 * BG + 1})


# ---- 1. exact arithmetic, dot metric --------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 3, 4, 5, DC - 1, DC, DC + 1, 2 * DC + 1])
def test_exact_integers_equal_the_yardstick(lib, depth):
    """Entries in -2..2: ties everywhere, so this is the test of the tie rule and of self-exclusion."""
    rng = np.random.default_rng(100 + depth)
    for N in sizes():
        V = np.asfortranarray(rng.integers(-2, 3, (depth, N)).astype(np.float64))
        for k in (1, 10, 64):
            equal(call(lib, V, k, DOT), posthoc.gram_topk_host(V, k=k, metric="dot"))


# ---- 2. adversarial order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64])
def test_adversarial_orders_are_exact(lib, k):
    """Depth DC + 1 (two chunks; the last row is a constant 1), 5000 vectors (j + 1) e_1 and the 40 queries from 1000 on,
    which are positive: ascending, every candidate beats the threshold, so each query's buffer of 32 slots fills after two
    base tiles and is merged about 150 times; descending: none does after the first k; all vectors equal: the tie rule
    alone decides."""
    depth, N, first, count = DC + 1, 5000, 1000, 40
    up = np.zeros((depth, N), order="F")
    up[0] = np.arange(1, N + 1)
    up[DC] = 1.0
    down = np.asfortranarray(up[:, ::-1])
    flat = np.zeros((depth, N), order="F")
    flat[0] = 3.0
    flat[DC] = 1.0
    for V in (up, down, flat):
        got = call(lib, V, k, DOT, first, count)
        equal(got, posthoc.gram_topk_host(V, k=k, metric="dot", first=first, count=count))
    assert np.array_equal(got["index"], np.tile(np.arange(k, dtype=np.int32), (count, 1)))
    got = call(lib, up, k, DOT, first, count)
    assert np.array_equal(got["index"][0], np.arange(N - 1, N - 1 - k, -1))


# ---- 3. real-valued inputs ------------------------------------------------------------------------------------------------
def real_inputs(depth, N, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((depth, N))
    V[:, rng.random(N) < 0.1] *= 1e-3
    V[:, rng.random(N) < 0.1] *= 1e3
    shifted = rng.random(N) < 0.2
    V[:, shifted] += 3.0 * V[:, shifted].std(axis=0)                 # mean / sd about 3
    return np.asfortranarray(V)


def reference_scores(V, metric):
    """The float64 score of every pair, its tolerance (N x N each) and who may be whose partner."""
    depth, N = V.shape
    W, alive = posthoc._gram_standardise(V, None, metric)
    S = W.T @ W
    eps = 4.0 * (depth + 8) * 2.0 ** -52
    if metric == COR:
        cen = V - V.mean(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            kappa = np.where(alive, np.sqrt(depth) * np.abs(V).mean(axis=0) / np.sqrt((cen * cen).sum(axis=0)), 0.0)
        T = eps * (1.0 + 2.0 * kappa[:, None] + 2.0 * kappa[None, :])
    elif metric == COS:
        T = np.full(S.shape, eps)
    else:
        nrm = np.sqrt((V * V).sum(axis=0))
        T = eps * nrm[:, None] * nrm[None, :]
    elig = alive[:, None] & alive[None, :] & ~np.eye(N, dtype=bool)
    return S, T, elig


@pytest.mark.parametrize("metric", [COR, COS, DOT])
@pytest.mark.parametrize("shape", [(37, 700), (300, 250), (1000, 130)])
def test_real_inputs_within_the_derived_bound(lib, metric, shape):
    depth, N = shape
    V = real_inputs(depth, N, 7 * depth + N)
    S, T, elig = reference_scores(V, metric)
    for k in (1, 10, 64):
        check_rule3(call(lib, V, k, metric), S, T, k, elig)


# ---- 4. open slots ----------------------------------------------------------------------------------------------------------
def test_open_slots(lib):
    rng = np.random.default_rng(4)
    # N - 1 < k: the head is right, the tail open
    V = np.asfortranarray(rng.integers(-2, 3, (6, 9)).astype(np.float64))
    got = call(lib, V, 12, DOT)
    equal(got, posthoc.gram_topk_host(V, k=12, metric="dot"))
    assert np.all(got["index"][:, :8] >= 0) and np.all(got["index"][:, 8:] == -1) and np.all(np.isnan(got["score"][:, 8:]))
    got = call(lib, V[:, :1].copy(order="F"), 3, DOT)                      # one vector: no partner at all
    assert np.all(got["index"] == -1) and np.all(np.isnan(got["score"]))
    # dead vectors: zero (both metrics) and constant (correlation only); fewer alive partners than k
    depth, N, k = 40, 70, 10
    V = np.zeros((depth, N), order="F")
    live = (3, 17, 18, 39, 64, 69)
    for j in live:
        V[:, j] = rng.standard_normal(depth)
    V[:, 5] = 2.5
    for metric in (COR, COS):
        S, T, elig = reference_scores(V, metric)
        got = call(lib, V, k, metric)
        check_rule3(got, S, T, k, elig)
        alive = sorted(live if metric == COR else live + (5,))
        dead = [j for j in range(N) if j not in alive]
        assert np.all(got["index"][dead] == -1) and np.all(np.isnan(got["score"][dead])) and not np.isin(got["index"], dead).any()
        assert np.all(np.sort(got["index"][list(alive), :len(alive) - 1], axis=1) ==
                      np.array([[j for j in alive if j != i] for i in alive]))
    Vi = np.asfortranarray(np.round(V * 4))
    equal(call(lib, Vi, k, DOT), posthoc.gram_topk_host(Vi, k=k, metric="dot"))   # under dot nothing is dead
    # an all-dead matrix
    for metric, W in ((COR, np.full((5, 20), 7.0, order="F")), (COS, np.zeros((5, 20), order="F"))):
        got = call(lib, W, 4, metric)
        assert np.all(got["index"] == -1) and np.all(np.isnan(got["score"]))


# ---- 5. window invariance and repeatability -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COR, COS, DOT])
def test_windows_and_repeats_are_bit_identical(lib, metric):
    depth, N, k = 70, 250, 10
    V = real_inputs(depth, N, 55)
    full = call(lib, V, k, metric)
    again = call(lib, V, k, metric)
    assert bits(full, OUT) == bits(again, OUT)
    for s, m in ((0, 1), (1, 16), (7, 33), (N - 17, 17)):
        part = call(lib, V, k, metric, s, m)
        assert bits(part, OUT) == bits(dict(index=full["index"][s:s + m], score=full["score"][s:s + m]), OUT), (s, m)


# ---- 6. C-ABI errors ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(lib):
    rng = np.random.default_rng(6)
    V = np.asfortranarray(rng.standard_normal((5, 20)))
    bad = _lib.ERR_ARG
    for pos in (0, 8, 9):                                                    # V, idx_out, score_out
        call(lib, V, 3, COS, expect=bad, null=(pos,))
    call(lib, V, 3, COS, depth=0, expect=bad)
    call(lib, V, 3, COS, depth=-1, expect=bad)
    call(lib, V, 3, COS, N=0, count=0, expect=bad)
    call(lib, V, 3, COS, N=-5, count=0, expect=bad)
    call(lib, V, 3, COS, N=2 ** 31, expect=bad)                              # (refused before V is read)
    call(lib, V, 0, COS, expect=bad)
    call(lib, V, 65, COS, expect=bad)
    call(lib, V, 3, 3, expect=bad)
    call(lib, V, 3, -1, expect=bad)
    call(lib, V, 3, COS, first=-1, count=2, expect=bad)
    call(lib, V, 3, COS, first=0, count=-1, expect=bad)
    call(lib, V, 3, COS, first=17, count=4, expect=bad)                      # 17 + 4 > 20
    call(lib, V, 3, COS, first=21, count=0, expect=bad)
    for val in (np.nan, np.inf, -np.inf):
        Vn = V.copy(order="F")
        Vn[4, 19] = val
        call(lib, Vn, 3, DOT, expect=bad)
    assert b"finite" in lib.insider_hip_last_error()
    # what is allowed: the last window; an empty window (OK, nothing written)
    assert call(lib, V, 3, COS, first=16, count=4)["index"].shape == (4, 3)
    assert call(lib, V, 3, COS, first=20, count=0)["index"].shape == (0, 3)
    assert call(lib, V, 3, COS, first=0, count=0)["index"].shape == (0, 3)
    # the wrapper refuses before the library is touched, and answers like the guarded call
    Vn = V.copy(order="F")
    Vn[0, 0] = np.nan
    with pytest.raises(_lib.InsiderError) as e:
        api.gram_topk(Vn, k=3)
    assert e.value.status == _lib.ERR_ARG
    got = api.gram_topk(V, k=3, metric="cosine", first=16)
    assert got["index"].dtype == np.int32 and bits(got, OUT) == bits(call(lib, V, 3, COS, first=16, count=4), OUT)
    assert lib.insider_hip_last_gram_topk_ms() >= 0.0


# ---- 7. the contract on the built library ------------------------------------------------------------------------------------
def test_contract_on_the_built_library(lib):
    for name in ("insider_hip_gram_topk", "insider_hip_last_gram_topk_ms", "insider_hip_coexpression"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert len(lib.insider_hip_gram_topk.argtypes) == 10 and len(lib.insider_hip_coexpression.argtypes) == 12
    assert lib.insider_hip_last_gram_topk_ms.restype is C.c_double
    assert os.path.join(_build.CSRC, "insider_coexpr.hpp") in _build.source_files()
    kern = open(os.path.join(ROOT, "insider_amd", "csrc", "insider_coexpr.hpp")).read()
    nn = open(os.path.join(ROOT, "insider_amd", "csrc", "insider_neighbors.hpp")).read()

    def const(src, name):
        return re.search(rf"constexpr int {name} = ([^;]+);", src).group(1).strip()

    assert int(const(kern, "CX_DC")) == api.CX_DC
    waves, bt = int(const(kern, "CX_WAVES")), int(const(kern, "CX_BT"))
    assert const(kern, "CX_QB") == "16 * CX_WAVES" and 16 * waves == api.CX_QB
    assert const(kern, "CX_BG") == "16 * CX_BT" and 16 * bt == api.CX_BG
    assert int(const(nn, "NN_MAX_TOPK")) == api.NEIGHBOR_MAX_K
