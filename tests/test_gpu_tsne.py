"""insider_hip_tsne on the device, stage by stage, against the dense longdouble evaluation of tests/tsne_reference.py and the
numpy yardstick posthoc.tsne_host().

Every call goes through ctypes with outputs prefilled with sentinels and NGUARD guard elements past every array's end; the
guards must be unchanged after every call, and after a refused call the whole output is.

Bounds are derived, not fitted (U = 2^-52; a sum of n terms in any order errs by at most (n - 1) 2^-53 sum |terms| to first
order, the constant 8 leaves room for the terms' own roundings and a reciprocal good to 2 ulp):
  conditionals   a row sums to 1 within (k + 4) U, open slots are exactly 0;
  beta           |H(beta_dev) - log perplexity|, H in longdouble, within 8 times the largest value the yardstick's own beta
                 reaches on the same rows (the 8: another exp and another summation order);
  Z              relative (Na + slabs + 8) U;
  gradient       4 [(m + 8) U sum |attractive terms| + (Na + slabs + 8) U sum_j |w^2 delta| / Z + |repulsive part| rz],
                 rz the bound of Z (posthoc.tsne_grad_bound on the reference's sums; slabs = 0 counts as 1: the order of a sum
                 does not enter the first-order bound);
  KL             (terms + 8) U sum |terms| + (sum P) rz  (the error of log Z enters every term).
Stages are tested one at a time: the reference of Z, KL and the gradient is built from the DEVICE's conditionals.

Whole runs cannot be bounded this way (the map amplifies rounding): the device may differ from the yardstick by at most 10
times what the yardstick itself moves when every gradient component is shifted by + or - its bound above.

Measured on an MI355X (every figure is printed by its test):
  beta           largest |H - log perplexity| over the cases with perplexity > 1: device 7.93e-16, yardstick 7.93e-16 (case by
                 case the two differ by at most a quarter); at perplexity 1 the target is 0 and the root is where exp
                 underflows: device 3.64e-316, yardstick 3.64e-316, equal in every case;
  Z, KL, gradient  largest error / bound over all cases and slabs: Z 0.060, gradient 0.066, KL 0.035;
  short runs     per N: what the yardstick moves under the perturbation (smallest .. largest over the 40 cases), the largest
                 |Y_dev - Y_host| and its largest share of the allowance (10 x the case's own move):
                   N = 3    3.4e-17 .. 4.5e-11   4.3e-14   0.021        N = 65    2.8e-17 .. 4.7e-09   2.7e-10   0.0063
                   N = 17   3.9e-17 .. 8.7e-11   1.4e-12   0.0098       N = 130   1.6e-17 .. 5.0e-10   1.8e-11   0.0054
                   N = 64   2.9e-17 .. 1.6e-08   1.4e-09   0.037        N = 257   1.1e-17 .. 4.2e-10   4.2e-12   0.0062
                 no case was left out as undecided."""
import ctypes as C

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from tests import tsne_reference as ref
from tests.support import bits, lib  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu

NGUARD = 7
SENTINEL = 12345.678
U = 2.0 ** -52
NAMES = ("Y", "kl_traj", "final_kl", "beta", "p_cond", "grad", "Z")


def call(lib, idx, d2, perplexity=2.0, init=None, max_iter=0, exag_iters=250, kl_every=50, exaggeration=12.0, eta=0.0, seed=7,
         slabs=0, N=None, k=None, expect=_lib.OK, null=()):
    """One guarded call; idx (N x k int32) and d2 (N x k) row-major.  N and k are passed as given; the arrays are sized from
    the graph's own shape."""
    Np, kp = idx.shape
    N = Np if N is None else N
    k = kp if k is None else k
    nrec = min(max(max_iter, 0), 10001) // max(kl_every, 1) + 1
    size = dict(Y=2 * Np, kl_traj=nrec, final_kl=1, beta=Np, p_cond=Np * kp, grad=2 * Np, Z=1)
    out = {n: np.full(size[n] + NGUARD, SENTINEL) for n in NAMES}
    idx, d2 = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(d2, dtype=np.float64)
    ip = None if init is None else _lib.ptr(np.ascontiguousarray(init, dtype=np.float64))
    args = [_lib.ptr(idx, C.c_int32), _lib.ptr(d2), N, k, perplexity, ip, max_iter, exag_iters, kl_every, exaggeration, eta, seed,
            slabs, 0] + [_lib.ptr(out[n]) for n in NAMES]
    for pos in null:
        args[pos] = None
    status = lib.insider_hip_tsne(*args)
    assert status == expect, (status, lib.insider_hip_last_error().decode(errors="replace"))
    for pos, n in enumerate(NAMES):
        used = size[n] if status == _lib.OK and 14 + pos not in null else 0
        assert np.all(out[n][used:] == SENTINEL), n
    if status != _lib.OK:
        return None
    rec = {n: out[n][:size[n]].copy() for n in NAMES}
    for n in ("Y", "grad"):
        rec[n] = rec[n].reshape(Np, 2)
    rec["p_cond"] = rec["p_cond"].reshape(Np, kp)
    rec["final_kl"], rec["Z"] = float(rec["final_kl"][0]), float(rec["Z"][0])
    return rec


def random_graph(N, k, seed, dead=(), open_rows=(), equal_rows=(), far_rows=()):
    """Row i names min(k, candidates) distinct others (half of them in open_rows); the points in dead have no slot and are named
    by nobody; equal_rows have equal distances; far_rows one distance of 1e6 (the underflow path)."""
    rng = np.random.default_rng(seed)
    idx = np.full((N, k), -1, dtype=np.int32)
    d2 = np.full((N, k), np.nan)
    ok = np.setdiff1d(np.arange(N), dead)
    for i in ok:
        cand = ok[ok != i]
        m = min(k, cand.size)
        if i in open_rows:
            m = max(1, m // 2)
        idx[i, :m] = rng.choice(cand, m, replace=False)
        d2[i, :m] = rng.random(m) * 3.0
        if i in equal_rows:
            d2[i, :m] = 0.75
        if i in far_rows:
            d2[i, m - 1] = 1e6
    return idx, d2


def knn_graph(X, k):
    """The exact k nearest neighbours of the rows of X (N x D) by squared Euclidean distance, on the host."""
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D2, np.inf)
    idx = np.argsort(D2, axis=1, kind="stable")[:, :k].astype(np.int32)
    return idx, np.take_along_axis(D2, idx, axis=1)


# ---- 1. calibration ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 12, 64])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 130])
def test_calibration(lib, N, k):
    """Measured on an MI355X, the largest |H(beta) - log perplexity| in longdouble: device 7.93e-16 against the yardstick's
    7.93e-16 for perplexity > 1, 3.64e-316 against 3.64e-316 at perplexity 1 (both maxima are printed per case)."""
    special = dict(dead=(5,), open_rows=(1, 7), equal_rows=(3,), far_rows=(9,)) if N > 10 else {}
    idx, d2 = random_graph(N, k, 1000 * N + k, **special)
    m = (idx >= 0).sum(axis=1)
    init = np.random.default_rng(1).standard_normal((N, 2))
    rows = np.arange(N)
    for perplexity in sorted({1.0, 4.0, max(1.0, k / 2.0), float(k), 100.0}):
        got = call(lib, idx, d2, perplexity=perplexity, init=init)
        host = posthoc.tsne_host(idx, d2, perplexity=perplexity, init=init, max_iter=0)
        alive = host["alive"]
        assert np.all(got["p_cond"][idx < 0] == 0.0) and np.all(np.isfinite(got["p_cond"]))
        assert np.all(np.abs(got["p_cond"].sum(axis=1)[m > 0] - 1.0) <= (k + 4) * U)
        assert np.all(np.isnan(got["beta"][~alive])) and np.all(np.isfinite(got["beta"][alive]))
        uniform = (m > 0) & (perplexity >= m)
        assert np.all(got["p_cond"][uniform] == np.where(idx[uniform] >= 0, 1.0 / m[uniform][:, None], 0.0))
        assert np.all(got["beta"][uniform] == 1.0)
        for i in special.get("equal_rows", ()):
            assert np.allclose(got["p_cond"][i, :m[i]], 1.0 / m[i], rtol=0, atol=4 * U)
            assert got["beta"][i] == (2.0 ** 100 if perplexity < m[i] else 1.0)
        search = (m > 0) & (perplexity < m) & ~np.isin(rows, special.get("equal_rows", ()))
        if not search.any():
            continue
        target = np.log(np.longdouble(perplexity))
        e_dev = np.abs(ref.entropy_ld(idx, d2, got["beta"])[0][search] - target)
        e_host = np.abs(ref.entropy_ld(idx, d2, host["beta"])[0][search] - target)
        print(f"N {N} k {k} perplexity {perplexity}: max |H - target| device {float(e_dev.max()):.3e} yardstick "
              f"{float(e_host.max()):.3e}")
        assert e_dev.max() <= 8 * e_host.max()
        # the conditionals at the device's own beta
        p_ld = ref.entropy_ld(idx, d2, got["beta"])[1]
        bd = np.where(idx >= 0, got["beta"][:, None] * (d2 - np.nanmin(np.where(idx >= 0, d2, np.inf), axis=1, keepdims=True)), 0.0)
        assert np.all(np.abs(got["p_cond"] - p_ld)[search] <= ((k + 4) * U * (1.0 + bd))[search])


# ---- 2. Z, KL and the gradient at a given map -----------------------------------------------------------------------------------
MAPS = ("tiny", "unit", "wide", "coincident", "dead")


@pytest.fixture(scope="module")
def eval_graphs():
    out = {}
    for N in (2, 3, 63, 64, 65, 127, 128, 129, 257, 1030):
        k = min(9, N - 1)
        for with_dead in (False, True):
            dead = (N - 2,) if with_dead and N > 3 else ((2,) if with_dead and N == 3 else ())
            out[N, with_dead] = random_graph(N, k, 77 * N, dead=dead, open_rows=(0,))
    return out


def grad_bound(ex, na, slabs):
    ev = {n: np.asarray(ex[n], dtype=np.float64) for n in ("attr_abs", "rep_abs", "rep", "terms")}
    ev["z"] = float(ex["z"])
    return posthoc.tsne_grad_bound(ev, na, slabs)


# (two points cannot spare a dead one: Na < 2 is refused, test_bad_arguments_are_refused_and_write_nothing)
@pytest.mark.parametrize("N,kind", [(N, kind) for N in (2, 3, 63, 64, 65, 127, 128, 129, 257, 1030) for kind in MAPS
                                    if (N, kind) != (2, "dead")])
def test_gradient_z_kl_at_a_given_map(lib, eval_graphs, N, kind):
    idx, d2 = eval_graphs[N, kind == "dead"]
    rng = np.random.default_rng(N)
    Y = rng.standard_normal((N, 2)) * {"tiny": 1e-4, "unit": 1.0, "wide": 50.0}.get(kind, 1.0)
    if kind == "coincident":
        Y[1] = Y[0]
    worst = dict(z=0.0, g=0.0, kl=0.0)
    ex = None
    for slabs in (0, 1, 2, 3, 7):
        got = call(lib, idx, d2, perplexity=3.0, init=Y, slabs=slabs)
        if ex is None:                                             # (the conditionals do not depend on slabs)
            first = got
            alive = (idx[:, 0] >= 0) | (np.bincount(idx[idx >= 0], minlength=N) > 0)
            na = int(alive.sum())
            assert na == N - (1 if kind == "dead" else 0)
            ex = ref.dense_eval(idx, got["p_cond"], Y, alive)
        assert np.array_equal(got["p_cond"], first["p_cond"]) and np.array_equal(got["beta"], first["beta"], equal_nan=True)
        s = max(slabs, 1)
        rz = (na + s + 8) * U
        assert np.array_equal(got["Y"][alive], Y[alive]) and np.all(np.isnan(got["Y"][~alive]))
        assert np.all(np.isnan(got["grad"][~alive]))
        zerr = abs(got["Z"] - ex["z"]) / ex["z"]
        gabs, gb = np.abs(got["grad"][alive] - ex["grad"][alive]).astype(np.float64), grad_bound(ex, na, s)[alive]
        assert np.all(gabs <= gb), (slabs, float(np.max(gabs - gb)))   # (two points on one spot: no force, 0 <= 0)
        gerr = np.where(gb > 0, gabs / np.where(gb > 0, gb, 1.0), 0.0)
        kbound = (ex["kl_terms"] + 8) * U * ex["kl_abs"] + ex["p_sum"] * rz
        kerr = abs(got["final_kl"] - ex["kl"]) / kbound
        worst = dict(z=max(worst["z"], float(zerr / rz)), g=max(worst["g"], float(gerr.max())), kl=max(worst["kl"], float(kerr)))
        assert zerr <= rz and np.all(gerr <= 1.0) and kerr <= 1.0, (slabs, float(zerr / rz), float(gerr.max()), float(kerr))
        assert got["kl_traj"][0] == got["final_kl"]
    print(f"N {N} {kind}: worst error / bound  Z {worst['z']:.3f}  gradient {worst['g']:.3f}  KL {worst['kl']:.3f}")


# ---- 3. exact arithmetic --------------------------------------------------------------------------------------------------------
def test_lattice_mirrors_to_the_bit_and_the_self_pair_costs_nothing(lib):
    rng = np.random.default_rng(3)
    N, k = 150, 6
    idx, _ = random_graph(N, k, 33)
    d2 = np.where(idx >= 0, 1.0, np.nan)                            # uniform rows
    Y = rng.integers(-2, 3, (N, 2)).astype(np.float64)              # ties and coincident points everywhere
    for slabs in (0, 1, 3):
        base = call(lib, idx, d2, perplexity=2.0, init=Y, slabs=slabs)
        assert np.all(base["p_cond"][idx >= 0] == 1.0 / k)
        for sx, sy in ((-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)):
            flip = np.array([sx, sy])
            got = call(lib, idx, d2, perplexity=2.0, init=Y * flip, slabs=slabs)
            assert np.array_equal(got["grad"], base["grad"] * flip)  # every operation is odd or even in a coordinate
            assert got["Z"] == base["Z"] and got["final_kl"] == base["final_kl"]
    # two points whose w is a power of two: Z = 2 w exactly, so the self pairs left nothing behind (the device leaves them out
    # of the sums; had it added their 1 and taken N off afterwards, the small w below would have lost its last bits)
    pair, dd = np.array([[1], [0]], dtype=np.int32), np.ones((2, 1))
    for a, b, z in (((0.0, 0.0), (1.0, 0.0), 1.0), ((0.0, 0.0), (0.0, 0.0), 2.0), ((-1.0, 2.0), (-1.0, 1.0), 1.0),
                    ((0.0, 0.0), (2.0 ** 30, 0.0), 2.0 / (1.0 + 2.0 ** 60)), ((0.0, 3.0), (0.0, 3.0 + 2.0 ** -30), 2.0 / (1.0 + 2.0 ** -60))):
        for slabs in (0, 1, 2, 5):
            got = call(lib, pair, dd, perplexity=1.0, init=np.array([a, b]), slabs=slabs)
            assert got["Z"] == z, (a, b, slabs, got["Z"])
    # all N points on one spot: every w is exactly 1, Z = N (N - 1) exactly, and no force
    spot = call(lib, idx, d2, perplexity=2.0, init=np.full((N, 2), 1.5))
    assert spot["Z"] == float(N * (N - 1)) and np.all(spot["grad"] == 0.0)


# ---- 4. short runs against the yardstick ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 17, 64, 65, 130, 257])
def test_short_runs_follow_the_yardstick(lib, N):
    """Measured on an MI355X: the table in the module docstring (printed per N)."""
    k = min(12, N - 1)
    perplexity = min(4.0, k / 2.0)
    left_out, cases, worst_dev, worst_ratio, moves = 0, 0, 0.0, 0.0, []
    for seed in range(100, 110):
        X = np.random.default_rng(seed).standard_normal((N, 6))
        idx, d2 = knn_graph(X, k)
        for max_iter in (1, 2, 5, 20):
            kw = dict(perplexity=perplexity, max_iter=max_iter, exag_iters=10, seed=seed)
            host = posthoc.tsne_host(idx, d2, **kw)
            cases += 1
            if min(host["min_g_margin"], host["min_v_margin"]) < 1.0:
                left_out += 1
                continue
            moved = posthoc.tsne_host(idx, d2, perturb_seed=seed, **kw)
            allowed = 10.0 * float(np.abs(moved["y"] - host["y"]).max())
            moves.append(allowed / 10.0)
            got = call(lib, idx, d2, **kw)
            diff = float(np.abs(got["Y"] - host["y"]).max())
            worst_dev, worst_ratio = max(worst_dev, diff), max(worst_ratio, diff / allowed)
            assert diff <= allowed, (seed, max_iter, diff, allowed)
            # centred: N differences rounded to U / 2 each, a mean good to N U / 2, and this sum's own N U / 2
            assert np.all(np.abs(got["Y"].sum(axis=0)) <= 4 * N * U * np.abs(got["Y"]).max())
    print(f"N {N}: {cases} cases, {left_out} left out, the yardstick moved by {min(moves):.3e} .. {max(moves):.3e} under the "
          f"perturbation, largest |Y_dev - Y_host| {worst_dev:.3e}, largest share of the allowance {worst_ratio:.3e}")
    assert left_out * 10 <= cases


# ---- 5. purity ------------------------------------------------------------------------------------------------------------------
def test_repeats_are_bit_identical_and_the_draw_is_the_hosts(lib):
    N, k = 300, 10
    idx, d2 = knn_graph(np.random.default_rng(5).standard_normal((N, 4)), k)
    idx[17], d2[17] = -1, np.nan                                    # a point with no row of its own (alive: others name it)
    kw = dict(perplexity=3.0, max_iter=30, exag_iters=10, kl_every=7, seed=0xFEEDFACE12345)
    for slabs in (0, 3):
        runs = [call(lib, idx, d2, slabs=slabs, **kw) for _ in range(3)]
        assert bits(runs[0], NAMES) == bits(runs[1], NAMES) == bits(runs[2], NAMES)
        assert np.all(np.isfinite(runs[0]["kl_traj"])) and runs[0]["kl_traj"].shape == (5,)
    given = call(lib, idx, d2, init=posthoc.tsne_draw_host(kw["seed"], N), **kw)
    assert bits(given, NAMES) == bits(call(lib, idx, d2, **kw), NAMES)
    assert lib.insider_hip_last_tsne_ms() > 0.0
    # optional outputs may be absent; what is present does not change
    some = call(lib, idx, d2, null=(17, 18, 19, 20), **kw)
    assert np.array_equal(some["Y"], given["Y"]) and some["final_kl"] == given["final_kl"]
    # kl_traj: entry j is KL at Y_(j kl_every); a multiple of kl_every ends on the final KL
    even = call(lib, idx, d2, **dict(kw, max_iter=28))
    assert even["kl_traj"].shape == (5,) and even["kl_traj"][4] == even["final_kl"]
    assert np.array_equal(even["kl_traj"][:4], given["kl_traj"][:4])


# ---- 6. a real map --------------------------------------------------------------------------------------------------------------
def test_three_blobs_separate(lib):
    """Measured on an MI355X: KL 3.266 at t = 0, 2.244 at t = 250, 0.6673 at the end; the yardstick's five finals 0.6430 .. 0.6615
    (spread 0.0289), the allowance (1 + spread) x 0.6522 = 0.6710; every point's nearest map neighbour is of its blob."""
    rng = np.random.default_rng(6)
    centres = 3.0 * rng.standard_normal((3, 5))
    label = np.repeat(np.arange(3), 100)
    X = centres[label] + 0.3 * rng.standard_normal((300, 5))
    idx, d2 = posthoc.embedding_graph(np.asfortranarray(X.T), 30)
    assert idx.shape == d2.shape == (300, 30) and idx.dtype == np.int32 and np.all(d2 >= 0)
    kw = dict(perplexity=10.0, max_iter=500)
    got = api.tsne(idx, d2, seed=1, **kw)
    Y = got["y"]
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, np.inf)
    assert np.array_equal(label[D.argmin(axis=1)], label)
    assert got["kl_traj"].shape == (11,) and got["final_kl"] < got["kl_traj"][5] and got["final_kl"] == got["kl_traj"][10]
    finals = np.array([posthoc.tsne_host(idx, d2, seed=s, **kw)["final_kl"] for s in range(1, 6)])
    spread = float((finals.max() - finals.min()) / finals.min())
    print("device final KL", got["final_kl"], "KL at 0 / 250", got["kl_traj"][0], got["kl_traj"][5], "yardstick finals", finals,
          "spread", spread, "ms", got["ms"])
    assert got["final_kl"] <= (1.0 + spread) * finals[0]


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(lib):
    idx, d2 = random_graph(12, 4, 11)
    init = np.random.default_rng(0).standard_normal((12, 2))
    bad = _lib.ERR_ARG
    ok = dict(init=init)
    for pos in (0, 1, 14, 15, 16):                                  # the graph and the required outputs
        call(lib, idx, d2, expect=bad, null=(pos,), **ok)
    call(lib, idx, d2, N=0, expect=bad, **ok)
    call(lib, idx, d2, N=-1, expect=bad, **ok)
    call(lib, idx, d2, N=2 ** 20 + 1, expect=bad, **ok)              # (refused before the graph is read)
    call(lib, idx, d2, k=0, expect=bad, **ok)
    call(lib, idx, d2, k=65, expect=bad, **ok)
    for p in (0.5, np.nan, np.inf, -3.0):
        call(lib, idx, d2, perplexity=p, expect=bad, **ok)
    for name, vals in (("max_iter", (-1, 10001)), ("exag_iters", (-1, 10001)), ("kl_every", (0, -1)), ("slabs", (-1, 65)),
                       ("exaggeration", (0.5, np.nan, np.inf)), ("eta", (-1.0, np.nan, np.inf))):
        for v in vals:
            call(lib, idx, d2, expect=bad, **dict(ok, **{name: v}))
    call(lib, idx, d2, max_iter=0, expect=bad)                      # without init
    for row, slot, val in ((3, 1, 12), (3, 1, -2), (5, 2, 5), (5, 1, -1)):   # out of range twice, a self edge, filled after open
        b = idx.copy()
        b[row, slot] = val
        call(lib, b, d2, expect=bad, **ok)
    b = idx.copy()
    b[5, 2] = b[5, 0]
    call(lib, b, d2, expect=bad, **ok)                              # a repeat within a row
    for val in (-0.5, np.nan, np.inf):
        b = d2.copy()
        b[7, 3] = val
        call(lib, idx, b, expect=bad, **ok)
    for val in (np.nan, np.inf):
        b = init.copy()
        b[4, 1] = val
        call(lib, idx, d2, init=b, expect=bad)
    assert b"finite" in lib.insider_hip_last_error()
    none, nan = np.full((5, 2), -1, dtype=np.int32), np.full((5, 2), np.nan)
    call(lib, none, nan, init=init[:5], expect=bad)                 # nobody is alive
    call(lib, none[:1, :1], nan[:1, :1], init=init[:1], expect=bad)  # N = 1: Na < 2
    # what is allowed: Na = 2 with a dead point, an open slot's d2 of any value, max_iter = 0 with init, eta given
    two = call(lib, np.array([[1], [-1], [-1]], dtype=np.int32), np.array([[0.5], [-7.0], [np.inf]]), perplexity=1.0, init=init[:3])
    assert np.all(np.isnan(two["Y"][2])) and two["Z"] > 0 and np.array_equal(two["p_cond"].ravel(), [1.0, 0.0, 0.0])
    assert np.all(np.isfinite(call(lib, idx, d2, max_iter=3, eta=10.0)["Y"]))
    # the wrapper reports its own refusal
    with pytest.raises(_lib.InsiderError) as e:
        api.tsne(idx, d2, perplexity=0.5)
    assert e.value.status == _lib.ERR_ARG


# ---- 8. users' calls -------------------------------------------------------------------------------------------------------------
def test_gene_map_and_sample_map_on_random_factors(lib):
    rng = np.random.default_rng(9)
    K, p, n, counts, m = 6, 200, 80, (4, 3), 2
    Cm = np.asfortranarray(rng.standard_normal((K, p)))
    zero = rng.random(p) < 0.2                                      # the elastic net's all-zero columns
    Cm[:, zero] = 0.0
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    A = [rng.standard_normal((L, K)) for L in counts] + [rng.standard_normal((m, K))]
    Zc = rng.standard_normal((n, m))
    got = posthoc.gene_map(Cm, max_iter=150, exag_iters=30)
    na = int((~zero).sum())
    assert got["perplexity"] == min(20.0, (na - 1) / 3.0) and got["k"] == min(64, p - 1, int(np.ceil(3 * got["perplexity"])))
    assert got["y"].shape == (p, 2) and np.array_equal(np.isnan(got["y"][:, 0]), zero) and np.array_equal(got["alive"], ~zero)
    assert got["kl_traj"].shape == (4,) and got["final_kl"] < got["kl_traj"][0] and got["final_kl"] == got["kl_traj"][3]
    assert got["ms"] > 0
    again = posthoc.gene_map(Cm, max_iter=150, exag_iters=30)
    assert np.array_equal(again["y"], got["y"], equal_nan=True)
    ex = ref.dense_eval(got["nbr_idx"], got["p_cond"], np.nan_to_num(got["y"]), got["alive"])
    assert abs(got["final_kl"] - ex["kl"]) <= (ex["kl_terms"] + 8) * U * ex["kl_abs"] + ex["p_sum"] * (na + 9) * U
    assert abs(got["z"] - ex["z"]) <= (na + 9) * U * ex["z"]
    smp = posthoc.sample_map(A, lev, Zc, perplexity=5.0, k=12, max_iter=40, seed=3)
    assert smp["y"].shape == (n, 2) and np.all(np.isfinite(smp["y"])) and smp["nbr_idx"].shape == (n, 12) and smp["k"] == 12


def test_cli_writes_the_map_records(tmp_path):
    from insider_amd import fit as fit_cli
    rng = np.random.default_rng(10)
    n, p, K = 60, 45, 4
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    np.save(tmp_path / "X.npy", rng.standard_normal((n, p)))
    np.save(tmp_path / "L.npy", conf)
    np.save(tmp_path / "Z.npy", rng.standard_normal((n, 2)))
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--ctns", str(tmp_path / "Z.npy"),
                         "--rank", str(K), "--lambda", "1", "--alpha", "0.2", "--max-iter", "3", "--gene-map", "--sample-map",
                         "--map-perplexity", "4", "--map-neighbors", "10", "--map-iters", "100", "--map-seed", "5",
                         "--out", str(out)]) == 0
    for who, count in (("gene", p), ("sample", n)):
        y, kl, beta = (np.load(out / f"ts_{who}_{name}.npy") for name in ("y", "kl", "beta"))
        assert y.shape == (count, 2) and beta.shape == (count,) and kl.shape == (4,) and kl[-1] == kl[-2]
        alive = ~np.isnan(y[:, 0])
        assert alive.sum() >= 2 and np.all(np.isfinite(beta[alive])) and np.all(np.isfinite(kl))
