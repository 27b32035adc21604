"""The numpy yardstick posthoc.tsne_host() against a brute-force dense evaluation in longdouble, the draw against the header's
formula in plain integers, every refusal of api.tsne_args() and the fit driver's flag errors.  No GPU.

The dense evaluation (tsne_reference.dense_eval) builds the N x N matrix P from the conditionals and sums Z, KL and the gradient
over all pairs in longdouble (u_ld = 2^-64 against 2^-53: its own error is three decimal orders below the bounds).  Bounds, with
U = 2^-52: Z relative (Na + 8) U; a gradient component posthoc.tsne_grad_bound() (slabs = 1); KL: (m_tot + 8) U sum |terms| +
(sum P) (Na + 8) U for the error of log Z, m_tot the number of terms.  The conditionals are compared at the yardstick's own
beta: p_s|i = exp(-beta d_s) / S errs by at most (k + 4) U (1 + beta d_s) (the exponent's rounding is amplified by its size).
The calibration itself: H(beta) is evaluated in fp64 with an error of about (m + 8) U (1 + E[beta d]), and the bisection
resolves beta to one ulp, which moves H by beta^2 Var(d) U <= E[(beta d)^2] U: |H - log perplexity| <= (m + 8) U (1 + E[beta d]
+ E[(beta d)^2]), the moments under p, in longdouble."""
import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from tests import tsne_reference as ref

U = 2.0 ** -52


def graph(N, k, seed, dead=(), open_rows=(), equal_rows=(), far_rows=()):
    """A random graph on N points: row i names k distinct others; rows in open_rows keep half their slots, the points in dead
    have no slot and are named by nobody, rows in equal_rows have equal distances, rows in far_rows one distance of 1e6."""
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


CASES = [dict(N=2, k=1, seed=1), dict(N=3, k=2, seed=2), dict(N=3, k=1, seed=3), dict(N=17, k=5, seed=4, dead=(6,), open_rows=(2, 9),
                                                                                    equal_rows=(4,), far_rows=(11,)),
         dict(N=17, k=16, seed=5, open_rows=(0,), equal_rows=(16,))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c['N']}k{c['k']}")
@pytest.mark.parametrize("perplexity", [1.0, 2.5, 64.0])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
def test_yardstick_against_dense_longdouble(case, perplexity, scale):
    c = dict(case)
    N, k, seed = c.pop("N"), c.pop("k"), c.pop("seed")
    idx, d2 = graph(N, k, seed, **c)
    Y = np.random.default_rng(seed + 100).standard_normal((N, 2)) * scale
    if N >= 3:
        Y[2] = Y[0]                                                 # two coincident points
    got = posthoc.tsne_host(idx, d2, perplexity=perplexity, init=Y, max_iter=0)
    alive = got["alive"]
    na = int(alive.sum())
    assert np.array_equal(alive, ~np.isin(np.arange(N), c.get("dead", ())))
    assert np.all(np.isnan(got["y"][~alive])) and np.array_equal(got["y"][alive], Y[alive])
    assert np.all(np.isfinite(got["beta"][alive])) and np.all(np.isfinite(got["p_cond"]))
    assert np.all(got["p_cond"][idx < 0] == 0.0)
    m = (idx >= 0).sum(axis=1)
    assert np.all(np.abs(got["p_cond"].sum(axis=1)[m > 0] - 1.0) <= (k + 4) * U)
    for i in c.get("equal_rows", ()):
        assert np.allclose(got["p_cond"][i, :m[i]], 1.0 / m[i], rtol=0, atol=4 * U)
        assert got["beta"][i] == (2.0 ** 100 if perplexity < m[i] else 1.0)
    # the calibration: H at the yardstick's beta, and the conditionals at that beta, in longdouble
    H, p_ld, mom = ref.entropy_ld(idx, d2, got["beta"])
    search = (m > 0) & (perplexity < m) & ~np.isin(np.arange(N), c.get("equal_rows", ()))
    if search.any():
        err = np.abs(H[search] - np.log(np.longdouble(perplexity)))
        print("max |H - log perplexity|", float(err.max()), "of bound", float(np.max(err / ((m[search] + 8) * U * mom[search]))))
        assert np.all(err <= (m[search] + 8) * U * mom[search])
    uniform = (m > 0) & (perplexity >= m)
    assert np.all(got["p_cond"][uniform] == np.where(idx[uniform] >= 0, 1.0 / m[uniform][:, None], 0.0))
    rows = search | np.isin(np.arange(N), c.get("equal_rows", ()))
    bd = np.where(idx >= 0, got["beta"][:, None] * (d2 - np.nanmin(np.where(idx >= 0, d2, np.inf), axis=1, keepdims=True)), 0.0)
    assert np.all(np.abs(got["p_cond"] - p_ld)[rows] <= ((k + 4) * U * (1.0 + bd))[rows])
    # Z, KL and the gradient over the dense P made of the yardstick's conditionals
    ex = ref.dense_eval(idx, got["p_cond"], Y, alive)
    assert abs(got["z"] - ex["z"]) <= (na + 8) * U * ex["z"]
    bound = got["grad_bound"]
    gerr = np.abs(got["grad"][alive] - ex["grad"][alive])
    print("max gradient error / bound", float(np.max(gerr / bound[alive])))
    assert np.all(gerr <= bound[alive]) and np.all(np.isnan(got["grad"][~alive]))
    assert abs(got["final_kl"] - ex["kl"]) <= (ex["kl_terms"] + 8) * U * ex["kl_abs"] + ex["p_sum"] * (na + 8) * U
    assert got["kl_traj"].shape == (1,) and got["kl_traj"][0] == got["final_kl"]
    assert abs(float(ex["p_sum"]) - 1.0) <= (N * k + 8) * U


def test_the_schedule_by_hand():
    """Three iterations against a plain transcription of the header's update on the dense longdouble gradient."""
    idx, d2 = graph(17, 5, 7, dead=(3,))
    kw = dict(perplexity=2.0, exag_iters=2, kl_every=2, exaggeration=4.0, seed=99)
    got = posthoc.tsne_host(idx, d2, max_iter=3, **kw)
    alive = got["alive"]
    na = int(alive.sum())
    Y = posthoc.tsne_draw_host(99, 17)
    gain, v = np.ones((17, 2)), np.zeros((17, 2))
    step = max(na / (4.0 * 4.0), 50.0)
    kls = []
    for t in range(3):
        a, mu = (4.0, 0.5) if t < 2 else (1.0, 0.8)
        ex = ref.dense_eval(idx, got["p_cond"], Y, alive, a)
        kls.append(float(ex["kl"]))
        g = np.where(alive[:, None], ex["grad"].astype(np.float64), 0.0)
        gain = np.maximum(np.where((g > 0) != (v > 0), gain + 0.2, gain * 0.8), 0.01)
        v = mu * v - (step * gain) * g
        Y = Y + v
        Y = Y - Y[alive].mean(axis=0)
    assert np.allclose(got["y"][alive], Y[alive], rtol=1e-9, atol=0) and np.all(np.isnan(got["y"][~alive]))
    assert got["kl_traj"].shape == (2,) and np.allclose(got["kl_traj"], [kls[0], kls[2]], rtol=1e-12)
    assert np.isfinite(got["min_abs_g"]) and np.isfinite(got["min_abs_v"]) and got["min_g_margin"] > 1.0
    again = posthoc.tsne_host(idx, d2, max_iter=3, **kw)
    assert np.array_equal(again["y"], got["y"], equal_nan=True)
    moved = posthoc.tsne_host(idx, d2, max_iter=3, perturb_seed=1, **kw)
    assert not np.array_equal(moved["y"], got["y"], equal_nan=True)
    assert np.allclose(moved["y"][alive], got["y"][alive], rtol=1e-6, atol=1e-12)


def _h32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


@pytest.mark.parametrize("seed", [0, 1, 0x1D5EED, 2 ** 64 - 1, 0xDEADBEEF12345678])
def test_the_draw_is_the_headers_formula(seed):
    N = 300
    Y = posthoc.tsne_draw_host(seed, N)
    key = _h32(_h32((seed & 0xFFFFFFFF) ^ 0x9E3779B9) ^ (seed >> 32))
    for i in (0, 1, 2, 17, 255, 299):
        for d in (0, 1):
            u = _h32(key ^ ((0x27D4EB2F * (2 * i + d + 1)) & 0xFFFFFFFF))
            assert Y[i, d] == ((u + 0.5) * 2.0 ** -32 - 0.5) * 1e-4
    assert Y.shape == (N, 2) and np.all(np.abs(Y) < 0.5e-4) and np.unique(Y).size == 2 * N
    assert abs(Y.mean()) < 1e-5 and 0.2e-4 < Y.std() < 0.4e-4


def test_every_refusal_of_tsne_args():
    idx, d2 = graph(12, 4, 11)
    init = np.random.default_rng(0).standard_normal((12, 2))

    def refused(i=idx, d=d2, **kw):
        with pytest.raises(_lib.InsiderError) as e:
            api.tsne_args(i, d, kw.pop("perplexity", 2.0), **kw)
        assert e.value.status == _lib.ERR_ARG

    api.tsne_args(idx, d2, 2.0)                                     # the base case is accepted
    refused(i=None)
    refused(d=None)
    refused(i=idx[:, 0])
    refused(i=idx.astype(np.float64))
    refused(i=np.full((2 ** 20 + 1, 1), -1, dtype=np.int32), d=np.zeros((2 ** 20 + 1, 1)))
    refused(i=np.zeros((4, 0), dtype=np.int32), d=np.zeros((4, 0)))
    wide = np.tile(np.arange(1, 66, dtype=np.int32), (70, 1))
    refused(i=wide, d=np.ones(wide.shape))                          # k = 65
    refused(d=d2[:, :3])
    for p in (0.5, np.nan, np.inf, -1.0, True, "2"):
        refused(perplexity=p)
    for name, vals in (("max_iter", (-1, 10001, 1.5, True)), ("exag_iters", (-1, 10001)), ("kl_every", (0, -5)), ("slabs", (-1, 65)),
                       ("seed", (-1, 2 ** 64)), ("exaggeration", (0.5, np.nan, np.inf)), ("eta", (-1.0, np.nan, np.inf))):
        for v in vals:
            refused(**{name: v})
    refused(max_iter=0)                                             # without init
    api.tsne_args(idx, d2, 2.0, init=init, max_iter=0)
    for bad_index in (12, -2):
        b = idx.copy()
        b[3, 1] = bad_index
        refused(i=b)
    b = idx.copy()
    b[5, 2] = 5
    refused(i=b)                                                    # a self edge
    b = idx.copy()
    b[5, 2] = b[5, 0]
    refused(i=b)                                                    # a repeat
    b = idx.copy()
    b[5, 1] = -1
    refused(i=b)                                                    # a filled slot after an open one
    for val in (-0.5, np.nan, np.inf):
        b = d2.copy()
        b[7, 3] = val
        refused(d=b)
    b, bd = idx.copy(), d2.copy()
    b[5, 3], bd[5, 3] = -1, -7.0                                    # (an open slot's d2 is not read)
    api.tsne_args(b, bd, 2.0)
    refused(init=init[:11])
    refused(init=init.T)
    bi = init.copy()
    bi[4, 1] = np.nan
    refused(init=bi)
    refused(i=np.full((1, 1), -1, dtype=np.int32), d=np.full((1, 1), np.nan))                    # N = 1: Na < 2
    refused(i=np.full((5, 2), -1, dtype=np.int32), d=np.full((5, 2), np.nan))                    # nobody is alive
    out = api.tsne_args(np.array([[1], [-1], [-1]]), np.array([[0.5], [np.nan], [np.nan]]), 1.0)  # Na = 2, one dead point
    assert out[0].dtype == np.int32 and out[0].flags.c_contiguous and np.array_equal(out[-1], [True, True, False])


def test_defaults_of_the_maps():
    assert posthoc.tsne_defaults(1000, 1000) == (20.0, 60)
    assert posthoc.tsne_defaults(10 ** 5, 10 ** 5, perplexity=30.0) == (30.0, 64)
    assert posthoc.tsne_defaults(31, 40) == (10.0, 30)
    assert posthoc.tsne_defaults(3, 3) == (1.0, 2)
    assert posthoc.tsne_defaults(50, 50, k=7) == (49 / 3.0, 7)


@pytest.mark.parametrize("argv", [["--gene-map", "--tune"], ["--sample-map", "--tune"], ["--map-perplexity", "5"],
                                  ["--map-neighbors", "10"], ["--gene-map", "--map-perplexity", "0.5"],
                                  ["--gene-map", "--map-perplexity", "nan"], ["--gene-map", "--map-neighbors", "0"],
                                  ["--sample-map", "--map-neighbors", "65"], ["--gene-map", "--map-iters", "0"],
                                  ["--gene-map", "--map-iters", "10001"], ["--gene-map", "--map-seed", "-1"],
                                  ["--gene-map", "--map-seed", str(2 ** 64)]])
def test_fit_flag_errors(argv, capsys):
    from insider_amd import fit
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    with pytest.raises(SystemExit) as e:
        fit.parse(base + argv)
    assert e.value.code == 2 and "--" in capsys.readouterr().err


def test_fit_flags_are_parsed():
    from insider_amd import fit
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.2"]
    a = fit.parse(base + ["--gene-map", "--sample-map", "--map-perplexity", "7.5", "--map-neighbors", "20", "--map-iters", "300",
                          "--map-seed", "5"])
    assert (a.gene_map, a.sample_map, a.map_perplexity, a.map_neighbors, a.map_iters, a.map_seed) == (True, True, 7.5, 20, 300, 5)
    a = fit.parse(base)
    assert (a.gene_map, a.sample_map, a.map_perplexity, a.map_neighbors, a.map_iters) == (False, False, None, None, 1000)
    rec = dict(y=np.zeros((4, 2)), kl_traj=np.arange(3.0), final_kl=9.0, beta=np.ones(4))
    out = fit.ts_records("ts_gene", rec)
    assert sorted(out) == ["ts_gene_beta", "ts_gene_kl", "ts_gene_y"] and np.array_equal(out["ts_gene_kl"], [0.0, 1.0, 2.0, 9.0])


def test_symbols_name_the_new_entry():
    assert "insider_hip_tsne" in _lib.SYMBOLS and "insider_hip_last_tsne_ms" in _lib.SYMBOLS
