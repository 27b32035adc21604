"""Every sample scored against every level of a covariate on the resident data set (insider_hip_level_scores, k_ls_prod /
k_ls_reduce) against the numpy yardstick posthoc.level_scores_host().

Tolerance (derived, not measured): |sse_gpu - sse_host| <= 1e-12 scale(i, l) with
    scale(i, l) = sum_{j in S_i} (|x_ij| + F_{-cov}(i, j) + G_l(j))^2,
F_{-cov} = sum_{b != cov} |A_b|[level] @ |C| (+ |Z| @ |B_c| @ |C|) and G_l = |e_l| @ |C|: the bounds of
tests/test_gpu_sampdecomp.py.  The device forms the expanded sum s0 - 2 P1 + P2, whose three sums of absolute terms
(sum d^2, 2 sum |d| G, sum G^2 with |d| <= |x| + F) add up to exactly this scale; a term is a K-term dot product of at most B
embeddings and a sum adds fewer than p terms on either side: fewer than (p + K + 8) 2^-53 of the scale, below 1e-12 for
p + K < 9000 (every shape here).  The counts are compared exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from tests.support import SAMPLES_3_5_7, close_resident, factors, levels, masks, planted, resident, same_bits

pytestmark = pytest.mark.gpu

ENTRIES = ("all", "train", "test")
EMPTY = {"all": (), "train": (5, 7), "test": (3, 7)}


# train, test and NA entries; sample 3 has no test entry, sample 5 no train entry, sample 7 is all NA
_masks = functools.partial(masks, empty=SAMPLES_3_5_7)


def _data(n, p, counts, m=0, seed=0):
    d = planted(n, p, counts, m, seed, empty=SAMPLES_3_5_7)
    return (resident(*d),) + d


def _scale(X, lev, Z, mask, A, Cm, cov, cand=None):
    """scale(i, l) of the module docstring, n x L."""
    aC = np.abs(Cm)
    c = lev.shape[1]
    F = np.zeros(X.shape)
    for b in range(c):
        if b != cov:
            F = F + np.abs(A[b])[lev[:, b] - 1] @ aC
    if Z is not None:
        F = F + np.abs(Z) @ (np.abs(A[c]) @ aC)
    w = np.ones(X.shape, bool) if mask is None else mask
    base = np.where(w, np.abs(X) + F, 0.0)
    G = np.abs(A[cov] if cand is None else cand) @ aC
    return (base * base).sum(axis=1)[:, None] + 2.0 * base @ G.T + w.astype(np.float64) @ (G * G).T


def _check(got, X, lev, Z, mask, A, Cm, cov, cand=None):
    ref = posthoc.level_scores_host(X, lev, Z, mask, A, Cm, cov, candidates=cand)
    sc = _scale(X, lev, Z, mask, A, Cm, cov, cand)
    assert got["sse"].shape == ref["sse"].shape and got["n"].shape == ref["n"].shape
    assert np.array_equal(got["n"], ref["n"])
    err = np.abs(got["sse"] - ref["sse"])
    print("max error / scale:", np.max(err / np.maximum(sc, 1e-300)))
    assert np.all(err <= 1e-12 * sc), np.max(err / np.maximum(sc, 1e-300))
    return ref, sc


_same_bits = functools.partial(same_bits, keys=("sse", "n"))


@pytest.fixture(scope="module")
def two():
    ds, X, lev, Z, masks = _data(203, 157, (5, 3), seed=1)
    yield ds, X, lev, Z, masks
    ds.close()


@pytest.mark.parametrize("K", [1, 16, 17, 63])
def test_records_match_host(two, K):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(K), (5, 3), 0, K, X.shape[1])
    for cov in (0, 1):
        for e in ENTRIES:
            got = ds.level_scores(A, Cm, cov, entries=e)
            assert ds.info("ls_path") == 1
            assert got["sse"].shape == (203, (5, 3)[cov]) and got["n"].shape == (203,)
            _check(got, X, lev, Z, masks[e], A, Cm, cov)
            d = posthoc.ls_derived(got, lev[:, cov])
            for i in EMPTY[e]:
                assert got["n"][i] == 0 and np.all(got["sse"][i] == 0) and d["best"][i] == 0
            live = np.setdiff1d(np.arange(203), EMPTY[e])
            assert np.all(d["best"][live] >= 1)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 128, 129, 200])
def test_level_tiles_and_windows(L):
    """One level tile (the narrow kernel form) up to 16 levels, the window form beyond, one window up to 128 levels, two
    beyond: a last tile of 1, 15 and 16 live columns, a second window of one tile."""
    ds, X, lev, Z, masks = _data(203, 37, (L, 3), seed=L)
    try:
        A, Cm = factors(np.random.default_rng(L + 1), (L, 3), 0, 5, X.shape[1])
        for e in ("all", "train"):
            got = ds.level_scores(A, Cm, 0, entries=e)
            assert ds.info("ls_path") == (1 if L <= 128 else 2)
            _check(got, X, lev, Z, masks[e], A, Cm, 0)
    finally:
        ds.close()


@pytest.mark.parametrize("slabs", [1, 2, 3, 7, 0])
def test_slabs(two, slabs):
    """157 genes in 1, 2, 3, 7 slabs (no even split, no multiple of the 16 genes of a staging step) and the automatic count:
    the same sums within the bound, the same bits for the same setting; a tiny partial budget lowers the automatic count."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(40), (5, 3), 0, 9, X.shape[1])
    ds.set_option("ls_slabs", slabs)
    try:
        a = ds.level_scores(A, Cm, 0, entries="train")
        used = ds.info("ls_slabs")
        if slabs:
            assert used == slabs
        else:      # eight blocks per compute unit over four sample tiles, at most 256 slabs, then slabs of equal length
            want = min(256, -(-2 * int(ds.info("n_simd")) // 4))
            assert used == -(-157 // -(-157 // want))
        b = ds.level_scores(A, Cm, 0, entries="train")
        assert ds.info("ls_slabs") == used
        _check(a, X, lev, Z, masks["train"], A, Cm, 0)
        _same_bits(a, b)
        if not slabs:
            row_mb = 203 * 16 * 8 / 1048576.0          # one slab's partial scores: n x the 5 levels padded to 16
            for mb, want in ((3.5 * row_mb, 3), (0.0, 1)):
                ds.set_option("ls_part_mb", mb)
                c = ds.level_scores(A, Cm, 0, entries="train")
                assert ds.info("ls_slabs") == want < used
                _check(c, X, lev, Z, masks["train"], A, Cm, 0)
    finally:
        ds.set_option("ls_slabs", 0)
        ds.set_option("ls_part_mb", 256)


@pytest.mark.parametrize("n", [17, 63, 64, 65, 257])
def test_partial_sample_tiles(n):
    """n = 17: one sample in the second wave; 63 / 64 / 65: a block short of one sample, full, and a second block of one
    sample; 257: a fifth block of one sample."""
    ds, X, lev, Z, masks = _data(n, 37, (4, 3), seed=n)
    try:
        A, Cm = factors(np.random.default_rng(n), (4, 3), 0, 7, X.shape[1])
        for slabs in (0, 2):
            ds.set_option("ls_slabs", slabs)
            for e in ENTRIES:
                _check(ds.level_scores(A, Cm, 1, entries=e), X, lev, Z, masks[e], A, Cm, 1)
    finally:
        ds.close()


@pytest.mark.parametrize("counts,m,cov", [((3, 5, 2), 0, 1), ((2, 3, 2, 4, 2, 3, 2, 2, 3), 0, 8), ((4, 6), 2, 0),
                                          ((4, 6), 2, 1)])
def test_other_blocks(counts, m, cov):
    """Three covariates scoring the middle one, nine scoring the last, and two continuous columns."""
    ds, X, lev, Z, masks = _data(131, 97, counts, m=m, seed=len(counts) + 10 * m)
    try:
        for K in (5, 33):
            A, Cm = factors(np.random.default_rng(K + m), counts, m, K, X.shape[1])
            for e in ENTRIES:
                got = ds.level_scores(A, Cm, cov, entries=e, inc_continuous=1 if m else 0)
                _check(got, X, lev, Z, masks[e], A, Cm, cov)
    finally:
        ds.close()


def test_candidates(two):
    ds, X, lev, Z, masks = two
    rng = np.random.default_rng(61)
    A, Cm = factors(rng, (5, 3), 0, 12, X.shape[1])
    for cov in (0, 1):
        own = ds.level_scores(A, Cm, cov, entries="train")
        _same_bits(own, ds.level_scores(A, Cm, cov, entries="train", candidates=A[cov]))
        _same_bits(own, ds.level_scores(A, Cm, cov, entries="train", candidates=np.ascontiguousarray(A[cov])))
    for rows in (1, 33):
        cand = rng.standard_normal((rows, 12))
        for e in ENTRIES:
            got = ds.level_scores(A, Cm, 0, entries=e, candidates=cand)
            assert got["sse"].shape == (203, rows)
            _check(got, X, lev, Z, masks[e], A, Cm, 0, cand=cand)
            d = posthoc.ls_derived(got, None)
            assert d["confusion"] is None and np.all(d["best"][got["n"] > 0] >= 1)


def test_assigned_column_is_the_sample_decomposition_rss(two):
    """sse[i, assigned_i - 1] is sample_decomposition()'s rss[i] within the sum of the two calls' bounds (both 1e-12 of the same
    scale: with the assigned level's G the scale above is that call's sum (|x| + F)^2), and n agrees exactly."""
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(12), (5, 3), 0, 11, X.shape[1])
    rows = np.arange(203)
    for cov in (0, 1):
        for e in ENTRIES:
            got = ds.level_scores(A, Cm, cov, entries=e)
            sd = ds.sample_decomposition(A, Cm, entries=e)
            sc = _scale(X, lev, Z, masks[e], A, Cm, cov)[rows, lev[:, cov] - 1]
            assert np.array_equal(got["n"], sd["n"])
            err = np.abs(got["sse"][rows, lev[:, cov] - 1] - sd["rss"])
            assert np.all(err <= 2e-12 * sc), np.max(err / np.maximum(sc, 1e-300))


@pytest.mark.parametrize("cov", [0, 1])
def test_planted_swaps_are_found(cov):
    """X = U C + 0.5 noise with the true embeddings as A; ten samples carry a wrong label of ``cov`` in the levels the handle
    gets.  Every sample with a scored entry is assigned its true level and exactly the ten are flagged, on every entry set.  Two
    levels' fits differ per entry by a K = 6 dot product of standard normals (spread sqrt(12)) against noise of 0.5, over at
    least 15 entries: the relative gap between best and second is far above any rounding (above 8 in the host form)."""
    rng = np.random.default_rng(100 + cov)
    n, p, K, counts = 203, 157, 6, (5, 3)
    truth = levels(rng, n, counts)
    A, Cm = factors(rng, counts, 0, K, p)
    X = np.asfortranarray(sum(A[b][truth[:, b] - 1] for b in range(2)) @ Cm + 0.5 * rng.standard_normal((n, p)))
    tr, te = _masks(rng, n, p)
    swapped = rng.choice(np.setdiff1d(np.arange(n), (3, 5, 7)), size=10, replace=False)
    given = truth.copy(order="F")
    given[swapped, cov] = (truth[swapped, cov] - 1 + rng.integers(1, counts[cov], size=10)) % counts[cov] + 1
    assert np.all(given[swapped, cov] != truth[swapped, cov])
    ds = api.InsiderData(X, given, np.asfortranarray(tr, dtype=np.uint8), np.asfortranarray(te, dtype=np.uint8))
    try:
        for e in ENTRIES:
            d = posthoc.ls_derived(ds.level_scores(A, Cm, cov, entries=e), given[:, cov])
            live = d["n"] > 0
            assert sorted(np.flatnonzero(~live)) == sorted(EMPTY[e])
            assert np.array_equal(d["best"][live], truth[live, cov])
            assert np.all(d["best"][~live] == 0)
            assert sorted(np.flatnonzero(d["flagged"])) == sorted(swapped)
            assert d["confusion"].sum() == live.sum() and np.trace(d["confusion"]) == live.sum() - 10
            assert np.all(d["margin"][swapped] > 0.5) and np.all(d["margin"][live & ~d["flagged"]] == 0)
    finally:
        ds.close()


def test_argument_errors_leave_the_outputs_untouched(two):
    ds, X, lev, Z, masks = two
    n = X.shape[0]
    A, Cm = factors(np.random.default_rng(17), (5, 3), 0, 4, X.shape[1])

    def status(fn):
        with pytest.raises(_lib.InsiderError) as e:
            fn()
        return e.value.status

    assert status(lambda: ds.level_scores(A, Cm, 0, entries="held-out")) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, 2)) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, -1)) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, "tissue")) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, 0.5)) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, 0, inc_continuous=1)) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, 0, inc_continuous=2)) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, 0, candidates=np.zeros((0, 4)))) == _lib.ERR_ARG
    assert status(lambda: ds.level_scores(A, Cm, 0, candidates=np.zeros((3, 5)))) == _lib.ERR_ARG
    A64, C64 = factors(np.random.default_rng(1), (5, 3), 0, 64, X.shape[1])
    assert status(lambda: ds.level_scores(A64, C64, 0)) == _lib.ERR_UNSUPPORTED
    # the same checks inside the library (the C ABI called directly): sentinel-filled outputs stay as they are
    lib = _lib.load()
    _, Cw, Aptrs = ds._marshal(A, Cm, 4, 0)
    sse, cnt = np.full((n, 8), -7.0, order="F"), np.full(n, -7.0)
    cand = np.asfortranarray(np.ones((3, 4)))

    def call(K=4, inc=0, entries=1, cov=0, cnd=None, n_cand=0, s=sse, c=cnt, ptrs=Aptrs, cw=Cw, h=None):
        return lib.insider_hip_level_scores(ds._h if h is None else h, ptrs, _lib.ptr(cw), inc, K, entries, cov,
                                            None if cnd is None else _lib.ptr(cnd), n_cand,
                                            None if s is None else _lib.ptr(s), None if c is None else _lib.ptr(c))

    for kw in (dict(cov=-1), dict(cov=2), dict(cov=3), dict(entries=3), dict(entries=-1), dict(inc=1), dict(inc=2),
               dict(cnd=cand, n_cand=0), dict(cnd=cand, n_cand=-2), dict(n_cand=3), dict(s=None), dict(c=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
    _, Cw64, Aptrs64 = ds._marshal(A64, C64, 64, 0)
    assert call(K=64, ptrs=Aptrs64, cw=Cw64) == _lib.ERR_UNSUPPORTED
    assert np.all(sse == -7.0) and np.all(cnt == -7.0)
    assert call(cnd=cand, n_cand=3) == _lib.OK            # and the valid call fills exactly n x 3 and n
    assert np.all(sse[:, :3] >= 0) and np.all(sse[:, 3:] == -7.0) and np.array_equal(cnt, masks["train"].sum(axis=1))


def test_continuous_block_is_not_a_candidate_covariate():
    ds, X, lev, Z, masks = _data(40, 21, (3, 2), m=2, seed=9)
    try:
        A, Cm = factors(np.random.default_rng(2), (3, 2), 2, 3, X.shape[1])
        _, Cw, Aptrs = ds._marshal(A, Cm, 3, 1)
        sse, cnt = np.full((40, 3), -7.0, order="F"), np.full(40, -7.0)
        assert _lib.load().insider_hip_level_scores(ds._h, Aptrs, _lib.ptr(Cw), 1, 3, 1, 2, None, 0, _lib.ptr(sse),
                                                    _lib.ptr(cnt)) == _lib.ERR_ARG
        assert np.all(sse == -7.0) and np.all(cnt == -7.0)
        with pytest.raises(_lib.InsiderError) as e:
            ds.level_scores(A, Cm, 0)                     # a handle with continuous covariates needs inc_continuous = 1
        assert e.value.status == _lib.ERR_ARG
    finally:
        ds.close()


def test_clone_and_remask_score_their_own_masks(two):
    ds, X, lev, Z, masks = two
    A, Cm = factors(np.random.default_rng(21), (5, 3), 0, 30, X.shape[1])
    tr2, te2 = _masks(np.random.default_rng(77), *X.shape)
    cl = ds.clone()
    rm = ds.remask(np.asfortranarray(tr2, dtype=np.uint8), np.asfortranarray(te2, dtype=np.uint8))
    try:
        for e in ENTRIES:
            a = ds.level_scores(A, Cm, 0, entries=e)
            _same_bits(a, cl.level_scores(A, Cm, 0, entries=e))
            _same_bits(a, ds.level_scores(A, Cm, 0, entries=e))          # two calls in a row: identical bits
            _check(rm.level_scores(A, Cm, 0, entries=e), X, lev, Z, {"all": None, "train": tr2, "test": te2}[e], A, Cm, 0)
        _check(cl.level_scores(A, Cm, 1, entries="test"), X, lev, Z, masks["test"], A, Cm, 1)
    finally:
        cl.close()
        rm.close()


def test_fitted_object_and_command_line(tmp_path):
    """posthoc.level_scores() on the resident handles of a fitted object, and --level-scores of the command line, against the
    host yardstick on the written factors."""
    rng = np.random.default_rng(8)
    n, p = 120, 90
    conf = np.column_stack([rng.integers(1, 4, n), rng.integers(1, 3, n)]).astype(np.int32)
    data = rng.standard_normal((n, p))
    obj = api.insider(data, conf)
    obj["params"]["max_iter"] = 3
    api.fit(obj, latent_dimension=4, lambda_=1.0, alpha=0.2)
    try:
        d = posthoc.level_scores(obj, 1, which="fit", entries="train")
        A, Cm = list(obj["cfd_matrices"].values()), obj["column_factor"]
        mask = (obj["train_indicator"] | obj["test_indicator"]).astype(bool)
        _check(d, obj["data"], obj["confounder"], None, mask, A, Cm, 1)
        assert d["best"].shape == (n,) and d["confusion"].shape == (2, 2) and d["confusion"].sum() == n
    finally:
        close_resident(obj)
    from insider_amd import fit as fit_cli
    np.save(tmp_path / "X.npy", data)
    np.save(tmp_path / "L.npy", conf)
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--level-scores", "1",
                         "--level-score-entries", "all", "--rank", "4", "--lambda", "1", "--alpha", "0.2", "--max-iter", "3",
                         "--out", str(out)]) == 0
    A = [np.load(out / f"A{i}.npy") for i in range(2)]
    Cm = np.load(out / "C.npy")
    ref = posthoc.ls_derived(posthoc.level_scores_host(data, conf, None, None, A, Cm, 0), conf[:, 0])
    np.testing.assert_allclose(np.load(out / "ls_sse.npy"), ref["sse"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(np.load(out / "ls_n.npy"), ref["n"])
    assert np.array_equal(np.load(out / "ls_best.npy"), ref["best"])
    np.testing.assert_allclose(np.load(out / "ls_margin.npy"), ref["margin"], rtol=1e-6, atol=1e-9)
    assert np.array_equal(np.load(out / "ls_confusion.npy"), ref["confusion"])
