"""insider_hip_enrichment on the device against the numpy yardstick posthoc.enrichment_host().

Every call goes through ctypes with outputs prefilled with sentinels and NGUARD guard elements past R * S; the guards must
be unchanged after every call.

Where the arithmetic is exact (weight 0, and weight 1 with integer scores in -2..2: every prefix sum is an integer, every
deviation two correctly rounded divisions and one subtraction of integers) es, peak, n_ge, n_same and hits_nonzero must EQUAL
the yardstick's; sum_same adds up to nperm scores, so it agrees within nperm 2^-52 max|ES| (assert_exact).

With real-valued scores the bound is derived, not fitted: an m-term prefix sum of non-negative weights errs, in any order, by
at most m u of its value (u = 2^-53), normalised to P_i / N <= 1 that and the two divisions and the subtraction stay under
(m + 4) u, and tol = 4 (m + 4) 2^-52 covers the device's and the yardstick's error together.  A count may differ from the
yardstick's only by draws whose comparison the yardstick decides by less than that: every count must lie in the interval
the yardstick gives when its comparisons are moved by +-tol, and peak is compared where the runner-up deviation is more
than tol away.  So that the intervals test something, at most 10 % of the (profile, set) pairs may have an interval that is
not a single value; that share is asserted on the yardstick alone, before the device is looked at (the pairs that do sit
at m in {1, 2, p - 1}, where the scores fall on a lattice and equal |ES| are common)."""
import ctypes as C
import functools

import numpy as np
import pytest

from insider_amd import _lib, api, posthoc
from tests.support import bits, lib  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu

NGUARD = 7
OUTS = (("es", np.float64, 12345.678), ("peak", np.int32, -77), ("n_ge", np.int32, -78), ("n_same", np.int32, -79),
        ("sum_same", np.float64, 8765.4321), ("hits_nonzero", np.int32, -80))
EXACT = ("es", "peak", "n_ge", "n_same", "hits_nonzero")
M_LIST = (1, 2, 15, 63, 64, 65, 127, 128, 129, 300)
U = 2.0 ** -52


def call(lib, sc, ptr, genes, weight, nperm, seed=api.DEFAULT_SEED):
    """One guarded call.  sc: R x p row-major."""
    sc = np.ascontiguousarray(sc, dtype=np.float64)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    genes = np.ascontiguousarray(genes, dtype=np.int32)
    R, p = sc.shape
    S = ptr.size - 1
    outs = [np.full(R * S + NGUARD, fill, dtype=dt) for _, dt, fill in OUTS]
    status = lib.insider_hip_enrichment(_lib.ptr(sc), R, p, _lib.ptr(ptr, C.c_int64), _lib.ptr(genes, C.c_int32), S, weight,
                                        nperm, seed, 0,
                                        *[_lib.ptr(o, C.c_int32 if o.dtype == np.int32 else C.c_double) for o in outs])
    assert status == _lib.OK, (status, lib.insider_hip_last_error().decode(errors="replace"))
    for o, (_, _, fill) in zip(outs, OUTS):
        assert np.all(o[R * S:] == fill)
    return {name: o[:R * S].reshape(R, S) for o, (name, _, _) in zip(outs, OUTS)}


def csr(sets):
    return (np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64),
            np.concatenate(sets).astype(np.int32))


def make_sets(p, rng):
    """One set of every size of the table that fits (m < p), p - 1 (4096, the largest set the library takes, at p = 4099); then
    three more sets of one size: another one, a copy of it (identical sets) and one that shares half its genes with it
    (overlapping sets)."""
    sizes = [m for m in M_LIST if m < p] + [min(p - 1, api.ENRICH_MAX_SET)]
    sets = [rng.choice(p, m, replace=False) for m in dict.fromkeys(sizes)]
    m = 15 if p > 15 else 1
    base = rng.choice(p, m, replace=False)
    rest = np.setdiff1d(np.arange(p), base)
    sets += [base, base.copy()[::-1], np.concatenate([base[:m // 2], rng.choice(rest, m - m // 2, replace=False)])]
    return sets


# ---- 1. exact arithmetic ----------------------------------------------------------------------------------------------------
SHAPES = ((2, 1, 1), (3, 3, 64), (63, 17, 65), (64, 3, 200), (65, 1, 64), (257, 3, 200), (1000, 17, 64), (4099, 3, 65))


@functools.lru_cache(maxsize=None)
def exact_case(p, R, nperm):
    rng = np.random.default_rng(1000 + p)
    sc = rng.integers(-2, 3, (R, p)).astype(np.float64)
    if R >= 3:
        sc[1] = 0.0                                       # a profile that is all zeros
    ptr, genes = csr(make_sets(p, rng))
    return sc, ptr, genes


@functools.lru_cache(maxsize=None)
def exact_ref(p, R, nperm, weight):
    sc, ptr, genes = exact_case(p, R, nperm)
    return posthoc.enrichment_host(sc, ptr, genes, nperm=nperm, weight=weight, seed=77 + p, return_null=True)


def assert_exact(got, ref, nperm):
    """sum_same: the device and the yardstick add the draws' scores in draw order with a compensated sum, good to about an ulp
    of a sum of at most nperm terms of magnitude max|ES_b|, the largest score among the pair's draws."""
    for name in EXACT:
        assert np.array_equal(got[name], ref[name]), name
    for s in range(ref["size"].size):
        emax = np.abs(ref["null"][:, int(np.searchsorted(ref["null_sizes"], ref["size"][s]))]).max(axis=1)
        err = np.abs(got["sum_same"][:, s] - ref["sum_same"][:, s])
        assert np.all(err <= nperm * U * emax), (s, err.max(), emax)


@pytest.mark.parametrize("weight", [0, 1])
@pytest.mark.parametrize("p,R,nperm", SHAPES)
def test_exact_scores_equal_the_yardstick(lib, p, R, nperm, weight):
    """Integer scores in -2..2: ties everywhere (the tie rule of the ranking and of peak) and many zeros (sets and draws of
    all-zero weight fall back to w = 1)."""
    sc, ptr, genes = exact_case(p, R, nperm)
    ref = exact_ref(p, R, nperm, weight)
    assert_exact(call(lib, sc, ptr, genes, weight, nperm, seed=77 + p), ref, nperm)
    assert lib.insider_hip_last_enrichment_ms() > 0.0


def test_more_draws_than_one_chunk(lib):
    """nperm = 1030 and 2049: the draws' scores are counted in chunks of 1024 (GS_CHUNK), the counts carried between them."""
    rng = np.random.default_rng(12)
    p = 65
    sc = rng.integers(-2, 3, (3, p)).astype(np.float64)
    ptr, genes = csr([rng.choice(p, m, replace=False) for m in (1, 15, 15, 64)])
    for nperm in (1030, 2049):
        ref = posthoc.enrichment_host(sc, ptr, genes, nperm=nperm, weight=1, seed=5, return_null=True)
        assert_exact(call(lib, sc, ptr, genes, 1, nperm, seed=5), ref, nperm)


def test_more_pairs_than_blocks(lib):
    """R S = 1 050 000 (profile, set) pairs: k_gs_observed's grid stops at 2^20 blocks and strides over the rest."""
    rng = np.random.default_rng(13)
    p, R, S = 64, 1050, 1000
    sc = rng.integers(-2, 3, (R, p)).astype(np.float64)
    ptr, genes = csr([rng.choice(p, 1 + s % 2, replace=False) for s in range(S)])
    ref = posthoc.enrichment_host(sc, ptr, genes, nperm=2, weight=1, seed=6, return_null=True)
    assert_exact(call(lib, sc, ptr, genes, 1, 2, seed=6), ref, 2)


# ---- 2. real-valued scores, about 60 % exact zeros -------------------------------------------------------------------------
REAL_SHAPES = ((2, 1, 1), (3, 1, 64), (63, 1, 65), (64, 1, 200), (65, 1, 64), (257, 3, 65), (1000, 3, 200), (4099, 17, 65))


def ranking(sc):
    order = np.argsort(-sc, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(sc.shape[1]), sc.shape), axis=1)
    return rank, np.abs(np.take_along_axis(sc, order, axis=1))


def count_intervals(ref, r, s, tol):
    """[lower, upper] of n_same and n_ge of pair (r, s) when every comparison of the yardstick is moved by +-tol: both the
    observed score and a draw's may be off by tol, so a sign test moves by tol and |ES_b| >= |ES| by 2 tol."""
    z = int(np.searchsorted(ref["null_sizes"], ref["size"][s]))
    e, obs = ref["null"][r, z], ref["es"][r, s]
    e_pos, e_neg, o_pos, o_neg = e >= tol, e < -tol, obs >= tol, obs < -tol
    same_lo = (e_pos & o_pos) | (e_neg & o_neg)
    same_hi = ~((e_pos & o_neg) | (e_neg & o_pos))
    d = np.abs(e) - abs(obs)
    return ((int(same_lo.sum()), int(same_hi.sum())),
            (int((same_lo & (d >= 2 * tol)).sum()), int((same_hi & (d >= -2 * tol)).sum())),
            float(np.abs(e).max()))


@pytest.fixture(scope="module")
def real_refs():
    """The inputs, the yardstick's record with its null table and the count intervals of every shape, computed once; the
    share of pairs with an interval that is not one value is asserted here, on the yardstick alone."""
    cases, open_pairs, pairs = {}, 0, 0
    for p, R, nperm in REAL_SHAPES:
        rng = np.random.default_rng(2000 + p)
        sc = rng.standard_normal((R, p))
        sc[rng.random((R, p)) < 0.6] = 0.0
        ptr, genes = csr(make_sets(p, rng))
        ref = posthoc.enrichment_host(sc, ptr, genes, nperm=nperm, weight=1, seed=99 + p, return_null=True)
        iv = {}
        for r in range(R):
            for s in range(ptr.size - 1):
                tol = 4 * (int(ref["size"][s]) + 4) * U
                iv[r, s] = count_intervals(ref, r, s, tol)
                pairs += 1
                open_pairs += iv[r, s][0][0] != iv[r, s][0][1] or iv[r, s][1][0] != iv[r, s][1][1]
        cases[p] = (sc, ptr, genes, ref, iv)
    print(f"pairs with a count interval that is not one value: {open_pairs} of {pairs}")
    assert open_pairs <= 0.10 * pairs, (open_pairs, pairs)
    return cases


@pytest.mark.parametrize("p,R,nperm", REAL_SHAPES)
def test_real_scores_within_the_derived_bound(lib, real_refs, p, R, nperm):
    sc, ptr, genes, ref, iv = real_refs[p]
    got = call(lib, sc, ptr, genes, 1, nperm, seed=99 + p)
    rank, aw = ranking(sc)
    assert np.array_equal(got["hits_nonzero"], ref["hits_nonzero"])
    checked_peaks = 0
    for s in range(ptr.size - 1):
        m = int(ref["size"][s])
        tol = 4 * (m + 4) * U
        worst = np.abs(got["es"][:, s] - ref["es"][:, s]).max()
        assert worst <= tol, (s, m, worst, tol)
        T = np.sort(rank[:, genes[ptr[s]:ptr[s + 1]]], axis=1)
        dh, dl = posthoc.gs_deviations(aw, T, 1)
        for r in range(R):
            (s_lo, s_hi), (g_lo, g_hi), emax = iv[r, s]
            assert s_lo <= got["n_same"][r, s] <= s_hi, (r, s, m)
            assert g_lo <= got["n_ge"][r, s] <= g_hi, (r, s, m)
            assert abs(got["sum_same"][r, s] - ref["sum_same"][r, s]) <= nperm * tol + (s_hi - s_lo + nperm * U) * emax
            hi, lo = dh[r].max(), dl[r].min()
            side = np.sort(dh[r])[::-1] if hi >= -lo else np.sort(dl[r])
            if abs(hi + lo) > 2 * tol and (m == 1 or abs(side[0] - side[1]) > tol):
                assert got["peak"][r, s] == ref["peak"][r, s], (r, s, m)
                checked_peaks += 1
    # (how many peaks qualify is a property of the yardstick: at p <= 3 most deviations tie exactly)
    assert checked_peaks >= (0.5 * R * (ptr.size - 1) if p >= 63 else 1)


# ---- 3. invariance ----------------------------------------------------------------------------------------------------------
def test_subsets_repeats_and_seeds(lib):
    rng = np.random.default_rng(31)
    p, R, nperm = 257, 5, 65
    sc = rng.standard_normal((R, p))
    sc[rng.random((R, p)) < 0.6] = 0.0
    sets = make_sets(p, rng)
    ptr, genes = csr(sets)
    full = call(lib, sc, ptr, genes, 1, nperm, seed=3)
    names = [name for name, _, _ in OUTS]
    assert bits(call(lib, sc, ptr, genes, 1, nperm, seed=3), names) == bits(full, names)    # repeated calls: identical bytes
    rows = [3, 1]
    part = call(lib, sc[rows], ptr, genes, 1, nperm, seed=3)                                # some of the profiles
    for name, _, _ in OUTS:
        assert np.array_equal(part[name], full[name][rows]), name
    cols = [len(sets) - 1, 0, 4, len(sets) - 3, 7]                                          # some of the sets, reordered
    part = call(lib, sc, *csr([sets[c] for c in cols]), 1, nperm, seed=3)
    for name, _, _ in OUTS:
        assert np.array_equal(part[name], full[name][:, cols]), name
    other = call(lib, sc, ptr, genes, 1, nperm, seed=4)                                     # the seed only moves the null
    for name in ("es", "peak", "hits_nonzero"):
        assert np.array_equal(other[name], full[name]), name
    assert np.any(other["n_ge"] != full["n_ge"])


# ---- 4. the layers above ----------------------------------------------------------------------------------------------------
def test_planted_set_and_driver_records(lib, tmp_path):
    """A small fit through the driver with --gene-sets: its records are those of posthoc.factor_enrichment /
    level_enrichment on the factors it wrote; then a set planted on a factor's top-loaded genes gets that factor's smallest
    p-value."""
    from insider_amd import fit as fit_cli, flatio
    rng = np.random.default_rng(41)
    n, p, K, counts = 60, 200, 3, (3, 2)
    conf = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    Ct = rng.standard_normal((K, p)) * (rng.random((K, p)) < 0.3)
    At = [rng.standard_normal((L, K)) for L in counts]
    X = (At[0][conf[:, 0] - 1] + At[1][conf[:, 1] - 1]) @ Ct + 0.1 * rng.standard_normal((n, p))
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "L.npy", conf)
    names = [f"gene{j}" for j in range(p)]
    (tmp_path / "names.txt").write_text("".join(g + "\n" for g in names))
    random_sets = [rng.choice(p, m, replace=False) for m in (20, 20, 20, 20, 20, 8, 8, 30, 45, 45, 60, 3, 70)]
    (tmp_path / "sets.gmt").write_text("".join(f"set{i}\tna\t" + "\t".join(names[g] for g in s) + "\n"
                                                 for i, s in enumerate(random_sets)))
    out = tmp_path / "out"
    assert fit_cli.main(["--x", str(tmp_path / "X.npy"), "--levels", str(tmp_path / "L.npy"), "--rank", str(K), "--lambda", "0.5",
                         "--alpha", "0.2", "--max-iter", "30", "--gene-sets", str(tmp_path / "sets.gmt"), "--gene-names",
                         str(tmp_path / "names.txt"), "--enrich-perms", "100", "--enrich-min-size", "5", "--enrich-max-size",
                         "60", "--enrich-levels", "1", "--out", str(out)]) == 0
    kept = [i for i, s in enumerate(random_sets) if 5 <= len(s) <= 60]
    assert (out / "gs_set_names.txt").read_text().split() == [f"set{i}" for i in kept]
    Cm, A0 = np.load(out / "C.npy"), np.load(out / "A0.npy")
    sets = flatio.read_gmt(str(tmp_path / "sets.gmt"), names, min_size=5, max_size=60)
    assert list(np.load(out / "gs_size.npy")) == [len(random_sets[i]) for i in kept]
    for prefix, rec, rows in (("gs_factor", posthoc.factor_enrichment(Cm, sets, nperm=100), K),
                              ("gs_level1", posthoc.level_enrichment(A0, Cm, sets, nperm=100), counts[0])):
        assert rec["names"] == [f"set{i}" for i in kept]
        for key in ("es", "nes", "pval", "fdr", "peak"):
            got = np.load(out / f"{prefix}_{key}.npy")
            assert got.shape == (rows, len(kept))
            assert np.array_equal(got, rec[key], equal_nan=True), (prefix, key)
        assert np.all((rec["pval"] > 0) & (rec["pval"] <= 1)) and np.all(rec["fdr"] >= rec["pval"] - 1e-15)
    k = int(np.argmax(np.abs(Cm).sum(axis=1)))
    planted = np.argsort(-np.abs(Cm[k]), kind="stable")[:20]
    assert np.count_nonzero(Cm[k, planted]) > 0
    cand = [s for s in random_sets if len(s) >= 5] + [planted]
    rec = posthoc.factor_enrichment(Cm, csr(cand), nperm=200)
    last = len(cand) - 1
    # all the weight of the top 20 positions sits in the set: P_i / N reaches 1 at its last non-zero loading with nothing missed
    assert rec["es"][k, last] == 1.0 and rec["peak"][k, last] == np.count_nonzero(Cm[k, planted]) - 1
    assert rec["n_ge"][k, last] == 0
    assert rec["pval"][k, last] == rec["pval"][k].min()
    assert sorted(posthoc.leading_edge(rec, k, last)) == sorted(planted[:rec["peak"][k, last] + 1])
