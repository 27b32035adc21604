"""The streaming products (k_mm_rows2, k_mm_reduce2: from 16384 genes on) at the size edges only a large extent switches on.

a. Q = S A and Qheld = S^held A (launch_q, k_mm_rows2<NB, false>) through insider_hip_col_stats(), against the
   float64 reference and the bounds of test_gpu_col_stats.py: the partial last tile of 16 genes, both sides of MM_FAST_MIN,
   one / two / eight / nine / seventeen chunks of 16 stacked levels (the second trip of the S0 loop starts at the ninth), both
   sides of the LDS fit of the staged factors for every NB (past it: k_mm_rows at streaming size), NB = 3 and 4, and more than
   one tile per wave (option "mm_tiles", and the natural rule at 4 n_simd + 4 tiles).
b. V = C A' (launch_gene_v, k_mm_rows2<NT, true>) and U'C (launch_mm_reduce_kp, k_mm_reduce2<NB, LT>) through
   insider_hip_optimize_row(), against oracle.optimize_row at the bound of test_gpu_row_update.py: the K tails of the 16-byte row
   reads, more than one column block (grid.y > 1), every length of k_mm_reduce2's last slab, tiles per wave.
c. One fit with "mm_tiles" = 3: the side-stream launches of optimize() carry the option.

q_kernel() / tiles() / v_nt() / reduce2_form() (tests/dispatch_rules.py) are the dispatch written out by hand from the plan's
rules (mm_rows2_fits(), mm_tiles_per_wave(), reduce_form() in insider_plan.hpp) and launch_gene_v(); every case asserts
insider_hip_get_info("col_q_kernel" / "mm_rows2_tiles" / "row_kernels") before it compares values, so a dispatch edit fails
the case written for the old kernel.
"""
import numpy as np
import pytest

from insider_amd import api, workloads
from tests import test_gpu_col_stats as cs
from tests import test_gpu_row_update as ru
from tests.dispatch_rules import MM_FAST_MIN, MM_SLAB, nb_of, q_kernel, reduce2_form, tiles, v_nt
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_chunk(oracle):
    """One gene per OpenMP chunk, as in test_gpu_row_update.py."""
    oracle.set_col_chunk(1)
    yield
    oracle.set_col_chunk(100)


@pytest.fixture(scope="module")
def n_simd():
    w = workloads.small()
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        return int(ds.info("n_simd"))
    finally:
        ds.close()


# ----------------------------------------------------------------------------------------------------------------------
# a. Q = S A and Qheld
# ----------------------------------------------------------------------------------------------------------------------
def qcase(name, K, levels, p, n=48, mm_fast=1, mm_tiles=0):
    c = cs.case("sp-" + name, K, levels, p=p, n=n, f=0.2, walk=True)
    c.update(mm_fast=mm_fast, mm_tiles=mm_tiles)
    return c


QCASES = []
# the partial last tile: 1, 15 and 1 (mod 16) genes in it
QCASES += [qcase(f"tail-p{p}", 5, (30, 7), p) for p in (16385, 16399, 16401)]
# both sides of MM_FAST_MIN
QCASES += [qcase("below-min", 5, (30, 7), 16383), qcase("at-min", 5, (30, 7), 16384),
           qcase("at-min-mm0", 5, (30, 7), 16384, mm_fast=0)]
# chunks of 16 stacked levels: nchunk 1, 2, 8, 9, 17; SL mod 16 in {0, 1, 3, 13, 15}; odd SL (a pad column in the 16-byte reads)
QCASES += [qcase(f"SL{SL}", 5, (SL - 3, 3), 16389, n=max(48, SL + 8)) for SL in (13, 16, 17, 31, 33, 127, 128, 129, 131, 255, 257)]
# the LDS fit per NB: ceil(SL / 16) NB = 32 fits, the next SL falls back to k_mm_rows
FIT_EDGE = {9: 512, 20: 256, 40: 160, 63: 128}
for K, SL in FIT_EDGE.items():
    QCASES += [qcase(f"fit-K{K}-SL{s}", K, (s - 3, 3), 16389, n=s + 8) for s in (SL, SL + 1)]
# NB = 3 and 4 inside the band
QCASES += [qcase(f"NB-K{K}", K, (40, 20, 3), 16389) for K in (33, 47, 48, 49, 63)]
# tiles per wave: 1032 tiles, the last one partial; 1032 is no multiple of 5 or 7 (the last wave runs out inside its loop)
P_TILES = 16384 + 16 * 7 + 5
QCASES += [qcase(f"tiles{t}", 5, (30, 7), P_TILES, mm_tiles=t) for t in (2, 3, 5, 7)]
QCASE_BY_ID = {c["id"]: c for c in QCASES}
assert len(QCASE_BY_ID) == len(QCASES)

Q_WANT = {"sp-below-min": 1, "sp-at-min": 2, "sp-at-min-mm0": 1}
Q_WANT.update({f"sp-fit-K{K}-SL{SL}": 2 for K, SL in FIT_EDGE.items()})
Q_WANT.update({f"sp-fit-K{K}-SL{SL + 1}": 1 for K, SL in FIT_EDGE.items()})


def g_genes(c):
    """The genes G is compared on: all of them while p K^2 is small, else the first and last 64 and every 64th (<= 512)."""
    p = c["p"]
    if p * c["K"] ** 2 <= 2_000_000:
        return None
    g = np.unique(np.concatenate([np.arange(64), np.arange(0, p, 64), np.arange(p - 64, p)]))
    assert g.size <= 512
    return g


def run_q(c, n_simd, keep=None):
    """col_stats() under col_factored = 0 (Qfull alone) and, where the level structure has a count table, = 3 (Qheld too): the
    launch facts, then the values."""
    K, p, SL = c["K"], c["p"], sum(c["levels"])
    A = cs.factors(c, np.random.default_rng(c["seed"] + 1))
    genes = g_genes(c)
    want = q_kernel(K, SL, p, c["mm_fast"])
    assert Q_WANT.get(c["id"], 2) == want, c["id"]           # (the cases written for one side of an edge name it)
    assert cs.structure(c)[3], c["id"]                         # a count table exists
    ref = cs.reference(c, A, genes)
    try:
        for cf in (0, 3):
            cc = dict(c, opts=dict(col_factored=cf))
            ds = cs.handle(cc)
            try:
                ds.set_option("mm_fast", c["mm_fast"])
                ds.set_option("mm_tiles", c["mm_tiles"])
                assert (ds.info("col_q_kernel"), ds.info("mm_rows2_tiles")) == (0, 0)
                got = ds.col_stats(A)
                cs.check_launch(cc, ds)
                assert cs.expected(cc)[0] in (("list", "list4") if cf == 0 else ("paircnt", "paircnt4_ms4", "paircnt4_ms8"))
                assert ds.info("col_q_kernel") == want, (c["id"], cf, ds.info("col_q_kernel"))
                assert ds.info("mm_rows2_tiles") == (tiles(p, n_simd, c["mm_tiles"]) if want == 2 else 0), (c["id"], cf)
            finally:
                ds.close()
            cs.check_values(cc, got, A, f"col_factored {cf}", genes=genes, ref=ref)
            if keep is not None:
                keep[cf] = got
    finally:
        cs._DATA.pop(c["id"], None)       # (these data sets are large: not kept for the session)


@pytest.mark.parametrize("cid", list(QCASE_BY_ID))
def test_q_products(cid, n_simd):
    run_q(QCASE_BY_ID[cid], n_simd)


def test_q_two_tiles_per_wave_equal_one_by_bits(n_simd):
    """A tile's sums do not depend on the wave that takes it."""
    one, two = {}, {}
    run_q(qcase("tiles1", 5, (30, 7), P_TILES, mm_tiles=1), n_simd, one)
    run_q(qcase("tiles1", 5, (30, 7), P_TILES, mm_tiles=2), n_simd, two)
    for cf in (0, 3):
        for x, y in zip(one[cf], two[cf]):
            assert np.array_equal(x, y), cf


def test_q_natural_rule_two_tiles_per_wave(n_simd):
    """4 n_simd + 4 tiles, the last one partial: mm_tiles_per_wave() gives 2 with the option at its default."""
    p = 16 * (4 * n_simd + 3) + 5
    assert p >= MM_FAST_MIN
    c = qcase("natural", 5, (10, 3), p, n=24)
    assert tiles(p, n_simd) == 2
    run_q(c, n_simd)


# ----------------------------------------------------------------------------------------------------------------------
# b. V = C A' and U'C
# ----------------------------------------------------------------------------------------------------------------------
def rcase(name, K, levels, p, covs=(0,), n=48, mm_fast=1, mm_tiles=0):
    c = ru.case("sp-" + name, K, levels, p=p, n=n, opts=dict(row_merged=2, mm_fast=mm_fast), f=0.15, covs=covs)
    c["mm_tiles"] = mm_tiles
    return c


RCASES = []
# the K tails of the 16-byte reads of C's rows (pitch KP): NT = 4 (63 stacked levels), and NT = 2 / 1 (23 / 11)
for K in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63):
    RCASES.append(rcase(f"K{K}", K, (40, 20, 3), 16389, covs=(0, 1, 2) if K <= 17 else (0,)))
for K in (1, 17, 63):
    RCASES += [rcase(f"K{K}-nt2", K, (20, 3), 16389), rcase(f"K{K}-nt1", K, (8, 3), 16389)]
# more than one block of 64 columns of V: grid.y = 2 and 3
for L in (70, 130):
    RCASES += [rcase(f"L{L}-K{K}", K, (L, 4), 16389, n=2 * L + 40) for K in (9, 24)]
# tiles per wave on the V site
RCASES += [rcase(f"tiles{t}-K{K}", K, (40, 20, 3), 16501, mm_tiles=t) for t in (2, 3, 7) for K in (5, 33)]
RCASE_BY_ID = {c["id"]: c for c in RCASES}
assert len(RCASE_BY_ID) == len(RCASES)

# the last slab of k_mm_reduce2 (MM_SLAB = 128 genes): r genes in it
SLAB_R = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65, 127)
SLAB = [(r, 9, (0, 1)) for r in SLAB_R] + [(r, 40, (0,)) for r in (1, 17, 33, 49)]


def run_row(oracle, c, n_simd, opts=None, refs=None):
    """optimize_row() of each covariate on a fresh handle: the kernel forms, the tile count, then the oracle (refs: its results
    by covariate, kept for a second run on the same data).  Returns the updated factors by covariate."""
    w, Mtr, Mte, A, C, Z, U = ru.data(c)
    refs = {} if refs is None else refs
    cc = dict(c, opts={**c["opts"], **(opts or {})})
    out = {}
    for cov in c["covs"]:
        want = ru.expected(cc, cov)
        assert "mm_rows2" in want
        ds = ru.handle(cc, w, Mtr, Mte, Z)
        try:
            ds.set_option("mm_tiles", c["mm_tiles"])
            got = ds.optimize_row(ru.factors(A, U), C, cov, lambda_=c["lam"], tuning=1)
            assert ru.launched(ds) == want, (cov, sorted(ru.launched(ds)), sorted(want))
            assert ds.info("mm_rows2_tiles") == tiles(c["p"], n_simd, c["mm_tiles"])
        finally:
            ds.close()
        if cov not in refs:
            refs[cov] = ru.reference(oracle, c, w, Mtr, A, C, Z, U, cov)
        err = relerr(got, refs[cov])
        print(f"\n{c['id']} cov {cov}: relerr {err:.3e}")
        assert err < 1e-9, (cov, err)
        out[cov] = got
    return out


@pytest.mark.parametrize("cid", list(RCASE_BY_ID))
def test_row_products(oracle, cid, n_simd):
    run_row(oracle, RCASE_BY_ID[cid], n_simd)


@pytest.mark.parametrize("r,K,covs", SLAB, ids=[f"r{r}-K{K}" for r, K, _ in SLAB])
def test_reduce2_last_slab(oracle, r, K, covs, n_simd):
    c = rcase(f"slab-r{r}-K{K}", K, (40, 20, 3), MM_FAST_MIN + r, covs=covs)
    assert c["p"] % MM_SLAB == r
    forms = {cov: reduce2_form(K, c["levels"][cov], c["p"]) for cov in covs}
    assert forms == ({0: (1, 4), 1: (1, 2)} if K == 9 else {0: (3, 2)})
    refs = {}
    one = run_row(oracle, c, n_simd, refs=refs)
    # mm_fast = 2: two column tiles per wave instead of four; the same products in the same order (insider_mm.hpp)
    assert reduce2_form(K, 40, c["p"], mm_fast=2) == (nb_of(K), 2)
    two = run_row(oracle, c, n_simd, opts=dict(mm_fast=2), refs=refs)
    for cov in covs:
        assert np.array_equal(one[cov], two[cov]), (cov, relerr(one[cov], two[cov]))


# ----------------------------------------------------------------------------------------------------------------------
# c. one fit: the side-stream launches of optimize() carry "mm_tiles"
# ----------------------------------------------------------------------------------------------------------------------
FIT = dict(K=20, levels=(130, 20, 3), p=16421, n=140, mm_tiles=3)


def test_fit_with_three_tiles_per_wave(oracle, n_simd):
    """Tolerances: test_gpu_parity.py::test_streaming_products_and_ticketed_statistics_vs_oracle_and_round4."""
    w = workloads.small(seed=77, n=FIT["n"], p=FIT["p"], level_counts=FIT["levels"], K=FIT["K"], f=0.15)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    try:
        for k, v in dict(row_merged=2, col_factored=3, row_counts=1, mm_tiles=FIT["mm_tiles"]).items():
            ds.set_option(k, v)
        got = ds.optimize([a.copy(order="F") for a in w.A0], w.C0.copy(order="F"), w.K, w.lam, w.lam, w.alpha, tuning=1,
                          max_iter=3, seed=4)
        assert ds.profile()["col_pair"] and ds.profile()["row_merged"]
        assert ds.info("col_q_kernel") == q_kernel(FIT["K"], sum(FIT["levels"]), FIT["p"]) == 2
        assert ds.info("mm_rows2_tiles") == 3
        assert {"mm_rows2", "mm_reduce2_4", "mm_reduce2_2", "gram_side"} <= ru.launched(ds)
    finally:
        ds.close()
    ref = oracle.optimize(w.X, w.levels, w.n_levels, w.A0, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, tuning=1,
                          max_iter=3, seed=4)
    assert got["iters"] == ref["iters"]
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-8, equal_nan=True)
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-6
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-6, i


# ----------------------------------------------------------------------------------------------------------------------
# every template instance the dispatch can launch is expected of some case
# ----------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_named():
    reached = {}

    def note(key, cid):
        reached.setdefault(key, []).append(cid)

    for c in QCASES:
        if q_kernel(c["K"], sum(c["levels"]), c["p"], c["mm_fast"]) == 2:
            note(f"k_mm_rows2<{nb_of(c['K'])}, false>", c["id"])
    rows = [(c, c["covs"]) for c in RCASES] + \
           [(rcase(f"slab-r{r}-K{K}", K, (40, 20, 3), MM_FAST_MIN + r, covs=covs), covs) for r, K, covs in SLAB]
    for c, covs in rows:
        note(f"k_mm_rows2<{v_nt(sum(c['levels']))[0]}, true>", c["id"])      # optimize_row(): V of every stacked level
        for cov in covs:
            for mm in (1, 2) if "slab" in c["id"] else (1,):
                f = reduce2_form(c["K"], c["levels"][cov], c["p"], mm)
                if f:
                    note(f"k_mm_reduce2<{f[0]}, {f[1]}>", f"{c['id']}:cov{cov}" + (":mm2" if mm == 2 else ""))
    # the fit: V of covariates 1.. first, then of each covariate but the last after its update; U'C of every covariate
    L = FIT["levels"]
    for N in [sum(L[1:])] + list(L[:-1]):
        note(f"k_mm_rows2<{v_nt(N)[0]}, true>", "fit")
    for l in L:
        f = reduce2_form(FIT["K"], l, FIT["p"])
        if f:
            note(f"k_mm_reduce2<{f[0]}, {f[1]}>", "fit")
    note(f"k_mm_rows2<{nb_of(FIT['K'])}, false>", "fit")
    want = [f"k_mm_rows2<{nb}, false>" for nb in (1, 2, 3, 4)] + [f"k_mm_rows2<{nt}, true>" for nt in (1, 2, 4)] + \
           [f"k_mm_reduce2<{nb}, 2>" for nb in (1, 2, 3, 4)] + [f"k_mm_reduce2<{nb}, 4>" for nb in (1, 2)]
    print("\ntemplate instances and the cases that reach them:")
    for key in want:
        print(f"  {key:24s} {len(reached.get(key, [])):4d}  {' '.join(reached.get(key, [])[:4])}")
    assert set(reached) == set(want), sorted(set(want) ^ set(reached))
    assert {v_nt(sum(c["levels"])) for c in RCASES} >= {(1, 1), (2, 1), (4, 1), (4, 2), (4, 3)}     # grid.y of V
