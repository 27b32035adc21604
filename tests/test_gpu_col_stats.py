"""Every column-statistics kernel form that launch_col_stats() can launch, against a float64 reference.

The column solve reads one record per gene: the training Gram XtX_j, the complement X'r and, in its corner, the sum of x^2
over the entries that are not training entries.  launch_col_stats() forms it with one of k_list_stats<NB> / k_list_stats4
(the held-out lists), k_col_factored (look-up form), k_col_paircnt (pair-count form, with or without real-valued counts of
the continuous covariates) or k_col_paircnt4 (the same with its second product on the 4x4x4 matrix instruction, MAXS = 4 or
8 k-steps, genes dealt by ticket from one or sixteen counters).  insider_hip_col_stats() (InsiderData.col_stats) runs the
first half of a column update and returns the record densified; insider_hip_get_info("col_stats_kernel" /
"col_stats_tickets" / "col_stats_blocks") reports what ran.  expected() is the dispatch written out by hand
(tests/dispatch_rules.py: col_structure(), col_stats_kernel(), check_pc4_blocks()) from the call's plan (col_stats_path(),
paircnt_plan(), list_stats4() in insider_plan.hpp) and stage_factored(): every case asserts the kernel it reached before it
compares values, so that a dispatch edit cannot quietly move a case onto another kernel.

Covered: every code at the K band edges, the covariate structures (c = 1, 8, 9, tied level counts, the largest covariate
first / in the middle / last), both sides of every fit boundary (look-up table, k-steps, k_col_paircnt4's LDS, the one-byte
count cell, k_col_factored's staged indices), continuous covariates, the ticket dealing (one and sixteen counters, blocks
that walk the genes, p >= 16384), stale records across launches on one workspace and on a clone, and one fit per form that
the parity tests do not reach.
"""
import numpy as np
import pytest

from insider_amd import _lib, api
from tests import dispatch_rules as dr
from tests.dispatch_rules import COL_OPTS as OPTS
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

CODE = {name: i for i, name in enumerate(_lib.COL_STATS_KERNELS)}
NAME = dict(enumerate(_lib.COL_STATS_KERNELS))


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch, by hand (tests/dispatch_rules.py) on this file's data
# ----------------------------------------------------------------------------------------------------------------------
def structure(c):
    """What stage_merged() / stage_factored() / stage_cont_factored() decide for a case's data set."""
    return dr.col_structure(c, max_cell(c))


def expected(c):
    """(col_stats_kernel, col_stats_tickets) of one col_stats() call on the case's handle."""
    return dr.col_stats_kernel(c, structure(c))


# ----------------------------------------------------------------------------------------------------------------------
# the data
# ----------------------------------------------------------------------------------------------------------------------
def case(name, K, levels, p=61, n=150, m=0, f=0.25, opts=None, cost=None, na=False, grid=False, walk=False, seed=None):
    return dict(id=name, K=K, levels=tuple(levels), p=p, n=n, m=m, f=f, opts=opts or {}, cost=cost, na=na, grid=grid,
                walk=walk, seed=seed if seed is not None else (K * 131 + p * 7 + n + sum(levels) * 3 + m) % 100003)


_DATA = {}


def data(c):
    """X, 1-based level table, masks and continuous columns of a case.  Special genes: 0 has no held-out entry, 1 is wholly
    held out (test entries and, with na, NA entries), 2 keeps every sample of level 1 of covariate 0 in training; with na,
    5 % of the other entries are NA (neither train nor test) and keep a non-zero x, which the record's corner counts."""
    if c["id"] in _DATA:
        return _DATA[c["id"]]
    rng = np.random.default_rng(c["seed"])
    n, p, levels = c["n"], c["p"], c["levels"]
    if c["grid"]:      # level t of sample i = (i / prod(L_<t)) mod L_t: every joint count is n / prod(L) exactly
        stride = np.cumprod((1,) + levels[:-1])
        lev = np.stack([(np.arange(n) // s) % L for s, L in zip(stride, levels)], axis=1)
    else:              # every level present, counts as even as n allows
        lev = np.stack([rng.permutation(np.arange(n) % L) for L in levels], axis=1)
    lev = np.asfortranarray(lev + 1, dtype=np.int32)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    held = rng.random((n, p)) < c["f"]
    na = (rng.random((n, p)) < 0.05) & held if c["na"] else np.zeros((n, p), bool)
    if p >= 3:
        held[:, 0] = False
        na[:, 0] = False
        held[:, 1] = True
        na[:, 1] = c["na"] & (np.arange(n) % 3 == 0)
        held[lev[:, 0] == 1, 2] = False
        na[:, 2] &= held[:, 2]
    Mtr = np.asfortranarray(~held, dtype=np.uint8)
    Mte = np.asfortranarray(held & ~na, dtype=np.uint8)
    Z = np.asfortranarray(rng.standard_normal((n, c["m"]))) if c["m"] else None
    _DATA[c["id"]] = (lev, X, Mtr, Mte, Z)
    return _DATA[c["id"]]


def max_cell(c):
    """The largest dense pair count of any gene: held-out samples of one level of a covariate and one level of another (when
    no gene holds more than 255 held-out entries: that number, a bound)."""
    lev, X, Mtr, Mte, Z = data(c)
    held = Mtr == 0
    if held.sum(0).max() <= 255 or len(c["levels"]) < 2:
        return int(held.sum(0).max()) if len(c["levels"]) >= 2 else 0
    best = 0
    for a in range(len(c["levels"])):
        for b in range(a + 1, len(c["levels"])):
            cell = (lev[:, a] - 1) * c["levels"][b] + (lev[:, b] - 1)
            for j in np.nonzero(held.sum(0) > 255)[0]:
                best = max(best, int(np.bincount(cell[held[:, j]]).max()))
    return best


def factors(c, rng):
    K = c["K"]
    A = [np.asfortranarray(rng.standard_normal((L, K)) * 0.5) for L in c["levels"]]
    if c["m"]:
        A.append(np.asfortranarray(rng.standard_normal((c["m"], K)) * 0.3))
    return A


def reference(c, A, genes=None):
    """G, q, ss of every gene in float64, and the scales of the bounds: ||R'R||, ||X'R|| per gene, sum x^2 per gene.  genes: the
    genes G is formed for (a large p: K^2 doubles per gene); q, ss and the scales are always those of every gene."""
    lev, X, Mtr, Mte, Z = data(c)
    ncov = len(c["levels"])
    R = sum(A[t][lev[:, t] - 1] for t in range(ncov))
    if c["m"]:
        R = R + Z @ A[ncov]
    T = Mtr.astype(np.float64)
    G = np.einsum("ij,ik,il->jkl", T if genes is None else T[:, genes], R, R)
    q = np.einsum("ij,ik->jk", T * X, R)
    ss = ((1.0 - T) * X * X).sum(0)
    return G, q, ss, np.linalg.norm(R.T @ R), np.linalg.norm(X.T @ R, axis=1), (X * X).sum(0)


def handle(c):
    lev, X, Mtr, Mte, Z = data(c)
    ds = api.InsiderData(X, lev, Mtr, Mte, n_levels=np.array(c["levels"], dtype=np.int32), ctns_confounder=Z)
    for k, v in {**OPTS, **c["opts"]}.items():
        ds.set_option(k, v)
    return ds


def check_values(c, got, A, tag="", genes=None, ref=None):
    """genes: compare G on these genes only (reference(c, A, genes)); ref: that reference, when the caller has it already."""
    G, q, ss = got
    Gr, qr, ssr, sG, sq, sx = ref if ref is not None else reference(c, A, genes)
    if genes is not None:
        G = G[genes]
    # every form but the lists builds train = full - complement: the bounds scale with the full products
    eG = np.linalg.norm(G - Gr, axis=(1, 2))
    assert np.all(eG <= 1e-12 * sG), (tag, int(np.argmax(eG / sG)), float(np.max(eG / sG)))
    eq = np.linalg.norm(q - qr, axis=1)
    assert np.all(eq <= 1e-12 * sq), (tag, int(np.argmax(eq / sq)), float(np.max(eq / sq)))
    es = np.abs(ss - ssr)
    assert np.all(es <= 1e-12 * sx), (tag, int(np.argmax(es / sx)), float(np.max(es / sx)))


def launched(ds):
    return NAME[int(ds.info("col_stats_kernel"))], int(ds.info("col_stats_tickets")), int(ds.info("col_stats_blocks"))


def check_launch(c, ds):
    kernel, tickets, blocks = launched(ds)
    want_k, want_t = expected(c)
    assert kernel == want_k, (c["id"], kernel, want_k)
    assert tickets == want_t, (c["id"], tickets, want_t)
    dr.check_pc4_blocks(c, kernel, tickets, blocks)


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
KS = [1, 14, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 49, 62, 63]
PS = [61, 64, 77, 60, 65]
CASES = []
for i, K in enumerate(KS):
    p, na = PS[i % len(PS)], K % 2 == 1
    CASES += [case(f"K{K}-lists", K, (60, 7), p=p, na=na, opts=dict(col_factored=0)),
              case(f"K{K}-lookup", K, (60, 7), p=p, na=na, opts=dict(col_factored=2)),
              case(f"K{K}-pair", K, (60, 7), p=p, na=na, opts=dict(col_factored=3, col_mfma4=0)),
              case(f"K{K}-pair-s5", K, (60, 20), p=p, na=not na, opts=dict(col_factored=3, col_mfma4=0)),
              case(f"K{K}-ctns2", K, (30, 7), p=p, m=2, na=na)]
    if 16 <= K <= 31:
        CASES.append(case(f"K{K}-lists-coarse", K, (60, 7), p=p, na=na, opts=dict(col_factored=0, list_fine=0)))
    if K <= 31:
        CASES += [case(f"K{K}-pair4", K, (60, 7), p=p, na=na, opts=dict(col_factored=3)),
                  case(f"K{K}-pair4-s5", K, (60, 20), p=p, na=not na, opts=dict(col_factored=3)),
                  case(f"K{K}-ctns2-nomfma4", K, (30, 7), p=p, m=2, na=na, opts=dict(col_mfma4=0))]
# covariate structure: one covariate (no count product), eight, nine (the lists), tied level counts, the largest covariate
# first, in the middle and last (the table skips its rows: tab_skip_lo = 0, 7, 12)
STRUCT = {"c1": (60,), "c8": (5, 4, 3, 3, 2, 2, 2, 2), "c9": (5, 4, 3, 3, 2, 2, 2, 2, 2), "tied": (10, 10, 6),
          "tied-later": (6, 10, 10), "big-first": (40, 7, 5), "big-middle": (7, 40, 5), "big-last": (7, 5, 40)}
for s, lv in STRUCT.items():
    for K in (9, 20, 40):
        CASES += [case(f"{s}-K{K}-lookup", K, lv, p=65, na=True, opts=dict(col_factored=2)),
                  case(f"{s}-K{K}-pair", K, lv, p=65, opts=dict(col_factored=3, col_mfma4=0))]
        if K <= 31:
            CASES.append(case(f"{s}-K{K}-pair4", K, lv, p=65, na=True, opts=dict(col_factored=3)))
# fit boundaries, both sides of each
CASES += [
    # the look-up table at KP = 32 (tab_rows 157 / 158) and KP = 64 (78 / 79): too many rows for a count table, so col_factored
    # = 2 falls back to the lists
    case("lookup-fits-kp32", 31, (160, 157), n=320, opts=dict(col_factored=2)),
    case("lookup-full-kp32", 31, (160, 158), n=320, opts=dict(col_factored=2)),
    case("lookup-full-kp32-coarse", 20, (160, 158), n=320, opts=dict(col_factored=2, list_fine=0)),
    case("lookup-fits-kp64", 63, (80, 78), n=200, opts=dict(col_factored=2)),
    case("lookup-full-kp64", 49, (80, 79), n=200, opts=dict(col_factored=2)),
    # k-steps of the count product: 16 / 17 table rows (MAXS 4 / 8) and 32 / 33 (33: no count table, col_factored = 3 takes
    # the look-up form)
    case("steps4", 9, (40, 16), opts=dict(col_factored=3)), case("steps5", 9, (40, 17), opts=dict(col_factored=3)),
    case("steps8", 20, (40, 32), opts=dict(col_factored=3)), case("steps9", 20, (40, 33), opts=dict(col_factored=3)),
    case("steps8-K40", 40, (40, 32), opts=dict(col_factored=3)),
    case("steps4-ctns", 9, (40, 16), m=2), case("steps5-ctns", 9, (40, 17), m=2),
    case("steps5-ctns-K20", 20, (40, 17), m=3),
    # k_col_paircnt4's LDS at KP = 32: nsteps + quads = 4 + 43 = 47 fits, 4 + 44 = 48 does not (k_col_paircnt)
    case("pc4-lds-fits", 20, (152, 16), n=320, opts=dict(col_factored=3)),
    case("pc4-lds-full", 20, (156, 16), n=320, opts=dict(col_factored=3)),
    # one-byte count cells: gene 1 (wholly held out) has 255 samples in every (level, level) cell, then 256 (the build's
    # overflow flag: no count table, col_factored = 3 takes the look-up form)
    case("cell255", 9, (2, 2), n=1020, p=16, grid=True, opts=dict(col_factored=3)),
    case("cell255-K20", 20, (2, 2), n=1020, p=16, grid=True, opts=dict(col_factored=3, col_mfma4=0)),
    case("cell256", 9, (2, 2), n=1024, p=16, grid=True, opts=dict(col_factored=3)),
    # k_col_factored's staged look-up indices: gene 1 holds 1100 entries x 2 later covariates > CF_CAP = 2048 (read from
    # memory), the others ~330 x 2 (staged)
    case("cf-cap", 9, (40, 6, 5), n=1100, f=0.3, na=True, opts=dict(col_factored=2)),
    case("cf-cap-K40", 40, (40, 6, 5), n=1100, f=0.3, opts=dict(col_factored=2)),
]
# continuous covariates: m = 1..4 on the pair-count form; m = 5 has no merged tables (the lists)
for m in (1, 2, 3, 4, 5):
    for K in (7, 20, 40):
        CASES.append(case(f"ctns{m}-K{K}", K, (30, 7), p=64, m=m, na=m % 2 == 0))
# the cost model (col_factored = 1, the default), pinned by hand: E = held-out list entries per gene (padded to 32)
#   K9 (60, 7), n 150, f 0.25, E ~ 48:  list 16 E ~ 770    < 1.3 pair 3055, 1.3 look-up 5720          -> lists
#   K9 (8, 4), n 1000, f 0.5, E ~ 520:  1.3 pair 723       < 1.3 look-up 2546 < list 8300             -> pair count
#   K40 (8, 4), n 1000, f 0.5:          1.3 pair 2886      < 1.3 look-up 6074 < list 50000            -> pair count (NB 3)
#   K9 (40, 40), n 1000, f 0.5:         1.3 look-up 4534   < list 8300; no count table (40 rows)      -> look-up
#   K9 (60,), n 400, f 0.5, E ~ 200:    1.3 look-up 1248   < 1.3 pair 2028 < list 3200                -> look-up
#   K20 (60,), n 150, f 0.25, E ~ 48:   list 3 x 16 E ~ 2300 < 1.3 look-up 3744                       -> lists
COST = [case("cost-list", 9, (60, 7), cost="list"), case("cost-pair", 9, (8, 4), n=1000, f=0.5, cost="pair"),
        case("cost-pair-K40", 40, (8, 4), n=1000, f=0.5, cost="pair"),
        case("cost-lookup", 9, (40, 40), n=1000, f=0.5, cost="lookup"),
        case("cost-lookup-c1", 9, (60,), n=400, f=0.5, cost="lookup"),
        case("cost-list-K20", 20, (60,), cost="list")]
CASES += COST
# ticket dealing of k_col_paircnt4: one counter up to p = 60 (15 blocks), sixteen from p = 61, partitions of
# cap = ceil(p / 16) = 4, 4, 5, 5 genes; p = 3300 is more than four genes per resident wave at three blocks per CU (256 CUs:
# 768 blocks, 3072 genes) and p = 16400 (Qheld on k_mm_rows2) more again: the blocks walk
for p in (1, 3, 60, 61, 64, 65, 77):
    CASES.append(case(f"tickets-p{p}", 9, (30, 7), p=p, opts=dict(col_factored=3)))
CASES += [case("tickets-walk", 9, (30, 7), p=3300, n=40, opts=dict(col_factored=3), walk=True),
          case("tickets-walk-ms8-K20", 20, (12, 10, 8), p=3300, n=48, opts=dict(col_factored=3), walk=True),
          case("tickets-p16400", 5, (30, 7), p=16400, n=48, f=0.2, opts=dict(col_factored=3), walk=True)]
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


@pytest.mark.parametrize("cid", list(CASE_BY_ID))
def test_col_stats_every_kernel(cid):
    c = CASE_BY_ID[cid]
    A = factors(c, np.random.default_rng(c["seed"] + 1))
    ds = handle(c)
    try:
        assert launched(ds) == ("none", 0, 0)
        got = ds.col_stats(A, inc_continuous=1 if c["m"] else 0)
        check_launch(c, ds)
    finally:
        ds.close()
    check_values(c, got, A)


def test_every_code_is_reached():
    """Every code but "none" is expected of some case (and each case asserts what it reached)."""
    reached = {}
    for c in CASES:
        reached.setdefault(expected(c)[0], []).append(c["id"])
    print("\ncol_stats_kernel codes and the cases that reach them:")
    for name in _lib.COL_STATS_KERNELS:
        print(f"  {name:16s} {len(reached.get(name, [])):4d}  {' '.join(reached.get(name, [])[:4])}")
    assert set(reached) == set(_lib.COL_STATS_KERNELS) - {"none"}, sorted(set(_lib.COL_STATS_KERNELS) - set(reached))
    assert {expected(c)[1] for c in CASES if expected(c)[0].startswith("paircnt4")} == {1, 16}


# ----------------------------------------------------------------------------------------------------------------------
# stale records: a gene the tickets skip keeps the previous launch's record
# ----------------------------------------------------------------------------------------------------------------------
STALE = [case("stale-p77", 9, (30, 7), p=77, opts=dict(col_factored=3)),
         case("stale-p60", 9, (30, 7), p=60, opts=dict(col_factored=3)),
         case("stale-p65-zt", 9, (30, 7), p=65, m=2),
         case("stale-walk", 9, (30, 7), p=3300, n=40, opts=dict(col_factored=3), walk=True)]


@pytest.mark.parametrize("c", STALE, ids=[c["id"] for c in STALE])
def test_col_stats_fresh_records_every_launch(c):
    rng = np.random.default_rng(c["seed"] + 7)
    inc = 1 if c["m"] else 0
    ds = handle(c)
    try:
        for rep in range(3):        # three launches on one workspace: the ticket base advances
            A = factors(c, rng)
            got = ds.col_stats(A, inc_continuous=inc)
            check_launch(c, ds)
            check_values(c, got, A, f"rep {rep}")
        other = ds.clone()          # a workspace of its own: its own counters and records
        try:
            for rep in range(3):
                for h in (other, ds, other) if rep % 2 else (ds, other):
                    A = factors(c, rng)
                    got = h.col_stats(A, inc_continuous=inc)
                    check_launch(c, h)
                    check_values(c, got, A, f"interleaved {rep} {'clone' if h is other else 'handle'}")
        finally:
            other.close()
    finally:
        ds.close()


# ----------------------------------------------------------------------------------------------------------------------
# fits through the forms the parity tests do not reach: NB = 3 look-up and pair-count, real-valued counts with 5 k-steps
# ----------------------------------------------------------------------------------------------------------------------
FITS = [case("fit-lookup-K40", 40, (60, 7), p=64, na=True, opts=dict(col_factored=2)),
        case("fit-pair-K40", 40, (60, 7), p=64, opts=dict(col_factored=3)),
        case("fit-pair-zt-steps5", 9, (30, 17), p=64, m=2, na=True)]


@pytest.mark.parametrize("c", FITS, ids=[c["id"] for c in FITS])
def test_fit_one_iteration_new_forms(oracle, c):
    lev, X, Mtr, Mte, Z = data(c)
    rng = np.random.default_rng(c["seed"] + 3)
    A = [a * 0.6 for a in factors(c, rng)]
    C = np.asfortranarray(rng.standard_normal((c["K"], c["p"])) * 0.3)
    inc = 1 if c["m"] else 0
    ds = handle(c)
    try:
        got = ds.optimize([a.copy(order="F") for a in A], C.copy(order="F"), c["K"], 2.0, 2.0, 0.4, max_iter=0, seed=17,
                          inc_continuous=inc)
        check_launch(c, ds)
    finally:
        ds.close()
    ref = oracle.optimize(X, lev, np.array(c["levels"]), A, C, Mtr, Mte, 2.0, 2.0, 0.4, max_iter=0, seed=17, row_threads=8,
                          col_threads=16, **(dict(ctns=Z) if c["m"] else {}))
    assert got["iters"] == ref["iters"]
    for i, a in enumerate(ref["row_matrices"]):
        assert relerr(got["row_matrices"][f"factor{i}"], a) < 1e-9, i
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-9
    np.testing.assert_allclose(got["traj"][:, 1:8], ref["traj"][:, 1:8], rtol=1e-9, equal_nan=True)
