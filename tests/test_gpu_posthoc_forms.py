"""Every (QT, KS) instantiation of the post-hoc product kernels, launched by name and compared with the float64 yardstick
and the bound of the call's own test file: k_ls_prod<QT,KS> (level scores), k_fd_prod<8,KS,true> (factor decomposition),
k_rc_back / k_rc_fwd<QT,KS> (residual products) and k_cx_stage<KS> (co-expression); KS = ceil(K / 16), QT the tiles of 16
output columns.  The library reports the instantiation of the last call's heavy launch (info "ls_form", "fd_form", "rc_form":
10 QT + KS; "cx_form": KS), and every case asserts the one FORMS claims for it: a change of the dispatch rule cannot leave an
instantiation unrun while the K lists still look complete.

No tolerance is introduced here: _check of tests/test_gpu_level_scores.py, tests/test_gpu_factdecomp.py and
tests/test_gpu_rescomp.py and reference + check_rule3 of tests/test_gpu_coexpression.py carry the bounds those files derive.
Run with -s to see every checker's largest error / bound ratio.

The last part is co-expression at its size edges.  With all-zero factors, no centre or scale and entries "all" the working
residual is (x - 0 - 0) x 1 = x to the bit, and k_cx_norm runs on the staged buffer the cx_standardise() that k_cx_prep runs
on a caller's vectors, so coexpression() must return gram_topk(X or X', "correlation") bit for bit: a tolerance-free check
that k_cx_stage puts every entry where k_cx_topk reads it."""
import numpy as np
import pytest

from insider_amd import api
from tests.support import (GENES_3_5_7, SAMPLES_3_5_7, SAMPLES_3_5_7_GENES_1_3, bits, factors, levels, lib, need_gpu,  # noqa: F401
                           planted, resident)
from tests.test_gpu_coexpression import center_scale, reference
from tests.test_gpu_factdecomp import _check as fd_check
from tests.test_gpu_level_scores import _check as ls_check
from tests.test_gpu_neighbors import check_rule3
from tests.test_gpu_rescomp import _center_scale as rc_center_scale
from tests.test_gpu_rescomp import _check as rc_check

pytestmark = pytest.mark.gpu

# (call, QT, KS) -> the cases below that launch it, by their ids.  level_scores: L levels of the scored covariate, K;
# factor_decomposition: K and the data set; residual_products: q columns of Q, K; coexpression: K.
FORMS = {
    ("level_scores", 1, 1): ("L5-K16",),
    ("level_scores", 1, 2): ("L5-K17", "L5-K32"),
    ("level_scores", 1, 3): ("L5-K33", "L5-K48"),
    ("level_scores", 1, 4): ("L5-K49", "L5-K63"),
    ("level_scores", 8, 1): ("L17-K16",),
    ("level_scores", 8, 2): ("L17-K17", "L17-K32", "L129-K17"),
    ("level_scores", 8, 3): ("L17-K33", "L17-K48", "L129-K33", "L17-K33-slabs3"),
    ("level_scores", 8, 4): ("L17-K49", "L17-K63", "L129-K63"),
    ("factor_decomposition", 8, 1): ("K16",),
    ("factor_decomposition", 8, 2): ("K32",),
    ("factor_decomposition", 8, 3): ("K33", "K47", "K48", "K48-three-blocks", "K40-continuous"),
    ("factor_decomposition", 8, 4): ("K49",),
    ("residual_products", 1, 1): ("q16-K16",),
    ("residual_products", 1, 2): ("q1-K17",),
    ("residual_products", 1, 3): ("q1-K33", "q16-K48"),
    ("residual_products", 1, 4): ("q16-K63",),
    ("residual_products", 2, 1): ("q32-K16",),
    ("residual_products", 2, 2): ("q17-K32",),
    ("residual_products", 2, 3): ("q17-K48",),
    ("residual_products", 2, 4): ("q32-K49",),
    ("residual_products", 3, 1): ("q48-K16",),
    ("residual_products", 3, 2): ("q33-K17",),
    ("residual_products", 3, 3): ("q48-K33",),
    ("residual_products", 3, 4): ("q33-K49",),
    ("residual_products", 4, 1): ("q64-K16",),
    ("residual_products", 4, 2): ("q49-K32",),
    ("residual_products", 4, 3): ("q49-K33", "q64-K48"),
    ("residual_products", 4, 4): ("q64-K63",),
    ("coexpression", 0, 1): ("K16",),
    ("coexpression", 0, 2): ("K17", "K32"),
    ("coexpression", 0, 3): ("K33",),
    ("coexpression", 0, 4): ("K49", "K63"),
}

# what the dispatch sites can produce: one tile of levels or the window of 8; one window width; ceil(q / 16) = 1..4; KS alone
DISPATCH = {"level_scores": (1, 8), "factor_decomposition": (8,), "residual_products": (1, 2, 3, 4), "coexpression": (0,)}
INFO = {"level_scores": "ls_form", "factor_decomposition": "fd_form", "residual_products": "rc_form", "coexpression": "cx_form"}

LS_CASES = [(L, K, 0) for L in (5, 17) for K in (16, 17, 32, 33, 48, 49, 63)] + [(129, K, 0) for K in (17, 33, 63)] + [(17, 33, 3)]
# K, (n, p), the covariates' level counts, continuous columns, "fd_path"
FD_CASES = {
    "K16": (16, (65, 70), (5, 3), 0, 1), "K32": (32, (65, 70), (5, 3), 0, 1), "K33": (33, (65, 70), (5, 3), 0, 1),
    "K47": (47, (65, 70), (5, 3), 0, 1), "K48": (48, (65, 70), (5, 3), 0, 1), "K49": (49, (65, 70), (5, 3), 0, 1),
    "K48-three-blocks": (48, (65, 37), (2, 3, 4), 0, 2),      # 144 columns: nine tiles, two windows
    "K40-continuous": (40, (65, 70), (5, 3), 2, 1),
}
RC_CASES = [(1, 33), (16, 48), (49, 33), (64, 48), (17, 32), (33, 49),                       # first launched here; block boundaries
            (16, 16), (1, 17), (16, 63), (32, 16), (17, 48), (32, 49), (48, 16), (33, 17), (48, 33), (64, 16), (49, 32), (64, 63)]
CX_K = (16, 17, 32, 33, 49, 63)


def ls_id(L, K, slabs):
    return f"L{L}-K{K}" + (f"-slabs{slabs}" if slabs else "")


def rc_id(q, K):
    return f"q{q}-K{K}"


CASE_IDS = {"level_scores": [ls_id(*c) for c in LS_CASES], "factor_decomposition": list(FD_CASES),
            "residual_products": [rc_id(*c) for c in RC_CASES], "coexpression": [f"K{K}" for K in CX_K]}


def form_of(call, case):
    """The instantiation FORMS claims for a case, as the library reports it."""
    (hit,) = [key for key, cases in FORMS.items() if key[0] == call and case in cases]
    return 10 * hit[1] + hit[2]


def test_the_table_lists_every_instantiation_once_and_every_case():
    want = {(call, qt, ks) for call, qts in DISPATCH.items() for qt in qts for ks in (1, 2, 3, 4)}
    assert set(FORMS) == want and len(want) == 32
    assert [sum(k[0] == call for k in FORMS) for call in DISPATCH] == [8, 4, 16, 4]
    for call, ids in CASE_IDS.items():
        listed = [c for key, cases in FORMS.items() if key[0] == call for c in cases]
        assert sorted(listed) == sorted(ids), call               # every case under exactly one form, no case unknown
    assert all(cases for cases in FORMS.values())


def test_no_call_yet_reports_form_0(lib):
    ds = resident(*planted(20, 18, (3, 2), seed=1))
    try:
        assert all(ds.info(key) == 0 for key in INFO.values())
    finally:
        ds.close()


# ---- the data sets: made once per shape, left unchanged ---------------------------------------------------------------------
_DATA = {}


def data(n, p, counts, m, seed, empty):
    key = (n, p, counts, m, seed, empty)
    if key not in _DATA:
        d = planted(n, p, counts, m, seed, empty=empty)
        _DATA[key] = (resident(*d),) + d
    return _DATA[key]


@pytest.fixture(scope="module", autouse=True)
def close_data():
    yield
    for d in _DATA.values():
        d[0].close()
    _DATA.clear()


# ---- level scores -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,K,slabs", LS_CASES, ids=CASE_IDS["level_scores"])
def test_level_scores_forms(lib, L, K, slabs):
    """L = 5: one level tile; 17: the window form with a last tile of one live column; 129: a second window of one tile with
    one live column.  n = 37: three wave tiles of samples, the last of 5 (n = 203 where 129 levels need the samples)."""
    n = 37 if L <= 37 else 203
    ds, X, lev, Z, masks = data(n, 37, (L, 3), 0, L, SAMPLES_3_5_7)
    A, Cm = factors(np.random.default_rng(100 * L + K), (L, 3), 0, K, 37)
    ds.set_option("ls_slabs", slabs)
    try:
        for e in ("all", "train"):
            got = ds.level_scores(A, Cm, 0, entries=e)
            assert ds.info("ls_form") == form_of("level_scores", ls_id(L, K, slabs)), ds.info("ls_form")
            assert ds.info("ls_path") == (1 if L <= 128 else 2)
            if slabs:
                assert ds.info("ls_slabs") == slabs
            ls_check(got, X, lev, Z, masks[e], A, Cm, 0)
    finally:
        ds.set_option("ls_slabs", 0)


# ---- factor decomposition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FD_CASES))
def test_factor_decomposition_forms(lib, case):
    K, (n, p), counts, m, path = FD_CASES[case]
    ds, X, lev, Z, masks = data(n, p, counts, m, n + p + m, GENES_3_5_7)
    A, Cm = factors(np.random.default_rng(K + len(counts)), counts, m, K, p)
    for e in ("all", "train", "test"):
        got = ds.factor_decomposition(A, Cm, entries=e, inc_continuous=1 if m else 0)
        assert ds.info("fd_form") == form_of("factor_decomposition", case), ds.info("fd_form")
        assert ds.info("fd_path") == path
        assert got["sum_h"].shape == (len(counts) + (1 if m else 0) + 1, K, p)
        fd_check(got, X, lev, Z, masks[e], A, Cm)


# ---- residual products ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,K", RC_CASES, ids=CASE_IDS["residual_products"])
def test_residual_products_forms(lib, q, K):
    """n = 70: two sample tiles of k_rc_fwd (the second of 6 samples) and three chunks of k_rc_back (the last of 6); p = 37: a
    ragged last gene group.  Y is requested, so both kernels run: automatic slabs without centre and scale on every entry,
    two slabs with them on the train entries."""
    n, p, counts = 70, 37, (4, 3)
    ds, X, lev, Z, masks = data(n, p, counts, 0, 7, SAMPLES_3_5_7_GENES_1_3)
    rng = np.random.default_rng(100 * q + K)
    A, Cm = factors(rng, counts, 0, K, p)
    Q = rng.standard_normal((n, q))
    ce, sc = rc_center_scale(rng, p)
    try:
        for slabs, e, cs in ((0, "all", (None, None)), (2, "train", (ce, sc))):
            ds.set_option("rc_slabs", slabs)
            got = ds.residual_products(A, Cm, Q, entries=e, center=cs[0], scale=cs[1])
            assert ds.info("rc_form") == form_of("residual_products", rc_id(q, K)), ds.info("rc_form")
            used = ds.info("rc_slabs")                          # (0 would mean that the forward pass did not run)
            assert used == slabs if slabs else used >= 1
            assert got["Y"] is not None
            rc_check(got, X, lev, Z, masks[e], A, Cm, Q, cs[0], cs[1])
    finally:
        ds.set_option("rc_slabs", 0)


# ---- co-expression --------------------------------------------------------------------------------------------------------------
AXES = ("genes", "samples")
OUT = ("index", "score")
COUNTS = (5, 3)


@pytest.mark.parametrize("K", CX_K, ids=CASE_IDS["coexpression"])
def test_coexpression_forms(lib, K):
    n, p, k = 37, 70, 10
    ds, X, lev, Z, masks = data(n, p, COUNTS, 0, n, SAMPLES_3_5_7_GENES_1_3)
    rng = np.random.default_rng(1000 * K + n)
    A, Cm = factors(rng, COUNTS, 0, K, p)
    ce, sc = center_scale(rng, p)
    for e in ("all", "train"):
        for axis in AXES:
            for kw in ({}, dict(center=ce, scale=sc)):
                S, T, elig, alive = reference(X, lev, Z, masks[e], A, Cm, axis, **kw)
                got = ds.coexpression(A, Cm, axis=axis, k=k, entries=e, **kw)
                assert ds.info("cx_form") == form_of("coexpression", f"K{K}"), ds.info("cx_form")
                check_rule3(got, S, T, k, elig)


# the vector count N is p for the genes and n for the samples, the depth the other dimension.  (32, 64): a depth of one whole
# chunk of 32, N = 64 without padding; (33, 65): one entry into a second chunk, a second query block with one live query;
# (64, 128); (5, 3): N below one tile; (2, 17): depths 2 and 17; (1, 20): depth 1, every gene dead.
EDGE_SHAPES = [(32, 64), (33, 65), (64, 128), (5, 3), (2, 17), (1, 20)]
EDGE_K = {s: (10,) for s in EDGE_SHAPES}
EDGE_K[(33, 65)] = (10, 64)


def _integer_data(n, p):
    """Small-integer X (equal scores are plentiful: the order by ascending index is exercised), gene 0 constant (dead: its row
    all open slots, nobody's partner) and the last gene a copy of gene 1; every entry present, split 80 / 20 into train and
    test."""
    rng = np.random.default_rng(1000 * n + p)
    X = rng.integers(-3, 4, size=(n, p)).astype(np.float64)
    X[:, 0] = 2.0
    X[:, p - 1] = X[:, 1]
    counts = tuple(min(c, n) for c in COUNTS)
    lev = levels(rng, n, counts)
    tr = rng.random((n, p)) < 0.8
    ds = api.InsiderData(np.asfortranarray(X), lev, np.asfortranarray(tr, dtype=np.uint8), np.asfortranarray(~tr, dtype=np.uint8))
    return ds, X, lev, counts


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coexpression_of_zero_factors_is_gram_topk_of_x_to_the_bit(lib, shape):
    n, p = shape
    ds, X, lev, counts = _integer_data(n, p)
    try:
        for K in (3, 63):
            A = [np.zeros((L, K), order="F") for L in counts]
            Cm = np.zeros((K, p), order="F")
            for axis in AXES:
                V = np.asfortranarray(X if axis == "genes" else X.T)
                N = V.shape[1]
                S, T, elig, alive = reference(X, lev, None, None, A, Cm, axis)
                for k in EDGE_K[shape]:
                    got = ds.coexpression(A, Cm, axis=axis, k=k, entries="all")
                    assert ds.info("cx_form") == (K + 15) // 16
                    gram = api.gram_topk(V, k=k, metric="correlation")
                    assert got["index"].shape == gram["index"].shape == (N, k)
                    assert np.array_equal(got["index"], gram["index"]), (axis, K, k)
                    assert bits(got, OUT) == bits(gram, OUT), (axis, K, k)
                    check_rule3(got, S, T, k, elig)                   # and both are right, not merely equal
                    if axis == "genes":
                        assert not alive[0] and np.all(got["index"][0] == -1) and not np.any(got["index"] == 0)
                        if n == 1:
                            assert not alive.any() and np.all(got["index"] == -1) and np.all(np.isnan(got["score"]))
                        elif n >= 5 and alive[1]:
                            # the copy of gene 1 shares gene 1's best score.  (With a depth of 2 every live pair scores +-1 up
                            # to rounding and the copy, the last index, need not be among the first k.)
                            at = np.flatnonzero(got["index"][1] == p - 1)
                            assert at.size == 1 and got["score"][1, at[0]] == got["score"][1, 0]
    finally:
        ds.close()


# the same edges through the NaN-as-unselected path.  The planting empties samples 3 / 5 / 7 and genes 1 / 3, so it needs 8
# samples and 4 genes: the three larger shapes.
MASKED_SHAPES = [s for s in EDGE_SHAPES if s[0] >= 8 and s[1] >= 4]


@pytest.mark.parametrize("shape", MASKED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coexpression_masked_at_the_size_edges(lib, shape):
    assert len(MASKED_SHAPES) == 3
    n, p = shape
    ds, X, lev, Z, masks = data(n, p, COUNTS, 0, n + p, SAMPLES_3_5_7_GENES_1_3)
    for K in (3, 63):
        A, Cm = factors(np.random.default_rng(K + n), COUNTS, 0, K, p)
        for e in ("train", "test"):
            for axis in AXES:
                S, T, elig, alive = reference(X, lev, Z, masks[e], A, Cm, axis)
                for k in EDGE_K[shape]:
                    got = ds.coexpression(A, Cm, axis=axis, k=k, entries=e)
                    assert ds.info("cx_form") == (K + 15) // 16
                    check_rule3(got, S, T, k, elig)
                if axis == "samples":
                    assert not alive[7] and np.all(got["index"][7] == -1)      # sample 7 is all NA
                else:
                    dead = {"train": 1, "test": 3}[e]                          # gene 1 has no train entry, gene 3 no test entry
                    assert not alive[dead] and np.all(got["index"][dead] == -1)
