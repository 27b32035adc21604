"""insider_hip_interaction_glm() form by form against tests/glm_reference.py (longdouble, direct RSS): every form of
k_resid_stats<NB,GT> by name (info "glm_form" = 10 NB + GT: 18, 24, 32, 42), one and several staging rounds per slab
(option / info "glm_slabs"), every lane of the group-sum kernels (K = 63: ldw = 64), k_mm_reduce<3> / <4> at pitch K, the
factor and the group solves at rank above 20, the continuous block, aliased rows at high K, near-exact fits (the RSS
cancellation) and rank deficiency by shape (more non-zero rows of C than genes).

coeff, se and dof are compared directly.  For group g and kept dimension k, with tol_c = 64 K 2^-52 cond2(C C'):
    |beta_dev - beta_ref| <= tol_c max_k |beta_ref,g|                                  (norm-wise)
    |se_dev^2 - se_ref^2| <= (1e-12 ss_g + 2 tol_c RSS_g) diag(G^-1)_k / (dof_g m_g)   (1e-12 of the absolute-sum scale: the
                                                                                       convention of test_gpu_variance.py)
    dof exact.
Every shape keeps p >= 2 K (cond2 at most about 40).  Each check prints its largest error / bound ratios before it asserts.
"""
import numpy as np
import pytest

from insider_amd import _lib
from tests import glm_reference as gr
from tests.support import SPLIT_80_20, factors, levels, masks, resident

pytestmark = pytest.mark.gpu

LD = np.longdouble
COUNTS = (5, 3)
GT_OF_NB = {1: 8, 2: 4, 3: 2, 4: 2}          # ph_gene_tiles in insider_hip.hip
WORST = {}                                   # test label -> (coeff ratio, se^2 ratio), the largest seen


def _cdiv(a, b):
    return -(-a // b)


class _Data:
    def __init__(self, n, p, m=0, seed=0, X=None):
        rng = np.random.default_rng(seed)
        self.X = np.asfortranarray(rng.standard_normal((n, p)) if X is None else X)
        self.lev = levels(rng, n, COUNTS)
        tr, te = masks(rng, n, p, empty=SPLIT_80_20)
        self.Z = np.asfortranarray(rng.standard_normal((n, m))) if m else None
        self.m = m
        self.ds = resident(self.X, self.lev, self.Z, {"train": tr, "test": te})

    def close(self):
        self.ds.close()


@pytest.fixture(scope="module")
def data():
    """One resident data set per (n, p, m): X standard normal, two categorical covariates (5, 3)."""
    cache = {}

    def get(n, p, m=0):
        if (n, p, m) not in cache:
            cache[(n, p, m)] = _Data(n, p, m, seed=100000 * m + 1000 * n + p)
        return cache[(n, p, m)]

    yield get
    for d in cache.values():
        d.close()


def _factors(rng, K, p, m=0):
    return factors(rng, COUNTS, m, K, p)


def _resid(d, A, Cm, sub):
    """X - U C in longdouble (U = the sum of the subtracted blocks' embeddings)."""
    c = d.lev.shape[1]
    U = np.zeros((d.X.shape[0], Cm.shape[0]), dtype=LD)
    for b in range(c):
        if sub[b]:
            U += A[b].astype(LD)[d.lev[:, b] - 1]
    if d.Z is not None and sub[c]:
        U += d.Z.astype(LD) @ A[c].astype(LD)
    return d.X.astype(LD) - U @ Cm.astype(LD)


def _form(K):
    nb = _cdiv(K, 16)
    return 10 * nb + GT_OF_NB[nb]


def _slabs(d, K, opt):
    """The slab count the rule gives: opt >= 1 clamped to 64, 0 = enough blocks for every SIMD four times over (at most 64);
    slabs of cdiv(p, want) genes rounded up to whole staging rounds of 16 GT genes."""
    n, p = d.X.shape
    row_blocks = _cdiv(_cdiv(n, 16), 8)
    want = min(opt, 64) if opt > 0 else max(1, min(64, _cdiv(4 * int(d.ds.info("n_simd")), row_blocks * 8)))
    round_ = 16 * GT_OF_NB[_cdiv(K, 16)]
    return _cdiv(p, _cdiv(_cdiv(p, want), round_) * round_)


def _call(d, A, Cm, group, sub, G, slabs=0, inc=0):
    d.ds.set_option("glm_slabs", slabs)
    try:
        got = d.ds.interaction_glm(A, Cm, group, subtract=sub, inc_continuous=inc, n_groups=G)
        K = Cm.shape[0]
        assert d.ds.info("glm_form") == _form(K), (K, d.ds.info("glm_form"))
        assert d.ds.info("glm_slabs") == _slabs(d, K, slabs), (K, slabs, d.ds.info("glm_slabs"))
    finally:
        d.ds.set_option("glm_slabs", 0)
    return got


def _check(got, ref, K, label, what):
    """The bounds of the module docstring, every group and kept dimension; prints the largest ratios, then asserts."""
    coeff, se, dof = got
    keep = ref["keep"]
    drop = np.setdiff1d(np.arange(K), keep)
    tol_c = LD(64 * K * 2.0 ** -52 * ref["cond"])
    rc = rs = 0.0
    bad = []
    for g in range(coeff.shape[0]):
        m = int(ref["m"][g])
        if m == 0:
            assert np.all(coeff[g] == 0) and np.all(se[g] == 0) and dof[g] == 0, (what, g)
            continue
        assert dof[g] == float(ref["dof"][g]), (what, g, dof[g], ref["dof"][g])
        assert np.all(np.isnan(coeff[g, drop])) and np.all(np.isnan(se[g, drop])), (what, g)
        bref = ref["coeff"][g, keep]
        ratio_c = float(np.abs(coeff[g, keep].astype(LD) - bref).max() / (tol_c * np.abs(bref).max()))
        s = se[g, keep]
        if not (np.all(np.isfinite(s)) and np.all(s >= 0)):
            bad.append((g, "se not finite or negative", s[~(np.isfinite(s) & (s >= 0))][:4]))
            continue
        bound = (LD(1e-12) * ref["ss"][g] + 2 * tol_c * ref["rss"][g]) * ref["dinv"][keep] / (ref["dof"][g] * m)
        ratio_s = float((np.abs(s.astype(LD) ** 2 - ref["se"][g, keep] ** 2) / bound).max())
        rc, rs = max(rc, ratio_c), max(rs, ratio_s)
        if not (ratio_c <= 1 and ratio_s <= 1):
            bad.append((g, ratio_c, ratio_s))
    w = WORST.get(label, (0.0, 0.0))
    WORST[label] = (max(w[0], rc), max(w[1], rs))
    print(f"glm-forms {label} {what}: cond {ref['cond']:.3g} error/bound coeff {rc:.3g} se^2 {rs:.3g}; "
          f"worst of {label} so far coeff {WORST[label][0]:.3g} se^2 {WORST[label][1]:.3g}")
    assert not bad, (what, bad[:5])


def _sweep_groups(n, seed):
    """Ids 0..6 in one vector: id 0 for about a tenth of the samples, 1 a singleton, 2 / 3 / 4 of 31 / 32 / 33 members (the
    PH_CHUNK edges), 5 empty, 6 the rest."""
    zero = n // 10
    ids = np.concatenate([np.zeros(zero), [1], np.full(31, 2), np.full(32, 3), np.full(33, 4)])
    assert n - ids.size >= 1
    ids = np.concatenate([ids, np.full(n - ids.size, 6)]).astype(np.int32)
    return np.random.default_rng(seed).permutation(ids), 6


K_SWEEP = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63]


@pytest.mark.parametrize("K", K_SWEEP)
def test_k_sweep_every_form_one_and_several_rounds(data, K):
    d = data(129, 257)
    rng = np.random.default_rng(7000 + K)
    A, Cm = _factors(rng, K, 257)
    group, G = _sweep_groups(129, K)
    sub = [1, 0]
    ref = gr.glm_reference(_resid(d, A, Cm, sub), group, G, Cm)
    rounds = {8: 3, 4: 5, 2: 9}[GT_OF_NB[_cdiv(K, 16)]]
    assert _cdiv(257, 16 * GT_OF_NB[_cdiv(K, 16)]) == rounds and 257 % 16 == 1      # one slab: a partial last round
    for slabs in (0, 1, 3):
        got = _call(d, A, Cm, group, sub, G, slabs)
        if slabs == 1:
            assert d.ds.info("glm_slabs") == 1
        _check(got, ref, K, "k_sweep", f"K={K} slabs={slabs}")


@pytest.mark.parametrize("K", [7, 20, 40, 63])
def test_every_sample_a_group_of_its_own(data, K):
    d = data(129, 257)                       # sample 128 is alone in the first tile of the second block
    rng = np.random.default_rng(7100 + K)
    A, Cm = _factors(rng, K, 257)
    group = np.arange(1, 130, dtype=np.int32)
    ref = gr.glm_reference(_resid(d, A, Cm, [1, 0]), group, 129, Cm)
    for slabs in (0, 1):
        _check(_call(d, A, Cm, group, [1, 0], 129, slabs), ref, K, "singletons", f"K={K} slabs={slabs}")


@pytest.mark.parametrize("p", [131, 256, 257, 389])
@pytest.mark.parametrize("n", [16, 17, 128, 129, 273])
def test_shape_edges(data, n, p):
    d = data(n, p)
    group, G = d.lev[:, 0].copy(), 5
    if n == 273:                             # more than four chunks of 32: the second stride of k_ph_group_sums
        group[np.random.default_rng(n + p).permutation(n)[:140]] = 6
        G = 6
    for K in (7, 20, 40, 63):
        rng = np.random.default_rng(7200 + 1000 * K + n + p)
        A, Cm = _factors(rng, K, p)
        ref = gr.glm_reference(_resid(d, A, Cm, [1, 0]), group, G, Cm)
        for slabs in (0, 1):
            _check(_call(d, A, Cm, group, [1, 0], G, slabs), ref, K, "shape_edges", f"n={n} p={p} K={K} slabs={slabs}")


@pytest.mark.parametrize("K", [5, 33])
def test_continuous_block(data, K):
    d = data(129, 257, 2)
    rng = np.random.default_rng(7300 + K)
    A, Cm = _factors(rng, K, 257, m=2)
    group, G = _sweep_groups(129, 50 + K)
    for sub in ([1, 0, 1], [1, 0, 0], [0, 1, 1]):
        ref = gr.glm_reference(_resid(d, A, Cm, sub), group, G, Cm)
        for slabs in (0, 1):
            _check(_call(d, A, Cm, group, sub, G, slabs, inc=1), ref, K, "continuous", f"K={K} sub={sub} slabs={slabs}")


@pytest.mark.parametrize("K,zero,copy", [(40, [0, 16, 39], (17, 1)), (63, [15, 62], (40, 3))])
def test_aliased_rows_at_high_k(data, K, zero, copy):
    d = data(129, 257)
    rng = np.random.default_rng(7400 + K)
    A, Cm = _factors(rng, K, 257)
    Cm[zero] = 0.0
    group, G = _sweep_groups(129, 60 + K)
    ref = gr.glm_reference(_resid(d, A, Cm, [1, 0]), group, G, Cm)
    assert list(np.setdiff1d(np.arange(K), ref["keep"])) == zero
    np.testing.assert_array_equal(ref["dof"].astype(np.float64)[ref["m"] > 0], ref["m"][ref["m"] > 0] * 257 - (K - len(zero)))
    first = {}
    for slabs in (0, 1):
        first[slabs] = _call(d, A, Cm, group, [1, 0], G, slabs)
        _check(first[slabs], ref, K, "aliased", f"K={K} zero={zero} slabs={slabs}")
    # one kept row an exact copy of another: singular, refused; the handle stays usable and correct
    Cc = Cm.copy(order="F")
    Cc[copy[0]] = Cc[copy[1]]
    with pytest.raises(_lib.InsiderError) as e:
        d.ds.interaction_glm(A, Cc, group, subtract=[1, 0], n_groups=G)
    assert e.value.status == _lib.ERR_SOLVE
    again = _call(d, A, Cm, group, [1, 0], G, 0)
    _check(again, ref, K, "aliased", f"K={K} after the refused call")
    for x, y in zip(again, first[0]):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("sigma", [1.0, 1e-3, 1e-6, 1e-9, 0.0])
@pytest.mark.parametrize("K", [63, 7])
def test_near_exact_fit(K, sigma):
    """subtract = [0, 0]: the residual is X, whose rows of a group are b_g' C + sigma E.  RSS = ss - m beta' mean(w) cancels
    to rounding noise of either sign as sigma -> 0: every se stays finite and >= 0, within the absolute term of the bound."""
    n, p = 24, 131
    rng = np.random.default_rng(7500 + K)
    A, Cm = _factors(rng, K, p)
    group = np.zeros(n, dtype=np.int32)
    order = rng.permutation(n)
    group[order[0]] = 1                      # a group of 1
    group[order[1:18]] = 2                   # and one of 17 members
    X = rng.standard_normal((n, p))
    E = rng.standard_normal((n, p))
    for g in (1, 2):
        rows = np.flatnonzero(group == g)
        X[rows] = rng.standard_normal(K) @ Cm + sigma * E[rows]
    d = _Data(n, p, seed=K, X=X)
    try:
        ref = gr.glm_reference(d.X.astype(LD), group, 2, Cm)
        for slabs in (0, 1):
            got = _call(d, A, Cm, group, [0, 0], 2, slabs)
            assert np.all(np.isfinite(got[1])) and np.all(got[1] >= 0), (K, sigma, got[1])
            _check(got, ref, K, "near_exact", f"K={K} sigma={sigma:g} slabs={slabs}")
    finally:
        d.close()


@pytest.mark.parametrize("K,p", [(7, 6), (20, 19), (40, 39), (63, 62)])
def test_more_rows_than_genes_is_refused(K, p):
    """p = K - 1 < rank: C C' is exactly rank-deficient, whatever rounding leaves in its last pivots."""
    n = 16
    d = _Data(n, p, seed=K)
    try:
        group = d.lev[:, 1]
        for seed in range(3):
            rng = np.random.default_rng(7600 + 10 * K + seed)
            A, Cm = _factors(rng, K, p)
            with pytest.raises(_lib.InsiderError) as e:
                d.ds.interaction_glm(A, Cm, group, subtract=[1, 0])
            assert e.value.status == _lib.ERR_SOLVE, (K, p, seed)
            # the handle stays usable: the next call (rank 3 <= p / 2) is correct
            Ks = 3
            A2, C2 = _factors(rng, Ks, p)
            ref = gr.glm_reference(_resid(d, A2, C2, [1, 0]), group, 3, C2)
            _check(_call(d, A2, C2, group, [1, 0], 3), ref, Ks, "p_below_rank", f"K={Ks} p={p} after K={K} seed={seed}")
    finally:
        d.close()


def test_repeat_is_bit_identical(data):
    d = data(129, 257)
    rng = np.random.default_rng(7700)
    A, Cm = _factors(rng, 63, 257)
    group, G = _sweep_groups(129, 77)
    a = _call(d, A, Cm, group, [1, 0], G)
    b = _call(d, A, Cm, group, [1, 0], G)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
