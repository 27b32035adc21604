"""Every form of solve(..., likely_sympd) on the device against tests/solve_reference.py (longdouble, iterative refinement).

a. Direct (api.solve_sympd, form "batch" = k_solve_batch at row pitch K; form "level" = the fit's k_level_solve<NB> on level
   equation records: the register Gauss-Jordan for K <= 31, the LDS Cholesky at pitch KP = 48 / 64 for K >= 32, the pivoted
   elimination at pitch KP on a reloaded record after a non-positive pivot), every K in 1..63 (and 64 for "batch"):
     i    spd          Q diag(s) Q', cond 1, 1e4, 1e8, 1e12
     ii   scaled       D A D, D = diag(10**u), u in [-3, 3]
     iii  indefinite   first non-positive pivot at position 0, K / 2 and K - 1 (the last: the positive-definite route has
                       overwritten the whole system when it fails)
     iv   zero_diag    a_00 = 0 over a non-zero column (a real row exchange), with and without a tie of the pivot magnitudes
     v    nonsymmetric "batch" only
     vi   exact cases, vii lambda on the device, viii routes 0 / 1 / -1 in one launch, ix repeats
b. The row update by kernel form (merged_solve, level_solve, merged_zero; "row_kernels"), c. the ridge columns (ridge_reg,
   ridge; info "col_solver") follow below with their own docstrings.

Bounds.  Primary, for every system: the backward error eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), evaluated
in longdouble, is at most
    min( K (3K + 1) 2**-52 rho ,  max( 8 Y , 4 * 2**-52 ) )
rho = the growth factor of the reference's partial pivoting on route 1, 1 on route 0 (Higham, Accuracy and Stability,
Theorems 10.3 and 9.4); Y = the largest backward error over the same family and K of the float64 yardstick of the route
(pivot-free Gauss-Jordan for the register route, Cholesky for the LDS route, row-pivoted Gauss-Jordan for the general one),
measured here on the CPU against the same reference; 8 for another summation order and fused multiply-adds.
Secondary, where cond_2(A) <= 1e8: ||x - x_ref||_inf <= 4 K^2 2**-52 rho cond_2(A) ||x_ref||_inf.  Family i is built at
cond 1e8 exactly and the computed cond_2 is a rounded value (relative error about cond * 2**-52 = 2e-8), so the comparison
is made with 1e8 (1 + 1e-6): the systems built at 1e8 are always checked.
The route of EVERY system is asserted against the reference's.  Each check prints its largest error / bound before it asserts.

Exact cases: A = I gives x = b by bits on every route.  A diagonal A gives b / d by bits wherever one division forms x: the
register route (x_i = b_i / pivot_i) and the general route (f = 0 in every row), and on the Cholesky routes for d a power of
4.  For other d the Cholesky routes form (b / s) / s with s = fl(sqrt d): the square root's rounding enters twice, each
division once, and fl(b / d), which the result is compared with, carries one more: |x - fl(b / d)| <= 5 * 2**-53
(1 + 2**-50) |b / d| is asserted there.
"""
import functools

import numpy as np
import pytest

from insider_amd import _lib, api
from tests import solve_reference as sr
from tests.support import need_gpu  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CHOL_DIAG_TOL = 5 * 2.0 ** -53 * (1 + 2.0 ** -50)            # a diagonal system on a Cholesky route (module docstring)
EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63]      # the register blocks and the pitches KP = 16, 32, 48, 64
FWD_COND = 1e8 * (1 + 1e-6)                                  # the forward check runs up to cond 1e8 (module docstring)
WORST = {}                                                   # (section, family, form) -> largest error / bound seen


def _yardstick_name(form, K, route):
    if route == 1:
        return "gj_rowpivot"
    return "gj_nopivot" if form == "level" and K <= 31 else "chol"


YARDSTICKS = {"gj_rowpivot": sr.gj_rowpivot_f64, "gj_nopivot": sr.gj_nopivot_f64, "chol": sr.chol_f64}


class _Family:
    """The systems of one family at one K with everything the checks need, computed once on the CPU: the reference's x,
    route and rho, cond_2, and the float64 yardsticks' largest backward error by yardstick."""

    def __init__(self, mats, rng):
        self.A = np.stack(mats)
        B, K = self.A.shape[:2]
        self.b = rng.standard_normal((B, K))
        self.x, self.route, self.rho, self.cond, self.yard = [], [], [], [], {}
        for A, b in zip(self.A, self.b):
            info = {}
            x, route = sr.solve_likely_sympd(A, b, info)
            self.x.append(x)
            self.route.append(route)
            self.rho.append(info["rho"])
            self.cond.append(float(np.linalg.cond(A)) if route >= 0 else np.inf)
            if route < 0:
                continue
            for name in ({"gj_nopivot", "chol"} if route == 0 else {"gj_rowpivot"}):
                y = YARDSTICKS[name](A, b)
                assert y is not None and np.all(np.isfinite(y)), name
                self.yard[name] = max(self.yard.get(name, 0.0), sr.backward_error(A, b, y))
        self.route = np.array(self.route, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _families(K):
    rng = np.random.default_rng(9000 + K)
    fams = {name: _Family([A for A, _ in systems], rng) for name, systems in sr.families(K, seed=1).items()}
    pos = sr.indefinite_positions(K)
    fams["nonsymmetric"] = _Family([sr.nonsymmetric(rng, K, pos[t % len(pos)]) for t in range(6)], rng)
    return fams


def _check(section, family, form, K, fam, x, route):
    """The bounds of the module docstring for every system of `fam`; prints the largest ratios, then asserts."""
    assert np.array_equal(route, fam.route), (section, family, form, K, route, fam.route)
    rb = rf = 0.0
    bad = []
    for s in range(fam.A.shape[0]):
        if fam.route[s] < 0:
            continue
        A, b, xr, rho = fam.A[s], fam.b[s], fam.x[s], fam.rho[s]
        assert np.all(np.isfinite(x[s])), (section, family, form, K, s)
        cap = K * (3 * K + 1) * EPS * rho
        yard = max(8.0 * fam.yard[_yardstick_name(form, K, fam.route[s])], 4.0 * EPS)
        ratio_b = sr.backward_error(A, b, x[s]) / min(cap, yard)
        ratio_f = 0.0
        if fam.cond[s] <= FWD_COND:
            fwd = float(np.abs(x[s].astype(sr.LD) - xr).max() / np.abs(xr).max())
            ratio_f = fwd / (4 * K * K * EPS * rho * fam.cond[s])
        rb, rf = max(rb, ratio_b), max(rf, ratio_f)
        if not (ratio_b <= 1 and ratio_f <= 1):
            bad.append((s, int(fam.route[s]), ratio_b, ratio_f))
    key = (section, family, form)
    w = WORST.get(key, (0.0, 0.0))
    WORST[key] = (max(w[0], rb), max(w[1], rf))
    print(f"solve-forms {section} {family} {form} K={K}: error/bound backward {rb:.3g} forward {rf:.3g}; worst so far "
          f"backward {WORST[key][0]:.3g} forward {WORST[key][1]:.3g}")
    assert not bad, (section, family, form, K, bad[:5])


def _forms(K):
    return ("batch", "level") if K <= 63 else ("batch",)


# ----------------------------------------------------------------------------------------------------------------------
# a. direct, both forms
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", list(range(1, 65)))
def test_direct_every_family(K):
    """i-v: every K, every system's route, the backward and forward bounds."""
    for family, fam in _families(K).items():
        assert 5 <= fam.A.shape[0] <= 9
        for form in _forms(K):
            if family == "nonsymmetric" and form == "level":
                continue
            x, route = api.solve_sympd(fam.A, fam.b, return_route=True, form=form)
            _check("direct", family, form, K, fam, x, route)


@pytest.mark.parametrize("K", EDGES + [64])
def test_exact_cases(K):
    rng = np.random.default_rng(9100 + K)
    B = 5
    b = rng.standard_normal((B, K))
    eye = np.broadcast_to(np.eye(K), (B, K, K)).copy()
    pow4 = np.stack([np.diag(4.0 ** rng.integers(-5, 6, K)) for _ in range(B)])
    anyd = np.stack([np.diag(rng.uniform(0.1, 10.0, K)) for _ in range(B)])
    neg = anyd.copy()
    neg[:, K // 2, K // 2] *= -1.0                      # one negative entry: the general route
    for form in _forms(K):
        x, route = api.solve_sympd(eye, b, return_route=True, form=form)
        assert np.array_equal(x, b) and np.all(route == 0), (form, K)
        x, route = api.solve_sympd(pow4, b, return_route=True, form=form)
        assert np.array_equal(x, b / np.diagonal(pow4, axis1=1, axis2=2)) and np.all(route == 0), (form, K)
        x, route = api.solve_sympd(neg, b, return_route=True, form=form)
        assert np.array_equal(x, b / np.diagonal(neg, axis1=1, axis2=2)) and np.all(route == 1), (form, K)
        x, route = api.solve_sympd(anyd, b, return_route=True, form=form)
        want = b / np.diagonal(anyd, axis1=1, axis2=2)
        assert np.all(route == 0), (form, K)
        if form == "level" and K <= 31:                 # the register route: one division
            assert np.array_equal(x, want), (form, K)
        else:                                           # Cholesky: (b / sqrt d) / sqrt d
            assert np.all(np.abs(x - want) <= CHOL_DIAG_TOL * np.abs(want)), (form, K)
        # b = 0 gives x = 0 on every route
        fam = _families(K)
        for family in ("spd", "indefinite"):
            x, route = api.solve_sympd(fam[family].A, np.zeros_like(fam[family].b), return_route=True, form=form)
            assert np.all(x == 0.0) and np.array_equal(route, fam[family].route), (form, K, family)


@pytest.mark.parametrize("form", ["batch", "level"])
def test_k_equals_one(form):
    a = np.array([4.0, 3.0, 1e-300, 1e300, -2.0, -0.375]).reshape(-1, 1, 1)
    b = np.array([3.0, 1.0, 7.0, -5.0, 9.0, 0.1]).reshape(-1, 1)
    x, route = api.solve_sympd(a, b, return_route=True, form=form)
    assert list(route) == [0, 0, 0, 0, 1, 1]
    want = (b / a[:, 0])
    if form == "level":                                 # register route and general route: one division
        assert np.array_equal(x, want)
    else:
        assert np.array_equal(x[[0, 4, 5]], want[[0, 4, 5]])
        assert np.all(np.abs(x - want) <= CHOL_DIAG_TOL * np.abs(want))
    with pytest.raises(_lib.InsiderError) as e:
        api.solve_sympd(np.array([[[4.0]], [[0.0]], [[-1.0]]]), np.ones((3, 1)), form=form)
    assert e.value.status == _lib.ERR_SOLVE and list(e.value.route) == [0, -1, 1]
    assert e.value.x[0, 0] == 0.25 and e.value.x[2, 0] == -1.0


@pytest.mark.parametrize("K", EDGES + [64])
def test_lambda_is_added_on_the_device(K):
    """vii: solve(A, b, lambda) equals solve(A + lambda I, b) formed on the host, by bits and by route, for both signs: the
    negative value lies inside the spectrum (cond 1e4: eigenvalues 1e-4 .. 1), so it turns the system indefinite."""
    fam = _families(K)["spd"]
    sel = [2, 3]                                        # the two systems of cond 1e4
    A, b = fam.A[sel], fam.b[sel]
    sv = np.logspace(0.0, -4.0, K)
    neg = -np.sqrt(sv[(K - 1) // 4] * sv[(K - 1) // 4 + 1]) if K > 1 else -2.0      # between two neighbouring eigenvalues
    for form in _forms(K):
        for lam, want_route in ((0.37, 0), (float(neg), 1)):
            host = A + lam * np.eye(K)
            infos = [{} for _ in sel]
            ref = [sr.solve_likely_sympd(h, bb, i) for h, bb, i in zip(host, b, infos)]
            assert all(r[1] == want_route for r in ref), (K, lam)
            ev = np.linalg.eigvalsh(host)
            assert np.all(np.abs(ev).min(axis=1) >= 1e-3 * np.abs(ev).max(axis=1)), (K, lam)   # no route is a coin toss
            x1, r1 = api.solve_sympd(A, b, return_route=True, lambda_=lam, form=form)
            x0, r0 = api.solve_sympd(host, b, return_route=True, form=form)
            assert np.array_equal(x1, x0) and np.array_equal(r1, r0) and np.all(r1 == want_route), (form, K, lam)
            for s in range(len(sel)):
                cap = K * (3 * K + 1) * EPS * infos[s]["rho"]
                assert sr.backward_error(host[s], b[s], x1[s]) <= cap, (form, K, lam, s)


def _singular(rng, K):
    """Symmetric with row and column K / 2 zero: the elimination meets an exactly zero pivot column."""
    A = sr.spd(rng, K, 10.0)
    A[K // 2, :] = 0.0
    A[:, K // 2] = 0.0
    return A


@pytest.mark.parametrize("K", EDGES)
def test_mixed_routes_in_one_launch(K):
    """viii: routes 0, 1 and -1 interleaved in one batch: ERR_SOLVE, every route as the reference's, and every solvable
    system's x by bits what that system gives alone."""
    rng = np.random.default_rng(9200 + K)
    pos = sr.indefinite_positions(K)
    mats = [sr.spd(rng, K, 1e4), sr.indefinite(rng, K, pos[-1]), _singular(rng, K), sr.spd(rng, K, 1e8),
            sr.indefinite(rng, K, pos[len(pos) // 2]), sr.spd(rng, K, 1.0), _singular(rng, K), sr.indefinite(rng, K, 0),
            sr.spd(rng, K, 1e12)]
    fam = _Family(mats, rng)
    assert list(fam.route) == [0, 1, -1, 0, 1, 0, -1, 1, 0]
    for form in _forms(K):
        with pytest.raises(_lib.InsiderError) as e:
            api.solve_sympd(fam.A, fam.b, form=form)
        assert e.value.status == _lib.ERR_SOLVE
        _check("mixed", "routes", form, K, fam, e.value.x, e.value.route)
        for s in np.flatnonzero(fam.route >= 0):
            x, route = api.solve_sympd(fam.A[s], fam.b[s], return_route=True, form=form)
            assert route == fam.route[s] and np.array_equal(x, e.value.x[s]), (form, K, s)
        # the refused call leaves nothing behind: the next batch is solved as before
        ok = np.flatnonzero(fam.route >= 0)
        x, route = api.solve_sympd(fam.A[ok], fam.b[ok], return_route=True, form=form)
        assert np.array_equal(x, e.value.x[ok]) and np.array_equal(route, fam.route[ok]), (form, K)


@pytest.mark.parametrize("K", [16, 31, 40, 63])
def test_repeat_is_bit_identical(K):
    for family, fam in _families(K).items():
        for form in _forms(K):
            if family == "nonsymmetric" and form == "level":
                continue
            a = api.solve_sympd(fam.A, fam.b, return_route=True, form=form)
            b = api.solve_sympd(fam.A, fam.b, return_route=True, form=form)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (family, form, K)


def test_stand_alone_entry_is_form_zero():
    """insider_hip_solve_sympd(...) is insider_hip_solve_sympd_form(..., lambda = 0, form = 0)."""
    import ctypes as C
    fam = _families(33)["indefinite"]
    Af = np.ascontiguousarray(np.transpose(fam.A, (0, 2, 1)))
    B, K = fam.b.shape
    x = np.zeros((B, K))
    route = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.load().insider_hip_solve_sympd(_lib.ptr(Af), _lib.ptr(fam.b), K, B, 0, _lib.ptr(x),
                                                   _lib.ptr(route, C.c_int32)))
    x2, route2 = api.solve_sympd(fam.A, fam.b, return_route=True)
    assert np.array_equal(x, x2) and np.array_equal(route, route2)


def test_arguments_are_checked():
    A, b = np.eye(64)[None], np.ones((1, 64))
    with pytest.raises(_lib.InsiderError) as e:
        api.solve_sympd(A, b, form="level")             # K = 64: no level record
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.InsiderError) as e:
        api.solve_sympd(A, b, form="columns")
    assert e.value.status == _lib.ERR_ARG
    with pytest.raises(_lib.InsiderError) as e:
        api.solve_sympd(A, b, lambda_=float("nan"))
    assert e.value.status == _lib.ERR_ARG


# ----------------------------------------------------------------------------------------------------------------------
# b. the row update by kernel form
# ----------------------------------------------------------------------------------------------------------------------
# ds.optimize_row(cov = 0) on n = 130 samples, p = 2 K + 40 genes, two covariates: the first with levels of 1, 64, 0, 33 and
# 32 samples (level 3 is empty: its row of A is kept by bits), the second with three levels whose contribution U C is
# subtracted.  C = P diag(sqrt s) Q' (Q: p x K orthonormal, P: K x K orthogonal, or the identity in the "plain" cases), so
# that cond(C C') = 1, 1e4, 1e8 with lambda = 0 and 1e-3; a negative lambda with cond 1 and with a two-cluster spectrum of
# cond 16 (s = 1 and 1 / 16), placed at minus the geometric mean of the smallest eigenvalues of the 1-sample and the
# 64-sample level's Gram part, so that the first is indefinite and the second positive definite.
#
# Reference: the level equations from their definition in longdouble,
#     masked:    H_l = sum_{r in l} C diag(m_r) C' + lambda I,   g_l = sum_{r in l} C (m_r o (x_r - C' u_r))
#     unmasked:  H_l = cnt_l C C' + lambda I,                     g_l = sum_{r in l} C (x_r - C' u_r)
# (m_r the sample's training mask, u_r its row of the other covariate's factor), then solve_likely_sympd.
#
# Margins, asserted on the CPU for EVERY level: with lambda < 0 the eigenvalue of H_l nearest to zero is at least 1e-3
# ||H_l||_2 away from it.  With lambda >= 0 the system is positive definite by construction, and lambda = 0 at cond 1e8
# cannot keep a relative distance of 1e-3 (its smallest eigenvalue is 1e-8 of the norm); there the margin is the one that
# decides the route in floating point: ev_min >= 16 K (3K + 1) 2**-52 ||H_l||_2 (Higham, Theorem 10.7: Cholesky runs to
# completion when cond_2 K (3K + 1) 2**-52 < 1 / 2 or so).  For the same reason a negative lambda that splits the levels of
# 1 and 64 samples exists only for cond(C C') of a few tens: 64 ev_min + lambda >= 1e-3 * 64 ev_max needs ev_min / ev_max
# above 1e-3.
#
# Bounds.  The device forms H_l and g_l in double.  Every entry is a sum of at most p + cnt products and differences, the
# residual entry x - u'C another K: with k = p + cnt + K + 8 and gamma_k = k 2**-53 / (1 - k 2**-53), whatever the order and
# whether the held-out part is subtracted from the full sum or the training part is summed directly,
#     |dH| <= gamma_k (cnt |C||C|' + |H|) =: E_H,      |dg| <= 2 gamma_k |C| sum_{r in l} (|x_r| + |C|'|u_r|) =: e_g.
# The device solution solves (H + dH + F) x = g + dg with F the solve's own backward error, so against the reference system
#     eta(x) <= eta_solve + eq,   eq = (||E_H||_inf ||x||_inf + ||e_g||_inf) / (||H||_inf ||x||_inf + ||g||_inf),
# eta_solve as in the module docstring (the yardstick: over the levels of the case, on the reference system rounded to
# double).  Forward, where cond_2(H) <= 1e8: ||x - x_ref||_inf / ||x_ref||_inf <= (4 K^2 2**-52 rho + 2 K eq) cond_2(H)
# (cond_inf <= K cond_2, and twice the normwise backward error for the first-order bound).
ROW_BIT = {name: 1 << i for i, name in enumerate(_lib.ROW_KERNELS)}
N_ROW = 130
ROW_LEVELS = np.repeat([1, 2, 4, 5], [1, 64, 33, 32])      # level 3 has no sample


def _launched(ds):
    mask = int(ds.info("row_kernels"))
    return {name for name, b in ROW_BIT.items() if mask & b}


def _col_factor(rng, K, p, s, rotate):
    Q, _ = np.linalg.qr(rng.standard_normal((p, K)))
    P = sr._orth(rng, K) if rotate else np.eye(K)
    return np.asfortranarray(P @ (np.sqrt(s)[:, None] * Q.T))


def _spectrum(K, cond):
    if cond == "two_cluster":
        s = np.ones(K)
        s[K - max(1, K // 4):] = 1.0 / 16.0
        return s
    return np.logspace(0.0, -np.log10(cond), K) if K > 1 else np.ones(1)


class _RowProblem:
    """X, levels, masks and the other covariate's factor of one K, with the resident data set."""

    def __init__(self, K):
        rng = np.random.default_rng(9300 + K)
        self.K, self.p = K, 2 * K + 40
        self.lev = np.asfortranarray(np.stack([rng.permutation(ROW_LEVELS),
                                               rng.permutation(np.arange(N_ROW) % 3 + 1)], axis=1).astype(np.int32))
        self.X = np.asfortranarray(rng.standard_normal((N_ROW, self.p)))
        self.Mtr = np.asfortranarray(rng.random((N_ROW, self.p)) < 0.8, dtype=np.uint8)
        self.A = [np.asfortranarray(rng.standard_normal((5, K)) * 0.5), np.asfortranarray(rng.standard_normal((3, K)) * 0.5)]
        self.rng = rng
        self.ds = api.InsiderData(self.X, self.lev, self.Mtr, np.asfortranarray(1 - self.Mtr, dtype=np.uint8),
                                  n_levels=[5, 3])

    def equations(self, Cm, lam, tuning):
        """Per non-empty level of covariate 0: (level, H, g, E_H, e_g) in longdouble."""
        LD = sr.LD
        C = Cm.astype(LD)
        U = self.A[1].astype(LD)[self.lev[:, 1] - 1]
        resid = self.X.astype(LD) - U @ C
        absC = np.abs(C)
        mag = np.abs(self.X).astype(LD) + np.abs(U) @ absC
        out = []
        for l in (1, 2, 4, 5):
            rows = np.flatnonzero(self.lev[:, 0] == l)
            cnt = rows.size
            if tuning == 1:
                M = self.Mtr[rows].astype(LD)
                H = (C * M.sum(axis=0)) @ C.T
                g = C @ (M * resid[rows]).sum(axis=0)
            else:
                H = LD(cnt) * (C @ C.T)
                g = C @ resid[rows].sum(axis=0)
            H = H + LD(lam) * np.eye(self.K, dtype=LD)
            k = self.p + cnt + self.K + 8
            gam = LD(k * 2.0 ** -53 / (1 - k * 2.0 ** -53))
            E_H = gam * (LD(cnt) * (absC @ absC.T) + np.abs(H))
            e_g = 2 * gam * (absC @ mag[rows].sum(axis=0))
            out.append((l, H, g, E_H, e_g))
        return out

    def split_lambda(self, Cm, tuning):
        """Minus the geometric mean of the smallest eigenvalues of the 1-sample and the 64-sample level's Gram part."""
        ev = {l: np.linalg.eigvalsh(H.astype(np.float64))[0] for l, H, *_ in self.equations(Cm, 0.0, tuning)}
        assert 0 < ev[1] < ev[2]
        return -float(np.sqrt(ev[1] * ev[2]))


@functools.lru_cache(maxsize=None)
def _row_problem(K):
    return _RowProblem(K)


def _row_configs(K):
    """(form asserted, tuning, options, yardstick of the positive-definite route)"""
    pd = "gj_nopivot" if K <= 31 else "chol"
    cfg = [("merged_solve" if K <= 31 else "level_solve", 1, dict(row_merged=2, row_fused=1), pd)]
    if K <= 31:
        cfg.append(("level_solve", 1, dict(row_merged=2, row_fused=0), pd))
    cfg.append(("merged_zero", 0, dict(row_merged=1, row_fused=1), pd))
    return cfg


ROW_CASES = [(c, lam, True) for c in (1.0, 1e4, 1e8) for lam in (0.0, 1e-3)] + \
            [(1e4, 0.0, False), (1e4, 1e-3, False), (1.0, "split", True), ("two_cluster", "split", True)]


@pytest.mark.parametrize("K", EDGES)
def test_row_update_by_kernel_form(K):
    P = _row_problem(K)
    for cond, lam_spec, rotate in ROW_CASES:
        Cm = _col_factor(np.random.default_rng(9400 + K), K, P.p, _spectrum(K, cond), rotate)
        ref = {}
        for form, tuning, opts, pd_yard in _row_configs(K):
            if tuning not in ref:                       # the reference of the case, once per tuning
                lam = P.split_lambda(Cm, tuning) if lam_spec == "split" else lam_spec
                levels = []
                yard = {}
                for l, H, g, E_H, e_g in P.equations(Cm, lam, tuning):
                    ev = np.linalg.eigvalsh(H.astype(np.float64))
                    norm = np.abs(ev).max()
                    if lam < 0:
                        assert np.abs(ev).min() >= 1e-3 * norm, (K, cond, lam, l, ev[:3])
                    else:
                        assert ev[0] >= 16 * K * (3 * K + 1) * EPS * norm, (K, cond, lam, l, ev[:3])
                    info = {}
                    x, route = sr.solve_likely_sympd(H, g, info)
                    assert route == (0 if ev[0] > 0 else 1), (K, cond, lam, l)
                    Hd, gd = H.astype(np.float64), g.astype(np.float64)
                    name = pd_yard if route == 0 else "gj_rowpivot"
                    yard[name] = max(yard.get(name, 0.0), sr.backward_error(Hd, gd, YARDSTICKS[name](Hd, gd)))
                    levels.append((l, H, g, E_H, e_g, x, route, info["rho"], norm / np.abs(ev).min(), name))
                if lam_spec == "split":                 # the two levels fall on different sides of definiteness
                    assert [lv[6] for lv in levels][:2] == [1, 0], (K, cond, lam)
                ref[tuning] = (lam, levels, yard)
            lam, levels, yard = ref[tuning]
            for name, v in opts.items():
                P.ds.set_option(name, v)
            A = [a.copy(order="F") for a in P.A]
            got = P.ds.optimize_row(A, Cm, 0, lambda_=lam, tuning=tuning)
            kernels = _launched(P.ds)
            assert form in kernels, (K, form, sorted(kernels))
            assert ("merged_solve" in kernels) == (K <= 31 and opts["row_fused"] == 1), (K, form, sorted(kernels))
            assert ("level_solve" in kernels) == (K >= 32 or opts["row_fused"] == 0), (K, form, sorted(kernels))
            assert np.array_equal(got[2], P.A[0][2]), (K, form, "the empty level's row changed")
            rb = rf = 0.0
            bad = []
            for l, H, g, E_H, e_g, x, route, rho, cond2, yname in levels:
                xd = got[l - 1].astype(sr.LD)
                assert np.all(np.isfinite(got[l - 1])), (K, form, l)
                xn = np.abs(xd).max()
                eq = float((np.abs(E_H).sum(axis=1).max() * xn + np.abs(e_g).max()) /
                           (np.abs(H).sum(axis=1).max() * xn + np.abs(g).max()))
                solve = min(K * (3 * K + 1) * EPS * rho, max(8.0 * yard[yname], 4.0 * EPS))
                ratio_b = sr.backward_error(H, g, xd) / (solve + eq)
                ratio_f = 0.0
                if cond2 <= FWD_COND:
                    fwd = float(np.abs(xd - x).max() / np.abs(x).max())
                    ratio_f = fwd / ((4 * K * K * EPS * rho + 2 * K * eq) * cond2)
                rb, rf = max(rb, ratio_b), max(rf, ratio_f)
                if not (ratio_b <= 1 and ratio_f <= 1):
                    bad.append((l, route, ratio_b, ratio_f))
            key = ("row", form, "lambda<0" if lam < 0 else "lambda>=0")
            w = WORST.get(key, (0.0, 0.0))
            WORST[key] = (max(w[0], rb), max(w[1], rf))
            print(f"solve-forms row {form} K={K} cond={cond} lambda={lam:.3g} rotate={rotate}: error/bound backward {rb:.3g} "
                  f"forward {rf:.3g}; worst so far backward {WORST[key][0]:.3g} forward {WORST[key][1]:.3g}")
            assert not bad, (K, form, cond, lam, bad)


# ----------------------------------------------------------------------------------------------------------------------
# c. the ridge columns (alpha = 0)
# ----------------------------------------------------------------------------------------------------------------------
# ds.optimize_col(alpha = 0), masked: gene j solves (R_j'R_j + lambda I) c = R_j'x_j over its training rows, by
# k_ridge_cols_reg (K <= 32: four genes per wave, ridge_solve_regs; a gene whose elimination meets a non-positive pivot is
# marked and k_ridge_cols runs again for the marked genes only) or by k_ridge_cols (K > 32: LDS Cholesky at pitch K, then the
# pivoted elimination on a reloaded system).  The kernel is asserted through info("col_solver").  (The batch entry
# strong_coordinate_descent(alpha = 0) does not reach these kernels: with lambda alpha = 0 it runs the elastic-net group
# kernels, coordinate descent without an l1 term.  Only the column update launches the ridge kernels.)
#
# Genes are "rich" (about 85 % of the n = 3 K + 40 samples train) or "poor" (K / 8 training rows, at least one: the Gram
# part is rank deficient, and its few non-zero eigenvalues lie far above the rich genes' smallest).
# A negative lambda between the two kinds' smallest eigenvalues makes every poor gene indefinite and leaves every rich gene
# positive definite; the poor genes sit alone in each of the four positions of a wave, in every pair of positions, in none
# and in all of them, and in a partial last wave of p mod 4 = 1, 2, 3 genes.  EVERY gene's reference system keeps its
# eigenvalue nearest to zero at least 1e-3 of its norm away from it (asserted).
#
# These systems are benign (cond_2 below 300).  test_ridge_columns_families further down puts the families i-iii of (a)
# through the same two kernels.
#
# Reference: G_j, q_j from their definition (X, mask, A) in longdouble, then solve_likely_sympd; beside it the oracle's
# optimize_col.  Bounds as in (b): the device forms R in double (one rounding per entry and covariate) and
# XtX_j = R'R - (held-out part), so with k = n + 10
#     |dG| <= gamma_k (|R|'|R| + |G_j|) =: E_G,    |dq| <= 2 gamma_k |R|'|x_j| =: e_q      (|R|'|R| over all n rows)
# and eta <= eta_solve + eq, forward <= (4 K^2 2**-52 rho + 2 K eq) cond_2(G_j); against the oracle (LAPACK in double, the
# same forward bound of its own) twice that.
POOR_PATTERNS = ["1000", "0100", "0010", "0001", "1100", "1010", "1001", "0110", "0101", "0011", "0000", "1111"]
LAST_WAVE = {1: "1", 2: "01", 3: "101"}


def _col_solver(ds):
    return _lib.COL_SOLVERS[int(ds.info("col_solver"))]


class _ColProblem:
    def __init__(self, K, p):
        from insider_amd import workloads
        rng = np.random.default_rng(9500 + 10 * K + p)
        self.K, self.p, self.n = K, p, 3 * K + 40
        n = self.n
        counts = (n // 2, 7)
        self.lev = workloads.cyclic_levels(n, counts)
        self.A = [np.asfortranarray(rng.standard_normal((L, K)) * 0.5) for L in counts]
        self.poor = np.array([ch == "1" for ch in "".join(POOR_PATTERNS) + LAST_WAVE[p % 4]])
        assert self.poor.size == p
        self.R = sum(self.A[i][self.lev[:, i] - 1, :] for i in range(2))
        self.X = np.asfortranarray(self.R @ rng.standard_normal((K, p)) + 0.5 * rng.standard_normal((n, p)))
        train = rng.random((n, p)) < 0.85
        for j in np.flatnonzero(self.poor):
            train[:, j] = False
            train[rng.permutation(n)[:max(1, K // 8)], j] = True
        self.Mtr = np.asfortranarray(train, dtype=np.uint8)
        self.Mte = np.asfortranarray(~train, dtype=np.uint8)
        self.C0 = np.asfortranarray(rng.standard_normal((K, p)) * 0.3)
        LD = sr.LD
        Rq = self.A[0].astype(LD)[self.lev[:, 0] - 1] + self.A[1].astype(LD)[self.lev[:, 1] - 1]
        k = n + 10
        gam = LD(k * 2.0 ** -53 / (1 - k * 2.0 ** -53))
        absR = np.abs(Rq)
        full = absR.T @ absR
        self.gram, self.q, self.e_q = [], [], []
        for j in range(p):
            rows = np.flatnonzero(train[:, j])
            self.gram.append(Rq[rows].T @ Rq[rows])
            self.q.append(Rq[rows].T @ self.X[rows, j].astype(LD))
            self.e_q.append(2 * gam * (absR.T @ np.abs(self.X[:, j]).astype(LD)))
        self.full, self.gam = full, gam
        self.ev = [np.linalg.eigvalsh(g.astype(np.float64)) for g in self.gram]

    def split_lambda(self):
        """Minus a fraction of the rich genes' smallest eigenvalue: the fraction (of a fixed grid) that keeps every gene's
        eigenvalues farthest from zero relative to its norm."""
        rich_min = min(self.ev[j][0] for j in np.flatnonzero(~self.poor))
        assert rich_min > 0

        def gap(lam):
            return min(np.abs(ev + lam).min() / np.abs(ev + lam).max() for ev in self.ev)
        cand = [lam for lam in -np.linspace(0.1, 0.8, 57) * rich_min
                if all(self.ev[j][0] + lam < 0 for j in np.flatnonzero(self.poor))]
        assert cand, (self.K, self.p)
        return float(max(cand, key=gap))

    def reference(self, lam, pd_yard):
        """Per gene: (G, q, E_G, e_q, x, route, rho, cond_2, yardstick name), and the yardsticks' largest backward error."""
        out, yard = [], {}
        eye = np.eye(self.K, dtype=sr.LD)
        for j in range(self.p):
            G = self.gram[j] + sr.LD(lam) * eye
            ev = self.ev[j] + lam
            if lam < 0:
                assert np.abs(ev).min() >= 1e-3 * np.abs(ev).max(), (self.K, self.p, j, lam, ev[:3])
            else:       # positive definite by construction: the margin of (b) for lambda >= 0
                assert ev[0] >= 16 * self.K * (3 * self.K + 1) * EPS * ev[-1], (self.K, self.p, j, lam, ev[:3])
            info = {}
            x, route = sr.solve_likely_sympd(G, self.q[j], info)
            assert route == (0 if ev[0] > 0 else 1), (self.K, j)
            Gd, qd = G.astype(np.float64), self.q[j].astype(np.float64)
            name = pd_yard if route == 0 else "gj_rowpivot"
            yard[name] = max(yard.get(name, 0.0), sr.backward_error(Gd, qd, YARDSTICKS[name](Gd, qd)))
            E_G = self.gam * (self.full + np.abs(G))
            out.append((G, self.q[j], E_G, self.e_q[j], x, route, info["rho"], float(np.abs(ev).max() / np.abs(ev).min()), name))
        return out, yard


def _check_cols(label, K, got, ref, yard, other=None):
    """got: K x p.  The bounds of section (c) for every gene; `other` (K x p, optional): the oracle's result, held to twice the
    forward bound."""
    rb = rf = ro = 0.0
    bad = []
    for j, (G, q, E_G, e_q, x, route, rho, cond2, yname) in enumerate(ref):
        xd = got[:, j].astype(sr.LD)
        assert np.all(np.isfinite(got[:, j])), (label, K, j)
        xn = np.abs(xd).max()
        eq = float((np.abs(E_G).sum(axis=1).max() * xn + np.abs(e_q).max()) / (np.abs(G).sum(axis=1).max() * xn + np.abs(q).max()))
        solve = min(K * (3 * K + 1) * EPS * rho, max(8.0 * yard[yname], 4.0 * EPS))
        ratio_b = sr.backward_error(G, q, xd) / (solve + eq)
        fbound = (4 * K * K * EPS * rho + 2 * K * eq) * cond2
        ratio_f = float(np.abs(xd - x).max() / np.abs(x).max()) / fbound if cond2 <= FWD_COND else 0.0
        ratio_o = 0.0
        if other is not None:
            assert cond2 <= FWD_COND, (label, K, j)
            ratio_o = float(np.abs(xd - other[:, j].astype(sr.LD)).max() / np.abs(x).max()) / (2 * fbound)
        rb, rf, ro = max(rb, ratio_b), max(rf, ratio_f), max(ro, ratio_o)
        if not (ratio_b <= 1 and ratio_f <= 1 and ratio_o <= 1):
            bad.append((j, route, ratio_b, ratio_f, ratio_o))
    w = WORST.get(("cols", label), (0.0, 0.0, 0.0))
    WORST[("cols", label)] = (max(w[0], rb), max(w[1], rf), max(w[2], ro))
    print(f"solve-forms cols {label} K={K} p={got.shape[1]}: error/bound backward {rb:.3g} forward {rf:.3g} oracle {ro:.3g}; "
          f"worst so far {WORST[('cols', label)]}")
    assert not bad, (label, K, bad[:5])


@pytest.mark.parametrize("K", EDGES)
def test_ridge_columns_mixed_waves(oracle, K):
    kernel = "ridge_reg" if K <= 32 else "ridge"
    pd_yard = "gj_nopivot" if K <= 32 else "chol"
    for p in (49, 50, 51):
        P = _ColProblem(K, p)
        lam = P.split_lambda()
        ref, yard = P.reference(lam, pd_yard)
        assert [r[5] for r in ref] == [1 if poor else 0 for poor in P.poor]     # the poor genes, and only they, retry
        ds = api.InsiderData(P.X, P.lev, P.Mtr, P.Mte)
        fresh = api.InsiderData(P.X, P.lev, P.Mtr, P.Mte)
        try:
            got = ds.optimize_col(P.A, P.C0.copy(order="F"), lambda_=lam, alpha=0.0, tuning=1)
            assert _col_solver(ds) == kernel and ds.info("col_ridge_fallback") == (kernel == "ridge_reg")
            orc = None
            if p == 51:
                orc, _ = oracle.optimize_col(P.X, P.Mtr, P.R, P.C0, lam, 0.0, tuning=1)
            _check_cols(f"{kernel} mixed", K, got, ref, yard, orc)
            again = ds.optimize_col(P.A, P.C0.copy(order="F"), lambda_=lam, alpha=0.0, tuning=1)
            assert np.array_equal(again, got), (K, p)
            if p != 51:
                continue
            # a following all-positive-definite call on the same handle: the marks do not leak
            lam_pd = abs(lam)
            ref_pd, yard_pd = P.reference(lam_pd, pd_yard)
            assert all(r[5] == 0 for r in ref_pd)
            after = ds.optimize_col(P.A, P.C0.copy(order="F"), lambda_=lam_pd, alpha=0.0, tuning=1)
            _check_cols(f"{kernel} after", K, after, ref_pd, yard_pd)
            clean = fresh.optimize_col(P.A, P.C0.copy(order="F"), lambda_=lam_pd, alpha=0.0, tuning=1)
            assert np.array_equal(after, clean), (K, p)
            if kernel == "ridge_reg":
                # the retry pass does not touch an unmarked gene: with every poor gene's mask replaced by a full one (its
                # Gram part then dominates every rich gene's, so it is positive definite under the same lambda) no gene is
                # marked, and the rich genes, whose data and masks are the same, come out the same by bits
                full = P.Mtr.copy(order="F")
                full[:, P.poor] = 1
                nomark = api.InsiderData(P.X, P.lev, full, np.asfortranarray(1 - full, dtype=np.uint8))
                try:
                    plain = nomark.optimize_col(P.A, P.C0.copy(order="F"), lambda_=lam, alpha=0.0, tuning=1)
                    assert _col_solver(nomark) == "ridge_reg"
                finally:
                    nomark.close()
                assert np.array_equal(plain[:, ~P.poor], got[:, ~P.poor]), K
                # the marked genes ARE the wave-per-gene kernel's work (cd_variant = 1: Cholesky, then the pivoted
                # elimination), by bits
                fresh.set_option("cd_variant", 1)
                lds = fresh.optimize_col(P.A, P.C0.copy(order="F"), lambda_=lam, alpha=0.0, tuning=1)
                assert _col_solver(fresh) == "ridge"
                _check_cols("ridge mixed", K, lds, *P.reference(lam, "chol"))
                assert np.array_equal(lds[:, P.poor], got[:, P.poor]), K
                # and the unmarked genes are NOT: a retry pass that ignored the marks would hand every gene to that kernel,
                # in this call and in every other ridge_reg call alike, so no comparison between two ridge_reg calls can
                # show it; what shows it is that the register elimination (one reciprocal per column, fused multiply-adds)
                # and the Cholesky (square roots, divisions) round differently.  Asserted from K = 3, where 37 genes with
                # 30 or more roundings each would all have to agree; at K = 1 and 2 a gene's solution is a handful of
                # roundings, and agreement there would say nothing
                if K >= 3:
                    assert not np.array_equal(lds[:, ~P.poor], got[:, ~P.poor]), K
        finally:
            ds.close()
            fresh.close()


# The families of (a) on the ridge kernels.  The column update forms its systems itself, G_j = R_j'R_j + lambda I, so a
# caller's matrix T is reached through the row factor: covariate 0 has K + 20 levels of two samples each (rows 2l and
# 2l + 1), covariate 1 two levels and a zero factor, so R = A0[level] exactly, and with A0 = U F / sqrt 2 (U: (K + 20) x K
# with orthonormal columns) the unmasked Gram matrix is R'R = 2 A0'A0 = F'F up to the rounding of A0:
#     i    spd         F = diag(sqrt s) Q', lambda = 0:       F'F = Q diag(s) Q', cond 1, 1e4, 1e8, 1e12
#     ii   scaled      F = diag(sqrt s) Q' D, lambda = 0:     F'F = D Q diag(s) Q' D, D = diag(10**u), u in [-3, 3]
#     iii  indefinite  F'F = T + mu I (Cholesky), lambda = -mu: G = T = sr.indefinite(K, pos), the first non-positive pivot
#                      at position 0, K / 2 and K - 1; mu = -ev_min(T) + ||T||_2 / 2
#     iv   zero_diag   cannot be reached: a diagonal entry of G is a sum of squares plus lambda, and it is exactly zero only
#                      where fl(sum of squares) = -lambda by bits, which the caller of a column update does not control.
# Unmasked (tuning = 0) the nine genes of a call share G and differ in their right-hand sides, so a wave of the register
# kernel holds the same ill-conditioned system four times; masked (tuning = 1, families i and ii) gene j keeps every first
# sample and a random half of the second ones, G_j = A0' W_j A0 with W_j = diag(1 or 2): between F'F / 2 and F'F in the
# Loewner order, so positive definite with cond_2 within a factor 2 of the family's, and different in every gene of a wave.
# K <= 32 runs both kernels (cd_variant 0: ridge_reg, with the indefinite genes retried in ridge; 1: ridge), K > 32 ridge.
#
# The reference is the longdouble Gram matrix of the float64 A0 that the device receives, so the rounding of A0 is no error
# of the device.  Bounds as above; the forward bound only where cond_2 <= 1e8 (family i unmasked: the cond it was built
# for), and the route of the reference is asserted for every gene (0 in i and ii, 1 in iii).
GRAM_P = 9                                                   # two waves of four genes and a partial one


class _GramProblem:
    def __init__(self, K):
        rng = np.random.default_rng(9600 + K)
        self.K, self.L = K, K + 20
        n = self.n = 2 * self.L
        r = np.arange(n)
        self.lev = np.asfortranarray(np.stack([r // 2 + 1, r % 2 + 1], axis=1).astype(np.int32))
        self.X = np.asfortranarray(rng.standard_normal((n, GRAM_P)))
        self.train = np.ones((n, GRAM_P), dtype=bool)
        self.train[1::2] = rng.random((self.L, GRAM_P)) < 0.5
        self.C0 = np.asfortranarray(rng.standard_normal((K, GRAM_P)) * 0.3)
        self.U = np.linalg.qr(rng.standard_normal((self.L, K)))[0]
        self.rng = rng
        self.ds = api.InsiderData(self.X, self.lev, np.asfortranarray(self.train, dtype=np.uint8),
                                  np.asfortranarray(~self.train, dtype=np.uint8), n_levels=[self.L, 2])

    def systems(self):
        """(family, F, lambda, the cond it was built for or None, the route expected)"""
        K, rng = self.K, self.rng
        out = []
        for cond in (1.0, 1e4, 1e8, 1e12):
            s = np.logspace(0.0, -np.log10(cond), K) if K > 1 else np.ones(1)
            out.append(("spd", np.sqrt(s)[:, None] * sr._orth(rng, K).T, 0.0, cond if K > 1 else 1.0, 0))
            d = 10.0 ** rng.uniform(-3.0, 3.0, K)
            out.append(("scaled", np.sqrt(s)[:, None] * sr._orth(rng, K).T * d[None, :], 0.0, None, 0))
        for pos in sr.indefinite_positions(K):
            T = sr.indefinite(rng, K, pos)
            ev = np.linalg.eigvalsh(T)
            mu = float(-ev[0] + 0.5 * np.abs(ev).max())
            out.append(("indefinite", np.linalg.cholesky(T + mu * np.eye(K)).T, -mu, None, 1))
        return out

    def factors(self, F):
        return [np.asfortranarray(self.U @ F / np.sqrt(2.0)), np.zeros((2, self.K), order="F")]

    def reference(self, A0, lam, tuning, built, want_route):
        """Per gene: (G, q, E_G, e_q, x, route, rho, cond_2, "pd" or "gj_rowpivot"), and the largest backward error of each
        float64 yardstick of the route."""
        LD, K = sr.LD, self.K
        Rq = A0.astype(LD)[self.lev[:, 0] - 1]
        k = self.n + 10
        gam = LD(k * 2.0 ** -53 / (1 - k * 2.0 ** -53))
        absR = np.abs(Rq)
        full = absR.T @ absR
        out, yard = [], {}
        for j in range(GRAM_P):
            rows = np.flatnonzero(self.train[:, j]) if tuning == 1 else np.arange(self.n)
            G = Rq[rows].T @ Rq[rows] + LD(lam) * np.eye(K, dtype=LD)
            q = Rq[rows].T @ self.X[rows, j].astype(LD)
            info = {}
            x, route = sr.solve_likely_sympd(G, q, info)
            assert route == want_route, (K, j, lam, tuning, route)
            Gd, qd = G.astype(np.float64), q.astype(np.float64)
            for name in (("gj_nopivot", "chol") if route == 0 else ("gj_rowpivot",)):
                y = YARDSTICKS[name](Gd, qd)
                assert y is not None and np.all(np.isfinite(y)), (K, j, name)
                yard[name] = max(yard.get(name, 0.0), sr.backward_error(Gd, qd, y))
            cond2 = built
            if built is None or tuning == 1:
                ev = np.abs(np.linalg.eigvalsh(Gd))
                cond2 = float(ev.max() / ev.min()) if ev.min() > 0 else np.inf
            E_G = gam * (full + np.abs(G))
            e_q = 2 * gam * (absR.T @ np.abs(self.X[:, j]).astype(LD))
            out.append((G, q, E_G, e_q, x, route, info["rho"], cond2, "pd" if route == 0 else "gj_rowpivot"))
        return out, yard


@pytest.mark.parametrize("K", EDGES)
def test_ridge_columns_families(K):
    P = _GramProblem(K)
    variants = [(0, "ridge_reg", "gj_nopivot"), (1, "ridge", "chol")] if K <= 32 else [(0, "ridge", "chol")]
    try:
        for family, F, lam, built, want_route in P.systems():
            A = P.factors(F)
            for tuning in ((0, 1) if family != "indefinite" else (0,)):
                ref, yard = P.reference(A[0], lam, tuning, built, want_route)
                for variant, kernel, pd_yard in variants:
                    P.ds.set_option("cd_variant", variant)
                    got = P.ds.optimize_col(A, P.C0.copy(order="F"), lambda_=lam, alpha=0.0, tuning=tuning)
                    assert _col_solver(P.ds) == kernel and P.ds.info("col_ridge_fallback") == (kernel == "ridge_reg")
                    if want_route == 0:
                        yard["pd"] = yard[pd_yard]
                    _check_cols(f"{kernel} {family} {'masked' if tuning else 'unmasked'}", K, got, ref, yard)
    finally:
        P.ds.close()
