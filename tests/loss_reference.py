"""A plain high-precision reference of the fit's loss checkpoint (evaluate() and compute_loss(), src/utils.cpp:56-102), for
the tests that compare the device's checkpoint evaluator by evaluator: every quantity in ``np.longdouble``, the residual
formed entry by entry, squared and summed (no difference of sums of squares).  Nothing of the product is imported.

The device never forms a residual (DESIGN §2 "Loss checkpoints"): per gene it writes
    sum_train (x - r'b)^2 = yy - b'(q + g),                    q = X'y, G = X'X over the train entries, g = q - G b,
    sum_test  (x - r'b)^2 = ss_held + b'(R'R b - (q - g) - 2 qc)      (data without NA entries),
with q = R'x - qc and G = R'R - Gc formed as full sums minus the complements over the held-out entries.  bounds() states
what forward error that route may have, emulate_identity() is the route in float64 NumPy, and planted() / the grids below
are the data both test files run on.

EXTENDED tells whether the host's long double is wider than double; where it is not, the reference carries double
rounding itself and only the bounds' slack (three orders, see tests/test_loss_reference_cpu.py) covers it."""
import functools

import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps < np.finfo(np.float64).eps)
U = 2.0 ** -53


def gamma(m):
    """gamma_m = m u / (1 - m u): the bound on the relative error of m successive roundings."""
    mu = LD(m) * LD(U)
    return mu / (LD(1) - mu)


def _levels(levels, n):
    return np.asarray(levels).reshape(n, -1, order="F").astype(np.int64)


def row_factor(levels, A, ctns=None, dtype=LD):
    """R = sum_i A_i[level_i] (+ Z A_c): n x K."""
    n = np.asarray(levels).shape[0]
    lev = _levels(levels, n)
    c = lev.shape[1]
    R = sum(np.asarray(A[i], dtype=dtype)[lev[:, i] - 1, :] for i in range(c))
    if ctns is not None:
        R = R + np.asarray(ctns, dtype=dtype).reshape(n, -1) @ np.asarray(A[c], dtype=dtype)
    return R


def product(R, C):
    """R C in longdouble (NumPy's longdouble matmul has no BLAS behind it and is several times slower on a column-major C)."""
    return np.ascontiguousarray(R, dtype=LD) @ np.ascontiguousarray(C, dtype=LD)


def fitted(levels, A, C, ctns=None):
    """R C in longdouble as sum_i (A_i C)[level_i] (+ Z (A_c C)): the same entries from fewer products (sum L rows, not n)."""
    n = np.asarray(levels).shape[0]
    lev = _levels(levels, n)
    c = lev.shape[1]
    out = sum(product(A[i], C)[lev[:, i] - 1, :] for i in range(c))
    if ctns is not None:
        out = out + product(np.asarray(ctns, dtype=LD).reshape(n, -1), product(A[c], C))
    return out


def _masks(X, M_train, M_test, tuning):
    """(train, test) as boolean n x p; tuning = 0: every entry is train and none is test."""
    if tuning == 0:
        return np.ones(X.shape, dtype=bool), np.zeros(X.shape, dtype=bool)
    if tuning != 1:
        raise ValueError("tuning is 0 or 1")
    return np.asarray(M_train) != 0, np.asarray(M_test) != 0


def _rmse(sse, cnt):
    return float(np.sqrt(sse / LD(cnt))) if cnt > 0 else float("nan")


def penalties(A, C, lam1, lam2, alpha):
    """The penalties of compute_loss(): (row_reg_half, col_reg_half, l1_reg), longdouble."""
    Cl = np.asarray(C, dtype=LD)
    return (LD(lam1) * sum((np.asarray(a, dtype=LD) ** 2).sum() for a in A) / 2,
            LD(lam2) * (LD(1) - LD(alpha)) * (Cl * Cl).sum() / 2, LD(lam2) * LD(alpha) * np.abs(Cl).sum())


def residual_sums(X, levels, n_levels, A, C, M_train, M_test, tuning, ctns=None, with_bounds=False):
    """The part of evaluate() that does not depend on the penalties (and, with_bounds, bounds() from the same residual)."""
    Xl = np.asarray(X, dtype=LD)
    n, p = Xl.shape
    c = _levels(levels, n).shape[1]
    if [int(L) for L in n_levels] != [np.asarray(A[i]).shape[0] for i in range(c)]:
        raise ValueError("row factors do not match n_levels")
    Cl = np.asarray(C, dtype=LD)
    res = Xl - fitted(levels, A, Cl, ctns)
    sq = res * res
    train, test = _masks(Xl, M_train, M_test, tuning)
    tr_gene = np.where(train, sq, LD(0)).sum(axis=0)
    te_gene = np.where(test, sq, LD(0)).sum(axis=0)
    sse_train, sse_test = tr_gene.sum(), te_gene.sum()
    cnt_train, cnt_test = int(train.sum()), int(test.sum())
    out = dict(sse_train=sse_train, sse_test=sse_test, cnt_train=cnt_train, cnt_test=cnt_test,
               train_rmse=_rmse(sse_train, cnt_train), test_rmse=_rmse(sse_test, cnt_test) if tuning == 1 else float("nan"),
               sse_half=sse_train / 2, sse_train_gene=tr_gene, sse_test_gene=te_gene)
    if with_bounds:
        out["bounds"] = _bounds(Xl, row_factor(levels, A, ctns, dtype=np.float64), Cl, len(A) if ctns is None else c + np.asarray(ctns).reshape(n, -1).shape[1],
                                sum(np.asarray(a).shape[0] for a in A), np.abs(res), train, test, tuning)
    return out


def with_penalties(sums, A, C, lam1, lam2, alpha):
    """residual_sums() completed to evaluate()'s dict."""
    row_reg_half, col_reg_half, l1_reg = penalties(A, C, lam1, lam2, alpha)
    return dict(sums, row_reg_half=row_reg_half, col_reg_half=col_reg_half, l1_reg=l1_reg,
                loss=sums["sse_half"] + row_reg_half + col_reg_half + l1_reg)


def evaluate(X, levels, n_levels, A, C, M_train, M_test, lam1, lam2, alpha, tuning, ctns=None):
    """The checkpoint of the factors (A, C) in its direct form.  -> dict of
        sse_train, sse_test (longdouble), cnt_train, cnt_test, train_rmse, test_rmse (NaN when tuning = 0 or no test entry),
        sse_half, row_reg_half, col_reg_half, l1_reg, loss (longdouble; the penalties of compute_loss()),
        sse_train_gene, sse_test_gene (p, longdouble)."""
    return with_penalties(residual_sums(X, levels, n_levels, A, C, M_train, M_test, tuning, ctns), A, C, lam1, lam2, alpha)


def bounds(X, levels, n_levels, A, C, M_train, M_test, tuning, ctns=None):
    """Forward-error bounds of the device's route, u = 2^-53.  -> dict of

    bound_stats: of every sum formed from statistics (sse_train always; sse_test on data without NA entries),
        gamma_m sum_j scale_j,  m = n + 2K + B + 16,
        scale_j = sum_i x_ij^2 + 2 |b_j|'|R|'|x_j| + |b_j|'(|R|'|R|)|b_j| = sum_i (|x_ij| + |R_i||b_j|)^2  over ALL n samples:
        q and G are full sums minus held-out complements, so their roundings scale with the full sums.  m counts the
        roundings of the longest sum involved: n terms of a product sum, K + K of b'(q + g) with g = q - G b, B blocks summed
        into a row of R (the covariates and the continuous columns), 16 for the wave and block reduction trees, the
        subtraction yy - b'(q + g) and the strided sum over the genes.
    bound_direct: of sse_test from explicit residuals (data with NA entries),
        sum_test (2 |r_ij| e_ij + e_ij^2) + gamma_len sse_test,  e_ij = gamma_{K+B+2} (|x_ij| + |R_i||b_j|),
        len = the longest held-out list + 16 + ceil(p / 256): the entries one lane chain and the wave tree sum (at most the
        list), plus the roundings the derivation from the list alone misses: the square itself, the six levels of the wave
        tree, and k_loss_reduce's strided sum over the genes (ceil(p / 256)) and its eight-level block tree.  0 when
        tuning = 0.
    rel_penalty: relative, (max(sum L, p) K + 16) u: sums of non-negative terms (sum L counts the continuous columns too).
    scale: sum_j scale_j."""
    Xl = np.asarray(X, dtype=LD)
    n = Xl.shape[0]
    Cl = np.asarray(C, dtype=LD)
    train, test = _masks(Xl, M_train, M_test, tuning)
    B = len(A) if ctns is None else _levels(levels, n).shape[1] + np.asarray(ctns).reshape(n, -1).shape[1]
    return _bounds(Xl, row_factor(levels, A, ctns, dtype=np.float64), Cl, B, sum(np.asarray(a).shape[0] for a in A),
                   np.abs(Xl - fitted(levels, A, Cl, ctns)), train, test, tuning)


def _bounds(Xl, R, Cl, B, levels_total, absres, train, test, tuning):
    n, p = Xl.shape
    K = Cl.shape[0]
    # |x_ij| + |R_i||b_j|: a sum of non-negative terms, formed in float64 (R in float64, the product on BLAS) and rounded up by
    # its own gamma_{K+B+2}, so that no bound is below the stated one
    reach = (np.abs(Xl) + (np.abs(R) @ np.abs(Cl).astype(np.float64)).astype(LD)) * (1 + gamma(K + B + 2))
    scale = (reach * reach).sum()
    out = dict(scale=scale, bound_stats=gamma(n + 2 * K + B + 16) * scale, bound_direct=LD(0),
               rel_penalty=(max(levels_total, p) * K + 16) * U)
    if tuning == 1:
        e = gamma(K + B + 2) * reach
        length = int((~train).sum(axis=0).max()) + 16 + -(-p // 256)
        out["bound_direct"] = (np.where(test, 2 * absres * e + e * e, LD(0)).sum()
                               + gamma(length) * np.where(test, absres * absres, LD(0)).sum())
    return out


def has_na(M_train, M_test):
    return bool(((np.asarray(M_train) != 0) | (np.asarray(M_test) != 0)).sum() < np.asarray(M_train).size)


def emulate_identity(X, levels, A, C, M_train, M_test, tuning, ctns=None):
    """The two identities in float64 NumPy, as the kernels write them: what a correct float64 implementation of the route
    loses.  The test sum is the direct float64 sum where the data has NA entries (k_test_sse_list).  -> dict of sse_train,
    sse_test (float64: the per-gene values summed), sse_train_gene, sse_test_gene, negative (genes whose train value is < 0)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    C = np.asarray(C, dtype=np.float64)
    R = row_factor(levels, A, ctns, dtype=np.float64)
    RtR = R.T @ R
    Qfull = R.T @ X
    yy_all = (X * X).sum(axis=0)
    train, test = _masks(X, M_train, M_test, tuning)
    direct = tuning == 1 and has_na(M_train, M_test)
    tr, te = np.zeros(p), np.zeros(p)
    for j in range(p):
        b = C[:, j]
        if tuning == 0:
            q, G, yy = Qfull[:, j], RtR, yy_all[j]
        else:
            held = ~train[:, j]
            Rh, xh = R[held], X[held, j]
            qc = Rh.T @ xh
            q, G = Qfull[:, j] - qc, RtR - Rh.T @ Rh
            yy = (X[train[:, j], j] ** 2).sum()
        g = q - G @ b
        tr[j] = yy - b @ (q + g)
        if direct:
            sel = test[:, j]
            te[j] = ((X[sel, j] - R[sel] @ b) ** 2).sum()
        elif tuning == 1:
            te[j] = (yy_all[j] - yy) + b @ (RtR @ b - (q - g) - 2.0 * qc)
    return dict(sse_train=float(tr.sum()), sse_test=float(te.sum()), sse_train_gene=tr, sse_test_gene=te,
                negative=int((tr < 0).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# the data of the GPU tests (tests/test_gpu_loss_checkpoint.py) and of the CPU check of the bounds on the same cells
# ----------------------------------------------------------------------------------------------------------------------
N, P, LEVELS = 240, 77, (120, 7)   # p = 77: the last wave is partial at 4 and at 16 genes per wave
G_EMPTY, G_HELD = 5, 40            # a gene that is all zero, a gene whose every entry is held out
DATA = ("train_test", "na", "unmasked")
# (sigma, offset): noise sd of X = R C + sigma E; offset 100 = one column of R is the constant 100
CONDITIONS = ((0.5, 0.0), (1e-6, 100.0), (0.0, 0.0), (0.0, 100.0))
KS = (1, 15, 16, 17, 18, 20, 22, 24, 25, 26, 28, 30, 31, 32, 33, 47, 48, 49, 63)   # every (SLOTS, KMAX) of REG_DISPATCH, every band edge
EXACT_KS, EXACT_SEEDS, EXACT_OFFSETS = (9, 30, 40, 56), tuple(range(8)), (0.0, 100.0)


def case_seed(K, cond):
    return 1000 * K + CONDITIONS.index(cond)


def level_ids(n, level_counts):
    """Level ids 1..L_i: covariate i changes every i + 1 samples and cycles; every level occurs (n >= (i + 1) L_i)."""
    r = np.arange(n)
    lev = np.stack([(r // (i + 1)) % L + 1 for i, L in enumerate(level_counts)], axis=1)
    for i, L in enumerate(level_counts):
        assert len(np.unique(lev[:, i])) == L
    return np.asfortranarray(lev, dtype=np.int32)


@functools.lru_cache(maxsize=4)
def _drawn(K, sigma, offset, data, seed, n, p, level_counts, m, f):
    """Everything planted() draws; the wholly held-out gene is applied afterwards, so that the data with and without it share
    every draw.  (The arrays are shared between calls: planted() copies what it changes.)"""
    rng = np.random.default_rng(seed)
    levels = level_ids(n, level_counts)
    A = [np.asfortranarray(rng.standard_normal((L, K)) * 0.5) for L in level_counts]
    Z = None
    if m:
        Z = np.asfortranarray(rng.standard_normal((n, m)))
        A.append(np.asfortranarray(rng.standard_normal((m, K)) * 0.5))
    if offset:
        A[0][:, 0] = offset
        for a in A[1:]:
            a[:, 0] = 0.0
    C = np.asfortranarray(rng.standard_normal((K, p)) * (rng.random((K, p)) < 0.5))
    g_empty = G_EMPTY if p > G_HELD else p // 2
    if p >= 4:
        C[:, g_empty] = 0.0
    R = row_factor(levels, A, Z, dtype=np.float64)
    X = np.asfortranarray(R @ C + (sigma * rng.standard_normal((n, p)) if sigma else 0.0))
    if p >= 4:
        X[:, g_empty] = 0.0
    test = rng.random((n, p)) < f
    test[0, 0] = False                                   # (at least one train entry at every shape)
    na = None
    if data == "na":
        na = rng.random((n, p)) < 0.05
        na[0, 0] = False
    elif data not in ("train_test", "unmasked"):
        raise ValueError(data)
    return levels, A, Z, C, X, test, na


def planted(K, sigma, offset, data, seed, n=N, p=P, level_counts=LEVELS, m=0, held_gene=True, f=0.15):
    """Planted factors (A, C) and X = R C + sigma E in float64, with the edges of _col_case (test_gpu_col_solvers.py): one
    all-zero gene (its column of C is zero too, so that sigma = 0 stays an exact fit) and, with ``held_gene``, one gene whose
    every entry is held out.  offset != 0: column 0 of R is that constant.  data: "train_test" (a fraction f held out, no
    NA), "na" (5 % NA entries as well: x = 0, neither train nor test), "unmasked" (tuning = 0; the masks are drawn all the
    same).  m continuous columns: A carries the m x K block last and Z is returned.  -> dict."""
    levels, A, Z, C, X, test, na = _drawn(K, sigma, offset, data, seed, n, p, tuple(level_counts), m, f)
    X, test = X.copy(order="F"), test.copy()
    g_held = G_HELD if p > G_HELD else p - 1
    held_gene = held_gene and p >= 4
    if held_gene:
        test[:, g_held] = True
    Mte = np.asfortranarray(test.astype(np.uint8))
    Mtr = np.asfortranarray((~test).astype(np.uint8))
    if na is not None:
        na = na.copy()
        if held_gene:
            na[:, g_held] = False                        # (its entries stay held out)
        X[na] = 0.0
        Mtr[na] = 0
        Mte[na] = 0
    return dict(X=X, levels=levels, n_levels=np.array(level_counts, dtype=np.int32), A=A, C=C, M_train=Mtr, M_test=Mte,
                tuning=0 if data == "unmasked" else 1, ctns=Z, K=K)


# the held-out lists of the flagged-list test: n is no multiple of 32, 64 or 128; list padding to 32, and one, two and four trips
# of the 64-lane loop
LIST_N, LIST_LEVELS = 203, (29, 7)
LIST_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 200)
LIST_P = len(LIST_LENGTHS) + 2 + 13
LIST_KS, LIST_CONDITIONS, LIST_MASKS = (7, 40), ((0.5, 0.0), (0.0, 100.0)), ("lists", "no_test", "all_train")


def list_case(K, cond, masks):
    """Genes 0..8: held-out lists of exactly LIST_LENGTHS entries (every fifth entry of a list NA, the others test); gene 9:
    40 held-out entries, all NA (every flag 0); gene 10: every entry test; the others: 15 % test, 5 % NA.
    masks "no_test": the NA entries stay, no entry is test.  "all_train": no held-out entry at all."""
    d = planted(K, *cond, "train_test", 500 + K, n=LIST_N, p=LIST_P, level_counts=LIST_LEVELS, held_gene=False)
    rng = np.random.default_rng(600 + K)
    test = d["M_test"] != 0
    na = ~test & (rng.random(test.shape) < 0.05)
    for j, length in enumerate(LIST_LENGTHS):
        rows = rng.choice(LIST_N, size=length, replace=False)
        test[:, j], na[:, j] = False, False
        test[rows, j] = True
        na[rows[4::5], j] = True
    g = len(LIST_LENGTHS)
    test[:, g], na[:, g] = False, False
    na[rng.choice(LIST_N, size=40, replace=False), g] = True
    test[:, g + 1], na[:, g + 1] = True, False
    test &= ~na
    if masks == "no_test":
        test[:] = False
    elif masks == "all_train":
        test[:], na[:] = False, False
    d["X"][na] = 0.0
    d["M_test"] = np.asfortranarray(test.astype(np.uint8))
    d["M_train"] = np.asfortranarray((~test & ~na).astype(np.uint8))
    return d


# the shape edges: k_loss_reduce's stride of 256 below, at and above one and two trips; the partial last block of the launches
# of four genes per block
SHAPE_LEVELS = {5: (3, 2), 64: (16, 3), 129: (16, 3)}
SHAPE_PS = (1, 3, 4, 5, 255, 256, 257, 515)
SHAPE_K, SHAPE_CONDITIONS, SHAPE_DATA = 6, ((0.5, 0.0), (1e-6, 100.0)), ("train_test", "na")


def shape_case(p, n, data, cond):
    return planted(SHAPE_K, *cond, data, 700 + p + n, n=n, p=p, level_counts=SHAPE_LEVELS[n], held_gene=p >= 4)


# the continuous block: m = 2 columns, R carries Z A_c
CTNS_KS, CTNS_CONDITIONS, CTNS_DATA = (9, 40), ((0.5, 0.0), (1e-6, 100.0)), ("train_test", "na")


def ctns_case(K, cond, data):
    return planted(K, *cond, data, 800 + K, m=2)
