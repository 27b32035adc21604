"""What the test files share: the relative error, three fixtures (imported by name into the module that uses them), the
planted data sets of the post-hoc tests and the bit comparisons.  Plain functions; an error bound, a reference or a helper
that one file uses stays in that file."""
import numpy as np
import pytest

import __graft_entry__ as ge
from insider_amd import _lib, api


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X box")


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


# ---- planted data: pure numpy, every array a function of the arguments alone ----------------------------------------------
def levels(rng, n, counts):
    """n x len(counts) level ids (int32, column-major), every level of every covariate present."""
    lev = np.empty((n, len(counts)), dtype=np.int32)
    for i, L in enumerate(counts):
        v = np.concatenate([np.arange(1, L + 1), rng.integers(1, L + 1, size=n - L)])
        lev[:, i] = rng.permutation(v)
    return np.asfortranarray(lev)


def factors(rng, counts, m, K, p):
    A = [np.asfortranarray(rng.standard_normal((L, K))) for L in counts]
    if m:
        A.append(np.asfortranarray(rng.standard_normal((m, K))))
    return A, np.asfortranarray(rng.standard_normal((K, p)))


# what masks() empties: one constant per variant in use, named at the call site
SAMPLES_3_5_7 = "samples 3/5/7"                    # sample 3 has no test entry, sample 5 no train entry, sample 7 is all NA
SAMPLES_3_5_7_GENES_1_3 = "samples 3/5/7, genes 1/3"       # ... and gene 1 has no train entry, gene 3 no test entry
GENES_3_5 = "genes 3/5"                            # gene 3 has no test entry, gene 5 no train entry
GENES_3_5_7 = "genes 3/5/7 where p > 7"            # ... and gene 7 is all NA; nothing is emptied when p <= 7
SPLIT_80_20 = "80/20 split"                        # no NA entry: train = u < 0.8, test = the rest; nothing emptied


def masks(rng, n, p, empty=None):
    """Train and test entries (bool, n x p) from one uniform draw: train u < 0.6, test 0.6 <= u < 0.85, the rest NA, then
    the samples and genes ``empty`` names are cleared."""
    u = rng.random((n, p))
    if empty == SPLIT_80_20:
        return u < 0.8, ~(u < 0.8)
    tr = u < 0.6
    te = (u >= 0.6) & (u < 0.85)
    if empty in (SAMPLES_3_5_7, SAMPLES_3_5_7_GENES_1_3):
        te[3] = False
        tr[5] = False
        tr[7] = te[7] = False
    if empty == SAMPLES_3_5_7_GENES_1_3:
        tr[:, 1] = False
        te[:, 3] = False
    if empty == GENES_3_5 or (empty == GENES_3_5_7 and p > 7):
        te[:, 3] = False
        tr[:, 5] = False
    if empty == GENES_3_5_7 and p > 7:
        tr[:, 7] = te[:, 7] = False
    return tr, te


def planted(n, p, counts, m=0, seed=0, offset=0.3, empty=None):
    """-> (X, lev, Z, {"all": None, "train": tr, "test": te}).  The order of the draws (X, levels, masks, Z) is fixed: the
    tests' data sets are these arrays bit for bit."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    X = np.asfortranarray(X + offset if offset else X)
    lev = levels(rng, n, counts)
    tr, te = masks(rng, n, p, empty)
    Z = np.asfortranarray(rng.standard_normal((n, m))) if m else None
    return X, lev, Z, {"all": None, "train": tr, "test": te}


def resident(X, lev, Z, masks):
    """The resident data set of a planted() result: the one GPU step."""
    tr, te = (np.asfortranarray(masks[k], dtype=np.uint8) for k in ("train", "test"))
    return api.InsiderData(X, lev, tr, te, ctns_confounder=Z)


def problem(seed, n, p, counts, m, K, scale=1.0):
    """A small host-side case: -> X, lev, Z, mask, A, Cm (``scale`` multiplies the row embeddings)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) + 0.5
    lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    Z = rng.standard_normal((n, m)) if m else None
    A = [scale * rng.standard_normal((L, K)) for L in counts] + ([scale * rng.standard_normal((m, K))] if m else [])
    Cm = rng.standard_normal((K, p))
    mask = rng.random((n, p)) < 0.7
    return X, lev, Z, mask, A, Cm


def blocks(lev, Z, A, Cm):
    """The fitted term of every block, n x p each."""
    g = [A[b][lev[:, b] - 1] @ Cm for b in range(lev.shape[1])]
    if Z is not None:
        g.append(Z @ A[lev.shape[1]] @ Cm)
    return g


# ---- results ------------------------------------------------------------------------------------------------------------------
def close_resident(obj):
    """Close the resident handles a fitted object holds."""
    for v in obj.values():
        if isinstance(v, api.InsiderData):
            v.close()


def same_bits(a, b, keys):
    for k in keys:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


def bits(r, names):
    return b"".join(np.asarray(r[n]).tobytes() for n in names)
