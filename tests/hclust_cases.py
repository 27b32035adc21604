"""The inputs and the error bounds that tests/test_hclust_cpu.py and tests/test_gpu_hclust.py share (agglomerative clustering,
insider_hip_hclust).  Pure numpy: every array is a function of the arguments alone.

The bounds.  u = eps / 2 is the unit roundoff, D the number of coordinates, mu = S / n a cluster's mean, h = |mu|^2.

Two implementations of the rule of include/insider_hip.h that start from the same working points and have made the same merges
so far hold the same sums S bit for bit (S_new = S_a + S_b is one rounded addition per coordinate either way, and the working
points themselves are formed by separately rounded operations in a stated order), hence the same mu and the same h.  They differ
only in the product p = mu_A . mu_B, a sum of D rounded products in some order with or without fused steps: each is within
gamma_D |mu_A| |mu_B| <= D u (h_A + h_B) / 2 of the exact sum, so two of them are within D u (h_A + h_B) of each other, and in the
few operations that follow, which the compiler may contract.

  Ward.  d = w ((h_A + h_B) - 2 p), w = n_A n_B / (n_A + n_B) (the product and the sum of the sizes are exact, one division).  The
  difference in p enters doubled: 2 D u (h_A + h_B).  The addition, the subtraction (or one fused step) and the multiplication by
  w round three times, each relative to a value of at most 2 (h_A + h_B) (|2 p| <= h_A + h_B): two implementations differ by at
  most 2 * 3 * 2 u (h_A + h_B) there.  Together |d - d'| <= (2 D + 12) u w (h_A + h_B) = (D + 6) eps * scale, scale = w (h_A + h_B).
  The height is sqrt(2 d); the tests compare in d (height^2 / 2), which adds the roundings of a square root, a square and a
  halving on each side: 4 u d.  WARD_BOUND = (D + 6) eps scale + 2 eps d.

  Cosine, average.  d = 1 - p with h <= 1 (means of unit vectors; the roundings of the normalisation put h above 1 by a few u at
  most, which the constant below absorbs): two products differ by at most D u (1 + 4 u), the subtraction rounds once on each side
  relative to |d| <= 2: 4 u.  COSINE_BOUND = (D + 4) u (1 + ...) <= (D + 6) eps / 2, taken as (D + 6) eps: scale = 1.

Against scipy (the CPU file) the other side is a different algorithm: the condensed distance matrix and the Lance-Williams
update, whose error grows with the number of updates a distance has gone through (at most N - 1), and the yardstick's sums S are
compared with exact sums, not with equal ones: a sum of up to N terms is within N u of exact, relative to the largest partial
sum.  Both add a term of N roundings, so there the constants above get 2 N more: (D + 6 + 2 N) eps (scale + 4 d), the 4 d for
Lance-Williams terms that are up to twice the result on each of its two sides.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
METRICS = ("cosine", "euclidean")
SCIPY_METHOD = {"cosine": "average", "euclidean": "ward"}


def planted(N, D, seed, centres=12, noise=0.3):
    """D x N points around ``centres`` standard-normal centres, noise 0.3 (column-major)."""
    rng = np.random.default_rng(seed)
    Cc = rng.standard_normal((D, centres))
    lab = rng.integers(0, centres, N)
    return np.asfortranarray(Cc[:, lab] + noise * rng.standard_normal((D, N)))


def seed_of(N, D):
    return 100 * N + D


def linkage_d(metric, height):
    """The linkage distance a height was made from (Ward: height = sqrt(2 d))."""
    return height * height / 2 if metric == "euclidean" else height


def pair_bound(metric, D, scale, d):
    """The largest |d - d'| of one merge between two implementations of the header's rule (the module's docstring)."""
    if metric == "euclidean":
        return (D + 6) * EPS * scale + 2 * EPS * d
    return (D + 6) * EPS * np.ones_like(scale)


def gap_bound(D):
    """What the yardstick's min_gap (a gap divided by the scale of its two pairs) must exceed four times over: the scaled part
    of pair_bound(), plus the relative part for d <= scale (Ward: d = w |mu_A - mu_B|^2 <= 2 w (h_A + h_B))."""
    return (D + 6 + 4) * EPS


def scipy_bound(metric, D, N, scale, d):
    if metric == "euclidean":
        return (D + 6 + 2 * N) * EPS * (scale + 4 * d)
    return (D + 6 + 2 * N) * EPS * (1 + 4 * d)


# ---- exact ties: small integers, 16 points so that the grand mean is a dyadic rational and every product is exact ----------------
TIE_WHICH = np.array([0, 2, 3, 1, 4, 0, 5, 2, 7, 0, 4, 6, 1, 8, 3, 5])      # the location of every point: 0 three times, 1..5 twice
TIE_ZERO = [(0, 5), (1, 7), (2, 14), (3, 12), (4, 10), (6, 15), (9, 16)]   # the height-0 rows: ascending a, then ((0, 5), 9)


def ties():
    """D x 16: location i = (2^i, i), i < 9; the triple is points 0, 5, 9, the pairs (1, 7), (2, 14), (3, 12), (4, 10),
    (6, 15).  The distinct locations are far apart (their gaps double), so nothing but the duplicates ties."""
    loc = np.array([[2.0 ** i, float(i)] for i in range(9)])
    return np.asfortranarray(loc[TIE_WHICH].T)


def chain(N=40, ratio=1.2):
    """2 x N collinear points whose gaps grow geometrically: few reciprocal pairs per round, the slow case."""
    return np.asfortranarray(np.outer([1.0, 0.5], np.cumsum(ratio ** np.arange(N))))
