"""Host-side checks of the gene-set enrichment (insider_hip_enrichment): the sampler of include/insider_sample.h (through
insider_hip_enrichment_sample, which opens no device) equals its numpy mirror posthoc.gs_sample_host(), is a bijection and
includes every position equally often; the yardstick posthoc.enrichment_host() equals a brute-force running sum over all p
positions; p, NES, Benjamini-Hochberg, the hypergeometric tail and the leading edge on a case computed by hand;
flatio.read_gmt(); every argument the library refuses is refused on the host with the outputs untouched."""
import ctypes as C
import math

import numpy as np
import pytest

from insider_amd import _lib, api, fit, flatio, posthoc
from tests.support import lib  # noqa: F401  (fixture)

I32 = C.c_int32


# ---- the sampler ------------------------------------------------------------------------------------------------------------
def sample(lib, seed, perm, m, p, expect=_lib.OK):
    out = np.full(m + 3, -5, dtype=np.int32)
    assert lib.insider_hip_enrichment_sample(seed, perm, m, p, _lib.ptr(out, I32)) == expect
    assert np.all(out[m if expect == _lib.OK else 0:] == -5)
    return out[:m]


@pytest.mark.parametrize("p", [2, 3, 5, 64, 65, 1000, 4097])
def test_sampler_equals_the_numpy_mirror_and_is_a_bijection(lib, p):
    for seed in (0, api.DEFAULT_SEED, 0x0123456789ABCDEF, 2 ** 64 - 1):
        for perm in (0, 1, 2, 999, 65535):
            got = sample(lib, seed, perm, p, p)
            assert np.array_equal(got, posthoc.gs_sample_host(seed, perm, p, p)), (seed, perm)
            assert np.array_equal(np.sort(got), np.arange(p))
            m = max(1, p // 3)                                                   # the sizes are nested
            assert np.array_equal(sample(lib, seed, perm, m, p), got[:m])
    if p >= 64:
        assert not np.array_equal(sample(lib, 1, 0, p, p), sample(lib, 1, 1, p, p))


def test_sampler_refuses_bad_arguments(lib):
    for m, p in ((1, 1), (0, 0), (3, 2), (-1, 5), (1, 2 ** 31)):
        out = np.full(8, -5, dtype=np.int32)
        assert lib.insider_hip_enrichment_sample(1, 0, m, p, _lib.ptr(out, I32)) == _lib.ERR_ARG
        assert np.all(out == -5)
    assert lib.insider_hip_enrichment_sample(1, 0, 1, 5, None) == _lib.ERR_ARG


def test_inclusion_frequencies_are_uniform(lib):
    """(p, m, draws) = (1000, 50, 20000): every position is in a draw with probability q = m / p, so its count has mean
    draws q and variance draws q (1 - q); the counts sum to draws m, which leaves p - 1 degrees of freedom."""
    p, m, draws = 1000, 50, 20000
    cnt = np.zeros(p)
    for b in range(draws):
        cnt[sample(lib, api.DEFAULT_SEED, b, m, p)] += 1
    q = m / p
    z = (cnt - draws * q) / math.sqrt(draws * q * (1 - q))
    chi2_df = float((z * z).sum()) * ((p - 1) / p) / (p - 1)
    print("chi2/df", chi2_df, "max |z|", np.abs(z).max())
    assert abs(chi2_df - 1.0) <= 5.0 * math.sqrt(2.0 / p)
    assert np.abs(z).max() < 5.0


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def brute(sc, genes, weight):
    """The running sum over all p positions: + w / N at a gene of the set, - 1 / (p - m) elsewhere.  -> (max, min with the
    empty prefix)."""
    p, m = sc.size, genes.size
    order = sorted(range(p), key=lambda g: (-sc[g], g))
    inset = set(int(g) for g in genes)
    w = [abs(sc[g]) if weight else 1.0 for g in order]
    N = math.fsum(w[t] for t in range(p) if order[t] in inset)
    if N == 0.0:
        w, N = [1.0] * p, float(m)
    run, hi, lo = 0.0, -math.inf, 0.0
    for t in range(p):
        run += w[t] / N if order[t] in inset else -1.0 / (p - m)
        hi, lo = max(hi, run), min(lo, run)
    return hi, lo


def test_host_yardstick_matches_the_running_sum():
    rng = np.random.default_rng(5)
    cases = zero_sets = 0
    for trial in range(60):
        p = int(rng.integers(2, 40))
        sc = rng.standard_normal((2, p)) if trial % 3 else rng.integers(-2, 3, (2, p)).astype(np.float64)
        sc[:, rng.random(p) < 0.5] = 0.0
        sets = [rng.choice(p, int(rng.integers(1, p)), replace=False) for _ in range(4)]
        zero = np.flatnonzero(sc[0] == 0.0)
        if 0 < zero.size < p:
            sets.append(zero[:max(1, zero.size // 2)])                           # all-zero weight in profile 0
        ptr = np.concatenate([[0], np.cumsum([s.size for s in sets])])
        genes = np.concatenate(sets).astype(np.int32)
        for weight in (0, 1):
            rec = posthoc.enrichment_host(sc, ptr, genes, nperm=2, weight=weight)
            for r in range(2):
                for s, g in enumerate(sets):
                    hi, lo = brute(sc[r], g, weight)
                    zero_sets += weight == 1 and not np.any(sc[r, g])
                    cases += 1
                    if abs(hi + lo) > 1e-9:                                      # (at hi = -lo rounding picks the side)
                        assert abs(rec["es"][r, s] - (hi if hi >= -lo else lo)) <= 1e-12
                    else:
                        assert abs(abs(rec["es"][r, s]) - hi) <= 1e-12
                    assert rec["hits_nonzero"][r, s] == np.count_nonzero(sc[r, g])
    assert cases >= 300 and zero_sets >= 20


def test_null_counts_follow_the_definitions():
    """The counts of the record from the null table it was counted on, draw by draw in Python."""
    rng = np.random.default_rng(6)
    p, nperm = 30, 40
    sc = rng.integers(-2, 3, (3, p)).astype(np.float64)
    ptr = np.array([0, 4, 8, 15])
    genes = np.concatenate([rng.choice(p, 4, replace=False), rng.choice(p, 4, replace=False), rng.choice(p, 7, replace=False)])
    rec = posthoc.enrichment_host(sc, ptr, genes, nperm=nperm, weight=1, seed=11, return_null=True)
    assert list(rec["null_sizes"]) == [4, 7] and rec["null"].shape == (3, 2, nperm)
    order = np.argsort(-sc, axis=1, kind="stable")
    for r in range(3):
        aw = np.abs(sc[r, order[r]])[None, :]
        for s, z in ((0, 0), (1, 0), (2, 1)):
            m = int(ptr[s + 1] - ptr[s])
            n_same = n_ge = 0
            total = 0.0
            for b in range(nperm):
                T = np.sort(posthoc.gs_sample_host(11, b, m, p))
                e = float(posthoc.gs_pick(*posthoc.gs_deviations(aw, T, 1), T)[0][0])
                assert e == rec["null"][r, z, b]
                if (e >= 0) == (rec["es"][r, s] >= 0):
                    n_same += 1
                    total += e
                    n_ge += abs(e) >= abs(rec["es"][r, s])
            assert (rec["n_same"][r, s], rec["n_ge"][r, s]) == (n_same, n_ge)
            assert abs(rec["sum_same"][r, s] - total) <= 1e-12


def test_derived_quantities_on_a_hand_computed_case():
    # scores 5 0 3 -1 4 -2: ranks of genes 0..5 are 0 3 2 4 1 5.  Set {4, 3, 0} sits at positions {0, 1, 4}, weights 5, 4, 1:
    # N = 10, p - m = 3; P_i / N - miss_i / 3 = .5, .9, 1 - 2/3; P_{i-1} / N - miss_i / 3 = 0, .5, .9 - 2/3: ES = .9 at position 1.
    sc = np.array([[5.0, 0.0, 3.0, -1.0, 4.0, -2.0]])
    rec = posthoc.enrichment_host(sc, [0, 3, 5], [4, 3, 0, 5, 3], nperm=3, weight=1)
    assert rec["es"][0, 0] == 0.9 and rec["peak"][0, 0] == 1 and rec["hits_nonzero"][0, 0] == 3
    assert list(posthoc.leading_edge(rec, 0, 0)) == [0, 4]
    # set {5, 3}: positions {4, 5}, weights 1, 2, N = 3, p - m = 4: hi = max(1/3 - 1, 1 - 1) = 0, lo = min(-1, 1/3 - 1) = -1
    assert rec["es"][0, 1] == -1.0 and rec["peak"][0, 1] == 4
    assert list(posthoc.leading_edge(rec, 0, 1)) == [3, 5]
    assert list(rec["size"]) == [3, 2] and list(rec["nonzero"]) == [5]
    # weight 0 on the first set: i / 3 - miss / 3 = 1/3, 2/3, 1 - 2/3
    rec0 = posthoc.enrichment_host(sc, [0, 3], [4, 3, 0], nperm=3, weight=0)
    assert rec0["es"][0, 0] == 2.0 / 3.0 - 0.0 / 3.0 and rec0["peak"][0, 0] == 1
    hand = dict(es=np.array([[0.5, -0.4, 0.3, 0.2, 0.1]]), n_ge=np.array([[0, 3, 2, 49, 0]], dtype=np.int32),
                n_same=np.array([[99, 99, 99, 99, 0]], dtype=np.int32), sum_same=np.array([[24.75, -19.8, 9.9, 9.9, 0.0]]),
                hits_nonzero=np.array([[3, 0, 2, 1, 3]], dtype=np.int32), size=np.array([3, 3, 3, 3, 3], dtype=np.int32),
                nonzero=np.array([5]), scores=sc)
    d = posthoc.gs_derived(hand)
    assert np.allclose(d["pval"], [[0.01, 0.04, 0.03, 0.5, 1.0]], rtol=0, atol=1e-15)
    # Benjamini-Hochberg over 5 sets: sorted .01 .03 .04 .5 1 -> x 5 / rank = .05 .075 .0667 .625 1 -> running minimum from the end
    assert np.allclose(d["fdr"], [[0.05, 0.2 / 3, 0.2 / 3, 0.625, 1.0]], rtol=0, atol=1e-15)
    assert np.allclose(d["nes"][0, :4], [2.0, 2.0, 3.0, 2.0], rtol=0, atol=1e-14) and np.isnan(d["nes"][0, 4])
    # 3 draws from 6 genes of which 5 are non-zero: P(X >= 3) = C(5,3) / C(6,3) = .5, P(X >= 2) = 1 = P(X >= 0)
    assert np.allclose(d["hyper_p"], [[0.5, 1.0, 1.0, 1.0, 0.5]], rtol=0, atol=1e-12)


# ---- read_gmt ---------------------------------------------------------------------------------------------------------------
def test_read_gmt(tmp_path):
    path = tmp_path / "sets.gmt"
    path.write_text("A\tfirst\tg3\tg1\tg3\tnope\tg0\n"            # a duplicate and an unknown token: {3, 1, 0}
                    "B\tsmall\tg2\n"                              # below min_size
                    "C\tbig\tg0\tg1\tg2\tg3\tg4\n"                # above max_size
                    "\n"
                    "D\t\tg4\tg2\r\n")                            # empty description, CRLF
    names = [f"g{i}" for i in range(5)]
    got = flatio.read_gmt(str(path), names, min_size=2, max_size=4)
    assert got[0] == ["A", "D"]
    assert got[1].dtype == np.int64 and list(got[1]) == [0, 3, 5]
    assert got[2].dtype == np.int32 and list(got[2]) == [3, 1, 0, 4, 2]
    idx = tmp_path / "idx.gmt"
    idx.write_text("A\tx\t3\t1\t3\t7\tg0\t0\nB\tx\t2\t4\n")       # 7 is kept as an index (the library checks the range)
    got = flatio.read_gmt(str(idx), None, min_size=1, max_size=10)
    assert got[0] == ["A", "B"] and list(got[1]) == [0, 4, 6] and list(got[2]) == [3, 1, 7, 0, 2, 4]
    got = flatio.read_gmt(str(idx))                               # the default window 15..500 drops both
    assert got[0] == [] and list(got[1]) == [0] and got[2].size == 0 and got[2].dtype == np.int32


def test_driver_flags_parse():
    base = ["--x", "X.npy", "--levels", "L.npy", "--rank", "3", "--lambda", "1", "--alpha", "0.1"]
    a = fit.parse(base + ["--gene-sets", "s.gmt", "--gene-names", "n.txt", "--enrich-perms", "50", "--enrich-min-size", "5",
                          "--enrich-max-size", "60", "--enrich-levels", "2"])
    assert (a.gene_sets, a.gene_names, a.enrich_perms, a.enrich_min_size, a.enrich_max_size, a.enrich_levels) == \
        ("s.gmt", "n.txt", 50, 5, 60, 2)
    a = fit.parse(base + ["--gene-sets", "s.gmt"])
    assert (a.enrich_perms, a.enrich_min_size, a.enrich_max_size, a.enrich_levels) == (1000, 15, 500, None)
    for bad in (["--enrich-levels", "1"], ["--gene-names", "n.txt"], ["--gene-sets", "s.gmt", "--enrich-perms", "0"],
                ["--gene-sets", "s.gmt", "--enrich-perms", "65537"], ["--gene-sets", "s.gmt", "--enrich-max-size", "4097"],
                ["--gene-sets", "s.gmt", "--enrich-levels", "0"], ["--gene-sets", "s.gmt", "--enrich-min-size", "0"]):
        with pytest.raises(SystemExit):
            fit.parse(base + bad)


# ---- refused arguments --------------------------------------------------------------------------------------------------
NGUARD = 5
OUTS = (("es", np.float64, 12345.678), ("peak", np.int32, -77), ("n_ge", np.int32, -78), ("n_same", np.int32, -79),
        ("sum_same", np.float64, 8765.4321), ("hits_nonzero", np.int32, -80))


def refused(lib, sc, ptr, genes, R=None, p=None, S=None, weight=1, nperm=10, null=(), expect=_lib.ERR_ARG):
    sc = np.ascontiguousarray(sc, dtype=np.float64)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    genes = np.ascontiguousarray(genes, dtype=np.int32)
    R = sc.shape[0] if R is None else R
    p = sc.shape[1] if p is None else p
    S = ptr.size - 1 if S is None else S
    outs = [np.full(max(R, 0) * max(S, 0) + NGUARD, fill, dtype=dt) for _, dt, fill in OUTS]
    args = [_lib.ptr(sc), R, p, _lib.ptr(ptr, C.c_int64), _lib.ptr(genes, I32), S, weight, nperm, 7, 0] + \
           [_lib.ptr(o, I32 if o.dtype == np.int32 else C.c_double) for o in outs]
    for pos in null:
        args[pos] = None
    status = lib.insider_hip_enrichment(*args)
    assert status == expect, (status, lib.insider_hip_last_error().decode(errors="replace"))
    for o, (_, _, fill) in zip(outs, OUTS):
        assert np.all(o == fill)


def test_bad_arguments_are_refused_on_the_host_and_write_nothing(lib):
    rng = np.random.default_rng(3)
    p = 12
    sc = rng.standard_normal((2, p))
    ptr, genes = [0, 3, 5], [1, 4, 7, 0, 11]
    for pos in (0, 3, 4, 10, 11, 12, 13, 14, 15):
        refused(lib, sc, ptr, genes, null=(pos,))
    refused(lib, sc, ptr, genes, R=-1)
    refused(lib, sc, ptr, genes, S=-1)
    refused(lib, sc[:, :1], [0, 1], [0], p=1)
    refused(lib, sc, ptr, genes, p=0)
    refused(lib, sc, ptr, genes, p=2 ** 31)
    for weight in (-1, 2):
        refused(lib, sc, ptr, genes, weight=weight)
    for nperm in (0, -1, 65537):
        refused(lib, sc, ptr, genes, nperm=nperm)
    refused(lib, sc, [0, 3, 3], [1, 4, 7])                                       # m < 1
    refused(lib, sc, [0, p], np.arange(p))                                       # m >= p
    refused(lib, np.zeros((1, 5000)), [0, 4097], np.arange(4097))                # m > 4096
    refused(lib, sc, ptr, [1, 4, -1, 0, 11])                                     # gene index out of range
    refused(lib, sc, ptr, [1, 4, p, 0, 11])
    refused(lib, sc, ptr, [1, 4, 1, 0, 11])                                      # repeated within a set
    refused(lib, sc, [0, 4, 3], genes)                                           # set_ptr decreases
    refused(lib, sc, [-1, 3, 5], genes)
    for bad in (np.nan, np.inf, -np.inf):
        sb = sc.copy()
        sb[1, 5] = bad
        refused(lib, sb, ptr, genes)
    # the same gene in two sets is fine, and no profiles or no sets is OK with nothing written (no device is opened)
    refused(lib, sc, [0, 2, 4], [1, 4, 4, 1], R=0, expect=_lib.OK)
    refused(lib, sc, [0], [0], expect=_lib.OK)
    # the shape checks of the Python layer
    for call in (api.enrichment, posthoc.enrichment_host):
        with pytest.raises(_lib.InsiderError) as e:
            call(sc, [0, 3, 9], genes)
        assert e.value.status == _lib.ERR_ARG
        with pytest.raises(_lib.InsiderError):
            call(sc, ptr, genes, nperm=2.5)
        with pytest.raises(_lib.InsiderError):
            call(sc, ptr, genes, seed=-1)
