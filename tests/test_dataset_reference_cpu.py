"""tests/dataset_reference.py checked against itself and against hand-worked cases (no GPU): the packed tables' encode / decode
round trips on random logical arrays, every sum against a plain triple loop on a 7 x 5 case, and the geometry rules against
cases worked out by hand below."""
import numpy as np
import pytest

from tests import dataset_reference as dr


# ---- geometry: hand-worked cases ------------------------------------------------------------------------------------------------
def test_geometry_three_covariates_largest_in_the_middle():
    """Level counts (3, 10, 4): by descending count the order is covariate 1, 2, 0; stacked offsets are 0, 3, 13.
    Position 0 (covariate 1, offset 3, 10 levels) is never a later covariate: its levels [3, 13) are not table rows, so the
    table has 17 - 10 = 7 rows -> 2 steps of four -> 4 bytes per lane.  The planes of slev hold the OTHER covariates in
    covariate order: covariate 1 keeps (0, 2), so its later covariates 2 and 0 are planes 1 and 0; covariate 2 keeps (0, 1), its
    later covariate 0 is plane 0.  Each position with later covariates has one block of 16 levels = 64 lanes x 4 bytes = 256."""
    g, ok = dr.geometry([3, 10, 4], 0, p=5, n=7)
    assert ok and g.cnt_built and not g.zc
    assert (g.c, g.nsteps, g.tab_skip_lo, g.tab_skip_n, g.tab_rows) == (3, 2, 3, 10, 7)
    assert g.L[:3] == [10, 4, 3] and g.off[:3] == [3, 13, 0] and g.nlater[:3] == [2, 1, 0] and g.pos_cov[:3] == [1, 2, 0]
    assert g.later_plane[0][:2] == [1, 0] and g.later_plane[1][:1] == [0]
    assert g.cnt_off[:3] == [0, 256, 512] and g.cnt_stride == 512
    assert g.hn_off[:3] == [0, 16, 32] and g.hn_stride == 48 and g.sq_stride == 3 * 36
    assert g.zt_stride == 0
    assert [dr.table_row(g, s) for s in (0, 2, 13, 16)] == [0, 2, 3, 6]


def test_geometry_equal_counts_keep_covariate_order_and_continuous_position():
    """Level counts (5, 5) with one continuous column: the tie keeps covariate order.  5 table rows -> 2 steps.  Only position
    0 has a later covariate: 256 count bytes.  1/2 n: 16 floats per position, then 16 zeros for position 2 (the continuous
    column) -> 48.  Real-valued counts: 64 doubles per block of 16 levels and position, then 64 for position 2 -> 192."""
    g, ok = dr.geometry([5, 5], 1, p=9, n=12)
    assert ok and g.zc
    assert g.pos_cov[:2] == [0, 1] and g.L[:3] == [5, 5, 1] and g.off[:3] == [0, 5, 10] and g.nlater[:3] == [1, 0, 0]
    assert (g.tab_skip_lo, g.tab_skip_n, g.tab_rows, g.nsteps) == (0, 5, 5, 2)
    assert g.later_plane[0][0] == 0
    assert g.cnt_off[:3] == [0, 256, 0] and g.cnt_stride == 256
    assert g.hn_off[:3] == [0, 16, 32] and g.hn_stride == 48 and g.sq_stride == 72
    assert g.zt_off[:3] == [0, 64, 128] and g.zt_stride == 192
    a = g.as_array()
    assert len(a) == dr.GEOMETRY_INTS == 136 and list(a[:10]) == [2, 2, 0, 5, 5, 256, 48, 192, 72, 1]
    back = dr.Geometry.from_array(a)
    assert np.array_equal(back.as_array(), a) and back.zc


def test_geometry_steps_and_limits():
    """17 table rows -> 5 steps -> 8 bytes per lane: (20, 17) has two blocks of 16 levels at position 0 = 2 x 64 x 8 = 1024
    bytes; 1/2 n: 32 + 32 floats.  33 table rows -> 9 steps, beyond CP_MAXSTEPS = 8: no pair counts, no half counts, the strides
    of the count table still say what it would have taken (3 blocks x 64 x 8).  16 / 32 rows are the last with 4 / 8 steps.  One
    covariate: no later covariate, no count bytes, the half counts stand alone.  A cell above 255 drops the form."""
    g, ok = dr.geometry([20, 17], 0, p=4, n=40)
    assert ok and (g.tab_rows, g.nsteps, g.bpl, g.cnt_stride) == (17, 5, 8, 1024)
    assert g.hn_off[:2] == [0, 32] and g.hn_stride == 64 and g.sq_stride == 4 * 36
    g, ok = dr.geometry([40, 33], 0, p=4, n=80)
    assert not ok and not g.cnt_built and (g.nsteps, g.cnt_stride, g.hn_stride, g.sq_stride) == (9, 1536, 0, 0)
    assert [dr.geometry([40, r], 0, 4, 80)[0].nsteps for r in (16, 17, 32, 33)] == [4, 5, 8, 9]
    g, ok = dr.geometry([6], 0, p=4, n=9)
    assert ok and not g.cnt_built and (g.tab_rows, g.nsteps, g.cnt_stride, g.hn_stride, g.sq_stride) == (0, 0, 0, 16, 36)
    g, ok = dr.geometry([3, 2], 0, p=4, n=300, overflow=True)
    assert not ok and g.cnt_built and g.hn_stride == 0
    # 64 KiB of count bytes per gene: 1100 levels are 69 blocks of 16, at 8 bytes per lane 69 x 512 = 35328 bytes (fits);
    # 2100 levels are 132 blocks = 67584 bytes (does not)
    g, ok = dr.geometry([1100, 30], 0, p=4, n=2000)
    assert g.cnt_stride == 69 * 512 and ok
    g, ok = dr.geometry([2100, 30], 0, p=4, n=4000)
    assert g.cnt_stride == 132 * 512 > 65536 and not ok and not g.cnt_built


def test_merged_shape_and_gu_fits_edges():
    """4 (SLcat + 512) 8 <= 65536 <=> SLcat <= 1536; at most four continuous columns.  k_gene_u_cnt's record: 4 (SL + L rounded
    up to 2 + 512) 8 <= 65536 <=> SL + L' <= 1536."""
    assert dr.merged_shape([1536], 0) and not dr.merged_shape([1537], 0)
    assert dr.merged_shape([1000, 536], 4) and not dr.merged_shape([5, 4], 5)
    assert dr.gu_fits([767], 1) and not dr.gu_fits([768], 1)           # 768 + 768 = 1536 | 769 + 768 > 1536
    assert dr.gu_fits([700, 135], 1) and not dr.gu_fits([700, 136], 1)     # 836 + 700 | 837 + 700


# ---- encode / decode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels,m", [((3, 10, 4), 0), ((20, 17), 0), ((5, 5), 1), ((33, 17, 2), 3), ((6,), 0), ((6,), 2)])
def test_packed_tables_round_trip(n_levels, m):
    rng = np.random.default_rng(3)
    p = 5
    g, ok = dr.geometry(list(n_levels), m, p, 50)
    assert ok
    c = g.c
    if g.cnt_built:
        logical = [None if g.nlater[t] == 0 else rng.integers(0, 256, (p, g.L[t], 4 * g.nsteps)) for t in range(c)]
        table = dr.encode_cnt(logical, g, p)
        back, addressed = dr.decode_cnt(table, g, p)
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(logical, back))
        assert not table[:, ~addressed].any()
        # every addressed byte belongs to exactly one cell
        assert addressed.sum() == sum(g.L[t] * 4 * g.nsteps for t in range(c) if g.nlater[t])
    hn = [rng.integers(1, 9, (p, g.L[t])).astype(np.float32) / 2 for t in range(c + (1 if g.zc else 0))]
    table = dr.encode_hn(hn, g, p)
    back, addressed = dr.decode_hn(table, g, p)
    assert all(np.array_equal(a, b) for a, b in zip(hn, back)) and not table[~addressed].any()
    assert addressed.sum() == p * sum(g.L[:len(hn)])
    if m == 0:
        sq = [rng.standard_normal((p, g.L[t], 2)) for t in range(c)]
        table = dr.encode_sq(sq, g, p)
        back, addressed = dr.decode_sq(table, g, p)
        assert all(np.array_equal(a, b) for a, b in zip(sq, back)) and not table[:, ~addressed].any()
        assert addressed.sum() == 2 * sum(g.L[:c])
    else:
        zt = [rng.standard_normal((p, g.L[t], m)) for t in range(c)] + [rng.standard_normal((p, m, m))]
        table = dr.encode_zt(zt, g, p)
        back, addressed = dr.decode_zt(table, g, p)
        assert all(np.array_equal(a, b) for a, b in zip(zt, back)) and not table[:, ~addressed].any()
        assert addressed.sum() == m * sum(g.L[:c]) + m * m


def test_exact_products_and_sums():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(200) * 1e3, rng.standard_normal(200)
    from fractions import Fraction
    exact = sum(Fraction(x) * Fraction(y) for x, y in zip(a, b))
    v, s, N = dr.dot_ref(a, b)
    assert v == float(exact) and N == 200 and abs(s - np.abs(a * b).sum()) < 1e-9 * s
    assert dr.sum_ref([1e16, 1.0, -1e16]) == (1.0, 2e16 + 1.0, 3)
    assert dr.dot_ref([], []) == (0.0, 0.0, 0)


# ---- every sum against a triple loop: 7 samples x 5 genes -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    n, p = 7, 5
    X = np.arange(1, n * p + 1, dtype=np.float64).reshape(n, p) % 11 - 4          # small integers: every sum is exact
    lev = np.array([[1, 2], [3, 1], [1, 1], [2, 2], [3, 2], [1, 1], [4, 2]], dtype=np.int32)   # level 4 of 5 declared: one member; level 5: none
    Z = np.array([[1, -2], [0, 1], [2, 2], [-1, 0], [1, 1], [-2, 1], [0, -1]], dtype=np.float64)
    tr = np.ones((n, p), dtype=bool)
    te = np.zeros((n, p), dtype=bool)
    for i, j in [(0, 0), (2, 0), (5, 0), (1, 1), (6, 3), (3, 3)]:
        tr[i, j], te[i, j] = False, True
    tr[4, 0] = False                                                             # NA
    tr[:, 4] = False                                                             # gene 4 wholly held out: test
    te[:, 4] = True
    return X, lev, [5, 2], Z, tr, te, dr.build(X, lev, [5, 2], Z, tr, te)


def test_tiny_sums_against_loops(tiny):
    X, lev, n_levels, Z, tr, te, R = tiny
    n, p = X.shape
    SLP = 10                                            # 5 + 2 levels + 2 columns = 9 -> 10
    assert R.info["ds_SLP"] == SLP and R.info["ds_ldn"] == 128 and R.info["ds_ldp"] == 128
    S = np.zeros((p, SLP)); St = np.zeros((p, SLP)); Sh = np.zeros((p, SLP)); ya = np.zeros(p); yt = np.zeros(p)
    off = [0, 5]
    for j in range(p):
        for i in range(n):
            for b in range(2):
                col = off[b] + lev[i, b] - 1
                S[j, col] += X[i, j]
                St[j, col] += X[i, j] * tr[i, j]
                Sh[j, col] += X[i, j] * (not tr[i, j])
            for k in range(2):
                S[j, 7 + k] += X[i, j] * Z[i, k]
                St[j, 7 + k] += X[i, j] * Z[i, k] * tr[i, j]
                Sh[j, 7 + k] += X[i, j] * Z[i, k] * (not tr[i, j])
            ya[j] += X[i, j] ** 2
            yt[j] += X[i, j] ** 2 * tr[i, j]
    A = R.arrays
    assert np.array_equal(A["S"].value.reshape(p, SLP), S) and np.array_equal(A["Strain"].value.reshape(p, SLP), St)
    assert np.array_equal(A["Sheld"].value.reshape(p, SLP), Sh)
    assert np.array_equal(A["yy_all"].value, ya) and np.array_equal(A["yy_train"].value, yt)
    assert R.info["ds_cnt_train"] == tr.sum() and R.info["ds_cnt_test"] == te.sum() and R.info["ds_no_na"] == 0
    assert R.info["ds_merged"] == 1 and R.info["ds_cf_pair_ok"] == 1 and R.info["ds_cont_merged"] == 1
    # term counts: level 1 of covariate 0 has samples 0, 2, 5
    assert A["S"].nterms.reshape(p, SLP)[0, 0] == 3 and A["S"].nterms.reshape(p, SLP)[0, 4] == 0
    # the real-valued counts and the pair "counts"
    g = R.geometry
    zt, addressed = dr.decode_zt(A["cf_zt"].value, g, p)
    for j in range(p):
        for t in range(2):
            for l in range(g.L[t]):
                for k in range(2):
                    want = sum(Z[i, k] for i in range(n) if not tr[i, j] and lev[i, g.pos_cov[t]] - 1 == l)
                    assert zt[t][j, l, k] == want
        for k in range(2):
            for k2 in range(2):
                assert zt[2][j, k, k2] == 0.5 * sum(Z[i, k] * Z[i, k2] for i in range(n) if not tr[i, j])
            assert A[f"contm.wl_w:{k}"].value[j] == sum(Z[i, k] ** 2 for i in range(n) if not tr[i, j])
    assert not A["cf_zt"].value.reshape(p, -1)[:, ~addressed].any()
    for i in range(2):
        pc = A[f"paircnt:{i}"].value
        want = np.zeros_like(pc)
        for r in range(n):
            want[lev[r, i] - 1, off[1 - i] + lev[r, 1 - i] - 1] += 1
            want[lev[r, i] - 1, 7:9] += Z[r]
        assert np.array_equal(pc, want)
    for k in range(2):
        want = np.zeros(9)
        for r in range(n):
            for b in range(2):
                want[off[b] + lev[r, b] - 1] += Z[r, k]
        want[7 + (1 - k)] = (Z[:, 0] * Z[:, 1]).sum()
        assert np.array_equal(A[f"cont_pair:{k}"].value, want)
        assert A["cont_cnt"].value[k] == (Z[:, k] ** 2).sum()


def test_tiny_lists_and_groups(tiny):
    X, lev, n_levels, Z, tr, te, R = tiny
    n, p = X.shape
    A = R.arrays
    # gene 0 holds out samples 0, 2, 4 (NA), 5; gene 1: 1; gene 2: none; gene 3: 3, 6; gene 4: all seven
    assert list(A["col_ptr"].value) == [0, 32, 64, 64, 96, 128]
    idx, val, flag = A["col_idx"].value, A["col_val"].value, A["col_flag"].value
    assert list(idx[:5]) == [0, 2, 4, 5, dr.LIST_PAD] and list(flag[:5]) == [1, 1, 0, 1, 0]
    assert list(val[:5]) == [X[0, 0], X[2, 0], X[4, 0], X[5, 0], 0.0]
    assert list(idx[96:104]) == [0, 1, 2, 3, 4, 5, 6, dr.LIST_PAD]
    assert A["col_idx"].defined.sum() == 128 and len(idx) == 128 + 64
    # sample 0 is held out in genes 0 and 4
    assert list(A["row_idx"].value[:3]) == [0, 4, dr.LIST_PAD] and list(A["row_ptr"].value[:3]) == [0, 32, 64]
    # groups of covariate 0 (levels of samples 0..6: 1 3 1 2 3 1 4): gene 0's held-out samples by level: (0, 2, 5), (), (4), (), ()
    grp = A["grp:0"].value.reshape(p, 6)
    assert list(grp[0]) == [0, 3, 3, 4, 4, 4] and list(grp[4]) == [96, 99, 100, 102, 103, 103]
    # the stacked level of the other covariate (offset 5) along gene 4's grouped samples 0, 2, 5 | 3 | 1, 4 | 6
    assert list(A["slev:0"].value[96:103]) == [6, 5, 5, 6, 5, 6, 6]
    # (gene, count) lists of covariate 0: level 1 -> genes 0 (3 samples), 4 (3); level 2 -> gene 3 (1), gene 4 (1); ...
    assert list(A["wl_idx:0"].value[:3]) == [0, 4, dr.LIST_PAD] and list(A["wl_w:0"].value[:3]) == [3.0, 3.0, 0.0]
    assert list(A["lvl_item_ptr:0"].value) == [0, 1, 2, 3, 4, 4]             # level 5 has no gene: no item
    assert R.info["ds_nitems:0"] == 4 and R.info["ds_npairs:0"] == 2 + 2 + 3 + 2
    # pair counts of gene 4 (all held out), position 0 = covariate 0 (5 levels), table rows = the two levels of covariate 1
    cnt, _ = dr.decode_cnt(A["cf_cnt"].value, R.geometry, p)
    assert cnt[0][4, 0, :2].tolist() == [2, 1] and cnt[0][4, 2, :2].tolist() == [1, 1] and cnt[1] is None
    hn, _ = dr.decode_hn(A["cf_hn"].value, R.geometry, p)
    assert hn[0][4].tolist() == [1.5, 0.5, 1.0, 0.5, 0.0] and hn[1][0].tolist() == [1.0, 1.0] and not hn[2].any()
    # chunk tables of covariate 0: level 1 has members 0, 2, 5 -> one chunk [0, 3)
    assert list(A["chunk_level:0"].value) == [0, 1, 2, 3] and list(A["lvl_chunk_ptr:0"].value) == [0, 1, 2, 3, 4, 4]
    assert list(A["members_all"].value[:7]) == [0, 2, 5, 3, 1, 4, 6]
    assert list(A["lvl_ptr_all"].value) == [0, 3, 4, 6, 7, 7, 0, 3, 7]


def test_fold_masks():
    ids = np.array([[0, 1, 2], [2, 2, 1]])
    tr, te = dr.fold_masks(ids, 2)
    assert tr.tolist() == [[False, True, False], [False, False, True]] and te.tolist() == [[False, False, True], [True, True, False]]
