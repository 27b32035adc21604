"""The resident data set, array by array: everything insider_hip_create_ex, insider_hip_remask and insider_hip_remask_fold
leave on the device is read back (insider_hip_get_array "ds:<name>", insider_hip_get_info "ds_*") and compared with the host
construction of tests/dataset_reference.py, which builds every table from its documented meaning.

Rules of comparison:
  exact     integers, copies and packed counts: equal bit for bit wherever the layout defines a value (pads included; the
            reference marks the few cells that are allocated and never defined);
  bounded   floating sums: |got - ref| <= N 2^-53 sum|term| (a sum of N terms in any order); with small-integer X and Z every
            sum is exact and the comparison is bitwise — each case runs both ways;
  identity  on the device's own arrays: Sheld = S - Strain bit for bit in the categorical columns (with the continuous columns
            on the merged form, Strain = S - Sheld in theirs), cf_sq = the device's S and Sheld at the decoded positions;
  decisions ds_merged, ds_cf_pair_ok, ds_cont_merged, whether cf_cnt / cf_sq / col_flag exist and the whole geometry are
            what the plain re-statement of the rules gives, and what every case below states for itself.
Run with -s to see the largest error / bound ratio of every bounded array."""
import ctypes

import numpy as np
import pytest

from insider_amd import _lib, api
from insider_amd._lib import InsiderError
from tests import dataset_reference as dr
from tests.support import need_gpu  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

# ---- array -> element type, rule, and the cases that build it ------------------------------------------------------------------
# `when` names the property of a case (CASES below) under which the data set builds the array; cases_building(name) lists the
# cases.  "never": a member that exists in the structure and that no data set builds.
EVERY, CONT, NA, MERGED, CNT, PAIR, PAIR_CAT, CONTM, CONTP, FOLDS, NEVER = (
    "every", "m > 0", "NA entries", "merged", "count table", "pair-count form", "pair-count form, m = 0",
    "continuous columns merged", "continuous pair counts", "fold ids set", "never")
_COV = {"chunk_level": ("i4", "exact", EVERY), "chunk_begin": ("i4", "exact", EVERY), "chunk_end": ("i4", "exact", EVERY),
        "lvl_chunk_ptr": ("i4", "exact", EVERY), "grp": ("u4", "exact", MERGED), "slev": ("u2", "exact", MERGED),
        "item_begin": ("u4", "exact", MERGED), "item_end": ("u4", "exact", MERGED), "lvl_item_ptr": ("i4", "exact", MERGED),
        "wl_idx": ("i4", "exact", MERGED), "wl_w": ("f8", "exact", MERGED), "paircnt": ("f8", "bounded", MERGED)}
ARRAYS = {
    "X": ("f8", "exact", EVERY), "codes": ("u1", "exact", EVERY), "lev": ("i4", "exact", EVERY),
    "lvl_off_d": ("i4", "exact", EVERY), "members_all": ("i4", "exact", EVERY), "lvl_ptr_all": ("i4", "exact", EVERY),
    "lvl_count_all": ("i4", "exact", EVERY), "Zc": ("f8", "exact", CONT), "one_count": ("i4", "exact", CONT),
    "ident_members": ("i4", "exact", CONT), "S": ("f8", "bounded", EVERY), "yy_train": ("f8", "bounded", EVERY),
    "yy_all": ("f8", "bounded", EVERY), "Strain": ("f8", "bounded", EVERY), "Sheld": ("f8", "bounded", MERGED),
    "col_ptr": ("u4", "exact", EVERY), "row_ptr": ("u4", "exact", EVERY), "col_idx": ("i4", "exact", EVERY),
    "row_idx": ("i4", "exact", EVERY), "col_val": ("f8", "exact", EVERY), "row_val": ("f8", "exact", EVERY),
    "col_flag": ("u1", "exact", NA), "cf_cnt": ("u1", "exact", CNT), "cf_hn": ("f4", "exact", PAIR),
    "cf_sq": ("f8", "identity", PAIR_CAT), "cf_zt": ("f8", "bounded", CONTM), "cont_cnt": ("f8", "bounded", CONTP),
    "cont_pair:#": ("f8", "bounded", CONTP), "fold_id": ("u1", "exact", FOLDS),
}
ARRAYS.update({f"{k}:#": v for k, v in _COV.items()})
ARRAYS.update({f"cont.{k}": (v[0], v[1], CONT if k in ("chunk_begin", "chunk_end", "lvl_chunk_ptr") else NEVER)
               for k, v in _COV.items()})
ARRAYS.update({f"contm.{k}:#": (v[0], "bounded" if k == "wl_w" else v[1], CONTM if k in ("wl_w", "paircnt") else NEVER)
               for k, v in _COV.items()})
ARRAYS.update({f"contm_lists.{k}": (v[0], v[1], CONTM if k in ("wl_idx", "item_begin", "item_end", "lvl_item_ptr") else NEVER)
               for k, v in _COV.items()})
# held jointly by a re-masked data set and its source (DataSet, "MASK-INDEPENDENT part")
SHARED = ("X", "lev", "lvl_off_d", "members_all", "lvl_ptr_all", "lvl_count_all", "Zc", "one_count", "ident_members", "S",
          "yy_all", "cont_cnt", "cont_pair:#", "chunk_level:#", "chunk_begin:#", "chunk_end:#", "lvl_chunk_ptr:#", "paircnt:#",
          "cont.chunk_begin", "cont.chunk_end", "cont.lvl_chunk_ptr", "fold_id")


# ---- masks -------------------------------------------------------------------------------------------------------------------
def m_random(held=0.3, na=True):
    def f(rng, n, p):
        u = rng.random((n, p))
        tr = u >= held
        te = ~tr & ((u < held / 2) if na else True)
        return tr, te
    return f


def m_line_counts(counts, genes=True, na=False):
    """Line i (gene, or sample) holds out exactly counts[i % len] entries (-1: the whole line), drawn at random."""
    def f(rng, n, p):
        lines, length = (p, n) if genes else (n, p)
        h = np.zeros((lines, length), dtype=bool)
        for i in range(lines):
            k = counts[i % len(counts)]
            k = length if k < 0 else min(k, length)
            h[i, rng.permutation(length)[:k]] = True
        h = h.T if genes else h
        te = h & (rng.random((n, p)) < 0.5) if na else h
        return ~h, te
    return f


def m_all_train(rng, n, p):
    return np.ones((n, p), dtype=bool), np.zeros((n, p), dtype=bool)


def m_unmasked(rng, n, p):
    return np.ones((n, p), dtype=bool), np.ones((n, p), dtype=bool)


def m_overlap_na(rng, n, p):
    """NA entries, and as many entries that are train and test at once: cnt_train + cnt_test = n p although entries are NA."""
    tr, te = m_random(0.3, na=True)(rng, n, p)
    k = int((~tr & ~te).sum())
    te.ravel()[np.flatnonzero(tr.ravel())[:k]] = True
    assert k > 0 and tr.sum() + te.sum() == n * p
    return tr, te


def m_gene0_whole(rng, n, p):
    tr, te = m_random(0.2, na=False)(rng, n, p)
    tr[:, 0], te[:, 0] = False, True
    return tr, te


def m_sample0_everywhere(rng, n, p):
    tr = np.ones((n, p), dtype=bool)
    tr[0] = False
    return tr, ~tr


# ---- levels ------------------------------------------------------------------------------------------------------------------
def lv_sizes(sizes):
    """Covariate 0 has exactly these level sizes (shuffled over the samples); the others are drawn."""
    def f(rng, n, counts):
        assert sum(sizes) == n and len(sizes) == counts[0]
        lev = np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
        lev[:, 0] = rng.permutation(np.repeat(np.arange(1, len(sizes) + 1), sizes))
        return lev
    return f


def lv_cell(k):
    """Two covariates of two levels; exactly k samples are in (level 1, level 1), the rest spread over the other cells."""
    def f(rng, n, counts):
        lev = np.empty((n, 2), dtype=np.int32)
        lev[:k] = (1, 1)
        lev[k:] = np.array([(1, 2), (2, 1), (2, 2)])[np.arange(n - k) % 3]
        return lev[rng.permutation(n)]
    return f


def lv_sample0_alone(rng, n, counts):
    lev = np.full((n, 2), 2, dtype=np.int32)
    lev[0] = (1, 1)
    return lev


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# id -> n, p, level counts, m, mask, levels (None: drawn, levels may stay without members), and what the data set must decide:
# merged (the merged row update's tables), cnt (the dense pair counts are built), pair (the pair-count form stands), contm
# (the continuous columns are on the merged form).  Stated by hand for every case: a data set that drops a form fails here.
def case(n, p, counts, m=0, mask=None, lv=None, merged=True, cnt=True, pair=True, contm=None):
    return dict(n=n, p=p, counts=tuple(counts), m=m, mask=mask or m_random(), lv=lv, merged=merged, cnt=cnt, pair=pair,
                contm=(m > 0 and pair) if contm is None else contm)


HELD = (0, 65, 1, 31, 32, 33, 63, 64, -1)        # a line without a held-out entry next to one with 65; -1: the whole line
CASES = {
    # line edges: the wave, the CHUNK pitch, four lines per block, the 32 x 32 tiles of the transpose
    "n1-p5": case(1, 5, (3, 2)), "n5-p1": case(5, 1, (3, 2), m=1), "n63-p3": case(63, 3, (3, 2)),
    "n64-p4": case(64, 4, (3, 2), m=1), "n65-p31": case(65, 31, (3, 2)), "n127-p32": case(127, 32, (3, 2)),
    "n128-p33": case(128, 33, (3, 2), m=1), "n129-p65": case(129, 65, (3, 2)), "n257-p130": case(257, 130, (3, 2)),
    "n19-p3": case(19, 3, (3, 2)), "n20-p4": case(20, 4, (3, 2)),
    # held-out entries per line, both sides; with and without NA; no held-out entry at all
    "held-genes": case(70, 18, (4, 3), mask=m_line_counts(HELD, genes=True)),
    "held-genes-na": case(70, 18, (4, 3), mask=m_line_counts(HELD, genes=True, na=True)),
    "held-samples": case(18, 70, (4, 3), mask=m_line_counts(HELD, genes=False)),
    "held-samples-na": case(18, 70, (4, 3), m=1, mask=m_line_counts(HELD, genes=False, na=True)),
    "all-train": case(40, 9, (4, 3), mask=m_all_train), "unmasked": case(40, 9, (4, 3), m=1, mask=m_unmasked),
    "overlap-na": case(40, 9, (4, 3), mask=m_overlap_na),      # entries that are train and test must not hide the NA entries
    # levels: one level; levels without members first, in the middle and last, sizes around LEVEL_CHUNK
    "L1": case(30, 6, (1,), cnt=False), "L1-L3": case(30, 6, (1, 3)),
    "level-sizes": case(27, 7, (8, 3), lv=lv_sizes((0, 1, 4, 0, 5, 8, 9, 0))),
    # k_group_count's run per lane (lanes past the end); largest covariate last / in the middle / first
    "L15-16-17": case(60, 6, (15, 16, 17)),
    "L64-65-63": case(90, 6, (64, 65, 63), cnt=False, pair=False),               # 127 table rows: beyond CP_MAXSTEPS
    "L130": case(150, 9, (130, 2)),
    # the builder's LDS pass: 256 levels at 4 bytes per lane, 128 at 8
    "L256": case(300, 4, (256, 3)), "L257": case(300, 4, (257, 3)),
    "L128-17": case(300, 4, (128, 17)), "L129-17": case(300, 4, (129, 17)),
    # covariate structure
    "c1": case(40, 7, (6,), cnt=False), "c3-middle": case(50, 9, (3, 10, 4)), "c5-ties": case(60, 7, (4, 4, 3, 5, 2)),
    "c8": case(80, 6, (3, 2, 4, 2, 3, 2, 2, 5)), "c9": case(80, 6, (2,) * 9, cnt=False, pair=False),
    "rows16": case(60, 5, (20, 16)), "rows17": case(60, 5, (20, 17)),
    "rows32": case(90, 5, (40, 16, 16)), "rows33": case(90, 5, (40, 17, 16), cnt=False, pair=False),
    # one cell of a wholly held-out gene with 255 / 256 samples
    "cell255": case(300, 3, (2, 2), mask=m_gene0_whole, lv=lv_cell(255)),
    "cell256": case(300, 3, (2, 2), mask=m_gene0_whole, lv=lv_cell(256), pair=False),
    "cell256-m1": case(300, 3, (2, 2), m=1, mask=m_gene0_whole, lv=lv_cell(256), pair=False),
    # continuous columns
    "m1": case(50, 9, (5, 4), m=1), "m3": case(50, 9, (5, 4), m=3), "m4": case(50, 9, (17, 4), m=4),
    "m5": case(50, 9, (5, 4), m=5, merged=False, cnt=False, pair=False),
    "m1-c9": case(80, 6, (2,) * 9, m=1, cnt=False, pair=False),
    # 4 (SLcat + 512) 8 = 65536 at SLcat = 1536
    "slcat1536": case(40, 3, (1530, 6)), "slcat1537": case(40, 3, (1531, 6), merged=False, cnt=False, pair=False),
    # a level list longer than SEG = 1024 entries: two work items, the second padded to LIST_ALIGN
    "work-items": case(8, 1100, (2, 2), mask=m_sample0_everywhere, lv=lv_sample0_alone),
}


def has(cs, when):
    return {EVERY: True, CONT: cs["m"] > 0, NA: None, MERGED: cs["merged"], CNT: cs["cnt"], PAIR: cs["pair"],
            PAIR_CAT: cs["pair"] and cs["m"] == 0, CONTM: cs["contm"],
            CONTP: cs["merged"] and cs["m"] > 0 and len(cs["counts"]) <= dr.CF_MAXC, FOLDS: False, NEVER: False}[when]


def cases_building(name):
    return [k for k, cs in CASES.items() if has(cs, ARRAYS[name][2])]


# ---- data, handles, reference ----------------------------------------------------------------------------------------------------
def data(cid, ints):
    cs = CASES[cid]
    rng = np.random.default_rng(sum(map(ord, cid)))
    n, p, counts, m = cs["n"], cs["p"], cs["counts"], cs["m"]
    X = rng.integers(-8, 9, (n, p)).astype(np.float64) if ints else rng.standard_normal((n, p)) + 0.3
    lev = cs["lv"](rng, n, counts) if cs["lv"] else np.column_stack([rng.integers(1, L + 1, n) for L in counts]).astype(np.int32)
    Z = None
    if m:
        Z = rng.integers(-2, 3, (n, m)).astype(np.float64) if ints else rng.standard_normal((n, m))
    tr, te = cs["mask"](rng, n, p)
    return np.asfortranarray(X), np.asfortranarray(lev), Z, tr, te


def create(X, lev, counts, Z, tr, te):
    return api.InsiderData(X, lev, np.asfortranarray(tr, dtype=np.uint8), np.asfortranarray(te, dtype=np.uint8),
                           n_levels=np.array(counts, dtype=np.int32), ctns_confounder=Z)


def expand(h, name):
    """The indexed names of a table entry on handle h."""
    if not name.endswith(":#"):
        return [name]
    count = h.m if name.startswith(("contm.", "cont_pair")) else h.c
    return [f"{name[:-1]}{i}" for i in range(count)]


def read_prefix(h, name, nbytes, room=None):
    """insider_hip_get_array itself: the first nbytes of "ds:<name>" into a buffer of `room` bytes -> (status, buffer)."""
    buf = np.zeros(room or nbytes, dtype=np.uint8)
    rc = _lib.load().insider_hip_get_array(h._h, ("ds:" + name).encode(), buf.ctypes.data_as(ctypes.c_void_p), nbytes)
    _lib.check(rc) if room is None else None
    return rc, buf


def raw(a):
    return np.ascontiguousarray(a).view(f"u{a.dtype.itemsize}")


RATIOS = {}         # bounded array -> largest error / bound seen (float data)


def check_against_reference(h, R, cid, ints):
    """Every array and fact of handle h against the reference R."""
    cs = CASES[cid]
    p = h.p
    for key, want in R.info.items():
        if key.startswith(("ds_", "col_entries", "row_entries")):       # (the rest: facts about the inputs)
            assert h.info(key) == want, (cid, key, h.info(key), want)
    assert (h.info("ds_merged"), h.info("ds_cf_pair_ok"), h.info("ds_cont_merged")) == (cs["merged"], cs["pair"], cs["contm"]), cid
    geo = h.array("cf_geometry", np.int32)
    assert np.array_equal(geo, R.geometry.as_array()), (cid, geo, R.geometry.as_array())
    g = dr.Geometry.from_array(geo)
    dev = {}
    for entry, (dtype, rule, when) in ARRAYS.items():
        if when == FOLDS:
            continue          # test_provenance
        for name in expand(h, entry):
            got = h.array(name, dtype)
            ref = R.arrays.get(name)
            built = has(cs, when)
            if when == NA:
                built = h.info("ds_no_na") == 0
                assert built == (R.info["n_na"] > 0), cid
                if R.info["disjoint"]:       # no entry is train and test at once
                    assert built == (h.info("ds_cnt_train") + h.info("ds_cnt_test") < h.n * h.p), cid
            assert (got is not None) == built, (cid, name, "built" if got is not None else "not built")
            assert (ref is not None) == built, (cid, name, "the reference disagrees with the case's statement")
            if got is None:
                with pytest.raises(InsiderError, match="did not build"):
                    read_prefix(h, name, 1)
                continue
            dev[name] = got
            if isinstance(ref, dr.Exact) and rule != "identity":
                want = ref.value.ravel().astype(got.dtype)
                assert got.shape == want.shape, (cid, name, got.shape, want.shape)
                d = slice(None) if ref.defined is None else ref.defined.ravel()
                bad = np.flatnonzero(raw(got)[d] != raw(want)[d])
                assert bad.size == 0, (cid, name, bad[:8], got[d][bad[:8]], want[d][bad[:8]])
            elif isinstance(ref, dr.Bounded):
                want = ref.value.ravel()
                assert got.shape == want.shape, (cid, name, got.shape, want.shape)
                err = np.abs(got - want)
                if ints:
                    assert np.array_equal(got, want), (cid, name, np.flatnonzero(got != want)[:8])
                else:
                    bound = ref.bound.ravel()
                    bad = np.flatnonzero(err > bound)
                    assert bad.size == 0, (cid, name, bad[:8], got[bad[:8]], want[bad[:8]], bound[bad[:8]])
                    pos = bound > 0
                    if pos.any():
                        RATIOS[entry] = max(RATIOS.get(entry, 0.0), float((err[pos] / bound[pos]).max()))
    # ---- identities on the device's own arrays ----
    SLP, SLcat = int(h.info("ds_SLP")), sum(cs["counts"])
    S, St = dev["S"].reshape(p, SLP), dev["Strain"].reshape(p, SLP)
    assert not S[:, SLcat + h.m:].any() and not St[:, SLcat + h.m:].any()             # the pad column of an odd SL
    if cs["merged"]:
        Sh = dev["Sheld"].reshape(p, SLP)
        assert np.array_equal(raw(Sh[:, :SLcat]), raw((S - St)[:, :SLcat])), cid
        if cs["contm"]:       # k_zt_build: S^held is summed over the list, S^train = S - S^held
            assert np.array_equal(raw(St[:, SLcat:]), raw((S - Sh)[:, SLcat:])), cid
        else:                 # S^train's continuous columns are never written (and never read)
            assert not St[:, SLcat:].any() and np.array_equal(raw(Sh[:, SLcat:]), raw(S[:, SLcat:])), cid
    # ---- the packed tables through their decoders: the logical values, and zero wherever the decoder does not look ----
    if cs["cnt"]:
        logical, addressed = dr.decode_cnt(dev["cf_cnt"], g, p)
        for t, want in enumerate(R.logical["cf_cnt"]):
            assert (want is None and logical[t] is None) or np.array_equal(logical[t], want), (cid, "cf_cnt", t)
        assert not dev["cf_cnt"].reshape(p, -1)[:, ~addressed].any(), cid
    else:
        assert "cf_cnt" not in dev
    if cs["pair"]:
        logical, addressed = dr.decode_hn(dev["cf_hn"], g, p)
        for t, want in enumerate(R.logical["cf_hn"]):
            assert np.array_equal(logical[t], want), (cid, "cf_hn", t)
        assert len(logical) == len(R.logical["cf_hn"]) == len(cs["counts"]) + (1 if cs["contm"] else 0)
        assert not dev["cf_hn"].reshape(p + 4, -1)[~addressed].any(), cid          # (the four zero rows included)
        if cs["contm"]:
            assert not logical[-1].any()                                            # position c: 1/2 n = 0
    if cs["pair"] and cs["m"] == 0:
        logical, addressed = dr.decode_sq(dev["cf_sq"], g, p)
        for t in range(g.c):
            cols = slice(g.off[t], g.off[t] + g.L[t])
            assert np.array_equal(raw(logical[t][:, :, 0]), raw(S[:, cols])), (cid, "cf_sq: S", t)
            assert np.array_equal(raw(logical[t][:, :, 1]), raw(Sh[:, cols])), (cid, "cf_sq: Sheld", t)
        assert not dev["cf_sq"].reshape(p, -1)[:, ~addressed].any(), cid
        if ints:
            assert np.array_equal(dev["cf_sq"], R.arrays["cf_sq"].value), cid
    if cs["contm"]:
        _, addressed = dr.decode_zt(dev["cf_zt"], g, p)
        assert not dev["cf_zt"].reshape(p, -1)[:, ~addressed].any(), cid
        for k in range(h.m):
            assert np.array_equal(raw(dev[f"contm.paircnt:{k}"]), raw(dev[f"cont_pair:{k}"]))
    return dev


def total_bytes(h, source):
    """Sum of ds_bytes over the built arrays; contm.paircnt:k is the allocation of cont_pair:k, and a source data set's fold
    ids (set after its creation) are not part of what it counted."""
    tot = 0
    for entry in ARRAYS:
        if entry == "contm.paircnt:#" or (source and entry == "fold_id"):
            continue
        for name in expand(h, entry):
            tot += int(h.info("ds_bytes:" + name))
    return tot


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_table_lists_every_name_the_library_knows():
    X, lev, Z, tr, te = data("m1", True)
    h = create(X, lev, CASES["m1"]["counts"], Z, tr, te)
    names = bytes(h.array("names", np.uint8)).decode().split()
    assert sorted(names) == sorted(ARRAYS), set(names) ^ set(ARRAYS)
    with pytest.raises(InsiderError, match="unknown data-set array"):
        h.info("ds_bytes:no_such_array")
    with pytest.raises(InsiderError, match="unknown data-set array"):
        h.info("ds_bytes:grp:2")                                  # two covariates
    with pytest.raises(InsiderError):
        h.info("ds_nitems:2")
    # the existing contract: more bytes than exist is an error, fewer is a prefix
    rc, _ = read_prefix(h, "yy_all", h.p * 8 + 8, room=h.p * 8 + 8)
    assert rc == _lib.ERR_ARG
    rc, buf = read_prefix(h, "yy_all", 8, room=h.p * 8 + 8)
    assert rc == 0
    assert buf[:8].view(np.float64)[0] == h.array("yy_all", np.float64)[0] and not buf[8:].any()
    h.close()


def test_every_array_is_built_by_some_case():
    for name, (_, _, when) in ARRAYS.items():
        if when == NA:
            continue          # decided by the data: asserted per case; built by the *-na cases (test_dataset)
        if when == FOLDS:
            continue          # test_provenance
        assert (when == NEVER) == (not cases_building(name)), name


@pytest.mark.parametrize("ints", [False, True], ids=["float", "ints"])
@pytest.mark.parametrize("cid", list(CASES))
def test_dataset(cid, ints):
    X, lev, Z, tr, te = data(cid, ints)
    cs = CASES[cid]
    R = dr.build(X, lev, cs["counts"], Z, tr, te)
    h = create(X, lev, cs["counts"], Z, tr, te)
    try:
        dev = check_against_reference(h, R, cid, ints)
        assert h.info("data_bytes_shared") == 0 and h.info("data_bytes_own") == total_bytes(h, source=True), cid
        if cid.endswith("-na"):
            assert "col_flag" in dev
        if cid == "cell255":
            assert dev["cf_cnt"].max() == 255 and dr.decode_cnt(dev["cf_cnt"], R.geometry, h.p)[0][0][0, 0, 0] == 255
        if cid.startswith("cell256"):
            # stage_factored stops at the overflow: the count table stays, clamped to 255, and nothing behind it is built
            assert dev["cf_cnt"].max() == 255 and h.info("pair_count_bytes_per_gene") == 0
            assert R.geometry.hn_stride == 0 and R.geometry.sq_stride == 0 and R.geometry.zt_stride == 0
        if cid == "work-items":
            assert h.info("ds_nitems:0") == 2 and h.info("ds_max_items") == 2       # level 1: 1100 -> 1024 + 96; level 2: none
            assert list(dev["item_begin:0"][:2]) == [0, 1024] and list(dev["item_end:0"][:2]) == [1024, 1120]
            assert dev["wl_idx:0"][1099] == 1099 and (dev["wl_idx:0"][1100:1120] == dr.LIST_PAD).all()
    finally:
        h.close()


def test_zz_ratios_reported():
    """Not a check of its own: prints what the float runs of test_dataset saw (run with -s)."""
    for name in sorted(RATIOS):
        print(f"largest error / bound  {name:18s} {RATIOS[name]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())


@pytest.mark.parametrize("cid", ["n65-p31", "n63-p3", "n128-p33", "n19-p3", "n20-p4", "held-genes-na", "m3", "c5-ties", "L257"])
def test_provenance(cid):
    """A remask handle and a remask_fold handle against a created one on the same masks: array by array, bit for bit; what a
    derived data set shares with its source reads the same through either; the byte counts add up."""
    X, lev, Z, tr, te = data(cid, False)
    cs = CASES[cid]
    n, p = X.shape
    rng = np.random.default_rng(5)
    na = ~tr & ~te
    u = rng.random((n, p))
    tr1, te1 = (u < 0.7) & ~na, (u >= 0.7) & ~na                       # the source's own masks: another draw, the same NA set
    ids = np.where(te, 2, np.where(tr, np.where(u < 0.5, 1, 3), 0)).astype(np.uint8)
    assert all(np.array_equal(a, b) for a, b in zip(dr.fold_masks(ids, 2), (tr, te)))
    src = create(X, lev, cs["counts"], Z, tr1, te1)
    ref = create(X, lev, cs["counts"], Z, tr, te)
    assert src.info("ds_bytes:fold_id") == 0
    src.set_folds(ids, 3)
    derived = {"remask": src.remask(tr, te), "fold": src.fold(2)}
    R = dr.build(X, lev, cs["counts"], Z, tr, te)
    try:
        fid = np.zeros((p, int(src.info("ds_ldn"))), dtype=np.uint8)
        fid[:, :n] = ids.T
        assert np.array_equal(src.array("fold_id"), fid.ravel())
        assert src.info("data_bytes_own") == total_bytes(src, source=True)
        for kind, h in derived.items():
            check_against_reference(h, R, cid, False)
            for entry, (dtype, _, _) in ARRAYS.items():
                for name in expand(h, entry):
                    got, want = h.array(name, dtype), ref.array(name, dtype)
                    if entry == "fold_id":
                        assert np.array_equal(got, fid.ravel()), kind
                        continue
                    assert (got is None) == (want is None), (kind, name)
                    if got is None:
                        continue
                    r = R.arrays[name]
                    d = r.defined if isinstance(r, dr.Exact) and r.defined is not None else slice(None)
                    assert np.array_equal(raw(got)[d], raw(want)[d]), (cid, kind, name)
                    if entry in SHARED:
                        assert np.array_equal(raw(got), raw(src.array(name, dtype))), (cid, kind, name, "shared")
            assert h.info("data_bytes_shared") > 0
            assert h.info("data_bytes_shared") + h.info("data_bytes_own") == total_bytes(h, source=False), (cid, kind)
            shared = sum(int(h.info("ds_bytes:" + name)) for entry in SHARED for name in expand(h, entry))
            assert h.info("data_bytes_shared") == shared, (cid, kind)
    finally:
        for h in (src, ref, *derived.values()):
            h.close()
