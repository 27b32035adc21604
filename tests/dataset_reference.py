"""A host construction (numpy, no GPU) of every array of the resident data set, from the documented meaning of each table.

build(X, levels, n_levels, ctns, M_train, M_test) -> Reference: what insider_hip_create_ex / _remask / _remask_fold are
documented to leave on the device for these inputs, array by array under the names of insider_hip_get_array "ds:<name>"
(include/insider_hip.h), and the scalar facts under the names of insider_hip_get_info.  fold_masks(ids, fold) gives the masks
of insider_hip_remask_fold.

Two kinds of entry:
  Exact(value, defined)   integers, copies and packed counts: the device array must equal `value` wherever `defined` is set
                          (None: everywhere; the cells the library documents as not defined are the 64 list entries behind
                          the last line, the slot behind the last work item and the pads of slev);
  Bounded(value, sumabs, nterms)   floating sums: `value` is the correctly rounded sum (math.fsum over the terms, products
                          split into exact halves first), `sumabs` = sum |term| and `nterms` = N per element, so that a sum of
                          the same terms in any order lies within N 2^-53 sum|term| of it.  Elements with nterms = 0 are exact.

Nothing here follows the kernels' index arithmetic: lists are built by sorting and counting entries, the packed tables by
a brute-force logical array (one cell per gene, position, level and table row) pushed through encode_*, whose inverse
decode_* the tests apply to the device's bytes.  The layouts are those of the comments of ColFacArgs
(insider_col_factored.hpp), k_group_count / k_group_fill (insider_row_merged.hpp), the list contract of k_fill_lists
(insider_kernels.hpp) and the staging functions of insider_hip.hip."""
import math
from dataclasses import dataclass

import numpy as np

# constants of the layouts (insider_kernels.hpp, insider_shapes.hpp, insider_col_factored.hpp, insider_hip.hip)
CHUNK = 128            # line pitch: ldn, ldp are multiples of it
LEVEL_CHUNK = 4        # member samples per chunk of the chunk tables
LIST_ALIGN = 32        # every list is padded to a multiple of it
LIST_BLOCK = 64        # entries allocated (and not defined) behind the last list
LIST_PAD = 0x7FFFFF    # index of a padding entry
SEG = 1024             # list entries per weighted-SYRK work item
CODE_TRAIN, CODE_TEST = 1, 2
CF_MAXC = 8            # covariates of the factored statistics
CP_MAXSTEPS = 8        # pair-count form: table rows / 4
CF_SQ_BLOCK = 36       # doubles per gene and block of 16 levels of cf_sq
GU_TILE, GU_BATCH, WAVE = 512, 8, 64
LDS_BYTES = 64 * 1024
GEOMETRY_INTS = 10 + 6 * (CF_MAXC + 1) + CF_MAXC + CF_MAXC * CF_MAXC
U = 2.0 ** -53


def round_up(x, a):
    return (x + a - 1) // a * a


@dataclass
class Exact:
    value: np.ndarray
    defined: np.ndarray = None


@dataclass
class Bounded:
    value: np.ndarray      # float64
    sumabs: np.ndarray
    nterms: np.ndarray

    @property
    def bound(self):
        return self.nterms * U * self.sumabs


# ---- sums -------------------------------------------------------------------------------------------------------------------
def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def exact_products(a, b):
    """a * b as unevaluated pairs (p, e) with p + e = a b exactly (Dekker); flat list of 2 len(a) floats."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def sum_ref(terms):
    """-> (correctly rounded sum, sum |term|, N) of the given terms."""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(terms), math.fsum(np.abs(terms)), len(terms)


def dot_ref(a, b):
    """-> (correctly rounded sum_i a_i b_i, sum |a_i b_i|, N)."""
    p, e = exact_products(np.ravel(a), np.ravel(b))
    return math.fsum(np.concatenate([p, e])), math.fsum(np.abs(p)), len(p)


def _bounded(shape):
    return Bounded(np.zeros(shape), np.zeros(shape), np.zeros(shape))


def _put(b, idx, triple):
    b.value[idx], b.sumabs[idx], b.nterms[idx] = triple


# ---- masks ------------------------------------------------------------------------------------------------------------------
def fold_masks(ids, fold):
    """Masks of insider_hip_remask_fold: test = the entries whose id is `fold`, train = the entries of every other fold, id 0 = NA."""
    ids = np.asarray(ids)
    return (ids != fold) & (ids != 0), ids == fold


# ---- geometry of the factored column statistics -------------------------------------------------------------------------------
@dataclass
class Geometry:
    """The static part of ColFacArgs; as_array() is "ds:cf_geometry" in the order of include/insider_hip.h."""
    c: int = 0
    nsteps: int = 0
    tab_skip_lo: int = 0
    tab_skip_n: int = 0
    tab_rows: int = 0
    cnt_stride: int = 0
    hn_stride: int = 0
    zt_stride: int = 0
    sq_stride: int = 0
    m: int = 0
    L: list = None
    off: list = None
    nlater: list = None
    cnt_off: list = None
    hn_off: list = None
    zt_off: list = None
    pos_cov: list = None
    later_plane: list = None
    # decisions (not part of the array)
    cnt_built: bool = False        # the dense pair counts are allocated (the geometry fits; cells may still overflow)
    zc: bool = False               # position c (the continuous columns) exists

    def __post_init__(self):
        for f in ("L", "off", "nlater", "cnt_off", "hn_off", "zt_off"):
            if getattr(self, f) is None:
                setattr(self, f, [0] * (CF_MAXC + 1))
        if self.pos_cov is None:
            self.pos_cov = [0] * CF_MAXC
        if self.later_plane is None:
            self.later_plane = [[0] * CF_MAXC for _ in range(CF_MAXC)]

    @property
    def bpl(self):                 # count bytes per lane and block of 16 levels
        return 4 if self.nsteps <= 4 else 8

    def as_array(self):
        g = [self.c, self.nsteps, self.tab_skip_lo, self.tab_skip_n, self.tab_rows, self.cnt_stride, self.hn_stride,
             self.zt_stride, self.sq_stride, self.m]
        for f in (self.L, self.off, self.nlater, self.cnt_off, self.hn_off, self.zt_off):
            g += list(f)
        g += list(self.pos_cov)
        for row in self.later_plane:
            g += list(row)
        assert len(g) == GEOMETRY_INTS
        return np.array(g, dtype=np.int32)

    @classmethod
    def from_array(cls, a):
        a = [int(x) for x in a]
        g = cls(*a[:10])
        o = 10
        for f in ("L", "off", "nlater", "cnt_off", "hn_off", "zt_off"):
            setattr(g, f, a[o:o + CF_MAXC + 1])
            o += CF_MAXC + 1
        g.pos_cov = a[o:o + CF_MAXC]
        o += CF_MAXC
        g.later_plane = [a[o + CF_MAXC * t:o + CF_MAXC * (t + 1)] for t in range(CF_MAXC)]
        g.zc = g.zt_stride > 0
        return g


def merged_shape(n_levels, m):
    """The merged row update's tables exist: at most four continuous columns, and four waves' look-up rows (all categorical
    levels + a tile of 512 entries, doubles) fit 64 KiB of LDS."""
    return m <= 4 and 4 * (sum(n_levels) + GU_TILE) * 8 <= LDS_BYTES


def gu_fits(n_levels, m):
    """Every covariate's per-wave record of k_gene_u_cnt — a row of V [SL], its output [L rounded up to 2] and GU_BATCH x 64
    partial sums, doubles, four waves per block — fits 64 KiB of LDS."""
    SL = sum(n_levels) + m
    return all(4 * (SL + round_up(L, 2) + GU_BATCH * WAVE) * 8 <= LDS_BYTES for L in n_levels)


def geometry(n_levels, m, p, n, overflow=False):
    """The geometry stage_factored and stage_cont_factored leave for level counts n_levels, m continuous columns and p genes of
    n samples; `overflow`: some cell of the dense pair counts exceeds 255.  -> (Geometry, cf_pair_ok).  Callers check
    merged_shape and c <= CF_MAXC first (no factored tables otherwise: an all-zero geometry)."""
    c = len(n_levels)
    lvl_off = np.concatenate([[0], np.cumsum(n_levels)]).astype(int)
    SLcat = int(lvl_off[c])
    order = sorted(range(c), key=lambda i: -n_levels[i])        # descending level count; sorted() is stable on ties
    g = Geometry(c=c, m=m)
    for t, o in enumerate(order):
        g.L[t], g.off[t], g.nlater[t], g.pos_cov[t] = int(n_levels[o]), int(lvl_off[o]), c - 1 - t, o
        # the planes of slev of covariate o hold the OTHER covariates in covariate order
        for k in range(t + 1, c):
            others = [q for q in range(c) if q != o]
            g.later_plane[t][k - t - 1] = others.index(order[k])
    g.tab_skip_lo, g.tab_skip_n = g.off[0], g.L[0]              # position 0 is never a later covariate: not a table row
    g.tab_rows = SLcat - g.tab_skip_n
    g.nsteps = (g.tab_rows + 3) // 4
    off = 0
    for t in range(c):
        g.cnt_off[t] = off
        if g.nlater[t] > 0:
            off += (g.L[t] + 15) // 16 * 64 * g.bpl
    g.cnt_stride = off
    fits = g.nsteps <= CP_MAXSTEPS
    pair_ok = False
    if fits and off <= 64 * 1024 and p * off <= 2 ** 32:
        g.cnt_built = off > 0
        pair_ok = not (g.cnt_built and overflow) and n < 2 ** 24
        if pair_ok:
            hoff = 0
            for t in range(c):
                g.hn_off[t] = hoff
                hoff += (g.L[t] + 15) // 16 * 16
            g.hn_stride = hoff
            g.sq_stride = hoff // 16 * CF_SQ_BLOCK
    if m > 0 and pair_ok and gu_fits(n_levels, m):
        g.zc = True
        g.L[c], g.off[c], g.nlater[c], g.cnt_off[c] = m, SLcat, 0, 0
        z = 0
        for t in range(c):
            g.zt_off[t] = z
            z += (g.L[t] + 15) // 16 * 64
        g.zt_off[c] = z
        g.zt_stride = z + 64
        g.hn_off[c] = g.hn_stride
        g.hn_stride += 16
    return g, pair_ok


def table_row(g, stacked):
    """Row of the look-up table of stacked level `stacked` (the levels of position 0 are not in the table)."""
    assert not g.tab_skip_lo <= stacked < g.tab_skip_lo + g.tab_skip_n
    return stacked if stacked < g.tab_skip_lo else stacked - g.tab_skip_n


# ---- the packed tables: logical array <-> bytes ---------------------------------------------------------------------------------
# cf_cnt: per gene and position t with later covariates, n_j(l, q) for level l of the covariate at t and table row q, one byte,
# at [l / 16][lane = (q % 4) * 16 + l % 16][q / 4] with bpl bytes per lane.  Logical array: list over positions of
# [p][L_t][4 nsteps] (None for a position without later covariates).
def _cnt_index(g, t, l, q):
    return g.cnt_off[t] + ((l // 16) * 64 + (q % 4) * 16 + l % 16) * g.bpl + q // 4


def encode_cnt(logical, g, p):
    out = np.zeros((p, g.cnt_stride), dtype=np.uint8)
    for t in range(g.c):
        if logical[t] is None:
            continue
        for l in range(g.L[t]):
            for q in range(logical[t].shape[2]):
                out[:, _cnt_index(g, t, l, q)] = logical[t][:, l, q]
    return out


def decode_cnt(table, g, p):
    """-> (logical, addressed): the counts per position, and a mask of the table's bytes the decoder read."""
    table = np.asarray(table).reshape(p, g.cnt_stride)
    addressed = np.zeros(g.cnt_stride, dtype=bool)
    logical = []
    for t in range(g.c):
        if g.nlater[t] == 0:
            logical.append(None)
            continue
        a = np.zeros((p, g.L[t], 4 * g.nsteps), dtype=np.int64)
        for l in range(g.L[t]):
            for q in range(4 * g.nsteps):
                i = _cnt_index(g, t, l, q)
                a[:, l, q] = table[:, i]
                addressed[i] = True
        logical.append(a)
    return logical, addressed


# cf_hn: 1/2 n_j(l) as floats, per position at [block of 16 levels][l % 4][(l % 16) / 4]; position c (continuous columns): 16
# zeros; four zero rows behind the last gene.  Logical: list over positions of [p][L_t] (position c: [p][m] zeros).
def _hn_index(g, t, l):
    return g.hn_off[t] + (l // 16) * 16 + (l % 4) * 4 + (l % 16) // 4


def _positions(g):
    return g.c + (1 if g.zc else 0)


def encode_hn(logical, g, p):
    out = np.zeros((p + 4, g.hn_stride), dtype=np.float32)
    for t in range(_positions(g)):
        for l in range(g.L[t]):
            out[:p, _hn_index(g, t, l)] = logical[t][:, l]
    return out


def decode_hn(table, g, p):
    table = np.asarray(table).reshape(p + 4, g.hn_stride)
    addressed = np.zeros((p + 4, g.hn_stride), dtype=bool)
    logical = []
    for t in range(_positions(g)):
        a = np.zeros((p, g.L[t]), dtype=np.float32)
        for l in range(g.L[t]):
            a[:, l] = table[:p, _hn_index(g, t, l)]
            addressed[:p, _hn_index(g, t, l)] = True
        logical.append(a)
    return logical, addressed


# cf_sq: per gene and block of 16 levels (the blocks of cf_hn) 36 doubles [S | S^held][l % 4][(l % 16) / 4], then four zeros.
# Logical: list over the categorical positions of [p][L_t][2] (S, S^held).
def _sq_index(g, t, l, which):
    return (g.hn_off[t] // 16 + l // 16) * CF_SQ_BLOCK + 16 * which + (l % 4) * 4 + (l % 16) // 4


def encode_sq(logical, g, p):
    out = np.zeros((p, g.sq_stride))
    for t in range(g.c):
        for l in range(g.L[t]):
            for w in range(2):
                out[:, _sq_index(g, t, l, w)] = logical[t][:, l, w]
    return out


def decode_sq(table, g, p):
    table = np.asarray(table).reshape(p, g.sq_stride)
    addressed = np.zeros(g.sq_stride, dtype=bool)
    logical = []
    for t in range(g.c):
        a = np.zeros((p, g.L[t], 2))
        for l in range(g.L[t]):
            for w in range(2):
                a[:, l, w] = table[:, _sq_index(g, t, l, w)]
                addressed[_sq_index(g, t, l, w)] = True
        logical.append(a)
    return logical, addressed


# cf_zt: real-valued counts zeta_jl[k] = sum_{i in l, held out in j} z_ik per categorical position at
# [position offset + block of 16 levels][lane = k * 16 + l % 16], and position c: 1/2 ZZ_j[k][k'] at lane k' * 16 + k.
# Logical: list over the categorical positions of [p][L_t][m], then [p][m][m].
def _zt_index(g, t, l, k):
    return g.zt_off[t] + (l // 16) * 64 + k * 16 + l % 16


def encode_zt(logical, g, p):
    out = np.zeros((p, g.zt_stride))
    for t in range(g.c):
        for l in range(g.L[t]):
            for k in range(g.m):
                out[:, _zt_index(g, t, l, k)] = logical[t][:, l, k]
    for k in range(g.m):
        for k2 in range(g.m):
            out[:, g.zt_off[g.c] + k2 * 16 + k] = logical[g.c][:, k, k2]
    return out


def decode_zt(table, g, p):
    table = np.asarray(table).reshape(p, g.zt_stride)
    addressed = np.zeros(g.zt_stride, dtype=bool)
    logical = []
    for t in range(g.c):
        a = np.zeros((p, g.L[t], g.m))
        for l in range(g.L[t]):
            for k in range(g.m):
                a[:, l, k] = table[:, _zt_index(g, t, l, k)]
                addressed[_zt_index(g, t, l, k)] = True
        logical.append(a)
    a = np.zeros((p, g.m, g.m))
    for k in range(g.m):
        for k2 in range(g.m):
            a[:, k, k2] = table[:, g.zt_off[g.c] + k2 * 16 + k]
            addressed[g.zt_off[g.c] + k2 * 16 + k] = True
    logical.append(a)
    return logical, addressed


# ---- lists ------------------------------------------------------------------------------------------------------------------
def padded_lists(lines):
    """lines: per line a list of (index, value, flag) tuples -> ptr (uint32, len + 1), idx, val, flag and `defined`: every
    line padded to a multiple of LIST_ALIGN with (LIST_PAD, 0.0, 0), LIST_BLOCK undefined entries behind the last."""
    ptr = [0]
    idx, val, flag = [], [], []
    for ln in lines:
        pad = round_up(len(ln), LIST_ALIGN) - len(ln)
        idx += [e[0] for e in ln] + [LIST_PAD] * pad
        val += [e[1] for e in ln] + [0.0] * pad
        flag += [e[2] for e in ln] + [0] * pad
        ptr.append(len(idx))
    defined = np.array([True] * len(idx) + [False] * LIST_BLOCK)
    tail = [0] * LIST_BLOCK
    return (np.array(ptr, dtype=np.uint32), np.array(idx + tail, dtype=np.int32), np.array(val + tail, dtype=np.float64),
            np.array(flag + tail, dtype=np.uint8), defined)


def work_items(list_lengths):
    """Work items of at most SEG entries over consecutive padded lists -> begin, end (one undefined slot behind), item ptr."""
    ib, ie, lip, start = [], [], [0], 0
    for ln in list_lengths:
        for b in range(start, start + ln, SEG):
            ib.append(b)
            ie.append(min(b + SEG, start + ln))
        start += ln
        lip.append(len(ib))
    defined = np.array([True] * len(ib) + [False])
    return (np.array(ib + [0], dtype=np.uint32), np.array(ie + [0], dtype=np.uint32), np.array(lip, dtype=np.int32), defined)


# ---- the data set -------------------------------------------------------------------------------------------------------------
class Reference:
    def __init__(self):
        self.arrays = {}       # name -> Exact | Bounded | None (known name, not built)
        self.info = {}         # name of insider_hip_get_info -> value
        self.geometry = None   # Geometry (all zero: no factored tables)
        self.logical = {}      # "cf_cnt", "cf_hn", "cf_sq", "cf_zt" -> the logical arrays the packed tables encode


def build(X, levels, n_levels, ctns, M_train, M_test):
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    lev = np.asarray(levels).reshape(n, -1).astype(np.int64) - 1          # 0-based
    c = lev.shape[1]
    n_levels = [int(v) for v in n_levels]
    Z = None if ctns is None else np.asarray(ctns, dtype=np.float64).reshape(n, -1)
    m = 0 if Z is None else Z.shape[1]
    tr, te = np.asarray(M_train).astype(bool), np.asarray(M_test).astype(bool)
    held = ~tr                                                             # held out = not a train entry (test or NA)
    ldn, ldp = round_up(n, CHUNK), round_up(p, CHUNK)
    lvl_off = [0]
    for L in n_levels:
        lvl_off.append(lvl_off[-1] + L)
    SLcat = lvl_off[c]
    SL = SLcat + m
    SLP = round_up(SL, 2)
    R = Reference()
    A, I = R.arrays, R.info
    I.update(ds_ldn=ldn, ds_ldp=ldp, ds_SLP=SLP, ds_cnt_train=int(tr.sum()), ds_cnt_test=int(te.sum()))
    no_na = not (~tr & ~te).any()                                          # every entry is train or test (or both)
    I["ds_no_na"] = int(no_na)
    I.update(n_na=int((~tr & ~te).sum()), disjoint=not (tr & te).any())    # facts about the masks (no library names)

    # X and the mask codes: p gene-major lines of pitch ldn; pads: x = 0, code = train (never held out)
    Xd = np.zeros((p, ldn))
    Xd[:, :n] = X.T
    A["X"] = Exact(Xd.ravel())
    codes = np.full((p, ldn), CODE_TRAIN, dtype=np.uint8)
    codes[:, :n] = (tr.T * CODE_TRAIN + te.T * CODE_TEST).astype(np.uint8)
    A["codes"] = Exact(codes.ravel())

    # level tables
    A["lev"] = Exact(lev.T.astype(np.int32).ravel())
    A["lvl_off_d"] = Exact(np.array(lvl_off, dtype=np.int32))
    members, ptrs, counts = [], [], []
    max_chunks = max_L = 0
    for i in range(c):
        L = n_levels[i]
        mem = [[r for r in range(n) if lev[r, i] == l] for l in range(L)]   # ascending sample id inside a level
        members.append(np.array([r for g_ in mem for r in g_], dtype=np.int32))
        ptr = np.concatenate([[0], np.cumsum([len(g_) for g_ in mem])]).astype(np.int32)
        ptrs.append(ptr)
        counts.append(np.array([len(g_) for g_ in mem], dtype=np.int32))
        cl, cb, ce, lcp = [], [], [], [0]
        for l in range(L):
            for b in range(int(ptr[l]), int(ptr[l + 1]), LEVEL_CHUNK):
                cl.append(l)
                cb.append(b)
                ce.append(min(b + LEVEL_CHUNK, int(ptr[l + 1])))
            lcp.append(len(cl))
        # (an allocation holds at least one element: an empty table is one undefined int)
        for name, v in (("chunk_level", cl), ("chunk_begin", cb), ("chunk_end", ce)):
            A[f"{name}:{i}"] = Exact(np.array(v or [0], dtype=np.int32), None if v else np.array([False]))
        A[f"lvl_chunk_ptr:{i}"] = Exact(np.array(lcp, dtype=np.int32))
        max_chunks, max_L = max(max_chunks, len(cl)), max(max_L, L)
    A["members_all"] = Exact(np.concatenate(members))
    A["lvl_ptr_all"] = Exact(np.concatenate(ptrs))
    A["lvl_count_all"] = Exact(np.concatenate(counts))
    if m:
        A["Zc"] = Exact(Z.T.ravel().copy())
        A["one_count"] = Exact(np.array([1], dtype=np.int32))
        A["ident_members"] = Exact(np.arange(n, dtype=np.int32))
        cb = list(range(0, n, LEVEL_CHUNK))
        A["cont.chunk_begin"] = Exact(np.array(cb, dtype=np.int32))
        A["cont.chunk_end"] = Exact(np.array([min(b + LEVEL_CHUNK, n) for b in cb], dtype=np.int32))
        A["cont.lvl_chunk_ptr"] = Exact(np.array([0, len(cb)], dtype=np.int32))
        max_chunks, max_L = max(max_chunks, len(cb)), max(max_L, 1)
    I.update(ds_max_chunks=max_chunks, ds_max_L=max_L)

    # per-level sums of X: all entries, train entries, held-out entries; sums of squares
    S, Strain, Sheld_direct = _bounded((p, SLP)), _bounded((p, SLP)), _bounded((p, SLP))
    yy_all, yy_train = _bounded(p), _bounded(p)
    for j in range(p):
        x = X[:, j]
        _put(yy_all, j, dot_ref(x, x))
        _put(yy_train, j, dot_ref(x[tr[:, j]], x[tr[:, j]]))
        for i in range(c):
            for l in range(n_levels[i]):
                inl = lev[:, i] == l
                _put(S, (j, lvl_off[i] + l), sum_ref(x[inl]))
                _put(Strain, (j, lvl_off[i] + l), sum_ref(x[inl & tr[:, j]]))
                _put(Sheld_direct, (j, lvl_off[i] + l), sum_ref(x[inl & held[:, j]]))
        for k in range(m):
            _put(S, (j, SLcat + k), dot_ref(x, Z[:, k]))
            _put(Strain, (j, SLcat + k), dot_ref(x[tr[:, j]], Z[tr[:, j], k]))
            _put(Sheld_direct, (j, SLcat + k), dot_ref(x[held[:, j]], Z[held[:, j], k]))
    A["S"], A["yy_all"], A["yy_train"] = S, yy_all, yy_train

    # held-out lists of both sides: ascending element index inside a line
    col_lines = [[(i, X[i, j], int(te[i, j])) for i in range(n) if held[i, j]] for j in range(p)]
    row_lines = [[(j, X[i, j], 0) for j in range(p) if held[i, j]] for i in range(n)]
    cptr, cidx, cval, cflag, cdef = padded_lists(col_lines)
    rptr, ridx, rval, _, rdef = padded_lists(row_lines)
    A["col_ptr"], A["col_idx"], A["col_val"] = Exact(cptr), Exact(cidx, cdef), Exact(cval, cdef)
    A["row_ptr"], A["row_idx"], A["row_val"] = Exact(rptr), Exact(ridx, rdef), Exact(rval, rdef)
    A["col_flag"] = None if no_na else Exact(cflag, cdef)       # kept only when the data has NA entries
    col_entries = int(cptr[-1])
    I.update(col_entries=col_entries, row_entries=int(rptr[-1]))
    plane = col_entries + LIST_BLOCK

    # level-pair sample counts (mask-independent; they count samples, not entries)
    merged = merged_shape(n_levels, m)
    I["ds_merged"] = int(merged)
    if merged:
        for i in range(c):
            pc = _bounded((n_levels[i], SL))                                # L rows of pitch SL (all levels + m)
            for l in range(n_levels[i]):
                inl = lev[:, i] == l
                for q in range(c):
                    if q != i:
                        for l2 in range(n_levels[q]):
                            pc.value[l, lvl_off[q] + l2] = np.sum(inl & (lev[:, q] == l2))
                for k in range(m):
                    _put(pc, (l, SLcat + k), sum_ref(Z[inl, k]))
            A[f"paircnt:{i}"] = pc
        if m and c <= CF_MAXC:
            cc = _bounded(m)
            for k in range(m):
                pc = _bounded(SL)
                for q in range(c):
                    for l2 in range(n_levels[q]):
                        _put(pc, lvl_off[q] + l2, sum_ref(Z[lev[:, q] == l2, k]))
                for k2 in range(m):
                    if k2 != k:
                        _put(pc, SLcat + k2, dot_ref(Z[:, k], Z[:, k2]))
                A[f"cont_pair:{k}"] = pc
                _put(cc, k, dot_ref(Z[:, k], Z[:, k]))
            A["cont_cnt"] = cc

    # merged row update: per covariate the genes' held-out samples stably grouped by level, and the (gene, count) lists
    grouped = {}                                                           # (i, j) -> the gene's held-out samples, grouped
    max_items = 0
    if merged:
        nplanes = max(c - 1, 1)
        for i in range(c):
            L = n_levels[i]
            grp = np.zeros((p, L + 1), dtype=np.uint32)
            slev = np.zeros((nplanes, plane), dtype=np.uint16)
            sdef = np.zeros((nplanes, plane), dtype=bool)
            cnt = np.zeros((p, L), dtype=np.int64)
            others = [q for q in range(c) if q != i]
            for j in range(p):
                hs = [e[0] for e in col_lines[j]]
                hs = sorted(hs, key=lambda r: lev[r, i])                   # stable: ascending sample id inside a level
                grouped[i, j] = hs
                for r in hs:
                    cnt[j, lev[r, i]] += 1
                grp[j] = int(cptr[j]) + np.concatenate([[0], np.cumsum(cnt[j])])
                for o, q in enumerate(others):
                    for x, r in enumerate(hs):
                        slev[o, int(cptr[j]) + x] = lvl_off[q] + lev[r, q]
                        sdef[o, int(cptr[j]) + x] = True
            A[f"grp:{i}"] = Exact(grp.ravel())
            A[f"slev:{i}"] = Exact(slev.ravel(), sdef.ravel())
            lines = [[(j, float(cnt[j, l]), 0) for j in range(p) if cnt[j, l]] for l in range(L)]
            wptr, widx, ww, _, wdef = padded_lists(lines)
            ib, ie, lip, idef = work_items(np.diff(wptr.astype(np.int64)))
            A[f"wl_idx:{i}"], A[f"wl_w:{i}"] = Exact(widx, wdef), Exact(ww, wdef)
            A[f"item_begin:{i}"], A[f"item_end:{i}"], A[f"lvl_item_ptr:{i}"] = Exact(ib, idef), Exact(ie, idef), Exact(lip)
            I[f"ds_nitems:{i}"] = len(ib) - 1
            I[f"ds_npairs:{i}"] = int((cnt > 0).sum())
            max_items = max(max_items, len(ib) - 1)
    else:
        for i in range(c):
            I[f"ds_nitems:{i}"] = I[f"ds_npairs:{i}"] = 0

    # factored column statistics
    R.geometry = Geometry()
    pair_ok = False
    if merged and c <= CF_MAXC:
        g0, _ = geometry(n_levels, m, p, n)
        # brute force over the entries: n_j(l, q) for every position with later covariates
        cnt_logical = []
        for t in range(c):
            if g0.nlater[t] == 0:
                cnt_logical.append(None)
                continue
            a = np.zeros((p, g0.L[t], 4 * g0.nsteps if g0.nsteps <= CP_MAXSTEPS else g0.tab_rows), dtype=np.int64)
            for j in range(p):
                for r in grouped[g0.pos_cov[t], j]:
                    for t2 in range(t + 1, c):
                        q = table_row(g0, g0.off[t2] + lev[r, g0.pos_cov[t2]])
                        a[j, lev[r, g0.pos_cov[t]], q] += 1
            cnt_logical.append(a)
        overflow = any(a is not None and a.max(initial=0) > 255 for a in cnt_logical)
        g, pair_ok = geometry(n_levels, m, p, n, overflow)
        R.geometry = g
        if g.cnt_built:
            # (a cell above 255 is stored as 255: the table is then not used, ds_cf_pair_ok = 0)
            R.logical["cf_cnt"] = [None if a is None else np.minimum(a, 255) for a in cnt_logical]
            A["cf_cnt"] = Exact(encode_cnt(R.logical["cf_cnt"], g, p).ravel())
        if pair_ok:
            hn = [np.array([[0.5 * sum(1 for r in grouped[g.pos_cov[t], j] if lev[r, g.pos_cov[t]] == l)
                             for l in range(g.L[t])] for j in range(p)], dtype=np.float32).reshape(p, g.L[t])
                  for t in range(c)]
            if g.zc:
                hn.append(np.zeros((p, m), dtype=np.float32))              # position c: 1/2 n = 0
            R.logical["cf_hn"] = hn
            A["cf_hn"] = Exact(encode_hn(hn, g, p).ravel())
    I["ds_cf_pair_ok"] = int(pair_ok)
    g = R.geometry

    # continuous columns on the pair-count form
    cont_merged = g.zc
    I["ds_cont_merged"] = int(cont_merged)
    if cont_merged:
        zt = [(_bounded((p, g.L[t], m))) for t in range(c)] + [_bounded((p, m, m))]
        wl = [_bounded(round_up(p, LIST_ALIGN) + LIST_BLOCK) for _ in range(m)]
        for j in range(p):
            h = held[:, j]
            for t in range(c):
                o = g.pos_cov[t]
                for l in range(g.L[t]):
                    for k in range(m):
                        _put(zt[t], (j, l, k), sum_ref(Z[h & (lev[:, o] == l), k]))
            for k in range(m):
                for k2 in range(m):
                    v, s, N = dot_ref(Z[h, k], Z[h, k2])
                    _put(zt[c], (j, k, k2), (0.5 * v, 0.5 * s, N))
                _put(wl[k], j, dot_ref(Z[h, k], Z[h, k]))
        R.logical["cf_zt"] = zt
        A["cf_zt"] = Bounded(*(encode_zt([getattr(b, f) for b in zt], g, p).ravel() for f in ("value", "sumabs", "nterms")))
        widx = np.full(round_up(p, LIST_ALIGN) + LIST_BLOCK, LIST_PAD, dtype=np.int32)
        widx[:p] = np.arange(p)
        wdef = np.arange(len(widx)) < round_up(p, LIST_ALIGN)
        ib, ie, lip, idef = work_items([round_up(p, LIST_ALIGN)])
        A["contm_lists.wl_idx"] = Exact(widx, wdef)
        A["contm_lists.item_begin"], A["contm_lists.item_end"] = Exact(ib, idef), Exact(ie, idef)
        A["contm_lists.lvl_item_ptr"] = Exact(lip)
        max_items = max(max_items, len(ib) - 1)
        for k in range(m):
            A[f"contm.wl_w:{k}"] = wl[k]                                    # (zero on the pads and behind them)
            A[f"contm.paircnt:{k}"] = A[f"cont_pair:{k}"]
    I["ds_max_items"] = max_items

    # S^train and S^held as the device keeps them.  Categorical columns: the sums over the train entries, and S - S^train
    # (terms of both).  Continuous columns: with the continuous columns on the merged form S^held is the sum of x z over the
    # gene's held-out list and S^train = S - S^held; without it S^train's continuous columns are never written (0) and no
    # kernel reads them.
    St = Bounded(Strain.value.copy(), Strain.sumabs.copy(), Strain.nterms.copy())
    Sh = Bounded(Sheld_direct.value.copy(), S.sumabs + Strain.sumabs, S.nterms + Strain.nterms)
    if m:
        cs = slice(SLcat, SL)
        if cont_merged:
            Sh.sumabs[:, cs], Sh.nterms[:, cs] = Sheld_direct.sumabs[:, cs], Sheld_direct.nterms[:, cs]
            St.sumabs[:, cs] = S.sumabs[:, cs] + Sheld_direct.sumabs[:, cs]
            St.nterms[:, cs] = S.nterms[:, cs] + Sheld_direct.nterms[:, cs]
        else:
            for b in (St.value, St.sumabs, St.nterms):
                b[:, cs] = 0.0
            Sh.value[:, cs], Sh.sumabs[:, cs], Sh.nterms[:, cs] = S.value[:, cs], S.sumabs[:, cs], S.nterms[:, cs]
    A["Strain"] = Bounded(St.value.ravel(), St.sumabs.ravel(), St.nterms.ravel())
    A["S"] = Bounded(S.value.ravel(), S.sumabs.ravel(), S.nterms.ravel())
    if merged:
        A["Sheld"] = Bounded(Sh.value.ravel(), Sh.sumabs.ravel(), Sh.nterms.ravel())
    if pair_ok and m == 0:
        sq = [np.stack([S.value[:, g.off[t]:g.off[t] + g.L[t]], Sh.value[:, g.off[t]:g.off[t] + g.L[t]]], axis=2)
              for t in range(c)]
        R.logical["cf_sq"] = sq                # (compared bit for bit with the DEVICE's S and Sheld: see the tests)
        A["cf_sq"] = Exact(encode_sq(sq, g, p).ravel())
    return R
