"""Host-side mirror of the reference's operator interface for the hot path.

Operator level (names and argument meaning of /root/reference/R/RcppExports.R:4-22):
    optimize(data, cfd_factors, column_factor, cfd_indicators, ctns_confounder, train_indicator,
             test_indicator, inc_continuous, latent_dim, lambda1, lambda2, alpha, tuning, global_tol,
             sub_tol, max_iter)
    strong_coordinate_descent(X, y, wstart, lambda_, alpha, XtX, Xty, tol)
    optimize_continuous_v2(data, indicator, updating_factor, c_factor, updating_confd, gram, lambda_, tuning)
Caller level (R/insider.R:18-216, R/utils.R:40-43,78-117) — R is absent from this pipeline, so the R S3 API is
mirrored here in Python with the same names, defaults and error behaviour:
    insider(), tune(), fit(), ratio_splitter(), init_parameters()

All compute goes through libinsider_hip.so (insider_amd/_lib.py); nothing here falls back to the CPU.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import InsiderError

DEFAULT_SEED = 0x1D5EED


class InsiderData:
    """A data set resident in HBM (insider_hip_create). Reused across optimize() calls, e.g. by tune()'s grid."""

    def __init__(self, data, cfd_indicators, train_indicator, test_indicator, device=0, n_levels=None,
                 ctns_confounder=None):
        lib = _lib.load()
        X = _lib.f64(data)
        n, p = X.shape
        lev = np.asfortranarray(np.asarray(cfd_indicators).reshape(n, -1), dtype=np.int32)
        c = lev.shape[1]
        if n_levels is None:
            # R/insider.R:107: factor_num <- length(unique(confounder[, i])); ids must be exactly 1..L_i
            n_levels = np.array([len(np.unique(lev[:, i])) for i in range(c)], dtype=np.int32)
        n_levels = np.ascontiguousarray(n_levels, dtype=np.int32)
        Mtr = np.asfortranarray(train_indicator, dtype=np.uint8)
        Mte = np.asfortranarray(test_indicator, dtype=np.uint8)
        if Mtr.shape != (n, p) or Mte.shape != (n, p):
            raise InsiderError(_lib.ERR_ARG, "indicator shape must match data")
        self.n, self.p, self.c = n, p, c
        self.n_levels = n_levels
        self._h = C.c_void_p()
        if ctns_confounder is not None:
            Z = _lib.f64(np.asarray(ctns_confounder, dtype=np.float64).reshape(n, -1))
            self.m = Z.shape[1]
            zp = _lib.ptr(Z)
        else:
            self.m, zp = 0, None
        _lib.check(lib.insider_hip_create_ex(_lib.ptr(X), n, p, _lib.ptr(lev, C.c_int32), c,
                                             _lib.ptr(n_levels, C.c_int32), zp, self.m, _lib.ptr(Mtr, C.c_uint8),
                                             _lib.ptr(Mte, C.c_uint8), int(device), C.byref(self._h)))
        self._cb = None  # keeps the ctypes callback alive
        # measurement knob: INSIDER_HIP_OPTIONS="name=value,name=value" applies library options to every handle this process
        # creates (A/B of an option through tools that do not expose it)
        for kv in filter(None, os.environ.get("INSIDER_HIP_OPTIONS", "").split(",")):
            name, value = kv.split("=")
            self.set_option(name.strip(), float(value))

    def clone(self):
        """Another handle on the SAME resident data set (insider_hip_clone): the device copy of X, the lists and the
        count tables are shared, the factor workspace, streams and options (copied as they stand) are its own.  Handles of
        one data set may fit at the same time from different threads (tune(concurrent=k))."""
        other = object.__new__(InsiderData)
        other.n, other.p, other.c, other.m, other.n_levels = self.n, self.p, self.c, self.m, self.n_levels
        other._h = C.c_void_p()
        other._cb = None
        other._options = dict(getattr(self, "_options", {}))       # the library copies the options as they stand
        other._folds = self._fold_state()                          # one data set: the clone sees the same fold ids
        _lib.check(_lib.load().insider_hip_clone(self._h, C.byref(other._h)))
        return other

    def _fold_state(self):
        """{"F": number of folds} once set_folds() has run on a handle of this data set; shared by its clones."""
        return self.__dict__.setdefault("_folds", {})

    def _derived(self, call):
        """A handle on a new data set over this one's resident X (insider_hip_remask / insider_hip_remask_fold)."""
        other = object.__new__(InsiderData)
        other.n, other.p, other.c, other.m, other.n_levels = self.n, self.p, self.c, self.m, self.n_levels
        other._h = C.c_void_p()
        other._cb = None
        other._options = dict(getattr(self, "_options", {}))
        other._folds = dict(self._fold_state())                    # the new data set carries the ids it was derived under
        _lib.check(call(C.byref(other._h)))
        return other

    def remask(self, train_indicator, test_indicator):
        """A handle on a NEW data set over the SAME resident X with other masks (insider_hip_remask): X, the level and chunk
        tables, the all-entry sums and the pair counts are shared with this handle's data set (no second upload, no second
        device copy); the codes, lists and per-gene counts are built for the new masks.  Everything a created data set does
        works on it, with bit-identical results; either handle may be closed first."""
        Mtr = np.asfortranarray(train_indicator, dtype=np.uint8)
        Mte = np.asfortranarray(test_indicator, dtype=np.uint8)
        if Mtr.shape != (self.n, self.p) or Mte.shape != (self.n, self.p):
            raise InsiderError(_lib.ERR_ARG, "indicator shape must match data")
        lib = _lib.load()
        return self._derived(lambda out: lib.insider_hip_remask(self._h, _lib.ptr(Mtr, C.c_uint8), _lib.ptr(Mte, C.c_uint8), out))

    def set_folds(self, fold_id, n_folds=None):
        """Store the fold ids of the resident matrix on the device (insider_hip_set_folds): n x p, 0 = NA, 1..F = the fold
        the entry is held out in (``n_folds`` = F, default the largest id).  fold(f) then re-masks without any upload."""
        ids = np.asarray(fold_id)
        if ids.shape != (self.n, self.p):
            raise InsiderError(_lib.ERR_ARG, "fold_id shape must match data")
        lo, hi = (int(ids.min()), int(ids.max())) if ids.size else (0, 0)
        F = hi if n_folds is None else int(n_folds)
        if not 1 <= F <= 255:
            raise InsiderError(_lib.ERR_ARG, "the number of folds must be in 1..255")
        if lo < 0 or hi > F or not np.array_equal(ids, np.round(ids)):
            raise InsiderError(_lib.ERR_ARG, f"fold ids must be integers within 0..{F}")
        ids = np.asfortranarray(ids, dtype=np.uint8)
        _lib.check(_lib.load().insider_hip_set_folds(self._h, _lib.ptr(ids, C.c_uint8), F))
        self._fold_state()["F"] = F

    def fold(self, f):
        """The data set of fold f (1-based; insider_hip_remask_fold): test = the entries whose fold id is f, train = the
        entries of every other fold, NA = id 0.  As remask(), with the codes formed on the device from the resident ids."""
        F = self._fold_state().get("F")
        if F is None:
            raise InsiderError(_lib.ERR_ARG, "no fold ids set: call set_folds() first")
        if int(f) != f or not 1 <= int(f) <= F:
            raise InsiderError(_lib.ERR_ARG, f"fold must be in 1..{F}")
        lib = _lib.load()
        return self._derived(lambda out: lib.insider_hip_remask_fold(self._h, int(f), out))

    def set_option(self, name, value):
        _lib.check(_lib.load().insider_hip_set_option(self._h, name.encode(), float(value)))
        self.__dict__.setdefault("_options", {})[name] = float(value)      # (what tune(concurrent=k) re-applies to its clones)

    def set_shard(self, gene_offset, rank, world, allreduce=None):
        """allreduce(ptr:int, count:int, stream:int) -> None sums `count` doubles at device pointer `ptr` across ranks in
        place, ordered against the library's HIP stream `stream` (see include/insider_hip.h)."""
        if allreduce is None:
            cb = C.cast(None, _lib.ALLREDUCE_FN)
        else:
            def _tramp(_user, ptr, count, stream):
                try:
                    allreduce(int(ptr), int(count), int(stream or 0))
                    return 0
                except Exception as e:  # never unwind through the C frame
                    print(f"[insider_amd] all-reduce callback failed: {e!r}", flush=True)
                    return 1
            cb = _lib.ALLREDUCE_FN(_tramp)
        self._cb = cb
        _lib.check(_lib.load().insider_hip_set_shard(self._h, int(gene_offset), int(rank), int(world), cb, None))

    def _marshal(self, cfd_factors, column_factor, K, inc_continuous):
        """F-ordered float64 views (or copies) of the factors plus the pointer array the C ABI takes."""
        A = []
        shapes = [int(L) for L in self.n_levels] + ([self.m] if inc_continuous else [])
        if len(cfd_factors) != len(shapes):
            raise InsiderError(_lib.ERR_ARG, f"expected {len(shapes)} row-factor matrices, got {len(cfd_factors)}")
        for i, a in enumerate(cfd_factors):
            a = np.asarray(a)
            if a.shape != (shapes[i], K):
                raise InsiderError(_lib.ERR_ARG, f"cfd_factors[{i}] must be {shapes[i]} x {K}")
            A.append(a if (a.dtype == np.float64 and a.flags.f_contiguous) else _lib.f64(a).copy(order="F"))
        Cm = np.asarray(column_factor)
        if Cm.shape != (K, self.p):
            raise InsiderError(_lib.ERR_ARG, f"column_factor must be {K} x {self.p}")
        Cw = Cm if (Cm.dtype == np.float64 and Cm.flags.f_contiguous) else _lib.f64(Cm).copy(order="F")
        Aptrs = (C.POINTER(C.c_double) * len(A))(*[_lib.ptr(a) for a in A])
        return A, Cw, Aptrs

    def optimize_row(self, cfd_factors, column_factor, cov, lambda_=1.0, tuning=1, inc_continuous=0):
        """One row update of covariate `cov` (optimize_row, src/optimize.cpp:139-198 as called at :339); returns the
        new L_cov x K factor and updates cfd_factors[cov] in place when it is an F-ordered float64 array."""
        K = int(np.asarray(column_factor).shape[0])
        A, Cw, Aptrs = self._marshal(cfd_factors, column_factor, K, inc_continuous)
        _lib.check(_lib.load().insider_hip_optimize_row(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K, int(cov),
                                                        float(lambda_), int(tuning)))
        i = min(int(cov), len(A) - 1)
        if A[i] is not cfd_factors[i] and isinstance(cfd_factors[i], np.ndarray):
            cfd_factors[i][...] = A[i]
        return A[i].copy()

    def optimize_col(self, cfd_factors, column_factor, lambda_=1.0, alpha=0.1, tuning=1, tol=1e-5, seed=DEFAULT_SEED,
                     it=0, inc_continuous=0):
        """One column update (optimize_col, src/optimize.cpp:200-253 as called at :376); returns the new K x p factor
        and updates column_factor in place when it is an F-ordered float64 array."""
        K = int(np.asarray(column_factor).shape[0])
        A, Cw, Aptrs = self._marshal(cfd_factors, column_factor, K, inc_continuous)
        _lib.check(_lib.load().insider_hip_optimize_col(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                        float(lambda_), float(alpha), int(tuning), float(tol), int(seed),
                                                        int(it)))
        if Cw is not column_factor and isinstance(column_factor, np.ndarray):
            column_factor[...] = Cw
        return Cw.copy()

    def optimize(self, cfd_factors, column_factor, latent_dim, lambda1=1.0, lambda2=1.0, alpha=0.1, tuning=1,
                 global_tol=1e-10, sub_tol=1e-5, max_iter=10000, seed=DEFAULT_SEED, inc_continuous=0, traj_cap=4096,
                 copy=True):
        """copy=False: the returned factors ARE the (updated in place) arguments instead of copies of them — what the C ABI
        itself does; the reference's List holds copies (src/optimize.cpp:413), hence the default."""
        lib = _lib.load()
        K = int(latent_dim)
        A, Cw, Aptrs = self._marshal(cfd_factors, column_factor, K, inc_continuous)
        traj = np.full((traj_cap, _lib.TRAJ_STRIDE), np.nan)
        tr, te, lo = C.c_double(), C.c_double(), C.c_double()
        rows, iters = C.c_int(), C.c_int()
        _lib.check(lib.insider_hip_optimize(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K, float(lambda1),
                                            float(lambda2), float(alpha), int(tuning), float(global_tol),
                                            float(sub_tol), int(max_iter), int(seed), C.byref(tr), C.byref(te),
                                            C.byref(lo), _lib.ptr(traj), traj_cap, C.byref(rows), C.byref(iters)))
        # the reference mutates cfd_factors / column_factor in place AND returns copies (src/optimize.cpp:283-284,413)
        for src, dst in zip(A, cfd_factors):
            if src is not dst and isinstance(dst, np.ndarray):
                dst[...] = src
        if Cw is not column_factor and isinstance(column_factor, np.ndarray):
            column_factor[...] = Cw
        return dict(row_matrices={f"factor{i}": (a.copy() if copy else a) for i, a in enumerate(A)},
                    column_factor=Cw.copy() if copy else Cw,
                    train_rmse=tr.value, test_rmse=te.value, loss=lo.value, traj=traj[: rows.value].copy(),
                    iters=iters.value)

    def _posthoc_args(self, cfd_factors, column_factor, subtract, inc_continuous):
        """K, the marshalled factors and the int32 subtract flags of the post-hoc calls (ERR_ARG on any mismatch)."""
        if inc_continuous not in (0, 1):
            raise InsiderError(_lib.ERR_ARG, "The value of prarameter inc_continuous can only be 0 or 1.")
        K = int(np.asarray(column_factor).shape[0])
        nb = self.c + int(inc_continuous)
        sub = np.ones(nb, dtype=np.int32) if subtract is None else np.asarray(subtract).ravel()
        if sub.shape != (nb,):
            raise InsiderError(_lib.ERR_ARG, f"subtract must hold one flag per covariate block ({nb}), got {sub.size}")
        sub = np.ascontiguousarray(sub != 0, dtype=np.int32)
        A, Cw, Aptrs = self._marshal(cfd_factors, column_factor, K, inc_continuous)
        return K, A, Cw, Aptrs, sub

    def residual(self, cfd_factors, column_factor, subtract=None, rows=None, inc_continuous=0):
        """Residual rows of the resident X minus the contributions of the covariate blocks flagged in ``subtract``
        (insider_hip_residual; None = every block): an (rows) x p array.  ``rows`` = (begin, end) or a slice (default: all)."""
        K, A, Cw, Aptrs, sub = self._posthoc_args(cfd_factors, column_factor, subtract, inc_continuous)
        if rows is None:
            rb, re_ = 0, self.n
        elif isinstance(rows, slice):
            if rows.step not in (None, 1):
                raise InsiderError(_lib.ERR_ARG, "rows must be a contiguous window")
            rb, re_, _ = rows.indices(self.n)
        else:
            rb, re_ = (int(v) for v in rows)
        if not 0 <= rb <= re_ <= self.n:
            raise InsiderError(_lib.ERR_ARG, f"rows must satisfy 0 <= begin <= end <= n = {self.n}")
        out = np.empty((re_ - rb, self.p), dtype=np.float64, order="F")
        _lib.check(_lib.load().insider_hip_residual(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                    _lib.ptr(sub, C.c_int32), rb, re_, _lib.ptr(out)))
        return out

    def interaction_glm(self, cfd_factors, column_factor, group, subtract=None, inc_continuous=0, n_groups=None):
        """glm_interaction() on the resident data set (insider_hip_interaction_glm): ``group`` holds n ids in 0..G (0 = in
        no group; G = ``n_groups``, default the largest id).  Returns (coeff, se, dof): G x K, G x K and G, row g-1 for id g;
        empty groups give zero rows, latent dimensions whose row of C is zero give NaN columns."""
        K, A, Cw, Aptrs, sub = self._posthoc_args(cfd_factors, column_factor, subtract, inc_continuous)
        grp = np.asarray(group).ravel()
        if grp.shape != (self.n,):
            raise InsiderError(_lib.ERR_ARG, f"group must hold n = {self.n} ids")
        if not np.issubdtype(grp.dtype, np.integer):
            if not np.all(np.isfinite(grp)) or not np.array_equal(grp, np.round(grp)):
                raise InsiderError(_lib.ERR_ARG, "group ids must be integers")
        grp = np.ascontiguousarray(grp, dtype=np.int64)
        G = int(grp.max(initial=0)) if n_groups is None else int(n_groups)
        if G < 1:
            raise InsiderError(_lib.ERR_ARG, "at least one group id must be positive")
        if grp.min(initial=0) < 0 or grp.max(initial=0) > G:
            raise InsiderError(_lib.ERR_ARG, f"group ids must be within 0..{G}")
        grp = grp.astype(np.int32)
        coeff = np.empty((G, K), dtype=np.float64, order="F")
        se = np.empty((G, K), dtype=np.float64, order="F")
        dof = np.empty(G, dtype=np.float64)
        _lib.check(_lib.load().insider_hip_interaction_glm(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                           _lib.ptr(sub, C.c_int32), _lib.ptr(grp, C.c_int32), G,
                                                           _lib.ptr(coeff), _lib.ptr(se), _lib.ptr(dof)))
        return coeff, se, dof

    VD_ENTRIES = {"all": 0, "train": 1, "test": 2}

    def _entries_code(self, entries, inc_continuous):
        """The C ABI's code of ``entries``; ERR_ARG for a bad ``entries``, then for a bad ``inc_continuous``."""
        if entries not in self.VD_ENTRIES:
            raise InsiderError(_lib.ERR_ARG, f"entries must be one of {sorted(self.VD_ENTRIES)}, got {entries!r}")
        if inc_continuous not in (0, 1):
            raise InsiderError(_lib.ERR_ARG, "The value of prarameter inc_continuous can only be 0 or 1.")
        return self.VD_ENTRIES[entries]

    def _fit_args(self, cfd_factors, column_factor, entries, inc_continuous):
        """What every call on a whole fit takes: K, the marshalled factors and their pointers, the entries code and the
        number of covariate blocks (ERR_ARG for ``entries``, then ``inc_continuous``, then the factors' shapes)."""
        code = self._entries_code(entries, inc_continuous)
        K = int(np.asarray(column_factor).shape[0])
        A, Cw, Aptrs = self._marshal(cfd_factors, column_factor, K, inc_continuous)
        return K, A, Cw, Aptrs, code, self.c + int(inc_continuous)

    @staticmethod
    def _sums_record(out, nb):
        """The raw sums of a decomposition from its records ``out`` (one row of 4 + 3 nb per gene or sample)."""
        blk = out[:, 4:].reshape(out.shape[0], nb, 3)
        return dict(n=out[:, 0].copy(), sum_x=out[:, 1].copy(), sum_xx=out[:, 2].copy(), rss=out[:, 3].copy(),
                    sum_g=blk[:, :, 0].T.copy(), sum_gg=blk[:, :, 1].T.copy(), sum_rg=blk[:, :, 2].T.copy())

    def _center_scale(self, center, scale, names):
        """``center`` and ``scale`` as contiguous float64 vectors of length p (None stays None); ``names`` words the error."""
        ce = None if center is None else np.ascontiguousarray(np.asarray(center, dtype=np.float64).ravel())
        sc = None if scale is None else np.ascontiguousarray(np.asarray(scale, dtype=np.float64).ravel())
        if (ce is not None and ce.shape != (self.p,)) or (sc is not None and sc.shape != (self.p,)):
            raise InsiderError(_lib.ERR_ARG, f"{names} must hold p = {self.p} values")
        return ce, sc

    def variance_decomposition(self, cfd_factors, column_factor, entries="train", inc_continuous=0):
        """Per-gene sums of the variance decomposition (insider_hip_variance_decomposition) over the entries ``entries``
        ("all", "train": the handle's train bit, "test": its test bit) of every gene: a dict of ``n``, ``sum_x``,
        ``sum_xx``, ``rss`` (length p) and ``sum_g``, ``sum_gg``, ``sum_rg`` (B x p, block b = covariate b, then the
        continuous block).  posthoc.vd_derived() turns them into r2 / rmse / explained / drop_one."""
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        out = np.empty((self.p, 4 + 3 * nb), dtype=np.float64)
        _lib.check(_lib.load().insider_hip_variance_decomposition(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                                  code, _lib.ptr(out)))
        return self._sums_record(out, nb)

    def sample_decomposition(self, cfd_factors, column_factor, entries="train", inc_continuous=0):
        """Per-sample sums of the fit diagnostics (insider_hip_sample_decomposition): variance_decomposition() along the
        other axis, over the selected entries of every sample: a dict of ``n``, ``sum_x``, ``sum_xx``, ``rss`` (length n) and
        ``sum_g``, ``sum_gg``, ``sum_rg`` (B x n).  posthoc.vd_derived() turns them into r2 / rmse / explained / drop_one,
        posthoc.level_decomposition() sums them per level of a covariate first."""
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        out = np.empty((self.n, 4 + 3 * nb), dtype=np.float64)
        _lib.check(_lib.load().insider_hip_sample_decomposition(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                                code, _lib.ptr(out)))
        return self._sums_record(out, nb)

    def level_scores(self, cfd_factors, column_factor, cov, entries="train", candidates=None, inc_continuous=0):
        """Every sample scored against every level of the categorical covariate ``cov`` (0-based; insider_hip_level_scores):
        ``sse[i, l]`` is the residual sum of squares of sample i over its selected entries when its embedding for ``cov`` is
        replaced by candidate l — the rows of ``cfd_factors[cov]`` (``candidates`` None, L = its levels) or of ``candidates``
        (L x K: any embeddings in the latent space, e.g. for samples that carry a placeholder level).  A dict of ``sse``
        (n x L) and ``n`` (length n, the selected entries of every sample; a sample without any has a row of zeros).
        posthoc.ls_derived() turns them into best / second / margin / flagged / confusion.  The device sums the expanded
        form sum d^2 - 2 sum d g + sum g^2: sse is never negative (a sum that cancels below 0 is returned as 0), but a value
        far below its row's other entries holds the rounding of those three sums, not digits of its own.
        A sample's own level was fitted WITH that sample: on ``entries="train"`` the assigned level is favoured, most for
        levels with few samples (a level with one sample fits itself); on a tuning handle ``entries="test"`` scores on
        entries no embedding has seen.  The call reports and corrects nothing."""
        self._entries_code(entries, inc_continuous)   # (reported before cov; the factors' shapes after it, as ever)
        if not isinstance(cov, (int, np.integer)) or isinstance(cov, bool) or not 0 <= cov < self.c:
            raise InsiderError(_lib.ERR_ARG, f"cov must be a categorical covariate in 0..{self.c - 1}, got {cov!r}")
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        if candidates is None:
            cand, L = None, int(self.n_levels[int(cov)])
        else:
            cand = np.asarray(candidates)
            if cand.ndim != 2 or cand.shape[0] < 1 or cand.shape[1] != K:
                raise InsiderError(_lib.ERR_ARG, f"candidates must be L x {K} with L >= 1")
            cand = _lib.f64(cand)
            L = cand.shape[0]
        sse = np.empty((self.n, L), dtype=np.float64, order="F")
        cnt = np.empty(self.n, dtype=np.float64)
        _lib.check(_lib.load().insider_hip_level_scores(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                        code, int(cov),
                                                        None if cand is None else _lib.ptr(cand), 0 if cand is None else L,
                                                        _lib.ptr(sse), _lib.ptr(cnt)))
        return dict(sse=sse, n=cnt)

    def factor_decomposition(self, cfd_factors, column_factor, entries="train", inc_continuous=0):
        """Per-gene sums of the per-factor decomposition (insider_hip_factor_decomposition) over the entries ``entries`` of
        every gene: variance_decomposition() split along the K latent factors.  A dict of ``n``, ``sum_x``, ``sum_xx``,
        ``rss`` (length p) and ``sum_h``, ``sum_hh``, ``sum_rh`` ((B + 1) x K x p: block b = covariate b, then the continuous
        block, then the total, whose embedding is the row factor).  posthoc.fd_derived() turns them into r2 / rmse /
        explained / drop_one per (block, factor, gene), posthoc.factor_summary() pools the genes."""
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        out = np.empty((self.p, 4 + 3 * (nb + 1) * K), dtype=np.float64)
        _lib.check(_lib.load().insider_hip_factor_decomposition(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                                code, _lib.ptr(out)))
        blk = out[:, 4:].reshape(self.p, nb + 1, K, 3)
        return dict(n=out[:, 0].copy(), sum_x=out[:, 1].copy(), sum_xx=out[:, 2].copy(), rss=out[:, 3].copy(),
                    sum_h=blk[..., 0].transpose(1, 2, 0).copy(), sum_hh=blk[..., 1].transpose(1, 2, 0).copy(),
                    sum_rh=blk[..., 2].transpose(1, 2, 0).copy())

    def residual_products(self, cfd_factors, column_factor, Q, entries="train", center=None, scale=None, inc_continuous=0,
                          want_y=True):
        """The masked, standardised residual of a fitted model applied to a block of vectors
        (insider_hip_residual_products): with r = (x - f - center[j]) / scale[j] on the entries ``entries`` and 0 elsewhere
        (``center`` None = 0, ``scale`` None = 1, each of length p; a gene whose scale is not finite or not > 0 is an all-zero
        column) and ``Q`` n x q (q in 1..64, finite), a dict of ``Z`` = R'Q (p x q), ``Y`` = R Z (n x q; None with
        ``want_y`` False: the forward pass is skipped) and ``rss`` (p, each gene's sum of r^2).  R never exists: each product is
        one streaming pass over the resident X.  posthoc.residual_components() iterates it to the leading singular directions
        of R."""
        self._entries_code(entries, inc_continuous)   # (reported before Q; the factors' shapes after it, as ever)
        Qm = np.asarray(Q, dtype=np.float64)
        if Qm.ndim == 1:
            Qm = Qm.reshape(-1, 1)
        if Qm.ndim != 2 or Qm.shape[0] != self.n or not 1 <= Qm.shape[1] <= 64:
            raise InsiderError(_lib.ERR_ARG, f"Q must be n x q with n = {self.n} and q in 1..64")
        if not np.all(np.isfinite(Qm)):
            raise InsiderError(_lib.ERR_ARG, "Q holds a value that is not finite")
        Qm = _lib.f64(Qm)
        q = Qm.shape[1]
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        ce, sc = self._center_scale(center, scale, "center and scale")
        Z = np.empty((self.p, q), dtype=np.float64, order="F")
        Y = np.empty((self.n, q), dtype=np.float64, order="F") if want_y else None
        rss = np.empty(self.p, dtype=np.float64)
        _lib.check(_lib.load().insider_hip_residual_products(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                             code,
                                                             None if ce is None else _lib.ptr(ce),
                                                             None if sc is None else _lib.ptr(sc), _lib.ptr(Qm), q,
                                                             _lib.ptr(Z), None if Y is None else _lib.ptr(Y), _lib.ptr(rss)))
        return dict(Z=Z, Y=Y, rss=rss)

    COEXPR_AXES = {"genes": 0, "samples": 1}

    def coexpression(self, cfd_factors, column_factor, axis="genes", k=10, entries="train", center=None, scale=None,
                     inc_continuous=0):
        """Residual co-expression (insider_hip_coexpression): the ``k`` most correlated partners of every gene
        (``axis="genes"``: N = p vectors, correlated over the samples) or of every sample (``axis="samples"``: N = n, over the
        genes) in the working residual of residual_products(): r = (x - f - center[j]) / scale[j] on the entries ``entries``
        and 0 elsewhere (``center`` None = 0, ``scale`` None = 1; a gene with a bad scale is an all-zero column).  A vector is
        centred by its mean over its selected entries (the unselected ones stay 0) and divided by the root of its centred sum
        of squares; one with fewer than two selected entries or no variance is dead: nobody's partner, a row of open slots.
        The score is the plain sum of products over the whole depth.  With a full selection this is Pearson's r; with missing
        entries it is the ZERO-FILLED correlation (|score| <= 1, shrinking with missingness), NOT the pairwise-complete one:
        that is coexpression_pairwise().
        -> dict(index=(N, k) int32, score=(N, k) float64): descending score, equal scores by ascending index, never the
        vector itself, -1 / NaN in open slots.  The standardised residual is staged once on the device (about 8 n p bytes,
        freed before the call returns); the N x N matrix never exists."""
        self._entries_code(entries, inc_continuous)   # (reported before axis and k; the factors' shapes after them, as ever)
        if axis not in self.COEXPR_AXES:
            raise InsiderError(_lib.ERR_ARG, f"axis must be one of {sorted(self.COEXPR_AXES)}, got {axis!r}")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NEIGHBOR_MAX_K:
            raise InsiderError(_lib.ERR_ARG, f"k must be an integer in 1..{NEIGHBOR_MAX_K}")
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        ce, sc = self._center_scale(center, scale, "center and scale")
        N = self.p if axis == "genes" else self.n
        index = np.full((N, int(k)), -1, dtype=np.int32)
        score = np.full((N, int(k)), np.nan)
        _lib.check(_lib.load().insider_hip_coexpression(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K, code,
                                                        None if ce is None else _lib.ptr(ce),
                                                        None if sc is None else _lib.ptr(sc), self.COEXPR_AXES[axis], int(k),
                                                        _lib.ptr(index, C.c_int32), _lib.ptr(score)))
        return dict(index=index, score=score)

    def coexpression_pairwise(self, cfd_factors, column_factor, axis="genes", k=10, min_overlap=None, entries="train",
                              center=None, scale=None, inc_continuous=0):
        """Pairwise-complete residual co-expression (insider_hip_coexpression_pairwise): coexpression() with the score of a
        pair taken over the entries selected in BOTH vectors, which is Pearson's r of the pair whatever is missing.  The
        residual, ``axis``, ``entries``, ``center`` / ``scale`` and the dead vectors are those of coexpression(); the score,
        the eligibility of a pair and ``min_overlap`` (None = max(3, ceil(depth / 4)), depth = n for genes, p for samples)
        are those of gram_topk_pairwise().  -> dict(index=(N, k) int32, score=(N, k) float64, overlap=(N, k) int32: the
        number of jointly selected entries of the pair): descending score, equal scores by ascending index, never the vector
        itself, -1 / NaN / -1 in open slots."""
        self._entries_code(entries, inc_continuous)   # (reported before axis and k; the factors' shapes after them, as ever)
        if axis not in self.COEXPR_AXES:
            raise InsiderError(_lib.ERR_ARG, f"axis must be one of {sorted(self.COEXPR_AXES)}, got {axis!r}")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NEIGHBOR_MAX_K:
            raise InsiderError(_lib.ERR_ARG, f"k must be an integer in 1..{NEIGHBOR_MAX_K}")
        min_overlap = pairwise_min_overlap(min_overlap, self.n if axis == "genes" else self.p)
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        ce, sc = self._center_scale(center, scale, "center and scale")
        N = self.p if axis == "genes" else self.n
        index = np.full((N, int(k)), -1, dtype=np.int32)
        score = np.full((N, int(k)), np.nan)
        overlap = np.full((N, int(k)), -1, dtype=np.int32)
        _lib.check(_lib.load().insider_hip_coexpression_pairwise(
            self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K, code, None if ce is None else _lib.ptr(ce),
            None if sc is None else _lib.ptr(sc), self.COEXPR_AXES[axis], min_overlap, int(k), _lib.ptr(index, C.c_int32),
            _lib.ptr(score), _lib.ptr(overlap, C.c_int32)))
        return dict(index=index, score=score, overlap=overlap)

    def outliers(self, cfd_factors, column_factor, scale, center=None, threshold=3.0, entries="train", inc_continuous=0,
                 cap=None):
        """The aberrant entries of a fitted model (insider_hip_outliers): the entries ``entries`` whose standardised residual
        z = (x - f - center[j]) / scale[j] has |z| >= ``threshold`` (``scale``, ``center``: length p, center None = 0; a gene
        whose scale is not finite or not > 0 gives no call).  A dict of ``rows``, ``cols`` (0-based sample and gene, int32),
        ``z`` (the calls in ascending gene, then ascending sample), ``total`` (the number of calls) and the complete counts
        ``gene_low``, ``gene_high`` (p), ``sample_low``, ``sample_high`` (n).  ``cap`` bounds the list: None = one call with a
        capacity of max(2^20, n p / 64) and, when ``total`` exceeds it, a second one with cap = total (the whole list); an
        integer = the first ``cap`` calls (compare ``total`` with it); 0 = counts only.
        posthoc.residual_center_scale() derives center and scale from a variance-decomposition record."""
        self._entries_code(entries, inc_continuous)   # (reported before scale and cap; the factors' shapes after them)
        if scale is None:
            raise InsiderError(_lib.ERR_ARG, "scale is required")
        if cap is not None and (int(cap) != cap or cap < 0):
            raise InsiderError(_lib.ERR_ARG, "cap must be None or an integer >= 0")
        K, A, Cw, Aptrs, code, nb = self._fit_args(cfd_factors, column_factor, entries, inc_continuous)
        ce, sc = self._center_scale(center, scale, "scale and center")
        gene = np.empty((self.p, 2), dtype=np.int32)
        samp = np.empty((self.n, 2), dtype=np.int32)
        total = C.c_int64()
        lib = _lib.load()

        def call(capacity):
            rows, cols = np.empty(capacity, dtype=np.int32), np.empty(capacity, dtype=np.int32)
            z = np.empty(capacity, dtype=np.float64)
            lists = (_lib.ptr(rows, C.c_int32), _lib.ptr(cols, C.c_int32), _lib.ptr(z)) if capacity else (None, None, None)
            _lib.check(lib.insider_hip_outliers(self._h, Aptrs, _lib.ptr(Cw), int(inc_continuous), K,
                                                code, None if ce is None else _lib.ptr(ce), _lib.ptr(sc),
                                                float(threshold), capacity, *lists, C.byref(total),
                                                _lib.ptr(gene, C.c_int32), _lib.ptr(samp, C.c_int32)))
            return rows, cols, z

        capacity = max(1 << 20, self.n * self.p // 64) if cap is None else int(cap)
        rows, cols, z = call(capacity)
        if cap is None and total.value > capacity:
            capacity = int(total.value)
            rows, cols, z = call(capacity)
        k = min(int(total.value), capacity)
        return dict(rows=rows[:k].copy(), cols=cols[:k].copy(), z=z[:k].copy(), total=int(total.value),
                    gene_low=gene[:, 0].copy(), gene_high=gene[:, 1].copy(), sample_low=samp[:, 0].copy(),
                    sample_high=samp[:, 1].copy())

    def masked_gram_cols(self, R):
        R = _lib.f64(R)
        K = R.shape[1]
        G = np.zeros((self.p, K, K))
        q = np.zeros((self.p, K))
        _lib.check(_lib.load().insider_hip_masked_gram_cols(self._h, _lib.ptr(R), K, _lib.ptr(G), _lib.ptr(q)))
        return G, q

    def col_stats(self, cfd_factors, inc_continuous=0):
        """The column-side statistics the column solve reads (insider_hip_col_stats), from the row factors alone: per gene j
        the training Gram G[j] = R_t'R_t, q[j] = R_t'x_t over its training entries t, and ss[j], the sum of x^2 over the
        others (held out and NA).  R = sum_i Z_i A_i (+ Z_c A_c with inc_continuous); the statistics kernel is the one the
        handle's options pick for a fit (info "col_stats_kernel")."""
        K = int(np.asarray(cfd_factors[0]).shape[1])
        A, _, Aptrs = self._marshal(cfd_factors, np.zeros((K, self.p), order="F"), K, inc_continuous)
        G = np.zeros((self.p, K, K))
        q = np.zeros((self.p, K))
        ss = np.zeros(self.p)
        _lib.check(_lib.load().insider_hip_col_stats(self._h, Aptrs, int(inc_continuous), K, _lib.ptr(G), _lib.ptr(q),
                                                     _lib.ptr(ss)))
        return G, q, ss

    def masked_gram_rows(self, Cmat):
        Cmat = _lib.f64(Cmat)
        K = Cmat.shape[0]
        H = np.zeros((self.n, K, K))
        b = np.zeros((self.n, K))
        _lib.check(_lib.load().insider_hip_masked_gram_rows(self._h, _lib.ptr(Cmat), K, _lib.ptr(H), _lib.ptr(b)))
        return H, b

    def profile(self):
        out = np.zeros(12)
        _lib.check(_lib.load().insider_hip_get_profile(self._h, _lib.ptr(out)))
        return dict(col_stats_launches=int(out[0]), col_stats_ms=out[1], row_stats_launches=int(out[2]),
                    row_stats_ms=out[3], cd_launches=int(out[4]), cd_ms=out[5], test_launches=int(out[6]),
                    test_ms=out[7], wall_ms=out[8], iters=int(out[9]), sweeps=int(out[10]),
                    col_factored=bool(int(out[11]) & 1), row_merged=bool(int(out[11]) & 2),
                    col_pair=bool(int(out[11]) & 4))

    def info(self, name):
        """A fact about the handle (insider_hip_get_info): "col_stats_path", "col_mfma_per_gene", ...; of its resident data
        set: "ds_ldn", "ds_SLP", "ds_no_na", "ds_merged", "ds_cf_pair_ok", "ds_nitems:<i>", ... and "ds_bytes:<name>[:<i>]",
        the size of a data-set array (0: this data set did not build it)."""
        out = C.c_double()
        _lib.check(_lib.load().insider_hip_get_info(self._h, name.encode(), C.byref(out)))
        return out.value

    def array(self, name, dtype=np.uint8):
        """A device array of the resident data set as it lies in memory (insider_hip_get_array "ds:<name>" or
        "ds:<name>:<i>"; include/insider_hip.h lists the names, layouts and element types), or None when this data set did not
        build it.  "cf_geometry" is the static part of the factored statistics' arguments (int32), "names" the list of names
        (bytes).  Diagnostics: the handle's stream is synchronised and the array copied; nothing is written."""
        nbytes = int(self.info("ds_bytes:" + name))
        if nbytes == 0:
            return None
        dtype = np.dtype(dtype)
        if nbytes % dtype.itemsize:
            raise InsiderError(_lib.ERR_ARG, f"{name}: {nbytes} bytes are no whole number of {dtype} elements")
        out = np.zeros(nbytes // dtype.itemsize, dtype=dtype)
        _lib.check(_lib.load().insider_hip_get_array(self._h, ("ds:" + name).encode(), out.ctypes.data_as(C.c_void_p), nbytes))
        return out

    def comm_init(self, unique_id, rank, world):
        """Join the in-library RCCL communicator (insider_hip_comm_init) after set_shard(); collective over all ranks."""
        buf = (C.c_char * _lib.COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _lib.check(_lib.load().insider_hip_comm_init(self._h, buf, int(rank), int(world)))

    def debug_array(self, name):
        """An internal per-gene int32 array (insider_hip_get_array): "cd_key0", "cd_key1", "gene_perm"."""
        out = np.zeros(self.p, dtype=np.int32)
        _lib.check(_lib.load().insider_hip_get_array(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def sweeps(self):
        """Per-gene sweep counts of the last column update."""
        out = np.zeros(self.p, dtype=np.int32)
        _lib.check(_lib.load().insider_hip_get_sweeps(self._h, _lib.ptr(out, C.c_int32)))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().insider_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------
# operator level — R/RcppExports.R:4-22
# ---------------------------------------------------------------------------------------------------------------
def optimize(data, cfd_factors, column_factor, cfd_indicators, ctns_confounder, train_indicator, test_indicator,
             inc_continuous, latent_dim, lambda1=1.0, lambda2=1.0, alpha=0.1, tuning=1, global_tol=1e-10, sub_tol=1e-5,
             max_iter=10000, seed=DEFAULT_SEED, device=0):
    """optimize() of R/RcppExports.R:20-22 (src/optimize.cpp:255-422): one-shot upload + fit, through
    ``insider_hip_optimize_oneshot_ex`` — the symbol r/insider_hip_shim.c binds for the R package.

    Returns dict(row_matrices, column_factor, train_rmse, test_rmse, loss) like the reference's List (:417-421);
    float64 Fortran-ordered ``cfd_factors`` / ``column_factor`` arrays are also updated in place (:283-284).
    """
    if tuning not in (0, 1):
        raise InsiderError(_lib.ERR_ARG, "Parameter tuning should be either 0 or 1!")
    if inc_continuous not in (0, 1):
        raise InsiderError(_lib.ERR_ARG, "The value of prarameter inc_continuous can only be 0 or 1.")
    lib = _lib.load()
    X = _lib.f64(data)
    n, p = X.shape
    K = int(latent_dim)
    lev = np.asfortranarray(np.asarray(cfd_indicators).reshape(n, -1), dtype=np.int32)
    c = lev.shape[1]
    n_levels = np.ascontiguousarray([len(np.unique(lev[:, i])) for i in range(c)], dtype=np.int32)   # R/insider.R:107
    Mtr = np.asfortranarray(train_indicator, dtype=np.uint8)
    Mte = np.asfortranarray(test_indicator, dtype=np.uint8)
    if Mtr.shape != (n, p) or Mte.shape != (n, p):
        raise InsiderError(_lib.ERR_ARG, "indicator shape must match data")
    if inc_continuous == 1:
        if ctns_confounder is None:
            raise InsiderError(_lib.ERR_ARG, "inc_continuous = 1 needs ctns_confounder (n x m)")
        Z = _lib.f64(np.asarray(ctns_confounder, dtype=np.float64).reshape(n, -1))
        m, zp = Z.shape[1], _lib.ptr(Z)
    else:
        m, zp = 0, None
    shapes = [int(L) for L in n_levels] + ([m] if inc_continuous else [])
    if len(cfd_factors) != len(shapes):
        raise InsiderError(_lib.ERR_ARG, f"expected {len(shapes)} row-factor matrices, got {len(cfd_factors)}")
    A = []
    for i, a in enumerate(cfd_factors):
        a = np.asarray(a)
        if a.shape != (shapes[i], K):
            raise InsiderError(_lib.ERR_ARG, f"cfd_factors[{i}] must be {shapes[i]} x {K}")
        A.append(a if (a.dtype == np.float64 and a.flags.f_contiguous) else _lib.f64(a).copy(order="F"))
    Cm = np.asarray(column_factor)
    if Cm.shape != (K, p):
        raise InsiderError(_lib.ERR_ARG, f"column_factor must be {K} x {p}")
    Cw = Cm if (Cm.dtype == np.float64 and Cm.flags.f_contiguous) else _lib.f64(Cm).copy(order="F")
    Aptrs = (C.POINTER(C.c_double) * len(A))(*[_lib.ptr(a) for a in A])
    tr, te, lo = C.c_double(), C.c_double(), C.c_double()
    _lib.check(lib.insider_hip_optimize_oneshot_ex(_lib.ptr(X), n, p, Aptrs, _lib.ptr(Cw), _lib.ptr(lev, C.c_int32), c,
                                                   _lib.ptr(n_levels, C.c_int32), zp, m, _lib.ptr(Mtr, C.c_uint8),
                                                   _lib.ptr(Mte, C.c_uint8), int(inc_continuous), K, float(lambda1),
                                                   float(lambda2), float(alpha), int(tuning), float(global_tol),
                                                   float(sub_tol), int(max_iter), int(seed), int(device), C.byref(tr),
                                                   C.byref(te), C.byref(lo)))
    for src, dst in zip(A, cfd_factors):
        if src is not dst and isinstance(dst, np.ndarray):
            dst[...] = src
    if Cw is not column_factor and isinstance(column_factor, np.ndarray):
        column_factor[...] = Cw
    return dict(row_matrices={f"factor{i}": a.copy() for i, a in enumerate(A)}, column_factor=Cw.copy(),
                train_rmse=tr.value, test_rmse=te.value, loss=lo.value)


def strong_coordinate_descent(X, y, wstart, lambda_, alpha, XtX=None, Xty=None, tol=1e-5, seed=DEFAULT_SEED, it=0,
                              order_mode=0, max_sweeps=1 << 24, device=0, return_sweeps=False):
    """strong_coordinate_descent() of R/RcppExports.R:8-10 (src/coordinate_descent.cpp:56-127).

    Single problem (the reference's signature): ``X`` m x K, ``y`` m; ``XtX`` / ``Xty`` are formed on the device as X'X
    and X'y when they are not given (``insider_hip_strong_cd_xy``).  Batched use: XtX of shape (B, K, K), Xty / wstart
    of shape (B, K); X and y are then not read (covariance form).
    """
    w = np.ascontiguousarray(wstart, dtype=np.float64)
    if XtX is None or Xty is None or np.ndim(Xty) == 1:
        if X is None and (XtX is None or Xty is None):
            raise InsiderError(_lib.ERR_ARG, "pass (X, y), or XtX and Xty")
        K = int(w.shape[0])
        Xf = _lib.f64(X) if X is not None else None
        yf = np.ascontiguousarray(y, dtype=np.float64) if y is not None else None
        if Xf is not None and (Xf.ndim != 2 or Xf.shape[1] != K or yf is None or yf.shape != (Xf.shape[0],)):
            raise InsiderError(_lib.ERR_ARG, "X must be m x K and y of length m")
        G = _lib.f64(XtX) if XtX is not None else None
        q = np.ascontiguousarray(Xty, dtype=np.float64) if Xty is not None else None
        if (G is not None and G.shape != (K, K)) or (q is not None and q.shape != (K,)):
            raise InsiderError(_lib.ERR_ARG, "XtX must be K x K and Xty of length K")
        beta = np.zeros(K)
        sw = np.zeros(1, dtype=np.int32)
        _lib.check(_lib.load().insider_hip_strong_cd_xy(
            _lib.ptr(Xf) if Xf is not None else None, _lib.ptr(yf) if yf is not None else None,
            int(Xf.shape[0]) if Xf is not None else 0, K, _lib.ptr(w), float(lambda_), float(alpha),
            _lib.ptr(G) if G is not None else None, _lib.ptr(q) if q is not None else None, float(tol), int(seed), int(it),
            int(order_mode), int(max_sweeps), int(device), _lib.ptr(beta), _lib.ptr(sw, C.c_int32)))
        return (beta, int(sw[0])) if return_sweeps else beta
    G = np.ascontiguousarray(XtX, dtype=np.float64)
    q = np.ascontiguousarray(Xty, dtype=np.float64)
    B, K = q.shape
    if G.shape != (B, K, K) or w.shape != (B, K):
        raise InsiderError(_lib.ERR_ARG, "XtX must be (B,K,K) and Xty/wstart (B,K)")
    beta = np.zeros((B, K))
    sw = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.load().insider_hip_strong_cd(_lib.ptr(G), _lib.ptr(q), _lib.ptr(w), K, B, float(lambda_),
                                                 float(alpha), float(tol), int(seed), int(it),
                                                 int(order_mode), int(max_sweeps), int(device), _lib.ptr(beta),
                                                 _lib.ptr(sw, C.c_int32)))
    return (beta, sw) if return_sweeps else beta


def optimize_continuous_v2(data, indicator, updating_factor, c_factor, updating_confd, gram, lambda_, tuning, device=0):
    """optimize_continuous_v2() of R/RcppExports.R:16-18 (src/optimize.cpp:76-137), the reference's eight arguments, through
    ``insider_hip_optimize_continuous_v2``: the update of one continuous covariate's K-vector against the matrix ``data``
    (n x p; inside optimize() the residual with this column's contribution added back, :344-345).  ``updating_factor`` is
    updated IN PLACE when it is a float64 array (the reference's ``rowvec&``) and returned.  ``indicator`` is read only when
    tuning = 1, ``gram`` only when tuning = 0 — as in the reference."""
    if tuning not in (0, 1):
        raise InsiderError(_lib.ERR_ARG, "Parameter tuning should be either 0 or 1!")
    D = _lib.f64(data)
    n, p = D.shape
    Cm = _lib.f64(c_factor)
    K = Cm.shape[0]
    z = np.ascontiguousarray(np.asarray(updating_confd, dtype=np.float64).reshape(-1))
    u = np.ascontiguousarray(np.asarray(updating_factor, dtype=np.float64).reshape(-1)).copy()
    if Cm.shape != (K, p) or z.shape != (n,) or u.shape != (K,):
        raise InsiderError(_lib.ERR_ARG, "c_factor must be K x p, updating_confd of length n, updating_factor of length K")
    M = g = None
    if tuning == 1:
        M = np.asfortranarray(np.asarray(indicator) != 0, dtype=np.uint8)
        if M.shape != (n, p):
            raise InsiderError(_lib.ERR_ARG, "indicator shape must match data")
    else:
        g = _lib.f64(gram)
        if g.shape != (K, K):
            raise InsiderError(_lib.ERR_ARG, "gram must be K x K")
    _lib.check(_lib.load().insider_hip_optimize_continuous_v2(
        _lib.ptr(D), n, p, _lib.ptr(M, C.c_uint8) if M is not None else None, _lib.ptr(u), _lib.ptr(Cm), K, _lib.ptr(z),
        _lib.ptr(g) if g is not None else None, float(lambda_), int(tuning), int(device)))
    if isinstance(updating_factor, np.ndarray) and updating_factor.dtype == np.float64:
        np.copyto(updating_factor, u.reshape(updating_factor.shape))   # (also through a non-contiguous view)
    return u


SOLVE_FORMS = {"batch": 0, "level": 1}


def solve_sympd(A, b, device=0, return_route=False, lambda_=0.0, form="batch"):
    """solve(A + lambda I, b, solve_opts::likely_sympd) (src/optimize.cpp:175,190,226,240), batched: A (B, K, K) or (K, K),
    b (B, K) or (K,).  Cholesky first, Gaussian elimination with partial pivoting when the matrix is not positive definite;
    ``lambda_`` is added to the diagonal on the device.  ``form``: "batch" = the stand-alone kernel (K <= 64), "level" = the
    fit's own level solve on every system packed as a level equation record (K <= 63, symmetric A only).  A singular system
    raises InsiderError(ERR_SOLVE); the error carries ``x`` and ``route`` of the whole batch as attributes."""
    if form not in SOLVE_FORMS:
        raise InsiderError(_lib.ERR_ARG, f"form must be one of {sorted(SOLVE_FORMS)}")
    Am = np.asarray(A, dtype=np.float64)
    bm = np.asarray(b, dtype=np.float64)
    single = Am.ndim == 2
    if single:
        Am, bm = Am[None], bm[None]
    B, K = bm.shape
    if Am.shape != (B, K, K):
        raise InsiderError(_lib.ERR_ARG, "A must be (B,K,K) and b (B,K)")
    Af = np.ascontiguousarray(np.transpose(Am, (0, 2, 1)))     # every block column-major
    bf = np.ascontiguousarray(bm)
    x = np.zeros((B, K))
    route = np.zeros(B, dtype=np.int32)
    try:
        _lib.check(_lib.load().insider_hip_solve_sympd_form(_lib.ptr(Af), _lib.ptr(bf), K, B, float(lambda_),
                                                            SOLVE_FORMS[form], int(device), _lib.ptr(x),
                                                            _lib.ptr(route, C.c_int32)))
    except InsiderError as e:
        if e.status == _lib.ERR_SOLVE:
            e.x, e.route = x, route
        raise
    if single:
        x, route = x[0], int(route[0])
    return (x, route) if return_route else x


NEIGHBOR_METRICS = {"cosine": 0, "dot": 1}
NEIGHBOR_MAX_K = 64


def neighbor_args(query, base, k, metric, exclude_self):
    """The checked arguments of neighbors() / posthoc.neighbors_host(): (Q, B, k, metric code, self_offset), Q and B
    column-major float64 (B is Q itself when ``base`` is None).  Shape, metric, k and window errors raise
    InsiderError(ERR_ARG)."""
    Q = _lib.f64(query)
    if Q.ndim != 2:
        raise InsiderError(_lib.ERR_ARG, "query must be a K x nq array")
    if base is None:
        B = Q
        if exclude_self is None:
            exclude_self = 0
    else:
        B = _lib.f64(base)
        if B.ndim != 2 or B.shape[0] != Q.shape[0]:
            raise InsiderError(_lib.ERR_ARG, "base must be a K x nb array with the K of query")
    if not 1 <= Q.shape[0] <= _lib.MAX_K:
        raise InsiderError(_lib.ERR_ARG, f"K must be in 1..{_lib.MAX_K}")
    if B.shape[1] < 1:
        raise InsiderError(_lib.ERR_ARG, "base must hold at least one column")
    if metric not in NEIGHBOR_METRICS:
        raise InsiderError(_lib.ERR_ARG, f"metric must be one of {sorted(NEIGHBOR_METRICS)}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NEIGHBOR_MAX_K:
        raise InsiderError(_lib.ERR_ARG, f"k must be an integer in 1..{NEIGHBOR_MAX_K}")
    if exclude_self is None or exclude_self is False:
        off = -1
    elif isinstance(exclude_self, (bool, float)) or not isinstance(exclude_self, (int, np.integer)):
        raise InsiderError(_lib.ERR_ARG, "exclude_self must be None, False or a window start (an integer >= 0)")
    else:
        off = int(exclude_self)
        if off < 0 or off + Q.shape[1] > B.shape[1]:
            raise InsiderError(_lib.ERR_ARG, "exclude_self: the window start + nq must lie within the base")
    return Q, B, int(k), NEIGHBOR_METRICS[metric], off


def neighbors(query, base=None, k=10, metric="cosine", exclude_self=None, device=0):
    """The k nearest base columns of every query column on the device (insider_hip_neighbors).  ``query`` (K x nq) and
    ``base`` (K x nb) hold one embedding per column, as column_factor does; base=None: the base is the queries and a query
    never returns itself.  metric "cosine" or "dot" (raw Euclidean distance is not offered: on unit-normalised columns it
    orders as cosine).  exclude_self: None / False = no exclusion, s >= 0 = the queries are base[:, s : s + nq] and query i
    never returns base column s + i.  -> dict(index=(nq, k) int32, score=(nq, k) float64): descending score, equal scores by
    ascending base index; a row with fewer than k eligible candidates ends in -1 / NaN (under cosine a zero column is
    nobody's neighbour and has none)."""
    Q, B, k, code, off = neighbor_args(query, base, k, metric, exclude_self)
    K, nq = Q.shape
    index = np.full((nq, k), -1, dtype=np.int32)
    score = np.full((nq, k), np.nan)
    if nq:
        if off >= 0 and (B is Q or np.array_equal(B[:, off:off + nq], Q)):
            # the self call: hand the library the window of B itself, so the matrix is checked and uploaded once
            qp = C.cast(B.ctypes.data + off * K * 8, C.POINTER(C.c_double))
        else:
            qp = _lib.ptr(Q)
        _lib.check(_lib.load().insider_hip_neighbors(qp, nq, _lib.ptr(B), B.shape[1], K, code, k, off, int(device),
                                                     _lib.ptr(index, C.c_int32), _lib.ptr(score)))
    return dict(index=index, score=score)


GRAM_METRICS = {"correlation": 0, "cosine": 1, "dot": 2}
# insider_amd/csrc/insider_coexpr.hpp: the queries a block of k_cx_topk owns (CX_QB), the base vectors it takes per step (CX_BG)
# and the depth chunk it stages (CX_DC): the sizes at which the kernel changes path
CX_QB = 64
CX_BG = 64
CX_DC = 32


def gram_topk_args(V, k, metric, first, count):
    """The checked arguments of gram_topk() / posthoc.gram_topk_host(): (V, k, metric code, first, count), V column-major
    float64 (depth x N).  Shape, metric, k, window and non-finite errors raise InsiderError(ERR_ARG)."""
    V = _lib.f64(V)
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1:
        raise InsiderError(_lib.ERR_ARG, "V must be a depth x N array with depth >= 1 and N >= 1")
    N = V.shape[1]
    if N > 2 ** 31 - 1:
        raise InsiderError(_lib.ERR_ARG, "N must be < 2^31")
    if metric not in GRAM_METRICS:
        raise InsiderError(_lib.ERR_ARG, f"metric must be one of {sorted(GRAM_METRICS)}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NEIGHBOR_MAX_K:
        raise InsiderError(_lib.ERR_ARG, f"k must be an integer in 1..{NEIGHBOR_MAX_K}")
    if count is None:
        count = N - first if isinstance(first, (int, np.integer)) and not isinstance(first, bool) else count
    for name, v in (("first", first), ("count", count)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise InsiderError(_lib.ERR_ARG, f"{name} must be an integer >= 0")
    if first + count > N:
        raise InsiderError(_lib.ERR_ARG, "the window first + count must lie within the N vectors")
    if not np.all(np.isfinite(V)):
        raise InsiderError(_lib.ERR_ARG, "V holds a value that is not finite")
    return V, int(k), GRAM_METRICS[metric], int(first), int(count)


def gram_topk(V, k=10, metric="correlation", first=0, count=None, device=0):
    """The k best partners of deep vectors on the device (insider_hip_gram_topk).  ``V`` (depth x N) holds one vector per
    column; the depth is not limited (neighbors() keeps K <= 63 in registers, this streams it).  metric "correlation" (each
    vector centred by its mean and divided by the root of its centred sum of squares), "cosine" (divided by the root of its
    sum of squares) or "dot" (as given); under the first two a vector without variance / norm is dead: nobody's partner, a row
    of open slots.  ``first`` / ``count``: the window of vectors to answer for (count None = to the end); the partners come
    from all N, never the vector itself.  -> dict(index=(count, k) int32, score=(count, k) float64): descending score, equal
    scores by ascending index, -1 / NaN in open slots.  Scores are not clipped."""
    V, k, code, first, count = gram_topk_args(V, k, metric, first, count)
    depth, N = V.shape
    index = np.full((count, k), -1, dtype=np.int32)
    score = np.full((count, k), np.nan)
    if count:
        _lib.check(_lib.load().insider_hip_gram_topk(_lib.ptr(V), depth, N, code, k, first, count, int(device),
                                                     _lib.ptr(index, C.c_int32), _lib.ptr(score)))
    return dict(index=index, score=score)


PAIRWISE_MIN_OVERLAP = 3   # with two joint entries every pair scores +-1


def pairwise_min_overlap(min_overlap, depth):
    """The checked ``min_overlap`` of the pairwise-complete calls: None = max(3, ceil(depth / 4)); an integer >= 3 otherwise
    (one above the depth is allowed: no pair is eligible then).  Raises InsiderError(ERR_ARG)."""
    if min_overlap is None:
        return max(PAIRWISE_MIN_OVERLAP, -(-int(depth) // 4))
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, np.integer)) or min_overlap < PAIRWISE_MIN_OVERLAP:
        raise InsiderError(_lib.ERR_ARG, f"min_overlap must be None or an integer >= {PAIRWISE_MIN_OVERLAP}")
    return int(min_overlap)


def gram_topk_pairwise_args(V, k, min_overlap, first, count):
    """The checked arguments of gram_topk_pairwise() / posthoc.gram_topk_pairwise_host(): (V, k, min_overlap, first, count),
    V column-major float64 (depth x N) in which a NaN is a missing entry.  Shape, k, min_overlap, window and infinite values
    raise InsiderError(ERR_ARG)."""
    V = _lib.f64(V)
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] < 1:
        raise InsiderError(_lib.ERR_ARG, "V must be a depth x N array with depth >= 1 and N >= 1")
    depth, N = V.shape
    if N > 2 ** 31 - 1 or depth > 2 ** 31 - 1:
        raise InsiderError(_lib.ERR_ARG, "depth and N must be < 2^31")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NEIGHBOR_MAX_K:
        raise InsiderError(_lib.ERR_ARG, f"k must be an integer in 1..{NEIGHBOR_MAX_K}")
    min_overlap = pairwise_min_overlap(min_overlap, depth)
    if count is None:
        count = N - first if isinstance(first, (int, np.integer)) and not isinstance(first, bool) else count
    for name, v in (("first", first), ("count", count)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise InsiderError(_lib.ERR_ARG, f"{name} must be an integer >= 0")
    if first + count > N:
        raise InsiderError(_lib.ERR_ARG, "the window first + count must lie within the N vectors")
    if np.any(np.isinf(V)):
        raise InsiderError(_lib.ERR_ARG, "V holds an infinite value (NaN is a missing entry)")
    return V, int(k), min_overlap, int(first), int(count)


def gram_topk_pairwise(V, k=10, min_overlap=None, first=0, count=None, device=0):
    """The k best partners of deep vectors with missing entries on the device (insider_hip_gram_topk_pairwise): gram_topk()'s
    correlation, but a NaN in ``V`` (depth x N, one vector per column) is a missing entry and the score of a pair is
    Pearson's r over the positions present in BOTH vectors (the pairwise-complete correlation), not clipped.  A vector with
    fewer than two entries or no variance is dead.  A pair is a candidate when both vectors are alive, it has at least
    ``min_overlap`` joint entries (None = max(3, ceil(depth / 4)); at least 3) and neither vector is constant on them (its
    joint variance must exceed 16 (depth + 8) 2^-52 of its joint sum of squares, taken on the standardised values).
    ``first`` / ``count`` as in gram_topk().  -> dict(index=(count, k) int32, score=(count, k) float64, overlap=(count, k)
    int32: the pair's joint entries): descending score, equal scores by ascending index, -1 / NaN / -1 in open slots."""
    V, k, min_overlap, first, count = gram_topk_pairwise_args(V, k, min_overlap, first, count)
    depth, N = V.shape
    index = np.full((count, k), -1, dtype=np.int32)
    score = np.full((count, k), np.nan)
    overlap = np.full((count, k), -1, dtype=np.int32)
    if count:
        _lib.check(_lib.load().insider_hip_gram_topk_pairwise(_lib.ptr(V), depth, N, min_overlap, k, first, count, int(device),
                                                              _lib.ptr(index, C.c_int32), _lib.ptr(score),
                                                              _lib.ptr(overlap, C.c_int32)))
    return dict(index=index, score=score, overlap=overlap)


ENRICH_MAX_SET = 4096
ENRICH_MAX_PERMS = 65536


def enrichment_args(scores, set_ptr, set_genes, nperm, weight, seed):
    """The arguments of enrichment() / posthoc.enrichment_host() in the library's types: (scores R x p row-major float64 (a
    vector is one profile), set_ptr int64 (S + 1), set_genes int32, nperm, weight, seed).  Shape errors raise
    InsiderError(ERR_ARG); the values are the library's to check."""
    sc = np.ascontiguousarray(np.atleast_2d(np.asarray(scores, dtype=np.float64)))
    ptr = np.ascontiguousarray(set_ptr, dtype=np.int64)
    genes = np.ascontiguousarray(set_genes, dtype=np.int32)
    if sc.ndim != 2 or ptr.ndim != 1 or genes.ndim != 1 or ptr.size < 1:
        raise InsiderError(_lib.ERR_ARG, "scores must be R x p, set_ptr (S + 1) and set_genes vectors")
    if ptr[-1] > genes.size:
        raise InsiderError(_lib.ERR_ARG, "set_ptr ends beyond set_genes")
    for name, v in (("nperm", nperm), ("weight", weight), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise InsiderError(_lib.ERR_ARG, f"{name} must be an integer")
    if not 0 <= seed < 2 ** 64:
        raise InsiderError(_lib.ERR_ARG, "seed must fit 64 bits")
    return sc, ptr, genes, int(nperm), int(weight), int(seed)


def enrichment(scores, set_ptr, set_genes, nperm=1000, weight=1, seed=DEFAULT_SEED, device=0):
    """Preranked gene-set enrichment of every profile (row of ``scores``, R x p) against every set (CSR: set_ptr, set_genes,
    0-based genes) with a permutation null of ``nperm`` random gene sets of equal size (insider_hip_enrichment; the
    definitions are in include/insider_hip.h).  weight 1 weights a gene by |score|, 0 is the classic statistic.  -> the raw
    record: es, sum_same (R x S float64), peak, n_ge, n_same, hits_nonzero (R x S int32), size (S), nonzero (R: the
    profile's non-zero scores), nperm, weight, seed and the inputs (scores, set_ptr, set_genes); posthoc.gs_derived() turns it
    into p, NES, FDR and the hypergeometric p, posthoc.leading_edge() lists a set's leading genes."""
    sc, ptr, genes, nperm, weight, seed = enrichment_args(scores, set_ptr, set_genes, nperm, weight, seed)
    R, p = sc.shape
    S = ptr.size - 1
    rec = dict(es=np.full((R, S), np.nan), sum_same=np.full((R, S), np.nan))
    for name in ("peak", "n_ge", "n_same", "hits_nonzero"):
        rec[name] = np.full((R, S), -1, dtype=np.int32)
    gp = genes if genes.size else np.zeros(1, dtype=np.int32)
    i32 = C.c_int32
    _lib.check(_lib.load().insider_hip_enrichment(_lib.ptr(sc), R, p, _lib.ptr(ptr, C.c_int64), _lib.ptr(gp, i32), S, weight,
                                                  nperm, seed, int(device), _lib.ptr(rec["es"]), _lib.ptr(rec["peak"], i32),
                                                  _lib.ptr(rec["n_ge"], i32), _lib.ptr(rec["n_same"], i32),
                                                  _lib.ptr(rec["sum_same"]), _lib.ptr(rec["hits_nonzero"], i32)))
    rec.update(size=np.diff(ptr).astype(np.int32), nonzero=np.count_nonzero(sc, axis=1).astype(np.int64), nperm=nperm,
               weight=weight, seed=seed, scores=sc, set_ptr=ptr, set_genes=genes)
    return rec


KMEANS_METRICS = {"cosine": 0, "euclidean": 1}
KMEANS_MAX_K = 4096
KMEANS_MAX_RESTARTS = 256
KMEANS_MAX_ITER = 10000


def kmeans_args(points, k, metric, init, restarts, max_iter, seed):
    """The checked arguments of kmeans() / posthoc.kmeans_host(): (P column-major float64 D x N, k, metric code, init
    column-major D x k or None, restarts, max_iter, seed).  Every argument error of insider_hip_kmeans (include/insider_hip.h)
    raises InsiderError(ERR_ARG) here, before the library is reached."""
    def bad(msg):
        return InsiderError(_lib.ERR_ARG, msg)
    P = _lib.f64(points)
    if P.ndim != 2:
        raise bad("points must be a D x N array")
    D, N = P.shape
    if not 1 <= D <= _lib.MAX_K:
        raise bad(f"D must be in 1..{_lib.MAX_K}")
    if not 1 <= N < 2 ** 31:
        raise bad("points must hold 1..2^31-1 columns")
    if metric not in KMEANS_METRICS:
        raise bad(f"metric must be one of {sorted(KMEANS_METRICS)}")
    for name, v, lo, hi in (("k", k, 1, KMEANS_MAX_K), ("restarts", restarts, 1, KMEANS_MAX_RESTARTS),
                            ("max_iter", max_iter, 0, KMEANS_MAX_ITER), ("seed", seed, 0, 2 ** 64 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise bad(f"{name} must be an integer in {lo}..{hi}")
    if not np.isfinite(P).all():
        raise bad("points must be finite")
    code = KMEANS_METRICS[metric]
    n_alive = int(np.count_nonzero((P * P).sum(axis=0) > 0)) if code == 0 else N
    if init is not None:
        init = _lib.f64(init)
        if init.ndim != 2 or init.shape != (D, k):
            raise bad("init must be a D x k array")
        if restarts != 1:
            raise bad("restarts must be 1 when init is given")
        if not np.isfinite(init).all():
            raise bad("init must be finite")
        if code == 0 and not ((init * init).sum(axis=0) > 0).all():
            raise bad("an init column has norm 0")
    elif n_alive < 2:
        raise bad("a drawn start needs at least 2 alive points")
    if k > n_alive:
        raise bad("k must not exceed the number of alive points")
    return P, int(k), code, init, int(restarts), int(max_iter), int(seed)


def kmeans(points, k, metric="cosine", init=None, restarts=8, max_iter=100, seed=DEFAULT_SEED, device=0):
    """K-means (Lloyd) of the columns of ``points`` (D x N, one point per column, as column_factor) on the device
    (insider_hip_kmeans; include/insider_hip.h states the definitions).  metric "cosine" is spherical k-means on the normalised
    columns (an all-zero column is dead: label -1, in no cluster), "euclidean" the plain one.  init: D x k starting centres
    (restarts must then be 1; max_iter = 0 assigns the points to them), None: ``restarts`` Forgy starts drawn from ``seed``, the
    one with the lowest final inertia is returned.  -> dict(centers (D x k), label, second (N int32, 0-based, -1 = none), dist,
    dist2 (N), sizes (k int32), traj (max_iter + 1: the inertia before every update, NaN beyond iters), final_inertia, iters,
    converged (restarts), best, ms (the HIP-event time of the call's kernels))."""
    P, k, code, init, restarts, max_iter, seed = kmeans_args(points, k, metric, init, restarts, max_iter, seed)
    D, N = P.shape
    i32 = C.c_int32
    rec = dict(centers=np.full((D, k), np.nan, order="F"), label=np.full(N, -1, dtype=np.int32), dist=np.full(N, np.nan),
               second=np.full(N, -1, dtype=np.int32), dist2=np.full(N, np.nan), sizes=np.zeros(k, dtype=np.int32),
               traj=np.full(max_iter + 1, np.nan), final_inertia=np.full(restarts, np.nan),
               iters=np.zeros(restarts, dtype=np.int32), converged=np.zeros(restarts, dtype=np.int32))
    best = np.zeros(1, dtype=np.int32)
    lib = _lib.load()
    _lib.check(lib.insider_hip_kmeans(_lib.ptr(P), N, D, k, code, None if init is None else _lib.ptr(init), restarts, max_iter,
                                      seed, int(device), _lib.ptr(rec["centers"]), _lib.ptr(rec["label"], i32),
                                      _lib.ptr(rec["dist"]), _lib.ptr(rec["second"], i32), _lib.ptr(rec["dist2"]),
                                      _lib.ptr(rec["sizes"], i32), _lib.ptr(rec["traj"]), _lib.ptr(rec["final_inertia"]),
                                      _lib.ptr(rec["iters"], i32), _lib.ptr(rec["converged"], i32), _lib.ptr(best, i32)))
    rec.update(best=int(best[0]), ms=float(lib.insider_hip_last_kmeans_ms()))
    return rec


HCLUST_METRICS = {"cosine": 0, "euclidean": 1}
HCLUST_LINKAGES = {"average": 0, "ward": 1}
HCLUST_PAIRS = {"cosine": "average", "euclidean": "ward"}      # the one linkage offered under each metric
HCLUST_MAX_D = 63                                               # HC_MAX_D of insider_amd/csrc/insider_hclust.hpp


def hclust_args(points, metric="cosine", linkage=None, max_rounds=None):
    """The checked arguments of hclust() / posthoc.hclust_host(): (P column-major float64 D x N, metric code, linkage code,
    max_rounds).  linkage None picks the metric's only linkage; max_rounds None is 2 N.  Every argument error of
    insider_hip_hclust (include/insider_hip.h) raises InsiderError(ERR_ARG) here, before the library is reached."""
    def bad(msg):
        return InsiderError(_lib.ERR_ARG, msg)
    P = _lib.f64(points)
    if P.ndim != 2:
        raise bad("points must be a D x N array")
    D, N = P.shape
    if not 1 <= D <= HCLUST_MAX_D:
        raise bad(f"D must be in 1..{HCLUST_MAX_D}")
    if not (N >= 1 and 2 * N - 1 < 2 ** 31):
        raise bad("points must hold 1..2^30 columns")
    if metric not in HCLUST_METRICS:
        raise bad(f"metric must be one of {sorted(HCLUST_METRICS)}")
    if linkage is None:
        linkage = HCLUST_PAIRS[metric]
    if linkage not in HCLUST_LINKAGES:
        raise bad(f"linkage must be one of {sorted(HCLUST_LINKAGES)} (single, complete, centroid and median are not offered)")
    if HCLUST_PAIRS[metric] != linkage:
        raise bad(f"metric {metric!r} with linkage {linkage!r} is not offered: {metric!r} goes with {HCLUST_PAIRS[metric]!r}")
    if max_rounds is None:
        max_rounds = min(2 * N, 2 ** 31 - 1)
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or not 1 <= max_rounds < 2 ** 31:
        raise bad("max_rounds must be an integer in 1..2^31-1")
    if not np.isfinite(P).all():
        raise bad("points must be finite")
    return P, HCLUST_METRICS[metric], HCLUST_LINKAGES[linkage], int(max_rounds)


def hclust(points, metric="cosine", linkage=None, max_rounds=None, device=0):
    """Agglomerative clustering of the columns of ``points`` (D x N, one point per column, as column_factor) on the device
    (insider_hip_hclust; include/insider_hip.h states the definitions and the tie rule).  metric "cosine" goes with linkage
    "average" (UPGMA of cosine distances; an all-zero column is dead: in no cluster), "euclidean" with "ward"; linkage None picks
    that one, any other combination is refused.  -> dict(merge ((N - 1) x 2 int32: the children of every merge, lower id first,
    leaves by point index, row r creates id N + r), height, size (N - 1), order (N int32: the leaf order, dead points last),
    rounds, queries, alive, ms (the HIP-event time of the call's kernels)); rows beyond alive - 1 hold -1 / NaN.  A run that
    max_rounds cuts short raises InsiderError(ERR_UNFINISHED)."""
    P, mcode, lcode, max_rounds = hclust_args(points, metric, linkage, max_rounds)
    D, N = P.shape
    i32 = C.c_int32
    rec = dict(merge=np.full((N - 1, 2), -1, dtype=np.int32), height=np.full(N - 1, np.nan), size=np.full(N - 1, -1, dtype=np.int32),
               order=np.full(N, -1, dtype=np.int32))
    rounds, alive, queries = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    lib = _lib.load()
    _lib.check(lib.insider_hip_hclust(_lib.ptr(P), N, D, mcode, lcode, max_rounds, int(device), _lib.ptr(rec["merge"], i32),
                                      _lib.ptr(rec["height"]), _lib.ptr(rec["size"], i32), _lib.ptr(rec["order"], i32),
                                      _lib.ptr(rounds, i32), _lib.ptr(queries, C.c_int64), _lib.ptr(alive, i32)))
    rec.update(rounds=int(rounds[0]), queries=int(queries[0]), alive=int(alive[0]), ms=float(lib.insider_hip_last_hclust_ms()))
    return rec


TSNE_MAX_N = 2 ** 20
TSNE_MAX_K = NEIGHBOR_MAX_K
TSNE_MAX_ITER = 10000
TSNE_MAX_SLABS = 64


def tsne_args(nbr_idx, nbr_d2, perplexity, init=None, max_iter=1000, exag_iters=250, kl_every=50, exaggeration=12.0, eta=0.0,
              seed=DEFAULT_SEED, slabs=0):
    """The checked arguments of tsne() / posthoc.tsne_host(): (nbr_idx int32 N x k and nbr_d2 float64 N x k, both row-major,
    perplexity, init row-major N x 2 or None, max_iter, exag_iters, kl_every, exaggeration, eta, seed, slabs, alive (N bool)).
    Every argument error of insider_hip_tsne (include/insider_hip.h) raises InsiderError(ERR_ARG) here, before the library is
    reached."""
    def bad(msg):
        return InsiderError(_lib.ERR_ARG, msg)
    if nbr_idx is None or nbr_d2 is None:
        raise bad("nbr_idx and nbr_d2 are required")
    raw = np.asarray(nbr_idx)
    if raw.ndim != 2 or raw.dtype.kind not in "iu":
        raise bad("nbr_idx must be an N x k integer array")
    N, k = raw.shape
    if not 1 <= N <= TSNE_MAX_N:
        raise bad("N must be in 1..2^20")
    if not 1 <= k <= TSNE_MAX_K:
        raise bad(f"k must be in 1..{TSNE_MAX_K}")
    if raw.min() < -1 or raw.max() >= N:
        raise bad("neighbour index out of range")
    idx = np.ascontiguousarray(raw, dtype=np.int32)
    d2 = np.ascontiguousarray(nbr_d2, dtype=np.float64)
    if d2.shape != idx.shape:
        raise bad("nbr_d2 must have the shape of nbr_idx")
    for name, v, lo, hi in (("max_iter", max_iter, 0, TSNE_MAX_ITER), ("exag_iters", exag_iters, 0, TSNE_MAX_ITER),
                            ("kl_every", kl_every, 1, 2 ** 31 - 1), ("seed", seed, 0, 2 ** 64 - 1), ("slabs", slabs, 0, TSNE_MAX_SLABS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise bad(f"{name} must be an integer in {lo}..{hi}")
    for name, v, lo in (("perplexity", perplexity, 1.0), ("exaggeration", exaggeration, 1.0), ("eta", eta, 0.0)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < lo:
            raise bad(f"{name} must be finite and >= {lo:g}")
    if max_iter == 0 and init is None:
        raise bad("max_iter = 0 needs init")
    filled = idx >= 0
    if (filled[:, 1:] & ~filled[:, :-1]).any():
        raise bad("a filled slot follows an open one")
    if (idx == np.arange(N, dtype=np.int32)[:, None]).any():
        raise bad("a row names itself")
    srt = np.sort(idx, axis=1)
    if ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any():
        raise bad("an index is repeated within a row")
    dv = d2[filled]
    if not (np.isfinite(dv) & (dv >= 0.0)).all():
        raise bad("d2 must be finite and >= 0 in a filled slot")
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.float64)
        if init.shape != (N, 2):
            raise bad("init must be an N x 2 array")
        if not np.isfinite(init).all():
            raise bad("init must be finite")
    alive = filled[:, 0] | (np.bincount(idx[filled], minlength=N) > 0)
    if int(alive.sum()) < 2:
        raise bad("fewer than 2 alive points")
    return (idx, d2, float(perplexity), init, int(max_iter), int(exag_iters), int(kl_every), float(exaggeration), float(eta),
            int(seed), int(slabs), alive)


def tsne(nbr_idx, nbr_d2, perplexity=20.0, init=None, max_iter=1000, exag_iters=250, kl_every=50, exaggeration=12.0, eta=0.0,
         seed=DEFAULT_SEED, slabs=0, device=0):
    """The exact t-SNE map of a neighbour graph on the device (insider_hip_tsne; include/insider_hip.h states the definitions).
    nbr_idx (N x k, 0-based, -1 = open slot) and nbr_d2 (N x k squared distances) are a row per point, as
    posthoc.embedding_graph() returns them.  init: N x 2 start (max_iter = 0 evaluates KL, Z and the gradient there), None: drawn
    from ``seed``.  eta = 0: max(Na / (4 exaggeration), 50).  slabs = 0: the library cuts the all-pairs sum.  -> dict(y (N x 2,
    NaN for a dead point), kl_traj (max_iter // kl_every + 1: KL at Y_t, t = 0, kl_every, ...), final_kl, beta (N), p_cond (N x k),
    grad (N x 2, at y under exaggeration 1), z, alive (N bool), ms (the HIP-event time of the call's kernels))."""
    idx, d2, perplexity, init, max_iter, exag_iters, kl_every, exaggeration, eta, seed, slabs, alive = tsne_args(
        nbr_idx, nbr_d2, perplexity, init, max_iter, exag_iters, kl_every, exaggeration, eta, seed, slabs)
    N, k = idx.shape
    rec = dict(y=np.full((N, 2), np.nan), kl_traj=np.full(max_iter // kl_every + 1, np.nan), beta=np.full(N, np.nan),
               p_cond=np.full((N, k), np.nan), grad=np.full((N, 2), np.nan))
    fin, z = np.full(1, np.nan), np.full(1, np.nan)
    lib = _lib.load()
    _lib.check(lib.insider_hip_tsne(_lib.ptr(idx, C.c_int32), _lib.ptr(d2), N, k, perplexity,
                                    None if init is None else _lib.ptr(init), max_iter, exag_iters, kl_every, exaggeration, eta,
                                    seed, slabs, int(device), _lib.ptr(rec["y"]), _lib.ptr(rec["kl_traj"]), _lib.ptr(fin),
                                    _lib.ptr(rec["beta"]), _lib.ptr(rec["p_cond"]), _lib.ptr(rec["grad"]), _lib.ptr(z)))
    rec.update(final_kl=float(fin[0]), z=float(z[0]), alive=alive, ms=float(lib.insider_hip_last_tsne_ms()))
    return rec


# ---------------------------------------------------------------------------------------------------------------
# caller level — R/insider.R, R/utils.R
# ---------------------------------------------------------------------------------------------------------------
def init_parameters(size, init_mean=0.0, init_std=0.001, rng=None):
    """R/utils.R:40-43: rnorm(size, mean, sd). ``rng`` replaces R's global RNG."""
    rng = rng if rng is not None else np.random.default_rng()
    return rng.normal(init_mean, init_std, size=size)


def ratio_splitter(data, ratio=0.1, rm_na_col=True, seed=123):
    """R/utils.R:78-117: element-wise hold-out without replacement; NA -> 0 and excluded; all-zero columns of the
    train set dropped.  (numpy PCG64 stands in for R's set.seed(123); sample().)"""
    data = np.array(data, dtype=np.float64, order="F")
    na = np.isnan(data)
    data[na] = 0.0
    train = ~na
    rng = np.random.Generator(np.random.PCG64(seed))
    existing = np.flatnonzero((~na).ravel(order="F"))
    k = int(np.floor(existing.size * ratio))
    test_idx = rng.choice(existing, size=k, replace=False)
    test = np.zeros(data.size, dtype=bool)
    test[test_idx] = True
    test = test.reshape(data.shape, order="F")
    testset = np.where(test, data, 0.0)
    trainset = np.where(test, 0.0, data)
    train &= ~test
    num_per_col = (trainset != 0).sum(axis=0)
    print(f"number of all zero columns removed: {int((num_per_col == 0).sum())}")
    keep = num_per_col != 0 if rm_na_col else np.ones(data.shape[1], dtype=bool)
    return dict(trainset=trainset[:, keep], testset=testset[:, keep], train_indicator=train[:, keep],
                test_indicator=test[:, keep], na_indicator=na[:, keep], kept_columns=keep)


def fold_splitter(data, folds=5, rm_na_col=True, seed=123):
    """k-fold counterpart of ratio_splitter(): NA -> 0 and fold id 0; the non-NA entries are permuted (numpy PCG64, like
    ratio_splitter) and dealt round-robin to the folds 1..F, so fold sizes differ by at most one and every non-NA entry is
    held out in exactly one fold.  A column is kept when its non-zero entries lie in at least two folds: R/utils.R:102-109
    drops a column whose train set is all zero, and the train set of fold f is every other fold, so the rule holds for every
    fold at once exactly then.  Returns fold_id (uint8), na_indicator and data over the kept columns, and kept_columns."""
    F = int(folds)
    if not 2 <= F <= 255:
        raise ValueError("fold_splitter(): folds must be in 2..255")
    data = np.array(data, dtype=np.float64, order="F")
    na = np.isnan(data)
    data[na] = 0.0
    rng = np.random.Generator(np.random.PCG64(seed))
    existing = np.flatnonzero((~na).ravel(order="F"))
    ids = np.zeros(data.size, dtype=np.uint8)
    ids[rng.permutation(existing)] = (np.arange(existing.size) % F + 1).astype(np.uint8)
    ids = ids.reshape(data.shape, order="F")
    nz = data != 0
    folds_with_nz = sum(((ids == f) & nz).any(axis=0).astype(np.int64) for f in range(1, F + 1))
    keep = folds_with_nz >= 2 if rm_na_col else np.ones(data.shape[1], dtype=bool)
    print(f"number of columns removed by the fold rule: {int((~keep).sum())}")
    return dict(fold_id=np.asfortranarray(ids[:, keep]), na_indicator=na[:, keep], kept_columns=keep,
                data=np.asfortranarray(data[:, keep]))


def pooled_rmse(fold_rmse, fold_counts):
    """Cross-validated RMSE of fold RMSEs rmse_f over n_f held-out entries each: sqrt(sum_f n_f rmse_f^2 / sum_f n_f) — every
    held-out entry counted once.  ``fold_rmse``: (..., F); ``fold_counts``: (F,)."""
    r = np.asarray(fold_rmse, dtype=np.float64)
    w = np.asarray(fold_counts, dtype=np.float64)
    return np.sqrt((r * r * w).sum(axis=-1) / w.sum())


class Insider(dict):
    """The reference's S3 object of class "insider" (a list, R/insider.R:24)."""


def insider(data, confounder, ctns_confounder=None, interaction_idx=None, split_ratio=0.1, global_tol=1e-9,
            sub_tol=1e-5, tuning_iter=30, max_iter=50000, device=0, seed=DEFAULT_SEED, folds=None):
    """insider() of R/insider.R:18-67.  ``folds`` = k (not in the reference): the object also carries ``fold_id``
    (fold_splitter) for tune(folds=True), over the columns both splitters keep."""
    data = np.asarray(data, dtype=np.float64)
    confounder = np.asarray(confounder)
    if confounder.ndim == 1:
        confounder = confounder[:, None]
    dataset = ratio_splitter(data, ratio=split_ratio)
    obj = Insider()
    keep = dataset["kept_columns"]
    fold_id = None
    if folds is not None:
        fs = fold_splitter(data, folds=folds)
        both = keep & fs["kept_columns"]
        fold_id = fs["fold_id"][:, both[fs["kept_columns"]]]
        for name in ("train_indicator", "test_indicator", "na_indicator"):
            dataset[name] = dataset[name][:, both[keep]]
        keep = both
    d = np.array(data[:, keep], dtype=np.float64, order="F")
    d[np.isnan(d)] = 0.0                                      # R/insider.R:26 (intent: NA -> 0)
    obj["data"] = d
    if interaction_idx is not None and len(interaction_idx) > 1 and \
            all(isinstance(v, (int, np.integer)) for v in interaction_idx):
        if max(interaction_idx) > confounder.shape[1]:
            raise ValueError("The interaction_idx is out of the range of confounder!")   # R/insider.R:30-32
        from .workloads import interaction_indicator
        obj["confounder"] = interaction_indicator(confounder.astype(np.int32), tuple(interaction_idx))  # :34-40
    elif interaction_idx is None:
        obj["confounder"] = np.asfortranarray(confounder, dtype=np.int32)                 # :43
    else:
        raise ValueError("The interaction_idx should be integers and its length must be greater than or equal to 2!")
    if ctns_confounder is not None:
        obj["inc_continuous"] = 1
        obj["ctns_confounder"] = np.asarray(ctns_confounder, dtype=np.float64)
    else:
        obj["inc_continuous"] = 0
        obj["ctns_confounder"] = np.zeros((confounder.shape[0], 1))
    obj["train_indicator"] = np.asfortranarray(dataset["train_indicator"], dtype=np.uint8)   # :57-59
    obj["test_indicator"] = np.asfortranarray(dataset["test_indicator"], dtype=np.uint8)
    obj["na_indicator"] = np.asfortranarray(dataset["na_indicator"], dtype=np.uint8)
    if fold_id is not None:
        obj["fold_id"] = np.asfortranarray(fold_id, dtype=np.uint8)
    obj["params"] = dict(global_tol=global_tol, sub_tol=sub_tol, tuning_iter=tuning_iter, max_iter=max_iter)
    obj["device"] = device
    obj["seed"] = seed
    return obj


def _resident(obj, which):
    """HBM-resident data set for the tune (train/test masks) or fit (train+test / NA masks) call pattern."""
    key = "_resident_" + which
    if key not in obj:
        if which == "tune":
            tr, te = obj["train_indicator"], obj["test_indicator"]
        else:  # R/insider.R:207-208: indicator = train + test, "test" = NA mask
            tr, te = obj["train_indicator"] + obj["test_indicator"], obj["na_indicator"]
        other = obj.get("_resident_" + ("fit" if which == "tune" else "tune"))
        if other is not None and getattr(other, "_h", None):
            # the same X under other masks: share the resident matrix instead of a second upload and device copy
            obj[key] = other.remask(tr, te)
        else:
            obj[key] = InsiderData(obj["data"], obj["confounder"], tr, te, device=obj.get("device", 0),
                                   ctns_confounder=obj["ctns_confounder"] if obj["inc_continuous"] == 1 else None)
    return obj[key]


def _fresh_inits(obj, latent_rank, rng):
    conf = obj["confounder"]
    cfd = [np.asfortranarray(init_parameters(len(np.unique(conf[:, i])) * latent_rank, rng=rng)
                             .reshape((-1, latent_rank), order="F")) for i in range(conf.shape[1])]     # :106-109
    if obj["inc_continuous"] == 1:
        cfd.append(np.asfortranarray(init_parameters(obj["ctns_confounder"].shape[1] * latent_rank, rng=rng)
                                     .reshape((-1, latent_rank), order="F")))                            # :111-113
    col = np.asfortranarray(init_parameters(latent_rank * obj["data"].shape[1], rng=rng)
                            .reshape((latent_rank, -1), order="F"))                                      # :114
    return cfd, col


def _grid_sum(rows, world):
    """Combine the per-rank result tables of a grid-parallel tune(): every rank filled only its own rows."""
    if world <= 1:
        return rows
    import torch
    import torch.distributed as dist
    t = torch.from_numpy(np.ascontiguousarray(rows))
    if dist.get_backend() == "nccl":
        t = t.cuda()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy()


def _nearest_finished(done, g, n_lambda):
    """Index of the finished grid point closest to g on the (alpha row, lambda column) lattice (expand.grid order: lambda
    fastest), ties to the lower index; None when nothing is finished yet."""
    best, bd = None, None
    for h in done:
        d = abs(h // n_lambda - g // n_lambda) + abs(h % n_lambda - g % n_lambda)
        if bd is None or d < bd or (d == bd and h < best):
            best, bd = h, d
    return best


def _usable_clone(hd, base):
    """The rule of tune()'s handle pools (_tune_clones, _fold_handles, _fold_clones): a handle made from `base` (``_src``) is
    usable only while it is open and `base` is still the handle it came from (bench.py closes clones between grids; a
    re-created resident data set is another `base`)."""
    return bool(getattr(hd, "_h", None)) and getattr(hd, "_src", None) is base


def _bring_options(hd, base):
    """A handle made from `base` copied its options as they stood then: bring the ones set on `base` since across."""
    for name, value in getattr(base, "_options", {}).items():
        if getattr(hd, "_options", {}).get(name) != value:
            hd.set_option(name, value)


def _clone(base):
    hd = base.clone()
    hd._src = base
    return hd


def _tune_handles(obj, ds, k):
    """k handles on the resident tune() data set: the data set's own plus k - 1 clones (insider_hip_clone: shared device
    arrays, private workspaces), kept on the object for the next call."""
    clones = [hd for hd in obj.get("_tune_clones", []) if _usable_clone(hd, ds)]
    while len(clones) < k - 1:
        clones.append(_clone(ds))
    obj["_tune_clones"] = clones
    for hd in clones[: k - 1]:
        _bring_options(hd, ds)
    return [ds] + clones[: k - 1]


def _fold_handles(obj, ds):
    """The fold data sets ds.fold(1..F) of the resident tune data set, derived once and kept on the object, and
    ``obj["_fold_clones"]``: {(worker, fold index): clone of that fold's handle}, the usable ones of earlier calls.  All of
    them carry the options of `ds` as they stand now."""
    hs = obj.get("_fold_handles", [])
    if not hs or not all(_usable_clone(hd, ds) for hd in hs):
        fold_id = np.asarray(obj["fold_id"])
        ds.set_folds(fold_id, int(fold_id.max()))
        hs = []
        for f in range(1, int(fold_id.max()) + 1):
            hd = ds.fold(f)
            hd._src = ds
            hs.append(hd)
        obj["_fold_handles"] = hs
        obj["_fold_clones"] = {}
    obj["_fold_clones"] = {(w, f): hd for (w, f), hd in obj.get("_fold_clones", {}).items() if _usable_clone(hd, hs[f])}
    for hd in hs:
        _bring_options(hd, ds)
    for (w, f), hd in obj["_fold_clones"].items():
        _bring_options(hd, hs[f])
    return hs


def _fold_clone(obj, base, worker, f):
    """Worker `worker` > 0's clone of the fold handle `base` of fold index f: made on first use, kept on the object."""
    clones = obj["_fold_clones"]
    if (worker, f) not in clones:
        clones[(worker, f)] = _clone(base)
    return clones[(worker, f)]


def _fit_points(obj, points, label, handle, F, k, rng, rank, world, timings, warm_cols=0, done=None):
    """tune()'s one scheduler: fit ``points`` — (K, lambda, alpha) in the reference's order — once per fold (``F`` folds,
    1 = the single hold-out), ``k`` fits in flight, and return the train and test RMSE tables (points x F) summed over the
    ranks.

    One producer thread walks all points: it draws every point's fresh inits from ``rng`` on every rank (the generator state
    depends on neither ``world`` nor the mode), and for the points of this rank (g % world == rank) queues one task per fold,
    at most 2 k F ahead of the fits: the arrays themselves when F == 1, F-ordered copies per fold otherwise (a fit updates its
    arguments in place).  Worker w takes tasks until its sentinel arrives and fits them on ``handle(w, fold)``.  With k == 1
    the one worker is the calling thread; with k > 1 every worker is a thread and the caller waits (two fits in flight are
    slower when the caller's thread drives one of them: profiles/tune_scheduler/README.md).  Once any draw or fit has failed
    the producer stops drawing and the workers discard what is queued, so nobody blocks on the queue; all threads are joined
    and the first error is raised.

    ``label(K, lambda, alpha)`` is printed when the first task of a point is taken.  ``warm_cols`` = n_lambda > 0 (k == 1 and
    F == 1 only): point g starts from copies of the fitted factors of _nearest_finished() instead of from its draw.  ``done(g,
    train, test)`` is called after the last fold of point g (k == 1 only: the points finish in order)."""
    import queue
    import threading
    import time as _time
    prm, seed = obj["params"], obj.get("seed", DEFAULT_SEED)
    train, test = np.zeros((len(points), F)), np.zeros((len(points), F))
    tasks = queue.Queue(maxsize=2 * k * F)
    lock = threading.Lock()
    errors, labelled = [], set()
    finished = {}           # warm start: point -> (row factors, column factor) of the points this rank has fitted

    def _producer():
        try:
            for g, (K, _, _) in enumerate(points):
                if errors:
                    break
                t_0 = _time.perf_counter()
                cfd, col = _fresh_inits(obj, K, rng)            # ONE draw per point, whatever the number of folds
                t_draw = _time.perf_counter() - t_0
                if g % world != rank:
                    continue
                for f in range(F):
                    tasks.put((g, f, cfd, col, t_draw) if F == 1 else
                              (g, f, [a.copy(order="F") for a in cfd], col.copy(order="F"), t_draw))
        except BaseException as e:      # a failed draw (MemoryError, ...) must not leave the workers waiting for ever
            errors.append(e)
        finally:
            for _ in range(k):          # one sentinel per worker, whatever happened above
                tasks.put(None)

    def _fit(w, t_wait, g, f, cfd, col, t_draw):
        K, l, a = points[g]
        t_1 = _time.perf_counter()
        with lock:
            if g not in labelled:
                labelled.add(g)
                print(label(K, l, a))
        src = _nearest_finished(finished, g, warm_cols) if warm_cols else None
        if src is not None:
            cfd, col = [x.copy(order="F") for x in finished[src][0]], finished[src][1].copy(order="F")
        hd = handle(w, f)
        fitted = hd.optimize(cfd, col, K, l, l, a, 1, prm["global_tol"], prm["sub_tol"], prm["tuning_iter"], seed=seed,
                             inc_continuous=obj["inc_continuous"], copy=False)
        if warm_cols:
            finished[g] = (list(fitted["row_matrices"].values()), fitted["column_factor"])
            for old_g in [h for h in finished if h < g - warm_cols * world - world]:     # keep about one alpha row back
                del finished[old_g]
        with lock:
            train[g, f], test[g, f] = fitted["train_rmse"], fitted["test_rmse"]
            if timings is not None:
                timings.append(dict(latent_rank=K, lambda_=l, alpha=a, init_s=t_draw, init_wait_s=t_wait if k == 1 else 0.0,
                                    warm_from=src, optimize_s=_time.perf_counter() - t_1, library_ms=hd.profile()["wall_ms"]))
                if F > 1:
                    timings[-1]["fold"] = f + 1
        if done is not None and f == F - 1:
            done(g, train, test)

    def _worker(w):
        while True:
            try:                        # BaseException: a lone worker is the caller's thread: a KeyboardInterrupt arrives here
                t_w = _time.perf_counter()
                item = tasks.get()
                if item is None:
                    return
                if not errors:
                    _fit(w, _time.perf_counter() - t_w, *item)
            except BaseException as e:
                errors.append(e)

    threads = [threading.Thread(target=_producer)] + [threading.Thread(target=_worker, args=(w,)) for w in range(k) if k > 1]
    for t in threads:
        t.start()
    if k == 1:
        _worker(0)
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return _grid_sum(train, world), _grid_sum(test, world)


def tune(obj, latent_dimension=None, lambda_=0.1, alpha=0.0, out_dir=None, rng=None, rank=0, world=1, timings=None,
         warm_start=False, concurrent=1, folds=None):
    """tune() of R/insider.R:81-176.  ``out_dir``: where to write the reference's CSVs (None = do not write).

    ``warm_start`` (opt-in, NOT the reference's behaviour, which draws fresh N(0, 0.001^2) inits for every grid point,
    R/insider.R:152-161): the fit of (lambda, alpha) grid point g starts from the fitted factors of the nearest grid point
    this rank has already finished instead of from its fresh draw (which is still drawn, so the generator state — and
    every point that does start cold — is unchanged).  The first outer iterations of a cold fit run thousands of
    coordinate sweeps per gene to leave the near-zero inits; a neighbouring optimum is a few hundred sweeps away.
    IT CHANGES THE ANSWER, not only the time: a tuning_iter = 30 fit is not converged, so a fit that starts near a
    neighbour's optimum ends elsewhere than the cold fit of the same point, and the grid's argmin may move.  Measured
    (profiles/r04/grid_c3_k2.json, grid_c2_k4.json): the selected (lambda, alpha) DIFFERED from the cold grid's at config 3
    and at config 2 (`best_point_agrees_with_cold` false in both; largest test-RMSE difference over the 40 points 2.4e-5
    and 4e-4).  Use it to explore a grid quickly; re-run the chosen neighbourhood cold before reporting a selection.

    ``rank`` / ``world``: grid-parallel tuning across the GPUs of a node: every rank keeps the
    whole data set resident, grid point g is fitted by rank g % world and the result tables are summed over
    torch.distributed.  The fresh inits of ALL grid points are drawn on every rank, in the reference's order, so
    the tables do not depend on ``world``.  ``timings``: a list that receives one dict per fit, of the rank sweep and of the
    grid, one per fold with ``folds`` (latent_rank, lambda_, alpha, with folds ``fold``; init_s = drawing the fresh inits,
    init_wait_s = what the one worker waited for them, 0.0 with several; warm_from; optimize_s = the optimize() call,
    library_ms = time inside the library).

    Every mode runs on one scheduler (_fit_points), once for the rank sweep and once for the grid: a producer thread draws the
    inits ahead of the fits (numpy's generator and the ctypes call both release the GIL), ``concurrent`` workers fit them,
    a single one on the calling thread.  The CSVs are rewritten after every point when one worker fits a hold-out
    sweep of a one-rank job, and written once at the end (by rank 0) otherwise.

    ``concurrent`` = k > 1: k points of this rank are fitted AT THE SAME TIME on the one GPU, each on its own handle of
    the shared resident data set (InsiderData.clone, kept on the object as ``_tune_clones``) from its own host thread.  The
    points are independent fits (R/insider.R:145-164), and a data set of the size real INSIDER inputs have does not fill an
    MI355X with one fit: its column step is bound by its longest gene's sequential sweep chain, which a second fit overlaps.
    The inits are still drawn by ONE generator in the reference's order, and every point's result is bit-identical to the
    serial sweep's (tests/test_gpu_sharded.py::test_concurrent_tune_is_bit_identical).  Not combinable with ``warm_start``
    (whose starting points depend on the order in which fits finish).

    ``folds`` (default None: the single hold-out above, unchanged): with ``folds=True`` every point of the rank sweep and of
    the grid is fitted once per fold of ``obj["fold_id"]`` (insider(folds=k)), on the data sets ``ds.fold(1..F)`` derived
    once from the resident tune data set (InsiderData.fold: X is not uploaded or copied again) and kept on the object.  The
    fresh inits of a point are drawn ONCE, in the reference's order from the one generator, and every fold of the point starts
    from copies of them: the generator state after tune() does not depend on ``folds``.  ``rank_tuning`` / ``reg_tuning``
    keep their columns, with train RMSE = the mean over the folds and test RMSE = the pooled (cross-validated) value
    sqrt(sum_f n_f rmse_f^2 / sum_f n_f), n_f = held-out entries of fold f; ``rank_tuning_folds`` / ``reg_tuning_folds``
    hold the per-fold test RMSE (points x F), ``*_test_sd`` their sample standard deviation.  ``concurrent`` = k runs up
    to k (point, fold) fits at once on the fold handles and clones of them; results are bit-identical to the serial order.
    Options set on the resident data set reach the fold handles and their clones at the next call.
    The CSVs keep their columns; a second file ``..._folds.csv`` holds the point's parameters and its per-fold test RMSE.
    Not combinable with ``warm_start`` (ValueError)."""
    if folds is not None and folds is not False:
        if warm_start:
            raise ValueError("tune(): folds and warm_start exclude each other")
        if folds is not True:
            raise ValueError("tune(): folds must be None or True (the folds are those of obj['fold_id'], insider(folds=k))")
        if "fold_id" not in obj:
            raise ValueError("tune(folds=True): the object carries no fold ids: build it with insider(..., folds=k)")
    if concurrent > 1 and warm_start:
        raise ValueError("tune(): concurrent > 1 and warm_start exclude each other")
    lat = np.atleast_1d(latent_dimension) if latent_dimension is not None else np.array([])
    lam = np.atleast_1d(np.asarray(lambda_, dtype=float))
    alp = np.atleast_1d(np.asarray(alpha, dtype=float))
    if lat.size == 0 or not np.issubdtype(lat.dtype, np.integer):
        raise ValueError("TUNNING: The element of latent_dimension, lambda, and alpha should be integer, numeric, "
                         "and numeric.")                                                                 # :83-85
    if lat.size <= 1 and lam.size <= 1 and alp.size <= 1:
        raise ValueError("TUNNING: The length of either latent_dimension or lambda and alpha should be greater "
                         "than 1.")                                                                      # :87-89
    rng = rng if rng is not None else np.random.default_rng(obj.get("seed", DEFAULT_SEED))
    ds = _resident(obj, "tune")
    k = max(1, int(concurrent))
    if folds:
        fold_handles = _fold_handles(obj, ds)
        F = len(fold_handles)
        n_f = np.array([(np.asarray(obj["fold_id"]) == f).sum() for f in range(1, F + 1)], dtype=np.float64)

        def handle(w, f):       # worker 0 fits on the fold handles themselves, worker w > 0 on its clones of them
            return fold_handles[f] if w == 0 else _fold_clone(obj, fold_handles[f], w, f)

        out = dict(rank_tuning=None, reg_tuning=None, rank_tuning_folds=None, reg_tuning_folds=None, rank_tuning_test_sd=None,
                   reg_tuning_test_sd=None, fold_counts=n_f)
    else:
        F = 1
        handles = _tune_handles(obj, ds, k) if k > 1 else [ds]

        def handle(w, f):
            return handles[w]

        out = dict(rank_tuning=None, latent_rank=None, reg_tuning=None)
    stepwise = not folds and world == 1 and k == 1      # the table is rewritten after every point, as the reference does

    def _table(head, train, test):
        """The reference's columns: the point's parameters, train RMSE (mean over the folds), test RMSE (pooled over them)."""
        return np.column_stack([head, train.mean(axis=1), pooled_rmse(test, n_f) if folds else test[:, 0]])

    def _save(name, table):
        if out_dir is not None and rank == 0:
            np.savetxt(os.path.join(out_dir, name), table, delimiter=",")

    def _sweep(which, csv, points, head, label, warm_cols=0):
        """Fit `points`, fill out[which] (with folds: its per-fold table and spread too) and write the CSVs."""
        head = np.array(head, dtype=np.float64).reshape(len(points), -1)
        done = (lambda g, tr, te: _save(csv + ".csv", _table(head[: g + 1], tr[: g + 1], te[: g + 1]))) if stepwise else None
        train, test = _fit_points(obj, points, label, handle, F, k, rng, rank, world, timings, warm_cols, done)
        out[which] = _table(head, train, test)
        if not stepwise:
            _save(csv + ".csv", out[which])
        if folds:
            out[which + "_folds"] = test
            out[which + "_test_sd"] = test.std(axis=1, ddof=1) if F > 1 else np.zeros(len(test))
            _save(csv + "_folds.csv", np.column_stack([head, test]))

    if lat.size > 1:                                                                                     # :98-132
        l_, a_ = (float(lam[0]), float(alp[0])) if lam.size == 1 and alp.size == 1 else (0.1, 0.0)      # :120-121
        _sweep("rank_tuning", "insider_rank_tuning_result", [(int(K), l_, a_) for K in lat], [int(K) for K in lat],
               lambda K, l, a: f"Latent rank:  {K} ---------------------------------")
        latent_rank = int(lat[int(np.argmin(out["rank_tuning"][:, 2]))])                                 # :136
    else:
        latent_rank = int(lat[0])
    out["latent_rank"] = latent_rank
    if lam.size > 1 or alp.size > 1:                                                                     # :142-174
        grid = [(round(float(l_), 2), round(float(a_), 2)) for a_ in alp for l_ in lam]   # expand.grid: lambda fastest
        _sweep("reg_tuning", f"insider_R{latent_rank}_reg_tuning_result", [(latent_rank, l_, a_) for l_, a_ in grid], grid,
               lambda K, l, a: f"parameter grid: {l},{a} ---------------------------------",
               warm_cols=lam.size if warm_start else 0)
    return out


def fit(obj, latent_dimension=None, lambda_=None, alpha=None, partition=0, rng=None):
    """fit() of R/insider.R:190-216."""
    prm = obj["params"]
    rng = rng if rng is not None else np.random.default_rng(obj.get("seed", DEFAULT_SEED))
    K = int(latent_dimension)
    cfd, col = _fresh_inits(obj, K, rng)
    ds = _resident(obj, "fit")
    fitted = ds.optimize(cfd, col, K, float(lambda_), float(lambda_), float(alpha), int(partition), prm["global_tol"],
                         prm["sub_tol"], prm["max_iter"], seed=obj.get("seed", DEFAULT_SEED),
                         inc_continuous=obj["inc_continuous"])
    obj["cfd_matrices"] = fitted["row_matrices"]                                                         # :211-213
    obj["column_factor"] = fitted["column_factor"]
    obj["test_rmse"] = fitted["test_rmse"]
    obj["train_rmse"] = fitted["train_rmse"]
    obj["loss"] = fitted["loss"]
    obj["traj"] = fitted["traj"]
    return obj
