"""Python side of the compiled reference (oracle/_ref/insider_ref, built by oracle/ref_build.py).

Lays a case out as raw little-endian column-major files plus a text manifest, runs the binary as a child process under a
time limit, and returns the arrays and scalars it wrote, the parsed log and the sweep count (calls of randperm: one per
coordinate-descent sweep).  The reference runs with the cyclic sweep order (order_mode = 1 of the library and the oracle).
"""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from . import ref_build

LOG_COLS = ("iter", "train_rmse", "test_rmse", "sse_half", "row_reg_half", "col_reg_half", "l1_reg", "delta_loss")
THREADS = 8     # cap of the child's OpenMP teams (the reference asks for 10 and 30 threads)


class RefError(RuntimeError):
    pass


def available():
    return ref_build.available()


def _write_case(d, entry, scalars, arrays):
    lines = ["entry %s" % entry]
    for k, v in scalars.items():
        lines.append("scalar %s %s" % (k, repr(float(v))))
    for k, a in arrays.items():
        a = np.asarray(a)
        if a.dtype.kind in "ui" or a.dtype == np.bool_:
            a = a.astype("<u4")
            dt = "u32"
        else:
            a = a.astype("<f8")
            dt = "f64"
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        assert a.ndim == 2, k
        lines.append("array %s %s %d %d" % (k, dt, a.shape[0], a.shape[1]))
        with open(os.path.join(d, k + ".bin"), "wb") as f:
            f.write(np.asfortranarray(a).tobytes(order="F"))
    with open(os.path.join(d, "manifest.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def _read_out(d):
    out = {}
    with open(os.path.join(d, "out_manifest.txt")) as f:
        for line in f:
            t = line.split()
            if t[0] == "scalar":
                out[t[1]] = float(t[2])
            else:
                r, c = int(t[3]), int(t[4])
                raw = np.fromfile(os.path.join(d, t[1] + ".bin"), dtype="<f8" if t[2] == "f64" else "<u4")
                out[t[1]] = raw.reshape((r, c), order="F")
    return out


_NUM = r"([-+0-9.eE]+|-?nan|-?inf)"
_PAT = [(re.compile(r"insider iter \d+: train rmse = " + _NUM), 1), (re.compile(r"insider iter \d+: test rmse = " + _NUM), 2),
        (re.compile(r"total_residual\t" + _NUM + ";"), 3), (re.compile(r"row_reg_loss:\t" + _NUM + ";"), 4),
        (re.compile(r"col_reg_loss:\t" + _NUM + ";"), 5), (re.compile(r"l1_reg_loss:\t" + _NUM + r"\."), 6)]
_DELTA = re.compile(r"Delta loss for iter (\d+):" + _NUM)


def parse_log(text):
    """The reference's 12-digit log as an array with columns LOG_COLS: one row for the evaluation of the initial values
    (iter -1, delta NaN), then one per checkpoint."""
    rows = []
    cur = None
    for line in text.splitlines():
        m = _DELTA.match(line)
        if m:
            cur[0], cur[7] = float(m.group(1)), float(m.group(2))
            continue
        for pat, col in _PAT:
            m = pat.match(line)
            if m:
                if col == 1:
                    cur = [np.nan] * len(LOG_COLS)
                    cur[0] = -1.0
                    rows.append(cur)
                cur[col] = float(m.group(1))
                break
    return np.array(rows, dtype=np.float64).reshape(-1, len(LOG_COLS))


def run_case(entry, scalars, arrays, timeout=600, binary=None, keep=None):
    """One call of the binary.  Returns dict(name -> array | float) with 'log' (text), 'traj' (parse_log) and 'sweeps'."""
    binary = binary or ref_build.BINARY
    if not os.path.isfile(binary):
        raise RefError("compiled reference not built: " + binary)
    d = keep or tempfile.mkdtemp(prefix="insider_ref_")
    try:
        _write_case(d, entry, scalars, arrays)
        env = dict(os.environ, OMP_THREAD_LIMIT=str(THREADS), OMP_NUM_THREADS=str(THREADS), OMP_DYNAMIC="false")
        try:
            r = subprocess.run([binary, d], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env,
                               timeout=timeout)
        except subprocess.TimeoutExpired:
            raise RefError("compiled reference: entry %s ran longer than %d s" % (entry, timeout))
        if r.returncode != 0:
            raise RefError("compiled reference: entry %s ended with status %d: %s" % (entry, r.returncode, r.stderr[-2000:]))
        out = _read_out(d)
        with open(os.path.join(d, "log.txt")) as f:
            out["log"] = f.read()
        out["traj"] = parse_log(out["log"])
        out["sweeps"] = int(out["sweeps"])
        return out
    finally:
        if keep is None:
            shutil.rmtree(d, ignore_errors=True)


# ---- one function per entry, with the argument order of oracle/c_oracle.py ---------------------------------------------------
def strong_cd(X, y, wstart, lam, alpha, XtX, Xty, tol=1e-5, **kw):
    """strong_coordinate_descent (src/coordinate_descent.cpp:56-127).  Returns (beta, sweeps)."""
    o = run_case("cd", dict(alpha=alpha, tol=tol, **{"lambda": lam}), dict(X=X, y=y, wstart=wstart, XtX=XtX, Xty=Xty), **kw)
    return o["beta"][:, 0], o["sweeps"]


def optimize_row(residual, M, A, Cmat, levels, gram, lam, tuning=1, **kw):
    o = run_case("row", dict(tuning=tuning, n_cores=10, **{"lambda": lam}),
                 dict(residual=residual, indicator=np.asarray(M, dtype=np.float64), factor=A, c_factor=Cmat,
                      confd=np.asarray(levels, dtype=np.uint32), gram=gram), **kw)
    return o["factor"]


def optimize_col(X, M, R, Cmat, lam, alpha, tuning=1, tol=1e-5, **kw):
    """Returns (c_factor, total sweeps)."""
    o = run_case("col", dict(alpha=alpha, tuning=tuning, n_cores=30, tol=tol, **{"lambda": lam}),
                 dict(residual=X, indicator=np.asarray(M, dtype=np.float64), row_factor=R, c_factor=Cmat), **kw)
    return o["c_factor"], o["sweeps"]


def optimize_continuous(data, M, u, Cmat, z, gram, lam, tuning=1, **kw):
    o = run_case("continuous", dict(tuning=tuning, **{"lambda": lam}),
                 dict(data=data, indicator=np.asarray(M, dtype=np.float64), u=np.asarray(u, dtype=np.float64).reshape(1, -1),
                      c_factor=Cmat, confd=z, gram=gram), **kw)
    return o["u"][0]


def state(X, R, A_list, Cmat, M_train, M_test, lam1, lam2, alpha, tuning, cd_residual, cd_beta, **kw):
    """predict, evaluate and both compute_loss (src/utils.cpp:46-102) on a fixed state."""
    arrays = dict(data=X, row_factor=R, column_factor=Cmat, train_indicator=np.asarray(M_train, dtype=np.float64),
                  test_indicator=np.asarray(M_test, dtype=np.float64), cd_residual=cd_residual, cd_beta=cd_beta)
    for i, a in enumerate(A_list):
        arrays["factor%d" % i] = a
    return run_case("state", dict(n_factors=len(A_list), tuning=tuning, lambda1=lam1, lambda2=lam2, alpha=alpha), arrays, **kw)


def optimize(X, levels, A_list, Cmat, M_train, M_test, lam1, lam2, alpha, tuning=1, global_tol=1e-10, sub_tol=1e-5,
             max_iter=10000, ctns=None, **kw):
    """optimize() (src/optimize.cpp:255-422).  Returns dict(row_matrices, column_factor, train_rmse, test_rmse (None under
    tuning = 0: the reference never writes it), loss, traj (LOG_COLS), iters (see below), total_sweeps, log)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    arrays = dict(data=X, column_factor=Cmat, levels=np.asarray(levels, dtype=np.uint32).reshape(n, -1),
                  train_indicator=np.asarray(M_train, dtype=np.float64), test_indicator=np.asarray(M_test, dtype=np.float64))
    for i, a in enumerate(A_list):
        arrays["factor%d" % i] = a
    if ctns is not None:
        arrays["ctns"] = np.asarray(ctns, dtype=np.float64).reshape(n, -1)
    sc = dict(n_factors=len(A_list), inc_continuous=0 if ctns is None else 1, latent_dim=np.asarray(Cmat).shape[0], lambda1=lam1,
              lambda2=lam2, alpha=alpha, tuning=tuning, global_tol=global_tol, sub_tol=sub_tol, max_iter=max_iter)
    o = run_case("optimize", sc, arrays, **kw)
    traj = o["traj"]
    last = int(traj[-1, 0])
    # a log that ends at a checkpoint with a further one still ahead shows the global_tol break (src/optimize.cpp:405), which
    # leaves the loop before iter++: the iteration count is then the last logged index, as the oracle reports it.  Otherwise
    # the log cannot tell a break at the last checkpoint from running out at max_iter; `iters` is None then.
    iters = last if (len(traj) > 1 and last + 10 <= max_iter) else None
    return dict(row_matrices=[o["factor%d" % i] for i in range(len(A_list))], column_factor=o["column_factor"],
                train_rmse=o["train_rmse"], test_rmse=o.get("test_rmse"), loss=o["loss"], traj=traj, iters=iters,
                total_sweeps=o["sweeps"], log=o["log"])
