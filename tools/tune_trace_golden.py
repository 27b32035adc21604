"""What api.tune() does around its fits, as one commit does it, for tests/test_tune_scheduler_cpu.py.
    python tools/tune_trace_golden.py [OUT.json]        (no GPU; default tests/golden/tune_trace_parent.json)
The committed file was written BEFORE tune()'s four schedulers (hold-out rank sweep, serial grid, concurrent grid, k-fold pool)
became one: the test replays every mode of MODES on the tree with the same stub handle and demands the same record.

The device fit is stubbed (Stub): optimize() logs (fold, K, lambda, alpha, key of the inits), adds 1 to its arguments in place
(a fold that saw another fold's arrays would log another key) and returns RMSEs that depend on all of them, and the factors.
Per mode the record holds the returned tables, every CSV's text, the generator's final state, stdout, the optimize() log, the
timings' warm_from sequence, key set and count.  Stdout and the log are sorted where several workers run."""
import contextlib
import io
import json
import os
import sys
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tune_trace_parent.json")

LAT, LAM, ALP = [3, 5], [1.0, 2.0, 3.0], [0.1, 0.3]
MODES = {
    "serial": dict(latent_dimension=LAT, lambda_=LAM, alpha=ALP),
    "concurrent3": dict(latent_dimension=LAT, lambda_=LAM, alpha=ALP, concurrent=3),
    "warm_start": dict(latent_dimension=LAT, lambda_=LAM, alpha=ALP, warm_start=True),
    "folds": dict(latent_dimension=LAT, lambda_=LAM, alpha=ALP, folds=True),
    "folds_concurrent2": dict(latent_dimension=LAT, lambda_=LAM, alpha=ALP, folds=True, concurrent=2),
    "rank_sweep_only": dict(latent_dimension=[3, 5, 4], lambda_=2.0, alpha=0.3),
    "grid_only": dict(latent_dimension=[4], lambda_=LAM, alpha=ALP),
}


class Stub:
    """Stands in for InsiderData.  ``trace``: dict(log=[], threads=[]) shared by every handle derived from this one; an optional
    trace["fail"] = {n: exception} makes the n-th optimize() (counted over all handles) raise it."""

    def __init__(self, trace, fold=0, src=None):
        self.trace, self.fold_no, self._h = trace, fold, True
        self._options = dict(src._options) if src is not None else {}

    def set_folds(self, ids, F):
        pass

    def fold(self, f):
        return type(self)(self.trace, f, self)

    def clone(self):
        return type(self)(self.trace, self.fold_no, self)

    def set_option(self, name, value):
        self._options[name] = float(value)

    def profile(self):
        return dict(wall_ms=0.0)

    def close(self):
        self._h = None

    def optimize(self, cfd, col, K, l1, l2, a, tuning, gt, st, iters, seed=None, inc_continuous=0, copy=True):
        key = float(sum(np.abs(x).sum() for x in cfd) + np.abs(col).sum())
        self.trace["log"].append([self.fold_no, int(K), float(l1), float(a), key])
        self.trace["threads"].append(threading.get_ident())
        if len(self.trace["log"]) in self.trace.get("fail", {}):
            raise self.trace["fail"][len(self.trace["log"])]
        for x in cfd:
            x += 1.0
        col += 1.0
        return dict(train_rmse=key + self.fold_no + 0.01 * K, test_rmse=key * (1 + self.fold_no) + l1 + a + 0.001 * K,
                    row_matrices={f"factor{i}": x for i, x in enumerate(cfd)}, column_factor=col)


def make_obj(folds=3):
    from insider_amd import api
    rng = np.random.default_rng(1)
    conf = np.column_stack([np.arange(40) % 4 + 1, np.arange(40) % 3 + 1])
    data = rng.standard_normal((40, 30))
    data[rng.random(data.shape) < 0.05] = np.nan
    with contextlib.redirect_stdout(io.StringIO()):
        return api.insider(data, conf, tuning_iter=3, seed=5, folds=folds)


def _plain(v):
    return v.tolist() if isinstance(v, np.ndarray) else v


def run_mode(name):
    """The record of one mode: see the module docstring."""
    from insider_amd import api
    kw = dict(MODES[name])
    kw["latent_dimension"] = np.array(kw["latent_dimension"])
    several = kw.get("concurrent", 1) > 1
    obj = make_obj(3 if kw.get("folds") else None)
    trace = dict(log=[], threads=[])
    obj["_resident_tune"] = Stub(trace)
    rng = np.random.default_rng(42)
    timings, stdout = [], io.StringIO()
    with tempfile.TemporaryDirectory() as d:
        with contextlib.redirect_stdout(stdout):
            out = api.tune(obj, rng=rng, timings=timings, out_dir=d, **kw)
        csv = {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}
    lines = stdout.getvalue().splitlines()
    state = rng.bit_generator.state
    return dict(tables={k: _plain(v) for k, v in sorted(out.items())}, csv=csv,
                rng_state=json.loads(json.dumps(state, default=int)),
                stdout=sorted(lines) if several else lines, log=sorted(trace["log"]) if several else trace["log"],
                warm_from=[t["warm_from"] for t in timings], timing_keys=sorted({k for t in timings for k in t}),
                timing_count=len(timings))


def main(path):
    sys.path.insert(0, ROOT)
    rec = {name: run_mode(name) for name in MODES}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(rec.items())) + "\n}\n")
    print(f"{len(rec)} modes -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
