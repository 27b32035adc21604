"""tune()'s scheduler (api._fit_points), host side, with the device fit stubbed out (no GPU).

tests/golden/tune_trace_parent.json holds what tune() did around its fits in seven modes when the hold-out rank sweep, the serial
grid, the concurrent grid and the k-fold pool were four schedulers (tools/tune_trace_golden.py wrote it at that commit): the
tables, the CSVs, the generator's final state, stdout, the optimize() calls.  The one scheduler must reproduce all of it; what
it changes on purpose — the timing dicts — is asserted by hand."""
import importlib.util
import json
import os
import threading

import numpy as np
import pytest

from insider_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("tune_trace_golden", os.path.join(os.path.dirname(HERE), "tools", "tune_trace_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(HERE, "golden", "tune_trace_parent.json")) as _f:
    PARENT = json.load(_f)
HOLD_OUT_KEYS = {"lambda_", "alpha", "init_s", "init_wait_s", "warm_from", "optimize_s", "library_ms"}


def test_the_fixture_covers_the_modes():
    assert set(PARENT) == set(gen.MODES) and len(gen.MODES) == 7


@pytest.mark.parametrize("mode", sorted(gen.MODES))
def test_tune_does_what_the_four_schedulers_did(mode):
    want = PARENT[mode]
    got = json.loads(json.dumps(gen.run_mode(mode)))        # through JSON, like the fixture: tuples -> lists, floats exact
    for field in ("tables", "csv", "rng_state", "stdout", "log"):
        assert got[field] == want[field], field
    kw = gen.MODES[mode]
    folds = bool(kw.get("folds"))
    n_rank = len(kw["latent_dimension"]) if len(kw["latent_dimension"]) > 1 else 0
    # the timing dicts: one per fitted (point, fold), the rank sweep included; every one carries latent_rank, `fold` only with folds
    assert got["timing_count"] == len(got["log"]) > 0
    assert set(got["timing_keys"]) == HOLD_OUT_KEYS | {"latent_rank"} | ({"fold"} if folds else set())
    assert set(got["timing_keys"]) >= set(want["timing_keys"])
    if folds:
        assert got["warm_from"] == want["warm_from"] and got["timing_count"] == want["timing_count"]
    else:                                                   # the rank sweep's points come first and start cold
        assert got["warm_from"] == [None] * n_rank + want["warm_from"]
        assert got["timing_count"] == n_rank + want["timing_count"]
    if mode == "warm_start":
        assert any(w is not None for w in got["warm_from"])


def _stubbed(folds=None, fail=None):
    obj = gen.make_obj(folds)
    trace = dict(log=[], threads=[], fail=fail or {})
    obj["_resident_tune"] = gen.Stub(trace)
    return obj, trace


def _tune_in_a_thread(obj, **kw):
    """tune() on a helper thread, joined for 60 s: -> (what it raised or "returned", the helper's ident, threads left over)."""
    before = threading.active_count()
    box = {}

    def run():
        box["ident"] = threading.get_ident()
        try:
            api.tune(obj, rng=np.random.default_rng(42), **kw)
            box["out"] = "returned"
        except BaseException as e:
            box["out"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(timeout=60)
    assert not t.is_alive(), "tune() hangs"
    return box["out"], box["ident"], threading.active_count() - before


@pytest.mark.parametrize("folds", [None, 3], ids=["hold_out", "folds"])
def test_serial_fits_run_on_the_calling_thread(folds):
    obj, trace = _stubbed(folds)
    out, ident, left = _tune_in_a_thread(obj, latent_dimension=np.array([3, 5]), lambda_=gen.LAM, alpha=gen.ALP,
                                         folds=True if folds else None)
    assert out == "returned" and left == 0
    assert len(trace["threads"]) == (folds or 1) * (2 + 6) and set(trace["threads"]) == {ident}


def test_an_interrupt_ends_a_serial_tune_cleanly():
    stop = KeyboardInterrupt()
    obj, trace = _stubbed(fail={2: stop})
    lam = [float(v) for v in range(1, 9)]
    out, _, left = _tune_in_a_thread(obj, latent_dimension=np.array([4]), lambda_=lam, alpha=[0.1, 0.3])      # a 16-point grid
    assert out is stop
    assert left == 0, "a thread of tune() outlives the call"
    assert len(trace["log"]) == 2                           # nothing was fitted after the interrupt


@pytest.mark.parametrize("kw", [dict(concurrent=3), dict(folds=True, concurrent=2)], ids=["concurrent3", "folds_concurrent2"])
def test_a_failing_fit_in_a_worker_thread_ends_tune_cleanly(kw):
    """The first fit that runs on another thread than the caller's raises: tune() raises that exception, no thread is left."""
    boom = RuntimeError("the fit failed")

    class _FailsOffTheCallingThread(gen.Stub):
        def optimize(self, *a, **k):
            if threading.get_ident() != self.trace["caller"] and not self.trace.setdefault("raised", False):
                self.trace["raised"] = True
                raise boom
            return super().optimize(*a, **k)

    obj = gen.make_obj(3 if kw.get("folds") else None)
    trace = dict(log=[], threads=[])
    obj["_resident_tune"] = _FailsOffTheCallingThread(trace)
    lam = [float(v) for v in range(1, 9)]
    before = threading.active_count()
    box = {}

    def run():
        trace["caller"] = threading.get_ident()
        try:
            api.tune(obj, rng=np.random.default_rng(42), latent_dimension=np.array([4]), lambda_=lam, alpha=[0.1, 0.3], **kw)
            box["out"] = "returned"
        except BaseException as e:
            box["out"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(timeout=60)
    assert not t.is_alive(), "tune() hangs after a fit failed in a worker thread"
    assert box["out"] is boom and trace["raised"]
    assert threading.active_count() == before, "a thread of tune() outlives the call"


def test_options_reach_the_fold_handles_and_their_clones():
    class _FoldHandlesWait(gen.Stub):
        """With concurrent=2 worker 0 fits on the fold handles, worker 1 on its clones of them.  A fit on a fold handle waits
        until the clones have fitted every fold, so after each tune() worker 1 has made (or met again) all three of its clones."""
        is_clone = False

        def clone(self):
            hd = super().clone()
            hd.is_clone = True
            return hd

        def optimize(self, *a, **k):
            if self.is_clone:
                self.trace["seen"].add(self.fold_no)
                if self.trace["seen"] == {1, 2, 3}:
                    self.trace["covered"].set()
            else:
                assert self.trace["covered"].wait(timeout=60)
            return super().optimize(*a, **k)

    trace = dict(log=[], threads=[], seen=set(), covered=threading.Event())
    obj = gen.make_obj(3)
    obj["_resident_tune"] = _FoldHandlesWait(trace)
    grid = dict(latent_dimension=np.array([3, 5]), lambda_=gen.LAM, alpha=gen.ALP, folds=True, concurrent=2)
    first = api.tune(obj, rng=np.random.default_rng(42), **grid)
    handles, clones = list(obj["_fold_handles"]), dict(obj["_fold_clones"])
    assert len(handles) == 3 and sorted(clones) == [(1, 0), (1, 1), (1, 2)]
    obj["_resident_tune"].set_option("cd_pass1", 128)
    again = api.tune(obj, rng=np.random.default_rng(42), **grid)
    assert obj["_fold_handles"] == handles and obj["_fold_clones"] == clones            # the same handles, kept
    for hd in handles + list(clones.values()):
        assert hd._h and hd._options.get("cd_pass1") == 128.0
    np.testing.assert_array_equal(again["reg_tuning"], first["reg_tuning"])
    # a closed clone is replaced, and the new one carries the option too
    clones[(1, 1)].close()
    trace["seen"].clear()
    trace["covered"].clear()
    api.tune(obj, rng=np.random.default_rng(42), **grid)
    assert sorted(obj["_fold_clones"]) == sorted(clones) and obj["_fold_clones"][(1, 1)] is not clones[(1, 1)]
    assert all(hd._h and hd._options.get("cd_pass1") == 128.0 for hd in obj["_fold_clones"].values())
