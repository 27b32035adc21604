"""The K <= 30 sweep kernels apply a sweep's coefficient increments once, in the sweep's exit block (insider_cd_reg.hpp).

Yardstick: the build before that change, bit for bit.  tests/golden/cd_deferred_parent.npz holds what that build returned from
the batch entry for every case of tools/cd_deferred_golden.py (written by that script on the GPU at the parent commit); the same
instruction on the same operands per lane must give the same solutions and sweep counts.  Alongside: the CPU oracle at the
tolerances of tests/test_gpu_col_solvers.py, and at fit level the two routings of a sweep (one step per block, blocks of two
steps) and the multi-pass solve against the single-pass one at an odd K.
"""
import importlib.util
import os

import numpy as np
import pytest

from insider_amd import _lib, api, workloads
from tests.support import need_gpu, relerr  # noqa: F401  (need_gpu: autouse fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("cd_deferred_golden", os.path.join(os.path.dirname(HERE), "tools", "cd_deferred_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "cd_deferred_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_golden_file_covers_every_case(golden):
    keys = [c[0] for K in gen.KS for c in gen.cases(K)]
    assert len(keys) == len(gen.KS) * len(gen.BS) * len(gen.REGIMES) * len(gen.MODES) * len(gen.CAPS) == 192
    assert sorted(golden) == sorted([k + "_beta" for k in keys] + [k + "_sweeps" for k in keys])


@pytest.mark.parametrize("regime", list(gen.REGIMES))
@pytest.mark.parametrize("K", gen.KS)
def test_batch_entry_is_bit_identical_to_the_parent_build(oracle, golden, K, regime):
    uneven = False
    for key, B, reg, lam, alpha, mode, cap, P in gen.cases(K):
        if reg != regime:
            continue
        Xs, ys, Gs, qs, ws = P
        assert not Gs[gen.ZERO_PROBLEM][:, K // 2].any()                   # the all-zero Gram column
        beta, sw = gen.solve(lam, alpha, mode, cap, P)
        assert _lib.COL_SOLVERS[_lib.load().insider_hip_last_cd_solver()] == "cd_reg", key
        # the oracle first: a wrong solve should say so in numbers, not only "different bits"
        for b in range(B):
            ob, osw = oracle.strong_cd(Xs[b], ys[b], ws[b], lam, alpha, Gs[b], qs[b], tol=gen.TOL, seed=5, unit=b, it=3,
                                       order_mode=mode, max_sweeps=cap)
            if cap != gen.UNCAPPED:   # a solve that leaves at the bound, directly after one sweep too, returns the updated beta
                assert sw[b] == osw, (key, b, sw[b], osw)
                assert np.max(np.abs(ob - beta[b])) < 1e-10 * max(1.0, np.max(np.abs(ob))), (key, b)
            else:
                assert abs(osw - sw[b]) <= 1, (key, b, osw, sw[b])
                assert np.max(np.abs(ob - beta[b])) < (1e-9 if osw == sw[b] else 50 * np.sqrt(gen.TOL)), (key, b)
                assert np.array_equal(ob == 0, beta[b] == 0), (key, b)
        assert np.array_equal(sw, golden[key + "_sweeps"]), (key, np.nonzero(sw != golden[key + "_sweeps"]))
        assert np.array_equal(beta, golden[key + "_beta"]), (key, np.nonzero((beta != golden[key + "_beta"]).any(1)))
        if cap == gen.UNCAPPED and B == 33:
            assert (beta == 0).any() and (beta != 0).any(), key             # exact zeros next to moving coordinates
            quads = np.asarray(sw[:32]).reshape(8, 4)                        # wave w solves problems 4 w ... 4 w + 3
            uneven = uneven or bool((quads.min(1) != quads.max(1)).any())
    assert uneven      # parking beside running wave-mates: some wave holds genes with different sweep counts


# ----------------------------------------------------------------------------------------------------------------------
# fit level, at an odd K under KMAX = 30
# ----------------------------------------------------------------------------------------------------------------------
FIT = dict(tuning=1, max_iter=4, sub_tol=1e-11, seed=9)
PASS1 = 32


def _cp(w):
    return [a.copy(order="F") for a in w.A0], w.C0.copy(order="F")


@pytest.fixture(scope="module")
def fits():
    """One workload, three fits: the default (blocks of two steps, single pass), one step per block, multi-pass."""
    w = workloads.small(K=29, n=120, p=333, f=0.2, seed=29)
    ds = api.InsiderData(w.X, w.levels, w.M_train, w.M_test)
    ds.set_option("profile", 1)
    ds.set_option("cd_pass1", 0)
    ds.optimize(*_cp(w), w.K, w.lam, w.lam, w.alpha, **dict(FIT, max_iter=0))
    cold_max = int(ds.sweeps().max())
    out = {"w": w, "cold_max": cold_max}

    def fit(name):
        r = ds.optimize(*_cp(w), w.K, w.lam, w.lam, w.alpha, **FIT)
        out[name] = (r, ds.sweeps().copy(), ds.profile()["sweeps"])

    fit("base")
    ds.set_option("cd_pairs", 0)
    fit("single_blocks")
    ds.set_option("cd_pairs", 1)
    ds.set_option("cd_cold_iters", 100)
    ds.set_option("cd_pass1", PASS1)
    ds.set_option("cd_pass_ratio", 2)
    fit("multipass")
    ds.close()
    return out


def _same_fit(fits, name):
    w = fits["w"]
    (a, sw_a, tot_a), (b, sw_b, tot_b) = fits["base"], fits[name]
    assert a["iters"] == b["iters"]
    assert np.array_equal(a["column_factor"], b["column_factor"])
    assert np.array_equal(a["traj"], b["traj"], equal_nan=True)
    for i in range(len(w.A0)):
        assert np.array_equal(a["row_matrices"][f"factor{i}"], b["row_matrices"][f"factor{i}"]), i
    assert np.array_equal(sw_a, sw_b) and tot_a == tot_b


def test_one_step_blocks_and_two_step_blocks_give_the_same_fit(fits):
    _same_fit(fits, "single_blocks")


def test_multipass_fit_is_bit_identical_at_odd_k(fits):
    assert fits["cold_max"] > PASS1 + 16, fits["cold_max"]     # the first pass really stops solves half-way
    _same_fit(fits, "multipass")


def test_fit_matches_oracle(oracle, fits):
    w = fits["w"]
    got, _, total = fits["multipass"]
    ref = oracle.optimize(w.X, w.levels, w.n_levels, w.A0, w.C0, w.M_train, w.M_test, w.lam, w.lam, w.alpha, **FIT)
    assert relerr(got["column_factor"], ref["column_factor"]) < 1e-6
    assert abs(total - ref["total_sweeps"]) <= max(3, 0.002 * ref["total_sweeps"])
