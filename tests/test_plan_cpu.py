"""The call plan (insider_amd/csrc/insider_plan.hpp) against the hand-written rules of tests/dispatch_rules.py, on the CPU.

tests/plan_driver.cpp includes the plan header and the header of shapes alone; it is built here with the host compiler and
fed the case lists of the GPU tests whose kernel path an option forces: the plan's answer must equal the hand rule, case by
case.  (Cases whose path the cost models pick need the padded entry counts of the device set-up: the GPU tests keep those.)
What the GPU tests add is the other half: that a launch helper launches what the plan says, reported at the launch.
Every group asserts that it compared as many cases as it listed.
"""
import os
import shutil
import subprocess

import pytest

from insider_amd import _lib
from tests import dispatch_rules as dr
from tests import test_gpu_col_solvers as t_solvers
from tests import test_gpu_col_stats as t_stats
from tests import test_gpu_loss_checkpoint as t_loss
from tests import test_gpu_row_update as t_rows
from tests import test_gpu_stream_products as t_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SIMD = 1024
# Options' defaults (insider_hip.hip), by PlanFacts name
DEFAULTS = dict(row_merged=1, col_factored=1, row_fused=1, row_gemm=1, row_counts=1, mm_fast=1, force_allreduce=0, wg_waves=1024,
                list_fine=1, mm_tiles=0, col_mfma4=1, cd_variant=0, cd_pairs=1, cd_cold_iters=3, cd_pass_first=64,
                cd_pass_ratio=4, max_sweeps=1 << 24)
OPTION_NAME = {"cd_pass1": "cd_pass_first", "row_gemm_waves": "wg_waves"}     # set_option's name -> the member's


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip("no host C++ compiler found (g++, c++, clang++ or $CXX): the plan driver cannot be built")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(ROOT, "tests", "plan_driver.cpp")])
    return exe


def facts(K, opts=None, **kw):
    """One driver line: the workspace's geometry for K as ensure_workspace() sets it, the options, then the given facts."""
    NB = dr.nb_of(K)
    f = dict(K=K, NB=NB, KP=16 * NB, lvl_zero=1, fperm=int(NB == 2 and K >= 16), n_simd=N_SIMD, world=1)
    o = dict(DEFAULTS)
    for k, v in (opts or {}).items():
        k = OPTION_NAME.get(k, k)
        assert k in o, k
        o[k] = max(64, int(v)) if k == "wg_waves" else int(v)
    f.update(kw)
    toks = [f"opt.{k}={v}" for k, v in o.items()]
    for k, v in f.items():
        if isinstance(v, (list, tuple)):
            v = ",".join(f"{x[0]}:{x[1]}" if isinstance(x, tuple) else str(x) for x in v)
        elif isinstance(v, float):
            v = repr(v)
        else:
            v = int(v)
        toks.append(f"{k}={v}")
    return " ".join(toks)


def plans(driver, lines):
    """The plan of every line, as a dict of strings; lists split."""
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [dict(tok.split("=", 1) for tok in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == len(lines), (len(rows), len(lines))
    for r in rows:
        for k in ("pass_limit", "u_cnt", "reduce", "v_nt", "wg"):
            r[k] = [x for x in r[k].split(",") if x]
    return rows


def data_set(levels, m, p, n, merged, pair, cont):
    """The facts of a data set with these covariates: merged tables, dense pair counts (with their static half counts),
    real-valued counts of the continuous columns."""
    levels = list(levels)
    c, SLcat = len(levels), sum(levels)
    SL = SLcat + m
    f = dict(c=c, m=m, L=levels, SLcat=SLcat, SL=SL, SLP=SL + SL % 2, p=p, n=n, merged=merged, cont_merged=cont, cf_pair_ok=pair,
             cf_hn=pair, cf_zt=cont)
    if c <= dr.CF_MAXC:   # the factored statistics' static part, positions by decreasing level count
        tab_rows = SLcat - max(levels)
        f.update(cf_c=c, cf_tab_rows=tab_rows, cf_nsteps=(tab_rows + 3) // 4,
                 cf_L=sorted(levels, reverse=True) + ([m] if cont else []),
                 cf_nlater=[c - 1 - t for t in range(c)] + ([0] if cont else []))
    return f


# ----------------------------------------------------------------------------------------------------------------------
# the column solve: solver, evaluation kernel, ridge fallback, order table; the batch entry
# ----------------------------------------------------------------------------------------------------------------------
def test_column_solver_every_cell(driver):
    cells = list(dict.fromkeys(t_solvers.CELLS + t_loss.CELLS))
    assert len(cells) >= len(t_solvers.CELLS) and {K for _, _, K in cells} >= {1, 16, 17, 32, 33, 48, 49, 63}
    lines = []
    for r, v, K in cells:
        lam, alpha = dr.REGIMES[r]
        lines.append(facts(K, dict(cd_variant=v), alpha=alpha, la=lam * alpha))
    compared = 0
    for (r, v, K), plan in zip(cells, plans(driver, lines)):
        got = _lib.COL_SOLVERS[int(plan["col_solver"])]
        want = dr.col_solver(r, v, K)
        assert got == want, (r, v, K, got, want)
        assert _lib.COL_SOLVERS[int(plan["col_eval"])] == dr.col_eval(want), (r, v, K)
        assert int(plan["ridge_fallback"]) == (want == "ridge_reg"), (r, v, K)
        # rows of 64 row offsets for K > 32 unless the register-resident kernel reads its successor list
        assert int(plan["order_wide"]) == (K > 32 and want != "cd_reg3"), (r, v, K)
        compared += 1
    assert compared == len(cells)


def test_batch_entry_solver(driver):
    """insider_hip_strong_cd: cd_solver() with the default cd_variant, K up to 64 (test_strong_cd_batch_every_solver's cells)."""
    coeff = {"alpha0": (3.0, 0.0), "lambda0": (0.0, 0.5), "enet": (0.7, 0.6)}
    cells = list(t_solvers.BATCH) + [(r, K) for K, r in t_solvers.CHUNKED]
    assert ("alpha0", 64) in cells and ("lambda0", 64) in cells
    lines = [f"K={K} batch=1 alpha={coeff[r][1]!r} la={coeff[r][0] * coeff[r][1]!r}" for r, K in cells]
    compared = 0
    for (r, K), plan in zip(cells, plans(driver, lines)):
        want = dr.col_solver("enet" if r == "enet" else "nol1", 0, K)
        assert _lib.COL_SOLVERS[int(plan["batch_solver"])] == want, (r, K)
        compared += 1
    assert compared == len(cells)


def test_cold_pass_limits(driver):
    period = dr.PERM_PERIOD
    cells = [(first, ratio, ms, iters) for first in (0, 31, 32, 64) for ratio in (1, 4)
             for ms in (1000, 4 * period - 1, 4 * period, 4 * period + 1, 1 << 24) for iters in (3, 9)]
    lam, alpha = dr.REGIMES["enet"]
    lines = [facts(9, dict(cd_pass1=first, cd_pass_ratio=ratio, max_sweeps=ms, cd_cold_iters=iters), alpha=alpha, la=lam * alpha)
             for first, ratio, ms, iters in cells]
    compared = 0
    for (first, ratio, ms, iters), plan in zip(cells, plans(driver, lines)):
        want = dr.pass_limits(first, ratio, ms)
        assert [int(x) for x in plan["pass_limit"]] == want, (first, ratio, ms)
        assert int(plan["npass"]) == len(want)
        assert int(plan["cold_iters"]) == (iters if first >= 32 else 0), (first, iters)
        compared += 1
    assert compared == len(cells)
    assert dr.pass_limits(64, 4, 1 << 24) == [64, 256, 1024, 4096, 16384] and dr.pass_limits(64, 1, 1000) == [64, 128, 256, 512]
    # the group kernels solve in one pass whatever the options
    plan, = plans(driver, [facts(9, dict(cd_variant=1), alpha=alpha, la=lam * alpha)])
    assert plan["pass_limit"] == [] and int(plan["cold_iters"]) == 0


# ----------------------------------------------------------------------------------------------------------------------
# the column statistics
# ----------------------------------------------------------------------------------------------------------------------
def test_column_statistics_forced_paths(driver):
    # (with continuous covariates the path follows from the data set's tables alone: those cases are compared too)
    cases = [c for c in t_stats.CASES + t_stats.STALE + t_stats.FITS if c["opts"].get("col_factored") in (0, 2, 3) or c["m"] > 0]
    assert len(cases) == len(t_stats.CASES + t_stats.STALE + t_stats.FITS) - len(t_stats.COST)
    lines = []
    for c in cases:
        merged, tab_rows, nsteps, pair_ok, zt = t_stats.structure(c)
        f = data_set(c["levels"], c["m"], c["p"], c["n"], merged, pair_ok, zt)
        assert c["m"] > 0 or len(c["levels"]) > dr.CF_MAXC or (f["cf_tab_rows"], f["cf_nsteps"]) == (tab_rows, nsteps)
        lines.append(facts(c["K"], {**dr.COL_OPTS, **c["opts"]}, masked=1, **f))
    compared, reached = 0, set()
    for c, plan in zip(cases, plans(driver, lines)):
        path = int(plan["col_path"])
        kernel = ("list4" if int(plan["list4"]) else "list") if path == 0 else "factored" if path == 1 else \
            _lib.COL_STATS_KERNELS[int(plan["pc_kernel"])]
        tickets, blocks = int(plan["pc_parts"]), int(plan["pc_blocks"])
        assert (kernel, tickets) == t_stats.expected(c), (c["id"], kernel, tickets, t_stats.expected(c))
        dr.check_pc4_blocks(c, kernel, tickets, blocks)
        reached.add(kernel)
        compared += 1
    assert compared == len(cases)
    assert reached == set(_lib.COL_STATS_KERNELS) - {"none"}, sorted(reached)


def test_list_form(driver):
    cells = [(K, fine, fperm) for K in (15, 16, 31, 32) for fine in (1, 0) for fperm in (1, 0)]
    lines = [facts(K, dict(list_fine=fine), fperm=fperm) for K, fine, fperm in cells]
    compared = 0
    for (K, fine, fperm), plan in zip(cells, plans(driver, lines)):
        assert ("list4" if int(plan["list4"]) else "list") == dr.list_form(K, fine, bool(fperm)), (K, fine, fperm)
        compared += 1
    assert compared == len(cells)
    assert [dr.list_form(K) for K in (15, 16, 31, 32)] == ["list", "list4", "list4", "list"]


# ----------------------------------------------------------------------------------------------------------------------
# the streaming products
# ----------------------------------------------------------------------------------------------------------------------
def test_streaming_products(driver):
    MR = {"0": None, "2": 2, "4": 4}
    levels_of = lambda SL: (SL - 3, 3)                                   # (test_gpu_stream_products.py's two covariates)
    cells = [(5, 37, p, mm, 0) for p in (16383, 16384) for mm in (0, 1, 2)]
    # the LDS edge of the staged factors for every NB: the last SL with ceil(SL / 16) NB <= 32 fits, the next does not
    for K, SL in t_stream.FIT_EDGE.items():
        assert -(-SL // 16) * dr.nb_of(K) <= 32 < -(-(SL + 1) // 16) * dr.nb_of(K)
        cells += [(K, s, p, 1, 0) for s in (SL, SL + 1) for p in (16383, 16384)]
    # tiles per wave: the option, and the natural rule at 4 n_simd + 4 tiles
    cells += [(5, 37, t_stream.P_TILES, 1, t) for t in (0, 2, 3, 5, 7)] + [(5, 13, 16 * (4 * N_SIMD + 3) + 5, 1, 0)]
    LS = (1, 16, 17, 32, 33, 48, 130)
    lines = []
    for K, SL, p, mm, mt in cells:
        f = data_set(levels_of(SL), 0, p, 48, True, False, False)
        lines.append(facts(K, dict(mm_fast=mm, mm_tiles=mt), sites=[(p, L) for L in LS], vn=list(LS), **f))
    compared = 0
    for (K, SL, p, mm, mt), plan in zip(cells, plans(driver, lines)):
        assert (2 if int(plan["q_rows2"]) else 1) == dr.q_kernel(K, SL, p, mm), (K, SL, p, mm)
        assert int(plan["v_rows2"]) == bool(mm and p >= dr.MM_FAST_MIN), (K, p, mm)
        assert int(plan["mm_tpw"]) == dr.tiles(p, N_SIMD, mt), (p, mt)
        for L, form, nt in zip(LS, plan["reduce"], plan["v_nt"]):
            want = dr.reduce2_form(K, L, p, mm)
            assert MR[form] == (want[1] if want else None) and (want is None or want[0] == int(plan["NB"])), (K, L, p, mm)
            assert int(nt) == dr.v_nt(L)[0], L
        compared += 1
    assert compared == len(cells)
    assert dr.tiles(16 * (4 * N_SIMD + 3) + 5, N_SIMD) == 2


# ----------------------------------------------------------------------------------------------------------------------
# the row update
# ----------------------------------------------------------------------------------------------------------------------
def plan_row_kernels(plan, case, cov, reduce_site):
    """The forms optimize_row() launches for a plan: row_update()'s switch (insider_hip.hip), form by form.  reduce_site: the
    index of this covariate's U'C among the sites asked."""
    c = len(case["levels"])
    cont, masked = cov >= c, case["tuning"] == 1
    merged, fused = int(plan["merged"]), int(plan["fused_solve"]) and not cont
    reduce = {"0": "mm_reduce", "2": "mm_reduce2_2", "4": "mm_reduce2_4"}[plan["reduce"][reduce_site]]
    s = set()
    if merged:
        s.add("mm_rows2" if int(plan["v_rows2"]) else "mm_rows")
    if cont and merged:
        s |= {"gene_uc", reduce, "merged"} | (set() if case["no_heldout"] else {"wsyrk"})
    elif merged:
        s |= {"gene_u_cnt" if int(plan["u_cnt"][cov]) else "gene_u", reduce}
        use, tiles, LT, zch = (int(x) for x in plan["wg"][cov].split(":")[:4])
        if use:
            s |= {f"wgemm{LT}"} | ({"wgemm_chunks"} if zch > 1 else set())
        elif not case["no_heldout"]:
            s.add("wsyrk")
        s.add(("merged_solve" if fused else "merged") if int(plan["row_fused"]) else "pack_reduce")
    elif not cont and int(plan["unmasked_fused"]):
        s |= {"merged_solve" if fused else "merged", "merged_zero"}
    else:
        s.add("level_partial")
        if masked:
            s.add("list_stats4" if int(plan["list4"]) else "list_stats")
    if not fused:
        s.add("cont_cd" if cont and masked else "level_solve")
    return s


def test_row_update_forced_paths(driver):
    cases = [c for c in t_rows.CASES + list(t_rows.FITS.values()) if c["opts"].get("row_merged") in (0, 2)]
    assert len(cases) > 100
    lines = []
    for c in cases:
        tables, pair, cont_merged = dr.row_structure(c)
        f = data_set(c["levels"], c["m"], c["p"], c["n"], tables, pair, cont_merged)
        sites = [(c["p"], L) for L in c["levels"]] + [(c["p"], 1)] * c["m"]
        lines.append(facts(c["K"], {**dr.ROW_OPTS, **c["opts"]}, masked=c["tuning"], sites=sites, **f))
    compared = 0
    for c, plan in zip(cases, plans(driver, lines)):
        ncov = len(c["levels"]) + c["m"]
        for cov in (c["covs"] if c["covs"] is not None else range(ncov)):
            got, want = plan_row_kernels(plan, c, cov, cov), dr.row_kernels(c, cov)
            assert got == want, (c["id"], cov, sorted(got), sorted(want))
            compared += 1
    assert compared == sum(len(c["covs"]) if c["covs"] is not None else len(c["levels"]) + c["m"] for c in cases)
