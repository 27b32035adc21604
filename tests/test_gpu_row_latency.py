"""k_level_merged requests its global loads in batches ahead of its sums (insider_row_merged.hpp), and a fit's main stream
joins the side stream's C'C once per iteration.  (The cases of k_gene_u_cnt's earlier tables guard a batched form of that loop,
which was measured slower and is not in the tree: profiles/row_latency/README.md.)

Yardstick: the build before that change, bit for bit — every sum kept its order on its operands.  tests/golden/
row_latency_parent.npz holds what that build returned for every case of tools/row_latency_golden.py (written by that script on
the GPU at the parent commit): optimize_row() of every covariate and one optimize(max_iter = 2) per case, at the edges of the
new loops' chunks and batches.  Each case also names the row kernels it must have reached.
"""
import importlib.util
import os

import numpy as np
import pytest

from tests.support import need_gpu  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("row_latency_golden", os.path.join(os.path.dirname(HERE), "tools", "row_latency_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "row_latency_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def _keys(c):
    nfac = len(c["levels"]) + (1 if c["m"] else 0)
    return ([f"{c['id']}/row{i}" for i in range(nfac)] + [f"{c['id']}/fit_A{i}" for i in range(nfac)]
            + [f"{c['id']}/fit_{x}" for x in ("C", "traj", "loss")])


def test_golden_file_covers_every_case(golden):
    assert sorted(golden) == sorted(k for c in gen.CASES for k in _keys(c))
    ids = set(gen.CASE_BY_ID)
    # the edges the issue names: earlier-table level counts, both count widths, slab counts, stacked levels, K
    assert {f"gu-L{L}-rows4" for L in (1, 15, 16, 17, 128, 129, 257)} <= ids
    assert {f"gu-L{L}-rows17" for L in (17, 128, 129, 257)} <= ids
    assert {f"lm-p{p}" for p in (100, 1920, 2048, 2049, 4100, 65536, 65537)} <= ids
    assert {f"lm-SL{s}" for s in (1, 3, 4, 5, 63, 64, 65, 128, 129)} <= ids
    assert {f"lm-K{K}" for K in (1, 15, 16, 17, 30, 31, 32, 33, 63)} <= ids


@pytest.mark.parametrize("cid", list(gen.CASE_BY_ID))
def test_row_updates_and_fit_are_bit_identical_to_the_parent_build(golden, cid):
    c = gen.CASE_BY_ID[cid]
    got, names = gen.run(c)
    assert set(c["expect"]) <= names, (sorted(c["expect"]), sorted(names))
    assert sorted(got) == sorted(_keys(c))
    for k in sorted(got):
        assert got[k].dtype == golden[k].dtype and got[k].shape == golden[k].shape, k
        assert np.array_equal(got[k], golden[k], equal_nan=True), (k, int(np.sum(got[k] != golden[k])))
    assert np.isfinite(got[f"{cid}/fit_loss"][0])
