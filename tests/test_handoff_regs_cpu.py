"""k_col_paircnt4 keeps three waves per SIMD: every launched instantiation within 168 registers, no spill, no scratch.

The kernel's grid and LDS are planned for three resident blocks of four waves per CU (paircnt_plan(), insider_plan.hpp).  The
form that makes Q and Qheld itself (<2, 4, 4, false, true>, option "stats_own_q") compiles to 166 registers, two below the
512 / 3 = 170 -> 168 a wave may hold at that occupancy; one more live value and it would run at two waves per SIMD with
nothing failing.  Read from the notes of the shipped code object, as tools/kernel_regs.sh does; needs no GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

from insider_amd import _lib
from tests.support import lib  # noqa: F401  (fixture: builds the library)

LLVM = "/opt/rocm/lib/llvm/bin"
# <NB, WPB, MAXS, ZC, OWNQ> as launch_paircnt() can launch them (MAXS = 8 with ZC is compiled, never launched)
LAUNCHED = [(nb, 4, ms, zc, own) for nb in (1, 2) for ms, zc, own in ((4, 0, 0), (8, 0, 0), (4, 1, 0), (4, 0, 1))]


def test_paircnt4_stays_at_three_waves_per_simd(tmp_path, lib):
    objdump, readelf = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    so = str(tmp_path / "libinsider_hip.so")
    shutil.copy(_lib.LIB_PATH, so)
    subprocess.run([objdump, "--offloading", so], cwd=str(tmp_path), check=True, capture_output=True)
    co = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert co, "no gfx950 code object in the library"
    notes = subprocess.run([readelf, "--notes", str(tmp_path / co[0])], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN7insider14k_col_paircnt4ILi(\d)ELi(\d)ELi(\d)ELb(\d)(?:ELb(\d))?EEE", name)
        if m:
            key = tuple(int(x) if x is not None else 0 for x in m.groups())
            found[key] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                          for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    for key in LAUNCHED:
        assert key in found, (key, sorted(found))
        f = found[key]
        print(key, f)
        assert f["vgpr_count"] <= 168, (key, f)
        assert f["vgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (key, f)
