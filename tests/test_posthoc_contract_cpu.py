"""Every post-hoc entry point is declared in include/insider_hip.h, listed in _lib.SYMBOLS and exported by the library, its
kernel header feeds the source hash, and the sizes the Python layer repeats are the kernels' own.  One row of CALLS per call;
a row holds exactly the checks its call needs, and a field it lacks is not checked for it."""
import ctypes as C
import os
import re

import pytest

from insider_amd import _build, _lib, api
from tests.support import lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET = object()        # a restype that only has to be declared

# symbols: the first is the call, declared "int name(" in the header, the others as ``header`` spells them out
# keys: info / option names the header documents; argtypes: of the call; restype: of the stopwatch (the second symbol)
# sources: files that must be in _build.source_files(); constants: (kernel header, regexes in it, (module, name), value)
CALLS = {
    "variance_decomposition": dict(symbols=("insider_hip_variance_decomposition",)),
    "sample_decomposition": dict(symbols=("insider_hip_sample_decomposition",)),
    "factor_decomposition": dict(symbols=("insider_hip_factor_decomposition",), keys=("fd_path",)),
    "level_scores": dict(symbols=("insider_hip_level_scores",), keys=("ls_path", "ls_slabs", "ls_part_mb"), argtypes=11),
    "outliers": dict(symbols=("insider_hip_outliers",), keys=("ol_path",), constants=(
        ("insider_outliers.hpp", (r"OL_WAVES = 4;", r"OL_SPL = 4;"), (_lib, "OL_TRIP"), 64 * 4 * 4),
        ("insider_outliers.hpp", (r"OL_SCAN_THREADS = 256, OL_SCAN_ITEMS = 4;",), (_lib, "OL_SCAN_CHUNK"), 256 * 4))),
    "residual_products": dict(symbols=("insider_hip_residual_products",), keys=("rc_slabs", "rc_ms"),
                              sources=("insider_rescomp.hpp",)),
    "neighbors": dict(symbols=("insider_hip_neighbors", "insider_hip_last_neighbors_ms"),
                      header=(r"\bdouble insider_hip_last_neighbors_ms\s*\(\s*void\s*\)",), argtypes=11, restype=SET,
                      sources=("insider_neighbors.hpp",),
                      constants=(("insider_neighbors.hpp", (r"NN_MAX_TOPK = 64;",), (api, "NEIGHBOR_MAX_K"), 64),)),
    "kmeans": dict(symbols=("insider_hip_kmeans", "insider_hip_last_kmeans_ms"),
                   header=(r"\bdouble insider_hip_last_kmeans_ms\s*\(\s*void\s*\)",), argtypes=21, restype=C.c_double,
                   sources=("insider_kmeans.hpp",),
                   constants=(("insider_kmeans.hpp", (r"KM_MAX_K = 4096;",), (api, "KMEANS_MAX_K"), 4096),)),
    "enrichment": dict(symbols=("insider_hip_enrichment", "insider_hip_last_enrichment_ms", "insider_hip_enrichment_sample"),
                       header=(r"\bdouble insider_hip_last_enrichment_ms\s*\(\s*void\s*\)",
                               r"\bint insider_hip_enrichment_sample\s*\("), argtypes=16, restype=C.c_double,
                       sources=("insider_enrich.hpp", "insider_sample.h"),
                       constants=(("insider_enrich.hpp", (r"GS_MAX_SET = 4096;",), (api, "ENRICH_MAX_SET"), 4096),)),
}


@pytest.mark.parametrize("call", CALLS)
def test_symbols_are_declared_listed_and_exported(lib, call):
    row = CALLS[call]
    hdr = open(os.path.join(ROOT, "include", "insider_hip.h")).read()
    first = row["symbols"][0]
    for rx in (rf"\bint {first}\s*\(",) + row.get("header", ()):
        assert re.search(rx, hdr), rx
    for key in row.get("keys", ()):
        assert f'"{key}"' in hdr, key
    for name in row["symbols"]:
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None, name
    if "argtypes" in row:
        assert len(getattr(lib, first).argtypes) == row["argtypes"]
    if "restype" in row:
        restype = getattr(lib, row["symbols"][1]).restype
        assert restype is not None if row["restype"] is SET else restype is row["restype"]
    files = [os.path.basename(f) for f in _build.source_files()]
    for name in row.get("sources", ()):
        assert name in files, name                     # the kernel header feeds the library's source hash
    for source, regexes, (module, name), value in row.get("constants", ()):
        src = open(os.path.join(ROOT, "insider_amd", "csrc", source)).read()
        for rx in regexes:
            assert re.search(rx, src), rx
        assert getattr(module, name) == value, name    # the size the tests take from Python is the kernel's own
