"""Recipe of the compiled reference: oracle/_ref/insider_ref.

The reference's own translation units are compiled UNMODIFIED, from where they lie, against the stand-in headers of
oracle/ref_shim (ahead of every other include path) and linked with oracle/ref_driver.cpp.  Nothing of the reference is
copied, patched or generated; RcppExports.cpp (R glue) is not compiled.  oracle/_ref/ is ignored by git.

The reference tree is looked for in $INSIDER_REFERENCE, then in a directory `reference` beside the repository.
"""
import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
OUT_DIR = os.path.join(_HERE, "_ref")
BINARY = os.path.join(OUT_DIR, "insider_ref")
BINARY_SAN = os.path.join(OUT_DIR, "insider_ref_san")
UNITS = ("src/optimize.cpp", "src/coordinate_descent.cpp", "src/utils.cpp", "src/fit_interaction.cpp")
OWN = (os.path.join(_HERE, "ref_driver.cpp"), os.path.join(_HERE, "ref_shim", "RcppArmadillo.h"), os.path.abspath(__file__))


def reference_dir():
    for d in (os.environ.get("INSIDER_REFERENCE"), os.path.join(os.path.dirname(ROOT), "reference")):
        if d and all(os.path.isfile(os.path.join(d, u)) for u in UNITS):
            return d
    return None


def compiler():
    return shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")


def available():
    return os.path.isfile(BINARY) and os.access(BINARY, os.X_OK)


def build(force=False, sanitize=False, quiet=True):
    """Returns the binary's path, or None when the reference tree or a C++ compiler is missing (silently)."""
    ref, cxx = reference_dir(), compiler()
    if ref is None or cxx is None:
        return None
    out = BINARY_SAN if sanitize else BINARY
    srcs = [os.path.join(ref, u) for u in UNITS] + [OWN[0]]
    deps = srcs + list(OWN[1:]) + [os.path.join(ref, "inst", "include", "insider_types.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-std=c++11", "-fopenmp", "-I", os.path.join(_HERE, "ref_shim")]
    flags += ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize \
        else ["-O2", "-ffp-contract=off"]
    tmp = out + ".tmp%d" % os.getpid()
    cmd = [cxx] + flags + srcs + ["-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("compiling the reference against oracle/ref_shim failed:\n" + r.stdout[-4000:])
    if not quiet and r.stdout.strip():
        print(r.stdout)
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    p = build(force="--force" in sys.argv, sanitize="--sanitize" in sys.argv, quiet=False)
    print(p if p else "reference tree or C++ compiler not found: nothing built")
